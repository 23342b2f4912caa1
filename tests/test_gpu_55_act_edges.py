"""GPU tests of the activation section of csrc/elementwise.hip at its edges, through the public entry points only (ops.act_fwd, ops.act_bwd,
ops.act_bwd_signs, ops.norm_add_fwd, ops.dropout_mask, batch-invariant mode): tfc_act_fwd_kernel, tfc_act_pool2_fwd_kernel, tfc_act_bwd_kernel,
tfc_act_pool2_bwd_kernel, tfc_blur1_kernel (forward and transpose), tfc_norm_add_kernel and, behind them, tfc_part_reduce_kernel.
Restatements, the launchers' routes, the case tables and the data live in tests/act_edges_ref.py and are checked on the CPU by
tests/test_act_edges_host.py, which also shows that the comparisons used here reject a list of one-line mutants.

  294 planes, H in 3..20, 31..33 x W in 3..8, 31..35, 63..65, one channel vector: every forward / backward route      test_geometry_cheap_width
  43 planes around the 8 / 16 / 32 tile edges and all of H, W <= 5 at 8 channel vectors: blur1 forward / transpose,
    with statistics, tiled pool-2 backward, and tfc_act_bwd_signs against tfc_act_bwd                               test_geometry_tiled_width
  every buffer a slice of one 2 C and 3 C wide, norm-add in place on x and on res                                    test_pitch_and_offset
  every legal C (bf16 8 .. 2048, fp32 4 .. 1024): cslice < 64, blockIdx.z > 1, PPB = 1, part-reduce at L = 4096      test_channel_widths
  act_grid's cap, plain (N = 64) and batch-invariant (N = 1, 2: image 0 bit-equal), second trip ragged             test_grid_cap_*
  dropout index at its five sites against ops.dropout_mask and O.hip_keep_mask, all-ones data                        test_dropout_index
  InstanceNorm forward, modes 1 and 2, norm-add, slope 0.2: bound tier                                               test_instance_norm_bound, test_slope02_bound
  refusals                                                                                                           test_refusals

Routes (act_edges_ref.ROUTES) by test: the generic kernels act_fwd / act_fwd<stats> / pool2_fwd<act|blur> / act_bwd<0,*> run in every exact test;
blur1_fwd, blur1_fwd<stats>, blur1_t, pool2_bwd<0> and pool2_bwd<signs> from the tiled width on (tiled geometry, pitch, widths >= 8 vectors);
pool2_bwd<1|2>, act_bwd<1|2,0|1> and norm_add in the InstanceNorm, pitch and grid-cap tests.

Two tiers. Exact: no normalisation, ternary inputs and gradients, slope 1, 1/4 or 0, dropout 0 or 1/2: every product and sum is exact in fp32 in
any order (asserted on the reference), and outputs, statistics and bias sums are torch.equal to the float64 restatement rounded once to the
storage type. Bound: per element |got - ref64| <= 8 e32 (+ 2^-8 |ref64| for a bf16 store), e32 = the largest error of the float32 numpy
restatement against float64 on the case's tensor, computed here; every ratio error / bound is printed with the prefix `act-edges:`
(profiles/act_edges.md holds one run's). The statistics a bound-tier forward returns are held, by the same rule, to the float64 sums of the
tensor the kernel itself stored (a reference tensor rounds to another bf16 neighbour on rare elements, which moves a sum by far more than e32).
Every output buffer starts as SENT and everything outside the written slice must still be SENT; inputs must come back unchanged.

Left out: tfc_act_pool2_fwd_kernel past the cap in plain mode (it strides over 2 x 2 output blocks: N C 16 nob > 16 x 4096 x 256 x ue input
elements, 268 MB; it is capped in batch-invariant mode, where the cap is 128 at any N). The generic backward with POOL == 2 and x, and modes
1 / 2 at POOL == 2 on the generic kernel, cannot be reached: every C fill_act accepts goes to the tiled kernel. Nothing else of the issue."""
import numpy as np
import pytest
import torch

from oracle import tfcgan_oracle as O
from tests import act_edges_ref as R
from tests import conv_exact as X
from tfc_gan_amd import _lib, ops
from tfc_gan_amd._lib import DT_BF16, DT_F32, check
from tfc_gan_amd.ops import View

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 7.0                                                        # exact in bf16; no exact-tier result reaches it
ALONE = (1, 0)                                                    # (pitch / C, channel offset / C)
IDS = {torch.float32: "fp32", torch.bfloat16: "bf16"}
dtypes = pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: IDS[d])


def dt_of(dtype):
    return DT_BF16 if dtype == torch.bfloat16 else DT_F32


def say(text):
    print("act-edges: " + text)


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def blank(N, H, W, C, dtype, form):
    mult, off = form
    return View(torch.full((N, H, W, mult * C), SENT, dtype=dtype, device=DEV), C, off * C)


def put(a, dtype, form):
    """NCHW numpy -> channels [off C, off C + C) of an NHWC buffer of pitch mult C whose other channels hold SENT"""
    N, C, H, W = a.shape
    v = blank(N, H, W, C, dtype, form)
    v.t[..., v.coff:v.coff + C] = dev(a, dtype).permute(0, 2, 3, 1)
    return v


def get(v):
    return v.t[..., v.coff:v.coff + v.C].permute(0, 3, 1, 2).contiguous().cpu()


def assert_guard(v, what):
    rest = torch.cat((v.t[..., :v.coff], v.t[..., v.coff + v.C:]), -1)
    assert torch.equal(rest, torch.full_like(rest, SENT)), f"{what}: channels outside the slice were written"


def tag(c, fx=ALONE, fo=ALONE):
    t = f"{c.kernel} {IDS[c.dtype]} N={c.N} C={c.C} {c.H}x{c.W} pool={c.pool} slope={c.slope} drop={c.drop}"
    t += "" if c.entry in ("fwd", "nadd") else f" x={int(c.use_x)} rstats={int(c.rstats)}"
    t += " inv" if c.inv else ""
    return t + ("" if (fx, fo) == (ALONE, ALONE) else f" forms={fx}{fo}")


def run_case(c, d, fx=ALONE, fo=ALONE, alias=None):
    """the case through its entry point; fx: the form of the buffers of the input plane (x, dx), fo: of the output plane (y, dy; res of a norm-add).
    Returns name -> CPU tensor (NCHW in the storage type; fp32 sums), after the guard checks."""
    dt, what = dt_of(c.dtype), tag(c, fx, fo)
    Ho, Wo = R.out_len(c.H, c.pool), R.out_len(c.W, c.pool)
    stats = dev(d["stats"]) if c.norm else None
    fother = ALONE if fx == ALONE else (5 - fx[0], 1)              # dx in a buffer of the other width than x
    out = {}
    if c.entry == "fwd":
        xv, yv = put(d["x"], c.dtype, fx), blank(c.N, Ho, Wo, c.C, c.dtype, fo)
        x0 = xv.t.clone()
        so = torch.full((c.N, c.C, 2), R.PREFILL, device=DEV) if c.stats_out else None
        ops.act_fwd(dt, xv, yv, stats=stats, slope=c.slope, pool=c.pool, drop_p=c.drop, seed=R.SEED, stats_out=so)
        out["y"] = get(yv)
        if so is not None:
            out["stats"] = so.cpu()
        assert_guard(yv, what)
        assert torch.equal(xv.t, x0), f"{what}: the input changed"
    elif c.entry == "nadd":
        xv, rv = put(d["x"], c.dtype, fx), put(d["res"], c.dtype, fo)
        yv = xv if alias == "x" else (rv if alias == "res" else blank(c.N, c.H, c.W, c.C, c.dtype, fother))
        x0, r0 = xv.t.clone(), rv.t.clone()
        ops.norm_add_fwd(dt, xv, rv, stats, yv)
        out["y"] = get(yv)
        for v in (xv, rv, yv):
            assert_guard(v, what)
        assert (alias == "x" or torch.equal(xv.t, x0)) and (alias == "res" or torch.equal(rv.t, r0)), f"{what}: an input changed"
    else:
        dyv = put(d["dy"], c.dtype, fo)
        dxv = blank(c.N, c.H, c.W, c.C, c.dtype, fother) if c.mode != 1 else None
        dy0 = dyv.t.clone()
        if c.mode == 0:
            rs = torch.full((c.N, c.C), R.PREFILL, device=DEV) if c.rstats else None
        else:
            rs = torch.zeros((c.N, c.C, 2), device=DEV) if c.mode == 1 else dev(d["rstats"])
        if c.entry == "signs":
            sm = X.sign_words(torch.from_numpy(d["x"])).to(DEV)
            ops.act_bwd_signs(dt, dyv, sm, c.N, c.H, c.W, c.C, dxv, slope=c.slope, rstats=rs)
        else:
            xv = put(d["x"], c.dtype, fx) if c.use_x else None
            ops.act_bwd(dt, c.mode, dyv, xv, c.N, c.H, c.W, c.C, dxv, stats=stats, slope=c.slope, pool=c.pool, drop_p=c.drop, seed=R.SEED, rstats=rs)
        if c.mode != 1:
            out["dx"] = get(dxv)
            assert_guard(dxv, what)
        if c.mode == 0 and c.rstats:
            out["bias"] = rs.cpu()
        if c.mode == 1:
            out["rstats"] = rs.cpu()
        if c.mode == 2:
            assert torch.equal(rs.cpu(), torch.from_numpy(d["rstats"])), f"{what}: mode 2 wrote rstats"
        assert torch.equal(dyv.t, dy0), f"{what}: the gradient changed"
    return out


def describe(got, want):
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)} for {tuple(want.shape)}"
    bad = (got.float() != want.float()) | torch.isnan(got.float())
    idx = bad.nonzero()
    first = [(tuple(i.tolist()), got[tuple(i)].item(), want[tuple(i)].item()) for i in idx[:6]]
    return f"{idx.shape[0]} of {got.numel()} differ; (index, got, want): {first}"


def check_case(c, got, d, what, worst=None):
    """exact tier: torch.equal to the reference rounded once. Bound tier: 8 e32 (+ 2^-8 |ref| for a bf16 store) per element, figures printed."""
    ref64 = R.case_reference(c, d)
    if R.is_exact(c):
        want = R.exact_want(c, ref64)
        assert set(got) == set(want), (what, sorted(got), sorted(want))
        for k in want:
            assert R.same_bits(got[k], want[k]), f"{what} [{k}]: {describe(got[k], want[k])}"
        return
    ref32 = R.case_reference(c, d, R.F32)
    figs = []
    for k in ref64:
        bf = R.is_tensor(k) and c.dtype == torch.bfloat16
        e32 = R.e32_of(ref32[k], ref64[k])
        ratio = R.bound_ratio(got[k].double().numpy(), ref64[k], e32, bf)
        figs.append((k, e32, ratio))
    if "stats" in got:                                             # the sums of the tensor the kernel stored
        y = got["y"].double().numpy()
        s64, s32 = R.stored_stats(y, R.F64) + R.PREFILL, R.stored_stats(y, R.F32) + R.F32(R.PREFILL)
        e32 = R.e32_of(s32, s64)
        figs.append(("stats", e32, R.bound_ratio(got["stats"].double().numpy(), s64, e32, False)))
    say(what + ": " + ", ".join(f"{k} e32={e:.3e} error/bound={r:.3f}" for k, e, r in figs))
    for k, e, r in figs:
        if worst is not None:
            worst[0] = max(worst[0], r)
        assert r <= 1.0, f"{what} [{k}]: error / bound = {r:.3f} (e32 = {e:.3e})"


def run_and_check(cases, fx=ALONE, fo=ALONE, worst=None):
    for c in cases:
        d = R.inputs_of(c)
        check_case(c, run_case(c, d, fx, fo), d, tag(c, fx, fo), worst)


# ---- 1. geometry ---------------------------------------------------------------------------------------------------------------------------------
GEO_CHUNKS = (R.GEO_H[:6], R.GEO_H[6:12], R.GEO_H[12:18], R.GEO_H[18:])


@dtypes
@pytest.mark.parametrize("rows", GEO_CHUNKS, ids=lambda r: f"H{r[0]}-{r[-1]}")
def test_geometry_cheap_width(rows, dtype):
    """Every (H, W) of the sweep at one channel vector (C = 8 bf16, 4 fp32), N = 2, exact tier. Per plane: act_fwd at pool 2 without statistics
    (tfc_act_pool2_fwd_kernel, ACT off at slope 1 and on at 1/4) and with (tfc_act_fwd_kernel<stats>) -- both equal the one reference, hence each
    other --, at pool 1 and 0 alike; act_bwd mode 0 at pools 0, 1, 2 with x (pool 2: the tiled kernel at cslice = C) and without (generic POOL == 2
    and POOL == 1), with and without the bias sums. H or W of 3, 4, 5 put two or three reflect aliases on one row or column."""
    cases = [c for c in R.geometry_cases(dtype, False) if c.H in rows]
    assert len(cases) == len(rows) * len(R.GEO_W) * 24
    run_and_check(cases)


@dtypes
def test_geometry_tiled_width(dtype):
    """The thinned sweep at 8 channel vectors (C = 64 bf16, 32 fp32), the narrowest blur1_launch takes: tfc_blur1_kernel forward with and without
    statistics and transposed at planes that straddle its 8 x 32 tile in one dimension only, declined at H or W = 3 (generic kernel, same bits
    asked); tfc_act_pool2_bwd_kernel across its 16 x 32 tile; in bf16 tfc_act_bwd_signs with sign words built from x against the reference of
    tfc_act_bwd with x itself (which runs on the same data in the same loop), with and without the bias sums."""
    cases = R.geometry_cases(dtype, True)
    kernels = {c.kernel for c in cases}
    assert {"blur1_fwd", "blur1_fwd<stats>", "blur1_t", "pool2_bwd<0>", "act_fwd", "act_bwd<0,1>"} <= kernels
    assert ("pool2_bwd<signs>" in kernels) == (dtype == torch.bfloat16)
    assert any(c.kernel == "act_fwd<stats>" and c.pool == 1 and c.slope == 1.0 and 3 in (c.H, c.W) for c in cases)      # blur1 declined
    run_and_check(cases)


# ---- 2. pitch and channel offset -----------------------------------------------------------------------------------------------------------------
@dtypes
def test_pitch_and_offset(dtype):
    """5 x 7 and 17 x 33: x, y / dy, dx and res each the upper half of a 2 C wide buffer or the last third of a 3 C wide one (in both
    assignments; dx always in the other width than x), the rest of every buffer SENT before and after. Every exact route at one and at eight
    channel vectors, and tfc_act_bwd_signs in bf16; the InstanceNorm routes (forward, modes 1 and 2 tiled and generic, norm-add) at 17 x 33 and eight vectors in the bound tier;
    norm-add also with y aliasing x and y aliasing res."""
    worst = [0.0]
    for fx, fo in (((2, 1), (3, 2)), ((3, 2), (2, 1))):
        for C in (R.cheap_c(dtype), R.tiled_c(dtype)):
            run_and_check(R.width_cases(dtype, (C,)), fx, fo)
        run_and_check(R.signs_cases(dtype, R.PITCH_SHAPES, "pitch"), fx, fo)
        normed = [c for c in R.norm_cases(dtype) if (c.H, c.W) == (17, 33) and c.C == R.tiled_c(dtype)]
        assert {c.kernel for c in normed} >= {"pool2_bwd<1>", "pool2_bwd<2>", "act_bwd<1,0>", "act_bwd<2,1>", "norm_add", "pool2_fwd<act>", "act_fwd<stats>"}
        run_and_check(normed, fx, fo, worst)
        for c in normed:
            if c.entry == "nadd":
                for alias in ("x", "res"):
                    d = R.inputs_of(c)
                    check_case(c, run_case(c, d, fx, fo, alias), d, tag(c, fx, fo) + f" y={alias}", worst)
    say(f"pitch {IDS[dtype]}: largest error / bound {worst[0]:.3f}")


# ---- 3. channel widths ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(9))
@dtypes
def test_channel_widths(dtype, k):
    """Every C fill_act accepts (ue x 2^k), 5 x 7 and 17 x 33, every exact route: the tiled pool-2 backward at cslice = C < 64 (fp32 C = 4: one
    channel vector, 256 pixel lanes) and at blockIdx.z > 1 from C = 128, the generic kernels down to one pixel per workgroup, and
    tfc_part_reduce_kernel at L = 2 C up to 4096"""
    C = R.legal_widths(dtype)[k]
    cases = R.width_cases(dtype, (C,))
    r = R.route("bwd", dtype, 2, 17, 33, C, pool=2)
    assert r.grid[2] == max(C // 64, 1)
    run_and_check(cases)


# ---- 4. grid cap ---------------------------------------------------------------------------------------------------------------------------------
@dtypes
def test_grid_cap_plain(dtype):
    """N = 64: cap 4096 / 64 = 64 workgroups per image, at the widest C whose partial sums fit the scratch (one or two pixels per workgroup),
    and the smallest plane with more pixels than the grid covers whose second trip is ragged (picked by the route function, asserted there and
    here). tfc_act_fwd_kernel with and without statistics and tfc_act_bwd_kernel mode 0 with bias sums in the exact tier; mode 1 and
    tfc_norm_add_kernel in the bound tier. In bf16 at C = 2048 the 64 x 64 slots of 2 C statistics pass the scratch: the entry point refuses
    and writes nothing."""
    cases = R.cap_cases(dtype, False, 64)
    assert [c.kernel for c in cases] == ["act_fwd<stats>", "act_fwd", "act_bwd<0,0>", "act_bwd<1,0>", "norm_add"]
    for c in cases:
        r = R.route_of(c)
        assert r.grid[0] == R.act_grid_cap(c.N, False) == 64 and r.trips == 2 and r.ragged and R.case_bytes(c) < 64 << 20
    run_and_check(cases)
    if dtype == torch.bfloat16:
        assert R.route("fwd", dtype, 64, 5, 13, 2048, slope=0.25, stats_out=True).kernel == R.REFUSED
        xv, yv = blank(64, 5, 13, 2048, dtype, ALONE), blank(64, 5, 13, 2048, dtype, ALONE)
        so = torch.full((64, 2048, 2), R.PREFILL, device=DEV)
        with pytest.raises(_lib.TfcError):
            ops.act_fwd(DT_BF16, xv, yv, slope=0.25, stats_out=so)
        assert (yv.t == SENT).all() and (so == R.PREFILL).all()


@dtypes
def test_grid_cap_batch_invariant(dtype):
    """Batch-invariant mode: the cap is 4096 / 32 = 128 whatever N is. The same six kernels (tfc_act_pool2_fwd_kernel included) at N = 2 and at
    N = 1 on image 0 of the same data: each against its reference, and image 0 bit-equal between the two."""
    two, one = R.cap_cases(dtype, True, 2), R.cap_cases(dtype, True, 1)
    assert [c.kernel for c in two] == ["act_fwd<stats>", "act_fwd", "pool2_fwd<act>", "act_bwd<0,0>", "act_bwd<1,0>", "norm_add"]
    prev = _lib.get_batch_invariant()
    try:
        _lib.set_batch_invariant(True)
        for c2, c1 in zip(two, one):
            assert c1 == c2._replace(N=1)
            for c in (c1, c2):
                r = R.route_of(c)
                assert r.grid[0] == 128 and r.trips == 2 and r.ragged
            assert R.route_of(c2._replace(inv=False)).trips == 1   # outside the mode this shape is not capped
            d2 = R.inputs_of(c2)
            d1 = {k: (v[:1] if isinstance(v, np.ndarray) else v) for k, v in d2.items()}
            g2, g1 = run_case(c2, d2), run_case(c1, d1)
            check_case(c2, g2, d2, tag(c2))
            check_case(c1, g1, d1, tag(c1))
            for k in g2:
                assert torch.equal(g1[k][0], g2[k][0]), f"{tag(c2)} [{k}]: image 0 differs between N = 1 and N = 2"
    finally:
        _lib.set_batch_invariant(prev)


# ---- 5. dropout index ----------------------------------------------------------------------------------------------------------------------------
@dtypes
def test_dropout_index(dtype):
    """drop_p = 1/2 on all-ones x and all-ones gradients, 5 x 7 and 17 x 33, pitched and sliced, at one channel vector, eight, and C = 128 (two
    slices of the tiled backward). ops.dropout_mask equals O.hip_keep_mask at index (n Ho Wo + opix) C + c; the forward's kept set (y = 2 keep:
    a blur of ones is one) equals it at the generic forward (pools 0, 1; pool 2 with statistics) and at the store lambda of the pooled forward;
    what the backward lets through equals it at POOL == 0 (dx = 2 keep), and at the tap lambda of the generic backward (pools 1, 2 without x) and
    the window staging of the tiled one (pool 2 with x) against the reference. Then the same routes on ternary data."""
    fx, fo = (2, 1), (3, 2)
    for C in R.drop_widths(dtype):
        for H, W in R.PITCH_SHAPES:
            cases = R.exact_routes(dtype, 2, H, W, C, 0.5)
            assert {c.kernel for c in cases} >= {"act_fwd", "act_fwd<stats>", "pool2_fwd<act>", "pool2_fwd<blur>", "act_bwd<0,0>", "act_bwd<0,1>", "act_bwd<0,2>",
                                                 "pool2_bwd<0>"}
            for c in cases:
                Ho, Wo = R.out_len(H, c.pool), R.out_len(W, c.pool)
                n = 2 * Ho * Wo * C
                flat = O.hip_keep_mask(R.SEED, n, 0.5)
                assert np.array_equal(ops.dropout_mask(n, 0.5, R.SEED, DEV).cpu().numpy().astype(bool), flat)
                keep = np.ascontiguousarray(flat.reshape(2, Ho, Wo, C).transpose(0, 3, 1, 2))
                assert np.array_equal(keep, R.keep_mask(R.SEED, 2, Ho, Wo, C, 0.5))
                d = {"x": np.ones((2, C, H, W)), "dy": np.ones((2, C, Ho, Wo)), "stats": None, "keep": keep}
                got = run_case(c, d, fx, fo)
                check_case(c, got, d, tag(c, fx, fo) + " ones")
                if c.entry == "fwd" or c.pool == 0:
                    k = "y" if c.entry == "fwd" else "dx"
                    assert torch.equal(got[k], R.store(2.0 * keep, dtype)), f"{tag(c)}: the kept set is not the mask"
    run_and_check(R.dropout_cases(dtype), fx, fo)


# ---- 6. InstanceNorm and slope 0.2: bound tier ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(3))
@dtypes
def test_instance_norm_bound(dtype, k):
    """(pool, slope, drop) in (2, 0.2, 0), (2, 0.2, 0.5), (0, 0, 0.5), (0, 0.2, 0), (1, 0.2, 0) x 3 x 3, 4 x 5, 7 x 7, 17 x 33 at C = 8 / 64 / 512
    (fp32: 4 / 32 / 256): forward with and without statistics, mode 1 (both sums against float64), mode 2 (generic at pools 0 and 1, tiled at
    pool 2; against the float64 gradient at mode 1's float64 sums rounded to the fp32 the kernel reads), norm-add. Statistics in: the sums of the
    stored x. Plane (0, 0) of every case is all zero: mean and xhat exactly 0, rstd = rsqrt(eps), act' = slope. |xhat| >= 0.1 elsewhere
    (asserted on the CPU): nothing is masked."""
    C = R.norm_widths(dtype)[k]
    cases = [c for c in R.norm_cases(dtype) if c.C == C]
    assert len(cases) == 4 * (5 * 4 + 1)
    worst = [0.0]
    run_and_check(cases, worst=worst)
    say(f"instance norm {IDS[dtype]} C={C}: largest error / bound {worst[0]:.3f}")


@dtypes
def test_slope02_bound(dtype):
    """slope 0.2 without normalisation (9/64 x 0.2f rounds, so no exact tier): the three forward kernels with and without statistics and mode 0
    with bias sums on both backward families, 5 x 7 and 17 x 33"""
    worst = [0.0]
    run_and_check(R.slope02_cases(dtype), worst=worst)
    say(f"slope 0.2 {IDS[dtype]}: largest error / bound {worst[0]:.3f}")


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """Bad arguments return non-zero with the cause in tfc_last_error() and write nothing: every buffer keeps its fill after a synchronize. Every
    other argument of each call is valid for buffers of 4096 elements. (N, H, W, C = 0: test_gpu_51_stream_edges.)"""
    lib = ops.lib()
    f32 = [torch.full((4096,), SENT, device=DEV) for _ in range(5)]
    b16 = [torch.full((4096,), SENT, dtype=torch.bfloat16, device=DEV) for _ in range(3)]
    u8 = torch.full((4096,), 7, dtype=torch.uint8, device=DEV)
    a, b, c, st_, rs = (t.data_ptr() for t in f32)
    h, k, m = (t.data_ptr() for t in b16)
    sm = u8.data_ptr()
    ws = ops.part_ws(torch.device(DEV))
    s = ops.stream_ptr()
    F, B = DT_F32, DT_BF16

    def fwd(dt, x, xp, C, y, yp, H=4, stats=None, norm=0, pool=0, drop=0.0, so=None, pw=None):
        return lambda: lib.tfc_act_fwd(s, dt, x, xp, 1, H, 4, C, stats, norm, 0.2, pool, drop, 1, y, yp, so, pw)

    def bwd(dt, mode, dy, x, dx, C=8, dxp=8, stats=None, norm=0, r=None, pw=None, pool=0):
        return lambda: lib.tfc_act_bwd(s, dt, mode, dy, C, x, C, 1, 4, 4, C, stats, norm, 0.2, pool, 0.0, 1, r, dx, dxp, pw)

    cases = [
        (b"C/8 = 3 must divide 256", fwd(B, h, 24, 24, k, 24)),
        (b"C=4 must be a multiple of 8", fwd(B, h, 8, 4, k, 8)),
        (b"C/4 = 3 must divide 256", fwd(F, a, 12, 12, b, 12)),
        (b"reflect pad needs H,W >= 3", fwd(F, a, 8, 8, b, 8, H=2, pool=1)),
        (b"reflect pad needs H,W >= 3", fwd(B, h, 8, 8, k, 8, H=2, pool=2)),
        (b"reflect pad needs H,W >= 3", lambda: lib.tfc_act_bwd(s, F, 0, a, 8, None, 0, 1, 2, 4, 8, None, 0, 1.0, 2, 0.0, 1, None, b, 8, None)),
        (b"pitches must be multiples of 8", fwd(B, h, 12, 8, k, 8)),
        (b"pitches must be multiples of 8", fwd(B, h, 8, 8, k, 12)),
        (b"pitches must be multiples of 4", fwd(F, a, 10, 8, b, 8)),
        (b"pitches must be multiples of 4", lambda: lib.tfc_act_bwd(s, F, 0, a, 10, None, 0, 1, 4, 4, 8, None, 0, 1.0, 0, 0.0, 1, None, b, 8, None)),
        (b"dx pitch 10 must be a multiple of 4", bwd(F, 0, a, None, b, dxp=10)),
        (b"dx pitch 12 must be a multiple of 8", bwd(B, 0, h, None, k, dxp=12)),
        (b"dx pitch 68 must be a multiple of 8", lambda: lib.tfc_act_bwd_signs(s, B, h, 64, sm, 1, 4, 4, 64, 0.2, None, k, 68, None)),
        (b"drop_p out of range", fwd(F, a, 8, 8, b, 8, drop=1.0)),
        (b"drop_p out of range", fwd(F, a, 8, 8, b, 8, drop=-0.5)),
        (b"stats is null", fwd(F, a, 8, 8, b, 8, norm=1)),
        (b"stats_out needs part_ws", fwd(F, a, 8, 8, b, 8, so=st_)),
        (b"modes 1/2 need norm and rstats", bwd(F, 1, a, b, None, r=rs, pw=ws)),
        (b"modes 1/2 need norm and rstats", bwd(F, 2, a, b, c, r=rs)),
        (b"modes 1/2 need norm and rstats", bwd(F, 1, a, b, None, stats=st_, norm=1, pw=ws)),
        (b"modes 1/2 need norm and rstats", bwd(F, 2, a, b, c, stats=st_, norm=1)),
        (b"norm needs stats and x", bwd(F, 1, a, b, None, norm=1, r=rs, pw=ws)),
        (b"norm needs stats and x", bwd(F, 2, a, None, c, stats=st_, norm=1, r=rs)),
        (b"a reduction into rstats needs part_ws", bwd(F, 0, a, None, c, r=rs)),
        (b"a reduction into rstats needs part_ws", bwd(F, 1, a, b, None, stats=st_, norm=1, r=rs)),
        (b"dx is null", bwd(F, 0, a, None, None)),
        (b"dx is null", bwd(F, 2, a, b, None, stats=st_, norm=1, r=rs)),
        (b"tfc_act_bwd_signs: bf16, 64 channels", lambda: lib.tfc_act_bwd_signs(s, B, h, 128, sm, 1, 4, 4, 128, 0.2, None, k, 128, None)),
        (b"tfc_act_bwd_signs: bf16, 64 channels", lambda: lib.tfc_act_bwd_signs(s, B, h, 8, sm, 1, 4, 4, 8, 0.2, None, k, 8, None)),
        (b"tfc_act_bwd_signs: bf16, 64 channels", lambda: lib.tfc_act_bwd_signs(s, F, a, 64, sm, 1, 4, 4, 64, 0.2, None, b, 64, None)),
        (b"a reduction into rstats needs part_ws", lambda: lib.tfc_act_bwd_signs(s, B, h, 64, sm, 1, 4, 4, 64, 0.2, rs, k, 64, None)),
        (b"must be >= C=16", lambda: lib.tfc_norm_add_fwd(s, F, a, 8, b, 16, 1, 4, 4, 16, st_, c, 16)),
        (b"must be >= C=16", lambda: lib.tfc_norm_add_fwd(s, F, a, 16, b, 8, 1, 4, 4, 16, st_, c, 16)),
        (b"must be >= C=16", lambda: lib.tfc_norm_add_fwd(s, B, h, 16, k, 16, 1, 4, 4, 16, st_, m, 8)),
        (b"must be >= C=8", lambda: lib.tfc_norm_add_fwd(s, F, a, 8, b, 10, 1, 4, 4, 8, st_, c, 8)),
        (b"stats is null", lambda: lib.tfc_norm_add_fwd(s, F, a, 8, b, 8, 1, 4, 4, 8, None, c, 8)),
    ]
    for i, (text, call) in enumerate(cases):
        assert call() != 0, f"case {i} was not refused"
        msg = lib.tfc_last_error()
        assert msg and text in msg, (i, text, msg)
    check(fwd(F, a, 8, 8, b, 8, pool=1)(), "tfc_act_fwd")          # the checks let a good call through: a blur of a constant is the constant
    torch.cuda.synchronize()
    for t in f32 + b16:
        assert (t == SENT).all()
    assert (u8 == 7).all()
