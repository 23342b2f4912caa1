"""GPU tests of the small streaming kernels past their grid caps: csrc/elementwise.hip below the activation section and the scalar heads of
csrc/losses.hip, through their public entry points only. Restatements, data and the caps (read from the launchers) live in
tests/stream_edges_ref.py and are checked on the CPU by tests/test_stream_edges_host.py.

  cast, axpby, dropout mask, Adam at 1 .. 2 x 4096 x 256 + 3 elements (third, ragged trip)       test_cast_*, test_axpby_*, test_dropout_*, test_adam_*
  column sums on both routes (one workgroup row; row split + tfc_part_reduce_kernel at 4, 5, 6, 9 slots)     test_colsum_exact
  tanh backward + bias sum at C = 1, 3, 4, past 1024 workgroups (tfc_part_reduce_strided_kernel)            test_tanh_bwd_pack_exact
  L1 sum through tfc_block_commit past 512 workgroups, and its slot across grids of 1, 512, 1 workgroups     test_l1_sum_*
  relativistic BCE past 256 workgroups, both store paths, both modes                                        test_bce_*
  spectral-norm backward past the 128 dot partials, accumulate on and off                                   test_spectral_norm_bwd
  PatchGAN head forward on both weight paths in both dtypes, past 512 workgroups                            test_patchgan_head_exact
  refusals of all of them, fill_act's C = 0 included                                                         test_refusals

Integer data wherever the arithmetic allows (torch.equal, no tolerance). Every other bound is a derived form (stated at the test) or 8 x the
error of the same expression in fp32 on the CPU against fp64, computed and printed here; every figure of a run is printed with the prefix
`stream-edges:` (profiles/stream_edges.md holds one run's).

Which weight path of tfc_head_fwd_kernel the older tests reach (the filter is in LDS when C / ue > 64): test_patchgan_head_kernel_matches_padconv
runs C = 512 in both dtypes, i.e. LDS in fp32 (128 units) and registers in bf16 (64 units); test_exact_patchgan_head_fwd is bf16 at C = 512:
registers. Registers in fp32 and LDS in bf16 ran nowhere; test_patchgan_head_exact runs all four (HEAD_CASES).

Left out: the ny cap of tfc_launch_colsum (2048 / nbx slots: rows > 2 097 152 / nbx with 1024 rows per slot, more than 250 MB of input at any C of
the step). Nothing else of the issue's list is absent."""
import numpy as np
import pytest
import torch

from oracle import tfcgan_oracle as O
from tests import conv_exact as X
from tests import stream_edges_ref as R
from tfc_gan_amd import ops
from tfc_gan_amd._lib import DT_BF16, DT_F32, check
from tfc_gan_amd.ops import View

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 7.0                                                        # fills whatever a kernel must not write; exact in bf16
DTYPES = [torch.float32, torch.bfloat16]


def dt_of(dtype):
    return DT_BF16 if dtype == torch.bfloat16 else DT_F32


def P(t, off=0):
    """device address of element `off` of t"""
    return None if t is None else t.data_ptr() + off * t.element_size()


def st():
    return ops.stream_ptr()


def guarded(t, dtype=None):
    """t (1-d, CPU) on the GPU with one SENT element behind it"""
    t = t if dtype is None else t.to(dtype)
    return torch.cat((t, torch.full((1,), SENT, dtype=t.dtype))).to(DEV)


def say(text):
    print("stream-edges: " + text)


# ---- 1. flat buffers: cap 4096 x 256 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.FLAT_SIZES)
def test_cast_bits(n):
    """fp32 -> bf16 equals x.to(torch.bfloat16) bit for bit on ties in both directions, +-0, +-inf, overflow to inf and denormals (a NaN is a
    NaN); bf16 -> fp32 is the 16-bit shift for all 65 536 patterns; in TFC_DT_F32 both directions copy the bits; the element behind n stays"""
    lib = ops.lib()
    x = R.cast_f32_data(n)
    xd = x.to(DEV)
    y = torch.full((n + 1,), SENT, dtype=torch.bfloat16, device=DEV)
    check(lib.tfc_cast(st(), DT_BF16, 0, P(xd), P(y), n), "tfc_cast")
    got = y.cpu()
    want = x.to(torch.bfloat16)
    bad = (R.bits16(got[:n]) != R.bits16(want)) & ~(torch.isnan(got[:n]) & torch.isnan(want))
    assert R.same_floats(got[:n], want), (int(bad.sum()), [hex(v) for v in R.bits32(x[bad][:8]).tolist()])
    assert got[n].item() == SENT
    b = R.cast_bf16_data(n)
    z = torch.full((n + 1,), SENT, device=DEV)
    check(lib.tfc_cast(st(), DT_BF16, 1, P(b.to(DEV)), P(z), n), "tfc_cast")
    got = z.cpu()
    assert torch.equal(R.bits32(got[:n]), R.bits16(b) << 16) and got[n].item() == SENT
    for to_f32 in (0, 1):
        z = torch.full((n + 1,), SENT, device=DEV)
        check(lib.tfc_cast(st(), DT_F32, to_f32, P(xd), P(z), n), "tfc_cast")
        got = z.cpu()
        assert torch.equal(R.bits32(got[:n]), R.bits32(x)) and got[n].item() == SENT


@pytest.mark.parametrize("n", R.FLAT_SIZES)
def test_axpby_bound_and_exact(n):
    """out = a x + b y against fp64 within 2^-23 (|a x| + |b y|) per element (two roundings at most, contracted or not), with y given and y = None,
    out of place and in place (out is x); with power-of-two coefficients on integer data torch.equal. The element behind n stays."""
    lib = ops.lib()
    worst = 0.0
    for exact, coeffs in ((False, R.AXPBY_AB), (True, R.AXPBY_AB_EXACT)):
        x, y = R.axpby_data(n, exact=exact)
        yd = y.to(DEV)
        for a, b in coeffs:
            for yy in (y, None):
                ref, bound = R.axpby_ref(x, yy, a, b)
                for inplace in (False, True):
                    xd = guarded(x)
                    out = xd if inplace else torch.full((n + 1,), SENT, device=DEV)
                    check(lib.tfc_axpby(st(), P(out), P(xd), None if yy is None else P(yd), n, a, b), "tfc_axpby")
                    got = out.cpu()
                    assert got[n].item() == SENT, (a, b, inplace)
                    err = (got[:n].double() - ref).abs()
                    if exact:
                        assert torch.equal(got[:n].double(), ref), (a, b, yy is None, inplace, int((err != 0).sum()))
                    else:
                        assert (err <= bound).all(), (a, b, yy is None, inplace, (err / bound).max().item())
                        worst = max(worst, (err / bound.clamp_min(1e-300)).max().item())
    say(f"axpby n={n}: largest error {worst:.3f} of the bound 2^-23 (|a x| + |b y|)")


@pytest.mark.parametrize("seed", R.DROP_SEEDS)
def test_dropout_mask_equals_host_hash(seed):
    """tfc_dropout_mask equals O.hip_keep_mask(seed, n, p) at every flat size (a mask of n is the first n of the longest: the index is the hash's
    only input, held on the host) for p = 0, 2^-24, 0.5, 1 - 2^-24; p = 0 keeps everything; the byte behind n stays"""
    lib = ops.lib()
    for p in R.DROP_P:
        want = torch.from_numpy(O.hip_keep_mask(seed, R.FLAT_SIZES[-1], p)).to(torch.uint8)
        for n in R.FLAT_SIZES:
            out = torch.full((n + 1,), 7, dtype=torch.uint8, device=DEV)
            check(lib.tfc_dropout_mask(st(), P(out), n, p, seed), "tfc_dropout_mask")
            got = out.cpu()
            assert torch.equal(got[:n], want[:n]), (p, n, int((got[:n] != want[:n]).sum()))
            assert got[n].item() == 7 and (p != 0.0 or bool(got[:n].all()))


_ADAM_C = {}


def adam_c(step, gscale):
    """c of the p bound for (step, gscale), measured once on the whole draw (stream_edges_ref.adam_c) and shared by every size"""
    if (step, gscale) not in _ADAM_C:
        full = R.adam_state(R.FLAT_SIZES[-1])
        _ADAM_C[step, gscale] = R.adam_c(R.adam_ref(*full, step, gscale, **R.ADAM_HP), R.adam_f32(*full, step, gscale, **R.ADAM_HP))
    return _ADAM_C[step, gscale]


@pytest.mark.parametrize("n", R.FLAT_SIZES)
def test_adam_one_step_from_a_state(n):
    """One tfc_adam_step from a given (p, m, v, g) -- blocks with g = 0 and with v = g = 0 (denominator = eps) included -- at steps 1, 2, 1000 and
    gscale 1, 0.5 against fp64 Adam with the hyper-parameters as floats and 1 - b^step in fp64:
      m, v within 2^-22 (|b x| + |(1 - b) y|);  p within 2^-24 |p_new| + c |delta|, c = 8 x the largest relative error of a plain fp32 numpy
      restatement of the update on the whole draw (printed; the fp32 bias correction alone gives 3.3e-6 at step 2).
    Past the cap, p, m and v of the second and third trip differ from their inputs: a loop that stops after one trip fails here by name."""
    lib = ops.lib()
    hp = R.ADAM_HP
    state = R.adam_state(n)
    for step in R.ADAM_STEPS:
        for gscale in R.ADAM_GSCALES:
            c = adam_c(step, gscale)
            ref = R.adam_ref(*state, step, gscale, **hp)
            p, m, v, g = (guarded(torch.from_numpy(t)) for t in state)
            check(lib.tfc_adam_step(st(), P(p), P(g), P(m), P(v), n, hp["lr"], hp["b1"], hp["b2"], hp["eps"], step, gscale), "tfc_adam_step")
            got = {k: t.cpu().numpy() for k, t in (("p", p), ("m", m), ("v", v), ("g", g))}
            assert all(got[k][n] == SENT for k in got) and np.array_equal(got["g"][:n], state[3])
            bounds = {"p": R.adam_p_bound(ref, c), "m": ref["m_bound"], "v": ref["v_bound"]}
            frac = {}
            for k in ("p", "m", "v"):
                err = np.abs(got[k][:n].astype(np.float64) - ref[k])
                frac[k] = float(np.max(err / np.maximum(bounds[k], 1e-300)))
                assert (err <= bounds[k]).all(), (k, step, gscale, frac[k], int(np.argmax(err / np.maximum(bounds[k], 1e-300))))
            say(f"adam n={n} step={step} gscale={gscale}: c={c:.3e}; largest error / bound: p {frac['p']:.3f}, m {frac['m']:.3f}, v {frac['v']:.3f}")
            for trip, lo in ((2, R.FLAT_CAP), (3, 2 * R.FLAT_CAP)):
                hi = min(n, lo + R.FLAT_CAP)
                for k, old in (("p", state[0]), ("m", state[1]), ("v", state[2])):
                    if hi > lo:
                        changed = got[k][lo:hi] != old[lo:hi]
                        assert changed.mean() > 0.999 and (hi - lo > 3 or changed.all()), f"{k}: trip {trip} of n={n} left its input in place"


# ---- 2. bias sums and the fixed-order reductions: exact integers -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def colsum_data():
    return R.ternary((max(R.COLSUM_ROWS_SPLIT), 512), 61)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route", ["one", "split"])
def test_colsum_exact(route, dtype, colsum_data):
    """tfc_colsum through the entry point, part_ws given or not to choose the route: out += column sums of ternary data, torch.equal to the fp64
    sum. One workgroup row at 1, 31, 32, 33, 4095 (and 8225) rows; the row split at 4096, 4097, 5121, 8225 rows = 4, 5, 6, 9 slots through
    tfc_part_reduce_kernel's 8 part-lanes. C / ue = 1, 3, 9 and 64 (fp32: 128): at 3 and 9 the `cv < CV` guard idles lanes. Alone (pitch C) and as
    channels [8, 8 + C) of a buffer of pitch C + 16 whose other channels hold 2^20. out starts as a non-zero integer vector."""
    lib = ops.lib()
    split = route == "split"
    ws = ops.part_ws(torch.device(DEV)) if split else None
    rows_list = R.COLSUM_ROWS_SPLIT if split else R.COLSUM_ROWS_ONE + (max(R.COLSUM_ROWS_SPLIT),)
    for rows in rows_list:
        for C in R.COLSUM_C[dtype]:
            ny = R.colsum_ny(rows, C, dtype, lib.tfc_part_ws_floats(), with_part=split)
            assert (ny in (4, 5, 6, 9)) if split else ny == 1
            want = (R.colsum_prefill(C).double() + colsum_data[:rows, :C].sum(0)).float()
            for wide in (False, True):
                buf, coff, pitch = R.colsum_buffer(colsum_data, rows, C, dtype, wide)
                bd = buf.to(DEV)
                out = guarded(R.colsum_prefill(C))
                check(lib.tfc_colsum(st(), dt_of(dtype), P(bd, coff), rows, pitch, C, P(out), ws), "tfc_colsum")
                got = out.cpu()
                bad = (got[:C] != want).nonzero().flatten()
                assert torch.equal(got[:C], want), (rows, C, wide, ny, len(bad), bad[:6].tolist())
                assert got[C].item() == SENT


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", R.TANH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tanh_bwd_pack_exact(shape, dtype):
    """tfc_tanh_bwd_pack at C = 1, 3, 4: g (1 - y^2) is an integer by construction, so channels 0..C-1, the zeroed channels C..7 and
    dbias += sum are all exact. (1, 512, 513) is 262 656 pixels: 1024 slots for tfc_part_reduce_strided_kernel's 32 part-lanes and a second trip
    for 512 of the threads. dbias entries C..3 and the one behind keep their values; dbias = None writes the same tensor."""
    lib = ops.lib()
    N, H, W = shape
    ws = ops.part_ws(torch.device(DEV))
    pre = torch.tensor([3.0, -2.0, 7.0, 1.0])
    for C in (1, 3, 4):
        g, y, want = R.tanh_case(N, C, H, W, 70 + C)
        gd, yd = g.to(DEV), y.to(DEV)
        want_px = torch.zeros((N, H, W, 8), dtype=torch.float64)
        want_px[..., :C] = want.permute(0, 2, 3, 1)
        want_db = pre.clone()
        want_db[:C] = (pre[:C].double() + want.sum((0, 2, 3))).float()
        for with_bias in (True, False):
            out = torch.full((N, H, W, 8), SENT, dtype=dtype, device=DEV)
            db = guarded(pre) if with_bias else None
            check(lib.tfc_tanh_bwd_pack(st(), dt_of(dtype), P(gd), P(yd), P(out), P(db), N, C, H, W, ws if with_bias else None), "tfc_tanh_bwd_pack")
            assert torch.equal(out.cpu().double(), want_px), (C, with_bias)
            if with_bias:
                got = db.cpu()
                assert torch.equal(got[:4], want_db) and got[4].item() == SENT, (C, got.tolist(), want_db.tolist())


def test_l1_sum_exact_past_the_cap():
    """tfc_l1_sum on ternary data with power-of-two scales: the total is an integer multiple of the scale below 2^24, exact whatever order the double
    atomics of tfc_block_commit arrive in. n = 1, 255, 512 x 256, + 1, 3 x 512 x 256 + 37; zero_first, and accumulation onto a pre-set out"""
    for n in R.L1_SIZES:
        a, b, tot = R.l1_case(n)
        ad, bd = a.to(DEV), b.to(DEV)
        for scale in (0.25, 4.0):
            out = torch.full((2,), SENT, device=DEV)
            ops.l1_sum(ad, bd, scale, out, zero_first=True)
            assert out.cpu().tolist() == [tot.item() * scale, SENT], (n, scale)
            out = torch.tensor([1000.0, SENT], device=DEV)
            ops.l1_sum(ad, bd, scale, out)
            ops.l1_sum(ad, bd, scale, out)
            assert out.cpu().tolist() == [1000.0 + 2 * tot.item() * scale, SENT], (n, scale)


def test_l1_sum_slot_is_rearmed_between_grids():
    """small n, the largest n, small n again on one stream without a synchronize in between: grids of 1, 512 and 1 workgroups share g_l1_slot. A
    ticket or an accumulator that the last arriver does not re-arm makes the second or third result wrong; all three are exact."""
    cases = [R.l1_case(n, seed) for n, seed in ((255, 35), (R.L1_SIZES[-1], 31), (1, 37), (257, 39))]
    dev = [(a.to(DEV), b.to(DEV)) for a, b, _ in cases]
    outs = [torch.full((1,), SENT, device=DEV) for _ in cases]
    for (ad, bd), out in zip(dev, outs):
        ops.l1_sum(ad, bd, 0.5, out, zero_first=True)
    assert [o.item() for o in outs] == [0.5 * tot.item() for _, _, tot in cases]
    acc = torch.zeros(1, device=DEV)
    for ad, bd in dev:
        ops.l1_sum(ad, bd, 2.0, acc)
    assert acc.item() == 2.0 * sum(tot.item() for _, _, tot in cases)


# ---- 3. relativistic BCE: cap 256 x 256 --------------------------------------------------------------------------------------------------------
BCE_LAYOUTS = ("pixel", "flat", "offset")


def bce_layout(layout, n):
    """-> (buffer elements, first element, stride): `pixel` = channel 0 of 8-channel pixels on a 16-byte aligned base (the whole pixel is written);
    `flat` = stride 1 with 8 guard elements on both sides; `offset` = stride 8 with the base one element in (not 16-byte aligned: single stores)"""
    return {"pixel": (8 * n, 0, 8), "flat": (n + 16, 8, 1), "offset": (8 * n + 8, 1, 8)}[layout]


def bce_place(vals, n, layout, fill):
    size, off, stride = bce_layout(layout, n)
    t = torch.full((size,), fill, dtype=vals.dtype)
    t[off:off + stride * n:stride] = vals[:n]
    return t.to(DEV)


def bce_take(buf, n, layout):
    """-> (the n addressed elements as float64, True when everything else is as it must be: zeros in channels 1..7 of a whole-pixel store, SENT
    wherever a single-element store must not reach)"""
    size, off, stride = bce_layout(layout, n)
    got = buf.cpu().double()
    want = torch.full((size,), 0.0 if layout == "pixel" else SENT, dtype=torch.float64)
    vals = got[off:off + stride * n:stride].clone()
    got[off:off + stride * n:stride] = 0
    want[off:off + stride * n:stride] = 0
    return vals, torch.equal(got, want)


def bce_call(dtype, a, b, n, layout, mode, gscale, loss, with_db):
    lib = ops.lib()
    size, off, stride = bce_layout(layout, n)
    da = torch.full((size,), SENT, dtype=dtype, device=DEV)
    db = torch.full((size,), SENT, dtype=dtype, device=DEV) if with_db else None
    check(lib.tfc_bce_relativistic(st(), dt_of(dtype), P(a, off), P(b, off), n, stride, R.BCE_T1, R.BCE_T2, mode, P(loss), P(da, off),
                                   None if db is None else P(db, off), gscale), "tfc_bce_relativistic")
    return da, db


@pytest.fixture(scope="module", params=DTYPES, ids=["fp32", "bf16"])
def bce_family(request):
    return (request.param,) + R.bce_logits(request.param)


@pytest.mark.parametrize("layout", BCE_LAYOUTS)
def test_bce_gradients_and_loss(layout, bce_family):
    """tfc_bce_relativistic at n = 1, 257, 256 x 256, + 1, 2 x 256 x 256 + 5, modes 0 and 1, t1 = 0.9, gscale 1 and 0.25, on logits covering
    [-30, 30], an exact 0 and +-90, against fp64 on the stored logits:
      gradient, fp32: 8 x the largest error of torch-CPU fp32 against fp64 (on the family's logits at this n); bf16: + 2^-8 |ref| for the storage rounding;
      loss: 8 x the largest per-logit error of torch-CPU fp32 binary_cross_entropy_with_logits (a mean is no further off than its worst term).
    Both figures are printed. da alone and da + db: db == -da exactly, and da of the two calls is bit-equal (the loss of the two is NOT asserted
    bit-equal: its double atomics arrive in any order). `pixel`: channels 1..7 of every pixel are 0 afterwards; `flat` / `offset`: only the
    addressed element changes. One loss buffer serves all calls: the kernel stores the mean, so no result contains an earlier one."""
    dtype, a, b = bce_family
    loss = torch.full((2,), SENT, device=DEV)
    for n in R.BCE_SIZES:
        ad, bd = bce_place(a, n, layout, 123.0), bce_place(b, n, layout, -77.0)
        for mode in (0, 1):
            for gscale in R.BCE_GSCALES:
                ref = R.bce_ref(a, b, n, mode, gscale)
                da1, _ = bce_call(dtype, ad, bd, n, layout, mode, gscale, loss, False)
                l1 = loss.cpu()
                da2, db2 = bce_call(dtype, ad, bd, n, layout, mode, gscale, loss, True)
                l2 = loss.cpu()
                (g1, ok1), (g2, ok2), (gb, okb) = bce_take(da1, n, layout), bce_take(da2, n, layout), bce_take(db2, n, layout)
                assert ok1 and ok2 and okb, (n, mode, gscale, "elements outside the addressed ones")
                assert torch.equal(g1, g2) and torch.equal(gb, -g2), (n, mode, gscale)
                bound = 8 * ref["grad_err"] + (R.EPS8 * ref["da"].abs() if dtype == torch.bfloat16 else 0.0)
                err = (g1 - ref["da"]).abs()
                lerr = max(abs(l1[0].item() - ref["loss"]), abs(l2[0].item() - ref["loss"]))
                say(f"bce {layout} {str(dtype)[6:]} n={n} mode={mode} gscale={gscale}: gradient error {err.max().item():.3e} "
                    f"(fp32-CPU error {ref['grad_err']:.3e}), loss error {lerr:.3e} (fp32-CPU per-logit error {ref['loss_err']:.3e})")
                assert (err <= bound).all(), (n, mode, gscale, err.max().item(), ref["grad_err"])
                assert lerr <= 8 * ref["loss_err"] and l1[1].item() == SENT and l2[1].item() == SENT, (n, mode, gscale, lerr, ref["loss_err"])


def test_bce_back_to_back_calls_do_not_mix(bce_family):
    """two calls with different n and no synchronize between them, into two loss buffers and then into one: each holds its own mean (grids of 256
    and 2 workgroups share g_bce_slot; a slot that is not re-armed, or a kernel that adds, puts the first loss into the second)"""
    dtype, a, b = bce_family
    n1, n2 = R.BCE_SIZES[-1], 257
    a1, b1, a2, b2 = (bce_place(t, n, "pixel", 0.0) for n in (n1, n2) for t in (a, b))
    r1, r2 = R.bce_ref(a, b, n1, 1, 1.0), R.bce_ref(a, b, n2, 0, 1.0)
    la, lb = torch.full((1,), SENT, device=DEV), torch.full((1,), SENT, device=DEV)
    bce_call(dtype, a1, b1, n1, "pixel", 1, 1.0, la, True)
    bce_call(dtype, a2, b2, n2, "pixel", 0, 1.0, lb, False)
    assert abs(la.item() - r1["loss"]) <= 8 * r1["loss_err"] and abs(lb.item() - r2["loss"]) <= 8 * r2["loss_err"]
    bce_call(dtype, a1, b1, n1, "pixel", 1, 1.0, la, False)
    bce_call(dtype, a2, b2, n2, "pixel", 0, 1.0, la, False)
    assert abs(la.item() - r2["loss"]) <= 8 * r2["loss_err"] and abs(r1["loss"] - r2["loss"]) > 1000 * r2["loss_err"]


# ---- 4. spectral-norm backward: 128 dot partials of 1024 elements ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_spectral_norm_bwd(shape):
    """tfc_spectral_norm_bwd with u, v and sigma2 = (sigma, 1 / sigma) as one tfc_spectral_norm_step leaves them, against the fp64 autograd of
    ((W / (u W v)) G).sum() at those u, v. Bound: 8 x the largest error of the same expression in torch-CPU fp32 (printed, both relative to
    max |grad|). accumulate = 0 into a SENT-filled gout; accumulate = 1 onto a pre-filled one, where `the same expression` includes the
    addition. (130, 1031) and (64, 8193) pass the 128-partial cap with ragged tails, on the scalar and on the float4 loop of tfc_dot_kernel.
    R = K = 1 is dyadic and its gradient identically zero: there the bound is 0 and the assertion is equality."""
    Rr, K = shape
    W, G, u, v = R.sn_case(Rr, K, 50 + Rr)
    Wd, Gd, ud, vd = (t.to(DEV) for t in (W, G, u, v))
    s2 = torch.zeros(2, device=DEV)
    ops.spectral_norm_step(Wd, ud, vd, s2, power_iter=True)
    u1, v1 = ud.cpu(), vd.cpu()
    ref, cpu = R.sn_grad(W, G, u1, v1, torch.float64), R.sn_grad(W, G, u1, v1, torch.float32)
    scale = max(ref.abs().max().item(), 1e-300)
    assert abs(s2[0].item() * s2[1].item() - 1) < 1e-6
    gout = torch.full((Rr * K + 1,), SENT, device=DEV)
    ops_ws = torch.empty(256, device=DEV)                          # the dot product's per-workgroup partials (128 doubles)
    check(ops.lib().tfc_spectral_norm_bwd(st(), P(Gd), P(Wd), P(ud), P(vd), P(s2), P(ops_ws), P(gout), Rr, K, 0), "tfc_spectral_norm_bwd")
    got = gout.cpu()
    err, err32 = (got[:-1].view(Rr, K).double() - ref).abs().max().item(), (cpu.double() - ref).abs().max().item()
    say(f"sn_bwd {Rr}x{K}: error {err / scale:.3e}, fp32-CPU error {err32 / scale:.3e} of max |grad| = {scale:.3e}")
    assert err <= 8 * err32 and got[-1].item() == SENT
    pre = torch.randn(Rr, K, generator=torch.Generator().manual_seed(9))
    gacc = guarded(pre.flatten())
    check(ops.lib().tfc_spectral_norm_bwd(st(), P(Gd), P(Wd), P(ud), P(vd), P(s2), P(ops_ws), P(gacc), Rr, K, 1), "tfc_spectral_norm_bwd")
    got = gacc.cpu()
    ref_acc = pre.double() + ref
    err, err32 = (got[:-1].view(Rr, K).double() - ref_acc).abs().max().item(), ((pre + cpu).double() - ref_acc).abs().max().item()
    say(f"sn_bwd {Rr}x{K} accumulate: error {err / scale:.3e}, fp32-CPU error {err32 / scale:.3e} of max |grad|")
    assert err <= 8 * err32 and got[-1].item() == SENT


# ---- 5. PatchGAN head forward ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,C", R.HEAD_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_patchgan_head_exact(dtype, C):
    """tfc_patchgan_head_fwd on ternary data (|sum| <= 16 C: exact in fp32, one storage rounding) at (1, 1, 1), (1, 3, 5) and (3, 27, 27) = 2187
    pixels, past the 2048 that 512 workgroups cover in one trip. Registers hold the filter at C = 64 (both dtypes) and C = 512 in bf16; LDS at
    C = 512 in fp32 and C = 1024 in bf16. The logit goes to channel 0 of an 8-channel buffer whose other channels keep SENT; x alone (pitch C) and
    as channels [8, 8 + C) of a buffer of pitch C + 16 filled with SENT."""
    dt = dt_of(dtype)
    assert R.head_uses_lds(dtype, C) == ((dtype, C) in ((torch.float32, 512), (torch.bfloat16, 1024)))
    for i, (N, H, W) in enumerate(R.HEAD_SHAPES):
        x, w, want = R.head_case(N, H, W, C, 80 + i)
        wd = w.float().to(DEV)
        want = X.store(want[:, 0], dt)
        for wide in (False, True):
            coff, pitch = (8, C + 16) if wide else (0, C)
            xb = torch.full((N, H, W, pitch), SENT, dtype=dtype)
            xb[..., coff:coff + C] = x.permute(0, 2, 3, 1).to(dtype)
            logits = torch.full((N, H, W, 8), SENT, dtype=dtype, device=DEV)
            ops.patchgan_head_fwd(dt, View(xb.to(DEV), C, coff), wd, View(logits, 1, 0))
            got = logits.cpu()
            bad = (got[..., 0] != want).nonzero()
            assert torch.equal(got[..., 0], want), (N, H, W, wide, len(bad), bad[:4].tolist())
            assert (got[..., 1:] == SENT).all(), (N, H, W, wide)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """Bad arguments to the entry points of this file return non-zero with the check's text in tfc_last_error(), and launch nothing: every
    buffer handed over keeps its fill after a synchronize. Null pointers and n <= 0 everywhere; C > 4 for tfc_tanh_bwd_pack, Ca + Cb > 8 for the
    packer, dbias without part_ws; tfc_colsum's pitch < C, pitch % ue != 0, unaligned x and C = 0; C = 0 and N, H, W = 0 in fill_act
    (tfc_act_fwd / tfc_act_bwd: 256 % (C / ue) divided by zero on the host before the check). Every other argument of each call is valid for
    buffers of 4096 elements, so nothing here could address out of range even if a check were missing."""
    lib = ops.lib()
    f32 = [torch.full((4096,), SENT, device=DEV) for _ in range(6)]
    b16 = [torch.full((4096,), SENT, dtype=torch.bfloat16, device=DEV) for _ in range(2)]
    u8 = torch.full((4096,), 7, dtype=torch.uint8, device=DEV)
    a, b, c, d, e, f = (P(t) for t in f32)
    h, k = (P(t) for t in b16)
    ws = ops.part_ws(torch.device(DEV))
    s = st()
    hp = (2e-4, 0.5, 0.999, 1e-8)
    cases = [
        (b"bad args", lambda: lib.tfc_cast(s, DT_F32, 0, None, b, 64)),
        (b"bad args", lambda: lib.tfc_cast(s, DT_BF16, 0, a, None, 64)),
        (b"bad args", lambda: lib.tfc_cast(s, DT_BF16, 1, h, b, 0)),
        (b"bad args", lambda: lib.tfc_axpby(s, None, a, b, 64, 1.0, 1.0)),
        (b"bad args", lambda: lib.tfc_axpby(s, c, None, b, 64, 1.0, 1.0)),
        (b"bad args", lambda: lib.tfc_axpby(s, c, a, b, -1, 1.0, 1.0)),
        (b"bad args", lambda: lib.tfc_dropout_mask(s, None, 64, 0.5, 1)),
        (b"bad args", lambda: lib.tfc_dropout_mask(s, P(u8), 0, 0.5, 1)),
        (b"bad args", lambda: lib.tfc_adam_step(s, None, b, c, d, 64, *hp, 1, 1.0)),
        (b"bad args", lambda: lib.tfc_adam_step(s, a, None, c, d, 64, *hp, 1, 1.0)),
        (b"bad args", lambda: lib.tfc_adam_step(s, a, b, None, d, 64, *hp, 1, 1.0)),
        (b"bad args", lambda: lib.tfc_adam_step(s, a, b, c, None, 64, *hp, 1, 1.0)),
        (b"bad args", lambda: lib.tfc_adam_step(s, a, b, c, d, 0, *hp, 1, 1.0)),
        (b"bad args", lambda: lib.tfc_adam_step(s, a, b, c, d, 64, *hp, 0, 1.0)),
        (b"x must be a 16-byte aligned", lambda: lib.tfc_colsum(s, DT_F32, None, 4, 8, 8, b, None)),
        (b"x must be a 16-byte aligned", lambda: lib.tfc_colsum(s, DT_F32, a + 4, 4, 8, 8, b, None)),
        (b"x must be a 16-byte aligned", lambda: lib.tfc_colsum(s, DT_BF16, h + 2, 4, 8, 8, b, None)),
        (b"bad args", lambda: lib.tfc_colsum(s, DT_F32, a, 4, 8, 8, None, None)),
        (b"bad args", lambda: lib.tfc_colsum(s, DT_F32, a, 0, 8, 8, b, None)),
        (b"bad args", lambda: lib.tfc_colsum(s, DT_F32, a, 4, 8, 0, b, None)),
        (b"bad args", lambda: lib.tfc_colsum(s, DT_BF16, h, 4, 16, 12, b, None)),
        (b"x pitch 4 must be >= 8", lambda: lib.tfc_colsum(s, DT_F32, a, 4, 4, 8, b, None)),
        (b"x pitch 12 must be >= 8 and a multiple of 8", lambda: lib.tfc_colsum(s, DT_BF16, h, 4, 12, 8, b, None)),
        (b"bad dtype 7", lambda: lib.tfc_colsum(s, 7, a, 4, 8, 8, b, None)),
        (b"bad args (C <= 4)", lambda: lib.tfc_tanh_bwd_pack(s, DT_F32, None, b, c, None, 1, 3, 4, 4, None)),
        (b"bad args (C <= 4)", lambda: lib.tfc_tanh_bwd_pack(s, DT_F32, a, b, None, None, 1, 3, 4, 4, None)),
        (b"bad args (C <= 4)", lambda: lib.tfc_tanh_bwd_pack(s, DT_F32, a, b, c, None, 1, 5, 4, 4, None)),
        (b"bad args (C <= 4)", lambda: lib.tfc_tanh_bwd_pack(s, DT_F32, a, b, c, None, 1, 0, 4, 4, None)),
        (b"bad args (C <= 4)", lambda: lib.tfc_tanh_bwd_pack(s, DT_F32, a, b, c, None, 0, 3, 4, 4, None)),
        (b"dbias needs part_ws", lambda: lib.tfc_tanh_bwd_pack(s, DT_F32, a, b, c, d, 1, 3, 4, 4, None)),
        (b"bad args", lambda: lib.tfc_pack_nhwc8(s, DT_F32, a, 5, b, 4, c, 1, 4, 4)),
        (b"bad args", lambda: lib.tfc_pack_nhwc8(s, DT_F32, None, 3, b, 3, c, 1, 4, 4)),
        (b"bad args", lambda: lib.tfc_pack_nhwc8(s, DT_F32, a, 3, None, 3, c, 1, 4, 4)),
        (b"bad args", lambda: lib.tfc_pack_nhwc8(s, DT_F32, a, 0, b, 3, c, 1, 4, 4)),
        (b"bad args", lambda: lib.tfc_pack_nhwc8(s, DT_F32, a, 3, b, 3, None, 1, 4, 4)),
        (b"bad args", lambda: lib.tfc_pack_nhwc8(s, DT_F32, a, 3, b, 3, c, 1, 0, 4)),
        (b"bad args", lambda: lib.tfc_l1_sum(s, None, b, 64, 1.0, c, 1)),
        (b"bad args", lambda: lib.tfc_l1_sum(s, a, None, 64, 1.0, c, 1)),
        (b"bad args", lambda: lib.tfc_l1_sum(s, a, b, 64, 1.0, None, 1)),
        (b"bad args", lambda: lib.tfc_l1_sum(s, a, b, 0, 1.0, c, 1)),
        (b"bad args", lambda: lib.tfc_bce_relativistic(s, DT_F32, None, b, 64, 8, 0.9, 0.0, 0, c, d, e, 1.0)),
        (b"bad args", lambda: lib.tfc_bce_relativistic(s, DT_F32, a, None, 64, 8, 0.9, 0.0, 0, c, d, e, 1.0)),
        (b"bad args", lambda: lib.tfc_bce_relativistic(s, DT_F32, a, b, 64, 8, 0.9, 0.0, 0, None, d, e, 1.0)),
        (b"bad args", lambda: lib.tfc_bce_relativistic(s, DT_F32, a, b, 0, 8, 0.9, 0.0, 0, c, d, e, 1.0)),
        (b"bad args", lambda: lib.tfc_bce_relativistic(s, DT_F32, a, b, 64, 0, 0.9, 0.0, 0, c, d, e, 1.0)),
        (b"bad args", lambda: lib.tfc_bce_relativistic(s, DT_F32, a, b, 64, 8, 0.9, 0.0, 2, c, d, e, 1.0)),
        (b"bad args (ws", lambda: lib.tfc_spectral_norm_bwd(s, None, b, c, d, e, ws, f, 4, 4, 0)),
        (b"bad args (ws", lambda: lib.tfc_spectral_norm_bwd(s, a, b, c, d, e, ws, None, 4, 4, 0)),
        (b"bad args (ws", lambda: lib.tfc_spectral_norm_bwd(s, a, b, c, d, e, None, f, 4, 4, 0)),
        (b"bad args (ws", lambda: lib.tfc_spectral_norm_bwd(s, a, b, c, d, e, ws.value + 4, f, 4, 4, 0)),
        (b"bad args (ws", lambda: lib.tfc_spectral_norm_bwd(s, a, b, c, d, e, ws, f, 0, 4, 0)),
        (b"bad args (ws", lambda: lib.tfc_spectral_norm_bwd(s, a, b, c, d, e, ws, f, 4, 0, 0)),
        (b"x must be a 16-byte aligned", lambda: lib.tfc_patchgan_head_fwd(s, DT_F32, None, 8, 1, 4, 4, 8, b, c, 8)),
        (b"x must be a 16-byte aligned", lambda: lib.tfc_patchgan_head_fwd(s, DT_F32, a + 4, 8, 1, 4, 4, 8, b, c, 8)),
        (b"bad args", lambda: lib.tfc_patchgan_head_fwd(s, DT_F32, a, 8, 1, 4, 4, 8, None, c, 8)),
        (b"bad args", lambda: lib.tfc_patchgan_head_fwd(s, DT_F32, a, 8, 1, 4, 4, 8, b, None, 8)),
        (b"bad args", lambda: lib.tfc_patchgan_head_fwd(s, DT_F32, a, 8, 0, 4, 4, 8, b, c, 8)),
        (b"bad args", lambda: lib.tfc_patchgan_head_fwd(s, DT_F32, a, 8, 1, 4, 4, 0, b, c, 8)),
        (b"bad args", lambda: lib.tfc_patchgan_head_fwd(s, DT_BF16, h, 8, 1, 4, 4, 4, b, k, 8)),
        (b"bad args", lambda: lib.tfc_patchgan_head_fwd(s, DT_F32, a, 4, 1, 4, 4, 8, b, c, 8)),
        (b"bad args", lambda: lib.tfc_patchgan_head_fwd(s, DT_F32, a, 8, 1, 4, 4, 8, b, c, 0)),
        (b"bad dims N=1 H=4 W=4 C=0", lambda: lib.tfc_act_fwd(s, DT_F32, a, 8, 1, 4, 4, 0, None, 0, 0.2, 0, 0.0, 0, b, 8, None, None)),
        (b"bad dims N=1 H=4 W=4 C=0", lambda: lib.tfc_act_fwd(s, DT_BF16, h, 8, 1, 4, 4, 0, None, 0, 0.2, 0, 0.0, 0, k, 8, None, None)),
        (b"bad dims N=0", lambda: lib.tfc_act_fwd(s, DT_F32, a, 8, 0, 4, 4, 8, None, 0, 0.2, 0, 0.0, 0, b, 8, None, None)),
        (b"bad dims N=1 H=0", lambda: lib.tfc_act_fwd(s, DT_F32, a, 8, 1, 0, 4, 8, None, 0, 0.2, 0, 0.0, 0, b, 8, None, None)),
        (b"bad dims N=1 H=4 W=0", lambda: lib.tfc_act_fwd(s, DT_F32, a, 8, 1, 4, 0, 8, None, 0, 0.2, 0, 0.0, 0, b, 8, None, None)),
        (b"bad dims N=1 H=4 W=4 C=0", lambda: lib.tfc_act_bwd(s, DT_F32, 0, a, 8, b, 8, 1, 4, 4, 0, None, 0, 0.2, 0, 0.0, 0, None, c, 8, None)),
    ]
    for i, (text, call) in enumerate(cases):
        assert call() != 0, f"case {i} was not refused"
        msg = lib.tfc_last_error()
        assert msg and text in msg, (i, text, msg)
    check(lib.tfc_colsum(s, DT_F32, a, 4, 8, 8, b, None), "tfc_colsum")          # the checks let a good call through: b[:8] += 4 x 7
    torch.cuda.synchronize()
    assert torch.equal(f32[1][:8].cpu(), torch.full((8,), 5 * SENT))
    f32[1][:8] = SENT
    for t in f32 + b16:
        assert (t == SENT).all()
    assert (u8 == 7).all()
