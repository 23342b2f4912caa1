"""Restatements, launch routes, case tables and input builders shared by tests/test_gpu_55_act_edges.py (against the kernels) and
tests/test_act_edges_host.py (against torch autograd, on the CPU): the activation section of csrc/elementwise.hip -- tfc_act_fwd_kernel,
tfc_act_pool2_fwd_kernel, tfc_act_bwd_kernel, tfc_act_pool2_bwd_kernel, tfc_blur1_kernel (forward and transpose) and tfc_norm_add_kernel.

ONE numpy restatement serves both precisions: every function takes the working dtype `wd` (np.float64: the reference; np.float32: the
restatement whose error against the reference scales the bound tier). The blur is a pair of [Lo, L] matrices with the reflect aliases merged
(conv_exact.blur / blur_t handle non-square planes too and are what the host test holds these matrices against; they are torch, float64 only,
and cannot carry the mutants of the sensitivity test, so the matrices are written here). Cross-pixel sums add in pixel order, one add per
pixel (np.cumsum), as a lane of the kernels does: a pairwise sum would understate the fp32 error the bound is scaled by.

route() restates the launchers (act_fwd_t, act_bwd_t, blur1_launch, tfc_launch_norm_add, tfc_launch_act_pool2_bwd_signs, act_grid and
tfc_act_grid_cap of csrc/elementwise.hip; fill_act of csrc/api.hip) and every case table below is built through it: an entry carries the
name of the route it is there for. No import side effects, no GPU."""
import functools
from collections import namedtuple

import numpy as np
import torch

from oracle import tfcgan_oracle as O

F32, F64 = np.float32, np.float64
EPS = float(np.float32(1e-5))                                     # ActParams.eps is a float
EPS8 = 2.0 ** -8
ACT_CAP, REF_BATCH, PART_WS_FLOATS = 4096, 32, 8 << 20            # TFC_ACT_CAP (elementwise.hip), TFC_REF_BATCH, TFC_PART_WS_FLOATS (tfc_desc.h)
BF16, FP32 = torch.bfloat16, torch.float32
DTYPES = (FP32, BF16)
SLOPES_EXACT = (1.0, 0.25, 0.0)                                   # dyadic: 9/64 x 0.2f rounds
MUTANTS = ("no_alias_n2", "no_alias_n3", "no_alias_m1", "swap_taps_last_row", "ho_half", "drop_npix_in", "drop_no_slice_offset", "slot_left_out",
           "swap_s1_s2", "act0_is_1", "mg_is_sum")


def ue_of(dtype):
    return 8 if dtype == BF16 else 4


def cheap_c(dtype):
    return ue_of(dtype)


def tiled_c(dtype):
    """the narrowest width blur1_launch accepts: 8 channel vectors"""
    return 8 * ue_of(dtype)


def legal_widths(dtype):
    """every C fill_act accepts: C / ue divides 256"""
    return tuple(ue_of(dtype) << k for k in range(9))


def out_len(L, pool, mutant=None):
    if pool != 2:
        return L
    return L // 2 if mutant == "ho_half" else (L - 1) // 2 + 1


# ---- launch routes -----------------------------------------------------------------------------------------------------------------------------
Route = namedtuple("Route", "kernel grid slots trips ragged")     # grid (x, y, z); slots: partial-sum slots per image (0: no reduction)
REFUSED = "refused: the partial sums pass part_ws"
ROUTES = ("act_fwd<stats>", "act_fwd", "pool2_fwd<act>", "pool2_fwd<blur>", "blur1_fwd<stats>", "blur1_fwd", "blur1_t",
          "act_bwd<0,0>", "act_bwd<0,1>", "act_bwd<0,2>", "act_bwd<1,0>", "act_bwd<1,1>", "act_bwd<2,0>", "act_bwd<2,1>",
          "pool2_bwd<0>", "pool2_bwd<1>", "pool2_bwd<2>", "pool2_bwd<signs>", "norm_add")


def act_grid_cap(N, inv):
    return max(ACT_CAP // (REF_BATCH if inv else N), 1)


def act_grid(npix, C, dtype, N, inv):
    """(workgroups per image, trips of the busiest lane, whether the last trip is ragged) of act_grid's capped grid-stride launch"""
    ppb = 256 // (C // ue_of(dtype))
    nb = min(-(-npix // ppb), act_grid_cap(N, inv))
    return nb, -(-npix // (nb * ppb)), npix % (nb * ppb) != 0


def blur1_accepts(dtype, H, W, C):
    return C % (8 * ue_of(dtype)) == 0 and H >= 4 and W >= 4


def route(entry, dtype, N, H, W, C, pool=0, norm=False, slope=1.0, drop=0.0, stats_out=False, use_x=True, rstats=False, mode=0, inv=False):
    """the kernel an entry point launches and its grid. entry: "fwd" (tfc_act_fwd), "bwd" (tfc_act_bwd), "signs", "nadd"."""
    ue = ue_of(dtype)
    Ho, Wo = out_len(H, pool), out_len(W, pool)

    def generic(kernel, npix, red_l):
        nb, trips, ragged = act_grid(npix, C, dtype, N, inv)
        if nb * N * red_l > PART_WS_FLOATS:                        # part_fits: the launcher returns hipErrorInvalidValue and launches nothing
            kernel = REFUSED
        return Route(kernel, (nb, N, 1), nb if red_l else 0, trips, ragged)

    def tiled(kernel, th, cs, red_l):
        nb = -(-W // 32) * -(-H // th)
        if nb * N * red_l > PART_WS_FLOATS:
            kernel = REFUSED
        return Route(kernel, (nb, N, C // cs), nb if red_l else 0, 1, H % th != 0 or W % 32 != 0)

    if entry == "nadd":
        return generic("norm_add", H * W, 0)
    if entry == "signs":
        return tiled("pool2_bwd<signs>", 16, 64, C if rstats else 0)
    if entry == "fwd":
        if pool == 2 and not stats_out:
            return generic("pool2_fwd<blur>" if (not norm and slope == 1.0) else "pool2_fwd<act>", ((Ho + 1) // 2) * ((Wo + 1) // 2), 0)
        if pool == 1 and not norm and slope == 1.0 and not drop and blur1_accepts(dtype, H, W, C):
            r = tiled("blur1_fwd<stats>" if stats_out else "blur1_fwd", 8, 8 * ue, 2 * C if stats_out else 0)
            if r.kernel != REFUSED:                                # blur1_launch declines; the generic kernel's launcher reports the error
                return r
        return generic("act_fwd<stats>" if stats_out else "act_fwd", Ho * Wo, 2 * C if stats_out else 0)
    assert entry == "bwd"
    red = 2 * C if mode == 1 else (C if (mode == 0 and rstats) else 0)
    if pool == 2 and use_x:                                       # every legal C is ue x 2^k: C < 64 is its own slice, C >= 64 a multiple of 64
        return tiled(f"pool2_bwd<{mode}>", 16, min(C, 64), red)
    if pool == 1 and mode == 0 and not use_x and not rstats and not drop and blur1_accepts(dtype, H, W, C):
        return tiled("blur1_t", 8, 8 * ue, False)
    return generic(f"act_bwd<{mode},{pool}>", H * W, red)


# ---- the blur as matrices ----------------------------------------------------------------------------------------------------------------------
def blur_matrix(L, pool, wd=F64, mutant=None):
    """[Lo, L]: row o holds the taps [1, 3, 3, 1] / 8 at padded positions o * pool - 1 + k, reflect pad (1, 2): -1 -> 1, L -> L - 2, L + 1 -> L - 3"""
    Lo = out_len(L, pool, mutant)
    B = np.zeros((Lo, L), dtype=F64)
    for o in range(Lo):
        taps = (3, 1, 1, 3) if (mutant == "swap_taps_last_row" and o == Lo - 1) else (1, 3, 3, 1)
        for k in range(4):
            p = o * pool - 1 + k
            if p == -1:
                if mutant == "no_alias_m1":
                    continue
                p = 1
            elif p == L:
                if mutant == "no_alias_n2":
                    continue
                p = L - 2
            elif p == L + 1:
                if mutant == "no_alias_n3":
                    continue
                p = L - 3
            B[o, p] += taps[k] / 8.0
    return B.astype(wd)


def blur_fwd(a, pool, wd=F64, mutant=None):
    """row mutants act on the vertical pass only ("the last output row")"""
    By = blur_matrix(a.shape[2], pool, wd, mutant)
    Bx = blur_matrix(a.shape[3], pool, wd, None if mutant == "swap_taps_last_row" else mutant)
    return np.einsum("oh,nchw,pw->ncop", By, a, Bx, optimize=True).astype(wd)


def blur_bwd(g, H, W, pool, wd=F64, mutant=None):
    By = blur_matrix(H, pool, wd, mutant)
    Bx = blur_matrix(W, pool, wd, None if mutant == "swap_taps_last_row" else mutant)
    g = g[:, :, :By.shape[0], :Bx.shape[0]]                        # a mutant's smaller plane reads what it covers
    return np.einsum("oh,ncop,pw->nchw", By, g, Bx, optimize=True).astype(wd)


# ---- restatements ------------------------------------------------------------------------------------------------------------------------------
def plane_sum(a, wd, mutant=None):
    """[N, C, H, W] -> [N, C], one add per pixel in pixel order. Mutant: the last pixel's slot (a PPB = 1 workgroup) is left out."""
    f = a.reshape(a.shape[0], a.shape[1], -1).astype(wd)
    if mutant == "slot_left_out":
        f = f[..., :-1]
    return np.cumsum(f, axis=-1, dtype=wd)[..., -1]


def norm_consts(stats, HW, wd=F64):
    """(mean, rstd) [N, C, 1, 1] from the fp32 sums (s1, s2) as the kernels derive them"""
    s = stats.astype(wd)
    inv = wd(1.0) / wd(HW)
    m = s[..., 0] * inv
    var = np.maximum(s[..., 1] * inv - m * m, wd(0.0))
    r = wd(1.0) / np.sqrt(var + wd(EPS))
    return m[:, :, None, None].astype(wd), r[:, :, None, None].astype(wd)


def keep_mask(seed, N, Ho, Wo, C, p, mutant=None, in_hw=None):
    """[N, C, Ho, Wo] bool: O.hip_keep_mask at element index (n Ho Wo + opix) C + c"""
    n, o, c = np.meshgrid(np.arange(N, dtype=np.int64), np.arange(Ho * Wo, dtype=np.int64), np.arange(C, dtype=np.int64), indexing="ij")
    per_image = in_hw if mutant == "drop_npix_in" else Ho * Wo
    cc = c % 64 if mutant == "drop_no_slice_offset" else c
    idx = (n * per_image + o) * C + cc
    flat = O.hip_keep_mask(seed, int(idx.max()) + 1, p)
    return np.ascontiguousarray(flat[idx].reshape(N, Ho, Wo, C).transpose(0, 3, 1, 2))


def xhat_of(x, stats, wd):
    x = x.astype(wd)
    if stats is None:
        return x, None
    m, r = norm_consts(stats, x.shape[2] * x.shape[3], wd)
    return (x - m) * r, r


def act_fwd_ref(x, stats=None, slope=1.0, pool=0, keep=None, drop_p=0.0, wd=F64, mutant=None):
    """[norm at stats] -> leaky(slope) -> blur(pool) -> dropout; NCHW numpy in, NCHW of dtype wd out"""
    xh, _ = xhat_of(x, stats, wd)
    a = np.where(xh > 0, xh, xh * wd(slope))
    if pool:
        a = blur_fwd(a, pool, wd, mutant)
    if keep is not None:
        if keep.shape != a.shape:                                  # a mutant's plane of another size
            keep = np.resize(keep, a.shape)
        a = np.where(keep, a * wd(1.0 / (1.0 - drop_p)), wd(0.0))
    return a.astype(wd)


def stored_stats(stored, wd=F64, mutant=None):
    """[N, C, 2]: sum and sum of squares of the STORED result"""
    s = stored.astype(wd)
    return np.stack((plane_sum(s, wd, mutant), plane_sum(s * s, wd, mutant)), -1)


def act_bwd_ref(mode, dy, x=None, stats=None, slope=1.0, pool=0, hw=None, keep=None, drop_p=0.0, rstats=None, wd=F64, mutant=None):
    """mode 0: (dx, per-image bias sums [N, C]); mode 1: [N, C, 2] = (sum g', sum g' xhat); mode 2: dx = rstd (g' - mg - xhat mgx).
    g' = blur^T(keep dy / (1 - p)) act'(xhat), act'(xhat) = xhat > 0 ? 1 : slope; x = None: act' = 1. hw: the input plane (H, W)."""
    H, W = hw
    g = dy.astype(wd)
    if keep is not None:
        g = np.where(keep, g * wd(1.0 / (1.0 - drop_p)), wd(0.0))
    if pool:
        g = blur_bwd(g, H, W, pool, wd, mutant)
    xh, r = (np.zeros_like(g), None) if x is None else xhat_of(x, stats, wd)
    if x is not None:
        pos = (xh >= 0) if mutant == "act0_is_1" else (xh > 0)
        g = g * np.where(pos, wd(1.0), wd(slope))
    if mode == 0:
        return g.astype(wd), plane_sum(g, wd, mutant)
    if mode == 1:
        s = (plane_sum(g, wd, mutant), plane_sum(g * xh, wd, mutant))
        return np.stack(s[::-1] if mutant == "swap_s1_s2" else s, -1)
    inv = wd(1.0) if mutant == "mg_is_sum" else wd(1.0) / wd(H * W)
    rs = rstats.astype(wd)
    mg, mgx = (rs[..., 0] * inv)[:, :, None, None], (rs[..., 1] * inv)[:, :, None, None]
    return (r * (g - mg - xh * mgx)).astype(wd)


def norm_add_ref(x, res, stats, wd=F64):
    xh, _ = xhat_of(x, stats, wd)
    return (res.astype(wd) + xh).astype(wd)


# ---- storage, comparison -----------------------------------------------------------------------------------------------------------------------
def store(a, dtype):
    """numpy -> torch in the storage type, rounded once (fp32, then round-to-nearest-even to bf16)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(dtype)


def stored_np(a, dtype):
    """the stored tensor's values as float64 numpy"""
    return store(a, dtype).to(torch.float64).numpy()


def assert_exact_ref(a, quantum, what):
    """the float64 reference is exact in fp32 in any order: every element a multiple of 1 / quantum, below 2^24 quanta (conv_exact.assert_dyadic)"""
    s = np.asarray(a, dtype=F64) * quantum
    assert np.array_equal(s, np.round(s)), f"{what}: the reference is not a multiple of 1/{quantum}"
    assert np.abs(s).max(initial=0.0) < (1 << 24), f"{what}: |reference| reaches 2^24 quanta"


def same_bits(got, want):
    """the exact tier's comparison: same shape, same type, torch.equal"""
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want)


def e32_of(ref32, ref64):
    """largest error of the fp32 restatement against the reference on the case's tensor"""
    return float(np.max(np.abs(ref32.astype(F64) - ref64), initial=0.0))


def bound_of(ref64, e32, bf16_store):
    """per element: 8 e32 (+ 2^-8 |ref| for a bf16 store)"""
    return 8.0 * e32 + (EPS8 * np.abs(ref64) if bf16_store else 0.0)


def bound_ratio(got, ref64, e32, bf16_store):
    """largest error / bound over every element (inf on a shape mismatch); the bound tier accepts <= 1"""
    got = np.asarray(got, dtype=F64)
    if got.shape != ref64.shape:
        return float("inf")
    b = bound_of(ref64, e32, bf16_store)
    err = np.abs(got - ref64)
    if not np.all(np.isfinite(err)):
        return float("inf")
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(b, 1e-300)), initial=0.0))


# ---- data --------------------------------------------------------------------------------------------------------------------------------------
def ternary(shape, seed):
    """float64 numpy in {-1, 0, 1} (conv_exact.ints at amp 1)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-1, 2, tuple(shape), generator=g, dtype=torch.int64).to(torch.float64).numpy()


def knife_free(shape, seed, dtype, lo=0.25, hi=2.0, zero_plane=True):
    """test_gpu_00_kernels.knife_free, rounded to the storage type (the pairs stay pairs), with plane (0, 0) all zero: every other plane is a
    permutation of its own of +v / -v pairs, |v| in [lo, hi] (odd size: plus 1, 1.5, -2.5), so its mean is ~0 and no |xhat| is below 0.1"""
    n, c, h, w = shape
    rng = np.random.default_rng(seed)
    m = h * w
    v = store(rng.uniform(lo, hi, size=(n, c, (m - 3) // 2 if m % 2 else m // 2)), dtype).float().numpy()
    vals = np.concatenate([v, -v] + ([np.broadcast_to(np.array([1.0, 1.5, -2.5], dtype=F32), (n, c, 3))] if m % 2 else []), -1)
    out = rng.permuted(vals, axis=-1)
    if zero_plane:
        out[0, 0] = 0.0
    return out.reshape(shape).astype(F64)


def gauss(shape, seed, dtype):
    """N(0, 1) rounded to the storage type, float64 numpy"""
    return stored_np(np.random.default_rng(seed).standard_normal(shape), dtype)


def stats_of(x):
    """fp32 [N, C, 2] sums of a stored tensor (exact sums, rounded once)"""
    return np.stack((x.sum((2, 3)), (x * x).sum((2, 3))), -1).astype(F32)


# ---- case tables -------------------------------------------------------------------------------------------------------------------------------
# A case: entry point and arguments; `kernel` is what route() says it runs (filled in by case()), `why` the reason it is in its table.
Case = namedtuple("Case", "entry dtype N H W C pool norm slope drop stats_out use_x rstats mode inv kernel why")


def case(entry, dtype, N, H, W, C, pool=0, norm=False, slope=1.0, drop=0.0, stats_out=False, use_x=True, rstats=False, mode=0, inv=False, why=""):
    r = route(entry, dtype, N, H, W, C, pool, norm, slope, drop, stats_out, use_x, rstats, mode, inv)
    return Case(entry, dtype, N, H, W, C, pool, norm, slope, drop, stats_out, use_x, rstats, mode, inv, r.kernel, why)


def route_of(c):
    return route(c.entry, c.dtype, c.N, c.H, c.W, c.C, c.pool, c.norm, c.slope, c.drop, c.stats_out, c.use_x, c.rstats, c.mode, c.inv)


def case_bytes(c):
    """bytes of the case's device tensors: input, output / gradient, dx, and res of a norm-add, at pitch C"""
    es = 2 if c.dtype == BF16 else 4
    Ho, Wo = out_len(c.H, c.pool), out_len(c.W, c.pool)
    return es * c.N * c.C * (3 * c.H * c.W if c.entry == "nadd" else 2 * c.H * c.W + Ho * Wo)


def exact_routes(dtype, N, H, W, C, drop=0.0, inv=False, why=""):
    """every forward and backward route of the exact tier at one shape: pool 2 / 1 / 0 forward with and without statistics at slope 1 and 0.25,
    mode 0 backward of every pool with and without x, with and without the bias sums"""
    out = []
    for slope in (1.0, 0.25):
        for pool in (2, 1, 0):
            for so in (False, True):
                out.append(case("fwd", dtype, N, H, W, C, pool, False, slope, drop, so, inv=inv, why=why))
    for pool in (0, 1, 2):
        for use_x in (True, False):
            for rs in (False, True):
                out.append(case("bwd", dtype, N, H, W, C, pool, False, 0.25 if use_x else 1.0, drop, False, use_x, rs, 0, inv, why))
    return out


GEO_H = tuple(range(3, 21)) + (31, 32, 33)
GEO_W = (3, 4, 5, 6, 7, 8, 31, 32, 33, 34, 35, 63, 64, 65)
GEO_SHAPES = tuple((h, w) for h in GEO_H for w in GEO_W)
# the thinned subset at the tiled width: all of H, W <= 5, and the tile edges 8, 16, 32 +- 1 in one dimension at a time and in both
_EDGE = (7, 8, 9, 15, 16, 17, 31, 32, 33)
GEO_SHAPES_TILED = tuple(sorted({(h, w) for h in (3, 4, 5) for w in (3, 4, 5)} | {(h, 5) for h in _EDGE} | {(5, w) for w in _EDGE} |
                                {(4, 33), (33, 4), (3, 32), (32, 3)} | {(h, w) for h in (7, 9, 15, 17) for w in (31, 33)} | {(16, 32), (8, 32), (17, 65), (33, 64)}))
PITCH_SHAPES = ((5, 7), (17, 33))
PITCH_FORMS = ((1, 0), (2, 1), (3, 2))                            # (pitch / C, channel offset / C): alone; the upper half of 2C; the last third of 3C


def signs_cases(dtype, shapes, why):
    """tfc_act_bwd_signs (bf16, 64 channels), with and without the bias sums"""
    return [case("signs", dtype, 2, H, W, 64, 2, False, 0.25, rstats=rs, why=why) for H, W in shapes for rs in (False, True)] if dtype == BF16 else []


def geometry_cases(dtype, tiled):
    C = tiled_c(dtype) if tiled else cheap_c(dtype)
    out = []
    for H, W in (GEO_SHAPES_TILED if tiled else GEO_SHAPES):
        out += exact_routes(dtype, 2, H, W, C, why=f"geometry {H}x{W}")
        if tiled:
            out += signs_cases(dtype, ((H, W),), f"geometry {H}x{W}")
    return out


def width_cases(dtype, widths=None):
    return [c for C in (widths or legal_widths(dtype)) for H, W in PITCH_SHAPES for c in exact_routes(dtype, 2, H, W, C, why=f"width {C}")]


def drop_widths(dtype):
    """one channel vector; the tiled kernels' slice; two 64-channel slices of the tiled backward (blockIdx.z = 1 adds its offset to the index)"""
    return (cheap_c(dtype), tiled_c(dtype), 128)


def dropout_cases(dtype):
    return [c for C in drop_widths(dtype) for H, W in PITCH_SHAPES for c in exact_routes(dtype, 2, H, W, C, 0.5, why="dropout index")]


NORM_PARAMS = ((2, 0.2, 0.0), (2, 0.2, 0.5), (0, 0.0, 0.5), (0, 0.2, 0.0), (1, 0.2, 0.0))   # (pool, slope, drop)
NORM_SHAPES = ((3, 3), (4, 5), (7, 7), (17, 33))


def norm_widths(dtype):
    return (8, 64, 512) if dtype == BF16 else (4, 32, 256)


def norm_cases(dtype):
    """InstanceNorm tier: forward with statistics out, modes 1 and 2 (tiled at pool 2, generic otherwise), and norm-add"""
    out = []
    for C in norm_widths(dtype):
        for H, W in NORM_SHAPES:
            for pool, slope, drop in NORM_PARAMS:
                kw = dict(pool=pool, norm=True, slope=slope, drop=drop, why="instance norm")
                out.append(case("fwd", dtype, 2, H, W, C, stats_out=True, **kw))
                out.append(case("fwd", dtype, 2, H, W, C, stats_out=False, **kw))
                out.append(case("bwd", dtype, 2, H, W, C, mode=1, rstats=True, **kw))
                out.append(case("bwd", dtype, 2, H, W, C, mode=2, rstats=True, **kw))
            out.append(case("nadd", dtype, 2, H, W, C, norm=True, why="instance norm"))
    return out


def slope02_cases(dtype):
    """slope 0.2 without normalisation (bound tier: 9/64 x 0.2f rounds), every forward kernel and mode 0 on both backward families"""
    out = []
    for H, W in PITCH_SHAPES:
        C = tiled_c(dtype)
        for pool in (2, 1, 0):
            for so in (False, True):
                out.append(case("fwd", dtype, 2, H, W, C, pool, False, 0.2, 0.0, so, why="slope 0.2"))
            out.append(case("bwd", dtype, 2, H, W, C, pool, False, 0.2, 0.0, False, True, True, 0, why="slope 0.2"))
    return out


def _cap_search(entry, dtype, inv, N, **kw):
    """the smallest plane (H <= W), at the widest C whose partial sums fit part_ws, for which route() says nb == cap, more than one trip, and a
    ragged last one"""
    for C in reversed(legal_widths(dtype)):
        for H, W in sorted(((h, w) for h in range(3, 48) for w in range(h, 48)), key=lambda s: (s[0] * s[1], s[1] - s[0])):
            r = route(entry, dtype, N, H, W, C, inv=inv, **kw)
            if r.kernel == REFUSED:
                break
            if r.grid[0] == act_grid_cap(N, inv) and r.trips > 1 and r.ragged:
                return case(entry, dtype, N, H, W, C, inv=inv, why="grid cap", **kw)
    raise AssertionError("no capped shape")


CAP_ROUTES = (("fwd", dict(pool=0, slope=0.25, stats_out=True)), ("fwd", dict(pool=0, slope=0.25)), ("fwd", dict(pool=2, slope=0.25)),
              ("bwd", dict(pool=0, slope=0.25, mode=0, rstats=True)), ("bwd", dict(pool=0, norm=True, slope=0.2, mode=1, rstats=True)),
              ("nadd", dict(norm=True)))


def cap_cases(dtype, inv, N):
    """one case per generic kernel past act_grid's cap. Plain mode: N = 64, cap 64. Batch-invariant mode: cap 4096 / 32 = 128 at any N.
    tfc_act_pool2_fwd_kernel strides over 2 x 2 output blocks: past the cap its input is N C 16 nob > 16 x 4096 x 256 x ue elements (268 MB) in
    plain mode, so it is capped in batch-invariant mode only."""
    return [_cap_search(e, dtype, inv, N, **kw) for e, kw in CAP_ROUTES if not (e == "fwd" and kw.get("pool") == 2 and not inv)]


def all_cases():
    out = []
    for dtype in DTYPES:
        out += geometry_cases(dtype, False) + geometry_cases(dtype, True) + width_cases(dtype) + dropout_cases(dtype)
        out += norm_cases(dtype) + slope02_cases(dtype) + cap_cases(dtype, False, 64) + cap_cases(dtype, True, 1) + cap_cases(dtype, True, 2)
    return out


# ---- a case's inputs and references ------------------------------------------------------------------------------------------------------------
SEED = 20             # dropout seed of every case
PREFILL = 3.0         # what stats_out / rstats hold before the call: the reductions add to it


def is_exact(c):
    """exact tier: no normalisation, dyadic slope, ternary data"""
    return not c.norm and c.slope in SLOPES_EXACT


def quantum(c):
    """the exact tier's results are multiples of 1 / quantum: taps / 64, slope 1/4, dropout x 2"""
    return 256 if c.slope == 0.25 else 64


def inputs_of(c):
    """case_inputs, shared between the cases that differ only in what they ask of the same tensors"""
    return _inputs(c._replace(kernel="", why="", stats_out=False, rstats=False, use_x=True, inv=False))


@functools.lru_cache(maxsize=16)
def _inputs(c):
    return case_inputs(c)


def case_inputs(c):
    """float64 numpy NCHW tensors holding storage-type values, the fp32 statistics, and the keep mask of the case"""
    Ho, Wo = out_len(c.H, c.pool), out_len(c.W, c.pool)
    xs, ys = (c.N, c.C, c.H, c.W), (c.N, c.C, Ho, Wo)
    key = c.H * 1000 + c.W + 7 * c.C
    d = {"keep": keep_mask(SEED, c.N, Ho, Wo, c.C, c.drop) if c.drop else None}
    if is_exact(c):
        d["x"], d["dy"] = ternary(xs, key), ternary(ys, key + 1)
    else:
        d["x"], d["dy"] = knife_free(xs, key, c.dtype, zero_plane=c.norm), gauss(ys, key + 1, c.dtype)
    d["stats"] = stats_of(d["x"]) if c.norm else None
    if c.entry == "nadd":
        d["res"] = gauss(xs, key + 2, c.dtype)
    if c.mode == 2:
        d["rstats"] = case_reference(c._replace(mode=1), d, F64)["rstats"].astype(F32)
    return d


def case_reference(c, d, wd=F64, mutant=None):
    """name -> numpy of dtype wd, before storage rounding: y (forward, norm-add); stats (exact tier, of the stored y, on top of PREFILL);
    dx and bias (mode 0; bias on top of PREFILL); rstats (mode 1, on top of zero); dx (mode 2)"""
    keep = d["keep"]
    if mutant in ("drop_npix_in", "drop_no_slice_offset") and c.drop:
        keep = keep_mask(SEED, c.N, out_len(c.H, c.pool), out_len(c.W, c.pool), c.C, c.drop, mutant, c.H * c.W)
    if c.entry == "nadd":
        return {"y": norm_add_ref(d["x"], d["res"], d["stats"], wd)}
    if c.entry == "fwd":
        out = {"y": act_fwd_ref(d["x"], d["stats"], c.slope, c.pool, keep, c.drop, wd, mutant)}
        if c.stats_out and is_exact(c):
            out["stats"] = stored_stats(stored_np(out["y"], c.dtype), wd, mutant) + wd(PREFILL)
        return out
    x = d["x"] if c.use_x else None
    r = act_bwd_ref(c.mode, d["dy"], x, d["stats"], c.slope, c.pool, (c.H, c.W), keep, c.drop, d.get("rstats"), wd, mutant)
    if c.mode == 0:
        return {"dx": r[0], "bias": r[1] + wd(PREFILL)} if c.rstats else {"dx": r[0]}
    return {"rstats": r} if c.mode == 1 else {"dx": r}


def is_tensor(name):
    """outputs in the storage type (the sums are fp32)"""
    return name in ("y", "dx")


def assert_exact_sums(terms, what):
    """plane sums of `terms` [N, C, H, W] are exact in fp32 in ANY order: every term is a multiple of 2^-k (k found here, at most 24) and
    the sum of |terms| of a plane stays below 2^24 such quanta, so no partial sum of any subset rounds"""
    t = np.asarray(terms, dtype=F64)
    k = next((k for k in range(25) if np.array_equal(t * 2.0 ** k, np.round(t * 2.0 ** k))), None)
    assert k is not None, f"{what}: terms are no multiples of 2^-24"
    assert np.abs(t).sum((2, 3)).max() * 2.0 ** k < (1 << 24), f"{what}: a plane's sum of |terms| reaches 2^24 quanta of 2^-{k}"


def exact_want(c, ref64):
    """the exact tier's expectation: the reference asserted exact (elements: multiples of 1 / quantum; sums: assert_exact_sums on their terms,
    on top of the integer PREFILL), rounded once to the storage type"""
    want = {}
    for k, v in ref64.items():
        if k == "stats":
            y = stored_np(ref64["y"], c.dtype)
            assert_exact_sums(y, f"{c.kernel} sum")
            assert_exact_sums(y * y, f"{c.kernel} sum of squares")
        elif k == "bias":
            assert_exact_sums(ref64["dx"], f"{c.kernel} bias")
        else:
            assert_exact_ref(v, quantum(c), f"{c.kernel} {k}")
        want[k] = store(v, c.dtype if is_tensor(k) else FP32)
        assert np.array_equal(want[k].to(torch.float64).numpy(), v) or (is_tensor(k) and c.dtype == BF16), f"{c.kernel} {k}: not exact in fp32"
    return want


def rejects(c, d, mutant):
    """whether the comparison of the GPU test fails a result computed by the mutant restatement (in float64, stored like a kernel's result)"""
    ref64 = case_reference(c, d, F64)
    bad = case_reference(c, d, F64, mutant)
    if is_exact(c):
        want = exact_want(c, ref64)
        return any(not same_bits(store(bad[k], c.dtype if is_tensor(k) else FP32), want[k]) for k in want)
    ref32 = case_reference(c, d, F32)
    for k in ref64:
        bf = is_tensor(k) and c.dtype == BF16
        got = store(bad[k], c.dtype if is_tensor(k) else FP32).to(torch.float64).numpy()
        if bound_ratio(got, ref64[k], e32_of(ref32[k], ref64[k]), bf) > 1.0:
            return True
    return False
