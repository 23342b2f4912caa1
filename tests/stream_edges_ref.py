"""fp64 restatements and input builders shared by tests/test_gpu_51_stream_edges.py (against the kernels) and tests/test_stream_edges_host.py
(against torch and numpy, on the CPU): the small streaming kernels of csrc/elementwise.hip below the activation section (Adam, axpby, the casts,
the dropout-mask export, the bias-gradient sums, the spectral-norm backward, the PatchGAN head) and the scalar heads of csrc/losses.hip that go
through tfc_block_commit (L1 sum, relativistic BCE).

Every size list sits on either side of a grid cap, and the caps are restated here from the launchers (csrc/elementwise.hip, csrc/losses.hip:
tfc_launch_*), not from a document. Data of one family is ONE seeded array; a case of n elements takes its first n. An error term that is measured
(reference in fp32 against reference in fp64) is taken over that whole array with the case's own n in the formula: the error of a single number can
fall within 1e-3 ulp of zero by chance and is no bound, so a case of one element is held to the same per-element figure as the largest one.
No import side effects, no GPU."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import conv_exact as X

F32 = np.float32
EPS24, EPS23, EPS22, EPS8 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -22, 2.0 ** -8

# ---- caps, as the launchers state them ---------------------------------------------------------------------------------------------------------
FLAT_CAP = 4096 * 256                                             # tfc_launch_adam / axpby / dropout_mask / cast: nb <= 4096 workgroups of 256
FLAT_SIZES = (1, 255, 257, FLAT_CAP, FLAT_CAP + 1, 2 * FLAT_CAP + 3)   # the last: two full trips and a third of three elements
L1_CAP = 512 * 256                                                # tfc_launch_l1_sum
L1_SIZES = (1, 255, L1_CAP, L1_CAP + 1, 3 * L1_CAP + 37)
BCE_CAP = 256 * 256                                               # tfc_launch_bce_rel
BCE_SIZES = (1, 257, BCE_CAP, BCE_CAP + 1, 2 * BCE_CAP + 5)
TANH_CAP = 1024 * 256                                             # tfc_launch_tanh_bwd_pack: pixels per trip
TANH_SHAPES = ((1, 1, 1), (1, 15, 17), (2, 16, 24), (1, 512, 513))   # the last: 262 656 pixels = one trip of 1024 slots + 512 pixels of a second
SN_PARTS, SN_PER_PART = 128, 1024                                 # tfc_launch_sn_bwd: nb = ceil(n / 1024) <= TFC_SN_BWD_PARTS (csrc/tfc_desc.h)
SN_SHAPES = ((1, 1), (3, 5), (128, 1024), (130, 1031), (64, 8192 + 1))
HEAD_CAP_PIXELS = 512 * 4                                         # tfc_launch_head_fwd: TFC_HEAD_NB workgroups, one pixel per wave
HEAD_SHAPES = ((1, 1, 1), (1, 3, 5), (3, 27, 27))                 # the last: 2187 pixels, 139 of them in a second trip
HEAD_CASES = ((torch.float32, 64), (torch.float32, 512), (torch.bfloat16, 64), (torch.bfloat16, 512), (torch.bfloat16, 1024))
COLSUM_ROWS_ONE = (1, 31, 32, 33, 4095)                           # one workgroup row (part_ws not given): 32 row-lanes, ragged on both sides
COLSUM_ROWS_SPLIT = (4096, 4097, 5 * 1024 + 1, 8192 + 33)         # rows >= 4096 with part_ws: ny = 4, 5, 6, 9 slots for a reducer of 8 lanes
COLSUM_C = {torch.bfloat16: (8, 24, 72, 512), torch.float32: (4, 12, 36, 512)}   # C / ue = 1, 3, 9, 64 (fp32: 128): 3 and 9 leave lanes of the 8 idle
COLSUM_SENTINEL = 2.0 ** 20                                       # around the summed window; one leaked element moves a sum by more than any sum


def ue_of(dtype):
    """elements per 16-byte unit"""
    return 8 if dtype == torch.bfloat16 else 4


def flat_grid(n, cap_blocks=4096):
    """(workgroups, trips of the longest thread) of a capped grid-stride launch over n elements"""
    nb = min((n + 255) // 256, cap_blocks)
    return nb, -(-n // (nb * 256))


def colsum_ny(rows, C, dtype, part_floats, with_part=True):
    """tfc_launch_colsum's row split, restated: the number of partial slots (1 = the single-workgroup-row route)"""
    nbx = (C // ue_of(dtype) + 7) // 8
    ny = 1
    if with_part and rows >= 4096:
        ny = min((rows + 1023) // 1024, max(2048 // nbx, 1))
        if ny * C > part_floats:
            ny = 1
    return ny


def head_uses_lds(dtype, C):
    """tfc_head_fwd_kernel keeps the filter in registers while a pixel is at most 64 16-byte units wide, and transposed in LDS beyond"""
    return C // ue_of(dtype) > 64


# ---- casts -------------------------------------------------------------------------------------------------------------------------------------
# fp32 bit patterns whose bf16 rounding is decided at an edge: exact ties to an even and to an odd upper half, both signs; +-0; +-inf; the quiet
# NaN; the largest finite fp32 (rounds to inf); denormals (the smallest, a tie to zero, a tie away from it, the largest: rounds to the smallest normal)
CAST_SPECIALS = (0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F7FFFFF,
                 0xFF7FFFFF, 0x00000001, 0x00008000, 0x00018000, 0x80018000, 0x00400000, 0x007FFFFF, 0x3F807FFF, 0x3F808001)


def bits_f32(patterns):
    return torch.from_numpy(np.asarray(patterns, dtype=np.uint32).view(np.float32).copy())


def cast_f32_data(n, seed=7):
    """n fp32 values ~ N(0, 1) x 2^k (k in -20..20), with CAST_SPECIALS at the front and again at the very end (the ragged last trip)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * torch.pow(2.0, torch.randint(-20, 21, (n,), generator=g).float())
    s = bits_f32(CAST_SPECIALS)
    k = min(n, len(s))
    x[:k] = s[:k]
    if n >= 2 * len(s):
        x[n - len(s):] = s
    return x


def cast_bf16_data(n):
    """n bf16 values walking all 65 536 bit patterns (NaNs and denormals included): widening to fp32 is a shift and exact for every one"""
    bits = (np.arange(n, dtype=np.int64) * 40503 + 0x3F81) % 65536
    return torch.from_numpy(bits.astype(np.uint16).view(np.int16).copy()).view(torch.bfloat16)


def bf16_rne_bits(x):
    """fp32 tensor -> int32 tensor of bf16 bit patterns, round-to-nearest-even on the integer representation (NaN -> the quiet NaN): the model
    that torch's own conversion is held against on the host"""
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return torch.where(nan, torch.full_like(r, 0x7FC0), r).to(torch.int32)


def bits16(t):
    """a bf16 tensor's bit patterns as int32 in 0..65535 (torch.equal on them distinguishes -0 from +0 and compares NaNs)"""
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def bits32(t):
    return t.contiguous().view(torch.int32)


def same_floats(got, want):
    """torch.equal on the bit patterns (so -0 is not +0), except that a NaN matches any NaN: torch's own fp32 -> bf16 conversion writes 0xFFFF
    or 0x7FC0 for the same NaN depending on whether its vector or its scalar path converts the element"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    bits = bits16 if got.dtype == torch.bfloat16 else bits32
    gn, wn = torch.isnan(got), torch.isnan(want)
    return torch.equal(gn, wn) and torch.equal(bits(got)[~gn], bits(want)[~wn])


# ---- axpby -------------------------------------------------------------------------------------------------------------------------------------
AXPBY_AB = ((0.3, -1.7), (-2.5, 0.0625))                          # general coefficients (rounded to fp32 by the entry point)
AXPBY_AB_EXACT = ((0.5, -2.0), (4.0, 0.25))                       # powers of two on integer data: every product and the sum are exact


def axpby_data(n, seed=11, exact=False):
    g = torch.Generator().manual_seed(seed)
    if exact:
        return torch.randint(-64, 65, (n,), generator=g).float() * 4, torch.randint(-64, 65, (n,), generator=g).float() * 4
    return torch.randn(n, generator=g), torch.randn(n, generator=g) * 3


def axpby_ref(x, y, a, b):
    """fp64 a x + b y with a, b as the entry point receives them (floats) -> (reference, bound per element = 2^-23 (|a x| + |b y|): at most two
    roundings whether or not the compiler contracts the expression into an fma)"""
    a, b = float(F32(a)), float(F32(b))
    ax = a * x.double()
    by = b * y.double() if y is not None else torch.zeros_like(ax)
    return ax + by, EPS23 * (ax.abs() + by.abs())


# ---- dropout mask ------------------------------------------------------------------------------------------------------------------------------
DROP_P = (0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24)                 # thresholds 0 (keep all), 1, 2^23, 2^24 - 1 on the hash's top 24 bits
DROP_SEEDS = (12345, 0x9E3779B1)                                  # the second is >= 2^31


# ---- Adam --------------------------------------------------------------------------------------------------------------------------------------
ADAM_HP = dict(lr=2e-4, b1=0.5, b2=0.999, eps=1e-8)               # the training step's (engine.py); 1 - b is exact in fp32 for b in [0.5, 1]
ADAM_STEPS = (1, 2, 1000)
ADAM_GSCALES = (1.0, 0.5)


def adam_blocks(n):
    """(slice with g = 0, slice with v = 0 and g = 0): the second makes the denominator eps alone. Both lie in the first sixteenth-wide blocks
    behind n / 8 and n / 4, so they exist from n = 255 on and never reach the second trip of the large sizes"""
    w = n // 16
    return slice(n // 8, n // 8 + w), slice(n // 4, n // 4 + w)


_ADAM_DRAW = {}


def adam_state(n, seed=21):
    """p ~ 0.02 N(0,1), m ~ 1e-3 N(0,1), v ~ 1e-6 chi^2(1), g ~ 1e-3 N(0,1) as fp32 numpy arrays: the first n of ONE draw of FLAT_SIZES[-1], plus
    the two zero blocks of adam_blocks(n)"""
    if seed not in _ADAM_DRAW:
        g_, nmax = torch.Generator().manual_seed(seed), FLAT_SIZES[-1]
        _ADAM_DRAW[seed] = ((0.02 * torch.randn(nmax, generator=g_)).numpy(), (1e-3 * torch.randn(nmax, generator=g_)).numpy(),
                            (1e-6 * torch.randn(nmax, generator=g_) ** 2).numpy(), (1e-3 * torch.randn(nmax, generator=g_)).numpy())
    p, m, v, g = (t[:n].copy() for t in _ADAM_DRAW[seed])
    g0, v0 = adam_blocks(n)
    g[g0] = 0
    g[v0] = 0
    v[v0] = 0
    return p, m, v, g


def adam_ref(p, m, v, g, step, gscale, lr, b1, b2, eps):
    """one Adam step in fp64 from fp32 state, the hyper-parameters rounded to fp32 first (the entry point takes floats: that is the operation it
    defines), bias corrections 1 - b^step in fp64 -> dict of p, m, v (new), delta (the update) and the m / v bounds 2^-22 (|b x| + |(1 - b) y|)"""
    lr, b1, b2, eps, gs = (float(F32(t)) for t in (lr, b1, b2, eps, gscale))
    p, m, v, g = (np.asarray(t, dtype=np.float64) for t in (p, m, v, g))
    gi = g * gs
    m1, m2 = b1 * m, (1 - b1) * gi
    v1, v2 = b2 * v, (1 - b2) * gi * gi
    mn, vn = m1 + m2, v1 + v2
    delta = (lr / (1 - b1 ** step)) * (mn / (np.sqrt(vn) / np.sqrt(1 - b2 ** step) + eps))
    return dict(p=p - delta, m=mn, v=vn, delta=delta, m_bound=EPS22 * (np.abs(m1) + np.abs(m2)), v_bound=EPS22 * (np.abs(v1) + np.abs(v2)))


def adam_f32(p, m, v, g, step, gscale, lr, b1, b2, eps):
    """the same step in plain fp32 numpy, every operation rounded, the bias corrections as tfc_adam_step forms them (1 - powf(b, step), sqrtf).
    NOT a bit model of the kernel (hipcc contracts a * b + c into an fma): it measures what fp32 arithmetic costs this formula."""
    lr, b1, b2, eps, gs, one = (F32(t) for t in (lr, b1, b2, eps, gscale, 1.0))
    bc1 = one - np.power(b1, F32(step), dtype=F32)
    bc2s = np.sqrt(one - np.power(b2, F32(step), dtype=F32), dtype=F32)
    gi = g * gs
    mn = b1 * m + (one - b1) * gi
    vn = b2 * v + (one - b2) * gi * gi
    delta = (lr / bc1) * (mn / (np.sqrt(vn) / bc2s + eps))
    assert mn.dtype == F32 and vn.dtype == F32 and delta.dtype == F32
    return dict(p=p - delta, m=mn, v=vn, delta=delta)


def adam_c(ref, f32):
    """c of the p bound: 8 x the largest relative error of the fp32 restatement's update against fp64 (over the elements with a non-zero update)"""
    nz = ref["delta"] != 0
    return 8 * float(np.max(np.abs(f32["delta"][nz].astype(np.float64) - ref["delta"][nz]) / np.abs(ref["delta"][nz])))


def adam_p_bound(ref, c):
    return EPS24 * np.abs(ref["p"]) + c * np.abs(ref["delta"])


# ---- bias sums: ternary integers, exact in any order -------------------------------------------------------------------------------------------
def ternary(shape, seed):
    """conv_exact.ints with amp 1: float64 integers in {-1, 0, 1}"""
    return X.ints(shape, seed)


def colsum_buffer(data, rows, C, dtype, wide):
    """rows x C of `data` (float64 [>= rows, >= C]) in storage dtype, alone (pitch C, offset 0) or as channels [8, 8 + C) of a [rows, C + 16]
    buffer whose other channels hold COLSUM_SENTINEL -> (buffer, channel offset, pitch)"""
    if not wide:
        return data[:rows, :C].to(dtype).contiguous(), 0, C
    t = torch.full((rows, C + 16), COLSUM_SENTINEL, dtype=dtype)
    t[:, 8:8 + C] = data[:rows, :C].to(dtype)
    return t, 8, C + 16


def colsum_prefill(C):
    """a non-zero integer vector: the contract is out += sum"""
    return ((torch.arange(C) % 7) - 3).float() * 5 + 1


def tanh_case(N, C, H, W, seed):
    """g in multiples of 4 from -8 to 8 and y in {0, +-0.5} (NCHW fp32): g (1 - y^2) is an integer in -8..8, exact in fp32 and in bf16, and so is
    every partial sum of it (|sum| <= 8 x 262 656 < 2^24) -> (g, y, want [N, C, H, W] float64)"""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randint(-2, 3, (N, C, H, W), generator=gen).float() * 4
    y = torch.randint(-1, 2, (N, C, H, W), generator=gen).float() * 0.5
    return g, y, g.double() * (1 - y.double() ** 2)


def l1_case(n, seed=31):
    """a, b ternary fp32 and sum |a - b| as a float64 integer (<= 2 n < 2^24 / 4 for every size: exact whatever order the atomics arrive in)"""
    a, b = ternary((n,), seed), ternary((n,), seed + 1)
    return a.float(), b.float(), (a - b).abs().sum()


# ---- relativistic BCE --------------------------------------------------------------------------------------------------------------------------
BCE_T1, BCE_T2 = 0.9, 0.0
BCE_GSCALES = (1.0, 0.25)


def bce_logits(dtype, seed=41):
    """the family's logit pair (a, b), 2 x 65 536 + 5 values in storage dtype: a, b ~ U(-15, 15) so that a - b covers [-30, 30]; among the first
    257 an exact 0 (a = b) and a - b = +-90, where expf(-|x|) underflows below the smallest normal float inside log1pf and the sigmoid
    saturates. 45 is a bf16 value."""
    n = BCE_SIZES[-1]
    g = torch.Generator().manual_seed(seed)
    a, b = (torch.rand(n, generator=g) * 30 - 15).to(dtype), (torch.rand(n, generator=g) * 30 - 15).to(dtype)
    for i in (5, 100, 70000):
        b[i] = a[i]
    for i, s in ((6, 1.0), (101, 1.0), (7, -1.0), (102, -1.0), (70001, 1.0), (70002, -1.0)):
        a[i], b[i] = 45.0 * s, -45.0 * s
    return a, b


def bce_terms(x, mode, t1, t2):
    """per-logit loss and d loss / d x (before the 1 / n of the mean) of the relativistic BCE in x's dtype, t1 / t2 as the entry point gets them:
    mode 0: BCE(x, t1); mode 1: 0.5 (BCE(x, t1) + BCE(-x, t2))"""
    t1, t2 = float(F32(t1)), float(F32(t2))
    l = F.binary_cross_entropy_with_logits(x, torch.full_like(x, t1), reduction="none")
    gx = torch.sigmoid(x) - t1
    if mode == 1:
        l = 0.5 * (l + F.binary_cross_entropy_with_logits(-x, torch.full_like(x, t2), reduction="none"))
        gx = 0.5 * (gx - (torch.sigmoid(-x) - t2))
    return l, gx


def bce_ref(a, b, n, mode, gscale, t1=BCE_T1, t2=BCE_T2):
    """fp64 reference on the first n stored logits -> (loss, da [n]); db = -da. With the error terms of torch-CPU fp32 on the WHOLE family at this
    n (see the module docstring): grad_err = max |g32 - g64|, loss_err = max per-logit |l32 - l64| (a mean cannot be further off than its worst
    term; the difference of two means is one random number and bounds nothing)."""
    x64 = a.double() - b.double()
    l64, g64 = bce_terms(x64, mode, t1, t2)
    x32 = a.float() - b.float()
    l32, g32 = bce_terms(x32, mode, t1, t2)
    inv32, gs32 = torch.tensor(1.0 / n, dtype=torch.float32), torch.tensor(gscale, dtype=torch.float32)
    da64 = g64 / n * float(F32(gscale))
    da32 = g32 * inv32 * gs32
    return dict(loss=l64[:n].mean().item(), da=da64[:n], grad_err=(da32.double() - da64).abs().max().item(),
                loss_err=(l32.double() - l64).abs().max().item())


# ---- spectral-norm backward --------------------------------------------------------------------------------------------------------------------
def sn_case(R, K, seed):
    """W ~ 0.05 N(0,1), G ~ N(0,1), u, v random unit vectors. R = K = 1 is dyadic (W = 0.5, G = 3, u = v = 1): the gradient of W / (u W v) G is
    identically zero there and every step of its evaluation exact, so that case asserts zeros, not a tolerance on a single number."""
    if R * K == 1:
        return torch.tensor([[0.5]]), torch.tensor([[3.0]]), torch.ones(1), torch.ones(1)
    g = torch.Generator().manual_seed(seed)
    W, G = 0.05 * torch.randn(R, K, generator=g), torch.randn(R, K, generator=g)
    return W, G, F.normalize(torch.randn(R, generator=g), dim=0), F.normalize(torch.randn(K, generator=g), dim=0)


def sn_grad(W, G, u, v, dtype):
    """autograd of ((W / (u . W v)) G).sum() in `dtype`, as in test_spectral_norm_step_and_backward"""
    Wr = W.to(dtype).clone().requires_grad_(True)
    sig = torch.dot(u.to(dtype), Wr @ v.to(dtype))
    ((Wr / sig) * G.to(dtype)).sum().backward()
    return Wr.grad


def sn_closed_form(W, G, u, v):
    """what tfc_sn_bwd_apply_kernel evaluates, in fp64: (G - (sum G W) / sigma u v^T) / sigma"""
    W, G, u, v = (t.double() for t in (W, G, u, v))
    sig = torch.dot(u, W @ v)
    return (G - ((G * W).sum() / sig) * torch.outer(u, v)) / sig


# ---- PatchGAN head -----------------------------------------------------------------------------------------------------------------------------
def head_case(N, H, W, C, seed):
    """ternary x [N, C, H, W] and w [1, C, 4, 4] (float64) and ZeroPad2d((1, 0, 1, 0)) + Conv2d(k4, p1) of them in fp64: |sum| <= 16 C < 2^24"""
    x, w = ternary((N, C, H, W), seed), ternary((1, C, 4, 4), seed + 1)
    return x, w, X.ref_fwd(X.OP_PADCONV, x, w)
