"""Exact-integer machinery of the batch-32 convolution tests (test_gpu_35_batch32_exact.py on the GPU, test_conv_exact_host.py on the host).

Every operand is a small integer or a dyadic fraction. Then every partial sum a kernel forms is exact in fp32 as long as its magnitude, counted in
units of the data's quantum, stays below 2^24: in any order, under any split-K, on the matrix core or on the VALU. The value a kernel stores is then
exactly the round-to-nearest-even of the true value, which a float64 torch op computes; the comparison is torch.equal, with no tolerance. One bad
tile, one image, one K-slice or one input channel changes at least one element, and the failure report names where.

CASES lists every (network, layer, entry point, pass, H, W, Cin, Cout, flags, view form) that the bf16 TrainStep issues at 256 x 256, plus the
13 LPIPS convolutions. It is written out by hand on purpose: test_conv_exact_host.py derives the same table from the network definitions, and the
GPU inventory test holds it against what a real step records.
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

from tfc_gan_amd import ops
from tfc_gan_amd.ops import OP_CONV, OP_CONV3, OP_CONVT, OP_PADCONV, OP_UPCONV, View

EXACT_BOUND = 1 << 24
BLUR_TAPS = (1, 3, 3, 1)                     # BlurPool filter per dimension, / 8 (oracle BLUR_TAPS): dyadic
TILE_H, TILE_W = 8, 16                       # gather-GEMM output tile (csrc/tfc_desc.h): failure reports group by it
BATCHES = (32, 13)                           # the benchmarked batch, and a prime: every per-image partition has a ragged tail

SLOPE = 0.25                                 # LeakyReLU slope of the exact fused-first-block tests (production: 0.2, tolerance tier)
OSCALE = 0.5                                 # 1 / sigma of the exact discriminator tests
FIRST_BWD_QUANTUM = 256                      # d_raw = slope x (dy x taps / 64): a multiple of 1 / 256
FIRST_BWD_DY_DENSITY = 16                    # one nonzero of dy_pooled per 16 (lattice): keeps the first block's weight gradient under 2^24 / 256

Case = namedtuple("Case", "net layer entry pas op H W Cin Cout flags view")

# view forms
FRESH = "fresh"                              # a buffer of its own, pitch = pad8(C)
WINDOW = "window"                            # the skip half of a concat buffer: pitch 2 C, channel offset C (nets.py cat[..].sub)
WHOLE = "whole"                              # a whole concat buffer read as one tensor (pitch = C)


def _c(net, layer, entry, pas, op, H, Cin, Cout, flags="", view=FRESH):
    return Case(net, layer, entry, pas, op, H, H, Cin, Cout, frozenset(f for f in flags.split(",") if f), view)


CASES = [
    # ---- generator forward ----
    _c("G", "down1", "first_block_fwd", 0, OP_CONV, 256, 3, 64, "gform,signs", WINDOW),
    _c("G", "down2", "conv_fwd", 0, OP_CONV, 128, 64, 128, "stats", WINDOW),
    _c("G", "down3", "conv_fwd", 0, OP_CONV, 64, 128, 256, "stats", WINDOW),
    _c("G", "down4", "conv_fwd", 0, OP_CONV, 32, 256, 512, "stats", WINDOW),
    _c("G", "down5", "conv_fwd", 0, OP_CONV, 16, 512, 512, "", WINDOW),
    _c("G", "down6", "conv_fwd", 0, OP_CONV, 8, 512, 512, "stats", WINDOW),
    _c("G", "up1", "conv_fwd", 0, OP_CONVT, 4, 512, 512),
    _c("G", "up2", "conv_fwd", 0, OP_CONVT, 8, 1024, 512, "", WHOLE),
    _c("G", "up3", "conv_fwd", 0, OP_CONVT, 16, 1024, 256, "", WHOLE),
    _c("G", "up4", "conv_fwd", 0, OP_CONVT, 32, 512, 128, "", WHOLE),
    _c("G", "up5", "conv_fwd", 0, OP_CONVT, 64, 256, 64, "", WHOLE),
    _c("G", "final", "upconv_head_fwd", 0, OP_UPCONV, 128, 128, 3, "bias,tanh", WHOLE),
    # ---- generator backward, in the order nets.py issues it ----
    _c("G", "final", "conv_wgrad", 2, OP_UPCONV, 128, 128, 3, "", WHOLE),
    _c("G", "final", "upconv_head_dgrad", 1, OP_UPCONV, 128, 128, 3, "", WHOLE),
    _c("G", "up5", "conv_wgrad", 2, OP_CONVT, 64, 256, 64, "", WHOLE),
    _c("G", "up5", "conv_dgrad", 1, OP_CONVT, 64, 256, 64, "", WHOLE),
    _c("G", "up4", "conv_wgrad", 2, OP_CONVT, 32, 512, 128, "", WHOLE),
    _c("G", "up4", "conv_dgrad", 1, OP_CONVT, 32, 512, 128, "", WHOLE),
    _c("G", "up3", "conv_wgrad", 2, OP_CONVT, 16, 1024, 256, "", WHOLE),
    _c("G", "up3", "conv_dgrad", 1, OP_CONVT, 16, 1024, 256, "", WHOLE),
    _c("G", "up2", "conv_wgrad", 2, OP_CONVT, 8, 1024, 512, "", WHOLE),
    _c("G", "up2", "conv_dgrad", 1, OP_CONVT, 8, 1024, 512, "", WHOLE),
    _c("G", "up1", "conv_wgrad", 2, OP_CONVT, 4, 512, 512),
    _c("G", "up1", "conv_dgrad", 1, OP_CONVT, 4, 512, 512),
    _c("G", "down6", "conv_wgrad", 2, OP_CONV, 8, 512, 512, "", WINDOW),
    _c("G", "down6", "conv_dgrad", 1, OP_CONV, 8, 512, 512, "accum", WINDOW),
    _c("G", "down5", "conv_wgrad", 2, OP_CONV, 16, 512, 512, "", WINDOW),
    _c("G", "down5", "conv_dgrad", 1, OP_CONV, 16, 512, 512, "accum", WINDOW),
    _c("G", "down4", "conv_wgrad", 2, OP_CONV, 32, 256, 512, "", WINDOW),
    _c("G", "down4", "conv_dgrad", 1, OP_CONV, 32, 256, 512, "accum", WINDOW),
    _c("G", "down3", "conv_wgrad", 2, OP_CONV, 64, 128, 256, "", WINDOW),
    _c("G", "down3", "conv_dgrad", 1, OP_CONV, 64, 128, 256, "accum", WINDOW),
    _c("G", "down2", "conv_wgrad", 2, OP_CONV, 128, 64, 128, "", WINDOW),
    _c("G", "down2", "conv_dgrad", 1, OP_CONV, 128, 64, 128, "accum", WINDOW),
    _c("G", "down1", "first_block_bwd_wgrad", 2, OP_CONV, 256, 3, 64, "signs", WINDOW),   # dy_pooled: the skip half of up5's concat gradient
    # ---- discriminator forward ----
    _c("D", "model.0", "first_block_fwd", 0, OP_CONV, 256, 6, 64, "bias,oscale,signs"),
    _c("D", "model.3", "conv_fwd", 0, OP_CONV, 128, 64, 128, "bias,oscale,leaky"),
    _c("D", "model.6", "conv_fwd", 0, OP_CONV, 64, 128, 256, "bias,oscale,leaky"),
    _c("D", "model.9", "conv_fwd", 0, OP_CONV, 32, 256, 512, "bias,oscale,leaky"),
    _c("D", "model.13", "patchgan_head_fwd", 0, OP_PADCONV, 16, 512, 1),
    # ---- discriminator backward (input gradients: generator step; weight gradients: discriminator step), in nets.py order ----
    _c("D", "model.13", "conv_wgrad", 2, OP_PADCONV, 16, 512, 1),
    _c("D", "model.13", "conv_dgrad", 1, OP_PADCONV, 16, 512, 1),
    _c("D", "model.9", "conv_wgrad", 2, OP_CONV, 32, 256, 512),
    _c("D", "model.9", "conv_dgrad", 1, OP_CONV, 32, 256, 512, "oscale"),
    _c("D", "model.6", "conv_wgrad", 2, OP_CONV, 64, 128, 256),
    _c("D", "model.6", "conv_dgrad", 1, OP_CONV, 64, 128, 256, "oscale"),
    _c("D", "model.3", "conv_wgrad", 2, OP_CONV, 128, 64, 128),
    _c("D", "model.3", "conv_dgrad", 1, OP_CONV, 128, 64, 128, "oscale"),
    _c("D", "model.0", "conv_dgrad_image", 1, OP_CONV, 256, 6, 64, "oscale"),
    _c("D", "model.0", "first_block_bwd_wgrad", 2, OP_CONV, 256, 6, 64, "signs,bias_sums"),
]
# the 13 VGG16 convolutions of LPIPS (3 x 3 in a 4 x 4 slot, bias + ReLU; the image is padded to 32 bf16 channels): forward and input gradient
LPIPS_LAYERS = [(256, 32, 64), (256, 64, 64), (128, 64, 128), (128, 128, 128), (64, 128, 256), (64, 256, 256), (64, 256, 256),
                (32, 256, 512), (32, 512, 512), (32, 512, 512), (16, 512, 512), (16, 512, 512), (16, 512, 512)]
for _i, (_h, _ci, _co) in enumerate(LPIPS_LAYERS):
    CASES.append(_c("LPIPS", f"conv{_i}", "conv_fwd", 0, OP_CONV3, _h, _ci, _co, "bias,relu"))
    CASES.append(_c("LPIPS", f"conv{_i}", "conv_dgrad", 1, OP_CONV3, _h, _ci, _co))

# the weight-gradient calls of one step in the order nets.py issues them: G's through one workspace, then D's
WGRAD_ENGINE_ORDER = [c for c in CASES if c.entry in ("conv_wgrad", "first_block_bwd_wgrad")]


def fp32_cases(pas):
    """the same layers as the fp32 parity mode runs them: every convolution through the gather GEMM (the first-layer, head and fused-block entry
    points are bf16 only), inputs in buffers of their own for the first layers (the 8-channel packed image)"""
    plain = {0: ("conv_fwd", "first_block_fwd"), 1: ("conv_dgrad", "upconv_head_dgrad", "conv_dgrad_image"),
             2: ("conv_wgrad", "first_block_bwd_wgrad")}[pas]
    out = []
    for c in CASES:
        if c.net == "LPIPS" or c.entry not in plain:
            continue
        first = c.Cin <= 8
        out.append(c._replace(entry={0: "conv_fwd", 1: "conv_dgrad", 2: "conv_wgrad"}[pas], view=FRESH if first else c.view,
                              flags=frozenset(f for f in c.flags if f in ("accum", "oscale"))))
    return out


def case_id(c):
    return f"{c.net}-{c.layer}-{c.entry}"


def prof_key(c):
    """(op, pass, H, W, Cin, Cout) as ops.prof_records() records the call; None for an entry point that records nothing"""
    if c.entry == "patchgan_head_fwd":
        return None
    if c.entry == "conv_dgrad_image":
        return (c.op, c.pas, c.H, c.W, 3, c.Cout)            # records the channels it writes: the generated image's 3
    return (c.op, c.pas, c.H, c.W, c.Cin, c.Cout)


def record_key(r):
    """key of one ops.prof_records() record: the finish pass of a weight gradient (pass 3) belongs to its pass-2 call"""
    return (r["op"], 2 if r["pass"] == 3 else r["pass"], r["H"], r["W"], r["Cin"], r["Cout"])


def out_hw(c):
    return ops.OUT_HW[c.op](c.H)


def weight_shape(c):
    return (c.Cin, c.Cout, 4, 4) if c.op == OP_CONVT else (c.Cout, c.Cin, 4, 4)


# ---- value ranges and the 2^24 bound ---------------------------------------------------------------------------------
TAPS = {OP_CONV: 16, OP_PADCONV: 16, OP_CONVT: 4, OP_UPCONV: 16, OP_CONV3: 9}   # forward taps per input channel of one output element
WGRAD_BASE_AMP = 4                           # |dw| an accumulating weight-gradient call starts from


def amplitudes(c):
    """(max |a|, max |b|, density of b, quantum): the pass multiplies integers in [-a, a] by integers in [-b, b] (b nonzero on one lattice point in
    `density`), and every partial sum is a multiple of 1 / quantum"""
    if c.entry == "first_block_bwd_wgrad":
        return 1, 1, FIRST_BWD_DY_DENSITY, FIRST_BWD_QUANTUM
    if c.entry == "first_block_fwd":
        return 1, 1, 1, 2 * 64 * 4                           # bias / 2, blur taps / 64, slope 1/4
    return 1, 1, 1, 2 if ("oscale" in c.flags or "bias" in c.flags) else 1


def worst_partial_sum(c, N):
    """an upper bound of |partial sum| in quanta over every element the pass computes at batch N"""
    a, b, dens, quantum = amplitudes(c)
    OH = out_hw(c)
    if c.entry == "first_block_bwd_wgrad":
        # d_raw = LeakyReLU'(y) x BlurPool^T(dy): the transposed blur keeps the L1 mass of dy (its taps sum to 1, reflection only moves mass), the
        # slope is <= 1. dw sums x d_raw over every pixel of every image, |x| <= a: |dw| <= a x N x (nonzeros of one dy plane) x b; the per-image
        # bias sums are a part of the same
        Po = (c.H - 2) // 2 + 1
        return N * -(-Po * Po // dens) * a * b * quantum
    if c.pas == 0:
        bias = 1 if "bias" in c.flags else 0
        return (ops.pad8(c.Cin) * TAPS[c.op] * a * b + bias) * quantum
    if c.pas == 1:
        # each input element gathers at most 16 taps x Cout (transposed: the 4 x 4 stride-2 dual), + the value an accumulating call adds to (|.| <= 1)
        return (ops.pad8(c.Cout) * 16 * a * b + 1) * quantum
    # wgrad: one filter tap sums over every output pixel of every image (transposed: every input pixel), + the value an accumulating call adds to
    per_tap = c.H * c.W if c.op == OP_CONVT else OH * OH
    return (N * per_tap * a * b + WGRAD_BASE_AMP) * quantum


# ---- integer data ------------------------------------------------------------------------------------------------------
def ints(shape, seed, amp=1, density=1, device="cpu"):
    """float64 integers uniform in [-amp, amp]. density k > 1 (NCHW only): only lattice points, (flat spatial index + 5 n + 3 c) % k == 0, are
    nonzero -- at most ceil(H W / k) per (n, c) plane, which is what worst_partial_sum() counts on"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-amp, amp + 1, tuple(shape), generator=g, dtype=torch.int64).to(torch.float64)
    if density > 1:
        n, c, h, w = shape
        lat = (torch.arange(h * w).view(1, 1, h, w) + 5 * torch.arange(n).view(n, 1, 1, 1) + 3 * torch.arange(c).view(1, c, 1, 1)) % density == 0
        v = v * lat
    return v.to(device)


# ---- float64 references and storage rounding -------------------------------------------------------------------------
def ref_fwd(op, x, w):
    """the convolution of `op` in float64 (NCHW x, torch-layout w; CONV3: the 3 x 3 filter in rows / columns 0..2 of the 4 x 4 slot)"""
    if op == OP_CONV:
        return F.conv2d(x, w, padding=1)
    if op == OP_PADCONV:
        return F.conv2d(F.pad(x, (1, 0, 1, 0)), w, padding=1)
    if op == OP_CONVT:
        return F.conv_transpose2d(x, w, stride=2, padding=1)
    if op == OP_UPCONV:
        return F.conv2d(F.pad(F.interpolate(x, scale_factor=2), (1, 0, 1, 0)), w, padding=1)
    if op == OP_CONV3:
        return F.conv2d(x, w[:, :, :3, :3], padding=1)
    raise ValueError(op)


def ref_dx(op, x_shape, w, dy):
    x = torch.zeros(x_shape, dtype=w.dtype, device=w.device, requires_grad=True)
    (gx,) = torch.autograd.grad(ref_fwd(op, x, w), x, dy)
    return gx.detach()


def ref_dw(op, x, w_shape, dy):
    w = torch.zeros(w_shape, dtype=x.dtype, device=x.device, requires_grad=True)
    (gw,) = torch.autograd.grad(ref_fwd(op, x, w), w, dy)
    return gw.detach()


def blur(x, stride):
    """BlurPool(stride) in float64: reflect pad (1, 2), taps [1, 3, 3, 1] / 8 per dimension"""
    k = torch.tensor(BLUR_TAPS, dtype=x.dtype, device=x.device)
    k2 = torch.outer(k, k) / 64.0
    C = x.shape[1]
    return F.conv2d(F.pad(x, (1, 2, 1, 2), mode="reflect"), k2[None, None].repeat(C, 1, 1, 1), stride=stride, groups=C)


def blur_t(g, shape, stride):
    """BlurPool(stride)^T: the gradient of blur() w.r.t. its input of `shape`"""
    x = torch.zeros(shape, dtype=g.dtype, device=g.device, requires_grad=True)
    (gx,) = torch.autograd.grad(blur(x, stride), x, g)
    return gx.detach()


def assert_dyadic(t, quantum, what):
    """the reference itself is exact: every element a multiple of 1 / quantum, below 2^24 quanta"""
    s = t * quantum
    assert torch.equal(s, s.round()), f"{what}: the float64 reference is not a multiple of 1/{quantum} (non-exact algorithm?)"
    assert s.abs().max().item() < EXACT_BOUND, f"{what}: |reference| reaches 2^24 quanta ({s.abs().max().item():.0f})"


def store(t64, dt):
    """round a float64 value the way the kernel stores it: exact in fp32 (asserted), then round-to-nearest-even to bf16 in bf16 mode"""
    f = t64.to(torch.float32)
    assert torch.equal(f.to(torch.float64), t64), "value not exact in fp32"
    return f.to(torch.bfloat16) if dt == ops.DT_BF16 else f


def leaky_f32(v32, slope):
    """fmaxf(v, slope * v) in fp32, as the epilogues compute it (one fp32 multiply: reproducible at any slope)"""
    return torch.maximum(v32, v32 * torch.tensor(slope, dtype=torch.float32, device=v32.device))


# (layer, C, H, pool, slope) of every pure-blur activation of the step (no statistics in, slope 1/4 in place of 0.2): the up path's pool-1 blur of the
# transposed convolution's output, the discriminator's pool-2 blur of its activated convolution output, and G down5 (not normalised: LeakyReLU + pool 2)
BLUR_ACTS = [("G-up1", 512, 8, 1, 1.0), ("G-up2", 512, 16, 1, 1.0), ("G-up3", 256, 32, 1, 1.0), ("G-up4", 128, 64, 1, 1.0), ("G-up5", 64, 128, 1, 1.0),
             ("D-model.3", 128, 127, 2, 1.0), ("D-model.6", 256, 63, 2, 1.0), ("D-model.9", 512, 31, 2, 1.0), ("G-down5", 512, 15, 2, SLOPE)]


class EngineStatsNorm(torch.autograd.Function):
    """InstanceNorm at the engine's statistics (sum, sum of squares of the stored tensor), the constants derived in fp32 as the kernels derive them
    (m = s1 / HW, var = max(s2 / HW - m^2, 0), rstd = rsqrt(var + eps)); the rest in the input's precision. Backward: the InstanceNorm backward with
    those constants."""

    @staticmethod
    def forward(ctx, x, stats, eps):
        hw = x.shape[2] * x.shape[3]
        inv = torch.tensor(1.0 / hw, dtype=torch.float32, device=stats.device)
        m = (stats[..., 0] * inv)[:, :, None, None]
        r = torch.rsqrt(((stats[..., 1] * inv)[:, :, None, None] - m * m).clamp_min(0.0) + eps)
        xh = (x - m.to(x.dtype)) * r.to(x.dtype)
        ctx.save_for_backward(xh, r.to(x.dtype))
        return xh

    @staticmethod
    def backward(ctx, g):
        xh, r = ctx.saved_tensors
        return r * (g - g.mean(dim=(2, 3), keepdim=True) - xh * (g * xh).mean(dim=(2, 3), keepdim=True)), None, None


def act_ref(x, stats, slope, pool, keep=None, drop_p=0.0):
    """the act_fwd chain in x's precision: InstanceNorm at `stats` -> LeakyReLU(slope) -> BlurPool(pool) -> dropout (keep mask, scale 1 / (1 - p))"""
    y = EngineStatsNorm.apply(x, stats, 1e-5)
    y = torch.where(y > 0, y, y * slope)
    if pool:
        y = blur(y, pool)
    if keep is not None:
        y = y * keep / (1.0 - drop_p)
    return y


# ---- views ---------------------------------------------------------------------------------------------------------------
SENTINEL = 5.0                               # fills everything around a window: a kernel that reads or writes past its window changes a result


def to_view(x64, dt, form=FRESH, fill=0.0):
    """float64 NCHW -> View in storage dtype dt. FRESH / WHOLE: a buffer of its own, channels padded with `fill` to pad8(C) (the engine's padded
    channels are zero). WINDOW: channels [C, 2C) of an [N, H, W, 2C] buffer whose other half holds SENTINEL"""
    N, C, H, W = x64.shape
    if form == WINDOW:
        t = torch.full((N, H, W, 2 * C), SENTINEL, dtype=ops.torch_dtype(dt), device=x64.device)
        t[..., C:] = x64.permute(0, 2, 3, 1).to(t.dtype)
        return View(t, C, C)
    t = torch.full((N, H, W, ops.pad8(C)), fill, dtype=ops.torch_dtype(dt), device=x64.device)
    t[..., :C] = x64.permute(0, 2, 3, 1).to(t.dtype)
    return View(t, C, 0)


def from_view(v, C=None):
    """the View's channels as an NCHW tensor in the storage dtype"""
    C = v.C if C is None else C
    return v.t[..., v.coff:v.coff + C].permute(0, 3, 1, 2)


def outside_window(v, C=None):
    """everything of the View's buffer outside channels [coff, coff + C), for the guard check"""
    C = v.C if C is None else C
    return torch.cat([v.t[..., :v.coff], v.t[..., v.coff + C:]], -1)


def assert_untouched(v, what, C=None, value=SENTINEL):
    rest = outside_window(v, C)
    if rest.numel():
        bad = int((rest.float() != value).sum())
        assert bad == 0, f"{what}: {bad} elements outside the channel window changed"


# ---- the localising exact compare -------------------------------------------------------------------------------------------
ACT_DIMS = (("image", 1), ("64-channel block", 64), ("tile row", TILE_H), ("tile column", TILE_W))
WGT_DIMS = (("64-block of dim 0", 64), ("64-block of dim 1", 64), ("filter row", 1), ("filter column", 1))
VEC_DIMS = (("image", 1), ("64-channel block", 64))


def assert_exact(got, want, what, dims=ACT_DIMS):
    """torch.equal; on a mismatch: how many elements differ and, per group of every dimension (image, 64-channel block, output-tile row and column
    for activations; channel blocks and filter taps for weights), which groups hold them and the first bad coordinate of each"""
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    bad = (got.float() != want.float()) | torch.isnan(got.float())
    idx = bad.nonzero().cpu()
    lines = [f"{what}: {idx.shape[0]} of {got.numel()} elements differ (shape {tuple(got.shape)})"]
    for d, (name, size) in enumerate(dims):
        grp = idx[:, d] // size
        ug, cnt = grp.unique(return_counts=True)
        parts = []
        for g, n in list(zip(ug.tolist(), cnt.tolist()))[:12]:
            first = idx[(grp == g).nonzero()[0, 0]].tolist()
            parts.append(f"{g}: {n} (first {first})")
        more = f" ... and {len(ug) - 12} more" if len(ug) > 12 else ""
        lines.append(f"  per {name}: {len(ug)} of {-(-got.shape[d] // size)} hold errors: " + "; ".join(parts) + more)
    for k in range(min(4, idx.shape[0])):
        i = tuple(idx[k].tolist())
        lines.append(f"  at {i}: got {got[i].item()!r}, want {want[i].item()!r}")
    raise AssertionError("\n".join(lines))


def sign_words(y):
    """uint8 [N, H, W, 8] sign words of a 64-channel NCHW tensor: bit c % 8 of byte c // 8 = (y[c] > 0)"""
    N, C, H, W = y.shape
    bits = (y.permute(0, 2, 3, 1) > 0).to(torch.int32).reshape(N, H, W, C // 8, 8)
    return (bits << torch.arange(8, device=y.device, dtype=torch.int32)).sum(-1).to(torch.uint8).contiguous()


# ---- workspace and destinations of the weight gradients ----------------------------------------------------------------------
def wgrad_slab_bytes():
    """bytes of split-K slabs in front of the fp32 accumulator of a weight-gradient workspace (api.hip: slabs first, then 16 x Cout x Cin floats
    rounded up to 256 bytes): taken from the library, 8 x 8 channels giving an accumulator of exactly 4096 bytes"""
    return ops.lib().tfc_conv_wgrad_ws_bytes(OP_CONV, 8, 8) - 16 * 8 * 8 * 4


def new_wgrad_ws(device):
    """one workspace for every weight gradient of the path, zeroed once (ops.conv_wgrad's own allocation rule)"""
    return torch.zeros(ops.lib().tfc_conv_wgrad_ws_bytes(OP_CONV, 1024, 512), dtype=torch.uint8, device=device)


def ws_accumulator(ws):
    """the accumulator region of a workspace: all-zero between calls (api.hip, tfc_conv_wgrad) -- layers that share a workspace rely on it"""
    return ws[wgrad_slab_bytes():].view(torch.float32)


GUARD_FLOATS = 64                            # sentinel floats on each side of a weight-gradient slice (keeps the slice 256-byte aligned)


def grad_slice(shape, init, device):
    """(flat, dw): dw is a window of a flat fp32 buffer, as the engine's gradients are gflat.grad_views slices, with GUARD_FLOATS of SENTINEL on
    either side; `init` (a float or a tensor) fills dw"""
    n = 1
    for d in shape:
        n *= d
    flat = torch.full((n + 2 * GUARD_FLOATS,), SENTINEL, dtype=torch.float32, device=device)
    dw = flat[GUARD_FLOATS:GUARD_FLOATS + n].view(shape)
    dw.copy_(init if torch.is_tensor(init) else torch.full(shape, float(init)))
    return flat, dw


def assert_slice_guarded(flat, what):
    g = torch.cat([flat[:GUARD_FLOATS], flat[-GUARD_FLOATS:]])
    bad = int((g != SENTINEL).sum())
    assert bad == 0, f"{what}: {bad} floats next to the gradient slice changed"
