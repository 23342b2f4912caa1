"""Bit-exact tests of every convolution kernel path of the bf16 training step at batch 32 and 13 (method and case table: tests/conv_exact.py).

The kernels split their work by the batch: wgrad split-K over images, the fused first block's workgroups per image, persistent kernels that walk
several tiles only when the work outgrows the grid, per-image statistics partials. The other kernel tests run at N <= 16 with tolerances of ~1 % of
max|y|; here every layer of both networks (and the LPIPS convolutions) runs at the shapes of the benchmarked step, with the engine's own dispatch
and view forms, on integer data whose every partial sum is exact -- so the result must equal a float64 reference bit for bit.
"""
import zlib

import pytest
import torch

import tfc_gan_amd as T
from tests import conv_exact as X
from tfc_gan_amd import _lib, ops
from tfc_gan_amd.ops import DT_BF16, DT_F32, OP_CONV, OP_CONV3, OP_UPCONV, View

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def engine_dispatch(monkeypatch):
    """the engine's heuristic dispatch and default kernel forms"""
    for k in ("TFC_FIRST_BWD_VALU", "TFC_NO_FUSED_FIRST_FWD", "TFC_NO_FUSED_FIRST_BWD"):
        monkeypatch.delenv(k, raising=False)
    _lib.check(_lib.load().tfc_debug_set_igemm_config(-1), "tfc_debug_set_igemm_config")
    yield


def seed(c, N, k):
    return zlib.crc32(f"{c.net}.{c.layer}.{c.entry}.{N}.{k}".encode())


def weights(c, N):
    w = X.ints(X.weight_shape(c), seed(c, N, 1), device=DEV)
    if c.op == OP_CONV3:
        w[:, :, 3, :] = 0
        w[:, :, :, 3] = 0
    return w


def bias_of(c, N):
    return X.ints((c.Cout,), seed(c, N, 2), device=DEV) / 2 if "bias" in c.flags else None     # half-integers


def osc_of(c):
    return torch.tensor([X.OSCALE], dtype=torch.float32, device=DEV) if "oscale" in c.flags else None


def f32(t):
    return None if t is None else t.to(torch.float32).contiguous()


def _cases(*entries):
    return [c for c in X.CASES if c.entry in entries]


def _params(cases):
    return [pytest.param(c, id=X.case_id(c)) for c in cases]


# ---- gather GEMM: forward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", X.BATCHES)
@pytest.mark.parametrize("c", _params(_cases("conv_fwd")))
def test_exact_conv_fwd(c, N):
    """conv_fwd with the layer's epilogue (bias, 1/sigma, LeakyReLU(0.2) / ReLU, InstanceNorm statistics), input in the engine's view form"""
    dt = DT_BF16
    OH = X.out_hw(c)
    x = X.ints((N, c.Cin, c.H, c.W), seed(c, N, 0), device=DEV)
    w, b, osc = weights(c, N), bias_of(c, N), osc_of(c)
    z = X.ref_fwd(c.op, x, w)
    X.assert_dyadic(z, 1, "forward reference")
    v = z * (X.OSCALE if osc is not None else 1.0) + (b.view(1, -1, 1, 1) if b is not None else 0.0)
    v32 = X.store(v, DT_F32)
    if "leaky" in c.flags:
        v32 = X.leaky_f32(v32, 0.2)
    if "relu" in c.flags:
        v32 = v32.clamp_min(0.0)
    want = v32.to(torch.bfloat16)
    xv = X.to_view(x, dt, c.view)
    yv = View(torch.full((N, OH, OH, ops.pad8(c.Cout)), X.SENTINEL, dtype=torch.bfloat16, device=DEV), c.Cout)
    stats = torch.zeros((N, c.Cout, 2), dtype=torch.float32, device=DEV) if "stats" in c.flags else None
    flags = (ops.EP_LEAKY if "leaky" in c.flags else 0) | (ops.EP_RELU if "relu" in c.flags else 0)
    pk = ops.pack_weight(dt, c.op, 0, f32(w), c.Cin, c.Cout)
    ops.conv_fwd(dt, c.op, xv, c.Cin, c.Cout, pk, yv, bias=f32(b), stats=stats, flags=flags, oscale=osc)
    torch.cuda.synchronize()
    got = X.from_view(yv)
    X.assert_exact(got, want, f"{X.case_id(c)} N={N} forward")
    X.assert_untouched(xv, "input window")
    if stats is not None:
        # the statistics epilogue sums the stored bf16 values in fp32, in a fixed order: exact while the sums stay under 2^24, fp32 round-off beyond
        g = got.double()
        for k, s in ((0, g.sum((2, 3))), (1, (g * g).sum((2, 3)))):
            a = (g.abs() if k == 0 else g * g).sum((2, 3))
            err = (stats[..., k].double() - s).abs()
            lim = torch.where(a < X.EXACT_BOUND, torch.zeros_like(a), a * 2.0 ** -20)
            bad = err > lim
            assert not bad.any(), (f"statistics {k}: {int(bad.sum())} (image, channel) sums off; images "
                                   f"{sorted(set(bad.nonzero()[:, 0].tolist()))[:16]}, worst {(err - lim).max().item():.3e}")


@pytest.mark.parametrize("N", X.BATCHES)
@pytest.mark.parametrize("c", _params(X.fp32_cases(0)))
def test_exact_conv_fwd_fp32_parity_mode(c, N):
    """the G / D layers in the fp32 parity mode (one-tile-per-workgroup kernel, the first layers too), plain forward"""
    dt = DT_F32
    OH = X.out_hw(c)
    x = X.ints((N, c.Cin, c.H, c.W), seed(c, N, 0), device=DEV)
    w = weights(c, N)
    want = X.store(X.ref_fwd(c.op, x, w), dt)
    yv = View(torch.full((N, OH, OH, ops.pad8(c.Cout)), X.SENTINEL, dtype=torch.float32, device=DEV), c.Cout)
    ops.conv_fwd(dt, c.op, X.to_view(x, dt, c.view), c.Cin, c.Cout, ops.pack_weight(dt, c.op, 0, f32(w), c.Cin, c.Cout), yv)
    torch.cuda.synchronize()
    X.assert_exact(X.from_view(yv), want, f"{X.case_id(c)} N={N} fp32 forward")


# ---- gather GEMM: input gradient ------------------------------------------------------------------------------------------------
# bf16: every table row; fp32 parity mode: the G / D layers as that mode runs them (the heads and the first layer through the gather GEMM too)
DGRAD_RUNS = ([pytest.param(c, N, DT_BF16, id=f"{X.case_id(c)}-N{N}-bf16") for c in _cases("conv_dgrad") for N in X.BATCHES]
              + [pytest.param(c, N, DT_F32, id=f"{X.case_id(c)}-{c.layer}-N{N}-fp32") for c in X.fp32_cases(1) for N in X.BATCHES])


@pytest.mark.parametrize("c,N,dt", DGRAD_RUNS)
def test_exact_conv_dgrad(c, N, dt):
    """conv_dgrad, plain and accumulating (bf16: the product is rounded, then added to the stored value in fp32 and rounded again -- the epilogue's
    order), into the engine's destination: the skip window of the concat gradient for the down path, a buffer of its own elsewhere"""
    OH = X.out_hw(c)
    w, osc = weights(c, N), osc_of(c)
    dy = X.ints((N, c.Cout, OH, OH), seed(c, N, 3), device=DEV)
    gx = X.ref_dx(c.op, (N, c.Cin, c.H, c.W), w, dy)
    X.assert_dyadic(gx, 1, "input-gradient reference")
    v = X.store(gx * (X.OSCALE if osc is not None else 1.0), dt)
    base = X.ints((N, c.Cin, c.H, c.W), seed(c, N, 4), device=DEV)
    dyv = X.to_view(dy, dt)
    pkd = ops.pack_weight(dt, c.op, 1, f32(w), c.Cin, c.Cout)
    form = X.WINDOW if c.view == X.WINDOW else X.FRESH
    # plain: the destination window holds garbage that must be overwritten
    dxv = X.to_view(torch.full_like(base, 3.0), dt, form)
    ops.conv_dgrad(dt, c.op, dyv, N, c.H, c.W, c.Cin, c.Cout, pkd, dxv, oscale=osc)
    torch.cuda.synchronize()
    X.assert_exact(X.from_view(dxv), v, f"{X.case_id(c)} N={N} input gradient")
    if form == X.WINDOW:
        X.assert_untouched(dxv, "destination window")
    # accumulate into what is there
    dxv = X.to_view(base, dt, form)
    ops.conv_dgrad(dt, c.op, dyv, N, c.H, c.W, c.Cin, c.Cout, pkd, dxv, accumulate=True, oscale=osc)
    torch.cuda.synchronize()
    want = X.store(v.double() + base, dt)
    X.assert_exact(X.from_view(dxv), want, f"{X.case_id(c)} N={N} accumulated input gradient")
    if form == X.WINDOW:
        X.assert_untouched(dxv, "destination window")


# ---- weight gradients: the whole path through ONE workspace, in engine order ----------------------------------------------------
def _check_wgrad(c, N, ws, dt=DT_BF16):
    """conv_wgrad into a slice of a flat gradient buffer (as gflat.grad_views), plain and accumulating"""
    OH = X.out_hw(c)
    x = X.ints((N, c.Cin, c.H, c.W), seed(c, N, 5), device=DEV)
    dy = X.ints((N, c.Cout, OH, OH), seed(c, N, 6), device=DEV)
    gw = X.ref_dw(c.op, x, X.weight_shape(c), dy)
    X.assert_dyadic(gw, 1, "weight-gradient reference")
    xv, dyv = X.to_view(x, dt, c.view), X.to_view(dy, dt)
    what = f"{X.case_id(c)} N={N} {'fp32 ' if dt == DT_F32 else ''}weight gradient"
    flat, dw = X.grad_slice(X.weight_shape(c), 7.0, DEV)
    ops.conv_wgrad(dt, c.op, xv, dyv, c.Cin, c.Cout, dw, ws=ws)
    torch.cuda.synchronize()
    X.assert_exact(dw, X.store(gw, DT_F32), what, X.WGT_DIMS)
    X.assert_slice_guarded(flat, what)
    _acc_zero(ws, c, N, "plain")
    base = X.ints(X.weight_shape(c), seed(c, N, 7), amp=X.WGRAD_BASE_AMP, device=DEV)
    flat, dw = X.grad_slice(X.weight_shape(c), f32(base), DEV)
    ops.conv_wgrad(dt, c.op, xv, dyv, c.Cin, c.Cout, dw, accumulate=True, ws=ws)
    torch.cuda.synchronize()
    X.assert_exact(dw, X.store(gw + base, DT_F32), "accumulated " + what, X.WGT_DIMS)
    X.assert_slice_guarded(flat, "accumulated " + what)
    _acc_zero(ws, c, N, "accumulate")
    if c.view == X.WINDOW:
        X.assert_untouched(xv, "input window")


def _first_block_data(c, N, slope):
    """x, w, (bias, oscale), the conv output's signs, dy_pooled and the float64 d_raw / dw / per-image bias sums of the fused backward"""
    Hc = c.H - 1
    Po = (Hc - 1) // 2 + 1
    x = X.ints((N, c.Cin, c.H, c.W), seed(c, N, 8), device=DEV)
    w = X.ints((64, c.Cin, 4, 4), seed(c, N, 9), device=DEV)
    y = X.ref_fwd(OP_CONV, x, w)
    dy = X.ints((N, 64, Po, Po), seed(c, N, 10), density=X.FIRST_BWD_DY_DENSITY, device=DEV)
    g = X.blur_t(dy, (N, 64, Hc, Hc), 2)
    d_raw = g * torch.where(y > 0, 1.0, slope)
    return x, w, y, dy, d_raw


def _check_first_bwd(c, N, ws):
    dt = DT_BF16
    x, w, y, dy, d_raw = _first_block_data(c, N, X.SLOPE)
    X.assert_dyadic(d_raw, X.FIRST_BWD_QUANTUM, "d_raw reference")
    assert torch.equal(X.store(d_raw, dt).double(), d_raw), "d_raw must be exact in bf16"
    gw = X.ref_dw(OP_CONV, x, (64, c.Cin, 4, 4), d_raw)
    X.assert_dyadic(gw, X.FIRST_BWD_QUANTUM, "weight-gradient reference")
    bsum = d_raw.sum((2, 3))
    xv = X.to_view(x, dt)
    dyv = X.to_view(dy, dt, c.view)                           # G: the skip half of up5's concat gradient (pitch 128, offset 64)
    mask = X.sign_words(y)
    sums = "bias_sums" in c.flags
    flat, dw = X.grad_slice((64, c.Cin, 4, 4), 7.0, DEV)
    rs = torch.zeros((N, 64), dtype=torch.float32, device=DEV) if sums else None
    ops.first_block_bwd_wgrad(dt, xv, None, dyv, c.Cin, 64, dw, slope=X.SLOPE, ws=ws, bias_sums=rs, sign_mask=mask)
    torch.cuda.synchronize()
    X.assert_exact(dw, X.store(gw, DT_F32), f"{X.case_id(c)} N={N} weight gradient (sign words)", X.WGT_DIMS)
    X.assert_slice_guarded(flat, f"{X.case_id(c)} N={N} weight gradient (sign words)")
    if sums:
        X.assert_exact(rs, X.store(bsum, DT_F32), f"{X.case_id(c)} N={N} per-image bias sums", X.VEC_DIMS)
    _acc_zero(ws, c, N, "sign words")
    # the form that reads the stored conv output instead of the sign words, accumulating
    base = X.ints((64, c.Cin, 4, 4), seed(c, N, 11), amp=X.WGRAD_BASE_AMP, device=DEV)
    flat, dw = X.grad_slice((64, c.Cin, 4, 4), f32(base), DEV)
    yv = X.to_view(y, dt)
    ops.first_block_bwd_wgrad(dt, xv, yv, dyv, c.Cin, 64, dw, slope=X.SLOPE, accumulate=True, ws=ws)
    torch.cuda.synchronize()
    X.assert_exact(dw, X.store(gw + base, DT_F32), f"{X.case_id(c)} N={N} accumulated weight gradient (stored tensor)", X.WGT_DIMS)
    X.assert_slice_guarded(flat, f"{X.case_id(c)} N={N} accumulated weight gradient (stored tensor)")
    X.assert_untouched(dyv, "dy_pooled window")
    _acc_zero(ws, c, N, "stored tensor")


def _acc_zero(ws, c, N, what):
    acc = X.ws_accumulator(ws)
    nz = int((acc != 0).sum())
    assert nz == 0, f"after {X.case_id(c)} N={N} ({what}): {nz} floats of the workspace accumulator are not zero (cross-layer reuse breaks)"


@pytest.mark.parametrize("N", X.BATCHES)
def test_exact_wgrad_engine_order_one_workspace(N):
    """every weight gradient of the step (fin direct-write, reduce + finish, c8, 2 x 2-tap, phase-fused transposed, head, fused first block) in the
    order nets.py issues them, all through ONE workspace as GeneratorCore._ws / DiscriminatorCore._ws thread it: each result exact, plain and
    accumulating, and the workspace's accumulator all-zero again after every call"""
    ws = X.new_wgrad_ws(DEV)
    for c in X.WGRAD_ENGINE_ORDER:
        if c.entry == "first_block_bwd_wgrad":
            _check_first_bwd(c, N, ws)
        else:
            _check_wgrad(c, N, ws)


@pytest.mark.parametrize("N", X.BATCHES)
def test_exact_wgrad_fp32_parity_mode_engine_order_one_workspace(N):
    """the same weight gradients in the fp32 parity mode (per-phase launches for the transposed and upsample convolutions, the first layers through
    the gather GEMM), in engine order through ONE workspace: exact, plain and accumulating, accumulator all-zero after every call"""
    ws = X.new_wgrad_ws(DEV)
    for c in X.fp32_cases(2):
        _check_wgrad(c, N, ws, DT_F32)


# ---- first layer and heads ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", X.BATCHES)
@pytest.mark.parametrize("c", _params(_cases("first_block_fwd")))
def test_exact_first_block_fwd_and_first_conv(c, N):
    """tfc_first_block_fwd (conv -> [+bias, x 1/sigma] -> LeakyReLU -> BlurPool, G form: activation after the rounding) into the engine's
    destination (G: the skip half of a concat buffer) with its sign words; and tfc_conv_first_fwd, the unfused first convolution"""
    dt = DT_BF16
    gform = "gform" in c.flags
    Hc = c.H - 1
    Po = (Hc - 1) // 2 + 1
    x = X.ints((N, c.Cin, c.H, c.W), seed(c, N, 0), device=DEV)
    w = X.ints((64, c.Cin, 4, 4), seed(c, N, 1), device=DEV)
    b = None if gform else X.ints((64,), seed(c, N, 2), device=DEV) / 2
    osc = None if gform else torch.tensor([X.OSCALE], dtype=torch.float32, device=DEV)
    z = X.ref_fwd(OP_CONV, x, w)
    v32 = X.store(z if gform else z * X.OSCALE + b.view(1, -1, 1, 1), DT_F32)
    yb = (v32 if gform else X.leaky_f32(v32, X.SLOPE)).to(torch.bfloat16).double()
    act = torch.where(yb > 0, yb, X.SLOPE * yb) if gform else yb
    pooled = X.blur(act, 2)
    want = X.store(pooled, dt)
    xv = X.to_view(x, dt)
    pk = ops.pack_weight(dt, OP_CONV, 0, f32(w), c.Cin, 64)
    out = X.to_view(torch.full((N, 64, Po, Po), X.SENTINEL, dtype=torch.float64, device=DEV), dt, X.WINDOW if c.view == X.WINDOW else X.FRESH)
    mask = torch.zeros((N, Hc, Hc, 8), dtype=torch.uint8, device=DEV)
    ops.first_block_fwd(dt, xv, c.Cin, 64, pk, out, bias=f32(b), oscale=osc, slope=X.SLOPE, act_after_rounding=gform, sign_mask=mask)
    torch.cuda.synchronize()
    X.assert_exact(X.from_view(out), want, f"{X.case_id(c)} N={N} pooled output")
    X.assert_untouched(out, "output window")
    X.assert_exact(mask.permute(0, 3, 1, 2), X.sign_words(yb).permute(0, 3, 1, 2), f"{X.case_id(c)} N={N} sign words",
                   (("image", 1), ("byte", 8), ("row", X.TILE_H), ("column", X.TILE_W)))
    # the unfused first convolution (weights-stationary kernel; D: LeakyReLU(0.2) in its epilogue)
    raw32 = v32 if gform else X.leaky_f32(v32, 0.2)
    yv = View(torch.full((N, Hc, Hc, 64), X.SENTINEL, dtype=torch.bfloat16, device=DEV), 64)
    m2 = torch.zeros_like(mask)
    ops.conv_first_fwd(dt, xv, c.Cin, 64, pk, yv, bias=f32(b), oscale=osc, flags=0 if gform else ops.EP_LEAKY, sign_mask=m2)
    torch.cuda.synchronize()
    X.assert_exact(X.from_view(yv), raw32.to(torch.bfloat16), f"{X.case_id(c)} N={N} first convolution")
    assert torch.equal(m2, mask), "conv_first_fwd and first_block_fwd sign words differ"


@pytest.mark.parametrize("N", X.BATCHES)
def test_exact_first_conv_dgrad_image(N):
    """tfc_conv_dgrad_image: the discriminator's input gradient w.r.t. the generated image (3 of 6 channels, x 1/sigma), fp32 NCHW"""
    (c,) = _cases("conv_dgrad_image")
    w = X.ints((64, c.Cin, 4, 4), seed(c, N, 1), device=DEV)
    dy = X.ints((N, 64, c.H - 1, c.W - 1), seed(c, N, 3), device=DEV)
    gx = X.ref_dx(OP_CONV, (N, c.Cin, c.H, c.W), w, dy)[:, :3] * X.OSCALE
    got = ops.conv_dgrad_image(DT_BF16, X.to_view(dy, DT_BF16), N, c.H, c.W, c.Cin, f32(w), osc_of(c), 3)
    torch.cuda.synchronize()
    X.assert_exact(got, X.store(gx, DT_F32), f"{X.case_id(c)} N={N}")


@pytest.mark.parametrize("N", X.BATCHES)
def test_exact_generator_head_dgrad(N):
    """tfc_upconv_head_dgrad: dy NHWC8 (3 channels, zero padding) at 256 x 256 -> the whole 128-channel gradient of the last concat buffer"""
    (c,) = _cases("upconv_head_dgrad")
    w = X.ints((c.Cout, c.Cin, 4, 4), seed(c, N, 1), device=DEV)
    dy = X.ints((N, c.Cout, 2 * c.H, 2 * c.W), seed(c, N, 3), device=DEV)
    gx = X.ref_dx(OP_UPCONV, (N, c.Cin, c.H, c.W), w, dy)
    X.assert_dyadic(gx, 1, "head input-gradient reference")
    dxv = View(torch.full((N, c.H, c.W, c.Cin), X.SENTINEL, dtype=torch.bfloat16, device=DEV), c.Cin)
    ops.upconv_head_dgrad(DT_BF16, X.to_view(dy, DT_BF16), N, c.H, c.W, f32(w), dxv)
    torch.cuda.synchronize()
    X.assert_exact(X.from_view(dxv), X.store(gx, DT_BF16), f"{X.case_id(c)} N={N}")


@pytest.mark.parametrize("N", X.BATCHES)
def test_exact_patchgan_head_fwd(N):
    """tfc_patchgan_head_fwd: 512 -> 1 at 16 x 16, into channel 0 of an 8-channel logit buffer whose other channels stay as they are"""
    (c,) = _cases("patchgan_head_fwd")
    x = X.ints((N, c.Cin, c.H, c.W), seed(c, N, 0), device=DEV)
    w = X.ints((1, c.Cin, 4, 4), seed(c, N, 1), device=DEV)
    want = X.store(X.ref_fwd(c.op, x, w), DT_BF16)
    logits = torch.full((N, c.H, c.W, 8), X.SENTINEL, dtype=torch.bfloat16, device=DEV)
    ops.patchgan_head_fwd(DT_BF16, X.to_view(x, DT_BF16), f32(w), View(logits, 1, 0))
    torch.cuda.synchronize()
    X.assert_exact(X.from_view(View(logits, 1, 0)), want, f"{X.case_id(c)} N={N}")
    X.assert_untouched(View(logits, 1, 0), "logit channels 1..7")


# ---- pooling activations ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", X.BATCHES)
@pytest.mark.parametrize("C,H,pool,slope", [pytest.param(*a[1:], id=a[0]) for a in X.BLUR_ACTS])
def test_exact_blur_act_fwd_bwd(C, H, pool, slope, N):
    """the pure-blur act_fwd (up path: pool 1 with the statistics of its output; discriminator: pool 2) and act_bwd mode 0 (LeakyReLU' x
    BlurPool^T, with the per-image bias-gradient sums the discriminator takes from it)"""
    dt = DT_BF16
    sd = zlib.crc32(f"act.{C}.{H}.{pool}.{N}".encode())
    x = X.ints((N, C, H, H), sd, device=DEV)                  # ternary: every blurred value is exact in bf16, so are the statistics
    a = torch.where(x > 0, x, slope * x)
    want = X.store(X.blur(a, pool), dt)
    Ho = want.shape[2]
    yv = View(torch.full((N, Ho, Ho, C), X.SENTINEL, dtype=torch.bfloat16, device=DEV), C)
    so = torch.zeros((N, C, 2), dtype=torch.float32, device=DEV) if pool == 1 else None
    ops.act_fwd(dt, X.to_view(x, dt), yv, stats=None, slope=slope, pool=pool, stats_out=so)
    torch.cuda.synchronize()
    got = X.from_view(yv)
    X.assert_exact(got, want, f"act_fwd C={C} H={H} pool={pool} N={N}")
    if so is not None:
        g = got.double()
        X.assert_exact(so[..., 0], X.store(g.sum((2, 3)), DT_F32), f"act_fwd statistics (sum) C={C} H={H} N={N}", X.VEC_DIMS)
        assert torch.allclose(so[..., 1].double(), (g * g).sum((2, 3)), rtol=1e-6, atol=0), "act_fwd statistics (sum of squares)"
    dy = X.ints((N, C, Ho, Ho), sd + 1, device=DEV)
    gin = X.blur_t(dy, (N, C, H, H), pool) * torch.where(x > 0, 1.0, slope)
    dxv = View(torch.full((N, H, H, C), X.SENTINEL, dtype=torch.bfloat16, device=DEV), C)
    rs = torch.zeros((N, C), dtype=torch.float32, device=DEV)
    ops.act_bwd(dt, 0, X.to_view(dy, dt), X.to_view(x, dt) if slope != 1.0 else None, N, H, H, C, dxv, stats=None, slope=slope, pool=pool,
                rstats=rs)
    torch.cuda.synchronize()
    X.assert_exact(X.from_view(dxv), X.store(gin, dt), f"act_bwd C={C} H={H} pool={pool} N={N}")
    X.assert_exact(rs, X.store(X.store(gin, dt).double().sum((2, 3)), DT_F32), f"act_bwd bias sums C={C} H={H} N={N}", X.VEC_DIMS)


# ---- tolerance tier: what is not exact by nature -------------------------------------------------------------------------------------------
def _rel_per_image(got, want):
    d = (got.double() - want.double()).flatten(1).norm(dim=1)
    return d / want.double().flatten(1).norm(dim=1).clamp_min(1e-30)


@pytest.mark.parametrize("N", [32])
def test_first_block_production_slope(N):
    """the fused first block at the production slope 0.2. D form (LeakyReLU before the rounding, bias, 1/sigma): still exact -- the epilogue's
    fmaxf(v, 0.2f * v) is one fp32 multiply the reference repeats, and with v a multiple of 5/2 every stored value is a multiple of 1/2, so the
    pooling sums stay exact. G form (LeakyReLU inside the pooling) and the backward: within the teacher-forced bars, per image."""
    dt = DT_BF16
    cd, cg = [c for c in _cases("first_block_fwd") if c.net == "D"][0], [c for c in _cases("first_block_fwd") if c.net == "G"][0]
    Hc = cd.H - 1
    Po = (Hc - 1) // 2 + 1
    # ---- D form, exact ----
    x = X.ints((N, cd.Cin, cd.H, cd.W), seed(cd, N, 20), device=DEV)
    w = 5 * X.ints((64, cd.Cin, 4, 4), seed(cd, N, 21), device=DEV)
    b = 2.5 * X.ints((64,), seed(cd, N, 22), device=DEV)
    osc = torch.tensor([X.OSCALE], dtype=torch.float32, device=DEV)
    v32 = X.store(X.ref_fwd(OP_CONV, x, w) * X.OSCALE + b.view(1, -1, 1, 1), DT_F32)
    yb = X.leaky_f32(v32, 0.2).to(torch.bfloat16).double()
    pooled = X.blur(yb, 2)
    X.assert_dyadic(pooled, 128, "pooled reference at slope 0.2")
    pk = ops.pack_weight(dt, OP_CONV, 0, f32(w), cd.Cin, 64)
    out = X.to_view(torch.full((N, 64, Po, Po), X.SENTINEL, dtype=torch.float64, device=DEV), dt)
    mask = torch.zeros((N, Hc, Hc, 8), dtype=torch.uint8, device=DEV)
    ops.first_block_fwd(dt, X.to_view(x, dt), cd.Cin, 64, pk, out, bias=f32(b), oscale=osc, slope=0.2, act_after_rounding=False, sign_mask=mask)
    torch.cuda.synchronize()
    X.assert_exact(X.from_view(out), X.store(pooled, dt), f"D first block N={N} slope 0.2")
    assert torch.equal(mask, X.sign_words(yb)), "sign words at slope 0.2"
    # ---- G form: forward per image against the storage-rounded reference (rel-L2 5e-4) ----
    xg = X.ints((N, cg.Cin, cg.H, cg.W), seed(cg, N, 20), device=DEV)
    wg = X.ints((64, cg.Cin, 4, 4), seed(cg, N, 21), device=DEV)
    zb = X.store(X.ref_fwd(OP_CONV, xg, wg), dt).double()
    want = X.blur(torch.where(zb > 0, zb, 0.2 * zb), 2).to(torch.float32).to(torch.bfloat16)      # not dyadic: rounded, not exact
    outg = ops.new_act(N, Po, Po, 64, dt, DEV)
    ops.first_block_fwd(dt, X.to_view(xg, dt), cg.Cin, 64, ops.pack_weight(dt, OP_CONV, 0, f32(wg), cg.Cin, 64), outg, slope=0.2,
                        act_after_rounding=True)
    torch.cuda.synchronize()
    got = X.from_view(outg)
    rel = _rel_per_image(got, want)
    assert rel.max().item() <= 5e-4, rel.tolist()
    # ---- backward (D form, with the per-image bias sums): rel-L2 5e-3 per image ----
    dy = X.ints((N, 64, Po, Po), seed(cd, N, 23), density=X.FIRST_BWD_DY_DENSITY, device=DEV)
    d_raw = X.blur_t(dy, (N, 64, Hc, Hc), 2) * torch.where(yb > 0, 1.0, 0.2)
    flat, dw = X.grad_slice((64, cd.Cin, 4, 4), 0.0, DEV)
    rs = torch.zeros((N, 64), dtype=torch.float32, device=DEV)
    ops.first_block_bwd_wgrad(dt, X.to_view(x, dt), None, X.to_view(dy, dt), cd.Cin, 64, dw, slope=0.2, bias_sums=rs, sign_mask=mask)
    torch.cuda.synchronize()
    X.assert_slice_guarded(flat, "weight gradient at slope 0.2")
    gw = X.ref_dw(OP_CONV, x, (64, cd.Cin, 4, 4), d_raw)
    assert _rel_per_image(dw.unsqueeze(0), gw.unsqueeze(0)).item() <= 5e-3
    rel = _rel_per_image(rs.unsqueeze(-1), d_raw.sum((2, 3)).unsqueeze(-1))
    assert rel.max().item() <= 5e-3, rel.tolist()


# (layer, tensor, pool, slope, dropout) of the step's statistics-normalised activations: forward act_fwd with the engine's statistics (down: the
# conv's statistics epilogue sums its stored output; up: the pure blur's stats_out sums the blurred tensor), backward act_bwd mode 1 + mode 2
NORM_ACTS = [("down2", 128, 127, 2, 0.2, 0.0), ("down3", 256, 63, 2, 0.2, 0.5), ("down4", 512, 31, 2, 0.2, 0.5), ("down6", 512, 7, 2, 0.2, 0.0),
             ("up2", 512, 16, 0, 0.0, 0.5), ("up3", 256, 32, 0, 0.0, 0.5), ("up5", 64, 128, 0, 0.0, 0.0)]
STEP_SEED = 9173


@pytest.mark.parametrize("layer,C,H,pool,slope,drop", NORM_ACTS, ids=[a[0] for a in NORM_ACTS])
def test_instance_norm_act_with_dropout_per_image(layer, C, H, pool, slope, drop):
    """InstanceNorm (at the engine's own statistics) -> LeakyReLU / ReLU -> [BlurPool] -> train-mode dropout at N = 32: the dropout masks equal
    O.hip_mask_fn bit for bit (over the whole N x C x H x W index range), forward within rel-L2 5e-4 of the storage-rounded reference and backward
    within 5e-3, per image"""
    from oracle import tfcgan_oracle as O
    dt, N = DT_BF16, 32
    g = torch.Generator().manual_seed(zlib.crc32(layer.encode()))
    x = torch.randn((N, C, H, H), generator=g, dtype=torch.float64).to(DEV).to(torch.bfloat16).double()
    stats = torch.stack((x.sum((2, 3)), (x * x).sum((2, 3))), -1).to(torch.float32).contiguous()   # sums of the stored tensor
    idx = int(layer[-1]) - 1 + (16 if layer.startswith("up") else 0)
    sd = STEP_SEED * 64 + idx
    Ho = (H - 1) // 2 + 1 if pool == 2 else H
    keep = None
    if drop:
        keep = O.hip_mask_fn(STEP_SEED)(layer, (N, C, Ho, Ho)).to(DEV)
        dev_keep = ops.dropout_mask(N * Ho * Ho * C, drop, sd, DEV).bool().view(N, Ho, Ho, C).permute(0, 3, 1, 2)
        assert torch.equal(dev_keep, keep), f"kernel dropout mask != hip_mask_fn: {int((dev_keep != keep).sum())} elements"
    xr = x.clone().requires_grad_(True)
    y = X.act_ref(xr, stats, slope, pool, keep, drop)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64).to(DEV).to(torch.bfloat16).double()
    (gx,) = torch.autograd.grad(y, xr, dy)
    y = y.detach()
    xv = X.to_view(x, dt)
    yv = ops.new_act(N, Ho, Ho, C, dt, DEV)
    ops.act_fwd(dt, xv, yv, stats=stats, slope=slope, pool=pool, drop_p=drop, seed=sd)
    torch.cuda.synchronize()
    got = X.from_view(yv)
    if keep is not None:
        live = y != 0
        assert torch.equal((got != 0)[live], keep[live]), "dropped elements differ from hip_mask_fn"
        assert not got[~keep].any(), "a dropped element is nonzero"
    rel = _rel_per_image(got, X.store(y.to(torch.float32).double(), dt))
    assert rel.max().item() <= 5e-4, (layer, rel.max().item())
    rstats = torch.zeros((N, C, 2), dtype=torch.float32, device=DEV)
    dyv = X.to_view(dy, dt)
    dxv = ops.new_act(N, H, H, C, dt, DEV)
    ops.act_bwd(dt, 1, dyv, xv, N, H, H, C, None, stats=stats, slope=slope, pool=pool, drop_p=drop, seed=sd, rstats=rstats)
    ops.act_bwd(dt, 2, dyv, xv, N, H, H, C, dxv, stats=stats, slope=slope, pool=pool, drop_p=drop, seed=sd, rstats=rstats)
    torch.cuda.synchronize()
    rel = _rel_per_image(X.from_view(dxv), gx)
    assert rel.max().item() <= 5e-3, (layer, rel.max().item())


@pytest.mark.parametrize("N", [32])
def test_generator_head_fwd_tanh_per_image(N):
    """tfc_upconv_head_fwd (+bias, tanh, fp32 NCHW): exact pre-activations, tanh within the forward bar, per image"""
    (c,) = _cases("upconv_head_fwd")
    x = X.ints((N, c.Cin, c.H, c.W), seed(c, N, 0), device=DEV)
    w = X.ints((c.Cout, c.Cin, 4, 4), seed(c, N, 1), device=DEV) / 64
    b = X.ints((c.Cout,), seed(c, N, 2), device=DEV) / 2
    want = torch.tanh(X.ref_fwd(OP_UPCONV, x, w) + b.view(1, -1, 1, 1))
    out = torch.full((N, c.Cout, 2 * c.H, 2 * c.W), X.SENTINEL, dtype=torch.float32, device=DEV)
    ops.upconv_head_fwd(DT_BF16, X.to_view(x, DT_BF16, X.WHOLE), f32(w), f32(b), out)
    torch.cuda.synchronize()
    rel = _rel_per_image(out, want)
    assert rel.max().item() <= 5e-4, rel.tolist()


# ---- inventory: the table covers every convolution a real step issues -------------------------------------------------------------------
def _recorded(fn):
    for k in range(4):
        ops.prof_collect(k)                                    # drop older records
    ops.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        recs = ops.prof_records(1 << 14)
    finally:
        ops.prof_enable(False)
        for k in range(4):
            ops.prof_collect(k)
    return recs


def test_inventory_train_step_and_lpips_batch32():
    """one bf16 TrainStep.step and one LPIPS value + gradient at N = 32 with the profiler on: every convolution they record is in the table
    (a new layer path or shape fails here until tests/conv_exact.py covers it), and every table entry of theirs was issued"""
    import warnings
    N = 32
    T.set_compute_dtype(torch.bfloat16)
    torch.manual_seed(0)
    G = T.GeneratorUNet((3, 256, 256)).to(DEV)
    D = T.Discriminator1((3, 256, 256)).to(DEV)
    G.apply(T.weights_init_normal)
    D.apply(T.weights_init_normal)
    ts = T.TrainStep(G, D)
    A, B = T.synthetic_pairs(N, seed=5)
    A, B = A.to(DEV), B.to(DEV)
    table = {X.prof_key(c): c for c in X.CASES if X.prof_key(c) is not None}
    recs = _recorded(lambda: ts.step(A, B))
    keys = {X.record_key(r) for r in recs}
    assert all(r["N"] == N for r in recs), sorted({r["N"] for r in recs})
    missing = sorted(keys - set(table))
    assert not missing, f"convolutions of the step that no exact test covers: {missing}"
    unused = sorted(k for k, c in table.items() if c.net in ("G", "D") and k not in keys)
    assert not unused, f"table entries the step never issued: {unused}"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lp = T.LPIPS(net_type="vgg", version="0.1", seed=0).to(DEV)
    recs = _recorded(lambda: lp.value_and_grad(A, B))
    keys = {X.record_key(r) for r in recs}
    missing = sorted(keys - set(table))
    assert not missing, f"LPIPS convolutions that no exact test covers: {missing}"
    unused = sorted(k for k, c in table.items() if c.net == "LPIPS" and k not in keys)
    assert not unused, f"LPIPS table entries never issued: {unused}"
    print(f"inventory: {len(table)} table keys, step + LPIPS covered")
