"""The five hand-written kernels of csrc/lpips.hip at the launch and shape edges the LPIPS workload takes, through the C ABI, against the float64
restatements of tests/lpips_ref.py (held against torch on the CPU by tests/test_lpips_host.py). Inputs are rounded to the storage type before the
reference sees them, so the bounds cover the kernels' arithmetic and their ONE store rounding, nothing else.

Head: `head_launch` restates the launcher's decomposition (tfc_launch_lpips_head: workgroups per image and their pixel range are functions of H*W,
C and the element type only) so that every case can ASSERT the branch it is there for; the cases are chosen by those properties, not by constants.
Bounds (against head_ref): value 1e-4 relative (non-negative weights: no cancellation); gradient fp32 |err| <= 1e-4 max|ref|; gradient bf16
|err| <= 2^-8 |ref| + 1e-4 max|ref| per element (the fp32 bound, plus ONE round-to-nearest bf16 store: half an ulp of 8 significant bits, which
reaches 2^-8 relative at the bottom of a binade -- observed up to 0.94 of the bound, so a second rounding anywhere would show). All-zero fx pixels are INCLUDED, with the analytic form the kernel documents; max|ref| is taken over those pixels and
over the rest separately, so that their 1e10-sized entries hide nothing elsewhere.
Reproducibility and batch independence of the head are bit comparisons. Max-pool and the ReLU backward are bit-exact. The input z-score is held
to 2 fp32 ulp of the float64 value before its store (lpips_ref.f32_interval)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tfc_gan_amd as T
from tests import lpips_ref as R
from tests.test_gpu_31_lpips import DEV, _module, from_view, q, rnd, to_view
from tfc_gan_amd import ops

pytestmark = pytest.mark.gpu
DTS = [ops.DT_F32, ops.DT_BF16]


def _lib():
    return ops.lib(), ops.stream_ptr()


# ---- head ------------------------------------------------------------------------------------------------------------------------------------
def head_launch(dt, C, HW):
    """tfc_launch_lpips_head's decomposition of one image, restated: lanes per pixel group, pixels per workgroup iteration, pixels per workgroup
    (a whole number of iterations), workgroups per image. No batch size in it."""
    units = C // (8 if dt == ops.DT_BF16 else 4)
    GS = 1
    while GS < units and GS < 64:
        GS *= 2
    ppb = 4 * (64 // GS)
    wpi = min(-(-HW // ppb), 64)
    chunk = -(-(-(-HW // wpi)) // ppb) * ppb
    return {"units": units, "GS": GS, "ppb": ppb, "chunk": chunk, "wpi": -(-HW // chunk), "capped": -(-HW // ppb) > 64}


def head_inputs(dt, N, C, H, W, seed=11):
    """post-ReLU-like features (many exact zeros) and non-negative head weights; all-zero fx vectors at the last pixel of image 0 (the last pixel of
    an image, and of its last workgroup's range) and at the first pixel of a workgroup's range in the last image (of its second workgroup if it has one)"""
    fx, fy = q(rnd((N, C, H, W), seed).clamp_min(0), dt), q(rnd((N, C, H, W), seed + 1).clamp_min(0), dt)
    L = head_launch(dt, C, H * W)
    for n, p in ((0, H * W - 1), (N - 1, L["chunk"] if L["wpi"] > 1 else 0)):
        fx[n, :, p // W, p % W] = 0
    w = torch.from_numpy(np.random.default_rng(seed + 2).random(C).astype(np.float32))
    return fx, fy, w


def run_head(dt, fx, fy, w, gscale, out0=None, want_grad=True):
    N, C, H, W = fx.shape
    lib, st = _lib()
    out = torch.zeros(N, device=DEV) if out0 is None else out0.clone().to(DEV)
    xv, yv, wd = to_view(fx, dt), to_view(fy, dt), w.to(DEV)
    dv = ops.new_act(N, H, W, C, dt, DEV) if want_grad else None
    T._lib.check(lib.tfc_lpips_head(st, dt, xv.ptr, yv.ptr, ops._p(wd), ops._p(out), None if dv is None else dv.ptr, N, H, W, C, gscale,
                                    ops.part_ws(DEV)), "tfc_lpips_head")
    return out.cpu(), None if dv is None else from_view(dv)


def assert_head_gradient(got, ref, fx, dt, what):
    zero = R.zero_pixels(fx.double()).expand_as(ref)
    assert zero.any() and not zero.all()
    for name, m in (("zero-vector pixels", zero), ("other pixels", ~zero)):
        r, err = ref[m], (got.double()[m] - ref[m]).abs()
        mx = r.abs().max().item()
        bound = 1e-4 * mx + (2.0 ** -8 * r.abs() if dt == ops.DT_BF16 else 0.0)
        print(f"{what} {name}: max|ref| {mx:.4e} max err {err.max().item():.4e} worst err/bound {(err / bound).max().item():.3f}")
        assert torch.isfinite(got[m]).all() and (err <= bound).all(), (what, name)


# (N, C, H, W), dtypes, the property of the launch it is there for (asserted on head_launch of every dtype it runs in)
HEAD_CASES = [
    ((2, 8, 3, 5), DTS, lambda L: L["GS"] in (1, 2) and L["units"] == L["GS"] and L["wpi"] == 1),
    ((3, 24, 5, 7), DTS, lambda L: L["units"] < L["GS"] and L["units"] in (3, 6)),
    ((131, 8, 1, 1), DTS, lambda L: L["wpi"] == 1 and L["chunk"] == L["ppb"] > 1),
    ((70, 64, 1, 1), DTS, lambda L: L["wpi"] == 1 and L["chunk"] == L["ppb"] > 1),
    ((3, 64, 6, 11), DTS, lambda L: 1 < L["wpi"] < 64 and not L["capped"] and L["chunk"] == L["ppb"] and 66 % L["ppb"]),
    ((2, 512, 17, 17), DTS, lambda L: L["capped"] and L["wpi"] < 64 and L["chunk"] == 2 * L["ppb"] and 289 % L["chunk"] == 1),
    ((3, 512, 53, 53), [ops.DT_F32], lambda L: L["capped"] and L["wpi"] == 64 and L["units"] == 2 * L["GS"] and L["chunk"] > L["ppb"] and (2809 % L["chunk"]) % L["ppb"]),
    ((3, 64, 150, 150), [ops.DT_BF16], lambda L: L["capped"] and L["wpi"] == 64 and L["GS"] == 8 and L["chunk"] > L["ppb"] and (22500 % L["chunk"]) % L["ppb"]),
]
HEAD_PARAMS = [pytest.param(dt, shape, prop, id=f"{'bf16' if dt == ops.DT_BF16 else 'f32'}-{'x'.join(map(str, shape))}")
               for shape, dts, prop in HEAD_CASES for dt in dts]


@pytest.mark.parametrize("dt,shape,prop", HEAD_PARAMS)
def test_head_value_and_gradient_at_launch_edges(dt, shape, prop):
    """Which branch each shape reaches (pixels of an image are dealt to its workgroups in ranges of `chunk`, a whole number of workgroup iterations
    of `ppb` pixels; a group of GS lanes owns a pixel):
      (2, 8, 3, 5)       one 16-byte unit per pixel and lane (GS = 1 in bf16, 2 in fp32); 15 pixels: one workgroup per image, its only iteration
                         mostly out of range (`live == false` in whole waves, whose leaders contribute 0)
      (3, 24, 5, 7)      units = 3 (bf16) / 6 (fp32) under GS = 4 / 8: idle lanes inside every pixel group
      (131, 8, 1, 1), (70, 64, 1, 1)   one pixel per image, more images than any one workgroup ever summed (64): grid.y walks the batch
      (3, 64, 6, 11)     several workgroups per image below the cap of 64, one iteration each, the last one partly out of range
      (2, 512, 17, 17)   the cap holds (289 pixels / 4 per iteration > 64), and rounding the range up to whole iterations leaves FEWER than 64
                         workgroups; the last one owns a single pixel; bf16: one unit per lane of a 64-lane group, fp32: two
      (3, 512, 53, 53)   fp32: cap, 64 workgroups per image, ranges of several iterations, the last range ends inside an iteration; two units per lane
      (3, 64, 150, 150)  bf16: the same with GS = 8 (eight pixels per wave)
    Variants: gscale 0.7 into a zeroed `out`; gscale -2.0 onto a non-zero running sum (the entry point adds); dfx = None (value only), whose `out`
    must have the bits of the run that also wrote gradients."""
    N, C, H, W = shape
    assert prop(head_launch(dt, C, H * W)), head_launch(dt, C, H * W)
    fx, fy, w = head_inputs(dt, N, C, H, W)
    val, g07 = R.head_ref(fx.double(), fy.double(), w.double(), 0.7)
    _, gm2 = R.head_ref(fx.double(), fy.double(), w.double(), -2.0)
    out, dfx = run_head(dt, fx, fy, w, 0.7)
    err = (out.double() - val).abs()
    print(f"value: max relative error {(err / val.clamp_min(1e-300)).max().item():.3e}")
    assert val.max().item() > 0 and (err <= 1e-4 * val).all()
    assert_head_gradient(dfx, g07, fx, dt, "gscale 0.7")
    out_only, none = run_head(dt, fx, fy, w, 0.7, want_grad=False)
    assert none is None and torch.equal(out_only, out)
    run0 = 0.125 * (1 + torch.arange(N) % 5).float()
    out2, dfx2 = run_head(dt, fx, fy, w, -2.0, out0=run0)
    want2 = run0.double() + val
    err2 = (out2.double() - want2).abs()
    print(f"running sum: max error / value {(err2 / val).max().item():.3e}")
    assert (err2 <= 1e-4 * val + 2.0 ** -23 * want2).all()         # 1e-4 on the value, and the one fp32 add onto the running sum
    assert_head_gradient(dfx2, gm2, fx, dt, "gscale -2.0")


def test_head_refuses_without_part_ws():
    fx, fy, w = head_inputs(ops.DT_F32, 2, 8, 3, 5)
    lib, st = _lib()
    out = torch.full((2,), 3.0, device=DEV)
    xv, yv, wd = to_view(fx, ops.DT_F32), to_view(fy, ops.DT_F32), w.to(DEV)
    assert lib.tfc_lpips_head(st, ops.DT_F32, xv.ptr, yv.ptr, ops._p(wd), ops._p(out), None, 2, 3, 5, 8, 1.0, None) != 0
    assert "part_ws" in lib.tfc_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())                                 # nothing ran


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [(2, 64, 64, 64), (3, 512, 53, 53)])
def test_head_is_bit_reproducible(dt, shape):
    """the same call five times into a zeroed `out`: value and gradient bits never change (float atomics, which this kernel once added its
    per-image sums with, gave a different last bit from run to run)"""
    fx, fy, w = head_inputs(dt, *shape, seed=21)
    out0, dfx0 = run_head(dt, fx, fy, w, 0.7)
    for _ in range(4):
        out, dfx = run_head(dt, fx, fy, w, 0.7)
        assert torch.equal(out, out0) and torch.equal(dfx, dfx0)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [(5, 64, 10, 13), (5, 256, 5, 7)])
def test_head_is_independent_of_the_batch(dt, shape):
    """out[n] and dfx[n] of a batch-5 call have the bits of the same image run alone and run in a batch of 2 (in either position)"""
    N, C, H, W = shape
    fx, fy, w = head_inputs(dt, N, C, H, W, seed=31)
    out5, dfx5 = run_head(dt, fx, fy, w, 0.7)
    assert len(set(out5.tolist())) == N
    for n in range(N):
        out1, dfx1 = run_head(dt, fx[n:n + 1], fy[n:n + 1], w, 0.7)
        assert torch.equal(out1[0], out5[n]) and torch.equal(dfx1[0], dfx5[n]), n
        pair = [n, (n + 1) % N]
        out2, dfx2 = run_head(dt, fx[pair], fy[pair], w, 0.7)
        assert torch.equal(out2, out5[pair]) and torch.equal(dfx2, dfx5[pair]), pair


def test_lpips_value_and_grad_is_bit_reproducible():
    m = _module(seed=7).to(DEV)
    x, y = (rnd((2, 3, 64, 48), 41) * 0.4).clamp(-1, 1).to(DEV), (rnd((2, 3, 64, 48), 42) * 0.4).clamp(-1, 1).to(DEV)
    v0, d0 = m.value_and_grad(x, y)
    v1, d1 = m.value_and_grad(x, y)
    assert v0.item() > 0 and d0.abs().max().item() > 0
    assert torch.equal(v0, v1) and torch.equal(d0, d1)


# ---- max-pool --------------------------------------------------------------------------------------------------------------------------------
def run_maxpool(dt, x, go):
    N, C, H, W = x.shape
    lib, st = _lib()
    xv, gov = to_view(x, dt), to_view(go, dt)
    yv, gv = ops.new_act(N, H // 2, W // 2, C, dt, DEV), ops.new_act(N, H, W, C, dt, DEV)
    T._lib.check(lib.tfc_maxpool2_fwd(st, dt, xv.ptr, yv.ptr, N, H, W, C), "tfc_maxpool2_fwd")
    T._lib.check(lib.tfc_maxpool2_bwd(st, dt, xv.ptr, gov.ptr, gv.ptr, N, H, W, C), "tfc_maxpool2_bwd")
    return from_view(yv), from_view(gv)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", [(1, 8, 2, 2), (3, 24, 6, 10), (2, 512, 4, 4), (5, 64, 14, 18)])
def test_maxpool_bit_exact_with_ties_and_negative_windows(dt, shape):
    """(1, 8, 2, 2): one window, one unit (fp32: two). (3, 24, 6, 10): three / six units per pixel. (2, 512, 4, 4): the widest layer.
    (5, 64, 14, 18): a thread count that is no multiple of 256 (the guard of the last workgroup). Values from five levels of both signs."""
    N, C, H, W = shape
    x = torch.from_numpy(np.random.default_rng(5).integers(-2, 3, shape).astype(np.float32) * 0.25)
    go = q(rnd((N, C, H // 2, W // 2), 6), dt)
    want_y, want_dx = R.maxpool_ref(x.double(), go.double())
    if N * C * H * W >= 256:
        v = R._windows(x)
        assert (v == v[0]).all(0).any() and (v.max(0).values < 0).any()       # four-way ties and all-negative windows are in the data
    y, dx = run_maxpool(dt, x, go)
    assert torch.equal(y, want_y.float()) and torch.equal(dx, want_dx.float())


@pytest.mark.parametrize("dt", DTS)
def test_maxpool_signed_zeros_as_torch(dt):
    """-0.0 and +0.0 in one window: value (with its sign) and gradient routing are what F.max_pool2d does on the CPU, whatever that is"""
    x = torch.tensor([[-0.0, 0.0, 0.0, -0.0, -0.5, -0.0], [-0.0, 0.0, -0.0, -0.0, 0.0, -0.5]]).reshape(1, 1, 2, 6).repeat(2, 8, 1, 1)
    xr = x.clone().requires_grad_(True)
    want = F.max_pool2d(xr, 2, 2)
    go = q(rnd(tuple(want.shape), 7), dt)
    (gx,) = torch.autograd.grad(want, xr, go)
    y, dx = run_maxpool(dt, x, go)
    assert torch.equal(y, want.detach()) and torch.equal(torch.signbit(y), torch.signbit(want.detach()))
    assert torch.equal(dx, gx)
    ry, rdx = R.maxpool_ref(x.double(), go.double())
    assert torch.equal(torch.signbit(ry), torch.signbit(want.detach())) and torch.equal(rdx.float(), gx)


# ---- ReLU backward ---------------------------------------------------------------------------------------------------------------------------
RELU_SIZES = {"one-unit": lambda ue: 8, "ragged": lambda ue: 8 * 257, "second-trip": lambda ue: ue * (8192 * 256 + 322)}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("size", list(RELU_SIZES))
def test_relu_bwd_bit_exact(dt, size):
    """n = 8: one workgroup, one or two live lanes. n = 8 * 257: the last workgroup partly idle. 8192 * 256 + 322 units: the launch caps the grid at
    8192 workgroups, so 322 lanes run a second trip of the grid-stride loop. With and without `extra`, in place (dz == dy, as lpips.py calls
    it) and out of place; y holds exact 0.0 and -0.0 (gradient 0) and negative values. fp32 is one IEEE add, bf16 is the fp32 sum of the two
    bf16 gradients rounded to nearest even: bit-equal, no tolerance."""
    tdt = ops.torch_dtype(dt)
    n = RELU_SIZES[size](8 if dt == ops.DT_BF16 else 4)
    g = torch.Generator().manual_seed(n % 1000)
    g1, g2, y = (torch.randn(n, generator=g).to(tdt) for _ in range(3))
    y[0::7], y[3::11] = 0.0, -0.0
    assert (y < 0).any() and (y > 0).any()
    lib, st = _lib()
    yd, g2d = y.to(DEV), g2.to(DEV)
    for extra in (True, False):
        s = g1.float() + g2.float() if extra else g1.float()
        want = torch.where(y.float() > 0, s.to(tdt), torch.zeros((), dtype=tdt))
        ref = R.relu_bwd_ref(g1.double(), y.double(), g2.double() if extra else None)
        assert (want.double() - ref).abs().max().item() <= (2.0 ** -8 if dt == ops.DT_BF16 else 2.0 ** -23) * ref.abs().max().item()
        for inplace in (True, False):
            dy = g1.to(DEV)
            dz = dy if inplace else torch.full((n,), 7.0, dtype=tdt, device=DEV)
            T._lib.check(lib.tfc_relu_bwd(st, dt, ops._p(dy), ops._p(yd), ops._p(g2d) if extra else None, ops._p(dz), n), "tfc_relu_bwd")
            assert torch.equal(dz.cpu(), want), (extra, inplace)
            if not inplace:
                assert torch.equal(dy.cpu(), g1)
    assert torch.equal(yd.cpu().view(torch.int16 if dt == ops.DT_BF16 else torch.int32), y.view(torch.int16 if dt == ops.DT_BF16 else torch.int32))


# ---- input z-score ---------------------------------------------------------------------------------------------------------------------------
def _store(lo, hi, dt):
    """the storage rounding applied to both ends of an fp32 interval (monotone)"""
    return (lo.bfloat16().float(), hi.bfloat16().float()) if dt == ops.DT_BF16 else (lo, hi)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("pitch", [8, 32])
@pytest.mark.parametrize("C", [1, 3, 8])
@pytest.mark.parametrize("N,H,W", [(1, 1, 1), (2, 7, 37), (3, 16, 17)])
def test_input_zscore_forward_and_backward(dt, pitch, C, N, H, W):
    """Forward: channels [0, C) within 2 fp32 ulp of the float64 (x - shift) / scale and then rounded to the storage type; channels [C, 8) written as
    zero; channels [8, pitch) keep the caller's sentinel. Backward: dx (=/+=) alpha * g / scale with alpha in {1, -0.5}, onto a non-zero dx when
    it accumulates: the quotient within 2 fp32 ulp, then the one fp32 add. (2, 7, 37): 518 pixels, three workgroups, the last partly idle."""
    tdt = ops.torch_dtype(dt)
    lib, st = _lib()
    x = (rnd((N, C, H, W), 51) * 0.5).clamp(-1, 1)
    if C == 3:
        shift, scale = torch.tensor([-.030, -.088, -.188]), torch.tensor([.458, .448, .450])
    else:
        shift, scale = rnd((C,), 52) * 0.3, torch.from_numpy(np.random.default_rng(53).random(C).astype(np.float32)) + 0.3
    out = torch.full((N, H, W, pitch), 7.0, dtype=tdt, device=DEV)
    xd, shd, scd = x.to(DEV), shift.to(DEV), scale.to(DEV)
    T._lib.check(lib.tfc_lpips_input_fwd(st, dt, ops._p(xd), ops._p(shd), ops._p(scd), ops._p(out), N, C, H, W, pitch), "tfc_lpips_input_fwd")
    got = out.float().cpu()
    lo, hi = _store(*R.f32_interval(R.input_ref(x.double(), shift.double(), scale.double()).permute(0, 2, 3, 1), 2), dt)
    assert (lo <= got[..., :C]).all() and (got[..., :C] <= hi).all()
    assert not got[..., C:8].any() and bool((got[..., 8:] == 7.0).all())
    g = rnd((N, H, W, pitch), 54).to(tdt)                            # channels [C, pitch) hold values the backward must not read into dx
    gd = g.to(DEV)
    vref = g.double()[..., :C].permute(0, 3, 1, 2)
    dx0 = rnd((N, C, H, W), 55)
    for alpha in (1.0, -0.5):
        lo, hi = R.f32_interval(R.input_bwd_ref(vref, scale.double(), alpha), 2)
        for accumulate in (0, 1):
            dx = dx0.to(DEV)
            T._lib.check(lib.tfc_lpips_input_bwd(st, dt, ops._p(gd), ops._p(scd), ops._p(dx), N, C, H, W, pitch, alpha, accumulate), "tfc_lpips_input_bwd")
            a, b = (dx0 + lo, dx0 + hi) if accumulate else (lo, hi)   # fp32 adds: IEEE, as the kernel's
            gotx = dx.cpu()
            assert (torch.minimum(a, b) <= gotx).all() and (gotx <= torch.maximum(a, b)).all(), (alpha, accumulate)
