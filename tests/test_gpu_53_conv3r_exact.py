"""Bit-exact tests of TFC_OP_CONV3R = nn.ReflectionPad2d(1) + nn.Conv2d(Cin, Cout, 3), all three passes, in every compute mode (method: tests/conv_exact.py,
as tests/test_gpu_49_conv2_exact.py applies it).

Operands are small integers (the bias: half-integers), so every partial sum is exact in fp32 in any order and the stored value must equal the rounding
of a float64 F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w[:, :, :3, :3]) or of its autograd adjoints: torch.equal, no tolerance. The input gradient
is the adjoint of the padding too: gradient that the forward read through a reflected pixel returns to the pixel it was read from, corners on both axes.

The shapes are the smallest that pin each border rule (see SHAPES); the batch-invariance and run-to-run tests use Gaussian data, where a different
order of additions would change bits.
"""
import zlib

import pytest
import torch
import torch.nn.functional as F

import tfc_gan_amd as T
from tests import conv_exact as X
from tfc_gan_amd import _lib, ops
from tfc_gan_amd.ops import DT_BF16, DT_BF16X3, DT_F32, View

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OP = getattr(_lib, "OP_CONV3R", None)        # None before the op exists: every test then fails at its first call

# (N, H, W, Cin, Cout)
SHAPES = [(3, 2, 2, 32, 32),                 # both borders reflect onto the same two rows; corners fold twice
          (2, 8, 16, 64, 64),                # exactly one tile: every halo edge is an image edge
          (2, 9, 17, 32, 64),                # ragged tiles: a tile border that is not an image border must not reflect
          (5, 5, 20, 64, 32),                # non-square, odd batch: no reflection into the next image
          (1, 16, 16, 256, 256)]             # the trunk's channels, several K chunks
DTS = [pytest.param(DT_BF16, id="bf16"), pytest.param(DT_F32, id="fp32"), pytest.param(DT_BF16X3, id="bf16x3")]
_ids = [f"N{n}-{h}x{w}-{ci}to{co}" for n, h, w, ci, co in SHAPES]
SLOT = (slice(None), slice(None), slice(0, 3), slice(0, 3))       # the 3 x 3 filter inside its [Cout][Cin][4][4] slot


@pytest.fixture(autouse=True)
def engine_dispatch():
    _lib.check(_lib.load().tfc_debug_set_igemm_config(-1), "tfc_debug_set_igemm_config")
    yield


def seed(shape, k):
    return zlib.crc32(f"conv3r.{shape}.{k}".encode())


def ref(x, w):
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w[:, :, :3, :3])


def f32(t):
    return None if t is None else t.to(torch.float32).contiguous()


def slot_weight(shape, k):
    """integer 3 x 3 filter in rows / columns 0..2 of the 4 x 4 slot, zeros in the seven unused taps (as the op is handed its weights)"""
    _, _, _, Cin, Cout = shape
    w = torch.zeros((Cout, Cin, 4, 4), dtype=torch.float64, device=DEV)
    w[SLOT] = X.ints((Cout, Cin, 3, 3), seed(shape, k), device=DEV)
    return w


def assert_exact_range(shape):
    """the test cannot pass on an inexact reference: the largest partial sum of every pass, in quanta, stays below 2^24"""
    N, H, W, Cin, Cout = shape
    assert 9 * ops.pad8(Cin) * 2 + 1 < X.EXACT_BOUND            # forward (quantum 1/2 with the half-integer bias)
    assert 9 * ops.pad8(Cin) < X.EXACT_BOUND
    assert 9 * ops.pad8(Cout) + 1 < X.EXACT_BOUND               # dgrad, + the value an accumulating call adds to
    assert N * H * W + X.WGRAD_BASE_AMP < X.EXACT_BOUND         # wgrad, + the value an accumulating call starts from


def _stats_exact(got, stats, what):
    """the statistics epilogue adds the STORED values and their squares in fp32: exact, in any order, while the sum of magnitudes stays below 2^24 quanta
    (values are multiples of 1/2, squares of 1/4) -- asserted on the data, then the sums are compared with =="""
    g = got.double()
    for k, s, a, q in ((0, g.sum((2, 3)), g.abs().sum((2, 3)), 2), (1, (g * g).sum((2, 3)), (g * g).sum((2, 3)), 4)):
        assert (a * q).max().item() < X.EXACT_BOUND, f"{what}: statistics {k} leave the exact range ({(a * q).max().item():.0f} quanta): shrink the data"
        X.assert_exact(stats[..., k].double(), s, f"{what} statistics {k}", X.VEC_DIMS)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_exact_conv3r_fwd(shape, dt):
    """forward with TFC_EP_BIAS, TFC_EP_BIAS | TFC_EP_RELU and TFC_EP_BIAS | TFC_EP_STATS (the statistics exactly)"""
    N, H, W, Cin, Cout = shape
    assert_exact_range(shape)
    x = X.ints((N, Cin, H, W), seed(shape, 0), device=DEV)
    w = slot_weight(shape, 1)
    b = X.ints((Cout,), seed(shape, 2), device=DEV) / 2
    z = ref(x, w)
    X.assert_dyadic(z, 1, "forward reference")
    assert tuple(z.shape[2:]) == (ops.OUT_HW[OP](H), ops.OUT_HW[OP](W)) == (H, W)
    v32 = X.store(z + b.view(1, -1, 1, 1), DT_F32)
    xv = X.to_view(x, dt)
    pk = ops.pack_weight(dt, OP, 0, f32(w), Cin, Cout)
    for name, flags, want32 in (("bias", 0, v32), ("bias|relu", ops.EP_RELU, torch.relu(v32)), ("bias|stats", 0, v32)):
        want = want32.to(ops.torch_dtype(dt))
        yv = View(torch.full((N, H, W, ops.pad8(Cout)), X.SENTINEL, dtype=ops.torch_dtype(dt), device=DEV), Cout)
        stats = torch.zeros((N, Cout, 2), dtype=torch.float32, device=DEV) if name == "bias|stats" else None
        ops.conv_fwd(dt, OP, xv, Cin, Cout, pk, yv, bias=f32(b), stats=stats, flags=flags)
        torch.cuda.synchronize()
        got = X.from_view(yv)
        X.assert_exact(got, want, f"conv3r {shape} forward ({name})")
        if stats is not None:
            _stats_exact(got, stats, f"conv3r {shape}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_exact_conv3r_dgrad(shape, dt):
    """input gradient = the exact adjoint (folded ring included), plain (the destination holds garbage) and with TFC_EP_ACCUM onto an integer tensor"""
    N, H, W, Cin, Cout = shape
    assert_exact_range(shape)
    w = slot_weight(shape, 1)
    dy = X.ints((N, Cout, H, W), seed(shape, 3), device=DEV)
    x0 = torch.zeros((N, Cin, H, W), dtype=torch.float64, device=DEV, requires_grad=True)
    (gx,) = torch.autograd.grad(ref(x0, w), x0, dy)
    X.assert_dyadic(gx, 1, "input-gradient reference")
    v = X.store(gx, dt)
    base = X.ints((N, Cin, H, W), seed(shape, 4), device=DEV)
    dyv = X.to_view(dy, dt)
    pkd = ops.pack_weight(dt, OP, 1, f32(w), Cin, Cout)
    dxv = X.to_view(torch.full_like(base, 3.0), dt)
    ops.conv_dgrad(dt, OP, dyv, N, H, W, Cin, Cout, pkd, dxv)
    torch.cuda.synchronize()
    X.assert_exact(X.from_view(dxv), v, f"conv3r {shape} input gradient")
    dxv = X.to_view(base, dt)
    ops.conv_dgrad(dt, OP, dyv, N, H, W, Cin, Cout, pkd, dxv, accumulate=True)
    torch.cuda.synchronize()
    X.assert_exact(X.from_view(dxv), X.store(v.double() + base, dt), f"conv3r {shape} accumulated input gradient")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_exact_conv3r_wgrad(shape, dt):
    """weight gradient into a guarded slice of a flat buffer, plain and accumulating: the 3 x 3 filter exactly, the seven unused taps of the slot zero
    (unchanged under `accumulate`), the guard floats untouched, the workspace's accumulator all-zero again afterwards"""
    N, H, W, Cin, Cout = shape
    assert_exact_range(shape)
    x = X.ints((N, Cin, H, W), seed(shape, 5), device=DEV)
    dy = X.ints((N, Cout, H, W), seed(shape, 6), device=DEV)
    w0 = torch.zeros((Cout, Cin, 4, 4), dtype=torch.float64, device=DEV, requires_grad=True)
    (gw,) = torch.autograd.grad(ref(x, w0), w0, dy)             # zero outside the 3 x 3 taps: w0[:, :, :3, :3] is all the reference reads
    X.assert_dyadic(gw, 1, "weight-gradient reference")
    unused = torch.ones((4, 4), dtype=torch.bool, device=DEV)
    unused[:3, :3] = False
    assert int(unused.sum()) == 7 and float(gw[:, :, unused].abs().sum()) == 0.0
    ws = X.new_wgrad_ws(DEV)
    xv, dyv = X.to_view(x, dt), X.to_view(dy, dt)
    flat, dw = X.grad_slice((Cout, Cin, 4, 4), 7.0, DEV)
    ops.conv_wgrad(dt, OP, xv, dyv, Cin, Cout, dw, ws=ws)
    torch.cuda.synchronize()
    X.assert_exact(dw, X.store(gw, DT_F32), f"conv3r {shape} weight gradient", X.WGT_DIMS)
    assert float(dw[:, :, unused].abs().sum()) == 0.0, "the seven unused taps of the slot are not zero"
    X.assert_slice_guarded(flat, "weight gradient")
    assert int((X.ws_accumulator(ws) != 0).sum()) == 0, "the workspace accumulator is not all-zero after the call"
    base = X.ints((Cout, Cin, 4, 4), seed(shape, 7), amp=X.WGRAD_BASE_AMP, device=DEV)
    flat, dw = X.grad_slice((Cout, Cin, 4, 4), f32(base), DEV)
    ops.conv_wgrad(dt, OP, xv, dyv, Cin, Cout, dw, accumulate=True, ws=ws)
    torch.cuda.synchronize()
    X.assert_exact(dw, X.store(gw + base, DT_F32), f"conv3r {shape} accumulated weight gradient", X.WGT_DIMS)
    assert torch.equal(dw[:, :, unused], f32(base)[:, :, unused]), "the seven unused taps changed under accumulate"
    X.assert_slice_guarded(flat, "accumulated weight gradient")
    assert int((X.ws_accumulator(ws) != 0).sum()) == 0, "the workspace accumulator is not all-zero after the accumulating call"


def _gauss(shape, s):
    g = torch.Generator().manual_seed(s)
    return torch.randn(shape, generator=g, dtype=torch.float32).to(DEV)


def _gauss_weight(Cin, Cout, s):
    w = torch.zeros((Cout, Cin, 4, 4), dtype=torch.float32, device=DEV)
    w[SLOT] = _gauss((Cout, Cin, 3, 3), s) * 0.05
    return w


def _run_all(dt, shape, x, w, b, dy, ws):
    n, (_, H, W, Cin, Cout) = x.shape[0], shape
    yv = ops.new_act(n, H, W, Cout, dt, DEV)
    st = torch.zeros((n, Cout, 2), dtype=torch.float32, device=DEV)
    ops.conv_fwd(dt, OP, X.to_view(x.double(), dt), Cin, Cout, ops.pack_weight(dt, OP, 0, w, Cin, Cout), yv, bias=b, stats=st)
    dxv = ops.new_act(n, H, W, Cin, dt, DEV)
    ops.conv_dgrad(dt, OP, X.to_view(dy.double(), dt), n, H, W, Cin, Cout, ops.pack_weight(dt, OP, 1, w, Cin, Cout), dxv)
    dw = torch.empty((Cout, Cin, 4, 4), dtype=torch.float32, device=DEV)
    ops.conv_wgrad(dt, OP, X.to_view(x.double(), dt), X.to_view(dy.double(), dt), Cin, Cout, dw, ws=ws)
    torch.cuda.synchronize()
    return yv.t.clone(), st.clone(), dxv.t.clone(), dw


@pytest.mark.parametrize("dt", DTS)
def test_conv3r_runs_are_bit_identical(dt):
    """no atomics anywhere: two runs of each pass on Gaussian data give the same bits"""
    shape = SHAPES[2]
    N, H, W, Cin, Cout = shape
    x, w, b, dy = _gauss((N, Cin, H, W), 1), _gauss_weight(Cin, Cout, 2), _gauss((Cout,), 3), _gauss((N, Cout, H, W), 4)
    ws = X.new_wgrad_ws(DEV)
    a, c = _run_all(dt, shape, x, w, b, dy, ws), _run_all(dt, shape, x, w, b, dy, ws)
    for name, p, q in zip(("forward", "statistics", "input gradient", "weight gradient"), a, c):
        assert p.abs().sum().item() > 0 and torch.equal(p, q), f"{name}: two runs differ"


@pytest.mark.parametrize("dt", DTS)
def test_conv3r_batch_invariant_image(dt):
    """batch-invariant mode: image 0 alone and image 0 inside N = 5 give equal forward (with statistics) and input-gradient bits"""
    shape = SHAPES[3]
    N, H, W, Cin, Cout = shape
    x, w, b, dy = _gauss((N, Cin, H, W), 5), _gauss_weight(Cin, Cout, 6), _gauss((Cout,), 7), _gauss((N, Cout, H, W), 8)
    ws = X.new_wgrad_ws(DEV)
    with ops.batch_invariant_scope(True):
        full = _run_all(dt, shape, x, w, b, dy, ws)
        one = _run_all(dt, shape, x[:1].contiguous(), w, b, dy[:1].contiguous(), ws)
    for name, a, p in list(zip(("forward", "statistics", "input gradient"), full, one)):
        assert a[:1].abs().sum().item() > 0
        assert torch.equal(a[:1], p), f"{name}: image 0 of the batch differs from the same image run alone"


def test_conv3r_refuses_a_one_pixel_axis():
    """H = 1 (or W = 1) cannot be reflect-padded by 1, as torch refuses it: an error of the entry point that names H and W"""
    pk = ops.pack_weight(DT_BF16, OP, 0, torch.zeros((32, 32, 4, 4), device=DEV), 32, 32)
    for h, w in ((1, 4), (4, 1)):
        x = View(torch.zeros((1, h, w, 32), dtype=torch.bfloat16, device=DEV), 32)
        y = View(torch.zeros((1, h, w, 32), dtype=torch.bfloat16, device=DEV), 32)
        with pytest.raises(T.TfcError, match=rf"H=.*W=|H={h} W={w}") as e:
            ops.conv_fwd(DT_BF16, OP, x, 32, 32, pk, y)
        assert f"H={h}" in str(e.value) and f"W={w}" in str(e.value)
