"""Bit-exact tests of TFC_OP_CONV2 = nn.Conv2d(Cin, Cout, 4, stride=2, padding=1), all three passes, in every compute mode (method: tests/conv_exact.py).

Operands are small integers (the bias: half-integers), so every partial sum is exact in fp32 in any order and the stored value must equal the rounding
of a float64 F.conv2d(stride=2, padding=1) or of its adjoints: torch.equal, no tolerance. The shapes are the smallest that reach each branch of the
stride-2 paths; the batch-invariance and run-to-run tests use Gaussian data, where a different order of additions would change bits.

The LeakyReLU of the convolution epilogue has the fixed slope 0.2 of TFC_EP_LEAKY; it is one fp32 multiply and a maximum, which conv_exact.leaky_f32
reproduces bit for bit, so the comparison stays torch.equal.
"""
import ctypes
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
OP = getattr(_lib, "OP_CONV2", None)         # None before the op exists: every test then fails at its first call

# (N, H, W, Cin, Cout)
SHAPES = [(3, 6, 6, 6, 64),                  # one partial 8 x 16 tile; the first layer's channel padding (6 -> 8)
          (2, 18, 34, 64, 128),              # output 9 x 17: one tile plus a ragged row and column
          (1, 32, 32, 256, 512),             # layer-4 channels, several K chunks
          (13, 4, 4, 128, 256)]              # output 2 x 2: a prime batch, an image smaller than a tile
DTS = [pytest.param(DT_BF16, id="bf16"), pytest.param(DT_F32, id="fp32"), pytest.param(DT_BF16X3, id="bf16x3")]
_ids = [f"N{n}-{h}x{w}-{ci}to{co}" for n, h, w, ci, co in SHAPES]


@pytest.fixture(autouse=True)
def engine_dispatch():
    _lib.check(_lib.load().tfc_debug_set_igemm_config(-1), "tfc_debug_set_igemm_config")
    yield


def seed(shape, k):
    return zlib.crc32(f"conv2.{shape}.{k}".encode())


def ref(x, w):
    return F.conv2d(x, w, stride=2, padding=1)


def f32(t):
    return None if t is None else t.to(torch.float32).contiguous()


def _stats_exact(got, stats, what):
    """the statistics epilogue adds the STORED values and their squares in fp32: exact, in any order, while the sum of magnitudes stays below 2^24 quanta
    (values are multiples of 1/2, squares of 1/4) -- asserted on the data, then the sums are compared with =="""
    g = got.double()
    for k, s, a, q in ((0, g.sum((2, 3)), g.abs().sum((2, 3)), 2), (1, (g * g).sum((2, 3)), (g * g).sum((2, 3)), 4)):
        assert (a * q).max().item() < X.EXACT_BOUND, f"{what}: statistics {k} leave the exact range ({(a * q).max().item():.0f} quanta): shrink the data"
        X.assert_exact(stats[..., k].double(), s, f"{what} statistics {k}", X.VEC_DIMS)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_exact_conv2_fwd(shape, dt):
    """forward with TFC_EP_BIAS, TFC_EP_BIAS | TFC_EP_LEAKY and TFC_EP_BIAS | TFC_EP_STATS (the statistics of the stride-2 output, exactly)"""
    _check_fwd(shape, dt)


def _check_fwd(shape, dt):
    N, H, W, Cin, Cout = shape
    x = X.ints((N, Cin, H, W), seed(shape, 0), device=DEV)
    w = X.ints((Cout, Cin, 4, 4), seed(shape, 1), device=DEV)
    b = X.ints((Cout,), seed(shape, 2), device=DEV) / 2
    z = ref(x, w)
    X.assert_dyadic(z, 1, "forward reference")
    assert tuple(z.shape[2:]) == (ops.OUT_HW[OP](H), ops.OUT_HW[OP](W))
    v32 = X.store(z + b.view(1, -1, 1, 1), DT_F32)
    xv = X.to_view(x, dt)
    pk = ops.pack_weight(dt, OP, 0, f32(w), Cin, Cout)
    for name, flags, want32 in (("bias", 0, v32), ("bias|leaky", ops.EP_LEAKY, X.leaky_f32(v32, 0.2)), ("bias|stats", 0, v32)):
        want = want32.to(ops.torch_dtype(dt))
        yv = View(torch.full((N, H // 2, W // 2, ops.pad8(Cout)), X.SENTINEL, dtype=ops.torch_dtype(dt), device=DEV), Cout)
        stats = torch.zeros((N, Cout, 2), dtype=torch.float32, device=DEV) if name == "bias|stats" else None
        ops.conv_fwd(dt, OP, xv, Cin, Cout, pk, yv, bias=f32(b), stats=stats, flags=flags)
        torch.cuda.synchronize()
        got = X.from_view(yv)
        X.assert_exact(got, want, f"conv2 {shape} forward ({name})")
        if stats is not None:
            _stats_exact(got, stats, f"conv2 {shape}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_exact_conv2_dgrad(shape, dt):
    """input gradient, plain (the destination holds garbage) and with TFC_EP_ACCUM (the rounded product is added to the stored value, rounded again)"""
    _check_dgrad(shape, dt)


# The default dispatch picks small-grid tile forms at these batches. At batch 32 the discriminator's layers run the persistent kernel in form 3
# (<4,1,1,4>: layers 2-4 forward, layers 3-4 dgrad) and form 1 (<2,1,2,2>: the 64 -> 128 dgrad); the test hook forces those forms onto the small shapes.
FORCED = [pytest.param(3, 2, id="form3-256to512"), pytest.param(3, 3, id="form3-128to256"), pytest.param(1, 1, id="form1-64to128")]


@pytest.mark.parametrize("cfg,si", FORCED)
def test_exact_conv2_fwd_dgrad_bf16_production_tile_forms(cfg, si):
    """the tile forms the layers take at batch 32, forced through tfc_debug_set_igemm_config: forward with every epilogue, dgrad plain and accumulating"""
    lib = _lib.load()
    q = (ctypes.c_int * 8)()
    N, H, W, Cin, Cout = SHAPES[si]
    _lib.check(lib.tfc_debug_set_igemm_config(cfg), "tfc_debug_set_igemm_config")
    try:
        for pas in (0, 1):                                        # the hook took: the plan reports the persistent kernel in the forced form
            assert lib.tfc_conv_plan_query(DT_BF16, OP, pas, N, H, W, Cin, Cout, ops.EP_BIAS if pas == 0 else 0, 256, q, 8) == 8
            assert (q[0], q[1]) == (1, cfg), (pas, list(q))
        _check_fwd(SHAPES[si], DT_BF16)
        _check_dgrad(SHAPES[si], DT_BF16)
    finally:
        _lib.check(lib.tfc_debug_set_igemm_config(-1), "tfc_debug_set_igemm_config")


def _check_dgrad(shape, dt):
    N, H, W, Cin, Cout = shape
    w = X.ints((Cout, Cin, 4, 4), seed(shape, 1), device=DEV)
    dy = X.ints((N, Cout, H // 2, W // 2), seed(shape, 3), device=DEV)
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
    X.assert_exact(X.from_view(dxv), v, f"conv2 {shape} input gradient")
    dxv = X.to_view(base, dt)
    ops.conv_dgrad(dt, OP, dyv, N, H, W, Cin, Cout, pkd, dxv, accumulate=True)
    torch.cuda.synchronize()
    X.assert_exact(X.from_view(dxv), X.store(v.double() + base, dt), f"conv2 {shape} accumulated input gradient")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_exact_conv2_wgrad(shape, dt):
    """weight gradient into a guarded slice of a flat buffer, plain and accumulating; the workspace's accumulator is all-zero again afterwards. bf16:
    one launch of the transposed convolution's phase-fused kernel with the two tensors exchanged; fp32 / bf16x3: one launch per parity plane"""
    _check_wgrad(shape, dt)


@pytest.mark.parametrize("shape", SHAPES[:2], ids=_ids[:2])
def test_exact_conv2_wgrad_bf16_per_plane_launches(shape):
    """bf16 through the four per-plane launches (what a layer too large for the fused kernel's slabs falls back to): test config 2 declines the fused
    launch, as it does for the transposed convolution"""
    _lib.check(_lib.load().tfc_debug_set_igemm_config(2), "tfc_debug_set_igemm_config")
    try:
        _check_wgrad(shape, DT_BF16)
    finally:
        _lib.check(_lib.load().tfc_debug_set_igemm_config(-1), "tfc_debug_set_igemm_config")


def _check_wgrad(shape, dt):
    N, H, W, Cin, Cout = shape
    x = X.ints((N, Cin, H, W), seed(shape, 5), device=DEV)
    dy = X.ints((N, Cout, H // 2, W // 2), seed(shape, 6), device=DEV)
    w0 = torch.zeros((Cout, Cin, 4, 4), dtype=torch.float64, device=DEV, requires_grad=True)
    (gw,) = torch.autograd.grad(ref(x, w0), w0, dy)
    X.assert_dyadic(gw, 1, "weight-gradient reference")
    ws = X.new_wgrad_ws(DEV)
    xv, dyv = X.to_view(x, dt), X.to_view(dy, dt)
    flat, dw = X.grad_slice((Cout, Cin, 4, 4), 7.0, DEV)
    ops.conv_wgrad(dt, OP, xv, dyv, Cin, Cout, dw, ws=ws)
    torch.cuda.synchronize()
    X.assert_exact(dw, X.store(gw, DT_F32), f"conv2 {shape} weight gradient", X.WGT_DIMS)
    X.assert_slice_guarded(flat, "weight gradient")
    assert int((X.ws_accumulator(ws) != 0).sum()) == 0, "the workspace accumulator is not all-zero after the call"
    base = X.ints((Cout, Cin, 4, 4), seed(shape, 7), amp=X.WGRAD_BASE_AMP, device=DEV)
    flat, dw = X.grad_slice((Cout, Cin, 4, 4), f32(base), DEV)
    ops.conv_wgrad(dt, OP, xv, dyv, Cin, Cout, dw, accumulate=True, ws=ws)
    torch.cuda.synchronize()
    X.assert_exact(dw, X.store(gw + base, DT_F32), f"conv2 {shape} accumulated weight gradient", X.WGT_DIMS)
    X.assert_slice_guarded(flat, "accumulated weight gradient")
    assert int((X.ws_accumulator(ws) != 0).sum()) == 0, "the workspace accumulator is not all-zero after the accumulating call"


def test_conv2_refuses_an_odd_size():
    """an odd H or W is an error of the entry point, not a wrong shape"""
    x = View(torch.zeros((1, 5, 6, 8), dtype=torch.bfloat16, device=DEV), 8)
    y = View(torch.zeros((1, 2, 3, 8), dtype=torch.bfloat16, device=DEV), 8)
    pk = ops.pack_weight(DT_BF16, OP, 0, torch.zeros((8, 8, 4, 4), device=DEV), 8, 8)
    with pytest.raises(T.TfcError, match="even"):
        ops.conv_fwd(DT_BF16, OP, x, 8, 8, pk, y)
    x = View(torch.zeros((1, 6, 5, 8), dtype=torch.bfloat16, device=DEV), 8)
    with pytest.raises(T.TfcError, match="even"):
        ops.conv_fwd(DT_BF16, OP, x, 8, 8, pk, y)


def _gauss(shape, s):
    g = torch.Generator().manual_seed(s)
    return torch.randn(shape, generator=g, dtype=torch.float32).to(DEV)


@pytest.mark.parametrize("dt", DTS[:2])
def test_conv2_batch_invariant_rows(dt):
    """batch-invariant mode: samples 5..8 of the 13-batch case have the bits of the same samples run alone, forward (with statistics) and dgrad"""
    N, H, W, Cin, Cout = SHAPES[3]
    x, w, b = _gauss((N, Cin, H, W), 1), _gauss((Cout, Cin, 4, 4), 2) * 0.05, _gauss((Cout,), 3)
    dy = _gauss((N, Cout, H // 2, W // 2), 4)

    def run(xs, dys):
        n = xs.shape[0]
        yv = ops.new_act(n, H // 2, W // 2, Cout, dt, DEV)
        st = torch.zeros((n, Cout, 2), dtype=torch.float32, device=DEV)
        ops.conv_fwd(dt, OP, X.to_view(xs.double(), dt), Cin, Cout, ops.pack_weight(dt, OP, 0, w, Cin, Cout), yv, bias=b, stats=st)
        dxv = ops.new_act(n, H, W, Cin, dt, DEV)
        ops.conv_dgrad(dt, OP, X.to_view(dys.double(), dt), n, H, W, Cin, Cout, ops.pack_weight(dt, OP, 1, w, Cin, Cout), dxv)
        torch.cuda.synchronize()
        return yv.t.clone(), st.clone(), dxv.t.clone()

    with ops.batch_invariant_scope(True):
        full = run(x, dy)
        part = run(x[5:9].contiguous(), dy[5:9].contiguous())
    for name, a, p in zip(("forward", "statistics", "input gradient"), full, part):
        assert a[5:9].abs().sum().item() > 0
        assert torch.equal(a[5:9], p), f"{name}: rows 5..8 of the batch differ from the same samples run alone"


@pytest.mark.parametrize("dt", DTS)
def test_conv2_wgrad_runs_are_bit_identical(dt):
    """no float atomics: two weight-gradient runs on Gaussian data give the same bits"""
    N, H, W, Cin, Cout = SHAPES[1]
    xv = X.to_view(_gauss((N, Cin, H, W), 5).double(), dt)
    dyv = X.to_view(_gauss((N, Cout, H // 2, W // 2), 6).double(), dt)
    ws = X.new_wgrad_ws(DEV)
    outs = []
    for _ in range(2):
        dw = torch.empty((Cout, Cin, 4, 4), dtype=torch.float32, device=DEV)
        ops.conv_wgrad(dt, OP, xv, dyv, Cin, Cout, dw, ws=ws)
        torch.cuda.synchronize()
        outs.append(dw)
    assert outs[0].abs().sum().item() > 0 and torch.equal(outs[0], outs[1])
