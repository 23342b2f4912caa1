"""The float64 restatements of tests/lpips_ref.py against torch on the CPU (float64 autograd, F.max_pool2d, F.relu), on random inputs with ties:
what tests/test_gpu_48_lpips_edges.py holds the kernels of csrc/lpips.hip against is itself held against torch here. No GPU."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import lpips_ref as R


def rnd64(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape))


def levels(shape, seed):
    """five levels spanning both signs: ties, four-way ties and all-negative windows occur"""
    return torch.from_numpy(np.random.default_rng(seed).integers(-2, 3, shape).astype(np.float64) * 0.25)


def torch_head(fx, fy, w):
    """the package's normalize_activation / squared difference / 1x1 conv / spatial mean, as tests/test_gpu_31_lpips.py restates it"""
    nx = fx / (fx.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    ny = fy / (fy.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    return F.conv2d((nx - ny) ** 2, w.view(1, -1, 1, 1)).mean((2, 3)).reshape(-1)


def test_head_ref_vs_autograd_away_from_zero_vectors():
    for (N, C, H, W), gscale in (((2, 8, 3, 5), 0.7), ((3, 24, 5, 7), -2.0), ((1, 64, 2, 2), 1.0)):
        fx = rnd64((N, C, H, W), 1).clamp_min(0)                    # post-ReLU features: many exact zeros, but (below) no all-zero vector
        fx[:, 0] += 0.05
        fy = rnd64((N, C, H, W), 2).clamp_min(0)
        fy[0, :, 0, 0] = 0                                          # an all-zero fy vector is harmless: n_y = 0 / 1e-10 = 0
        w = torch.from_numpy(np.random.default_rng(3).random(C))
        fx.requires_grad_(True)
        want = torch_head(fx, fy, w)
        (gx,) = torch.autograd.grad(want.sum() * gscale, fx)
        val, dfx = R.head_ref(fx.detach(), fy, w, gscale)
        assert not R.zero_pixels(fx.detach()).any()
        assert torch.allclose(val, want.detach(), rtol=1e-12, atol=0)
        assert (dfx - gx).abs().max().item() <= 1e-11 * gx.abs().max().item()


def test_head_ref_at_a_zero_vector_is_the_documented_analytic_form():
    N, C, H, W, gscale = 2, 8, 3, 5, 0.7
    fx, fy = rnd64((N, C, H, W), 4).clamp_min(0) + 0.01, rnd64((N, C, H, W), 5).clamp_min(0) + 0.01
    w = torch.from_numpy(np.random.default_rng(6).random(C))
    base_val, base = R.head_ref(fx, fy, w, gscale)
    fx[1, :, 2, 4] = 0
    val, dfx = R.head_ref(fx, fy, w, gscale)
    assert R.zero_pixels(fx).sum().item() == 1 and torch.isfinite(dfx).all() and torch.isfinite(val).all()
    ny = fy[1, :, 2, 4] / (fy[1, :, 2, 4].pow(2).sum().sqrt() + 1e-10)
    want = (gscale / (H * W)) * 2.0 * w * (-ny) / 1e-10            # s * 2 w_c d_c / a, d_c = -n_y,c, a = 1e-10, norm term 0
    assert torch.allclose(dfx[1, :, 2, 4], want, rtol=1e-14, atol=0)
    assert dfx[1, :, 2, 4].abs().max().item() > 1e6                 # the 1e10-sized entries the GPU tests keep apart from the rest
    other = torch.ones(N, 1, H, W, dtype=torch.bool)
    other[1, 0, 2, 4] = False
    assert torch.equal(dfx * other, base * other) and torch.equal(val[0], base_val[0])       # pixels are independent
    # the value of a zero pixel is sum_c w_c n_y,c^2
    zero_only = torch.zeros_like(fx)
    v0, _ = R.head_ref(zero_only, fy, w, gscale)
    ny_all = fy / (fy.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    assert torch.allclose(v0, (w.view(1, C, 1, 1) * ny_all ** 2).sum(1).mean((1, 2)), rtol=1e-13, atol=0)


def test_maxpool_ref_vs_torch_with_ties():
    for N, C, H, W in ((1, 8, 2, 2), (3, 24, 6, 10), (2, 5, 14, 18)):
        x = levels((N, C, H, W), 7).requires_grad_(True)
        y = F.max_pool2d(x, 2, 2)
        dy = rnd64(tuple(y.shape), 8)
        (gx,) = torch.autograd.grad(y, x, dy)
        m, dx = R.maxpool_ref(x.detach(), dy)
        assert torch.equal(m, y.detach()) and torch.equal(dx, gx)
        assert torch.equal(R.maxpool_ref(x.detach()), m)
    v = R._windows(x.detach())
    assert ((v == v[0]).all(0)).any() and (v.max(0).values < 0).any()          # the data has four-way ties and all-negative windows


def test_maxpool_ref_signed_zeros_as_torch():
    x = torch.tensor([[-0.0, 0.0, 0.0, -0.0, -0.5, -0.0], [-0.0, 0.0, -0.0, -0.0, 0.0, -0.5]], dtype=torch.float64).reshape(1, 1, 2, 6)
    x = x.repeat(1, 8, 1, 1).requires_grad_(True)
    y = F.max_pool2d(x, 2, 2)
    dy = rnd64(tuple(y.shape), 9)
    (gx,) = torch.autograd.grad(y, x, dy)
    m, dx = R.maxpool_ref(x.detach(), dy)
    assert torch.equal(m, y.detach()) and torch.equal(torch.signbit(m), torch.signbit(y.detach())) and torch.equal(dx, gx)


def test_relu_bwd_ref_vs_autograd():
    z = levels((4, 8, 5, 6), 10)                                    # exact zeros (and negatives) in z
    z[0, 0, 0, 0] = -0.0
    z.requires_grad_(True)
    y = F.relu(z)
    g1, g2 = rnd64(tuple(z.shape), 11), rnd64(tuple(z.shape), 12)
    (a,) = torch.autograd.grad(y, z, g1, retain_graph=True)
    (b,) = torch.autograd.grad(y, z, g1 + g2)
    assert (y.detach() == 0).any()
    assert torch.equal(R.relu_bwd_ref(g1, y.detach()), a) and torch.equal(R.relu_bwd_ref(g1, y.detach(), g2), b)
    yz = torch.tensor([0.0, -0.0, 1.0, -1.0], dtype=torch.float64)
    assert R.relu_bwd_ref(torch.ones(4, dtype=torch.float64), yz).tolist() == [0.0, 0.0, 1.0, 0.0]


def test_input_ref_vs_autograd():
    for C in (1, 3, 8):
        x = rnd64((2, C, 7, 5), 13).requires_grad_(True)
        shift, scale = rnd64((C,), 14) * 0.3, torch.from_numpy(np.random.default_rng(15).random(C)) + 0.3
        y = (x - shift.view(1, C, 1, 1)) / scale.view(1, C, 1, 1)
        g = rnd64(tuple(y.shape), 16)
        (gx,) = torch.autograd.grad(y, x, g * -0.5)
        assert torch.equal(R.input_ref(x.detach(), shift, scale), y.detach())
        assert torch.allclose(R.input_bwd_ref(g, scale, -0.5), gx, rtol=1e-15, atol=0)
        dx0 = rnd64(tuple(x.shape), 17)
        assert torch.allclose(R.input_bwd_ref(g, scale, -0.5, dx0), dx0 + gx, rtol=1e-14, atol=1e-15)


def test_f32_interval_is_the_set_of_fp32_numbers_within_k_ulp():
    ref = torch.cat((rnd64((4096,), 18), rnd64((4096,), 19) * 1e-3, torch.tensor([1.0, -1.0, 0.5, 2.0 ** -130, 0.0, 1.0 + 2.0 ** -30])))
    lo, hi = R.f32_interval(ref, 2)
    f = ref.float()
    assert (lo <= f).all() and (f <= hi).all()
    u = torch.pow(torch.full_like(ref, 2.0), torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 23).clamp_min(2.0 ** -149)
    assert ((ref - lo.double()) <= 2 * u).all() and ((hi.double() - ref) <= 2 * u).all()
    below, above = torch.nextafter(lo, torch.full_like(lo, float("-inf"))), torch.nextafter(hi, torch.full_like(hi, float("inf")))
    assert ((ref - below.double()) > 2 * u).all() and ((above.double() - ref) > 2 * u).all()     # the interval is tight
    one = torch.tensor([1.0], dtype=torch.float64)
    lo1, hi1 = R.f32_interval(one, 2)
    assert lo1.item() == 1.0 - 2.0 ** -22 and hi1.item() == 1.0 + 2.0 ** -22
