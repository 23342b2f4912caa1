"""Plain float64 restatements of the five kernels of csrc/lpips.hip, shared by tests/test_gpu_48_lpips_edges.py and tests/test_gpu_31_lpips.py
(against the kernels) and tests/test_lpips_host.py (against torch on the CPU). Every tensor is NCHW here, whatever layout the kernels use; nothing
of the package is imported and nothing touches a GPU.

    head_ref        value per image and d (gscale * sum_n value_n) / d fx, the gradient WRITTEN OUT (not autograd), with the kernel's documented
                    convention at an all-zero fx pixel
    maxpool_ref     2x2 / stride 2 forward; backward to the first maximum of the window in row-major order
    relu_bwd_ref    (y > 0) ? dy (+ extra) : 0
    input_ref       (x - shift[c]) / scale[c];  input_bwd_ref  alpha * g / scale[c] (+ dx)
    f32_interval    the fp32 numbers within k fp32 ulp of a float64 value: what "k ulp of fp32 arithmetic, then one rounding" is tested with
"""
import torch

EPS = 1e-10                                                       # lpips_pytorch's normalize_activation: x / (sqrt(sum_c x^2) + 1e-10)


def head_ref(fx, fy, w, gscale):
    """fx, fy [N,C,H,W], w [C], all float64 -> (value [N], dfx [N,C,H,W]).
    value_n = mean_pixels sum_c w_c d_c^2,  d = fx / a_x - fy / a_y,  a = r + EPS,  r = sqrt(sum_c f_c^2).
    dfx_j = s * (g_j / a_x - fx_j * (sum_c g_c fx_c) / (r_x a_x^2)),  g_c = 2 w_c d_c,  s = gscale / (H W): from d n_c / d x_j = delta_cj / a -
    x_c x_j / (r a^2). At r_x == 0 the second (norm) term is DEFINED as 0 (every x_c is 0 there; its limit does not exist), leaving
    s * 2 w_j d_j / EPS with d_j = -fy_j / a_y: the form the kernel documents."""
    assert fx.dtype == fy.dtype == w.dtype == torch.float64
    N, C, H, W = fx.shape
    wc = w.view(1, C, 1, 1)
    rx, ry = fx.pow(2).sum(1, keepdim=True).sqrt(), fy.pow(2).sum(1, keepdim=True).sqrt()
    ax, ay = rx + EPS, ry + EPS
    d = fx / ax - fy / ay
    value = (wc * d * d).sum(1).mean((1, 2))
    g = 2.0 * wc * d
    dot = (g * fx).sum(1, keepdim=True)
    zero = rx == 0
    k2 = torch.where(zero, torch.zeros_like(dot), dot / torch.where(zero, torch.ones_like(rx), rx * ax * ax))
    dfx = (gscale / (H * W)) * (g / ax - fx * k2)
    return value, dfx


def zero_pixels(fx):
    """[N,1,H,W] bool: the pixels whose feature vector is all zero"""
    return fx.pow(2).sum(1, keepdim=True) == 0


def _windows(x):
    """the four members of every 2x2 window in row-major order: [4, N, C, H/2, W/2]"""
    return torch.stack((x[..., 0::2, 0::2], x[..., 0::2, 1::2], x[..., 1::2, 0::2], x[..., 1::2, 1::2]))


def maxpool_ref(x, dy=None):
    """x [N,C,H,W] (H, W even) -> y [N,C,H/2,W/2], and with dy (y's shape) also dx: dy lands on the FIRST member, in row-major order, that equals
    the maximum; every other member gets 0. The maximum is found by a scan that replaces the running maximum only by a GREATER value, as torch's
    is: of equal values (-0.0 and +0.0 among them) the first one seen is the result."""
    v = _windows(x)
    m = v[0].clone()
    for k in range(1, 4):
        m = torch.where(v[k] > m, v[k], m)
    if dy is None:
        return m
    taken = torch.zeros_like(m, dtype=torch.bool)
    dx = torch.zeros_like(x)
    for k, (i, j) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        hit = ~taken & (v[k] == m)
        dx[..., i::2, j::2] = torch.where(hit, dy, torch.zeros_like(dy))
        taken |= hit
    return m, dx


def relu_bwd_ref(dy, y, extra=None):
    g = dy if extra is None else dy + extra
    return torch.where(y > 0, g, torch.zeros_like(g))


def input_ref(x, shift, scale):
    """x [N,C,H,W], shift, scale [C] -> (x - shift) / scale"""
    C = x.shape[1]
    return (x - shift.view(1, C, 1, 1)) / scale.view(1, C, 1, 1)


def input_bwd_ref(g, scale, alpha=1.0, dx=None):
    """g [N,C,H,W] -> alpha * g / scale (+ dx)"""
    v = alpha * g / scale.view(1, g.shape[1], 1, 1)
    return v if dx is None else dx + v


def f32_interval(ref, ulps=2):
    """ref float64 -> (lo, hi) float32: the smallest and the largest fp32 number inside [ref - ulps * u, ref + ulps * u], u = the fp32 ulp of
    ref's binade (2^(e - 23), e = floor(log2 |ref|), not below the subnormal spacing 2^-149). A result of fp32 arithmetic that is within `ulps`
    ulp of ref lies in [lo, hi]; because rounding is monotone, whatever is then done to it by ONE further rounding (a bf16 store, an fp32 add of
    a known number) lies between the same operation applied to lo and to hi."""
    assert ref.dtype == torch.float64
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))
    u = torch.pow(torch.full_like(ref, 2.0), e - 23).clamp_min(2.0 ** -149)
    lo64, hi64 = ref - ulps * u, ref + ulps * u
    lo, hi = lo64.float(), hi64.float()
    lo = torch.where(lo.double() < lo64, torch.nextafter(lo, torch.full_like(lo, float("inf"))), lo)
    hi = torch.where(hi.double() > hi64, torch.nextafter(hi, torch.full_like(hi, float("-inf"))), hi)
    return lo, hi
