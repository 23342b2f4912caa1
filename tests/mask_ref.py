"""Torch restatement of the edge mask of TFCGAN_multigpu_patchFFT_experiment.py ("4X") :385-390, usable in fp32 and fp64 and differentiable by autograd:

    mask      = K.filters.laplacian(K.color.rgb_to_grayscale(img), 7).abs()
    mask_norm = (mask - mask.min()) / (mask.max() - mask.min())
    mask_blur = K.filters.gaussian_blur2d(mask_norm, (9, 9), (1.6, 1.6))
    mask_blur = mask_blur / mask_blur.max()

kornia is not installed; its three functions are restated from their documented definitions (parity with kornia itself is not pinned):
    rgb_to_grayscale : 0.299 R + 0.587 G + 0.114 B
    laplacian(x, 7)  : 7x7 kernel of ones with centre 1 - 49, divided by the sum of its absolute values (96), border "reflect"
    gaussian_blur2d  : separable 9 taps exp(-x^2 / (2 sigma^2)), x = -4..4, normalised to sum 1, border "reflect"
`K` below is the stand-in namespace the fixture generator hands to the lifted `mask_maker`.

The explicit gather adjoints at the bottom are the formula csrc/mask.hip implements for the backward of the two reflect-padded filters.
"""
import types

import torch
import torch.nn.functional as F

GRAY = (0.299, 0.587, 0.114)
LAP_K, LAP_PAD = 7, 3
GAUSS_K, GAUSS_PAD, SIGMA = 9, 4, 1.6


def laplacian_kernel(dtype=torch.float64):
    k = torch.ones(LAP_K, LAP_K, dtype=dtype)
    k[LAP_PAD, LAP_PAD] = 1 - LAP_K * LAP_K
    return k / k.abs().sum()


def gaussian_taps(dtype=torch.float64):
    x = torch.arange(GAUSS_K, dtype=dtype) - GAUSS_PAD
    g = torch.exp(-x * x / (2 * SIGMA * SIGMA))
    return g / g.sum()


def rgb_to_grayscale(img):
    return GRAY[0] * img[:, 0:1] + GRAY[1] * img[:, 1:2] + GRAY[2] * img[:, 2:3]


def laplacian(x, kernel_size=7):
    assert kernel_size == LAP_K
    k = laplacian_kernel(x.dtype).to(x.device)
    return F.conv2d(F.pad(x, (LAP_PAD,) * 4, mode="reflect"), k[None, None])


def gaussian_blur2d(x, kernel_size=(9, 9), sigma=(1.6, 1.6)):
    assert tuple(kernel_size) == (GAUSS_K, GAUSS_K) and tuple(sigma) == (SIGMA, SIGMA)
    g = gaussian_taps(x.dtype).to(x.device)
    return F.conv2d(F.pad(x, (GAUSS_PAD,) * 4, mode="reflect"), torch.outer(g, g)[None, None])


K = types.SimpleNamespace(color=types.SimpleNamespace(rgb_to_grayscale=rgb_to_grayscale),
                          filters=types.SimpleNamespace(laplacian=laplacian, gaussian_blur2d=gaussian_blur2d))


def mask_parts(img):
    """every stage of the operator: dict(lap, L, mn, mx, Mn, Bl, M, mask)"""
    lap = laplacian(rgb_to_grayscale(img), 7)
    L = lap.abs()
    mn, mx = L.min(), L.max()
    Mn = (L - mn) / (mx - mn)
    Bl = gaussian_blur2d(Mn, (9, 9), (1.6, 1.6))
    M = Bl.max()
    return {"lap": lap, "L": L, "mn": mn, "mx": mx, "Mn": Mn, "Bl": Bl, "M": M, "mask": Bl / M}


def mask_maker(img):
    return mask_parts(img)["mask"]


def mask_l1(fake, real, scale=1.0):
    return scale * (mask_maker(fake) - mask_maker(real)).abs().mean()


def mask_vjp(img, dout):
    """autograd's gradient of sum(dout * mask_maker(img)) w.r.t. img (torch's full-tensor min() / max() split a tie evenly)"""
    x = img.detach().clone().requires_grad_(True)
    (mask_maker(x) * dout).sum().backward()
    return x.grad


def mask_l1_grad(fake, real, scale=1.0):
    x = fake.detach().clone().requires_grad_(True)
    loss = mask_l1(x, real, scale)
    loss.backward()
    return loss.detach(), x.grad


# ---- the two filters as plain operators on one [H,W] plane, and their explicit gather adjoints ------------------------------------------------
def box7(x):
    """S49 - 49 x over 96 is the Laplacian; this is the reflect-padded 7x7 box SUM alone"""
    return F.conv2d(F.pad(x[None, None], (LAP_PAD,) * 4, mode="reflect"), torch.ones(1, 1, LAP_K, LAP_K, dtype=x.dtype))[0, 0]


def lap_op(x):
    return laplacian(x[None, None])[0, 0]


def gauss_op(x):
    return gaussian_blur2d(x[None, None])[0, 0]


def adjoint_1d(y, taps, dim):
    """adjoint of the reflect-padded correlation with symmetric `taps` (length 2p+1) along `dim`, as a gather:
        x'[j] = sum_d w[d] (y0[j-d] + [j >= 1] y0[-j-d] + [j <= n-2] y0[2n-2-j-d]),   y0 = y extended by zeros
    the two extra terms fold what the padding copied from pixel j back onto it."""
    y = y.movedim(dim, -1)
    n, p = y.shape[-1], (len(taps) - 1) // 2
    out = torch.zeros_like(y)

    def y0(i):
        return y[..., i] if 0 <= i < n else torch.zeros_like(y[..., 0])

    for j in range(n):
        acc = torch.zeros_like(y[..., 0])
        for d in range(-p, p + 1):
            w = taps[d + p]
            acc = acc + w * y0(j - d)
            if j >= 1:
                acc = acc + w * y0(-j - d)
            if j <= n - 2:
                acc = acc + w * y0(2 * n - 2 - j - d)
        out[..., j] = acc
    return out.movedim(-1, dim)


def lap_adjoint(y):
    ones = torch.ones(LAP_K, dtype=y.dtype)
    return (adjoint_1d(adjoint_1d(y, ones, 1), ones, 0) - LAP_K * LAP_K * y) / 96


def gauss_adjoint(y):
    g = gaussian_taps(y.dtype)
    return adjoint_1d(adjoint_1d(y, g, 1), g, 0)
