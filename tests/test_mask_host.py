"""Host-side tests of the edge-mask configuration MASK-4: the filters of the restatement tests/mask_ref.py, the explicit gather adjoints that
csrc/mask.hip implements for its backward, the fixtures lifted from the reference script, the generator's key list, the script weights and the
exported symbols. No GPU."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import tfc_gan_amd as T
from oracle import tfcgan_oracle as O
from tests import mask_ref as R
from tfc_gan_amd import _lib


def test_filter_taps():
    k = R.laplacian_kernel()
    assert abs(float(k.sum())) <= 1e-15 and abs(float(k.abs().sum()) - 1.0) <= 1e-15
    assert float(k[3, 3]) == -48.0 / 96.0 and float(k[0, 0]) == 1.0 / 96.0
    g = R.gaussian_taps()
    assert abs(float(g.sum()) - 1.0) <= 1e-15 and len(g) == 9 and torch.equal(g, g.flip(0))
    assert abs(float(g[4] / g[3]) - float(np.exp(1 / (2 * 1.6 * 1.6)))) <= 1e-12


def test_gather_adjoints_are_the_transposes_of_the_reflect_padded_filters():
    """<A x, y> = <x, A^T y> in fp64 on a 19 x 37 plane for both filters; and the forward operator used as its own transpose is NOT (border)"""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(19, 37, dtype=torch.float64, generator=g)
    y = torch.randn(19, 37, dtype=torch.float64, generator=g)
    for op, adj in ((R.lap_op, R.lap_adjoint), (R.gauss_op, R.gauss_adjoint)):
        lhs, rhs = float((op(x) * y).sum()), float((x * adj(y)).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), (lhs, rhs)
        # against autograd, entry by entry
        xx = x.clone().requires_grad_(True)
        (op(xx) * y).sum().backward()
        assert float((xx.grad - adj(y)).abs().max()) <= 1e-13
        wrong = float((op(y) - adj(y)).norm() / adj(y).norm())
        interior = float((op(y) - adj(y))[8:-8, 8:-8].abs().max())
        assert wrong > 1e-2 and interior <= 1e-13, (wrong, interior)
    # 8 x 8: both folds of the blur land on the same pixels
    x8 = torch.randn(8, 8, dtype=torch.float64, generator=g)
    y8 = torch.randn(8, 8, dtype=torch.float64, generator=g)
    for op, adj in ((R.lap_op, R.lap_adjoint), (R.gauss_op, R.gauss_adjoint)):
        assert abs(float((op(x8) * y8).sum()) - float((x8 * adj(y8)).sum())) <= 1e-12


def test_extrema_terms_dominate_the_gradient():
    """treating min / max as constants is not an approximation of this operator's backward"""
    g = torch.Generator().manual_seed(1)
    img = torch.tanh(torch.randn(2, 3, 32, 32, dtype=torch.float64, generator=g))
    dout = torch.randn(2, 1, 32, 32, dtype=torch.float64, generator=g)
    full = R.mask_vjp(img, dout)
    x = img.clone().requires_grad_(True)
    L = R.laplacian(R.rgb_to_grayscale(x)).abs()
    mn, mx = L.min().detach(), L.max().detach()
    Bl = R.gaussian_blur2d((L - mn) / (mx - mn))
    ((Bl / Bl.max().detach()) * dout).sum().backward()
    assert float((x.grad - full).norm() / full.norm()) > 0.1


def test_fixture_equals_the_restatement(golden):
    """the operator fixture came from the script's own mask_maker on the stand-in K; the restatement, on regenerated inputs, gives the same numbers"""
    g = golden("mask_maker")
    for tag, shape, seed in (("n1_8x8", (1, 8, 8), 0), ("n3_19x37", (3, 19, 37), 2)):
        gen = torch.Generator().manual_seed(seed)
        img = torch.tanh(torch.randn(shape[0], 3, shape[1], shape[2], generator=gen))
        dout = torch.randn(shape[0], 1, shape[1], shape[2], generator=gen)
        assert np.abs(R.mask_maker(img.double()).numpy() - g[f"mask_{tag}"]).max() <= 1e-12
        want = g[f"grad_{tag}"]
        assert np.abs(R.mask_vjp(img.double(), dout.double()).numpy() - want).max() <= 1e-12 * np.abs(want).max()
    A, B = O.synthetic_pairs(2, seed=465)
    assert np.abs(R.mask_maker(A.double())[:, :, ::4, ::4].numpy() - g["mask_A_sub"]).max() <= 1e-12
    assert np.abs(R.mask_maker(B.double())[:, :, ::4, ::4].numpy() - g["mask_B_sub"]).max() <= 1e-12
    s = golden("train_step_mask4")
    # the script's loss_FFT sums the four patches, the package logs their mean: the factor mask_weights() puts into lambda_fft
    assert abs(float(s["loss_FFT_script"]) - 4 * float(s["loss_FFT"])) <= 1e-5 * float(s["loss_FFT_script"])
    w = T.mask_weights()
    for pre, lam in (("", 0.0), ("b_", w["lambda_mask"])):
        total = (w["lambda_gan"] * float(s[pre + "loss_GAN_g"]) + w["lambda_trip"] * float(s[pre + "loss_triplet_patch"])
                 + w["lambda_fft"] * float(s[pre + "loss_FFT"]) + lam * float(s[pre + "loss_mask"]))
        assert abs(total - float(s[pre + "loss_G"])) <= 1e-5 * abs(total)
    assert float(s["loss_mask"]) == float(s["b_loss_mask"]) and np.array_equal(s["fake_sub"], s["b_fake_sub"])     # the two runs share their state


def test_mask_generator_keys_and_shapes(golden):
    g = golden("mask_maker")
    G = T.GeneratorUNet((3, 256, 256), mask=True)
    assert list(G.state_dict().keys()) == list(g["g_keys"])
    assert tuple(G.down1.model[0].weight.shape) == (64, 4, 4, 4)
    plain = T.GeneratorUNet((3, 256, 256))
    assert tuple(plain.down1.model[0].weight.shape) == (64, 3, 4, 4) and not plain.mask and G.mask
    assert list(plain.state_dict().keys()) == list(G.state_dict().keys())
    with pytest.raises(T.TfcError, match="mutually exclusive"):
        T.GeneratorUNet((3, 256, 256), labels=3, mask=True)
    with pytest.raises(T.TfcError):
        T.nets.GeneratorCore(T.ops.DT_F32, 3, 3, True)


def test_mask_weights_values():
    w = T.mask_weights()
    assert w == {"lambda_gan": 0.5, "lambda_trip": 0.5, "lambda_fft": 4 * 0.001, "lambda_mask": 0.5}
    assert "loss_triplet_patch" in T.mask_weights.__doc__ and "loss_patch" in T.mask_weights.__doc__
    sig = inspect.signature(T.TrainStep.__init__).parameters
    assert sig["mask"].default is False and sig["lambda_mask"].default == 0.5
    assert set(w) - {"lambda_mask"} <= set(sig)


def test_mask_symbols_are_declared_and_exported():
    names = ("tfc_mask_ws_bytes", "tfc_mask_fwd", "tfc_mask_scale", "tfc_mask_bwd", "tfc_pack_nhwc8_plane")
    for n in names:
        assert n in _lib.PROTOTYPES, n                                # = declared in the header
    assert "mask.hip" in _lib.SOURCES
    T.build()
    so = ctypes.CDLL(_lib.SO_PATH)
    for n in names:
        assert hasattr(so, n), n
    assert any(g.startswith("tfc_mask_") for g in _lib.GUARDED_KERNELS)           # the no-spill gate covers the tile kernels
    for n in ("mask_maker", "mask_l1_loss", "mask_weights"):
        assert n in T.__all__ and callable(getattr(T, n))


def test_mask_refusals_need_no_gpu():
    with pytest.raises(T.TfcError):
        T.mask_maker(torch.zeros(1, 3, 16, 16))                    # CPU tensor: no fallback
    with pytest.raises(T.TfcError, match="forward-only"):
        T.mask_maker(torch.zeros(1, 3, 16, 16, requires_grad=True))
