"""Host-side tests of the DarkVisible feature (no GPU): the stride-2 convolution op is declared on every layer of the binding and its gather
descriptors reproduce torch's convolution and both adjoints in the library's host emulator; the step fixture exists and a CPU recomposition of the step
-- oracle generators, the pix2pix restatement, the package's localiser on the CPU, torch's two warp calls -- reproduces its eight losses;
Pix2PixDiscriminator has the fixture's keys."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tfc_gan_amd as T
from oracle import tfcgan_oracle as O
from tests import pix2pix_ref as R
from tfc_gan_amd import _lib, ops, stn21

LOSSES = ("loss_G", "loss_GAN", "recon_loss", "perc_loss", "loss_FFT", "loss_D", "loss_D1", "loss_D2")


def test_op_conv2_is_declared_bound_and_exported():
    assert _lib.CONSTANTS["OP_CONV2"] == 5                        # the header's value
    assert _lib.OP_CONV2 == 5 and ops.OP_CONV2 == 5
    lib = _lib.load()
    assert {"tfc_affine_warp_mode_fwd", "tfc_affine_warp_mode_bwd"} <= set(_lib.PROTOTYPES)
    assert len(_lib.PROTOTYPES["tfc_affine_warp_mode_fwd"][1]) == 9 and len(_lib.PROTOTYPES["tfc_affine_warp_mode_bwd"][1]) == 12
    for name in _lib.PROTOTYPES:
        assert hasattr(lib, name), name
    assert lib.tfc_abi_version() == 3                             # symbols are only added
    assert lib.tfc_conv_packed_bytes(ops.DT_BF16, _lib.OP_CONV2, 0, 64, 128) > 0 and lib.tfc_conv_packed_bytes(ops.DT_BF16, _lib.OP_CONV2, 1, 64, 128) > 0


def test_out_hw_of_conv2():
    f = ops.OUT_HW[_lib.OP_CONV2]
    assert [f(h) for h in (2, 4, 18, 256)] == [1, 2, 9, 128]


def _nhwc8(x):
    n, c, h, w = x.shape
    out = np.zeros((n, h, w, (c + 7) // 8 * 8), dtype=np.float32)
    out[..., :c] = x.detach().numpy().transpose(0, 2, 3, 1)
    return np.ascontiguousarray(out)


def _emulate(pas, es, a, b, out_shape, N, H, W, Cin, Cout):
    y = np.zeros(out_shape, dtype=np.float32)
    rc = _lib.load().tfc_host_emulate_conv(_lib.OP_CONV2, pas, es, a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p),
                                           y.ctypes.data_as(ctypes.c_void_p), N, H, W, Cin, Cout)
    _lib.check(rc, "tfc_host_emulate_conv")
    return y


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(3, 6, 6, 6, 64), (2, 18, 34, 16, 32), (1, 4, 4, 32, 16), (2, 2, 2, 8, 8)])
@pytest.mark.parametrize("es", [2, 4])
def test_conv2_gather_model_matches_torch(N, H, W, Cin, Cout, es):
    """the descriptors of the three passes (four parity planes forward, four output phases dgrad, one plane per phase wgrad) and the packed operand
    stream, evaluated by the library's host emulator, against F.conv2d(stride=2, padding=1) and its adjoints; bounds of test_host_logic.py"""
    rng = np.random.default_rng(500 + Cin)
    x = torch.from_numpy(rng.standard_normal((N, Cin, H, W)).astype(np.float32)).requires_grad_(True)
    w = torch.from_numpy((rng.standard_normal((Cout, Cin, 4, 4)) * 0.1).astype(np.float32)).requires_grad_(True)
    y = F.conv2d(x, w, stride=2, padding=1)
    go = torch.from_numpy(rng.standard_normal(tuple(y.shape)).astype(np.float32))
    gx, gw = torch.autograd.grad(y, (x, w), go)
    c8 = lambda c: (c + 7) // 8 * 8  # noqa: E731
    wn = np.ascontiguousarray(w.detach().numpy())
    got = _emulate(0, es, _nhwc8(x), wn, (N, H // 2, W // 2, c8(Cout)), N, H, W, Cin, Cout)
    np.testing.assert_allclose(got[..., :Cout], y.detach().numpy().transpose(0, 2, 3, 1), atol=2e-4)
    got = _emulate(1, es, _nhwc8(go), wn, (N, H, W, c8(Cin)), N, H, W, Cin, Cout)
    np.testing.assert_allclose(got[..., :Cin], gx.numpy().transpose(0, 2, 3, 1), atol=2e-4)
    got = _emulate(2, es, _nhwc8(x), _nhwc8(go), (Cout, Cin, 4, 4), N, H, W, Cin, Cout)
    np.testing.assert_allclose(got, gw.numpy(), atol=2e-3, rtol=1e-4)


def test_conv2_launch_plans():
    """host only: bf16 takes the phase-fused weight-gradient launch (TFC_K_WGRADT / TFC_K_WGRADT2), fp32 the per-plane kernel; the first layer's
    forward stays off the stride-1 first-layer kernel (TFC_K_CONV_C8)"""
    lib = _lib.load()
    q = (ctypes.c_int * 8)()

    def plan(dt, pas, N, H, Cin, Cout, flags=0):
        assert lib.tfc_conv_plan_query(dt, _lib.OP_CONV2, pas, N, H, H, Cin, Cout, flags, 256, q, 8) == 8, lib.tfc_last_error()
        return list(q)
    assert plan(ops.DT_BF16, 2, 32, 128, 64, 128)[0] in (15, 16)
    assert plan(ops.DT_BF16, 2, 32, 256, 6, 64)[0] in (15, 16)
    assert plan(ops.DT_F32, 2, 32, 128, 64, 128)[0] == 10
    assert plan(ops.DT_BF16X3, 2, 32, 128, 64, 128)[0] == 13
    assert plan(ops.DT_BF16, 0, 32, 256, 6, 64, _lib.EP_BIAS | _lib.EP_LEAKY)[0] == 0
    assert plan(ops.DT_BF16, 0, 32, 128, 64, 128, _lib.EP_BIAS | _lib.EP_STATS)[0] == 1
    lib.tfc_set_batch_invariant(1)
    try:
        a, b = plan(ops.DT_BF16, 0, 13, 32, 256, 512, _lib.EP_BIAS | _lib.EP_STATS), plan(ops.DT_BF16, 0, 4, 32, 256, 512, _lib.EP_BIAS | _lib.EP_STATS)
        assert a == b                                             # batch-invariant mode: the plan does not depend on N
        assert plan(ops.DT_BF16, 1, 13, 32, 256, 512) == plan(ops.DT_BF16, 1, 4, 32, 256, 512)
    finally:
        lib.tfc_set_batch_invariant(0)


def test_conv2_refuses_an_odd_size_on_the_host():
    lib = _lib.load()
    rc = lib.tfc_conv_fwd(None, ops.DT_BF16, _lib.OP_CONV2, None, 8, 1, 5, 6, 8, 8, None, None, 8, None, None, None, None, 0, None)
    assert rc != 0 and b"even" in lib.tfc_last_error()


def test_pix2pix_discriminator_keys_equal_the_fixtures(golden):
    g = golden("train_step_darkvisible")
    want = [str(k) for k in g["d_keys"]]
    assert want == ["model.0.weight", "model.0.bias", "model.2.weight", "model.2.bias", "model.5.weight", "model.5.bias", "model.8.weight",
                    "model.8.bias", "model.12.weight"]
    assert list(T.Pix2PixDiscriminator((3, 256, 256)).state_dict().keys()) == want
    assert list(R.Pix2PixRef().state_dict().keys()) == want
    assert [k for k, _ in stn21.Net((3, 32, 32), localiser="torch", patch_size=16, sample_align_corners=False).state_dict().items()] == [str(k) for k in g["net_keys"]]


def test_fixture_losses_from_a_cpu_recomposition(golden):
    """the forward half of TFCGAN_STN21_Eur_DarkVisible.py:677-731 at the fixture's conditions (N = 1, eval-mode dropout, portable weights, no LPIPS)
    from code of this repository alone: the eight losses to 1e-5 relative"""
    g = golden("train_step_darkvisible")
    torch.set_num_threads(8)
    shp = (3, 256, 256)
    G1, G2, D1, D2 = O.GeneratorUNet(shp), O.GeneratorUNet(shp), R.Pix2PixRef(), R.Pix2PixRef()
    net = stn21.Net(shp, localiser="torch", patch_size=16, sample_align_corners=False)
    for i, m in enumerate((G1, G2, D1, D2, net)):
        O.init_weights_portable(m, seed=101 + i)
        m.eval()
    A, B = O.synthetic_pairs(1, seed=105)
    with torch.no_grad():
        net.fc_loc[6].weight.mul_(4.0)
        net.fc_loc[6].bias.copy_(torch.tensor([0.03, -0.02, 0.04, 0.02, -0.03, -0.05]))
        fake_B = G1(A)
        theta = net.stn_phi(torch.cat((A, fake_B), 1)).reshape(1, 6) + torch.tensor([1.0, 0, 0, 0, 1.0, 0])
        warped_B = R.mixed_warp(B, theta.view(1, 2, 3))
        fake_A = G2(warped_B)
        recon = F.l1_loss(warped_B, fake_B)
        _, la, lp = O.global_fft_loss(fake_A, A)
        fft = la + lp

        def bce(x, t):
            return F.binary_cross_entropy_with_logits(x, torch.full_like(x, t))
        pf1, pr1 = D1(fake_B, A), D1(B, A)
        pf2, pr2 = D2(fake_A, B), D2(A, B)
        gan = bce(pf1 - pr1, 0.9) + bce(pf2 - pr2, 0.9)
        lD1 = bce(pr1 - pf1, 0.9) + bce(pf1 - pr1, 0.0)
        lD2 = bce(pr2 - pf2, 0.9) + bce(pf2 - pr2, 0.0)
    got = {"loss_G": gan + recon + fft, "loss_GAN": gan, "recon_loss": recon, "perc_loss": torch.zeros(()), "loss_FFT": fft,
           "loss_D": 0.5 * (lD1 + lD2), "loss_D1": lD1, "loss_D2": lD2}
    for k in LOSSES:
        w = float(g[k])
        assert abs(float(got[k]) - w) <= 1e-5 * max(abs(w), 1e-30) or (w == 0.0 and float(got[k]) == 0.0), (k, float(got[k]), w)
    assert (warped_B[:, :, ::8, ::8] - torch.from_numpy(g["warped_sub"])).abs().max().item() <= 1e-4
    # a bias in front of InstanceNorm: torch's gradient is rounding noise (the engine returns exact zeros there)
    assert np.abs(g["g_D2_b8"]).max() <= 1e-5 * float(g["g_D2_w8_absmax"])
