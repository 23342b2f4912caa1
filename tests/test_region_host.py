"""CPU side of the regional FFT loss (TFCGAN_multigpu_patchFFT_withregion_FFT.py = "4R", ..._withregion_FFT_KL.py = "4K"): the numpy / torch restatement
tests/region_ref.py against the fixtures made from the reference's own (lifted) definitions by tests/golden/make_golden_region.py, the C ABI's new
symbols, and the host-side pieces of the package. No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import tfc_gan_amd as T
from oracle import tfcgan_oracle as O
from tests import region_ref as RR
from tfc_gan_amd import _lib

NEW_SYMBOLS = ("tfc_fft_spectrum_rect", "tfc_fft_spectrum_rect_ws_bytes", "tfc_batch_kl_sum")


@pytest.fixture(autouse=True)
def host_independent_cpu_numerics():
    """the CPU numerics the fixtures were made with (tests/test_oracle_golden.py does the same)"""
    threads, mkldnn = torch.get_num_threads(), torch.backends.mkldnn.enabled
    torch.set_num_threads(8)
    torch.backends.mkldnn.enabled = False
    yield
    torch.set_num_threads(threads)
    torch.backends.mkldnn.enabled = mkldnn


def t(a):
    return torch.from_numpy(np.asarray(a))


def test_new_symbols_are_declared_bound_and_exported():
    for name in NEW_SYMBOLS:
        assert name in _lib.PROTOTYPES, name                                          # = declared in the header
    lib = ctypes.CDLL(_lib.build())                                                   # the built library, without touching a GPU
    for name in NEW_SYMBOLS:
        assert getattr(lib, name) is not None
    lib.tfc_abi_version.restype = ctypes.c_int
    assert lib.tfc_abi_version() == 3
    ws = lib.tfc_fft_spectrum_rect_ws_bytes
    ws.restype, ws.argtypes = ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]
    assert ws(100, 4) == 4 * 129 * 100 * 8 and ws(2, 1) == 129 * 2 * 8 and ws(256, 1) == 129 * 256 * 8
    assert ws(1, 4) == 0 and ws(257, 4) == 0 and ws(100, 0) == 0                      # a refused H has no scratch size


def test_region_weights_reproduce_each_scripts_loss_G():
    assert T.region_weights("l1") == {"lambda_gan": 0.5, "lambda_trip": 0.5, "lambda_fft": 0.5 * 1e-4 * 4, "lambda_region": 0.5e-4}
    assert T.region_weights("kl") == {"lambda_gan": 0.5, "lambda_trip": 0.5, "lambda_fft": 0, "lambda_region": 0.5e-6}
    for kind in ("l1", "kl"):
        w = T.region_weights(kind)
        got = (w["lambda_gan"], w["lambda_trip"], w["lambda_fft"], w["lambda_region"])
        assert np.allclose(got, RR.region_weights(kind), rtol=1e-12, atol=0.0)
    with pytest.raises(T.TfcError):
        T.region_weights("mse")


def test_ref_regional_head_reproduces_the_fixture(golden):
    g = golden("fft_region")
    fake, _ = RR.head_inputs(1)
    amp, pha = RR.regional_fft_components(fake, "eyes")
    assert amp.shape == (1, 1, 100, 129)
    a_ref, p_ref = t(g["amp_eyes0"]), t(g["pha_eyes0"])
    assert (amp[0, 0] - a_ref).abs().max().item() <= 1e-6 * a_ref.max().item()
    dphi = (pha[0, 0] - p_ref).abs()
    dphi = torch.minimum(dphi, 2 * np.pi - dphi)
    assert (dphi * a_ref).max().item() <= 1e-6 * a_ref.max().item()
    amp2, _ = RR.regional_fft_components(fake, (100, 100))
    assert torch.equal(amp, amp2)
    for kind, ns in (("l1", (1, 3)), ("kl", (1, 2, 3))):
        for n in ns:
            fk, rl = RR.head_inputs(n)
            got = RR.regional_fft_loss(fk, rl, kind)
            for v, want in zip(got, g[f"{kind}_n{n}"]):
                assert abs(float(v) - float(want)) <= 1e-6 * abs(float(want)) + 1e-6, (kind, n, float(v), float(want))
            got64 = RR.regional_fft_loss(fk, rl, kind, dtype=torch.float64)            # fp32 loss arithmetic is no further than this from double
            for v, want in zip(got64, g[f"{kind}_n{n}"]):
                assert abs(float(v) - float(want)) <= 2e-6 * abs(float(want)) + 1e-6, (kind, n, float(v), float(want))
    assert float(g["kl_n1"][0]) == 0.0 and float(g["kl_n1"][1]) == 0.0 and float(g["kl_n1"][2]) == 0.0
    # the issue's probes of the lifted functions, to their printed digits
    assert abs(float(g["l1_n1"][0]) - 5906.19) < 0.01 and abs(float(g["kl_n2"][0]) - 975.3198) < 1e-3 and abs(float(g["kl_n3"][0]) - 1013.5365) < 1e-3


@pytest.mark.parametrize("kind,seed", [("l1", 511), ("kl", 512)])
def test_ref_region_train_step_reproduces_the_fixture(golden, kind, seed):
    """one step of 4R:594-642 / 4K:611-658 restated on the oracle's networks against the step of the lifted networks at N = 2 (tolerances of
    tests/test_patch4_host.py::test_ref_train_step_reproduces_the_fixture)"""
    g = golden("train_step_region_" + kind)
    G = O.init_weights_portable(O.GeneratorUNet((3, 256, 256)), seed=61).eval()
    D = O.init_weights_portable(O.Discriminator1((3, 256, 256)), seed=62).train()
    gb = {k: v.clone() for k, v in G.state_dict().items()}
    db = {k: v.clone() for k, v in D.state_dict().items()}
    A, B = O.synthetic_pairs(2, seed=seed)
    out = RR.train_step(G, D, A, B, g["neg_idx"].tolist(), kind)
    for k in ("loss_G", "loss_GAN_g", "loss_triplet_patch", "loss_FFT", "loss_FFT_reg", "loss_Amp_reg", "loss_Pha_reg", "loss_D"):
        assert abs(float(out[k]) - float(g[k])) <= 1e-5 * max(1.0, abs(float(g[k]))), (k, float(out[k]), float(g[k]))
    assert abs(4.0 * float(out["loss_FFT"]) - float(g["fft_loss_sum"])) <= 1e-5 * float(g["fft_loss_sum"])     # the script's sum over the four patches
    assert float(g["loss_FFT_reg"]) > 1.0                                                                      # N = 2: the KL term does not vanish
    assert torch.allclose(out["fake_B"][:, :, ::8, ::8], t(g["fake_sub"]), atol=2e-6)
    assert torch.allclose(G.state_dict()["final.2.weight"] - gb["final.2.weight"], t(g["g_delta_final_w"]), atol=1e-6)
    assert torch.allclose(G.state_dict()["down1.model.0.weight"] - gb["down1.model.0.weight"], t(g["g_delta_down1"]), atol=1e-6)
    assert torch.allclose(D.state_dict()["model.13.weight"] - db["model.13.weight"], t(g["d_delta_head"]), atol=1e-6)
    assert torch.allclose(D.state_dict()["model.3.parametrizations.weight.0._u"], t(g["d_u3"]), atol=1e-5)


def test_cpu_tensors_and_unknown_kinds_are_refused():
    x = torch.zeros(2, 3, 256, 256)
    for kind in ("l1", "kl"):
        with pytest.raises(T.TfcError):
            T.regional_fft_loss(x, x, kind)                          # CPU tensors: no fallback
    with pytest.raises(T.TfcError):
        T.regional_fft_components(x, "eyes")
    with pytest.raises(T.TfcError):
        T.ops.fft_spectrum_rect(x, 100, 0, 100, 2)
    with pytest.raises(T.TfcError):
        T.ops.batch_kl_sum(x, x, x, 1.0, torch.zeros(2))
    with pytest.raises(T.TfcError):
        T.regional_fft_loss(x, x, "mse")


def test_share_of_bins_the_phase_comparison_leaves_out():
    """the rectangular-spectrum tests on the GPU compare phases where amp > 1e-3 * max(amp) and cap the share of a window's bins that this mask
    drops: numpy float64 on the very inputs of those tests (the DC bin sets the maximum)"""
    from tests import patch4_ref as R4
    x = R4.spectrum_inputs(3)
    for row0s, H, lo, hi in (((0, 100), 100, 0.1475, 0.1615), ((3,), 7, 0.0075, 0.0145), ((0, 250), 6, 0.0075, 0.0145), ((0,), 2, 0.0, 0.0085),
                             ((0,), 256, 0.3425, 0.3475)):         # 14.8 - 16.1 %, 0.8 - 1.4 %, 0 - 0.8 %, 34.3 - 34.7 %, to the printed digit
        share = RR.masked_share(x, row0s, H)
        assert share.shape == (3 * len(row0s),)
        assert lo <= share.min() and share.max() <= hi, (H, share.min(), share.max())


def test_emulated_column_pass_meets_the_fixture_bounds():
    """scripts/emulate_rect_cols.py restates the column kernel's order of operations (mean removed, sequential fp32 sum from the rounded table) in numpy
    float32; on the fixture's window ("eyes" of sample 0) it stays inside the bounds that the GPU test sets on the kernel: amplitude 2e-6 * max + 2e-2,
    max(dphi * amp) <= 0.05. The script is the record behind the kernel's extra pass, so it has to keep running."""
    import importlib.util
    import os
    from tests import patch4_ref as R4
    spec = importlib.util.spec_from_file_location("emulate_rect_cols", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "emulate_rect_cols.py"))
    emu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(emu)
    fake, _ = RR.head_inputs(1)
    row0, H = RR.REGIONS["eyes"]
    d_amp, d_pa, a_max = emu.deviations(np.asarray(R4.luma_of(fake[0][:, row0:row0 + H, :256])), remove_mean=True)
    print(f"emulated column pass: amp error {d_amp:.3e} at max {a_max:.4g}, max(dphi * amp) {d_pa:.3e}")
    assert d_amp <= 2e-6 * a_max + 2e-2 and d_pa <= 0.05
