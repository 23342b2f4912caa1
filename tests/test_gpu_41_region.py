"""GPU tests of the regional FFT loss (TFCGAN_multigpu_patchFFT_withregion_FFT.py = "4R", L1 form; ..._withregion_FFT_KL.py = "4K", KL form over the
batch): the rectangular-window spectra (tfc_fft_spectrum_rect: 256-point row FFT with a run-time row count, direct H-point column DFT), the batch
log-softmax KL reduction (tfc_batch_kl_sum), regional_fft_components / regional_fft_loss and TrainStep(patches=4, region_fft=...), against
tests/region_ref.py and the fixtures of tests/golden/make_golden_region.py."""
import functools

import numpy as np
import pytest
import torch

import tfc_gan_amd as T
from oracle import tfcgan_oracle as O
from tests import patch4_ref as R4
from tests import region_ref as RR
from tfc_gan_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PI32 = float(np.float32(np.pi))


def t(a):
    return torch.from_numpy(np.asarray(a))


def wrapped(a, b):
    d = (a - b).abs()
    return torch.minimum(d, 2 * np.pi - d)


@functools.lru_cache(maxsize=None)
def spectrum_images():
    """patch4_ref.spectrum_inputs(3) and a strided view of the same pixels inside a wider, taller buffer (row stride 512, rows from 16, columns from 100)"""
    x = R4.spectrum_inputs(3)
    big = torch.zeros(3, 3, 272, 512)
    big[:, :, 16:, 100:356] = x
    return x, big


def numpy_spectra(x, row0s, H, shift):
    """numpy float64 rfft2 of the uint8 luma of every window, in the kernel's window order [n][k] -> complex [N*wins][H][129]"""
    return np.stack([RR.window_spectrum(x[n], r, H, shift) for n in range(x.shape[0]) for r in row0s])


def self_conjugate_bins(H, shift):
    """(rows, columns) of the bins whose imaginary part is exactly zero: kx in {0, 128}, ky = 0 and, for even H, ky = H/2"""
    kys = [0] + ([H // 2] if H % 2 == 0 else [])
    kxs = [0, 128]
    if shift:
        kys, kxs = [(k + H // 2) % H for k in kys], [(k + 64) % 129 for k in kxs]
    return kys, kxs


# ---- 1. spectra against numpy float64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,row0,step,wins,shift,view,cap", [
    (100, 0, 100, 2, False, False, 0.18),       # the reference's two regions: 100 = 3 * 32 + 4 rows -> a ragged fourth row block; 100 = 4 * 5 * 5
    (100, 0, 100, 2, True, False, 0.18),
    (7, 3, 0, 1, True, False, 0.03),            # odd H: the last row is paired with zeros, no ky = H/2 bin
    (6, 0, 250, 2, False, False, 0.03),         # the second window ends on the image's last row
    (2, 0, 0, 1, True, False, 0.03),            # the smallest window: one row pair
    (100, 0, 100, 2, True, True, 0.18),         # a non-contiguous view (row stride 512, offset origin)
])
def test_rect_spectrum_vs_numpy_float64(H, row0, step, wins, shift, view, cap):
    """amplitude within 4e-6 * max(amp) (the bound of the existing numpy comparisons); phase within 2e-3 rad where amp > 1e-3 * max(amp), the share
    of bins a window loses to that mask capped (numpy on these inputs: 14.8 - 16.1 % at H = 100, 0.8 - 1.4 % at H = 6 / 7, 0 - 0.8 % at H = 2:
    tests/test_region_host.py); the self-conjugate bins read exactly 0 or pi."""
    x, big = spectrum_images()
    img = big.to(DEV)[:, :, 16:, 100:356] if view else x.to(DEV)
    assert img.is_contiguous() != view and img.shape == (3, 3, 256, 256)
    row0s = [row0 + k * step for k in range(wins)]
    amp, pha = ops.fft_spectrum_rect(img, H, row0, step, wins, shift=shift)
    assert amp.shape == pha.shape == (3 * wins, H, 129)
    f = numpy_spectra(x, row0s, H, shift)
    a_ref, p_ref = t(np.abs(f)), t(np.arctan2(f.imag, f.real))
    scale = a_ref.max().item()
    a_err = (amp.cpu().double() - a_ref).abs().max().item()
    big_bins = a_ref > 1e-3 * scale
    share = 1.0 - big_bins.flatten(1).double().mean(dim=1)
    dp = wrapped(pha.cpu().double(), p_ref)
    print(f"H={H} shift={shift} view={view}: amp {a_err / scale:.3e} of max ({scale:.4g}), phase {dp[big_bins].max().item():.3e} rad, "
          f"masked share {share.min().item():.4f} .. {share.max().item():.4f}")
    assert a_err <= 4e-6 * scale
    assert share.max().item() <= cap
    assert dp[big_bins].max().item() <= 2e-3
    kys, kxs = self_conjugate_bins(H, shift)
    corner = pha[:, kys][:, :, kxs]
    assert bool(((corner == 0.0) | (corner == PI32)).all())


# ---- 2. H = 256 against the square FFT path -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [True, False])
def test_rect_spectrum_at_256_rows_matches_the_square_fft(shift):
    """the direct column DFT cross-checked against the established radix-4 transform: same shape, same shift convention, amplitude within 2e-6 * max,
    phase within 2e-3 rad where amp > 1e-3 * max (numpy: 34.3 - 34.7 % of a window's bins masked, cap 36 %)"""
    x = spectrum_images()[0].to(DEV)
    a0, p0 = ops.fft_spectrum(x, 256, 1, 1, shift=shift)
    a1, p1 = ops.fft_spectrum_rect(x, 256, 0, 0, 1, shift=shift)
    assert a1.shape == a0.shape == (3, 256, 129)
    scale = a0.max().item()
    err = (a1 - a0).abs().max().item()
    big_bins = a0 > 1e-3 * scale
    share = 1.0 - big_bins.flatten(1).float().mean(dim=1)
    dp = wrapped(p1, p0)
    print(f"rect vs square, shift={shift}: amp {err / scale:.3e} of max, phase {dp[big_bins].max().item():.3e} rad, "
          f"masked share {share.min().item():.4f} .. {share.max().item():.4f}")
    assert err <= 2e-6 * scale
    assert share.max().item() <= 0.36
    assert dp[big_bins].max().item() <= 2e-3


@pytest.mark.parametrize("shift", [True, False])
@pytest.mark.parametrize("S,wx,wy", [(64, 2, 3), (128, 2, 1)])
def test_square_spectrum_every_window_vs_numpy_float64(S, wx, wy, shift):
    """tfc_fft_spectrum, EVERY window of a non-square window grid on the non-contiguous view (row stride 512, offset origin), against numpy float64
    rfft2 of the window's uint8 luma: the FFT and the direct-DFT kernels share the luma and the window origin, so comparing them with each other
    cannot see a geometry slip (x and y swapped, a wrong step). Amplitude within 4e-6 * max(amp), the bound of the numpy comparisons above -- a
    wrong origin shows there; the phase of the four self-conjugate bins is exactly 0 or pi."""
    x, big = spectrum_images()
    img = big.to(DEV)[:2, :, 16:, 100:356]
    assert not img.is_contiguous() and img.stride(2) == 512
    amp, pha = ops.fft_spectrum(img, S, wx, wy, shift=shift)
    nb = S // 2 + 1
    assert amp.shape == pha.shape == (2 * wx * wy, S, nb)
    f = np.stack([np.fft.rfft2(R4.luma_of(x[n, :, (k // wx) * S:(k // wx) * S + S, (k % wx) * S:(k % wx) * S + S])) for n in range(2) for k in range(wx * wy)])
    a_ref = t(np.abs(np.fft.fftshift(f, axes=(-2, -1)) if shift else f))
    scale = a_ref.max().item()
    a_err = (amp.cpu().double() - a_ref).abs().flatten(1).max(dim=1).values
    print(f"S={S} {wx}x{wy} shift={shift}: amp error per window / max ({scale:.4g}): {(a_err / scale).tolist()}")
    assert a_err.max().item() <= 4e-6 * scale
    kys, kxs = [0, S // 2], [0, S // 2]
    if shift:
        kys, kxs = [(k + S // 2) % S for k in kys], [(k + nb // 2) % nb for k in kxs]
    corner = pha[:, kys][:, :, kxs]
    assert bool(((corner == 0.0) | (corner == PI32)).all())


# ---- 3. against the reference's own values --------------------------------------------------------------------------------------------------
def test_regional_components_vs_reference_golden(golden):
    """regional_fft_components(.., "eyes") against the lifted reg_fft: the forms of the S = 128 fixture test (amplitude 2e-6 * max + 2e-2,
    max(dphi * amp) <= 0.05)"""
    g = golden("fft_region")
    fake, _ = RR.head_inputs(1)
    amp, pha = T.regional_fft_components(fake.to(DEV), "eyes")
    assert amp.shape == pha.shape == (1, 1, 100, 129)
    a_ref, p_ref = t(g["amp_eyes0"]), t(g["pha_eyes0"])
    a_err = (amp[0, 0].cpu() - a_ref).abs()
    pa = wrapped(pha[0, 0].cpu(), p_ref) * a_ref
    print(f"eyes, sample 0: amp error {a_err.max().item():.3e} (max amp {a_ref.max().item():.4g}), max(dphi * amp) {pa.max().item():.3e} at bin "
          f"{np.unravel_index(int(pa.argmax()), pa.shape)}")
    assert a_err.max().item() <= 2e-6 * a_ref.max().item() + 2e-2
    assert pa.max().item() <= 0.05
    amp2, pha2 = T.regional_fft_components(fake.to(DEV), (100, 100))
    assert torch.equal(amp, amp2) and torch.equal(pha, pha2)
    amp_h, _ = T.regional_fft_components(fake.to(DEV), "hair")
    both, _ = ops.fft_spectrum_rect(fake.to(DEV), 100, 0, 100, 2, shift=True)
    assert torch.equal(both[0], amp_h[0, 0]) and torch.equal(both[1], amp[0, 0])      # window order [n][hair, eyes]


@pytest.mark.parametrize("kind,N", [("l1", 1), ("l1", 3), ("kl", 2), ("kl", 3)])
def test_regional_loss_vs_reference_golden(golden, kind, N):
    """total and amplitude part relative (l1: 2e-4 / 1e-4, kl: 2e-4 / 2e-4), phase part 2e-3 absolute"""
    want = [float(v) for v in golden("fft_region")[f"{kind}_n{N}"]]
    fake, real = RR.head_inputs(N)
    got = [float(v) for v in T.regional_fft_loss(fake.to(DEV), real.to(DEV), kind)]
    print(f"{kind} N={N}: total {got[0]:.7g} (reference {want[0]:.7g}, rel {abs(got[0] - want[0]) / want[0]:.2e}), amp {got[1]:.7g} ({want[1]:.7g}, "
          f"rel {abs(got[1] - want[1]) / want[1]:.2e}), pha {got[2]:.7g} ({want[2]:.7g}, abs {abs(got[2] - want[2]):.2e})")
    assert abs(got[0] - want[0]) <= 2e-4 * want[0]
    assert abs(got[1] - want[1]) <= (1e-4 if kind == "l1" else 2e-4) * want[1]
    assert abs(got[2] - want[2]) <= 2e-3


# ---- 4. properties --------------------------------------------------------------------------------------------------------------------------
def test_regional_loss_properties():
    fake, real = RR.head_inputs(3)
    fake, real = fake.to(DEV), real.to(DEV)
    # the KL form at N = 1: every log-softmax is 0
    for v in T.regional_fft_loss(fake[:1], real[:1], "kl"):
        assert v.item() == 0.0
    # identical images
    for v in T.regional_fft_loss(real, real, "l1"):
        assert v.item() == 0.0
    total, amp_part, pha_part = T.regional_fft_loss(real, real, "kl")
    assert amp_part.item() == 0.0 and np.isfinite(pha_part.item()) and total.item() == 0.5 * pha_part.item()
    # an all-black batch (amp 0 everywhere), against itself and against an image
    black = torch.zeros_like(real)
    for kind in ("l1", "kl"):
        for a, b in ((black, black), (black, real), (fake, black)):
            assert all(np.isfinite(v.item()) for v in T.regional_fft_loss(a, b, kind)), kind
    amp0, pha0 = T.regional_fft_components(black, "hair")
    assert amp0.abs().max().item() == 0.0 and pha0.abs().max().item() == 0.0
    # the L1 form is a batch mean of per-sample values
    whole = [v.item() for v in T.regional_fft_loss(fake, real, "l1")]
    per = [[v.item() for v in T.regional_fft_loss(fake[i:i + 1], real[i:i + 1], "l1")] for i in range(3)]
    for j in range(3):
        composed = 3.0 * whole[j] - (per[1][j] + per[2][j])
        assert abs(composed - per[0][j]) <= 1e-5 * abs(per[0][j]), (j, composed, per[0][j])
    # run to run
    for kind in ("l1", "kl"):
        first, second = T.regional_fft_loss(fake, real, kind), T.regional_fft_loss(fake, real, kind)
        assert all(torch.equal(a, b) for a, b in zip(first, second)), kind
    # the KL kernel alone against torch on the device: values where exp(t) underflows, N = 5, M not a multiple of 256
    gen = torch.Generator().manual_seed(5)
    af, pf, ar = (torch.randn(5, 1000, generator=gen) * s for s in (3e5, 2.0, 3e5))
    out = torch.zeros(2, device=DEV)
    ops.batch_kl_sum(af.to(DEV), pf.to(DEV), ar.to(DEV), 1.0 / af.numel(), out)
    tt = torch.log_softmax(ar.double(), 0)
    want = [(tt.exp() * (tt - torch.log_softmax(v.double(), 0))).mean().item() for v in (af, pf)]
    assert abs(out[0].item() - want[0]) <= 1e-5 * abs(want[0]) and abs(out[1].item() - want[1]) <= 1e-5 * abs(want[1]) + 1e-6


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_rect_spectrum_and_engine_refuse_bad_arguments():
    x = torch.zeros(1, 3, 256, 256, device=DEV)
    for H, row0, step, wins, word in ((1, 0, 0, 1, "rows"), (257, 0, 0, 1, "rows"), (100, 57, 100, 2, "height"), (6, 251, 0, 1, "height")):
        assert (ops.lib().tfc_fft_spectrum_rect_ws_bytes(H, wins) == 0) == (H in (1, 257))      # a refused H has no scratch size
        with pytest.raises(T.TfcError) as e:
            ops.fft_spectrum_rect(x, H, row0, step, wins)
        assert word in str(e.value), str(e.value)
    with pytest.raises(T.TfcError) as e:
        ops.fft_spectrum_rect(x[:, :, :, :128], 100, 0, 100, 2)       # 128 columns
    assert "width" in str(e.value)
    with pytest.raises(T.TfcError):
        T.regional_fft_components(x, (200, 100))                     # rows 200 .. 299 of a 256-row image
    amp = torch.empty(1, 100, 129, device=DEV)
    rc = ops.lib().tfc_fft_spectrum_rect(ops.stream_ptr(), x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), 3, 256, 256, 1, 0, 0, 1, 1,
                                         amp.data_ptr(), amp.clone().data_ptr(), 0, amp.clone().data_ptr())
    assert rc != 0 and len(ops.lib().tfc_last_error()) > 0
    ok, out2 = torch.zeros(2, 6, device=DEV), torch.zeros(2, device=DEV)                # the KL reduction reads contiguous fp32 of one shape
    for bad in (ok.double(), ok.half(), ok[:, :5], ok.t(), torch.zeros(0, 6, device=DEV)):
        with pytest.raises(T.TfcError):
            ops.batch_kl_sum(ok, bad, ok, 1.0, out2)
    with pytest.raises(T.TfcError):
        ops.batch_kl_sum(ok, ok, ok, 1.0, out2.double())
    assert out2.abs().max().item() == 0.0
    ts_args = (T.GeneratorUNet((3, 256, 256)).to(DEV), T.Discriminator1((3, 256, 256)).to(DEV))
    with pytest.raises(T.TfcError):
        T.TrainStep(*ts_args, patches=16, region_fft="l1")
    with pytest.raises(T.TfcError):
        T.TrainStep(*ts_args, region_fft="kl")                       # patches defaults to 16
    with pytest.raises(T.TfcError):
        T.TrainStep(*ts_args, patches=4, region_fft="mse")
    with pytest.raises(T.TfcError):
        T.regional_fft_loss(x, x, "mse")


# ---- 6. the step against the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,seed", [("l1", 511), ("kl", 512)])
def test_region_train_step_fp32_vs_reference_golden(golden, kind, seed):
    """TrainStep(patches=4, region_fft=kind, **region_weights(kind)) at N = 2 in fp32 compute mode against one step of the networks lifted from 4R / 4K:
    the checks and tolerances of test_patch4_train_step_fp32_vs_reference_golden (losses 2e-4, gradient tensors 1e-2 relative L2, Adam deltas 2e-6)"""
    g = golden("train_step_region_" + kind)
    T.set_compute_dtype(torch.float32)
    try:
        G = O.init_weights_portable(T.GeneratorUNet((3, 256, 256)), seed=61).to(DEV).eval()
        D = O.init_weights_portable(T.Discriminator1((3, 256, 256)), seed=62).to(DEV).train()
        gb = {k: v.clone() for k, v in G.state_dict().items()}
        db = {k: v.clone() for k, v in D.state_dict().items()}
        A, B = O.synthetic_pairs(2, seed=seed)
        ts = T.TrainStep(G, D, compute_dtype=torch.float32, patches=4, region_fft=kind, **T.region_weights(kind))
        out = ts.step(A.to(DEV), B.to(DEV), neg_idx=g["neg_idx"].tolist())
        torch.cuda.synchronize()
    finally:
        T.set_compute_dtype(torch.bfloat16)
    assert set(out) == {"loss_G", "loss_GAN_g", "loss_triplet_patch", "loss_FFT", "loss_Amp", "loss_Pha", "loss_D", "fake_B",
                        "loss_FFT_reg", "loss_Amp_reg", "loss_Pha_reg"}                       # PATCH-4's keys plus the three new ones
    for k in ("loss_G", "loss_GAN_g", "loss_triplet_patch", "loss_FFT", "loss_FFT_reg", "loss_Amp_reg", "loss_Pha_reg", "loss_D"):
        want = float(g[k])
        print(f"  {k}: {float(out[k]):.7g} (reference {want:.7g})")
        assert abs(float(out[k]) - want) <= 2e-4 * max(1.0, abs(want)), (k, float(out[k]), want)
    assert (out["fake_B"].cpu()[:, :, ::8, ::8] - t(g["fake_sub"])).abs().mean().item() <= 1e-4

    def close(got, want, tol=1e-2):
        want = t(want).double()
        rel = ((got.cpu().double() - want).norm() / want.norm()).item()
        print(f"  grad rel-L2 error {rel:.3e} (tol {tol})")
        return rel <= tol

    assert close(ts.gflat.grad_views["down1.model.0.weight"], g["g_grad_down1"])
    assert close(ts.gflat.grad_views["up3.model.0.weight"][::16, ::16], g["g_grad_up3"])
    assert close(ts.dflat.grad_views["model.13.weight"], g["d_grad_head"])
    assert close(ts.dflat.grad_views["model.0.bias"], g["d_grad_b0"])
    assert close(ts.dflat.grad_views["model.3.parametrizations.weight.original"][::8, ::8], g["d_grad_w3"])
    for key, ref in (("final.2.weight", g["g_delta_final_w"]), ("down1.model.0.weight", g["g_delta_down1"])):
        got = (G.state_dict()[key] - gb[key]).cpu()
        assert (got - t(ref)).abs().mean().item() <= 2e-6, key
    got = (D.state_dict()["model.13.weight"] - db["model.13.weight"]).cpu()
    assert (got - t(g["d_delta_head"])).abs().mean().item() <= 2e-6
    assert torch.allclose(D.state_dict()["model.3.parametrizations.weight.0._u"].cpu(), t(g["d_u3"]), atol=1e-4)


# ---- 7. the default step is untouched; the region step is deterministic ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def two_steps(region, two_streams):
    """two steps from the same state (bf16, N = 2, negatives drawn by shared_neg_idx(patches=4)); what the second one left behind"""
    prev = T.set_wgrad_stream(two_streams)
    try:
        G = O.init_weights_portable(T.GeneratorUNet((3, 256, 256)), seed=71).to(DEV)
        D = O.init_weights_portable(T.Discriminator1((3, 256, 256)), seed=72).to(DEV)
        A, B = O.synthetic_pairs(2, seed=73)
        A, B = A.to(DEV), B.to(DEV)
        ts = T.TrainStep(G, D, compute_dtype=torch.bfloat16, patches=4, region_fft=region)
        ts.step(A, B)
        out2 = ts.step(A, B)
        torch.cuda.synchronize()
        return {"g_w": ts.gflat.data.clone(), "d_w": ts.dflat.data.clone(), "g_grad": ts.gflat.grad.clone(), "d_grad": ts.dflat.grad.clone(),
                "fake": out2["fake_B"].clone(), "losses": {k: out2[k].reshape(()).float().clone() for k in out2 if k != "fake_B"}}
    finally:
        T.set_wgrad_stream(prev)


def test_region_term_does_not_disturb_the_step():
    """the term has no gradient: TrainStep(patches=4) and TrainStep(patches=4, region_fft="kl") from the same state and inputs leave the same bits in
    fake_B, every gradient, every weight and every logged loss that both return, except loss_G (which gains the weighted term)"""
    base, reg = two_steps(None, True), two_steps("kl", True)
    for k in ("fake", "g_grad", "d_grad", "g_w", "d_w"):
        assert torch.equal(base[k], reg[k]), k
    assert set(reg["losses"]) - set(base["losses"]) == {"loss_FFT_reg", "loss_Amp_reg", "loss_Pha_reg"}
    for k in base["losses"]:
        if k != "loss_G":
            assert torch.equal(base["losses"][k], reg["losses"][k]), k
    assert reg["losses"]["loss_FFT_reg"].item() > 0.0
    want = base["losses"]["loss_G"].item() + 0.5e-4 * reg["losses"]["loss_FFT_reg"].item()       # lambda_region's default
    assert abs(reg["losses"]["loss_G"].item() - want) <= 1e-5 * abs(want)


@pytest.mark.parametrize("kind", ["l1", "kl"])
def test_region_step_is_bit_deterministic_on_one_and_two_streams(kind):
    """the form of test_patch4_step_is_bit_deterministic_on_one_and_two_streams with the region term on"""
    ref = two_steps(kind, True)
    two_steps.cache_clear()                                          # a second run, not the cached one
    again, one = two_steps(kind, True), two_steps(kind, False)
    assert all(torch.isfinite(v) for v in ref["losses"].values()) and ref["g_grad"].abs().max().item() > 0
    for what, other in (("two streams, run to run", again), ("two streams vs one stream", one)):
        for k in ref:
            if k == "losses":
                assert set(ref[k]) == set(other[k])
                for name in ref[k]:
                    assert torch.equal(ref[k][name], other[k][name]), (what, name)
            else:
                assert torch.equal(ref[k], other[k]), (what, k)
