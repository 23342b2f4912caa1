"""CPU restatement (numpy float64 / torch) of the regional FFT loss of TFCGAN_multigpu_patchFFT_withregion_FFT.py ("4R", L1 form, 4R:353-401) and
TFCGAN_multigpu_patchFFT_withregion_FFT_KL.py ("4K", KL form over the batch, 4K:357-420) and of one training step of each script without the LPIPS /
temperature terms, for the tests. tests/golden/make_golden_region.py pins it to the reference's own (ast-lifted) definitions through the fixtures
fft_region / train_step_region_l1 / train_step_region_kl (tests/test_region_host.py)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import tfcgan_oracle as O
from tests import patch4_ref as R4

REGIONS = {"hair": (0, 100), "eyes": (100, 100)}                    # 4R:375-376: rows 0..99 and 100..199 (100:img_width-56), all 256 columns


def head_inputs(N):
    """inputs of the head fixtures: fake = tanh(1.5 * A) * 0.999 of synthetic_pairs(N, seed=501) (three different channels, negatives wrap), real = B"""
    x, real = O.synthetic_pairs(N, seed=501)
    return torch.tanh(x * 1.5) * 0.999, real


def window_spectrum(chw, row0, H, shift=True):
    """numpy float64: rfft2 of the uint8 luma of rows row0 .. row0+H-1 (all 256 columns) of one [3,h,256] sample -> complex [H,129]"""
    f = np.fft.rfft2(R4.luma_of(chw[:, row0:row0 + H, :256]))
    return np.fft.fftshift(f) if shift else f


def regional_fft_components(thermal_tensor, region, shift=True):
    """the nested reg_fft of 4R:358-371 on one region ("hair", "eyes" or (row0, H)): per sample ToPILImage -> L -> np.fft.rfft2 (float64) ->
    fftshift of both axes -> abs, arctan2 -> float32; (AMP, PHA) [N,1,H,129]"""
    row0, H = REGIONS[region] if isinstance(region, str) else region
    fs = [window_spectrum(thermal_tensor[t], row0, H, shift) for t in range(thermal_tensor.shape[0])]
    amp = torch.tensor(np.stack([np.abs(f) for f in fs]), dtype=torch.float32)
    pha = torch.tensor(np.stack([np.arctan2(f.imag, f.real) for f in fs]), dtype=torch.float32)
    return amp[:, None], pha[:, None]


def kl_mean(x, t):
    """nn.KLDivLoss(reduction="mean", log_target=True): the mean over ALL elements of exp(t) (t - x)"""
    return (torch.exp(t) * (t - x)).mean()


def regional_fft_loss(fake_B, real_B, kind="l1", dtype=torch.float32):
    """(loss_FFT_reg, loss_Amp_reg, loss_Pha_reg) of 4R:384-399 (kind "l1") / 4K:388-418 (kind "kl"). The spectra are float32 tensors as in the
    reference; dtype=torch.float64 carries the loss arithmetic (softmax, exp, means) in double -- the yardstick for the fp32 ones.
    kl: log_softmax over dim 0 (the batch); the target of the PHASE term is log_softmax of the real AMPLITUDES (4K:401, :404), literally."""
    la = lp = 0.0
    for region in ("hair", "eyes"):
        af, pf = (v.to(dtype) for v in regional_fft_components(fake_B, region))
        ar, pr = (v.to(dtype) for v in regional_fft_components(real_B, region))
        if kind == "l1":
            la = la + F.l1_loss(af, ar)
            lp = lp + F.l1_loss(pf, pr)
        else:
            t = F.log_softmax(ar, dim=0)
            la = la + kl_mean(F.log_softmax(af, dim=0), t)
            lp = lp + kl_mean(F.log_softmax(pf, dim=0), t)
    return 0.5 * (la + lp), la, lp


def region_weights(kind):
    """loss_G of 4R:603-620 / 4K:617-636 without LPIPS / temperature, as weights of (GAN, triplet, MEAN patch FFT loss, regional loss)"""
    return {"l1": (0.5, 0.5, 0.5 * 1e-4 * 4, 0.5 * 1e-4), "kl": (0.5, 0.5, 0.0, 0.5 * 1e-4 * 0.01)}[kind]


def train_step(G, D, real_A, real_B, neg_idx, kind, lr=2e-4, b1=0.5, b2=0.999):
    """One step of 4R:594-642 (kind "l1") / 4K:611-658 (kind "kl") without LPIPS and the temperature head, fp32, no GradScaler. G, D: oracle modules.
    4R: loss_G = 1/2 (GAN + 1e-4 * fft_loss + 1e-4 * regional + patch), fft_loss = the SUM over the four patches = 4 * patch4_ref.patch_fft_loss;
    4K: loss_G = 1/2 (GAN + 1e-4 * (0.01 * regional) + patch). The discriminator step is 4P's."""
    w_gan, w_trip, w_fft, w_reg = region_weights(kind)
    opt_G = torch.optim.Adam(G.parameters(), lr=lr, betas=(b1, b2))
    opt_D = torch.optim.Adam(D.parameters(), lr=lr, betas=(b1, b2))
    opt_G.zero_grad()
    fake_B = G(real_A)
    pred_fake = D(fake_B, real_A)
    real_pred = D(real_B, real_A)
    loss_gan = O.loss_gan_generator(pred_fake, real_pred)
    loss_trip = R4.patch_triplet_loss(fake_B, real_B, neg_idx)
    with torch.no_grad():
        loss_fft, _, _ = R4.patch_fft_loss(fake_B, real_B)
        loss_reg, la, lp = regional_fft_loss(fake_B, real_B, kind)
    loss_G = w_gan * loss_gan + w_trip * loss_trip + w_fft * loss_fft + w_reg * loss_reg
    loss_G.backward()
    opt_G.step()
    opt_D.zero_grad()
    pred_real = D(real_B, real_A)
    pred_fake = D(fake_B.detach(), real_A)
    loss_D = O.loss_discriminator(pred_real, pred_fake)
    loss_D.backward()
    opt_D.step()
    return {"loss_G": loss_G.detach(), "loss_GAN_g": loss_gan.detach(), "loss_triplet_patch": loss_trip.detach(), "loss_FFT": loss_fft,
            "loss_FFT_reg": loss_reg, "loss_Amp_reg": la, "loss_Pha_reg": lp, "loss_D": loss_D.detach(), "fake_B": fake_B.detach()}


def masked_share(x, row0s, H):
    """numpy float64: per window (rows row0 .. row0+H-1 of x [N,3,h,256], row0 in row0s) the share of bins with amp <= 1e-3 * max(amp over all
    windows) -- the bins the phase comparison of the GPU test leaves out"""
    amps = np.stack([np.abs(window_spectrum(x[n], r, H, shift=False)) for n in range(x.shape[0]) for r in row0s])
    return (amps <= 1e-3 * amps.max()).reshape(len(amps), -1).mean(axis=1)
