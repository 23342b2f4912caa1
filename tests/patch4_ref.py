"""CPU restatement (torch / numpy) of the 4-patch heads of TFCGAN_multigpu_patchFFT.py ("4P", PATCH-4) and TFCGAN_multigpu_globalFFT.py ("4G",
GLO-4) for the tests: the 2x2 grid of 128x128 patches, the 4-fold triplet mean, the 128 x 65 patch spectra and one training step without the
LPIPS / temperature terms. tests/golden/make_golden_patch4.py pins it to the reference's own (ast-lifted) definitions through the fixtures
triplet4 / fft_patch128 / train_step_patch4 / train_step_glo4 (tests/test_patch4_host.py)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import tfcgan_oracle as O


def make_4_patches(B):
    """4P:468-471: fake_B1..4 = B[:, :, 0:128 | 128:256, 0:128 | 128:256], row-major (views)."""
    return tuple(B[:, :, 128 * (k // 2):128 * (k // 2) + 128, 128 * (k % 2):128 * (k % 2) + 128] for k in range(4))


def patch_triplet_loss(fake_B, real_B, neg_idx, dtype=None):
    """4P:474-481 with the four random indices given: 0.25 * sum_k TripletMarginLoss(margin=1, p=2)(fake_k, B_k, B_{r_k}); the distance runs over
    the last dim (one 128-pixel patch row). dtype=torch.float64: the same formula in double precision (error yardstick of the GPU test)."""
    if dtype is not None:
        fake_B, real_B = fake_B.to(dtype), real_B.to(dtype)
    fp, rp = make_4_patches(fake_B), make_4_patches(real_B)
    total = 0.0
    for k in range(4):
        total = total + F.triplet_margin_loss(fp[k], rp[k], rp[int(neg_idx[k])], margin=1.0, p=2)
    return 0.25 * total


def luma_of(thermal_chw):
    """4P:270: ToPILImage -> convert("L") of one [3,H,W] sample -> uint8 [H,W]"""
    return O.pil_luma(O.to_pil_uint8(thermal_chw))


def fft_components(thermal_tensor):
    """4P:263-288 on [N,3,S,S] (S = 128 for a patch; 4G:266 takes the whole 256x256 image): per sample ToPILImage -> L -> np.fft.rfft2 (float64) ->
    fftshift -> abs, arctan2 -> float32; [N,1,S,S//2+1]."""
    amps, phas = [], []
    for t in range(thermal_tensor.shape[0]):
        a, p = O.spectrum_components(luma_of(thermal_tensor[t]))
        amps.append(torch.tensor(a, dtype=torch.float32))
        phas.append(torch.tensor(p, dtype=torch.float32))
    return torch.stack(amps)[:, None], torch.stack(phas)[:, None]


def patch_fft_loss(fake_B, real_B):
    """4P:499-511: loss_Amp = 0.25 * sum_k L1mean(A_k^fake, A_k^real), same for the phase; loss_FFT = (loss_Amp + loss_Pha) / 2."""
    la = lp = 0.0
    for fk, rk in zip(make_4_patches(fake_B), make_4_patches(real_B)):
        af, pf = fft_components(fk)
        ar, pr = fft_components(rk)
        la = la + F.l1_loss(af, ar)
        lp = lp + F.l1_loss(pf, pr)
    la, lp = 0.25 * la, 0.25 * lp
    return 0.5 * (la + lp), la, lp


def global_fft_loss(fake_B, real_B):
    """4G:495-499: L1 of amplitude and phase of the whole-image spectra (256 x 129)."""
    af, pf = fft_components(fake_B)
    ar, pr = fft_components(real_B)
    la, lp = F.l1_loss(af, ar), F.l1_loss(pf, pr)
    return 0.5 * (la + lp), la, lp


def sample_spectra(thermal_tensor):
    """4P:291-301 (FFT_Components.make_spectra 4P:254-259): log|fftshift(fft2(luma))| per sample, float32 [N,1,S,S]"""
    return O.sample_spectra(thermal_tensor)


def train_step(G, D, real_A, real_B, neg_idx, fft_mode="patch", lr=2e-4, b1=0.5, b2=0.999):
    """One step of 4P:455-541 (fft_mode="global": 4G:495-504) without LPIPS and the temperature head, fp32, no GradScaler:
    loss_G = 0.5 * GAN + triplet4 + 0.01 * FFT (4P:515); loss_D = 0.5 * (real + fake) (4P:535-537). G, D: oracle modules."""
    opt_G = torch.optim.Adam(G.parameters(), lr=lr, betas=(b1, b2))
    opt_D = torch.optim.Adam(D.parameters(), lr=lr, betas=(b1, b2))
    opt_G.zero_grad()
    fake_B = G(real_A)
    pred_fake = D(fake_B, real_A)
    real_pred = D(real_B, real_A)
    loss_gan = O.loss_gan_generator(pred_fake, real_pred)
    loss_trip = patch_triplet_loss(fake_B, real_B, neg_idx)
    with torch.no_grad():
        loss_fft, la, lp = (patch_fft_loss if fft_mode == "patch" else global_fft_loss)(fake_B, real_B)
    loss_G = 0.5 * loss_gan + loss_trip + 0.01 * loss_fft
    loss_G.backward()
    opt_G.step()
    opt_D.zero_grad()
    pred_real = D(real_B, real_A)
    pred_fake = D(fake_B.detach(), real_A)
    loss_D = O.loss_discriminator(pred_real, pred_fake)
    loss_D.backward()
    opt_D.step()
    return {"loss_G": loss_G.detach(), "loss_GAN_g": loss_gan.detach(), "loss_triplet_patch": loss_trip.detach(), "loss_FFT": loss_fft,
            "loss_Amp": la, "loss_Pha": lp, "loss_D": loss_D.detach(), "fake_B": fake_B.detach()}


def spectrum_inputs(N):
    """inputs of the S = 128 spectrum tests: tanh(1.7 * synthetic_pairs(N, seed=428)) * 0.999 (visible image: three different channels)"""
    x, _ = O.synthetic_pairs(N, seed=428)
    return torch.tanh(x * 1.7) * 0.999


def masked_share(x, wx, wy):
    """numpy float64: per 128 x 128 window of x [N,3,256,256] the share of bins with amp <= 1e-3 * max(amp over all windows) -- the bins the phase
    comparison of the GPU test leaves out"""
    amps = []
    for n in range(x.shape[0]):
        for k in range(wx * wy):
            y0, x0 = (k // wx) * 128, (k % wx) * 128
            amps.append(np.abs(np.fft.rfft2(luma_of(x[n, :, y0:y0 + 128, x0:x0 + 128]))))
    amps = np.stack(amps)
    return (amps <= 1e-3 * amps.max()).reshape(len(amps), -1).mean(axis=1)
