"""Loss heads of the PATCH-16 step with the reference's call surface (TFCGAN_multigpu_patchFFT_16P.py):

  make_16_patches(B)                     :227-253   16 views, patch k -> rows 64*(k//4).., cols 64*(k%4)..
  ContrastiveLoss / patch_triplet_loss   :75, :558-583   16x nn.TripletMarginLoss(margin=1, p=2) with given negatives
  FFT_Components / fft_components / calculate_ffts   :271-375
  relativistic BCE                       :554, :628-630 (engine.py uses the fused kernel directly)

and the 4-patch family (TFCGAN_multigpu_patchFFT.py = "4P", TFCGAN_multigpu_globalFFT.py): the same heads on a 2x2 grid of 128x128 patches

  make_4_patches(B)                      4P:468-471   4 views, patch k -> rows 128*(k//2).., cols 128*(k%2)..
  patch_triplet_loss with 4 indices      4P:474-481   0.25 * sum of 4 nn.TripletMarginLoss
  fft_components on 128x128 patches      4P:263-288   128 x 65 spectra;  patch_fft_loss(patches=4)  4P:499-511

and the regional FFT loss of the two 4-patch scripts that carry one (TFCGAN_multigpu_patchFFT_withregion_FFT.py = "4R", ..._withregion_FFT_KL.py = "4K")

  regional_fft_components / regional_fft_loss   4R:353-401 (L1 form), 4K:357-420 (KL form over the batch)   100 x 129 spectra of rows 0..99, 100..199

The reference has no class called ContrastiveLoss: the "16-patch contrastive head" named by the project brief IS the
16-fold triplet mean above; `ContrastiveLoss` here is defined as exactly that.
"""
import numpy as np
import torch
import torch.nn as nn

from . import ops

PATCH = 64
GRID = 4


def make_16_patches(B):
    """16 zero-copy views of B[N,C,256,256], row-major 4x4 grid of 64x64 patches (reference order B1..B16)."""
    assert B.shape[-1] == 256 and B.shape[-2] == 256, "the reference hard-codes offsets 64/128/192 (256x256 images only)"
    return tuple(B[:, :, 64 * (k // GRID):64 * (k // GRID) + PATCH, 64 * (k % GRID):64 * (k % GRID) + PATCH] for k in range(16))


def make_4_patches(B):
    """4 zero-copy views of B[N,C,256,256], row-major 2x2 grid of 128x128 patches (reference order B1..B4, 4P:468-471)."""
    assert B.shape[-1] == 256 and B.shape[-2] == 256, "the reference hard-codes the offset 128 (256x256 images only)"
    return tuple(B[:, :, 128 * (k // 2):128 * (k // 2) + 128, 128 * (k % 2):128 * (k % 2) + 128] for k in range(4))


def patch_first_flat_index(k, width=256, grid=GRID):
    """flat NCHW offset (within one channel plane) of the first element of patch k of a grid x grid patch grid:
    grid 4: 0,64,128,192,16384,...; grid 2: 0,128,32768,32896"""
    p = width // grid
    return p * (k // grid) * width + p * (k % grid)


class _Triplet16Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fake, real, neg_idx):
        loss, dfake = ops.patch_triplet(fake.detach(), real.detach(), neg_idx, want_grad=fake.requires_grad)
        ctx.save_for_backward(dfake) if dfake is not None else None
        ctx.has = dfake is not None
        ctx.in_dtype = fake.dtype
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        if not ctx.has:
            return None, None, None
        (dfake,) = ctx.saved_tensors
        return (dfake * g).to(ctx.in_dtype), None, None


def patch_triplet_loss(fake_B, real_B, neg_idx):
    """(1/P) * sum_k TripletMarginLoss(fake patch k, real patch k, real patch neg_idx[k]) -- one fused kernel; P = len(neg_idx) = 16 (4x4 grid of
    64x64 patches) or 4 (2x2 grid of 128x128 patches, 4P:468-481)."""
    return _Triplet16Fn.apply(fake_B, real_B, [int(i) for i in neg_idx])


class ContrastiveLoss(nn.Module):
    """The patch triplet head (patches = 16, or 4 for the 2x2 grid of the 4-patch scripts). Two call forms:
         loss(fake_B, real_B, neg_idx=None)          whole images [N,C,256,256]; neg_idx: 16 (or 4) ints (drawn with
                                                     np.random.randint(patches) per patch like the reference when None)
         loss(anchor, positive, negative)            three [N,C,64,64] (or [N,C,128,128]) patch tensors = nn.TripletMarginLoss(margin=1, p=2)
                                                     on one patch (composed from the same kernel by embedding the patch)."""

    def __init__(self, margin=1.0, p=2, patches=16):
        super().__init__()
        assert margin == 1.0 and p == 2, "the reference uses margin=1.0, p=2 (:75)"
        assert patches in (4, 16)
        self.patches = patches

    def forward(self, a, b, c=None):
        if torch.is_tensor(c):
            return _single_patch_triplet(a, b, c)
        if c is None:
            c = [int(np.random.randint(self.patches, size=1).item()) for _ in range(self.patches)]
        return patch_triplet_loss(a, b, c)


def _single_patch_triplet(anchor, positive, negative):
    """nn.TripletMarginLoss on one 64x64 patch through the 16-patch kernel: put anchor / positive in patch 0 and the negative
    in patch 1 of zero images; patches 1..15 use themselves as negatives and contribute exactly 1.0 each. (128x128 patches: the 4-patch
    kernel, patches 1..3.) The embedding copy stays in the autograd graph, so the gradient reaches `anchor`."""
    N, C = anchor.shape[:2]
    P = anchor.shape[-1]                                          # 64: the 16-patch kernel; 128: the 4-patch kernel (total * 4 - 3)
    assert P in (64, 128) and anchor.shape[-2] == P
    npatch = (256 // P) ** 2
    dev = anchor.device
    fake = torch.zeros((N, C, 256, 256), dtype=torch.float32, device=dev)
    real = torch.zeros_like(fake)
    fake[:, :, :P, :P] = anchor.float()
    real[:, :, :P, :P] = positive.detach().float()
    real[:, :, :P, P:2 * P] = negative.detach().float()
    neg = [1] + list(range(1, npatch))
    total = patch_triplet_loss(fake, real, neg)
    return total * float(npatch) - float(npatch - 1)


class FFT_Components(object):
    """reference :271-289. `image`: 2-D uint8 array-like (a PIL "L" image in the reference) or a [1|3,H,W] tensor in [-1,1]."""

    def __init__(self, image):
        self.image = image

    def _as_tensor(self):
        img = self.image
        if torch.is_tensor(img):
            return img
        arr = np.asarray(img).astype(np.float32)                  # uint8 luma -> value whose *255 truncation gives it back
        t = torch.from_numpy((arr + 0.5) / 255.0)[None]
        return t

    def make_components(self):
        t = self._as_tensor().cuda()
        S = t.shape[-1]
        amp, pha = ops.fft_spectrum(t[None].expand(1, 3 if t.shape[0] == 3 else 1, S, S).contiguous(), S, 1, 1, shift=True)
        return amp[0], pha[0]

    def make_spectra(self):
        """reference :284-289: log|fftshift(fft2(image))|, the full S x S magnitude spectrum (S = 64, 128 or 256), fp32 on the GPU."""
        t = self._as_tensor().cuda()
        S = t.shape[-1]
        return _full_log_spectrum(t[None].expand(1, 3 if t.shape[0] == 3 else 1, S, S).contiguous(), S)[0]


def _full_log_spectrum(img, S):
    """log-magnitude of the fftshifted FULL spectrum from the half spectrum of tfc_fft_spectrum: for real input |F[ky][kx]| = |F[-ky][-kx]|, so
    columns S/2+1 .. S-1 are the point reflection of columns S/2-1 .. 1 (pure indexing, no arithmetic beyond the kernel's)."""
    amp, _ = ops.fft_spectrum(img, S, 1, 1, shift=False)          # [N][S][S/2+1], unshifted
    nb = S // 2 + 1
    ky = torch.arange(S, device=amp.device)
    neg_ky = (-ky) % S
    right = amp[:, neg_ky][:, :, 1:nb - 1].flip(-1)               # kx = S/2+1 .. S-1  <-  conj partner (S-ky, S-kx)
    full = torch.cat((amp, right), dim=-1)                        # [N][S][S], kx = 0 .. S-1
    return torch.log(torch.fft.fftshift(full, dim=(-2, -1)))


def sample_spectra(thermal_tensor):
    """reference :378-388: thermal_tensor [N,3,S,S] in [-1,1] -> log-magnitude spectra [N,1,S,S] fp32 (S = 64, 128 or 256) for the sample grids."""
    S = thermal_tensor.shape[-1]
    assert thermal_tensor.shape[-2] == S and S in (64, 128, 256)
    return _full_log_spectrum(thermal_tensor.detach(), S)[:, None]


def fft_components(thermal_tensor, patch=True):
    """reference :293-319. thermal_tensor [N,3,S,S] in [-1,1] -> (AMP, PHA) each [N,1,S,S//2+1] fp32, fftshifted.
    patch=True: S taken from the tensor, 64 (33 columns, P16) or 128 (65 columns, 4P:280-281); patch=False: S=256 (129)."""
    S = thermal_tensor.shape[-1] if patch else 256
    assert S in ((64, 128) if patch else (256,)) and thermal_tensor.shape[-1] == S and thermal_tensor.shape[-2] == S
    N = thermal_tensor.shape[0]
    amp, pha = ops.fft_spectrum(thermal_tensor, S, 1, 1, shift=True)
    return amp.reshape(N, 1, S, S // 2 + 1), pha.reshape(N, 1, S, S // 2 + 1)


def _spectral_l1(spectrum, fake, real, scale, out=None):
    """The spectral L1 loss on one window grid: `spectrum(img)` -> (amp, pha) of every window of a batch. Adds scale * sum |amp_fake - amp_real| to
    out[0] and the same of the phases to out[1] (`out`: two zeros unless given) and returns out."""
    af, pf = spectrum(fake.detach())
    ar, pr = spectrum(real.detach())
    if out is None:
        out = torch.zeros(2, dtype=torch.float32, device=fake.device)
    ops.l1_sum(af, ar, scale, out[0:1])
    ops.l1_sum(pf, pr, scale, out[1:2])
    return out


def patch_fft_loss(fake_B, real_B, patches=16):
    """loss_FFT of calculate_ffts on whole images: 0.5 * (mean_k L1(amp) + mean_k L1(phase)) over the 16 patches (patches=4: the four
    128 x 128 patches with 128 x 65 spectra, 4P:499-511). Carries no gradient, exactly like the reference (tensor -> PIL -> numpy round trip,
    :300-302)."""
    assert patches in (4, 16)
    N = fake_B.shape[0]
    S, g = (64, 4) if patches == 16 else (128, 2)
    scale = 1.0 / (float(patches) * N * S * (S // 2 + 1))
    out = _spectral_l1(lambda img: ops.fft_spectrum(img, S, g, g, shift=False), fake_B, real_B, scale)
    return 0.5 * (out[0] + out[1]), out[0], out[1]


def global_fft_loss(fake_B, real_B):
    """GLO-16 variant (TFCGAN_multigpu_globalFFT_16P.py:294-313, :524-529): rfft2 of the whole 256x256 image."""
    N = fake_B.shape[0]
    out = _spectral_l1(lambda img: ops.fft_spectrum(img, 256, 1, 1, shift=False), fake_B, real_B, 1.0 / (N * 256 * 129))
    return 0.5 * (out[0] + out[1]), out[0], out[1]


# ---- regional FFT loss (4R:353-401, 4K:357-420) -------------------------------------------------------------------------------
REGIONS = {"hair": (0, 100), "eyes": (100, 100)}      # (first row, rows): fake_B[:, :, 0:100, :] and fake_B[:, :, 100:img_width-56, :] (4R:375-376); rows 200..255 unused


def regional_fft_components(thermal_tensor, region):
    """The nested reg_fft of regional_fft_loss (4R:358-371) on one region of whole images: thermal_tensor [N,3,256,256] in [-1,1]; region "hair" (rows
    0..99), "eyes" (rows 100..199) or an explicit (row0, H) with H in 2 .. 256. Per sample ToPILImage -> convert("L") -> np.fft.rfft2 (H x 129) ->
    fftshift of both axes -> abs, arctan2. Returns (AMP, PHA), each [N,1,H,129] fp32. N comes from the tensor (the reference loops opt.batch_size)."""
    row0, H = REGIONS[region] if isinstance(region, str) else (int(region[0]), int(region[1]))
    N = thermal_tensor.shape[0]
    amp, pha = ops.fft_spectrum_rect(thermal_tensor.detach(), H, row0, 0, 1, shift=True)
    return amp.reshape(N, 1, H, 129), pha.reshape(N, 1, H, 129)


def regional_fft_loss(fake_B, real_B, kind="l1", batch_scope="global"):
    """regional_fft_loss of 4R (kind="l1", 4R:353-401) or 4K (kind="kl", 4K:357-420) -> (loss_FFT_reg, loss_Amp_reg, loss_Pha_reg), device scalars
    without gradient (the reference goes tensor -> PIL -> numpy) and without a host synchronisation.
      l1: loss_Amp_reg = L1mean(Ah_F, Ah_R) + L1mean(Ae_F, Ae_R) -- a SUM over the two regions --, loss_Pha_reg the same of the phases (4R:391-398).
      kl: every spectrum through F.log_softmax(., dim=0), i.e. over the BATCH, then nn.KLDivLoss(reduction="mean", log_target=True) = mean of
          exp(t)(t - x), summed over the two regions (4K:400-417). The reference builds the real PHASE target from the real AMPLITUDES (4K:401, :404);
          that is reproduced literally: the target of the phase term is the target of the amplitude term. At N = 1 the loss is exactly 0.
    loss_FFT_reg = 1/2 (loss_Amp_reg + loss_Pha_reg) in both. The spectra are taken unshifted: every term is a sum over all bins.
    batch_scope (kind="kl" on several ranks): "global", the softmax runs over the batch of ALL ranks and each rank returns the mean of its own terms --
    the mean over ranks is the loss of the gathered batch (ops.batch_kl_sum); "shard", over this rank's samples only. The L1 form is per sample."""
    if kind not in ("l1", "kl"):
        raise ops._lib.TfcError(f"regional_fft_loss: kind={kind!r} ('l1': ..._withregion_FFT.py, 'kl': ..._withregion_FFT_KL.py)")
    ops.phased_scope(batch_scope, "regional_fft_loss")
    ops.require_gpu(fake_B, real_B)
    N = fake_B.shape[0]
    (_, H), step = REGIONS["hair"], REGIONS["eyes"][0]
    spectrum = lambda img: ops.fft_spectrum_rect(img, H, 0, step, 2, shift=False)    # noqa: E731  [N*2][100][129]: sample n = windows 2n (hair), 2n+1 (eyes)
    scale = 1.0 / (N * H * 129)                                    # the mean of one region; the two regions add
    if kind == "l1":
        out = _spectral_l1(spectrum, fake_B, real_B, scale)
    else:
        (af, pf), (ar, _) = spectrum(fake_B.detach()), spectrum(real_B.detach())
        out = torch.zeros(2, dtype=torch.float32, device=fake_B.device)
        ops.batch_kl_sum(af.reshape(N, -1), pf.reshape(N, -1), ar.reshape(N, -1), scale, out, batch_scope=batch_scope)
    return 0.5 * (out[0] + out[1]), out[0], out[1]


def region_weights(kind):
    """TrainStep keyword values that reproduce loss_G of 4R (kind="l1", 4R:603-620) / 4K (kind="kl", 4K:617-636) without the LPIPS and temperature terms:
      4R: loss_G = 1/2 (GAN + 1e-4 * fft_loss + 1e-4 * regional + patch + ..);  fft_loss is the SUM over the four patches (4R:315-317) and
          patch_fft_loss returns their mean, hence the factor 4 in lambda_fft.
      4K: loss_G = 1/2 (GAN + 1e-4 * (0.01 * regional) + patch + ..);  the patch FFT loss is logged only."""
    if kind == "l1":
        return {"lambda_gan": 0.5, "lambda_trip": 0.5, "lambda_fft": 0.5 * 1e-4 * 4, "lambda_region": 0.5e-4}
    if kind == "kl":
        return {"lambda_gan": 0.5, "lambda_trip": 0.5, "lambda_fft": 0.0, "lambda_region": 0.5e-6}
    raise ops._lib.TfcError(f"region_weights: kind={kind!r} ('l1' or 'kl')")


def debias_weights(kind):
    """TrainStep keyword values of the label-conditioned 4-patch scripts (TFCGAN_multigpu_patchFFT_debiased.py "DB1", ..._V2.py, ..._V3.py) without their
    LPIPS and temperature terms; use with patches=4:
      v1 (DB1:572): loss_G = GAN + triplet + label + 0.001 FFT; G is fed the drawn labels, loss_label is taken against them (DB1:508, :522)
      v2 (DB2:582): loss_G = GAN + label + 0.001 FFT; G is fed the real labels (DB2:512, :530); the discriminator's label sums carry 1/3 (DB2:611, :617)
      v3 (DB3:583): v2 with the ethnicity term of loss_label weighted 10 (DB3:531); the discriminator's label sums stay unweighted (DB3:612, :618)"""
    if kind == "v1":
        return {"lambda_gan": 1.0, "lambda_fft": 0.001, "lambda_trip": 1.0, "labels": "generated", "label_weights": (1.0, 1.0, 1.0), "d_label_scale": 1.0}
    if kind == "v2":
        return {"lambda_gan": 1.0, "lambda_fft": 0.001, "lambda_trip": 0.0, "labels": "real", "label_weights": (1.0, 1.0, 1.0), "d_label_scale": 1.0 / 3.0}
    if kind == "v3":
        return {"lambda_gan": 1.0, "lambda_fft": 0.001, "lambda_trip": 0.0, "labels": "real", "label_weights": (1.0, 10.0, 1.0), "d_label_scale": 1.0 / 3.0}
    raise ops._lib.TfcError(f"debias_weights: kind={kind!r} ('v1', 'v2' or 'v3')")


def mask_weights():
    """TrainStep keyword values of the edge-mask 4-patch script (TFCGAN_multigpu_patchFFT_experiment.py "4X") without its LPIPS and temperature terms;
    use with patches=4, mask=True. 4X:587: loss_G = 0.5 GAN + 0.5 LPIPS + 0.5 loss_triplet_patch + 0.5 temp + 0.001 FFT + 0.5 mask. 4X:335-337 SUMS
    the amplitude and phase terms over the four patches where patch_fft_loss returns their mean, so lambda_fft is four times the script's 0.001 (the
    way region_weights derives it). Name slip of the script: its loop assigns the patch triplet to `loss_patch` (4X:575) and :587 adds
    `loss_triplet_patch`, a name the loop never assigns; the triplet term is what is meant and what runs here."""
    return {"lambda_gan": 0.5, "lambda_trip": 0.5, "lambda_fft": 4 * 0.001, "lambda_mask": 0.5}


def mask_maker(img, batch_scope="global"):
    """reference 4X:385-390: the edge mask [N,1,H,W] of img [N,3,H,W] -- |7x7 normalised Laplacian| of the grayscale image, min/max-normalised over
    the WHOLE batch, 9x9 Gaussian blur (sigma 1.6), divided by its batch maximum (csrc/mask.hip; fp32 in every compute mode). Forward only: the exact
    backward lives in mask_l1_loss / TrainStep(mask=True). A constant batch (max == min) gives NaN, as in the reference. On several ranks the whole
    batch is the gathered batch of all ranks (batch_scope="global", two small exchanges: ops.mask_fwd) or this rank's samples ("shard")."""
    if torch.is_grad_enabled() and img.requires_grad:
        raise ops._lib.TfcError("mask_maker is forward-only (no autograd graph): call it under torch.no_grad() / on a detached image; the gradient of "
                                "the mask loss comes from tfc_gan_amd.mask_l1_loss(fake, real) or TrainStep(mask=True)")
    return ops.mask_scale(ops.mask_fwd(img, batch_scope=batch_scope))


def mask_l1_loss(fake, real, scale=1.0, want_grad=True, real_mask=None, batch_scope="global"):
    """(loss, dfake): scale * mean|mask_maker(fake) - mask_maker(real)| (4X:584-585) and its exact gradient w.r.t. fake (None without want_grad),
    through the batch extrema, their ties and both reflect-padded filters. real_mask: mask_maker(real) when the caller already has it.
    batch_scope="global" on several ranks: both masks are normalised over the gathered batch; loss is this rank's share (the mean over ranks is the
    loss of the gathered batch) and dfake the gradient of the sum of the shares, as a gradient MEAN over ranks expects (ops.mask_bwd)."""
    ops.phased_scope(batch_scope, "mask_l1_loss")
    if real_mask is None:
        real_mask = ops.mask_scale(ops.mask_fwd(real, batch_scope=batch_scope))
    loss, dfake = ops.mask_bwd(ops.mask_fwd(fake, batch_scope=batch_scope), ref=real_mask, scale=scale, want_grad=want_grad, batch_scope=batch_scope)
    return loss.reshape(()), dfake


def calculate_ffts(*patches):
    """reference :323-375: calculate_ffts(fake_B1..fake_B16, B1..B16) -> loss_FFT (scalar, no gradient). With 8 tensors (fake_B1..4, B1..4 of
    128 x 128): the inline form of the 4-patch script (4P:499-511)."""
    assert len(patches) in (8, 32), "expects 16 (or 4) fake patches followed by as many real patches"
    P = len(patches) // 2
    S = 64 if P == 16 else 128
    dev = patches[0].device
    N = patches[0].shape[0]
    out = torch.zeros(2, dtype=torch.float32, device=dev)
    scale = 1.0 / (float(P) * N * S * (S // 2 + 1))
    for k in range(P):
        _spectral_l1(lambda img: ops.fft_spectrum(img, S, 1, 1, shift=True), patches[k], patches[P + k], scale, out)
    return 0.5 * (out[0] + out[1])


# ---- temperature head (rank 1 of SURVEY.md section 8f; reference :255-268, :587-595) -------------------------------------------
T = np.linspace(24, 38, num=256)                      # reference :256 -- Celsius per uint8 code
_LUT = {}


def _temp_lut(dev):
    if dev not in _LUT:
        _LUT[dev] = torch.from_numpy(T.astype(np.float32)).to(dev)
    return _LUT[dev]


def vectorize_temps(fake_B):
    """reference :260-268: per sample ToPILImage -> red channel uint8 -> temperature LUT; returns [N,1,H,W] fp32 (no gradient)."""
    t = ops.vectorize_temps(fake_B.detach(), _temp_lut(fake_B.device))
    return t.reshape(t.shape[0], 1, t.shape[1], t.shape[2])


def temperature_triplet_loss(fake_B, TB, B_tf, lambda_t=10.0):
    """loss_temp_g of reference :587-595: criterion_temp(vectorize_temps(fake_B), TB, vectorize_temps(B_tf)) * lambda_t.
    TB: [N,H,W] (or [N,1,H,W]) ground-truth temperatures from the dataset (datasets_temp.py:66-67); B_tf: the augmented real_B
    that serves as negative (the reference draws it with torchvision ColorJitter, :591-592 -- see color_jitter_thermal)."""
    tfb = ops.vectorize_temps(fake_B.detach(), _temp_lut(fake_B.device))
    tneg = ops.vectorize_temps(B_tf.detach(), _temp_lut(fake_B.device))
    tb = TB.reshape(tfb.shape).to(tfb.device, torch.float32)
    return ops.row_triplet(tfb, tb, tneg, 1.0).reshape(()) * lambda_t


def color_jitter_params(rng, brightness=0.5, contrast=0.75, saturation=1.5, hue=0.5):
    """The random draw of transforms.ColorJitter(brightness=0.5, contrast=0.75, saturation=1.5, hue=0.5) (reference :591) as
    explicit values: op order (permutation of 0..3 = brightness, contrast, saturation, hue) and the four factors."""
    return {"order": [int(i) for i in rng.permutation(4)],
            "brightness": float(rng.uniform(max(0.0, 1 - brightness), 1 + brightness)),
            "contrast": float(rng.uniform(max(0.0, 1 - contrast), 1 + contrast)),
            "saturation": float(rng.uniform(max(0.0, 1 - saturation), 1 + saturation)),
            "hue": float(rng.uniform(-hue, hue))}


def color_jitter_thermal(real_B, params):
    """ColorJitter restricted to thermal images (R = G = B, datasets_temp.py:33): brightness and contrast are blends clamped to
    [0,1]; saturation blends with the luma 0.2989R+0.587G+0.114B (= 0.9999 v on grey); hue leaves grey pixels unchanged.
    torchvision is not installed here, so this restates its published tensor semantics -- PARITY UNPINNED; it only prepares
    the negatives of the (gradient-free) temperature term and is plain elementwise torch, not a kernel."""
    x = real_B.float()
    for op in params["order"]:
        if op == 0:
            x = (x * params["brightness"]).clamp(0.0, 1.0)
        elif op == 1:
            f = params["contrast"]
            mean = (0.9999 * x[:, :1]).mean(dim=(1, 2, 3), keepdim=True)
            x = (f * x + (1.0 - f) * mean).clamp(0.0, 1.0)
        elif op == 2:
            f = params["saturation"]
            x = (f * x + (1.0 - f) * 0.9999 * x).clamp(0.0, 1.0)
    return x


def other_spec(real_gray, fake_gray):
    """Evaluation metric of TFC-GAN-FFT/eval/Eurecom/Eurecom_MagOther.py:90-118: per image pair sklearn mean_absolute_error(log|fftshift(fft2(real))|,
    log|fftshift(fft2(fake))|) (= the mean absolute difference over the whole spectrum). Same inputs and return convention as mse_spec."""
    return mse_spec(real_gray, fake_gray, absolute=True)


def mse_spec(real_gray, fake_gray, absolute=False):
    """Evaluation metric of TFC-GAN-FFT/Devcom_MagMSE.py:91-118: per image pair MSE(log|fftshift(fft2(real))|, log|fftshift(fft2(fake))|).
    real_gray / fake_gray: uint8 grayscale images [N,256,256] (tensor or array, as cv2.imread(path, 0) yields). Returns [N] fp32."""
    def prep(g):
        t = torch.as_tensor(np.asarray(g) if not torch.is_tensor(g) else g)
        assert t.dtype == torch.uint8 and t.shape[-2:] == (256, 256), "mse_spec expects uint8 [N,256,256] gray images"
        t = t.reshape(-1, 1, 256, 256).to("cuda", non_blocking=True).float()
        return (t + 0.5) / 255.0                      # the spectrum kernel truncates x*255 back to the same uint8
    a, _ = ops.fft_spectrum(prep(real_gray), 256, 1, 1, shift=False)
    b, _ = ops.fft_spectrum(prep(fake_gray), 256, 1, 1, shift=False)
    return ops.logmag_mse(a, b, absolute=absolute)
