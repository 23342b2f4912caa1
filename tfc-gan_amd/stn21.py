"""STN21 configuration (BASELINE.json configs[4]; reference TFC-STN/TFCGAN_STN21_Original_NewModel3_Official.py, "STN") as a runnable step.

The script's generators and discriminators are the SAME classes as the PATCH-16 path (GeneratorUNet1/2 = STN:276-357 and Discriminator1/2 =
STN:360-420 match P16:136-211 layer for layer), so `GeneratorUNet` / `Discriminator1` of this package serve as all four; what the
configuration adds is

    Net (STN:170-231)          localiser (kornia VisionTransformer + MLP) -> theta -> per-sample bicubic warp            -> `Net` below
    morph_triplet (STN:444-459)                                                                                           -> stn.morph_triplet
    the training step (STN:609-672): fake_B = G1(A); fake_A1 = G2(B); warped_B = Net(A, fake_A1, src=B); fake_A2 = G2(warped_B)
        loss_G = mean(GAN1 + GAN2) + 0.01 * L1(fake_A2, A) + mean(LPIPS(fake_A2, A) + LPIPS(fake_B, B)) + morph_triplet(A, B, warped_B)
        loss_D = 0.5 * (0.25 * (...D1...) + 0.25 * (...D2...))                                                         -> `STN21Step`

Everything heavy runs on the package's HIP kernels through the modules' autograd Functions (both generators, both discriminators, the warp,
the morphological gradient, LPIPS); the generator now returns its INPUT gradient, which is how the warp and the localiser train through
`G2(warped_B)`. The localiser is 17 tokens x 768 channels (patch 64; `patch_size` 32 / 16 give the 65 / 257 tokens of the reference's other STN
scripts) and runs one of two ways (`Net.localiser`, default from TFC_LOCALISER): "torch"
(default) as plain torch layers (library GEMMs), "hip" on the package's own kernels (vit.py: one autograd Function over csrc/vit.hip, batch
invariant, compute dtype from `set_compute_dtype`). kornia is absent from this image, so `VisionTransformer` is restated from its published architecture (patch embedding, class token, learned positions, 12 pre-norm encoder blocks
with 12 heads and a 4x GELU MLP, final LayerNorm) with matmul / softmax / LayerNorm only (no MIOpen convolution, no fused attention: their
first-use compilation takes minutes on a fresh box): PARITY UNPINNED. The step keeps torch autograd across the five modules (their heavy
parts are the package's own hand-written forward / backward chains) but owns the parameters the way the PATCH-16 engine does: flat fp32
buffers, bucketed all-reduce from gradient hooks, `tfc_adam_step` -- so configuration C5 shards over GPUs like C4. A reference `model`
(STN) checkpoint does NOT load into `Net`: kornia's VisionTransformer key names are not reproduced.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import stn
from .models import Discriminator1, GeneratorUNet, Pix2PixDiscriminator, get_compute_dtype, weights_init_normal


class _Attention(nn.Module):
    """multi-head self-attention over 17 tokens as plain matmuls + softmax (library GEMMs; no fused-attention or MIOpen kernels, whose first-use
    compilation takes minutes on a fresh box)"""

    def __init__(self, dim, heads):
        super().__init__()
        self.heads = heads
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        n, t, d = x.shape
        q, k, v = self.qkv(x).reshape(n, t, 3, self.heads, d // self.heads).permute(2, 0, 3, 1, 4)
        att = torch.softmax((q @ k.transpose(-2, -1)) * (d // self.heads) ** -0.5, dim=-1)
        return self.proj((att @ v).transpose(1, 2).reshape(n, t, d))


class _EncoderBlock(nn.Module):
    def __init__(self, dim, heads, mlp_ratio=4):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = _Attention(dim, heads)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = nn.Sequential(nn.Linear(dim, mlp_ratio * dim), nn.GELU(), nn.Linear(mlp_ratio * dim, dim))

    def forward(self, x):
        x = x + self.attn(self.norm1(x))
        return x + self.mlp(self.norm2(x))


class _PatchEmbed(nn.Module):
    """Conv2d(in_channels, embed_dim, patch, stride=patch) computed as unfold + GEMM (the parameter keeps the convolution's shape and name)"""

    def __init__(self, in_channels, embed_dim, patch):
        super().__init__()
        self.patch_size = patch
        self.weight = nn.Parameter(torch.randn(embed_dim, in_channels, patch, patch) * 0.02)
        self.bias = nn.Parameter(torch.zeros(embed_dim))

    def forward(self, x):
        n, c, h, w = x.shape
        p = self.patch_size
        t = x.reshape(n, c, h // p, p, w // p, p).permute(0, 2, 4, 1, 3, 5).reshape(n, (h // p) * (w // p), c * p * p)
        return F.linear(t, self.weight.reshape(self.weight.shape[0], -1), self.bias)


class VisionTransformer(nn.Module):
    """kornia.contrib.VisionTransformer(image_size, patch_size, in_channels) restated (defaults embed_dim 768, depth 12, 12 heads): returns
    the encoded tokens [N, 1 + (image_size / patch_size)^2, 768] (class token first). Parity unpinned."""

    def __init__(self, image_size=256, patch_size=64, in_channels=6, embed_dim=768, depth=12, num_heads=12):
        super().__init__()
        self.patch = _PatchEmbed(in_channels, embed_dim, patch_size)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        n = (image_size // patch_size) ** 2 + 1
        self.positions = nn.Parameter(torch.randn(n, embed_dim) * 0.02)
        self.blocks = nn.Sequential(*[_EncoderBlock(embed_dim, num_heads) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=1e-6)

    def forward(self, x):
        t = self.patch(x)
        t = torch.cat((self.cls_token.expand(t.shape[0], -1, -1), t), 1) + self.positions
        return self.norm(self.blocks(t))


MAX_TOKENS = 1025                                                 # the tiled attention kernels' range: 512 x 512 at patch 16


def token_count(h, w, patch_size):
    """tokens of an h x w image at this patch size (patches + the class token); ValueError when the patch does not divide the image or the
    count passes MAX_TOKENS"""
    p = int(patch_size)
    if p <= 0 or h % p or w % p:
        raise ValueError(f"patch_size {patch_size!r} must be a positive divisor of the image height {h} and width {w}")
    ntok = (h // p) * (w // p) + 1
    if ntok > MAX_TOKENS:
        raise ValueError(f"patch_size {p} on a {h} x {w} image gives {ntok} tokens: the limit is {MAX_TOKENS} (512 x 512 at patch 16)")
    return ntok


class LocalizerVIT(nn.Module):
    """STN:150-163. patch_size: 64 (STN), 32, or 16 (the DarkVisible and test scripts, the archived STN17..21 scripts)"""

    def __init__(self, img_shape, patch_size=64):
        super().__init__()
        channels, self.h, self.w = img_shape
        token_count(self.h, self.w, patch_size)
        self.vit = nn.Sequential(VisionTransformer(image_size=self.h, patch_size=int(patch_size), in_channels=channels * 2))

    def forward(self, x):
        return self.vit(x)


LOCALISERS = ("torch", "hip")


def _check_localiser(v):
    if v not in LOCALISERS:
        raise ValueError(f"localiser must be one of {LOCALISERS}, got {v!r}")
    return v


def default_localiser():
    """TFC_LOCALISER from the environment: "torch" (unset) or "hip"; anything else raises ValueError"""
    return _check_localiser(os.environ.get("TFC_LOCALISER", "torch"))


class Net(nn.Module):
    """STN:170-231. forward(img_A, img_B, src): theta = identity + fc_loc(ViT(cat(img_A, img_B))), every sample of `src` warped with its own
    matrix (F.affine_grid + F.grid_sample(bicubic, border, align_corners=True), fused in tfc_affine_warp_fwd/bwd).
    localiser: "torch" (the ViT and fc_loc as torch layers), "hip" (vit.stn_phi: the package's kernels, GPU tensors only) or None (TFC_LOCALISER,
    default "torch"); readable and settable as `net.localiser`. Both run on the same parameters.
    patch_size: the ViT's patch (64 = STN; 16 = the DarkVisible and test scripts, `fc_loc[0]` = Linear(257 * 768, 1024) at 256 x 256; 32 in
    between), readable as `net.patch_size`. It must divide the image and give at most MAX_TOKENS tokens; state_dict key names do not depend on it.
    sample_align_corners: the align_corners of the grid_sample (True = STN; False = the DarkVisible script, whose grid is still align_corners=True)."""

    def __init__(self, img_shape=(3, 256, 256), localiser=None, patch_size=64, sample_align_corners=True):
        super().__init__()
        self.localiser = default_localiser() if localiser is None else localiser
        channels, h, w = img_shape
        ntok = token_count(h, w, patch_size)                      # 17 / 65 / 257 at 256 x 256 and patch 64 / 32 / 16
        self.patch_size = int(patch_size)
        self.localization = LocalizerVIT(img_shape, self.patch_size)
        self.theta_emb = nn.Linear(1, h * w)                      # declared and never used by the reference (STN:178); kept for the state_dict
        self.fc_loc = nn.Sequential(nn.Linear(ntok * 768, 1024), nn.ReLU(True), nn.Linear(1024, 512), nn.ReLU(True), nn.Linear(512, 256), nn.Sigmoid(),
                                    nn.Linear(256, 3 * 2))
        self.fc_loc[2].bias.data.zero_()                          # STN:193
        self.warp = stn.Warp(sample_align_corners)

    @property
    def localiser(self):
        return self._localiser

    @localiser.setter
    def localiser(self, v):
        object.__setattr__(self, "_localiser", _check_localiser(v))

    def stn_phi(self, x):
        if self._localiser == "hip":
            from . import vit
            return vit.stn_phi(self, x)
        xs = self.localization(x)
        return self.fc_loc(xs.reshape(xs.shape[0], -1)).view(-1, 2, 3)

    def forward(self, img_A, img_B, src):
        if self._localiser == "hip":                              # the patch embedding reads both images in place: no torch.cat
            from . import vit
            dtheta = vit.stn_phi(self, img_A, img_B)
        else:
            dtheta = self.stn_phi(torch.cat((img_A, img_B), 1))
        return self.warp(dtheta, src)


def _bce_rel(a, b, target):
    """criterion_GAN(a - b, target) with a constant target (STN:482-505: BCEWithLogitsLoss, mean over all logits)"""
    x = a - b
    return F.binary_cross_entropy_with_logits(x, torch.full_like(x, target))


def _refuse_bf16x3(who="STN21Step"):
    if get_compute_dtype() == "bf16x3":
        raise ValueError(f'{who} does not support the "bf16x3" compute mode (its ViT localiser kernels run bf16 or fp32 only): '
                         'use torch.bfloat16 or torch.float32')


class STN21Step:
    """The batch-loop body of STN:609-672 as an engine: the five networks' parameters live in TWO flat fp32 buffers in gradient-completion order
    (generator side: localiser + MLP, generator 2, generator 1 -- optimizer_G of STN:546; discriminator side: both discriminators -- optimizer_D),
    module parameters are views of them, autograd accumulates straight into the flat gradient buffers, `tfc_adam_step` updates each side in one
    launch, and -- one process per GPU, as for PATCH-16 -- the gradient buffers are sum-all-reduced in buckets that are issued from
    post-accumulate hooks while the rest of the backward still runs (the reference wraps all five modules in nn.DataParallel, STN:536-540).
    Every loss of the step is a batch mean except LPIPS, a batch SUM in lpips_pytorch: it is scaled by the world size so that the rank-averaged
    gradient equals the reference's on the gathered batch. lpips: a module with the reference's call surface (tfc_gan_amd.LPIPS) or None.
    localiser: "torch", "hip" or None (TFC_LOCALISER), and patch_size (64, 32, 16, ..), passed to `Net`. batch_invariant: True / False, or None for the global setting."""

    def __init__(self, img_shape=(3, 256, 256), lpips=None, lr=2e-4, b1=0.5, b2=0.999, device="cuda:0", alpha2=0.01, eps=1e-8, bucket_bytes=32 << 20,
                 seed=0, localiser=None, batch_invariant=None, patch_size=64):
        from . import ops, parallel
        _refuse_bf16x3(type(self).__name__)
        self.batch_invariant = batch_invariant                    # None: the global setting (set_batch_invariant / TFC_BATCH_INVARIANT) at each step
        dev = torch.device(device)
        self.dev = dev
        self.G1, self.G2 = GeneratorUNet(img_shape).to(dev), GeneratorUNet(img_shape).to(dev)
        self.D1, self.D2 = self._make_discriminator(img_shape).to(dev), self._make_discriminator(img_shape).to(dev)
        self.net = self._make_net(img_shape, localiser, patch_size).to(dev)
        for m in (self.G1, self.G2, self.D1, self.D2, self.net):
            m.apply(weights_init_normal)                          # STN:539-543
        self.lpips, self.alpha2, self._bucket_bytes = lpips, alpha2, bucket_bytes
        self.lr, self.b1, self.b2, self.eps = lr, b1, b2, eps
        self.step_no = 0
        for i, m in enumerate((self.G1, self.G2)):                # dropout streams: a function of (seed, rank, module), not of id()
            object.__setattr__(m, "_drop_seed", (seed * 7919 + parallel.rank() * 1299709 + i * 104729 + 0x5EED) & 0x7FFFFFFF)
        self._flatten()

    # gradient-completion order of loss_G.backward() on the generator side: fake_A2 = G2(warped_B) is the last forward and the first backward, the
    # localiser follows, then G2's first use finishes its gradients, G1 (the first forward) comes last
    _G_ORDER = ("net", "G2", "G1")

    def _make_discriminator(self, img_shape):
        return Discriminator1(img_shape)

    def _make_net(self, img_shape, localiser, patch_size):
        return Net(img_shape, localiser=localiser, patch_size=patch_size)

    def _flatten(self):
        """(re)build the flat buffers from the modules' current parameters (call again after load_state_dict on a module)"""
        from . import parallel
        gnamed, dnamed = {}, {}
        for pre, m in ((n + ".", getattr(self, n)) for n in self._G_ORDER):
            items = list(m.named_parameters())
            for k, p in (reversed(items) if pre == "net." else items):
                gnamed[pre + k] = p
        for pre, m in (("D1.", self.D1), ("D2.", self.D2)):
            for k, p in m.named_parameters():
                dnamed[pre + k] = p
        self.gflat = parallel.FlatParams(gnamed, list(gnamed), self.dev)
        self.dflat = parallel.FlatParams(dnamed, list(dnamed), self.dev)
        self._hooks = []
        for flat, named, side in ((self.gflat, gnamed, "g"), (self.dflat, dnamed, "d")):
            for k, p in named.items():
                p.data = flat.views[k]
                p.grad = flat.grad_views[k]
                self._hooks.append(p.register_post_accumulate_grad_hook(lambda _p, k=k, side=side: self._ready(side, k)))
        parallel.broadcast_flat(self.gflat)
        parallel.broadcast_flat(self.dflat)
        parallel.broadcast_tensors([b for D in (self.D1, self.D2) for b in D.named_core_buffers().values()])
        self.gm, self.gv = torch.zeros_like(self.gflat.data), torch.zeros_like(self.gflat.data)
        self.dm, self.dv = torch.zeros_like(self.dflat.data), torch.zeros_like(self.dflat.data)
        self.g_reduce = parallel.BucketReducer(self.gflat, self._bucket_bytes)
        self.d_reduce = parallel.BucketReducer(self.dflat, 8 << 20)
        self._bump()

    def _ready(self, side, name):
        (self.g_reduce if side == "g" else self.d_reduce).ready(name)

    def _bump(self):
        """the raw-pointer Adam kernel moves neither data_ptr nor _version of a parameter: tell the modules' operand-stream caches"""
        for m in (self.G1, self.G2, self.D1, self.D2):
            m._weights_gen += 1

    def _d_requires_grad(self, on):
        for D in (self.D1, self.D2):
            for p in D.parameters():
                p.requires_grad_(on)

    def step(self, real_A, real_B):
        from . import ops
        _refuse_bf16x3(type(self).__name__)
        with ops.batch_invariant_scope(self.batch_invariant):     # covers autograd's backward threads too: the setting is process-wide (_lib.load)
            return self._step(real_A, real_B)

    _VALID, _FAKE = 0.9, 0.0                                      # STN:613-615

    def _perc(self, fake_A, real_A, fake_B, real_B):
        if self.lpips is None:
            return fake_B.new_zeros(())
        return (self.lpips(fake_A, real_A) + self.lpips(fake_B, real_B)).mean()           # a batch SUM inside lpips_pytorch (STN:641-643)

    def _gan(self, fake_B, fake_A, real_A, real_B):
        gan1 = _bce_rel(self.D1(fake_B, real_A), self.D1(real_B, real_A).detach(), self._VALID)
        gan2 = _bce_rel(self.D2(fake_A, real_B), self.D2(real_A, real_B).detach(), self._VALID)
        return gan1 + gan2                                        # (loss_GAN1 + loss_GAN2).mean() of two scalars

    def _loss_G(self, t):
        return t["loss_GAN"] + self.alpha2 * t["recon_loss"] + t["perc_loss"] + t["morph_loss"]

    def _d_loss(self, pr, pf):
        return 0.25 * (_bce_rel(pr, pf, self._VALID) + _bce_rel(pf, pr, self._FAKE))

    def _g_update(self, loss):
        """backward of the generator side's loss (the hooks issue the bucket all-reduces as gradients become final), then its Adam step"""
        from . import ops
        loss.backward()
        gscale = self.g_reduce.finish()
        ops.adam_step(self.gflat.data, self.gflat.grad, self.gm, self.gv, self.lr, self.b1, self.b2, self.eps, self.step_no, gscale)

    def _d_step(self, real_A, real_B, fake_B, fake_A):
        """the discriminator side (STN:668-676): D1 on (real_B | fake_B) given real_A, D2 on (real_A | fake_A) given real_B, backward, Adam.
        Returns loss_D, loss_D1, loss_D2."""
        from . import ops
        self._d_requires_grad(True)
        self.dflat.grad.zero_()

        def disc(D, real, fake_img, cond):
            pr, pf = D(real, cond), D(fake_img.detach(), cond)
            return self._d_loss(pr, pf)
        loss_D1, loss_D2 = disc(self.D1, real_B, fake_B, real_A), disc(self.D2, real_A, fake_A, real_B)
        loss_D = 0.5 * (loss_D1 + loss_D2)
        loss_D.backward()
        dscale = self.d_reduce.finish()
        ops.adam_step(self.dflat.data, self.dflat.grad, self.dm, self.dv, self.lr, self.b1, self.b2, self.eps, self.step_no, dscale)
        self._bump()
        return loss_D, loss_D1, loss_D2

    def _logged(self, terms, d_losses, world, **images):
        """what step() returns: loss_G of the terms, the terms, the discriminator losses -- over several ranks their means, which for these batch
        means are the global-batch values (LPIPS, a batch sum: the sum) -- and the images"""
        from . import parallel
        terms = {k: v.detach() for k, v in terms.items()}
        out = {"loss_G": self._loss_G(terms), **terms, **{k: v.detach() for k, v in zip(("loss_D", "loss_D1", "loss_D2"), d_losses)}}
        if world > 1:
            out = {k: v * (world if k == "perc_loss" else 1.0) for k, v in parallel.all_reduce_mean_scalars(out).items()}
            out["loss_G"] = self._loss_G(out)
        out.update({k: v.detach() for k, v in images.items()})
        return out

    def _step(self, real_A, real_B):
        from . import parallel
        self.step_no += 1
        world = parallel.world_size()
        # ---------------- generators + STN (STN:620-662) ----------------
        self.gflat.grad.zero_()                                   # autograd ACCUMULATES into the flat gradient views
        self._d_requires_grad(False)                              # the reference computes (and then zeroes) discriminator gradients here: skipped
        fake_B = self.G1(real_A)
        fake_A1 = self.G2(real_B)
        warped_B = self.net(real_A, fake_A1, real_B)
        fake_A2 = self.G2(warped_B)
        recon = F.l1_loss(fake_A2, real_A)
        perc = self._perc(fake_A2, real_A, fake_B, real_B)
        morph = stn.morph_triplet(real_A, real_B, warped_B)
        loss_gan = self._gan(fake_B, fake_A2, real_A, real_B)
        terms = {"loss_GAN": loss_gan, "recon_loss": recon, "perc_loss": perc, "morph_loss": morph}
        self._g_update(loss_gan + self.alpha2 * recon + perc * world + morph)
        d_losses = self._d_step(real_A, real_B, fake_B, fake_A2)
        return self._logged(terms, d_losses, world, fake_B=fake_B, fake_A2=fake_A2, warped_B=warped_B)


class DarkVisibleStep(STN21Step):
    """The batch-loop body of TFC-STN/TFCGAN_STN21_Eur_DarkVisible.py:677-735 ("DV") on the engine of STN21Step: the same two flat fp32 buffers,
    `tfc_adam_step`, bucketed reducers from post-accumulate hooks, sharding over ranks. What differs from STN21Step:

        fake_B = G1(real_A); warped_B = Net(real_A, fake_B, src=real_B); fake_A = G2(warped_B)      (no G2(real_B) pass; G1 also trains through the
                                                                                                      localiser's input)
        recon  = L1(warped_B, fake_B), unweighted, gradient to both sides;  no morphological triplet
        FFT    = L1(amp) + L1(phase) of the whole-image spectra of (fake_A, real_A): through PIL and numpy in the reference, so a VALUE of loss_G only --
                 computed on detached images (losses.global_fft_loss) and added to nothing that is differentiated
        loss_G = GAN + recon + perc + FFT;  loss_D_k = loss_real + loss_fake;  loss_D = 0.5 (D1 + D2)
        both discriminators are the plain pix2pix PatchGAN (Pix2PixDiscriminator); Net(patch_size=16, sample_align_corners=False); lr 1e-4

    The generator side of the flat buffers is ordered by gradient completion for this wiring: G2, the localiser, G1. LPIPS is a batch sum scaled by
    the world size, as in STN21Step. fft=False skips the FFT term (loss_FFT = 0): it changes no gradient. "bf16x3" is refused, as there."""

    _G_ORDER = ("G2", "net", "G1")

    def __init__(self, img_shape=(3, 256, 256), lpips=None, lr=1e-4, b1=0.5, b2=0.999, device="cuda:0", eps=1e-8, bucket_bytes=32 << 20, seed=0,
                 localiser=None, batch_invariant=None, patch_size=16, sample_align_corners=False, fft=True):
        self._sample_align_corners = bool(sample_align_corners)
        self.fft = bool(fft)
        super().__init__(img_shape, lpips=lpips, lr=lr, b1=b1, b2=b2, device=device, eps=eps, bucket_bytes=bucket_bytes, seed=seed,
                         localiser=localiser, batch_invariant=batch_invariant, patch_size=patch_size)

    def _make_discriminator(self, img_shape):
        return Pix2PixDiscriminator(img_shape)

    def _make_net(self, img_shape, localiser, patch_size):
        return Net(img_shape, localiser=localiser, patch_size=patch_size, sample_align_corners=self._sample_align_corners)

    def _loss_G(self, t):
        return t["loss_GAN"] + t["recon_loss"] + t["perc_loss"] + t["loss_FFT"]

    def _d_loss(self, pr, pf):
        return _bce_rel(pr, pf, self._VALID) + _bce_rel(pf, pr, self._FAKE)

    def _step(self, real_A, real_B):
        from . import losses, parallel
        self.step_no += 1
        world = parallel.world_size()
        # ---------------- generators + STN (DV:677-718) ----------------
        self.gflat.grad.zero_()
        self._d_requires_grad(False)
        fake_B = self.G1(real_A)
        warped_B = self.net(real_A, fake_B, real_B)
        fake_A = self.G2(warped_B)
        recon = F.l1_loss(warped_B, fake_B)
        perc = self._perc(fake_A, real_A, fake_B, real_B)
        if self.fft:                                              # no gradient: the reference goes tensor -> PIL -> numpy (DV:551-569, :700-704)
            _, l_amp, l_pha = losses.global_fft_loss(fake_A.detach(), real_A.detach())
            loss_fft = (l_amp + l_pha).detach()
        else:
            loss_fft = fake_B.new_zeros(())
        loss_gan = self._gan(fake_B, fake_A, real_A, real_B)
        terms = {"loss_GAN": loss_gan, "recon_loss": recon, "perc_loss": perc, "loss_FFT": loss_fft}
        self._g_update(loss_gan + recon + perc * world)
        d_losses = self._d_step(real_A, real_B, fake_B, fake_A)   # DV:725-734
        return self._logged(terms, d_losses, world, fake_B=fake_B, fake_A=fake_A, warped_B=warped_B)
