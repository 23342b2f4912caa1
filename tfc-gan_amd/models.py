"""nn.Module mirrors of the reference's network classes, running on the HIP kernels.

Same names, constructor signatures, child names (`down1..down6, up1..up5, final`, `.model` nn.Sequential indices) and
therefore the same state_dict keys / shapes as TFC-GAN-FFT/TFCGAN_multigpu_patchFFT_16P.py:102-211, so the reference's
train / test scripts (`.apply(weights_init_normal)`, `load_state_dict`, `.cuda()`, test_TFCGAN_16Patches.py's
`load_clean_state`) work unchanged.  `nn.DataParallel` (P16:444-445) is accepted as a wrapper on ONE device only: its
multi-device replicas hold no Parameters and would share one operand-stream cache across threads, so a replica's forward
raises TfcError pointing at the one-process-per-GPU path (TrainStep + parallel.py), which is how this engine scales.  The stock torch modules inside `.model` only HOLD parameters and buffers; `forward`
never calls them -- it runs the gather-GEMM / fused kernels through torch.autograd.Function wrappers.

There is no `ContrastiveLoss` / `Discriminator` class in the reference script; both names are exported as documented
aliases (see losses.py and the bottom of this file).
"""
import numpy as np
import torch
import torch.nn as nn

from . import nets, ops
from .ops import DT_BF16, DT_F32

_DEFAULT_DTYPE = torch.bfloat16


def set_compute_dtype(dtype):
    """torch.bfloat16 (default: bf16 storage, fp32 MFMA accumulate), torch.float32 (exact-fp32 parity mode) or "bf16x3" (fp32 storage, the
    convolutions as three bf16 products of split operands on the bf16 matrix cores: fp32-parity results at the bf16 MFMA rate)."""
    global _DEFAULT_DTYPE
    ops.dt_of(dtype)
    _DEFAULT_DTYPE = dtype


def get_compute_dtype():
    return _DEFAULT_DTYPE


def set_batch_invariant(on):
    """True: every launch choice that shapes the arithmetic of one sample (tile form, kernel variant, partial slots, split counts) comes from the layer's
    per-image geometry alone, so a sample's activations, statistics and gradients are bit-identical whatever batch it is computed in -- one rank with 2N
    images and two ranks with N each then differ only in how the weight gradients are summed. False (default, or TFC_BATCH_INVARIANT unset / '' / '0'):
    the launchers choose by speed for the batch at hand. At batch 32 the two settings run the same kernels. Applies to every thread of the process."""
    ops._lib.set_batch_invariant(on)


def get_batch_invariant():
    return ops._lib.get_batch_invariant()


class BlurPool(nn.Module):
    """antialiased_cnns.BlurPool(channels, stride) stand-in (third-party, un-vendored in the reference; call sites :109,
    :123, :192): reflect pad (1,2,1,2), depthwise [1,3,3,1] x [1,3,3,1] / 64, buffer `filt` [C,1,4,4]."""

    def __init__(self, channels, stride=2):
        super().__init__()
        self.channels, self.stride = channels, stride
        a = np.array([1.0, 3.0, 3.0, 1.0])
        filt = torch.tensor(a[:, None] * a[None, :], dtype=torch.float32)
        filt = filt / filt.sum()
        self.register_buffer("filt", filt[None, None].repeat(channels, 1, 1, 1))

    def forward(self, x):
        return _BlurFn.apply(x, self.stride, ops.dt_of(get_compute_dtype()))


def _to_nhwc(x, dt):
    """module-boundary plumbing for stand-alone blocks: NCHW any float dtype -> NHWC View in the compute dtype."""
    t = x.detach().permute(0, 2, 3, 1).contiguous().to(ops.torch_dtype(dt))
    return ops.View(t, t.shape[3])


def _to_nchw(v, like):
    return v.t[..., v.coff:v.coff + v.C].permute(0, 3, 1, 2).to(like.dtype)


class _BlurFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, stride, dt):
        ops.require_gpu(x)
        xv = _to_nhwc(x, dt)
        N, H, W, C = xv.t.shape
        Ho = nets.pooled(H) if stride == 2 else H
        y = ops.new_act(N, Ho, nets.pooled(W) if stride == 2 else W, C, dt, x.device)
        ops.act_fwd(dt, xv, y, stats=None, slope=1.0, pool=stride)
        ctx.meta = (stride, dt, N, H, W, C)
        return _to_nchw(y, x)

    @staticmethod
    def backward(ctx, g):
        stride, dt, N, H, W, C = ctx.meta
        gv = _to_nhwc(g, dt)
        dx = ops.new_act(N, H, W, C, dt, g.device)
        ops.act_bwd(dt, 0, gv, None, N, H, W, C, dx, stats=None, slope=1.0, pool=stride)
        return _to_nchw(dx, g), None, None


def _next_seed(module):
    """per-MODULE dropout seed stream (an LCG on an attribute of the module: no process-global mutable state)"""
    s = (getattr(module, "_drop_seed", 0x5EED ^ (id(module) & 0xFFFF)) * 1103515245 + 12345) & 0x7FFFFFFF
    object.__setattr__(module, "_drop_seed", s)
    return s


def _refuse_replica(module):
    """nn.DataParallel's replicate() marks its per-device copies `_is_replica`; they carry plain tensors instead of Parameters and share
    this module's operand-stream cache between threads -- refuse loudly instead of computing with a mix of weights"""
    if getattr(module, "_is_replica", False):
        raise ops._lib.TfcError(f"{type(module).__name__} was called inside a multi-device nn.DataParallel replica. This engine scales as one "
                                "process per GPU: launch with torch.distributed.run, build the modules on cuda:LOCAL_RANK and use "
                                "tfc_gan_amd.TrainStep (bucketed RCCL all-reduce, tfc_gan_amd.parallel) instead of nn.DataParallel (INTEGRATION.md).")


class _DownFn(torch.autograd.Function):
    """Conv2d(k4,s1,p1,no bias) -> [InstanceNorm2d] -> LeakyReLU(0.2) -> BlurPool(s2) -> [Dropout]  (reference :102-115)"""

    @staticmethod
    def forward(ctx, x, w, normalize, drop_p, seed, dt):
        ops.require_gpu(x, w)
        cout, cin = w.shape[:2]
        xv = _to_nhwc(x, dt)
        if xv.C % 8:
            t = torch.zeros((*xv.t.shape[:3], ops.pad8(xv.C)), dtype=xv.t.dtype, device=x.device)
            t[..., :xv.C] = xv.t
            xv = ops.View(t, t.shape[3])
        N, H, W, _ = xv.t.shape
        wf = w.detach().float().contiguous()
        y = ops.new_act(N, nets.pooled(H - 1), nets.pooled(W - 1), cout, dt, x.device)
        raw, stats = nets.down_block_fwd(dt, xv, cin, cout, ops.pack_weight(dt, ops.OP_CONV, 0, wf, cin, cout), y, normalize, drop_p, seed)
        ctx.saved = (xv, wf, raw, stats, drop_p, seed, dt, cin, cout)
        ctx.x_needs = x.requires_grad
        return _to_nchw(y, x)

    @staticmethod
    def backward(ctx, g):
        xv, wf, raw, stats, drop_p, seed, dt, cin, cout = ctx.saved
        N = raw.N
        d_raw = ops.new_act(N, raw.H, raw.W, cout, dt, g.device)
        nets.norm_act_bwd(dt, _to_nhwc(g, dt), raw, d_raw, stats, 0.2, 2, drop_p, seed)
        gw = torch.empty_like(wf)
        ops.conv_wgrad(dt, ops.OP_CONV, xv, d_raw, cin, cout, gw)
        gx = None
        if ctx.x_needs:
            dx = ops.new_act(N, xv.H, xv.W, ops.pad8(cin), dt, g.device)
            ops.conv_dgrad(dt, ops.OP_CONV, d_raw, N, xv.H, xv.W, cin, cout, ops.pack_weight(dt, ops.OP_CONV, 1, wf, cin, cout), dx)
            gx = _to_nchw(ops.View(dx.t, cin, 0), g)
        return gx, gw, None, None, None, None


class _UpFn(torch.autograd.Function):
    """ConvTranspose2d(k4,s2,p1,no bias) -> BlurPool(s1) -> InstanceNorm2d -> ReLU -> [Dropout]  (reference :118-130)"""

    @staticmethod
    def forward(ctx, x, w, drop_p, seed, dt):
        ops.require_gpu(x, w)
        cin, cout = w.shape[:2]
        xv = _to_nhwc(x, dt)
        N, H, W, _ = xv.t.shape
        wf = w.detach().float().contiguous()
        y = ops.new_act(N, 2 * H, 2 * W, cout, dt, x.device)
        blur, bstats = nets.up_block_fwd(dt, xv, cin, cout, ops.pack_weight(dt, ops.OP_CONVT, 0, wf, cin, cout), y, drop_p, seed)
        ctx.saved = (xv, wf, blur, bstats, drop_p, seed, dt, cin, cout)
        return _to_nchw(y, x)

    @staticmethod
    def backward(ctx, g):
        xv, wf, blur, bstats, drop_p, seed, dt, cin, cout = ctx.saved
        _, d_rawT = nets.up_block_act_bwd(dt, _to_nhwc(g, dt), blur, bstats, drop_p, seed)
        gw = torch.empty_like(wf)
        ops.conv_wgrad(dt, ops.OP_CONVT, xv, d_rawT, cin, cout, gw)
        dx = ops.new_act(xv.N, xv.H, xv.W, cin, dt, g.device)
        ops.conv_dgrad(dt, ops.OP_CONVT, d_rawT, xv.N, xv.H, xv.W, cin, cout, ops.pack_weight(dt, ops.OP_CONVT, 1, wf, cin, cout), dx)
        return _to_nchw(dx, g), gw, None, None, None


class UNetDown(nn.Module):
    def __init__(self, in_size, out_size, normalize=True, dropout=0.0):
        super().__init__()
        layers = [nn.Conv2d(in_size, out_size, 4, 1, 1, bias=False)]
        if normalize:
            layers.append(nn.InstanceNorm2d(out_size))
        layers.append(nn.LeakyReLU(0.2))
        layers.append(BlurPool(out_size, stride=2))
        if dropout:
            layers.append(nn.Dropout(dropout))
        self.model = nn.Sequential(*layers)
        self.normalize, self.dropout = bool(normalize), float(dropout)

    def forward(self, x):
        p = self.dropout if self.training else 0.0
        return _DownFn.apply(x, self.model[0].weight, self.normalize, p, _next_seed(self), ops.dt_of(get_compute_dtype()))


class UNetUp(nn.Module):
    def __init__(self, in_size, out_size, dropout=0.0):
        super().__init__()
        layers = [nn.ConvTranspose2d(in_size, out_size, 4, 2, 1, bias=False), BlurPool(out_size, stride=1),
                  nn.InstanceNorm2d(out_size), nn.ReLU(inplace=True)]
        if dropout:
            layers.append(nn.Dropout(dropout))
        self.model = nn.Sequential(*layers)
        self.dropout = float(dropout)

    def forward(self, x, skip_input):
        p = self.dropout if self.training else 0.0
        y = _UpFn.apply(x, self.model[0].weight, p, _next_seed(self), ops.dt_of(get_compute_dtype()))
        return torch.cat((y, skip_input.to(y.dtype)), 1)


class _CoreModule:
    """What the three network modules share: a core of nets.py on the module's own parameters, rebuilt when the compute dtype changes and re-packed
    when the weights do. A module gives `_make_core(dt)` and `named_core_params()`; with `_core_buffers` its `named_core_buffers()` are the core's
    second argument and part of the key."""
    _core_buffers = False

    def _init_core(self):
        self.compute_dtype = None            # None -> package default
        self._core = None
        self._core_key = None
        self._weights_gen = 0                # bumped by the step engines after each raw-pointer Adam update (neither data_ptr nor _version moves)

    def _core_for(self, device):
        dt = ops.dt_of(self.compute_dtype or get_compute_dtype())
        params = self.named_core_params()
        bufs = self.named_core_buffers() if self._core_buffers else {}
        key = ((dt, str(device), self._weights_gen) + tuple((p.data_ptr(), p._version) for p in params.values())
               + tuple(b.data_ptr() for b in bufs.values()))
        if self._core is None or self._core.dt != dt:
            self._core = self._make_core(dt)
        if key != self._core_key:
            for k, p in list(params.items()) + list(bufs.items()):
                if p.dtype != torch.float32 or not p.is_cuda:
                    raise ops._lib.TfcError(f"{type(self).__name__} {'tensor' if self._core_buffers else 'parameter'} {k} must be an fp32 CUDA tensor "
                                            f"(got {p.dtype}, {p.device})")
            self._core.set_params({k: p.detach() for k, p in params.items()}, *([dict(bufs)] if self._core_buffers else []))
            self._core.repack()
            self._core_key = key
        return self._core


class _GeneratorFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, module, x, seed, *params):
        core = module._core_for(x.device)
        fake, gctx = core.forward(x.detach().float().contiguous(), seed=seed, train=module.training)
        ctx.core, ctx.gctx, ctx.module = core, gctx, module
        return fake

    @staticmethod
    def backward(ctx, g):
        core = ctx.core
        names = nets.g_param_names()
        grads = {k: torch.empty_like(core.params[k]) for k in names}
        gx = core.backward(ctx.gctx, g, grads, need_input_grad=ctx.needs_input_grad[1])
        ctx.gctx = None
        return (None, gx, None) + tuple(grads[k] for k in names)


def _refuse_autograd(module, tensors):
    """the label-conditioned forms train through TrainStep only: their modules' own forward carries no autograd graph, so it refuses to run where one
    is expected instead of leaving None gradients behind"""
    if not (torch.is_grad_enabled() and (any(p.requires_grad for p in module.parameters())
                                         or any(torch.is_tensor(t) and t.requires_grad for t in tensors))):
        return
    if getattr(module, "mask", False):
        raise ops._lib.TfcError(f"{type(module).__name__}: the mask-fed forward (edge mask as the 4th input channel) has no autograd backward. Train with "
                                "tfc_gan_amd.TrainStep(G, D, patches=4, mask=True, **tfc_gan_amd.mask_weights()), which runs its hand-written backward; "
                                "call the module itself under torch.no_grad() (sample_images, inference).")
    raise ops._lib.TfcError(f"{type(module).__name__}: the label-conditioned forward (label plane / auxiliary heads) has no autograd backward. Train with "
                            "tfc_gan_amd.TrainStep(G, D, **tfc_gan_amd.debias_weights(kind), patches=4), which runs its hand-written backward; "
                            "call the module itself under torch.no_grad() (sample_images, inference).")


class GeneratorUNet(_CoreModule, nn.Module):
    """reference :136-174. forward(x[N,3,S,S]) -> fake_B in (-1,1), fp32 NCHW (the reference casts to HalfTensor, :173).
    labels=3: the label-conditioned generator of TFCGAN_multigpu_patchFFT_debiased.py:142-186 -- fc = nn.Linear(3, h*w) of the labels, reshaped to a
    plane, is the 4th input channel of down1; forward(x, labels[N,3]).
    mask=True: the generator of TFCGAN_multigpu_patchFFT_experiment.py:141-181 -- the edge mask of img_A (tfc_gan_amd.mask_maker) is the 4th input
    channel of down1; forward(img_A, mask_A[N,1,S,S]). One of labels= and mask= at most."""

    def __init__(self, img_shape, labels=0, mask=False):
        super().__init__()
        channels, self.h, self.w = img_shape
        if labels not in (0, 3):
            raise ops._lib.TfcError(f"GeneratorUNet: labels={labels} (0: the plain generator, 3: gender / ethnicity / age through fc)")
        if labels and mask:
            raise ops._lib.TfcError("GeneratorUNet: labels= and mask= are mutually exclusive (each script feeds its own 4th input channel)")
        self.labels = labels
        self.mask = bool(mask)
        if labels:
            self.fc = nn.Linear(labels, self.h * self.w)        # first, as in the reference: state_dict() lists fc.* ahead of down1
        self.down1 = UNetDown(channels + (1 if (labels or mask) else 0), 64, normalize=False)
        self.down2 = UNetDown(64, 128)
        self.down3 = UNetDown(128, 256, dropout=0.5)
        self.down4 = UNetDown(256, 512, dropout=0.5)
        self.down5 = UNetDown(512, 512, normalize=False)
        self.down6 = UNetDown(512, 512)
        self.up1 = UNetUp(512, 512)
        self.up2 = UNetUp(1024, 512, dropout=0.5)
        self.up3 = UNetUp(1024, 256, dropout=0.5)
        self.up4 = UNetUp(512, 128)
        self.up5 = UNetUp(256, 64)
        self.final = nn.Sequential(nn.Upsample(scale_factor=2), nn.ZeroPad2d((1, 0, 1, 0)), nn.Conv2d(128, channels, 4, padding=1), nn.Tanh())
        self.channels = channels
        self._init_core()

    def named_core_params(self):
        sd = dict(self.named_parameters())
        return {k: sd[k] for k in nets.g_param_names(self.labels)}

    def _make_core(self, dt):
        return nets.GeneratorCore(dt, self.channels, self.labels, self.mask)

    def forward(self, x, labels=None, mask_A=None):
        _refuse_replica(self)
        if self.mask:
            if mask_A is None:                                    # forward(img_A, mask_A): the mask is this generator's second argument
                mask_A, labels = labels, None
            if labels is not None or mask_A is None:
                raise ops._lib.TfcError("GeneratorUNet(img_shape, mask=True): forward(img_A, mask_A) with mask_A [N,1,S,S] (tfc_gan_amd.mask_maker(img_A))")
            _refuse_autograd(self, (x, mask_A))
            core = self._core_for(x.device)
            fake, _ = core.forward(x.detach().float().contiguous(), seed=_next_seed(self), train=self.training, save=False,
                                   plane=mask_A.detach().to(x.device).float().contiguous())
            return fake
        if mask_A is not None:
            raise ops._lib.TfcError("GeneratorUNet: forward(img_A, mask_A) belongs to GeneratorUNet(img_shape, mask=True)")
        if (labels is not None) != bool(self.labels):
            raise ops._lib.TfcError("GeneratorUNet: forward(x, labels) belongs to GeneratorUNet(img_shape, labels=3), forward(x) to the plain generator")
        if self.labels:
            _refuse_autograd(self, (x, labels))
            core = self._core_for(x.device)
            fake, _ = core.forward(x.detach().float().contiguous(), seed=_next_seed(self), train=self.training, save=False,
                                   labels=labels.detach().to(x.device).float())
            return fake
        params = self.named_core_params()
        return _GeneratorFn.apply(self, x, _next_seed(self), *params.values())


class _PatchGANFn(torch.autograd.Function):
    """both discriminators: `params` are the module's named_core_params() and `names` their keys; `fwd_kw` is what its core's forward takes beside
    the two images"""

    @staticmethod
    def forward(ctx, module, names, fwd_kw, img_a, img_b, *params):
        core = module._core_for(img_a.device)
        logits, dctx = core.forward(img_a.detach().float().contiguous(), img_b.detach().float().contiguous(), **fwd_kw)
        ctx.core, ctx.dctx, ctx.names = core, dctx, names
        ctx.need_a = img_a.requires_grad
        ctx.need_w = any(p.requires_grad for p in params)
        N, H, W = logits.N, logits.H, logits.W
        return logits.t[..., 0].reshape(N, 1, H, W).float()

    @staticmethod
    def backward(ctx, g):
        core, dctx, names = ctx.core, ctx.dctx, ctx.names
        N, _, H, W = g.shape
        gl = ops.new_act(N, H, W, 8, core.dt, g.device, zero=True)
        gl.t[..., 0] = g.reshape(N, H, W).to(gl.t.dtype)
        grads = {k: torch.empty_like(core.params[k]) for k in names} if ctx.need_w else None
        ga = core.backward(dctx, gl, grads, need_input_grad=ctx.need_a)
        ctx.dctx = None
        return (None, None, None, ga, None) + (tuple(grads[k] for k in names) if grads else (None,) * len(names))


class Discriminator1(_CoreModule, nn.Module):
    """reference :182-211 (spectral-norm PatchGAN). forward(img_A, img_B) -> logits [N,1,S/16,S/16] fp32.
    aux_classes=(2, 4, 3): the label-conditioned discriminator of TFCGAN_multigpu_patchFFT_debiased.py:194-233 -- aux_gender / aux_ethn / aux_age, each
    nn.Sequential(nn.Linear(6*h*w, C), nn.Softmax()) on the flattened input; forward then returns (logits, gender_hat, ethn_hat, age_hat)."""
    _core_buffers = True                     # u / v of the spectral norm: the core updates them in place

    def __init__(self, img_shape, aux_classes=None):
        super().__init__()
        channels, self.h, self.w = img_shape

        def discriminator_block(in_filters, out_filters):
            return [torch.nn.utils.parametrizations.spectral_norm(nn.Conv2d(in_filters, out_filters, 4, stride=1, padding=1)),
                    nn.LeakyReLU(0.2, inplace=True), BlurPool(out_filters, stride=2)]

        self.model = nn.Sequential(*discriminator_block(channels * 2, 64), *discriminator_block(64, 128),
                                   *discriminator_block(128, 256), *discriminator_block(256, 512),
                                   nn.ZeroPad2d((1, 0, 1, 0)), nn.Conv2d(512, 1, 4, padding=1, bias=False))
        self.aux_classes = tuple(aux_classes) if aux_classes else None
        if self.aux_classes:
            if self.aux_classes != tuple(c for _, c in nets.D_AUX):
                raise ops._lib.TfcError(f"Discriminator1: aux_classes={aux_classes} (None, or (2, 4, 3): gender, ethnicity, age as in the reference)")
            for name, c in nets.D_AUX:
                setattr(self, name, nn.Sequential(nn.Linear(channels * 2 * self.h * self.w, c), nn.Softmax(dim=1)))
        self.channels = channels
        self._init_core()

    def named_core_params(self):
        sd = dict(self.named_parameters())
        return {k: sd[k] for k in nets.d_param_names(bool(self.aux_classes))}

    def _make_core(self, dt):
        return nets.DiscriminatorCore(dt, self.channels, self.aux_classes)

    def named_core_buffers(self):
        sd = dict(self.named_buffers())
        out = {}
        for i, _, _ in nets.D_BLOCKS:
            for s in ("_u", "_v"):
                k = f"model.{i}.parametrizations.weight.0.{s}"
                out[k] = sd[k]
        return out

    def forward(self, img_A, img_B):
        _refuse_replica(self)
        if self.aux_classes:
            _refuse_autograd(self, (img_A, img_B))
            core = self._core_for(img_A.device)
            x8 = ops.pack_nhwc8(core.dt, img_A.detach().float(), img_B.detach().float())
            logits, _ = core.forward(img_A.detach().float().contiguous(), img_B.detach().float().contiguous(), power_iter=self.training, save=False)
            N = x8.N
            probs, _, _ = ops.softmax_ce_heads(core.heads(x8), torch.zeros((N, 3), dtype=torch.int32, device=img_A.device), want_grad=False,
                                               classes=self.aux_classes)
            hats = torch.split(probs, list(self.aux_classes), dim=1)
            return (logits.t[..., 0].reshape(N, 1, logits.H, logits.W).float(),) + tuple(h.contiguous() for h in hats)
        params = self.named_core_params()
        return _PatchGANFn.apply(self, tuple(params), {"power_iter": self.training}, img_A, img_B, *params.values())


class Pix2PixDiscriminator(_CoreModule, nn.Module):
    """The plain pix2pix PatchGAN of TFC-STN/TFCGAN_STN21_Eur_DarkVisible.py:370-423 (its Discriminator1 / Discriminator2, and the same block in the
    archived STN scripts, cyclegan_og and ThermalGAN): four blocks Conv2d(k4, stride 2, p1, bias) -> [InstanceNorm2d, not the first] ->
    LeakyReLU(0.2), then ZeroPad2d((1, 0, 1, 0)) + Conv2d(512, 1, 4, padding=1, bias=False). No spectral norm, no BlurPool.
    forward(img_A, img_B) -> logits [N, 1, H/16, W/16] fp32 (H, W multiples of 16); state_dict keys model.{0,2,5,8}.{weight,bias}, model.12.weight.
    Gradients: all five weights, the bias of block 1, and img_A (the generators train through it). The biases of blocks 2-4 sit in front of an
    InstanceNorm: their gradient is mathematically zero, torch returns rounding noise there, this module returns exact zeros."""

    def __init__(self, img_shape):
        super().__init__()
        self.channels, self.h, self.w = (int(v) for v in img_shape)
        # the table of nets.Pix2PixCore places every module at the index the state_dict keys name: a convolution per entry, its InstanceNorm where
        # the entry has one, LeakyReLU behind both, and the padded head at P2P_HEAD
        mods, cin = {}, 2 * self.channels
        for idx, cout, norm in nets.P2P_BLOCKS:
            mods[idx] = nn.Conv2d(cin, cout, kernel_size=4, stride=2, padding=1, bias=True)
            if norm:
                mods[idx + 1] = nn.InstanceNorm2d(cout)
            mods[idx + 1 + int(norm)] = nn.LeakyReLU(0.2, inplace=True)
            cin = cout
        mods[nets.P2P_HEAD - 1] = nn.ZeroPad2d((1, 0, 1, 0))
        mods[nets.P2P_HEAD] = nn.Conv2d(cin, 1, kernel_size=4, padding=1, bias=False)
        assert sorted(mods) == list(range(nets.P2P_HEAD + 1))
        self.model = nn.Sequential(*(mods[i] for i in range(nets.P2P_HEAD + 1)))
        self._init_core()

    def named_core_params(self):
        sd = dict(self.named_parameters())
        return {k: sd[k] for k in nets.p2p_param_names()}

    def named_core_buffers(self):
        return {}

    def _make_core(self, dt):
        return nets.Pix2PixCore(dt, self.channels)

    def forward(self, img_A, img_B):
        _refuse_replica(self)
        params = self.named_core_params()
        return _PatchGANFn.apply(self, tuple(params), {}, img_A, img_B, *params.values())


class _TrunkFn(torch.autograd.Function):
    """the residual trunk (nets.ResNetTrunkCore) at the fp32 NCHW module boundary: one pack to NHWC in front of it, one unpack behind it.
    `params` are the module's named_core_params() in the order of its core's param_names()."""

    @staticmethod
    def forward(ctx, module, x, *params):
        ops.require_gpu(x)
        core = module._core_for(x.device)
        y, tctx = core.forward(_to_nhwc(x, core.dt))
        ctx.core, ctx.tctx = core, tctx
        ctx.need_w = any(p.requires_grad for p in params)
        return _to_nchw(y, x)

    @staticmethod
    def backward(ctx, g):
        core = ctx.core
        names = core.param_names()
        grads = {k: torch.empty_like(core.params[k]) for k in names} if ctx.need_w else None
        gv = _to_nhwc(g, core.dt)
        if gv.t.data_ptr() == g.data_ptr():                       # a channels-last fp32 gradient: the core updates its argument in place
            gv = ops.View(gv.t.clone(), gv.C)
        gx = core.backward(ctx.tctx, gv, grads)
        ctx.tctx = None
        return (None, _to_nchw(gx, g)) + (tuple(grads[k] for k in names) if grads else (None,) * len(names))


def _reflect_pad(x, p):
    """nn.ReflectionPad2d(p) as slices, flips and concatenations: the same values, and a backward of plain additions -- torch's own
    reflection_pad2d backward scatters with float atomics on the GPU, which would make every gradient in front of it vary from run to run"""
    x = torch.cat((x[..., 1:p + 1].flip(-1), x, x[..., -p - 1:-1].flip(-1)), -1)
    return torch.cat((x[..., 1:p + 1, :].flip(-2), x, x[..., -p - 1:-1, :].flip(-2)), -2)


def _run_layers(layers, x):
    """the torch layers of a GeneratorResNet in order, its ReflectionPad2d modules (which hold nothing) through _reflect_pad"""
    for m in layers:
        if isinstance(m, nn.ReflectionPad2d):
            x = _reflect_pad(x, m.padding[0])
        else:
            x = m.forward_torch(x) if isinstance(m, ResidualBlock) else m(x)
    return x


class ResidualBlock(_CoreModule, nn.Module):
    """cyclegan_og/models.py:29-46: x + [ReflectionPad2d(1), Conv2d(C, C, 3), InstanceNorm2d, ReLU, ReflectionPad2d(1), Conv2d(C, C, 3),
    InstanceNorm2d](x). state_dict keys block.{1,5}.{weight,bias}. forward: fp32 NCHW in and out on the HIP kernels (one-block nets.ResNetTrunkCore);
    the stock torch modules inside `.block` hold the parameters and serve forward_torch(), the A/B partner and the CPU path."""

    def __init__(self, in_features):
        super().__init__()
        C = int(in_features)
        self.block = nn.Sequential(nn.ReflectionPad2d(1), nn.Conv2d(C, C, 3), nn.InstanceNorm2d(C), nn.ReLU(inplace=True),
                                   nn.ReflectionPad2d(1), nn.Conv2d(C, C, 3), nn.InstanceNorm2d(C))
        self.features = C
        self._init_core()

    def named_core_params(self):
        sd = dict(self.named_parameters())
        return {k: sd[k] for k in nets.res_block_keys("")}

    def _make_core(self, dt):
        return nets.ResNetTrunkCore(dt, self.features, 1, prefixes=[""])

    def forward_torch(self, x):
        return x + _run_layers(self.block, x)

    def forward(self, x):
        _refuse_replica(self)
        return _TrunkFn.apply(self, x, *self.named_core_params().values())


RESNET_TRUNK_FIRST = 10                  # index of the first residual block inside GeneratorResNet.model


class GeneratorResNet(_CoreModule, nn.Module):
    """CycleGAN's generator, cyclegan_og/models.py:49-102, with the reference's state_dict keys (model.1 / .4 / .7 the stem and the two stride-2
    convolutions, model.10 ... model.{9 + n} the residual blocks, then the two upsample convolutions and the 7 x 7 head: model.20 / .24 / .28 at n = 9).
    forward(x [N, channels, H, W]) -> fp32 NCHW in (-1, 1); H and W multiples of 4.
    trunk="hip": the residual blocks -- 76 % of the arithmetic at 256 x 256 with 9 blocks -- run on nets.ResNetTrunkCore; the stem, the two stride-2
    convolutions, the two upsample convolutions and the head are torch layers in fp32. trunk="torch": the whole module as torch layers (the A/B
    partner, and the CPU path)."""

    def __init__(self, input_shape, num_residual_blocks, trunk="hip"):
        super().__init__()
        if trunk not in ("hip", "torch"):
            raise ops._lib.TfcError(f"GeneratorResNet: trunk={trunk!r} (\"hip\": residual blocks on the HIP kernels, \"torch\": torch layers throughout)")
        channels = int(input_shape[0])
        self.channels, self.num_residual_blocks, self.trunk = channels, int(num_residual_blocks), trunk
        feats = 64
        # the reference pads by `channels` in front of its 7 x 7 convolutions (3 only because the images have 3 channels); kept as it is
        layers = [nn.ReflectionPad2d(channels), nn.Conv2d(channels, feats, 7), nn.InstanceNorm2d(feats), nn.ReLU(inplace=True)]
        for _ in range(2):
            layers += [nn.Conv2d(feats, 2 * feats, 3, stride=2, padding=1), nn.InstanceNorm2d(2 * feats), nn.ReLU(inplace=True)]
            feats *= 2
        assert len(layers) == RESNET_TRUNK_FIRST
        self.features = feats
        layers += [ResidualBlock(feats) for _ in range(self.num_residual_blocks)]
        for _ in range(2):
            layers += [nn.Upsample(scale_factor=2), nn.Conv2d(feats, feats // 2, 3, stride=1, padding=1), nn.InstanceNorm2d(feats // 2),
                       nn.ReLU(inplace=True)]
            feats //= 2
        layers += [nn.ReflectionPad2d(channels), nn.Conv2d(feats, channels, 7), nn.Tanh()]
        self.model = nn.Sequential(*layers)
        self._init_core()

    def _prefixes(self):
        return nets.res_prefixes(self.num_residual_blocks, RESNET_TRUNK_FIRST, "model.")

    def named_core_params(self):
        sd = dict(self.named_parameters())
        return {k: sd[k] for p in self._prefixes() for k in nets.res_block_keys(p)}

    def _make_core(self, dt):
        return nets.ResNetTrunkCore(dt, self.features, self.num_residual_blocks, prefixes=self._prefixes())

    def forward(self, x):
        _refuse_replica(self)
        end = RESNET_TRUNK_FIRST + self.num_residual_blocks
        if self.trunk == "torch":
            return _run_layers(self.model, x)
        ops.require_gpu(x)
        x = _run_layers(self.model[:RESNET_TRUNK_FIRST], x.float())
        if self.num_residual_blocks:
            x = _TrunkFn.apply(self, x, *self.named_core_params().values())
        return _run_layers(self.model[end:], x)


# The reference script names the class Discriminator1; older scripts of the same repo (TFC-STN/archive/*) call the identical
# class Discriminator -- north_star uses that name.
Discriminator = Discriminator1


def weights_init_normal(m):
    """reference :218-224: N(0, 0.02) on every module whose class name contains "Conv" (BatchNorm2d: N(1, 0.02), bias 0)."""
    classname = m.__class__.__name__
    if classname.find("Conv") != -1:
        torch.nn.init.normal_(m.weight.data, 0.0, 0.02)
    elif classname.find("BatchNorm2d") != -1:
        torch.nn.init.normal_(m.weight.data, 1.0, 0.02)
        torch.nn.init.constant_(m.bias.data, 0.0)
