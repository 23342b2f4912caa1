"""The PATCH-16 training step (reference TFCGAN_multigpu_patchFFT_16P.py:545-638) as one engine object; `patches=4` runs the same step with the
2x2 patch grid of TFCGAN_multigpu_patchFFT.py (PATCH-4, fft_mode="patch") / TFCGAN_multigpu_globalFFT.py (GLO-4, fft_mode="global").

    G step : fake = G(A); pf = D(fake, A); pr = D(B, A)
             loss_G = 0.5 * BCE(pf - pr.detach(), 0.9) + triplet16(fake, B, neg_idx) + 0.01 * patchFFT(fake, B)   (:554-607)
             backward through D (input gradient only) and G; Adam(G)
    D step : pr = D(B, A); pf = D(fake.detach(), A); loss_D = 0.5 * [BCE(pr - pf, 0.9) + BCE(pf - pr, 0)]          (:623-630)
             backward; Adam(D)

Scope notes: LPIPS (:598) needs VGG weights that cannot be fetched offline; `extra_loss_G` lets a caller
plug it in.  The temperature head (:587-595, zero gradient) is computed when the caller passes `T_B` (and the augmented
negatives `B_tf`): it adds 0.5 * loss_temp_g to the logged loss_G exactly as :607 does.  The FFT term carries no gradient in the reference (tensor -> PIL -> numpy, :300-302) and none here.  bf16 needs no
GradScaler (:518); the reference's wasted D weight-gradients during the G step (:619 zeroes them) are simply not computed.

`patches=4, region_fft="l1" | "kl"` adds the regional FFT loss of TFCGAN_multigpu_patchFFT_withregion_FFT.py ("4R", L1 form) /
..._withregion_FFT_KL.py ("4K", KL form over the batch): lambda_region * regional_fft_loss(fake, B) joins the logged loss_G (4R:606-620, 4K:623-636;
losses.region_weights gives each script's weights). It carries no gradient in the reference and none here; the discriminator step is PATCH-4's.

`patches=4, labels="generated" | "real"` runs the label-conditioned ("debiased") scripts TFCGAN_multigpu_patchFFT_debiased.py (DB1), ..._V2.py (DB2) and
..._V3.py (DB3) on GeneratorUNet(labels=3) / Discriminator1(aux_classes=(2, 4, 3)); losses.debias_weights gives each script's keywords.
    G step : fake = G(A, gl), gl = the drawn labels ("generated", DB1:504-508) or the real ones ("real", DB2:512)
             loss_G += loss_label = sum_h label_weights[h] * CE(head_h(fake, A), gl[:, h])                              (DB1:522, DB3:531)
             its gradient reaches fake through the heads' input gradient, and fc through the input gradient of down1
    D step : loss_D = 0.5 * ((loss_real + real_loss_label) + (loss_fake + fake_loss_label))                           (DB1:609)
             real_loss_label = d_label_scale * sum_h CE(head_h(B, A), labels[:, h]); fake_loss_label the same on (fake, A) against the DRAWN labels
             in every variant (DB1:603-606, DB3:612-618)
CE is the reference's nn.CrossEntropyLoss applied to the heads' Softmax output (two softmaxes), kept as it is. V4..V7 of the family (two frozen
pretrained ResNet18 classifiers) are not covered. Every term of the labelled step is per sample: it shards like PATCH-4 (tests/test_gpu_46_coupled_ddp.py).

`patches=4, mask=True` runs the edge-mask script TFCGAN_multigpu_patchFFT_experiment.py ("4X") on GeneratorUNet(mask=True); losses.mask_weights gives
its keywords.
    G step : mask_A = mask_maker(real_A) (data, no gradient); fake = G(real_A, mask_A)                                   (4X:548, :563)
             loss_G += lambda_mask * loss_mask, loss_mask = L1(mask_maker(fake), mask_maker(real_B))                      (4X:584-587)
             its exact gradient (csrc/mask.hip: batch extrema with ties, adjoints of the reflect-padded filters) joins the gradient of fake
    D step : PATCH-4's.
The mask normalises by extrema of the WHOLE batch, so the samples of a batch are coupled by definition: an explicit batch_invariant=True is refused.

`batch_scope="global"` (the default) keeps the two batch-coupled terms -- the mask's extrema, the KL form's softmax over the batch -- those of the
gathered batch on several ranks, as the reference's DataParallel computes them: their kernels run in phases and the ranks exchange the state of the
reductions in between (six small all-gathers per MASK-4 step on top of mask_A's two, one per KL step). "shard" takes them over each
rank's own samples. Without active collectives both are the same launches.
"""
import math
import os

import torch

from . import nets, ops, parallel
from .losses import global_fft_loss, mask_l1_loss, patch_fft_loss, regional_fft_loss, temperature_triplet_loss
from .ops import DT_BF16


def draw_gen_labels(N, seed, step, rank=0, classes=ops.AUX_CLASSES):
    """the generator's labels of one step, int64 numpy [N,3] -- np.random.randint(0, 2 | 4 | 3, (batch, 1)) per column in the reference (DB1:504-506), here
    a deterministic function of (seed, step, rank): reproducible, and different on every rank (each rank draws for its own shard)"""
    import numpy as np
    rng = np.random.default_rng([int(seed), int(step), int(rank), 0xDEB1A5])
    return np.stack([rng.integers(0, c, size=N) for c in classes], 1)


class TrainStep:
    def __init__(self, generator, discriminator, lr=2e-4, b1=0.5, b2=0.999, eps=1e-8, compute_dtype=torch.bfloat16,
                 fft_mode="patch", seed=0, bucket_bytes=16 << 20, lambda_gan=0.5, lambda_fft=0.01, lambda_trip=1.0, d_bucket_bytes=4 << 20,
                 batch_invariant=None, patches=16, region_fft=None, lambda_region=0.5e-4, labels=None, label_weights=(1.0, 1.0, 1.0),
                 d_label_scale=1.0, mask=False, lambda_mask=0.5, batch_scope="global"):
        dev = next(generator.parameters()).device
        ops.phased_scope(batch_scope, "TrainStep")                # refuses an unknown value
        self.batch_scope = batch_scope
        if patches not in (4, 16):
            raise ops._lib.TfcError(f"TrainStep: patches={patches} (16: the 4x4 grid of 64x64 patches, 4: the 2x2 grid of 128x128 patches)")
        self.patches = patches
        if region_fft not in (None, "l1", "kl"):
            raise ops._lib.TfcError(f"TrainStep: region_fft={region_fft!r} (None, 'l1': the L1 regional FFT loss, 'kl': its batch-softmax KL form)")
        if region_fft is not None and patches != 4:
            raise ops._lib.TfcError("TrainStep: region_fft belongs to the 4-patch scripts (patches=4); no reference script combines it with 16 patches")
        self.region_fft, self.lambda_region = region_fft, lambda_region
        if labels not in (None, "generated", "real"):
            raise ops._lib.TfcError(f"TrainStep: labels={labels!r} (None, 'generated': G is fed the drawn labels, 'real': the batch's own)")
        if labels is not None:
            if patches != 4:
                raise ops._lib.TfcError("TrainStep: labels= belongs to the label-conditioned 4-patch scripts (patches=4); no reference script combines it "
                                        "with 16 patches")
            if not getattr(generator, "labels", 0) or not getattr(discriminator, "aux_classes", None):
                raise ops._lib.TfcError("TrainStep(labels=...) needs GeneratorUNet(img_shape, labels=3) and Discriminator1(img_shape, aux_classes=(2, 4, 3))")
            if len(label_weights) != 3:
                raise ops._lib.TfcError(f"TrainStep: label_weights={label_weights!r} (three weights: gender, ethnicity, age)")
        elif getattr(generator, "labels", 0) or getattr(discriminator, "aux_classes", None):
            raise ops._lib.TfcError("TrainStep: a label-conditioned generator / discriminator needs labels='generated' or 'real' (losses.debias_weights)")
        self.labels, self.label_weights, self.d_label_scale = labels, tuple(float(w) for w in label_weights), float(d_label_scale)
        if mask:
            if patches != 4:
                raise ops._lib.TfcError("TrainStep: mask=True belongs to the edge-mask 4-patch script (patches=4); no reference script combines it with "
                                        "16 patches")
            if labels is not None:
                raise ops._lib.TfcError("TrainStep: mask=True and labels= are two different scripts (each feeds its own 4th input channel to G)")
            if not getattr(generator, "mask", False):
                raise ops._lib.TfcError("TrainStep(mask=True) needs GeneratorUNet(img_shape, mask=True)")
            if batch_invariant:
                raise ops._lib.TfcError("TrainStep(mask=True, batch_invariant=True): the mask is normalised by the extrema of the whole batch, so the "
                                        "samples of a batch are coupled by definition; there is no batch-invariant form of this step")
        elif getattr(generator, "mask", False):
            raise ops._lib.TfcError("TrainStep: a generator built with mask=True needs TrainStep(..., patches=4, mask=True) (losses.mask_weights)")
        self.mask, self.lambda_mask = bool(mask), float(lambda_mask)
        if dev.type != "cuda":
            raise ops._lib.TfcError("TrainStep needs the modules on a CUDA/HIP device (no CPU fallback)")
        self.dev, self.dt = dev, ops.dt_of(compute_dtype)
        self.G_mod, self.D_mod = generator, discriminator
        self.lr, self.b1, self.b2, self.eps = lr, b1, b2, eps
        self.lambda_gan, self.lambda_fft, self.lambda_trip = lambda_gan, lambda_fft, lambda_trip
        self.fft_mode = fft_mode
        self.seed = seed
        self.batch_invariant = batch_invariant                    # None: the global setting (set_batch_invariant / TFC_BATCH_INVARIANT) at each step
        self.step_no = 0
        # flat fp32 parameter / gradient / Adam buffers in backward order; module parameters become views of them, so
        # state_dict()/load_state_dict() keep working and stay in the reference's layout.
        self.gflat = parallel.FlatParams(generator.named_core_params(), nets.g_backward_order(), dev)
        self.dflat = parallel.FlatParams(discriminator.named_core_params(), nets.d_backward_order(), dev)
        for mod, flat in ((generator, self.gflat), (discriminator, self.dflat)):
            named = dict(mod.named_parameters())
            for k in flat.order:
                named[k].data = flat.views[k]
                named[k].grad = flat.grad_views[k]
        parallel.broadcast_flat(self.gflat)
        parallel.broadcast_flat(self.dflat)
        self.dbufs = discriminator.named_core_buffers()
        parallel.broadcast_tensors(list(self.dbufs.values()))
        self.gm, self.gv = torch.zeros_like(self.gflat.data), torch.zeros_like(self.gflat.data)
        self.dm, self.dv = torch.zeros_like(self.dflat.data), torch.zeros_like(self.dflat.data)
        self.g_reduce = parallel.BucketReducer(self.gflat, bucket_bytes)
        # the discriminator's 11 MB of gradients: its largest layer (model.9, 8.4 MB) is final first, so a 4 MiB cut lets that part of the exchange
        # run under the rest of the D backward; only the last ~2.6 MB (model.6, .3, .0) are exposed
        self.d_reduce = parallel.BucketReducer(self.dflat, min(bucket_bytes, d_bucket_bytes))
        self.G = nets.GeneratorCore(self.dt, generator.channels, getattr(generator, "labels", 0), self.mask)
        self.G.set_params(self.gflat.views)
        self.D = nets.DiscriminatorCore(self.dt, discriminator.channels, getattr(discriminator, "aux_classes", None))
        self.D.set_params(self.dflat.views, self.dbufs)
        self.G.repack()
        self.D.repack()
        self._pversions = self._param_versions()
        self.last = {}

    def _param_versions(self):
        """autograd version counters of the module parameters: they move when the CALLER writes the weights (load_state_dict,
        optimizer of its own, .apply(init)); the raw-pointer Adam kernel of this class does not touch them."""
        return tuple(p._version for m in (self.G_mod, self.D_mod) for p in m.parameters())

    def _invalidate_module_cores(self):
        """the modules' own forward (sample_images P16:391-416, eval) caches operand streams keyed on (data_ptr, _version); the Adam
        kernel changes neither, so bump the modules' weight generation after every update"""
        self.G_mod._weights_gen += 1
        self.D_mod._weights_gen += 1

    def _gl(self, like):
        return ops.new_act(like.N, like.H, like.W, 8, self.dt, self.dev)      # tfc_bce_relativistic writes whole 8-channel pixels (logit gradient, 7 zeros)

    def step(self, real_A, real_B, neg_idx=None, extra_loss_G=None, T_B=None, B_tf=None, labels=None, gen_labels=None):
        with ops.batch_invariant_scope(self.batch_invariant):     # both streams of the step launch from this thread: one setting for all of it
            return self._step(real_A, real_B, neg_idx, extra_loss_G, T_B, B_tf, labels, gen_labels)

    def _label_tensors(self, labels, gen_labels, N, t):
        """the step's two label sets as (fp32 [N,3] device, int32 [N,3] device, int32 numpy) each; checked on the host. gen_labels=None draws them as
        the reference does per step (DB1:504-506), from (seed, step, rank)."""
        if labels is None:
            raise ops._lib.TfcError("TrainStep(labels=...).step needs labels= (float or integer [N,3]: gender, ethnicity, age; batch['LAB'])")
        if gen_labels is None:
            gen_labels = draw_gen_labels(N, self.seed, t, parallel.rank(), self.D.aux_classes)
        out = []
        for v in (labels, gen_labels):
            host = ops.check_targets(v, self.D.aux_classes)
            if host.shape[0] != N:
                raise ops._lib.TfcError(f"TrainStep: {host.shape[0]} label rows for a batch of {N}")
            ti = torch.from_numpy(host).to(self.dev, non_blocking=True)
            out.append((ti.float(), ti, host))
        return out

    def _step(self, real_A, real_B, neg_idx=None, extra_loss_G=None, T_B=None, B_tf=None, labels=None, gen_labels=None):
        """real_A, real_B: fp32 NCHW [N,3,256,256] in [-1,1] on the GPU (this rank's shard). Returns a dict of device scalars.
        T_B [N,256,256] + B_tf [N,3,256,256] (augmented real_B) switch the gradient-free temperature term on.
        extra_loss_G(fake, real_B) -> (loss, dfake) runs on the SIDE stream beside the discriminator chain (with the triplet / FFT heads): it may use any
        kernel of the package except tfc_bce_relativistic, whose scalar-reduction slot belongs to the main stream's call (csrc/common.h: TfcRedSlot)."""
        dt = self.dt
        self.step_no += 1
        t = self.step_no
        if neg_idx is None:
            neg_idx = parallel.shared_neg_idx(t, self.seed, self.patches)
        if len(neg_idx) != self.patches:
            raise ops._lib.TfcError(f"TrainStep(patches={self.patches}): neg_idx has {len(neg_idx)} entries")
        drop_seed = (self.seed * 7919 + t * 104729 + parallel.rank() * 1299709) & 0x3FFFFFF
        train = self.G_mod.training
        lab = None
        if self.labels is not None:
            lab_real, lab_gen = self._label_tensors(labels, gen_labels, real_A.shape[0], t)
            lab = lab_gen if self.labels == "generated" else lab_real          # what G is fed and what its loss_label is taken against
        elif labels is not None or gen_labels is not None:
            raise ops._lib.TfcError("TrainStep.step: labels / gen_labels belong to TrainStep(labels='generated' | 'real')")
        g_labels = None if lab is None else lab[0]
        pv = self._param_versions()
        if pv != self._pversions:                                 # weights written from outside since the last step (load_state_dict): re-pack
            self.G.repack()
            self.D.repack()
            self._invalidate_module_cores()
            self._pversions = pv
        ops.arena_begin(self.dev)                                 # one fill for all the small zero-initialised buffers of this step
        # ---------------- generator step ----------------
        def pixel_losses():                                       # everything that needs only the generated image (beside the discriminator chain)
            lt, gt = ops.patch_triplet(fake, real_B, neg_idx, want_grad=True, gscale=self.lambda_trip)
            lf = patch_fft_loss(fake, real_B, self.patches) if self.fft_mode == "patch" else global_fft_loss(fake, real_B)
            ex = extra_loss_G(fake, real_B) if extra_loss_G is not None else None     # optional pluggable term (LPIPS, P16:598): (loss, dfake), already weighted
            # forward-only head: beside the other pixel losses, on their stream; (loss_FFT_reg, loss_Amp_reg, loss_Pha_reg) or None
            reg = regional_fft_loss(fake, real_B, self.region_fft, batch_scope=self.batch_scope) if self.region_fft is not None else None
            # the mask term: (lambda_mask * loss_mask, its gradient w.r.t. fake); mask(real_B) once per step. With batch_scope="global" on several ranks
            # its exchanges are issued here, on the stream the pixel losses run on, in program order like every collective of the step
            mk = mask_l1_loss(fake, real_B, scale=self.lambda_mask, batch_scope=self.batch_scope) if (self.mask and self.lambda_mask != 0.0) else None
            return lt, gt, lf, ex, reg, mk
        g_in = {"labels": g_labels}
        if self.mask:                                             # mask_A = mask_maker(real_A): Bl and its batch maximum stay on the device, the
            mctx = ops.mask_fwd(real_A, batch_scope=self.batch_scope)     # packing kernel divides on the way into input channel 3
            g_in = {"plane": mctx.bl, "plane_div": mctx.M}
        if nets.side_stream_on() and os.environ.get("TFC_NO_GSTEP_OVERLAP", "0") in ("", "0"):
            # Two-stream form of the same program (nets.py: side stream). Both power iterations of this step's two discriminator calls come first, in
            # call order (they read the weights only); the chain of the SECOND call (real pair, no gradient) then runs beside the generator forward,
            # and the triplet / FFT losses of the generated image beside the first call's chain.
            snap_f = self.D.sn_snapshot(self.dev, True, True)
            snap_r = self.D.sn_snapshot(self.dev, True, False)
            pr = nets.on_side(self.dev, lambda: self.D.chain(real_B, real_A, snap_r, save=False), snap_r[2][0])[0]
            pr_ready = nets.side_mark(self.dev)
            fake, gctx = self.G.forward(real_A, seed=drop_seed, train=train, **g_in)
            loss_trip, g_trip, (loss_fft, loss_amp, loss_pha), extra_pair, region, mask_pair = nets.on_side(self.dev, pixel_losses)
            pf, dctx_f = self.D.chain(fake, real_A, snap_f, save=True)
            nets.wait_mark(self.dev, pr_ready)                    # the logits of the real pair; the pixel losses (LPIPS: 6 ms) run on, D.backward below joins
        else:
            fake, gctx = self.G.forward(real_A, seed=drop_seed, train=train, **g_in)
            pf, dctx_f = self.D.forward(fake, real_A, power_iter=True, save=True)
            pr, _ = self.D.forward(real_B, real_A, power_iter=True, save=False)
            loss_trip, g_trip, (loss_fft, loss_amp, loss_pha), extra_pair, region, mask_pair = pixel_losses()
        g_pf = self._gl(pf)
        loss_gan = ops.bce_relativistic(dt, pf, pr, 0, 0.9, da=ops.View(g_pf.t, 1, 0), gscale=self.lambda_gan)
        g_fake = self.D.backward(dctx_f, g_pf, grads=None, need_input_grad=True)
        ops.axpby(g_fake, g_fake, g_trip, 1.0, 1.0)
        if mask_pair is not None:
            ops.axpby(g_fake, g_fake, mask_pair[1], 1.0, 1.0)
        label_out = None
        if lab is not None:
            # the heads of the fake pair, on the caller's stream on both forms of the step (same launches, same order: same bits)
            probs_g, ll_g, dl_g = ops.softmax_ce_heads(self.D.heads(dctx_f.ins[0]), lab[1], self.label_weights, 1.0, classes=self.D.aux_classes,
                                                       targets_host=lab[2])
            self.D.heads_input_grad(g_fake, dl_g)
            label_out = {"loss_label": ll_g[3], "fake_probs": probs_g}
        extra = None
        if extra_pair is not None:
            extra, g_extra = extra_pair
            ops.axpby(g_fake, g_fake, g_extra, 1.0, 1.0)
        self.G.backward(gctx, g_fake, self.gflat.grad_views, hook=self.g_reduce.ready)
        def g_update():
            gscale = self.g_reduce.finish()
            ops.adam_step(self.gflat.data, self.gflat.grad, self.gm, self.gv, self.lr, self.b1, self.b2, self.eps, t, gscale)
            self.G.repack()
        if nets.side_stream_on() and os.environ.get("TFC_NO_GUPDATE_OVERLAP", "0") in ("", "0"):
            nets.on_side(self.dev, g_update)                      # HBM-bound Adam + re-pack beside the discriminator step's first chain (joined by D.backward)
        else:
            g_update()
        # ---------------- discriminator step ----------------
        (pr2, dctx_r), (pf2, dctx_f2) = self.D.forward_pair(real_B, real_A, fake, real_A, power_iter=True, save=True)
        g_pr, g_pf2 = self._gl(pr2), self._gl(pf2)
        loss_d = ops.bce_relativistic(dt, pr2, pf2, 1, 0.9, 0.0, da=ops.View(g_pr.t, 1, 0), db=ops.View(g_pf2.t, 1, 0))
        if lab is not None:
            # real pair against the real labels, fake pair against the drawn ones; 0.5 * d_label_scale is each sum's factor in loss_D (DB1:609), so the
            # kernel's total is half the logged term (a power of two: 2 * total is the same float as the sum scaled by d_label_scale alone)
            hs = 0.5 * self.d_label_scale
            ones = (1.0, 1.0, 1.0)
            probs_r, ll_r, dl_r = ops.softmax_ce_heads(self.D.heads(dctx_r.ins[0]), lab_real[1], ones, hs, classes=self.D.aux_classes, targets_host=lab_real[2])
            probs_f, ll_f, dl_f = ops.softmax_ce_heads(self.D.heads(dctx_f2.ins[0]), lab_gen[1], ones, hs, classes=self.D.aux_classes, targets_host=lab_gen[2])
            # the heads' gradients first: they need nothing from the convolution backward, and their 14 MB bucket is the first in D's order
            self.D.heads_wgrad(dctx_r.ins[0], dl_r, dctx_f2.ins[0], dl_f, self.dflat.grad_views, accumulate=False, hook=self.d_reduce.ready)
            label_out.update(real_loss_label=2.0 * ll_r[3], fake_loss_label=2.0 * ll_f[3], d_real_probs=probs_r, d_fake_probs=probs_f)
            loss_d = loss_d + (ll_r[3] + ll_f[3])
        self.D.backward(dctx_r, g_pr, grads=self.dflat.grad_views, need_input_grad=False, accumulate=False)
        self.D.backward(dctx_f2, g_pf2, grads=self.dflat.grad_views, need_input_grad=False, accumulate=True, hook=self.d_reduce.ready)
        dscale = self.d_reduce.finish()
        ops.adam_step(self.dflat.data, self.dflat.grad, self.dm, self.dv, self.lr, self.b1, self.b2, self.eps, t, dscale)
        self.D.repack()
        ops.arena_end(self.dev)
        self._invalidate_module_cores()
        loss_g = self.lambda_gan * loss_gan + self.lambda_trip * loss_trip + self.lambda_fft * loss_fft
        if label_out is not None:
            loss_g = loss_g + label_out["loss_label"]
        if mask_pair is not None:
            loss_g = loss_g + mask_pair[0].reshape(loss_g.shape)
        if extra is not None:
            loss_g = loss_g + extra.reshape(loss_g.shape).to(loss_g.dtype)
        loss_temp = None
        if T_B is not None:
            loss_temp = temperature_triplet_loss(fake, T_B, B_tf if B_tf is not None else real_B)
            loss_g = loss_g + 0.5 * loss_temp
        self.last = {"loss_G": loss_g.reshape(()), "loss_GAN_g": loss_gan.reshape(()), "loss_triplet_patch": loss_trip.reshape(()),
                     "loss_FFT": loss_fft.reshape(()), "loss_Amp": loss_amp, "loss_Pha": loss_pha, "loss_D": loss_d.reshape(()),
                     "fake_B": fake}
        if loss_temp is not None:
            self.last["loss_temp_g"] = loss_temp
        if extra is not None:
            self.last["loss_extra_g"] = extra.reshape(())
        if label_out is not None:                                 # loss_label / real_loss_label / fake_loss_label, and the heads' probabilities [N,9]
            self.last.update({k: (v.reshape(()) if v.numel() == 1 else v) for k, v in label_out.items()})
        if self.mask:                                             # the script's loss_mask (unweighted); 0 when the term is switched off
            self.last["loss_mask"] = (mask_pair[0] / self.lambda_mask).reshape(()) if mask_pair is not None else torch.zeros((), device=self.dev)
        if region is not None:
            loss_reg, loss_amp_reg, loss_pha_reg = region
            self.last["loss_G"] = self.last["loss_G"] + self.lambda_region * loss_reg
            self.last.update(loss_FFT_reg=loss_reg, loss_Amp_reg=loss_amp_reg, loss_Pha_reg=loss_pha_reg)
        # Every logged loss is a batch mean or, for the two batch-coupled terms under batch_scope="global" (loss_mask; loss_FFT_reg, loss_Amp_reg,
        # loss_Pha_reg of region_fft="kl"), this rank's share of one: the mean over ranks is the global-batch value. Under batch_scope="shard" those
        # terms are normalised per shard and their logged values are the mean of per-shard values, not the reference's.
        if parallel.collectives_active():
            # the scalars (not fake_B, not the heads' probabilities)
            self.last.update(parallel.all_reduce_mean_scalars({k: v for k, v in self.last.items() if v.numel() == 1}))
        return self.last

    # algorithmic work of one step per image: conv / convT MACs x 2
    G_FWD_GFLOP = 23.574
    D_FWD_GFLOP = 13.224
    STEP_GFLOP = 3 * 23.574 + 4 * 13.224 + 13.224 + 2 * 2 * 13.224
