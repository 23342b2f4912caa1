"""Forward / backward orchestration of the networks on the HIP kernels.

`GeneratorCore` mirrors GeneratorUNet (reference TFCGAN_multigpu_patchFFT_16P.py:136-174), `DiscriminatorCore` mirrors
Discriminator1 (:182-211), `Pix2PixCore` the plain PatchGAN of the DarkVisible script, `ResNetTrunkCore` the residual blocks of CycleGAN's
GeneratorResNet (cyclegan_og/models.py:29-46).  All work on raw NHWC buffers and hand-written
backward chains (no autograd inside); the nn.Module mirrors in models.py wrap them in torch.autograd.Function, and engine.py calls them directly.

Layout: the side stream, the tables and parameter names, then the BLOCK STEPS -- every sequence of launches that more than one network runs (a
block's forward, its activation backward, a parameter gradient on the side stream with its hooks, the PatchGAN head, operand-stream planning),
each written once as a plain function -- and the three cores, whose loops are built from those steps. The stand-alone UNetDown / UNetUp of
models.py call the same steps.

Skip connections never copy: each UNetUp output and its skip tensor are two channel windows of ONE concat buffer,
the down path writes its pooled output straight into the skip window, and the transposed convolution reads the whole
buffer (reference torch.cat, :133).  Gradients mirror that: the convT dgrad writes the whole concat gradient, the
down path accumulates into its window.
"""
import os

import torch

from . import ops
from .ops import (DT_BF16, OP_CONV, OP_CONV2, OP_CONV3R, OP_CONVT, OP_PADCONV, OP_UPCONV, View, new_act)

# Weight gradients on a second HIP stream. The weight gradient of layer i needs only the gradient of its output, which the main chain (input gradient ->
# activation backward -> next layer) has finished with, so it runs beside that chain and fills the tails of its persistent launches (same-box A/B:
# 10.22 -> 10.05 ms per step). Everything that touches a layer's parameter gradients (wgrad, spectral-norm backward, bias column sum, the all-reduce
# hook) stays together on the side stream, in program order; backward() joins before it returns. Results are bit-identical either way (no atomics
# cross the streams). TFC_WGRAD_STREAM=0 or set_wgrad_stream(False) serialises everything on the caller's stream (bench.py does that in its
# instrumented steps, so that a launch's duration is kernel time).
_SIDE = {"on": os.environ.get("TFC_WGRAD_STREAM", "1") not in ("", "0"), "streams": {}}


def set_wgrad_stream(on):
    """weight gradients on a second stream (default) or in line on the caller's stream; returns the previous setting"""
    prev, _SIDE["on"] = _SIDE["on"], bool(on)
    return prev


def side_stream_on():
    """side stream in use? Not under a gloo process group: its collectives on device tensors block the host until the stream they were issued on has
    drained, which serialises the two streams the hard way (one-card rehearsal, 2 ranks: 53 ms per step on one stream, 180-500 ms on two). RCCL's are
    stream-ordered and return at once."""
    if not _SIDE["on"]:
        return False
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_backend() == "gloo":
        return False
    return True


def _side_stream(dev):
    st = _SIDE["streams"].get(dev)
    if st is None:
        st = _SIDE["streams"][dev] = torch.cuda.Stream(dev)
    return st


def on_side(dev, fn, *tensors):
    """run fn() on the side stream behind everything queued on the current stream so far; `tensors` are temporaries fn reads that the caller drops
    before the join (the caching allocator must not hand them out again until the side stream is done with them); a None among them is skipped"""
    if not side_stream_on():
        return fn()
    cur, st = torch.cuda.current_stream(dev), _side_stream(dev)
    st.wait_stream(cur)
    with torch.cuda.stream(st):
        out = fn()
    for t in tensors:
        if t is not None:
            (t.t if isinstance(t, View) else t).record_stream(st)
    return out


def join_side(dev):
    if side_stream_on():
        torch.cuda.current_stream(dev).wait_stream(_side_stream(dev))


def side_mark(dev):
    """an event behind everything queued on the side stream so far (None when the side stream is not in use); wait_mark() makes the caller's stream wait
    for it -- a partial join: what was queued on the side stream AFTER the mark keeps running beside the caller"""
    if not side_stream_on():
        return None
    ev = torch.cuda.Event()
    ev.record(_side_stream(dev))
    return ev


def wait_mark(dev, ev):
    if ev is not None:
        torch.cuda.current_stream(dev).wait_event(ev)

# (name, Cin, Cout, normalize, dropout)  -- reference :140-145
G_DOWN = [("down1", 3, 64, False, 0.0), ("down2", 64, 128, True, 0.0), ("down3", 128, 256, True, 0.5),
          ("down4", 256, 512, True, 0.5), ("down5", 512, 512, False, 0.0), ("down6", 512, 512, True, 0.0)]
# (name, Cin, Cout, dropout, skip = index of the down block concatenated)  -- reference :147-151
G_UP = [("up1", 512, 512, 0.0, 4), ("up2", 1024, 512, 0.5, 3), ("up3", 1024, 256, 0.5, 2), ("up4", 512, 128, 0.0, 1),
        ("up5", 256, 64, 0.0, 0)]
# (index in nn.Sequential, Cin, Cout)  -- reference :194-202
D_BLOCKS = [(0, 6, 64), (3, 64, 128), (6, 128, 256), (9, 256, 512)]


def down_weight_key(name):
    return f"{name}.model.0.weight"


G_FC = ["fc.weight", "fc.bias"]         # the label plane of the label-conditioned generator (TFCGAN_multigpu_patchFFT_debiased.py:149)
# the auxiliary classifier heads of the label-conditioned discriminator (..._debiased.py:218-220): (child name, classes)
D_AUX = [("aux_gender", 2), ("aux_ethn", 4), ("aux_age", 3)]


def g_param_names(labels=0):
    names = [down_weight_key(n) for n, *_ in G_DOWN] + [f"{n}.model.0.weight" for n, *_ in G_UP]
    return names + ["final.2.weight", "final.2.bias"] + (G_FC if labels else [])


def g_backward_order():
    """Parameter names in the order their gradients become final during backward (bucket order for DDP). fc.* (label-conditioned generator only) come
    last: they hang off the input gradient of down1."""
    return (["final.2.weight", "final.2.bias"] + [f"{n}.model.0.weight" for n, *_ in reversed(G_UP)]
            + [down_weight_key(n) for n, *_ in reversed(G_DOWN)] + G_FC)


def d_aux_names():
    out = []
    for n, _ in D_AUX:
        out += [f"{n}.0.weight", f"{n}.0.bias"]
    return out


def d_param_names(aux=False):
    out = []
    for i, _, _ in D_BLOCKS:
        out += [f"model.{i}.bias", f"model.{i}.parametrizations.weight.original"]
    return out + ["model.13.weight"] + (d_aux_names() if aux else [])


def d_backward_order():
    """the heads' parameters (label-conditioned discriminator only) come first: their gradients need nothing from the convolution backward, so their
    14 MB bucket can leave before it starts"""
    out = d_aux_names() + ["model.13.weight"]
    for i, _, _ in reversed(D_BLOCKS):
        out += [f"model.{i}.parametrizations.weight.original", f"model.{i}.bias"]
    return out


# the pix2pix PatchGAN of the DarkVisible script (TFC-STN/TFCGAN_STN21_Eur_DarkVisible.py:370-423): (index in nn.Sequential, Cout, InstanceNorm);
# the first block reads 2 * channels inputs, the head is model.12
P2P_BLOCKS = [(0, 64, False), (2, 128, True), (5, 256, True), (8, 512, True)]
P2P_HEAD = 12


def p2p_param_names():
    out = []
    for i, _, _ in P2P_BLOCKS:
        out += [f"model.{i}.weight", f"model.{i}.bias"]
    return out + [f"model.{P2P_HEAD}.weight"]


def p2p_backward_order():
    out = [f"model.{P2P_HEAD}.weight"]
    for i, _, _ in reversed(P2P_BLOCKS):
        out += [f"model.{i}.weight", f"model.{i}.bias"]
    return out


def pooled(h):
    return (h - 1) // 2 + 1


class _Ctx:
    pass


# ---- block steps: every sequence of launches that more than one network runs, written once ------------------------------------------------------
# The cores below and the stand-alone blocks of models.py are loops and call sequences over these. A `core` argument is any of the three cores:
# the steps read its dt and debug, and keep the persistent weight-gradient scratch in its _ws.

def plan_streams(dt, entries, packed):
    """one PackPlan for the operand streams of a network. entries: (slot, op, pass, weight, Cin, Cout); every stream is filed as packed[slot]"""
    plan = ops.PackPlan(dt, [e[1:] for e in entries])
    for (slot, *_), buf in zip(entries, plan.streams):
        packed[slot] = buf
    return plan


def param_grad(dev, work, hook=None, keys=(), keep=()):
    """a parameter gradient, the way every one of them runs: work() on the side stream, hook(key) for each of `keys` behind it in that order (the
    bucket reducers count on it), the temporaries `keep` that work() reads held until the side stream is done with them. Returns what work() returns;
    the caller's backward() joins."""
    def run():
        out = work()
        if hook:
            for k in keys:
                hook(k)
        return out
    return on_side(dev, run, *keep)


def bias_grad(sums, gbias, accumulate):
    """bias gradient from the per-image sums [N, Cout] an activation backward left behind: zero unless accumulating, then their column sum.
    sums None: a bias in front of an InstanceNorm, whose gradient is exactly zero."""
    if not accumulate:
        gbias.zero_()
    if sums is not None:
        N, cout = sums.shape
        ops.colsum(ops.DT_F32, View(sums.view(N, 1, 1, cout), cout), gbias)


def norm_act_bwd(dt, g, x, d_x, stats, slope, pool, drop_p=0.0, seed=0, bias_sums=None):
    """backward of [InstanceNorm] -> activation(slope) -> [BlurPool(pool)] -> [Dropout] into d_x, which gives the sizes. stats (of the forward): the
    reduction pass (mode 1) into fresh rstats, then the pass that uses them (mode 2). stats None: one pass (mode 0), which also leaves the per-image
    sums of d_x -- the bias gradient of the convolution in front -- in bias_sums where the caller gives that buffer."""
    N, H, W, C = d_x.N, d_x.H, d_x.W, d_x.C
    if stats is not None:
        rstats = ops.zeros_f32((N, C, 2), d_x.t.device)
        ops.act_bwd(dt, 1, g, x, N, H, W, C, None, stats=stats, slope=slope, pool=pool, drop_p=drop_p, seed=seed, rstats=rstats)
        ops.act_bwd(dt, 2, g, x, N, H, W, C, d_x, stats=stats, slope=slope, pool=pool, drop_p=drop_p, seed=seed, rstats=rstats)
    else:
        ops.act_bwd(dt, 0, g, x, N, H, W, C, d_x, stats=None, slope=slope, pool=pool, drop_p=drop_p, seed=seed, rstats=bias_sums)


def down_block_fwd(dt, x, cin, cout, packed, dst, normalize, drop_p=0.0, seed=0):
    """Conv2d(k4,s1,p1,no bias) -> [InstanceNorm2d] -> LeakyReLU(0.2) -> BlurPool(s2) -> [Dropout] into dst (unfused: the conv output is stored).
    Returns (raw, stats) for the backward."""
    dev = x.t.device
    raw = new_act(x.N, x.H - 1, x.W - 1, cout, dt, dev)
    stats = ops.zeros_f32((x.N, cout, 2), dev) if normalize else None
    ops.conv_fwd(dt, OP_CONV, x, cin, cout, packed, raw, stats=stats)
    ops.act_fwd(dt, raw, dst, stats=stats, slope=0.2, pool=2, drop_p=drop_p, seed=seed)
    return raw, stats


def up_block_fwd(dt, x, cin, cout, packed, dst, drop_p=0.0, seed=0):
    """ConvTranspose2d(k4,s2,p1,no bias) -> BlurPool(s1) -> InstanceNorm2d -> ReLU -> [Dropout] into dst. Returns (blur, bstats) for the backward."""
    dev = x.t.device
    rawT = new_act(x.N, 2 * x.H, 2 * x.W, cout, dt, dev)
    ops.conv_fwd(dt, OP_CONVT, x, cin, cout, packed, rawT)
    blur = new_act(x.N, 2 * x.H, 2 * x.W, cout, dt, dev)
    bstats = ops.zeros_f32((x.N, cout, 2), dev)
    ops.act_fwd(dt, rawT, blur, stats=None, slope=1.0, pool=1, stats_out=bstats)
    ops.act_fwd(dt, blur, dst, stats=bstats, slope=0.0, pool=0, drop_p=drop_p, seed=seed)
    return blur, bstats


def up_block_act_bwd(dt, g_out, blur, bstats, drop_p=0.0, seed=0):
    """backward of up_block_fwd from the gradient of its output through to the transposed convolution's output. Returns (d_blur, d_rawT)."""
    N, H, W, C = blur.N, blur.H, blur.W, blur.C
    dev = blur.t.device
    d_blur = new_act(N, H, W, C, dt, dev)
    norm_act_bwd(dt, g_out, blur, d_blur, bstats, 0.0, 0, drop_p, seed)
    d_rawT = new_act(N, H, W, C, dt, dev)
    ops.act_bwd(dt, 0, d_blur, None, N, H, W, C, d_rawT, stats=None, slope=1.0, pool=1)
    return d_blur, d_rawT


def first_block_fwd(core, ctx, x, cin, cout, packed, dst, save, bias=None, oscale=None, act_in_conv=False, seed=0):
    """conv [+ bias, x 1/sigma] -> LeakyReLU(0.2) -> BlurPool(s2) of a network's first block (8 padded input channels, no norm, no dropout) into dst,
    one of three ways:
      fused       ops.first_block_fwd: ONE kernel, the 266 MB conv output is never written; returns None for it. Not while core.debug is set.
      sign words  ops.conv_first_fwd stores the conv output and leaves one sign bit per value, all the fused backward reads of it
      plain       the convolution and the pooling pass of any down block (a layer the first-block kernels do not serve, or nothing to save)
    ctx.mask1: the sign words of the first two (None: none written). Returns the stored conv output, or None.
    act_in_conv: LeakyReLU in the convolution's epilogue -- the stored tensor is the ACTIVATED one, and the backward's slope test (y > 0) is the same
    on y = LeakyReLU(z) as on z -- instead of in the pooling pass on the rounded conv output."""
    dt, dev = core.dt, x.t.device
    N, h = x.N, x.H
    signs = ops.first_block_bwd_supported(dt, cin, cout)
    fused = signs and core.debug is None and ops.first_block_fwd_supported()
    ctx.mask1 = torch.empty((N, h - 1, h - 1, 8), dtype=torch.uint8, device=dev) if signs and save else None
    if fused:
        ops.first_block_fwd(dt, x, cin, cout, packed, dst, bias=bias, oscale=oscale, slope=0.2, act_after_rounding=not act_in_conv, sign_mask=ctx.mask1)
        return None
    raw = new_act(N, h - 1, h - 1, cout, dt, dev)
    flags = ops.EP_LEAKY if act_in_conv else 0
    if ctx.mask1 is not None:
        ops.conv_first_fwd(dt, x, cin, cout, packed, raw, bias=bias, oscale=oscale, flags=flags, sign_mask=ctx.mask1)
    else:
        ops.conv_fwd(dt, OP_CONV, x, cin, cout, packed, raw, bias=bias, oscale=oscale, flags=flags)
    ops.act_fwd(dt, raw, dst, stats=None, slope=1.0 if act_in_conv else 0.2, pool=2, seed=seed)
    return raw


def first_block_bwd(core, ctx, g, x, raw, cin, cout, want_d_raw, accumulate=False, bias_sums=None, seed=0):
    """backward of first_block_fwd's block, from the gradient g of its pooled output. Returns (d_raw, wgrad); wgrad(dw) computes the weight gradient
    into dw (for param_grad) and returns the scratch for core._ws.
    Where nothing but the parameter gradients needs the 266 MB gradient of the conv output (want_d_raw False) it is never written: d_raw is None and
    wgrad is ops.first_block_bwd_wgrad (igemm.hip: tfc_act_bwd(mode 0, pool 2) + tfc_conv_wgrad in one kernel, same bits), which also fills
    bias_sums. Otherwise d_raw comes from the sign words (a fused forward stored no conv output: raw None) or from the stored tensor, with the
    per-image sums in bias_sums, and wgrad is the plain convolution weight gradient. core.debug keeps the unfused form."""
    dt = core.dt
    N, Hc = x.N, x.H - 1
    if not want_d_raw and core.debug is None and ops.first_block_bwd_supported(dt, cin, cout) and pooled(Hc) >= 2:
        return None, lambda dw: ops.first_block_bwd_wgrad(dt, x, raw, g, cin, cout, dw, slope=0.2, accumulate=accumulate, ws=core._ws,
                                                          bias_sums=bias_sums, sign_mask=ctx.mask1)
    d_raw = new_act(N, Hc, Hc, cout, dt, x.t.device)
    if raw is None:
        ops.act_bwd_signs(dt, g, ctx.mask1, N, Hc, Hc, cout, d_raw, slope=0.2, rstats=bias_sums)
    else:
        norm_act_bwd(dt, g, raw, d_raw, None, 0.2, 2, seed=seed, bias_sums=bias_sums)
    return d_raw, lambda dw: ops.conv_wgrad(dt, OP_CONV, x, d_raw, cin, cout, dw, accumulate, core._ws)


def patchgan_head_fwd(dt, ctx, cur, weight, save):
    """ZeroPad2d((1, 0, 1, 0)) + Conv2d(512, 1, 4, padding=1, no bias) of both discriminators. Returns (logits View, pitch 8, channel 0; ctx or None)"""
    logits = new_act(ctx.N, cur.H, cur.W, 8, dt, cur.t.device)    # only channel 0 is ever written or read (bce: stride 8; modules: [..., 0])
    ops.patchgan_head_fwd(dt, cur, weight, View(logits.t, 1, 0))
    ctx.p4 = cur
    return View(logits.t, 1, 0), (ctx if save else None)


def patchgan_head_bwd(core, ctx, g_logits, grads, key, packed, accumulate, hook):
    """backward of patchgan_head_fwd: the head's weight gradient (grads[key], where gradients are wanted) as a param_grad, and the gradient of the
    512-channel features it read, which is returned. g_logits: View [N,h,w,8] (channel 0 = gradient, channels 1..7 zero)."""
    dt, p4 = core.dt, ctx.p4
    dev = g_logits.t.device
    gl = View(g_logits.t, 8, 0)
    if grads is not None:
        core._ws = param_grad(dev, lambda: ops.conv_wgrad(dt, OP_PADCONV, p4, gl, 512, 1, grads[key], accumulate, core._ws), hook, (key,))
    g_cur = new_act(ctx.N, p4.H, p4.W, 512, dt, dev)
    ops.conv_dgrad(dt, OP_PADCONV, gl, ctx.N, p4.H, p4.W, 512, 1, packed, g_cur)
    return g_cur


class GeneratorCore:
    def __init__(self, dt=DT_BF16, channels=3, labels=0, mask=False):
        self.dt = dt
        self.channels = channels
        self.labels = int(labels)                                 # 3: fc(labels) is down1's extra input channel (label-conditioned generator)
        self.mask = bool(mask)                                    # the edge mask of img_A is down1's extra input channel (MASK-4 generator); it is data
        if self.labels and self.mask:
            raise ops._lib.TfcError("GeneratorCore: labels= and mask= are two different scripts' fourth input channel (one of them at most)")
        self.in_channels = channels + (1 if (self.labels or self.mask) else 0)
        self.down = [(G_DOWN[0][0], self.in_channels) + G_DOWN[0][2:]] + G_DOWN[1:]
        self.params = None
        self.packed = {}                                          # (block name, "fwd" | "dgrad") -> operand stream
        self._plan = None
        self._ws = None                                           # persistent wgrad scratch (zeroed once, re-zeroed by the kernels)
        self.debug = None                                         # tests: a dict that receives the stored gradients; selects the unfused first block

    # ---- weights ----
    def set_params(self, params):
        """params: dict state_dict-key -> fp32 CUDA tensor in torch layout (may be views into a flat buffer)."""
        self.params = params
        self.packed = {}
        self._plan = None

    def repack(self):
        """re-pack every operand stream (fwd + dgrad) from the current weights: ONE launch over a device-resident plan"""
        if self._plan is None:
            P, entries = self.params, []
            for name, cin, cout, _, _ in self.down:
                entries.append(((name, "fwd"), OP_CONV, 0, P[down_weight_key(name)], cin, cout))
                if name != "down1":
                    entries.append(((name, "dgrad"), OP_CONV, 1, P[down_weight_key(name)], cin, cout))
            for name, cin, cout, _, _ in G_UP:
                for pas, key in ((0, "fwd"), (1, "dgrad")):
                    entries.append(((name, key), OP_CONVT, pas, P[f"{name}.model.0.weight"], cin, cout))
            for pas, key in ((0, "fwd"), (1, "dgrad")):
                entries.append((("final", key), OP_UPCONV, pas, P["final.2.weight"], 128, self.channels))
            self._plan = plan_streams(self.dt, entries, self.packed)
        self._plan.run()

    # ---- forward ----
    def forward(self, x, seed=0, train=True, save=True, labels=None, plane=None, plane_div=None):
        """x: fp32 NCHW [N,3,S,S] (S multiple of 64, >= 128). Returns (fake fp32 NCHW in (-1,1), ctx). down1 runs as ONE kernel (conv + LeakyReLU +
        BlurPool, first_block_fwd): its 266 MB conv output is never written, the backward needs its signs only and gets them as sign words.
        labels: fp32 [N,3] on the device, for a label-conditioned core (its fc plane is written as input channel 3 by the packing kernel).
        plane: fp32 [N,1,S,S] on the device, for a mask core: input channel 3 (plane_div: a device float it is divided by on the way, ops.MaskCtx.M)."""
        ops.require_gpu(x, labels, plane)
        if (labels is not None) != bool(self.labels):
            raise ops._lib.TfcError("GeneratorCore: labels go with a label-conditioned generator (labels=3) and only with it")
        if (plane is not None) != self.mask:
            raise ops._lib.TfcError("GeneratorCore: the mask plane goes with a mask generator (mask=True) and only with it")
        if not self.packed:
            self.repack()
        dt, dev = self.dt, x.device
        N, C, S, S2 = x.shape
        assert C == self.channels and S == S2 and S % 64 == 0 and S >= 128, "GeneratorUNet needs square inputs, S % 64 == 0, S >= 128"
        ctx = _Ctx()
        ctx.N, ctx.S, ctx.seed, ctx.train = N, S, seed, train
        if self.labels:
            if tuple(labels.shape) != (N, self.labels):
                raise ops._lib.TfcError(f"GeneratorCore: labels {tuple(labels.shape)} for a batch of {N} (expected [N, {self.labels}])")
            labels = labels.contiguous().float()
            x8 = ops.pack_nhwc8_labels(dt, x, labels, self.params["fc.weight"], self.params["fc.bias"])
        elif self.mask:
            x8 = ops.pack_nhwc8_plane(dt, x, plane, plane_div)
        else:
            x8 = ops.pack_nhwc8(dt, x)
        ctx.labels = labels
        # concat buffers: cat[k] = (up_k output | skip) at the resolution of the skip
        sizes = [S >> (i + 1) for i in range(6)]                 # pooled sizes of down1..down6: 128,64,32,16,8,4
        cat = {}
        for name, cin, cout, _, skip in G_UP:
            sc = G_DOWN[skip][2]
            cat[name] = new_act(N, sizes[skip], sizes[skip], cout + sc, dt, dev)
        d6 = new_act(N, sizes[5], sizes[5], 512, dt, dev)
        skip_of = {4: "up1", 3: "up2", 2: "up3", 1: "up4", 0: "up5"}
        ctx.x8, ctx.cat, ctx.d6 = x8, cat, d6
        ctx.raw, ctx.stats, ctx.dins = [], [], []
        cur = x8
        for i, (name, cin, cout, normalize, drop) in enumerate(self.down):
            if i < 5:
                up = cat[skip_of[i]]
                dst = up.sub(up.C - cout, cout)                   # the skip window of the concat buffer
            else:
                dst = d6
            if i == 0 and not normalize and drop == 0.0:
                raw, stats = first_block_fwd(self, ctx, cur, cin, cout, self.packed[name, "fwd"], dst, save, seed=seed * 64 + i), None
            else:
                raw, stats = down_block_fwd(dt, cur, cin, cout, self.packed[name, "fwd"], dst, normalize, drop if train else 0.0, seed * 64 + i)
            ctx.raw.append(raw)
            ctx.stats.append(stats)
            ctx.dins.append(cur)
            cur = dst
        ctx.blur, ctx.bstats, ctx.uins = [], [], []
        for j, (name, cin, cout, drop, skip) in enumerate(G_UP):
            blur, bstats = up_block_fwd(dt, cur, cin, cout, self.packed[name, "fwd"], cat[name].sub(0, cout), drop if train else 0.0,
                                        seed * 64 + 16 + j)
            ctx.blur.append(blur)
            ctx.bstats.append(bstats)
            ctx.uins.append(cur)
            cur = View(cat[name].t, cat[name].t.shape[3], 0)
        fake = torch.empty((N, self.channels, S, S), dtype=torch.float32, device=dev)
        if dt == DT_BF16 and self.channels <= 4:                 # phases as columns of one 16-wide MFMA tile, filter in registers
            ops.upconv_head_fwd(dt, cur, self.params["final.2.weight"], self.params["final.2.bias"], fake)
        else:
            ops.conv_fwd(dt, OP_UPCONV, cur, 128, self.channels, self.packed["final", "fwd"], None, bias=self.params["final.2.bias"],
                         out_nchw=fake)
        ctx.u5 = cur
        ctx.fake = fake
        if not save:
            return fake, None
        return fake, ctx

    # ---- backward ----
    def backward(self, ctx, g_fake, grads, hook=None, accumulate=False, need_input_grad=False):
        try:
            return self._backward(ctx, g_fake, grads, hook, accumulate, need_input_grad)
        finally:
            join_side(g_fake.device)                              # the weight gradients may have run on the side stream

    def _backward(self, ctx, g_fake, grads, hook=None, accumulate=False, need_input_grad=False):
        """g_fake: fp32 NCHW gradient of the loss wrt fake. grads: dict key -> fp32 tensor (torch layout) that receives the
        parameter gradients (overwritten, or accumulated when `accumulate`). hook(key) fires when a gradient is final.
        need_input_grad: also return d loss / d x as fp32 NCHW (STN21: fake_A2 = generator2(warped_B), STN:629 -- the warp and the localiser
        train through the generator's input); the PATCH-16 step never asks for it."""
        dt, N = self.dt, ctx.N
        dev = g_fake.device
        ch = self.channels
        want_gx, need_input_grad = need_input_grad, need_input_grad or bool(self.labels)   # fc trains through down1's input gradient (channel 3)
        gb = grads["final.2.bias"]
        if not accumulate:
            gb.zero_()
        dyf = ops.tanh_bwd_pack(dt, g_fake.contiguous().float(), ctx.fake, dbias=gb)
        self._ws = param_grad(dev, lambda: ops.conv_wgrad(dt, OP_UPCONV, ctx.u5, dyf, 128, ch, grads["final.2.weight"], accumulate, self._ws),
                              hook, ("final.2.weight", "final.2.bias"), (dyf,))
        g_cat = new_act(N, ctx.u5.H, ctx.u5.W, ctx.u5.pitch, dt, dev)
        if dt == DT_BF16 and ch <= 8 and ctx.u5.pitch == 128:
            ops.upconv_head_dgrad(dt, dyf, N, ctx.u5.H, ctx.u5.W, self.params["final.2.weight"], g_cat)    # weights-stationary head kernel
        else:
            ops.conv_dgrad(dt, OP_UPCONV, dyf, N, ctx.u5.H, ctx.u5.W, 128, ch, self.packed["final", "dgrad"], g_cat)
        dbg = self.debug
        if dbg is not None:
            dbg["dyf"], dbg["g_u5"] = dyf, ops.View(g_cat.t.clone(), g_cat.C)   # clone: the skip window is accumulated into later
        g_skip = [None] * 6                                       # gradient window of d1..d5 (views), g_d6 separately
        for j in range(4, -1, -1):
            name, cin, cout, drop, skip = G_UP[j]
            uin = ctx.uins[j]
            g_out = g_cat.sub(0, cout)
            g_skip[skip] = g_cat.sub(cout, g_cat.pitch - cout)
            d_blur, d_rawT = up_block_act_bwd(dt, g_out, ctx.blur[j], ctx.bstats[j], drop if ctx.train else 0.0, ctx.seed * 64 + 16 + j)
            key = f"{name}.model.0.weight"
            if dbg is not None:
                dbg[f"{name}.g_out"] = ops.View(g_cat.t.clone(), g_cat.C)       # gradient of the whole concat buffer (up window | skip window)
                dbg[f"{name}.d_blur"], dbg[f"{name}.d_rawT"] = d_blur, d_rawT
            self._ws = param_grad(dev, lambda: ops.conv_wgrad(dt, OP_CONVT, uin, d_rawT, cin, cout, grads[key], accumulate, self._ws),
                                  hook, (key,), (d_rawT,))
            g_in = new_act(N, uin.H, uin.W, uin.pitch, dt, dev)
            ops.conv_dgrad(dt, OP_CONVT, d_rawT, N, uin.H, uin.W, cin, cout, self.packed[name, "dgrad"], g_in)
            if dbg is not None:
                dbg[f"{name}.g_in"] = ops.View(g_in.t.clone(), g_in.C)          # before the down path accumulates into its skip window
            g_cat = g_in                                          # gradient of the next concat buffer (or of d6 when j == 0)
        g_cur = g_cat                                             # = gradient of d6
        for i in range(5, -1, -1):
            name, cin, cout, normalize, drop = self.down[i]
            raw, din = ctx.raw[i], ctx.dins[i]
            key = down_weight_key(name)
            if i == 0 and not normalize and drop == 0.0:
                d_raw, wgrad = first_block_bwd(self, ctx, g_cur, din, raw, cin, cout, need_input_grad, accumulate, seed=ctx.seed * 64 + i)
            else:
                d_raw = new_act(N, din.H - 1, din.H - 1, cout, dt, dev)
                norm_act_bwd(dt, g_cur, raw, d_raw, ctx.stats[i], 0.2, 2, drop if ctx.train else 0.0, ctx.seed * 64 + i)
                def wgrad(dw):
                    return ops.conv_wgrad(dt, OP_CONV, din, d_raw, cin, cout, dw, accumulate, self._ws)
            if dbg is not None:
                dbg[f"{name}.g_out"] = ops.View(g_cur.t[..., g_cur.coff:g_cur.coff + g_cur.C].clone(), g_cur.C)   # incl. the accumulated skip part
                dbg[f"{name}.d_raw"] = d_raw
            self._ws = param_grad(dev, lambda: wgrad(grads[key]), hook, (key,), (g_cur if d_raw is None else d_raw,))
            if i > 0:
                tgt = g_skip[i - 1]                               # window of d_{i} gradient already holding the skip-path part
                ops.conv_dgrad(dt, OP_CONV, d_raw, N, din.H, din.W, cin, cout, self.packed[name, "dgrad"], tgt, accumulate=True)
                g_cur = tgt
            elif need_input_grad:
                w1 = self.params[key]
                if dt == DT_BF16 and cout == 64 and cin <= 4:
                    gx = ops.conv_dgrad_image(dt, d_raw, N, din.H, din.W, cin, w1, None, cin)   # rows-packed kernel, fp32 NCHW out
                else:
                    gx8 = new_act(N, din.H, din.W, din.pitch, dt, dev)
                    ops.conv_dgrad(dt, OP_CONV, d_raw, N, din.H, din.W, cin, cout, ops.pack_weight(dt, OP_CONV, 1, w1.contiguous(), cin, cout), gx8)
                    gx = ops.unpack_nchw(dt, gx8, cin, c0=0)
                if not self.labels:
                    return gx
                # channel 3 is the gradient of the label plane: d fc.weight / d fc.bias, the last gradients of the generator
                param_grad(dev, lambda: ops.label_plane_bwd(gx, ctx.labels, grads["fc.weight"], grads["fc.bias"], ch=ch, accumulate=accumulate),
                           hook, G_FC, (gx,))
                return gx[:, :ch].contiguous() if want_gx else None
        return None


class DiscriminatorCore:
    def __init__(self, dt=DT_BF16, channels=3, aux_classes=None):
        self.dt = dt
        self.channels = channels
        self.aux_classes = tuple(aux_classes) if aux_classes else None      # (2, 4, 3): the three auxiliary classifier heads on the raw input
        self.params = None
        self.buffers = None
        self.head_packed = {}
        self._plan = None
        self._ws = None                                           # persistent wgrad scratch (zeroed once, re-zeroed by the kernels)
        self._sn_ws = None
        self.debug = None                                         # tests: a dict that receives the stored gradients; selects the unfused first block

    def set_params(self, params, buffers):
        """params: dict key -> fp32 tensor ('model.{0,3,6,9}.bias', '...parametrizations.weight.original', 'model.13.weight');
        buffers: dict 'model.{i}.parametrizations.weight.0._u' / '._v' -> fp32 tensors (updated in place)."""
        self.params, self.buffers = params, buffers
        self.head_packed = {}
        self._plan = None

    def repack(self):
        """operand streams of the UN-normalised weights, once per weight update (one launch); 1/sigma is applied in the GEMM epilogue"""
        if self._plan is None:
            w = self.params["model.13.weight"]
            entries = [("fwd", OP_PADCONV, 0, w, 512, 1), ("dgrad", OP_PADCONV, 1, w, 512, 1)]
            for i, cin, cout in D_BLOCKS:
                W = self.params[f"model.{i}.parametrizations.weight.original"]
                entries += [(f"f{i}", OP_CONV, 0, W, cin, cout), (f"d{i}", OP_CONV, 1, W, cin, cout)]
            self._plan = plan_streams(self.dt, entries, self.head_packed)
        self._plan.run()

    def forward(self, img_a, img_b, power_iter=True, save=True, after_sn=None):
        """img_a, img_b: fp32 NCHW [N,3,S,S]. Returns (logits View [N,S/16,S/16,pitch 8] channel 0, ctx).
        = sn_snapshot() + chain(). after_sn: called once the power iteration of this call is queued -- everything after it reads only this call's
        snapshots of u, v, sigma, so a second forward may start from there on another stream (forward_pair)."""
        ops.require_gpu(img_a, img_b)
        snapshot = self.sn_snapshot(img_a.device, power_iter, save)
        if after_sn is not None:
            after_sn()
        return self.chain(img_a, img_b, snapshot, save)

    def sn_snapshot(self, dev, power_iter=True, save=True):
        """one power iteration of the four spectrally normalised blocks (u, v updated in place as the reference's training-mode forward does) and this
        call's snapshots (u, v, [sigma, 1/sigma]) -- all a forward / backward pass of this call reads afterwards. Depends on the weights only, so the
        generator step takes both of its calls' snapshots up front, in order, and runs the second call's chain beside the generator."""
        if not self.head_packed:
            self.repack()
        # spectral norm of all four blocks in one batched power iteration; per-call snapshots of u, v, sigma for the backward
        Ws = [self.params[f"model.{i}.parametrizations.weight.original"] for i, _, _ in D_BLOCKS]
        us = [self.buffers[f"model.{i}.parametrizations.weight.0._u"] for i, _, _ in D_BLOCKS]
        vs = [self.buffers[f"model.{i}.parametrizations.weight.0._v"] for i, _, _ in D_BLOCKS]
        nu, nv = [u.numel() for u in us], [v.numel() for v in vs]
        snap = torch.empty(sum(nu) + sum(nv) + 2 * len(Ws), dtype=torch.float32, device=dev)
        offs, o = [], 0
        for a in nu + nv + [2] * len(Ws):
            offs.append(o)
            o += a
        L = len(Ws)
        usn = [snap[offs[k]:offs[k] + nu[k]] for k in range(L)]
        vsn = [snap[offs[L + k]:offs[L + k] + nv[k]] for k in range(L)]
        sig = [snap[offs[2 * L + k]:offs[2 * L + k] + 2] for k in range(L)]
        self._sn_ws = ops.spectral_norm_step_batched(Ws, us, vs, sig, power_iter=power_iter, u_snaps=usn if save else None,
                                                     v_snaps=vsn if save else None, ws=self._sn_ws)
        return usn, vsn, sig

    def chain(self, img_a, img_b, snapshot, save=True):
        """the convolution chain of one call, given its sn_snapshot(). Block 1 runs as one kernel (first_block_fwd) that keeps sign words
        instead of its 266 MB conv output (all any backward reads of it)."""
        usn, vsn, sig = snapshot
        dt, dev = self.dt, img_a.device
        N, C, S, _ = img_a.shape
        ctx = _Ctx()
        ctx.N, ctx.S = N, S
        x8 = ops.pack_nhwc8(dt, img_a, img_b)
        ctx.ins, ctx.raw, ctx.sn = [], [], []
        cur = x8
        for bi, (i, cin, cout) in enumerate(D_BLOCKS):
            sigma2 = sig[bi]
            h = cur.H
            bias, packed = self.params[f"model.{i}.bias"], self.head_packed[f"f{i}"]
            out = new_act(N, pooled(h - 1), pooled(h - 1), cout, dt, dev)
            # SN-conv + bias + LeakyReLU(0.2) in one kernel (P16:188-190): `raw` holds the ACTIVATED tensor, the pooling pass only blurs
            if bi == 0:
                raw = first_block_fwd(self, ctx, cur, cin, cout, packed, out, save, bias=bias, oscale=sigma2[1:], act_in_conv=True)
            else:
                raw = new_act(N, h - 1, h - 1, cout, dt, dev)
                ops.conv_fwd(dt, OP_CONV, cur, cin, cout, packed, raw, bias=bias, oscale=sigma2[1:], flags=ops.EP_LEAKY)
                ops.act_fwd(dt, raw, out, stats=None, slope=1.0, pool=2)
            ctx.ins.append(cur)
            ctx.raw.append(raw)
            ctx.sn.append((usn[bi], vsn[bi], sigma2) if save else None)
            cur = out
        return patchgan_head_fwd(dt, ctx, cur, self.params["model.13.weight"], save)

    # ---- auxiliary classifier heads (label-conditioned discriminator): three Linear on the flattened 6 x S x S input ----
    def aux_params(self, src=None):
        src = self.params if src is None else src
        return [src[f"{n}.0.weight"] for n, _ in D_AUX], [src[f"{n}.0.bias"] for n, _ in D_AUX]

    def heads(self, x8):
        """x8: the packed input of a call (ctx.ins[0] of chain()). Returns the heads' logits [N, sum classes] fp32 (the Softmax of the modules and the
        reference's cross entropy on top of it live in ops.softmax_ce_heads)."""
        if not self.aux_classes:
            raise ops._lib.TfcError("DiscriminatorCore.heads: this discriminator has no auxiliary heads (aux_classes=None)")
        ws, bs = self.aux_params()
        return ops.aux_heads_fwd(self.dt, x8, ws, bs, self.aux_classes)

    def heads_input_grad(self, g_img, dlogits):
        """g_img (fp32 NCHW gradient of img_A, in place) += the heads' share"""
        return ops.aux_heads_dgrad(g_img, self.aux_params()[0], dlogits, self.aux_classes)

    def heads_wgrad(self, x_r, dl_r, x_f, dl_f, grads, accumulate=False, hook=None):
        """gradients of the six head parameters from the real pair and the fake pair, straight into the torch-layout views `grads`"""
        dws, dbs = self.aux_params(grads)
        param_grad(x_r.t.device, lambda: ops.aux_heads_wgrad(self.dt, x_r, dl_r, x_f, dl_f, dws, dbs, accumulate, self.aux_classes),
                   hook, d_aux_names(), (dl_r, dl_f))

    def forward_pair(self, a1, b1, a2, b2, power_iter=True, save=True):
        """forward(a1, b1) then forward(a2, b2), same results as the two calls in that order (the second power iteration follows the first). With the
        side stream on, the second call's convolution chain runs beside the first's: two independent chains of MFMA-bound GEMMs and HBM-bound
        blur-pools that fill each other's gaps."""
        if not side_stream_on() or os.environ.get("TFC_NO_FWD_PAIR", "0") not in ("", "0"):    # (A/B knob)
            return self.forward(a1, b1, power_iter, save), self.forward(a2, b2, power_iter, save)
        dev = a1.device
        if not self.head_packed:
            self.repack()
        box = {}

        def second():
            box["r"] = on_side(dev, lambda: self.forward(a2, b2, power_iter, save))
        first = self.forward(a1, b1, power_iter, save, after_sn=second)
        join_side(dev)
        return first, box["r"]

    def backward(self, ctx, g_logits, grads=None, need_input_grad=True, accumulate=False, hook=None, ws=None):
        try:
            return self._backward(ctx, g_logits, grads, need_input_grad, accumulate, hook, ws)
        finally:
            join_side(g_logits.t.device)                          # the weight gradients may have run on the side stream

    def _backward(self, ctx, g_logits, grads=None, need_input_grad=True, accumulate=False, hook=None, ws=None):
        """g_logits: View [N,h,w,8] (channel 0 = gradient, channels 1..7 zero). grads: dict key -> fp32 tensor or None
        (skip all weight gradients: generator step). Returns fp32 NCHW gradient of img_a (first argument) or None."""
        dt, N = self.dt, ctx.N
        dev = g_logits.t.device
        if ws is not None:
            self._ws = ws
        g_cur = patchgan_head_bwd(self, ctx, g_logits, grads, "model.13.weight", self.head_packed["dgrad"], accumulate, hook)
        for bi in range(3, -1, -1):
            i, cin, cout = D_BLOCKS[bi]
            raw, xin = ctx.raw[bi], ctx.ins[bi]
            u, v, sigma2 = ctx.sn[bi]
            wkey, bkey = f"model.{i}.parametrizations.weight.original", f"model.{i}.bias"
            W = self.params[wkey]
            gb_img = ops.zeros_f32((N, cout), dev) if grads is not None else None      # per-image bias gradient, from the activation backward
            if bi == 0:
                # discriminator step: block 1's conv-output gradient (266 MB) feeds only its weight / bias gradients -> never written
                d_raw, wgrad = first_block_bwd(self, ctx, g_cur, xin, raw, cin, cout, grads is None or need_input_grad, bias_sums=gb_img)
            else:
                d_raw = new_act(N, xin.H - 1, xin.H - 1, cout, dt, dev)
                norm_act_bwd(dt, g_cur, raw, d_raw, None, 0.2, 2, bias_sums=gb_img)
                def wgrad(dw):
                    return ops.conv_wgrad(dt, OP_CONV, xin, d_raw, cin, cout, dw, False, self._ws)
            if self.debug is not None:
                self.debug[f"b{bi}.g_out"], self.debug[f"b{bi}.d_raw"] = g_cur, d_raw
            if grads is not None:
                def sn_grads():
                    gsn = torch.empty_like(W)                     # gradient of the normalised weight; spectral_norm_bwd takes it to W's
                    if d_raw is None:                             # the fused kernel writes the bias sums itself: ahead of their column sum
                        self._ws = wgrad(gsn)
                    bias_grad(gb_img, grads[bkey], accumulate)
                    if d_raw is not None:
                        self._ws = wgrad(gsn)
                    ops.spectral_norm_bwd(gsn, W, u, v, sigma2, grads[wkey], accumulate)
                param_grad(dev, sn_grads, hook, (wkey, bkey), (g_cur if d_raw is None else d_raw, gb_img))
            if bi == 0 and need_input_grad and dt == DT_BF16 and self.channels <= 4 and cout == 64:
                # gradient w.r.t. the generated image only (3 of the 6 input channels): rows-packed 16-wide MFMA kernel, fp32 NCHW out
                return ops.conv_dgrad_image(dt, d_raw, N, xin.H, xin.W, cin, W, sigma2[1:], self.channels)
            if bi > 0 or need_input_grad:
                g_in = new_act(N, xin.H, xin.W, xin.pitch, dt, dev)
                ops.conv_dgrad(dt, OP_CONV, d_raw, N, xin.H, xin.W, cin, cout, self.head_packed[f"d{i}"], g_in, oscale=sigma2[1:])
                g_cur = g_in
        if need_input_grad:
            return ops.unpack_nchw(dt, g_cur, self.channels, c0=0)
        return None


class Pix2PixCore:
    """The plain pix2pix PatchGAN (no spectral norm, no BlurPool): four blocks Conv2d(k4, s2, p1, bias) -> [InstanceNorm2d] -> LeakyReLU(0.2), then
    ZeroPad2d((1, 0, 1, 0)) + Conv2d(512, 1, 4, padding=1, no bias). Block 1 is one TFC_OP_CONV2 launch with bias and LeakyReLU in its epilogue; blocks
    2-4 are TFC_OP_CONV2 with bias and the InstanceNorm statistics in the epilogue, then the fused normalise + activate pass; the head is the PatchGAN
    head kernel of DiscriminatorCore.

    A bias in front of InstanceNorm cannot change the output, so its gradient is mathematically zero (torch leaves rounding noise there, ~1e-6 of the
    weight gradient's size): backward() writes exact zeros for the biases of blocks 2-4."""

    def __init__(self, dt=DT_BF16, channels=3):
        self.dt = dt
        self.channels = channels
        self.params = None
        self.packed = {}
        self._plan = None
        self._ws = None                                           # persistent wgrad scratch (zeroed once, re-zeroed by the kernels)
        self.debug = None                                         # tests: a dict that receives the stored gradients of every block

    def blocks(self):
        cin = 2 * self.channels
        for i, cout, norm in P2P_BLOCKS:
            yield i, cin, cout, norm
            cin = cout

    def set_params(self, params):
        """params: dict key -> fp32 tensor: 'model.{0,2,5,8}.weight' / '.bias', 'model.12.weight'"""
        self.params = params
        self.packed = {}
        self._plan = None

    def repack(self):
        """operand streams of the nine convolution passes, once per weight update (one launch)"""
        if self._plan is None:
            entries = [("dhead", OP_PADCONV, 1, self.params[f"model.{P2P_HEAD}.weight"], 512, 1)]
            for i, cin, cout, _ in self.blocks():
                W = self.params[f"model.{i}.weight"]
                entries += [(f"f{i}", OP_CONV2, 0, W, cin, cout), (f"d{i}", OP_CONV2, 1, W, cin, cout)]
            self._plan = plan_streams(self.dt, entries, self.packed)
        self._plan.run()

    def forward(self, img_a, img_b, save=True):
        """img_a, img_b: fp32 NCHW [N, channels, H, W], H and W multiples of 16. Returns (logits View [N, H/16, W/16, pitch 8] channel 0, ctx)."""
        ops.require_gpu(img_a, img_b)
        dt, dev = self.dt, img_a.device
        N, _, H, W = img_a.shape
        if H % 16 or W % 16:
            raise ops._lib.TfcError(f"Pix2PixDiscriminator: the four stride-2 blocks need H and W in multiples of 16 (got {H} x {W})")
        if not self.packed:
            self.repack()
        ctx = _Ctx()
        ctx.N = N
        ctx.ins, ctx.raw, ctx.stats = [], [], []
        cur = ops.pack_nhwc8(dt, img_a, img_b)
        for i, cin, cout, norm in self.blocks():
            h, w = cur.H // 2, cur.W // 2
            bias = self.params[f"model.{i}.bias"]
            if norm:
                raw = new_act(N, h, w, cout, dt, dev)
                st = ops.zeros_f32((N, cout, 2), dev)
                ops.conv_fwd(dt, OP_CONV2, cur, cin, cout, self.packed[f"f{i}"], raw, bias=bias, stats=st)
                out = new_act(N, h, w, cout, dt, dev)
                ops.act_fwd(dt, raw, out, stats=st, slope=0.2, pool=0)
            else:
                # `raw` holds the ACTIVATED tensor: the backward's slope test (y > 0) is the same on LeakyReLU(z) as on z
                raw, st = new_act(N, h, w, cout, dt, dev), None
                ops.conv_fwd(dt, OP_CONV2, cur, cin, cout, self.packed[f"f{i}"], raw, bias=bias, flags=ops.EP_LEAKY)
                out = raw
            ctx.ins.append(cur)
            ctx.raw.append(raw)
            ctx.stats.append(st)
            cur = out
        return patchgan_head_fwd(dt, ctx, cur, self.params[f"model.{P2P_HEAD}.weight"], save)

    def backward(self, ctx, g_logits, grads=None, need_input_grad=True, accumulate=False, hook=None):
        try:
            return self._backward(ctx, g_logits, grads, need_input_grad, accumulate, hook)
        finally:
            join_side(g_logits.t.device)                          # the weight gradients may have run on the side stream

    def _backward(self, ctx, g_logits, grads, need_input_grad, accumulate, hook):
        """g_logits: View [N, h, w, 8] (channel 0 = gradient, channels 1..7 zero). grads: dict key -> fp32 tensor, or None (no parameter gradients: the
        generator step). Returns the fp32 NCHW gradient of img_a, or None."""
        dt, N = self.dt, ctx.N
        dev = g_logits.t.device
        g_cur = patchgan_head_bwd(self, ctx, g_logits, grads, f"model.{P2P_HEAD}.weight", self.packed["dhead"], accumulate, hook)
        blocks = list(self.blocks())
        for bi in range(len(blocks) - 1, -1, -1):
            i, cin, cout, norm = blocks[bi]
            xin, raw = ctx.ins[bi], ctx.raw[bi]
            wkey, bkey = f"model.{i}.weight", f"model.{i}.bias"
            d_raw = new_act(N, raw.H, raw.W, cout, dt, dev)
            # block 1: the per-image bias gradient rides on the activation backward; behind InstanceNorm the bias gradient is exactly zero
            gb_img = ops.zeros_f32((N, cout), dev) if grads is not None and not norm else None
            norm_act_bwd(dt, g_cur, raw, d_raw, ctx.stats[bi], 0.2, 0, bias_sums=gb_img)
            if self.debug is not None:
                self.debug[f"b{bi}.g_out"], self.debug[f"b{bi}.d_raw"] = g_cur, d_raw
            if grads is not None:
                def block_grads():
                    bias_grad(gb_img, grads[bkey], accumulate)
                    self._ws = ops.conv_wgrad(dt, OP_CONV2, xin, d_raw, cin, cout, grads[wkey], accumulate, self._ws)
                param_grad(dev, block_grads, hook, (wkey, bkey), (d_raw, gb_img))
            if bi > 0 or need_input_grad:
                g_in = new_act(N, xin.H, xin.W, xin.pitch, dt, dev)
                ops.conv_dgrad(dt, OP_CONV2, d_raw, N, xin.H, xin.W, cin, cout, self.packed[f"d{i}"], g_in)
                g_cur = g_in
        if need_input_grad:
            return ops.unpack_nchw(dt, g_cur, self.channels, c0=0)
        return None


# ---- the residual trunk of CycleGAN's GeneratorResNet (cyclegan_og/models.py:29-46, :79-80) -----------------------------------------------------
RES_CONVS = (1, 5)                      # indices of the two convolutions inside a block's nn.Sequential


def res_block_keys(prefix):
    """state_dict keys of one residual block in forward order: (weight, bias) of block.1, then of block.5"""
    return [f"{prefix}block.{i}.{s}" for i in RES_CONVS for s in ("weight", "bias")]


def res_prefixes(n_blocks, first=0, stem=""):
    """key prefixes of n_blocks consecutive blocks: GeneratorResNet holds them as model.{10 + b}."""
    return [f"{stem}{first + b}." for b in range(n_blocks)]


class ResNetTrunkCore:
    """n_blocks x [ReflectionPad2d(1) -> Conv2d(C, C, 3) -> InstanceNorm2d -> ReLU -> ReflectionPad2d(1) -> Conv2d(C, C, 3) -> InstanceNorm2d, + x] on
    NHWC Views. Per block: TFC_OP_CONV3R with bias and the InstanceNorm statistics in its epilogue, the fused normalise + ReLU pass, TFC_OP_CONV3R
    again, and tfc_norm_add_fwd (normalise + skip in one pass). The backward mirrors it; the input gradient of a block's first convolution is
    ACCUMULATED onto the skip gradient in place (the fold pass of the convolution's input gradient honours TFC_EP_ACCUM).

    The state_dict holds 3 x 3 filters and the convolution op takes [C][C][4][4] slots: the core keeps one zero-padded copy of all its filters
    (refreshed by repack(), ahead of the one packing launch) and one 4 x 4 staging slot for the weight gradients.
    prefixes: the key prefix of every block (default "0.", "1.", ...); a block's keys are prefix + block.{1,5}.{weight,bias}."""

    def __init__(self, dt, features, n_blocks, prefixes=None):
        self.dt = dt
        self.features = int(features)
        self.n_blocks = int(n_blocks)
        self.prefixes = list(prefixes) if prefixes is not None else res_prefixes(self.n_blocks)
        assert len(self.prefixes) == self.n_blocks
        unit = 32 if dt == DT_BF16 else 16
        if self.features % unit:
            raise ops._lib.TfcError(f"ResNetTrunkCore: {self.features} features; the reflect-padded 3x3 convolution needs channel bytes in multiples of 64 "
                                    f"(a multiple of {unit} channels in this compute mode)")
        self.params = None
        self.packed = {}                                          # (block, conv, "fwd" | "dgrad") -> operand stream
        self._plan = None
        self._w4 = None                                           # [2 * n_blocks, C, C, 4, 4]: the filters in the op's 4 x 4 slots
        self._g4 = None                                           # [C, C, 4, 4]: staging slot of a weight gradient
        self._ws = None                                           # persistent wgrad scratch (zeroed once, re-zeroed by the kernels)
        self.debug = None                                         # tests: a dict that receives the stored gradients of every block

    def param_names(self):
        return [k for p in self.prefixes for k in res_block_keys(p)]

    def backward_order(self):
        """parameter names in the order their gradients become final during backward"""
        out = []
        for p in reversed(self.prefixes):
            w1, b1, w2, b2 = res_block_keys(p)
            out += [w2, b2, w1, b1]
        return out

    def set_params(self, params):
        """params: dict key -> fp32 CUDA tensor: weights [C, C, 3, 3] and biases [C] under param_names()"""
        self.params = params
        self.packed = {}
        self._plan = None

    def _weights(self):
        return [self.params[f"{p}block.{i}.weight"] for p in self.prefixes for i in RES_CONVS]

    def repack(self):
        """refresh the 4 x 4 copies of the filters, then re-pack every operand stream (fwd + dgrad): ONE packing launch over a device-resident plan"""
        C = self.features
        ws = self._weights()
        if self._plan is None:
            for w in ws:
                if tuple(w.shape) != (C, C, 3, 3):
                    raise ops._lib.TfcError(f"ResNetTrunkCore: a filter of shape {tuple(w.shape)} (expected {(C, C, 3, 3)})")
            self._w4 = torch.zeros((len(ws), C, C, 4, 4), dtype=torch.float32, device=ws[0].device)
            entries = []
            for b in range(self.n_blocks):
                for c in range(2):
                    w4 = self._w4[2 * b + c]
                    entries += [((b, c, "fwd"), OP_CONV3R, 0, w4, C, C), ((b, c, "dgrad"), OP_CONV3R, 1, w4, C, C)]
            self._plan = plan_streams(self.dt, entries, self.packed)
        self._w4[..., :3, :3].copy_(torch.stack([w.detach() for w in ws]))
        self._plan.run()

    # ---- forward ----
    def forward(self, x: View, save=True):
        """x: NHWC View of `features` channels in the compute dtype (H, W >= 2). Returns (output View, ctx or None)."""
        ops.require_gpu(x.t)
        if x.C != self.features:
            raise ops._lib.TfcError(f"ResNetTrunkCore: input of {x.C} channels for a trunk of {self.features}")
        if not self.packed:
            self.repack()
        dt, dev, C = self.dt, x.t.device, self.features
        N, H, W = x.N, x.H, x.W
        ctx = _Ctx()
        ctx.N, ctx.H, ctx.W = N, H, W
        ctx.blocks = []
        cur = x
        for b, p in enumerate(self.prefixes):
            _, b1, _, b2 = res_block_keys(p)
            raw1, st1 = new_act(N, H, W, C, dt, dev), ops.zeros_f32((N, C, 2), dev)
            ops.conv_fwd(dt, OP_CONV3R, cur, C, C, self.packed[b, 0, "fwd"], raw1, bias=self.params[b1], stats=st1)
            a1 = new_act(N, H, W, C, dt, dev)
            ops.act_fwd(dt, raw1, a1, stats=st1, slope=0.0, pool=0)
            raw2, st2 = new_act(N, H, W, C, dt, dev), ops.zeros_f32((N, C, 2), dev)
            ops.conv_fwd(dt, OP_CONV3R, a1, C, C, self.packed[b, 1, "fwd"], raw2, bias=self.params[b2], stats=st2)
            out = new_act(N, H, W, C, dt, dev)
            ops.norm_add_fwd(dt, raw2, cur, st2, out)
            if save:
                ctx.blocks.append((cur, raw1, st1, a1, raw2, st2))
            cur = out
        if self.debug is not None:
            self.debug["ctx"] = ctx                               # the stored tensors and statistics of every block, for the per-stage tests
        return cur, (ctx if save else None)

    # ---- backward ----
    def backward(self, ctx, g: View, grads, hook=None, accumulate=False):
        try:
            return self._backward(ctx, g, grads, hook, accumulate)
        finally:
            join_side(g.t.device)                                 # the parameter gradients may have run on the side stream

    def _conv_grads(self, x, d_raw, wkey, bkey, grads, accumulate, hook):
        """weight and bias gradient of one convolution on the side stream: the weight gradient through the 4 x 4 staging slot into the 3 x 3 tensor,
        the bias gradient as the per-channel sums of the gradient that enters the convolution"""
        dt, C = self.dt, self.features
        dev = d_raw.t.device

        def work():
            if self._g4 is None:
                self._g4 = torch.zeros((C, C, 4, 4), dtype=torch.float32, device=dev)
            self._ws = ops.conv_wgrad(dt, OP_CONV3R, x, d_raw, C, C, self._g4, False, self._ws)
            if accumulate:
                grads[wkey].add_(self._g4[..., :3, :3])
            else:
                grads[wkey].copy_(self._g4[..., :3, :3])
                grads[bkey].zero_()
            ops.colsum(dt, d_raw, grads[bkey])
        param_grad(dev, work, hook, (wkey, bkey), (d_raw,))

    def _backward(self, ctx, g, grads, hook, accumulate):
        """g: NHWC View, the gradient of the trunk's output; it is UPDATED IN PLACE block by block and returned as the gradient of the trunk's input.
        grads: dict key -> fp32 tensor (3 x 3 filters, biases) that receives the parameter gradients (overwritten, or accumulated when `accumulate`),
        or None (input gradient only). hook(key) fires when a gradient is final."""
        dt, C = self.dt, self.features
        N, H, W = ctx.N, ctx.H, ctx.W
        dev = g.t.device
        dbg = self.debug
        for b in range(self.n_blocks - 1, -1, -1):
            x, raw1, st1, a1, raw2, st2 = ctx.blocks[b]
            w1, b1, w2, b2 = res_block_keys(self.prefixes[b])
            if dbg is not None:
                dbg[f"{b}.g_out"] = View(g.t.clone(), g.C)
            # the skip's gradient is g itself; through the second InstanceNorm (no activation: slope 1)
            d_raw2 = new_act(N, H, W, C, dt, dev)
            norm_act_bwd(dt, g, raw2, d_raw2, st2, 1.0, 0)
            if grads is not None:
                self._conv_grads(a1, d_raw2, w2, b2, grads, accumulate, hook)
            d_a1 = new_act(N, H, W, C, dt, dev)
            ops.conv_dgrad(dt, OP_CONV3R, d_raw2, N, H, W, C, C, self.packed[b, 1, "dgrad"], d_a1)
            d_raw1 = new_act(N, H, W, C, dt, dev)
            norm_act_bwd(dt, d_a1, raw1, d_raw1, st1, 0.0, 0)
            if grads is not None:
                self._conv_grads(x, d_raw1, w1, b1, grads, accumulate, hook)
            ops.conv_dgrad(dt, OP_CONV3R, d_raw1, N, H, W, C, C, self.packed[b, 0, "dgrad"], g, accumulate=True)   # onto the skip gradient
            if dbg is not None:
                dbg[f"{b}.d_raw2"], dbg[f"{b}.d_a1"], dbg[f"{b}.d_raw1"] = d_raw2, d_a1, d_raw1
                dbg[f"{b}.g_in"] = View(g.t.clone(), g.C)
        return g
