"""Restatement of CycleGAN's ResidualBlock / GeneratorResNet (cyclegan_og/models.py:29-102) in plain torch.nn.functional, written from the module
definitions, in the precision of its input (the tests use float64).

  x -> ReflectionPad2d(1) -> Conv2d(C, C, 3) -> InstanceNorm2d -> ReLU -> ReflectionPad2d(1) -> Conv2d(C, C, 3) -> InstanceNorm2d, + x

`store="bf16"` models the engine's bf16 storage: values AND their gradients are rounded to bf16 where the engine stores a tensor (after each
convolution, after the activation, after the add), the filters are rounded where they are packed (their gradients stay fp32), and the gradient of a
reflect-PADDED input is rounded before the padding's adjoint folds it (the fold pass reads that tensor from bf16 scratch). `stats` hands over the
engine's InstanceNorm statistics (conv_exact.EngineStatsNorm: the constants in fp32 as the kernels derive them), `force` the engine's stored tensors:
the computation continues from them (teacher forcing), so each stage is compared on its own and a ReLU mask is decided by identical numbers.

`store="bf16x3"` models the third compute mode (include/tfc_gan.h, TFC_DT_BF16X3): storage is fp32, and each of the three convolution passes splits
both of ITS operands a into hi = bf16(a), lo = bf16(a - hi) and adds hi*hi + hi*lo + lo*hi -- the lo*lo term, up to 2^-16 |a b| per product, is
dropped. The forward splits (x, w), the input gradient (dy, w), the weight gradient (x, dy): three different roundings, so the convolution is a
torch.autograd.Function with that backward and not the autograd adjoint of its forward.
"""
import torch
import torch.nn.functional as F

from tests.conv_exact import EngineStatsNorm

EPS = 1e-5


def _bf(x):
    return x.to(torch.bfloat16).to(x.dtype)


class _RoundBoth(torch.autograd.Function):                       # a stored activation: the value and its gradient are bf16 tensors
    @staticmethod
    def forward(ctx, x):
        return _bf(x)

    @staticmethod
    def backward(ctx, g):
        return _bf(g)


class _RoundFwd(torch.autograd.Function):                        # a bf16 operand whose gradient stays fp32 (the packed filters)
    @staticmethod
    def forward(ctx, x):
        return _bf(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundBwd(torch.autograd.Function):                        # a value that is never stored, whose gradient is (the padded gradient in scratch)
    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return _bf(g)


def _ident(x):
    return x


def _split(a):
    hi = _bf(a)
    return hi, _bf(a - hi)


def _three(f, a, b):
    """f bilinear in (a, b): f(hi, hi) + f(hi, lo) + f(lo, hi) of the split operands"""
    (ah, al), (bh, bl) = _split(a), _split(b)
    return f(ah, bh) + f(ah, bl) + f(al, bh)


class _ConvX3(torch.autograd.Function):                          # valid 3 x 3 convolution of an already padded input, every pass as bf16x3 computes it
    @staticmethod
    def forward(ctx, xp, w, b):
        ctx.save_for_backward(xp, w)
        return _three(F.conv2d, xp, w) + b.view(1, -1, 1, 1)

    @staticmethod
    def backward(ctx, g):
        xp, w = ctx.saved_tensors
        gx = _three(lambda gg, ww: torch.nn.grad.conv2d_input(xp.shape, ww, gg), g, w)
        gw = _three(lambda xx, gg: torch.nn.grad.conv2d_weight(xx, w.shape, gg), xp, g)
        return gx, gw, g.sum((0, 2, 3))


def rounders(store):
    """(stored activation, packed filter, scratch gradient) rounding of a storage model: None -> identities, "bf16" -> the three above"""
    if store in (None, "bf16x3"):                                 # bf16x3 stores fp32: what it rounds is inside its convolutions (conv3r)
        return _ident, _ident, _ident
    assert store == "bf16"
    return _RoundBoth.apply, _RoundFwd.apply, _RoundBwd.apply


def instance_norm(x, stats=None):
    """nn.InstanceNorm2d (biased variance, eps 1e-5, no affine), or the same at the engine's statistics [N, C, 2]"""
    if stats is not None:
        return EngineStatsNorm.apply(x, stats, EPS)
    m = x.mean(dim=(2, 3), keepdim=True)
    v = ((x - m) ** 2).mean(dim=(2, 3), keepdim=True)
    return (x - m) / torch.sqrt(v + EPS)


def conv3r(x, w, b, rw=_ident, rg=_ident, x3=False):
    """nn.ReflectionPad2d(1) + nn.Conv2d(C, C', 3); x3: the three passes of the convolution as the bf16x3 mode computes them"""
    xp = rg(F.pad(x, (1, 1, 1, 1), mode="reflect"))
    return _ConvX3.apply(xp, w, b) if x3 else F.conv2d(xp, rw(w), b)


class _ForceGrad(torch.autograd.Function):                       # identity; backward: files the arriving gradient under `key`, passes the engine's on
    @staticmethod
    def forward(ctx, z, g_engine, seen, key):
        ctx.g_engine, ctx.seen, ctx.key = g_engine, seen, key
        return z.clone()

    @staticmethod
    def backward(ctx, g):
        ctx.seen[ctx.key] = g
        return ctx.g_engine.to(g.dtype), None, None, None


def _forced(z, key, force, gforce=None, seen=None):
    """continue from the engine's stored tensor force[key] (values), and from the engine's stored gradient gforce[key] on the way back"""
    if force is not None:
        z = z + (force[key].to(z.dtype) - z).detach()
    if gforce is not None:
        z = _ForceGrad.apply(z, gforce[key], seen, key)
    return z


def residual_block(x, w1, b1, w2, b2, store=None, stats=None, force=None, gforce=None, seen=None):
    """returns the stages {raw1, a1, raw2, out} (as computed, before any teacher forcing) of one block. stats: (stats of raw1, stats of raw2) or None.
    force: {raw1, a1, raw2} engine tensors (NCHW) to continue from, or None. gforce: the engine's stored GRADIENTS of the same three tensors: the
    backward continues from them too, and the gradient the restatement itself arrives at is filed in the dict `seen` under the same keys."""
    rb, rw, rg = rounders(store)
    s1, s2 = stats if stats is not None else (None, None)
    x3 = store == "bf16x3"
    raw1 = rb(conv3r(x, w1, b1, rw, rg, x3))
    a1 = rb(F.relu(instance_norm(_forced(raw1, "raw1", force, gforce, seen), s1)))
    raw2 = rb(conv3r(_forced(a1, "a1", force, gforce, seen), w2, b2, rw, rg, x3))
    out = rb(x + instance_norm(_forced(raw2, "raw2", force, gforce, seen), s2))
    return {"raw1": raw1, "a1": a1, "raw2": raw2, "out": out}


def block_params(sd, prefix):
    return [sd[f"{prefix}block.{i}.{s}"] for i in (1, 5) for s in ("weight", "bias")]


def trunk(x, sd, prefixes, store=None):
    """the residual blocks under the key prefixes `prefixes` of a state dict, one after the other"""
    for p in prefixes:
        x = residual_block(x, *block_params(sd, p), store=store)["out"]
    return x


def generator_resnet(x, sd, n_blocks):
    """GeneratorResNet((channels, H, W), n_blocks).forward from its state dict `sd` (keys model.<index>...): 7 x 7 stem behind a reflection pad of
    `channels` pixels, two stride-2 3 x 3 convolutions, the blocks, two nearest-neighbour upsample + 3 x 3 convolutions, the 7 x 7 head and tanh"""
    ch = x.shape[1]
    conv = lambda i: (sd[f"model.{i}.weight"], sd[f"model.{i}.bias"])  # noqa: E731
    h = F.relu(instance_norm(F.conv2d(F.pad(x, (ch,) * 4, mode="reflect"), *conv(1))))
    for i in (4, 7):
        h = F.relu(instance_norm(F.conv2d(h, *conv(i), stride=2, padding=1)))
    h = trunk(h, sd, [f"model.{10 + b}." for b in range(n_blocks)])
    for i in (11 + n_blocks, 15 + n_blocks):
        h = F.relu(instance_norm(F.conv2d(F.interpolate(h, scale_factor=2, mode="nearest"), *conv(i), padding=1)))
    return torch.tanh(F.conv2d(F.pad(h, (ch,) * 4, mode="reflect"), *conv(19 + n_blocks)))
