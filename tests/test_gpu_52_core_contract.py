"""What the step engines and the bucket reducers count on in the three network cores of nets.py and no other test pins: the order in which the
gradient hooks fire (with the side stream and without), `accumulate=True` (a second backward of the same context doubles every gradient exactly),
and `grads=None` (the input gradient of a discriminator does not depend on whether parameter gradients are computed beside it).
Every case at the smallest size its core accepts, N = 1."""
import numpy as np
import pytest
import torch

import tfc_gan_amd as T
from tfc_gan_amd import nets, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTS = {"bf16": (ops.DT_BF16, torch.bfloat16), "fp32": (ops.DT_F32, torch.float32)}


def rnd(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)).to(DEV)


@pytest.fixture(autouse=True)
def _side_stream_as_it_was():
    prev = nets.set_wgrad_stream(True)
    nets.set_wgrad_stream(prev)
    yield
    nets.set_wgrad_stream(prev)


def _params(module, names):
    module.apply(T.weights_init_normal)
    sd = dict(module.named_parameters())
    return {k: sd[k].detach().clone().to(DEV) for k in names}


def _logit_grad(logits, dt, seed):
    gl = ops.new_act(logits.N, logits.H, logits.W, 8, dt, DEV, zero=True)
    gl.t[..., 0] = rnd((logits.N, logits.H, logits.W), seed, 1e-2).to(gl.t.dtype)
    return gl


def make_g(dt, labels=0):
    """GeneratorCore at N = 1, S = 128; returns (core, params, forward() -> ctx, backward(ctx, grads, **kw))"""
    torch.manual_seed(1)
    params = _params(T.GeneratorUNet((3, 128, 128), labels=labels), nets.g_param_names(labels))
    core = nets.GeneratorCore(dt, 3, labels)
    core.set_params(params)
    x, g_fake = rnd((1, 3, 128, 128), 2, 0.5), rnd((1, 3, 128, 128), 3, 1e-2)
    lab = torch.tensor([[1.0, 2.0, 0.0]], device=DEV) if labels else None

    def forward():
        return core.forward(x, seed=5, train=True, labels=lab)[1]

    def backward(ctx, grads, **kw):
        return core.backward(ctx, g_fake, grads, **kw)
    return core, params, forward, backward


def make_d(dt):
    """DiscriminatorCore at N = 1, 64 x 64"""
    torch.manual_seed(2)
    mod = T.Discriminator1((3, 64, 64))
    params = _params(mod, nets.d_param_names())
    bufs = {k: v.detach().clone().to(DEV) for k, v in mod.named_core_buffers().items()}
    core = nets.DiscriminatorCore(dt, 3)
    core.set_params(params, bufs)
    a, b = rnd((1, 3, 64, 64), 4, 0.5), rnd((1, 3, 64, 64), 5, 0.5)

    def forward():
        logits, ctx = core.forward(a, b, power_iter=False)
        ctx.gl = _logit_grad(logits, dt, 6)
        return ctx

    def backward(ctx, grads, **kw):
        return core.backward(ctx, ctx.gl, grads, **kw)
    return core, params, forward, backward


def make_p(dt):
    """Pix2PixCore at N = 1, 32 x 48"""
    torch.manual_seed(3)
    params = _params(T.Pix2PixDiscriminator((3, 32, 48)), nets.p2p_param_names())
    core = nets.Pix2PixCore(dt, 3)
    core.set_params(params)
    a, b = rnd((1, 3, 32, 48), 7, 0.5), rnd((1, 3, 32, 48), 8, 0.5)

    def forward():
        logits, ctx = core.forward(a, b)
        ctx.gl = _logit_grad(logits, dt, 9)
        return ctx

    def backward(ctx, grads, **kw):
        return core.backward(ctx, ctx.gl, grads, **kw)
    return core, params, forward, backward


def _fresh(params):
    return {k: torch.full_like(v, 7.0) for k, v in params.items()}      # a backward overwrites: nothing of the 7 may survive


# (maker, backward keywords, the order the hooks must fire in)
HOOK_CASES = {
    "generator": (lambda dt: make_g(dt), {}, lambda: [k for k in nets.g_backward_order() if k not in nets.G_FC]),
    "generator_labels": (lambda dt: make_g(dt, labels=3), {"need_input_grad": False}, lambda: nets.g_backward_order()),
    "discriminator": (make_d, {"need_input_grad": False}, lambda: [k for k in nets.d_backward_order() if k not in nets.d_aux_names()]),
    "pix2pix": (make_p, {"need_input_grad": False}, lambda: nets.p2p_backward_order()),
}


@pytest.mark.parametrize("side", [True, False], ids=["side_stream", "one_stream"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("case", list(HOOK_CASES))
def test_hooks_fire_in_backward_order(case, dtype, side):
    """hook(key) once per parameter, in the order of *_backward_order() filtered to the parameters the core has: the bucket reducers issue a
    bucket's all-reduce when its LAST gradient reports, so an order that differs from the flat buffer's sends buckets late or not at all. bf16 takes
    the fused first block and the head kernels, fp32 the plain branches."""
    dt, tdt = DTS[dtype]
    T.set_compute_dtype(tdt)
    try:
        nets.set_wgrad_stream(side)
        make, kw, order = HOOK_CASES[case]
        core, params, forward, backward = make(dt)
        fired = []
        backward(forward(), _fresh(params), hook=fired.append, **kw)
        torch.cuda.synchronize()
        want = [k for k in order() if k in params]
        assert sorted(want) == sorted(params)
        assert fired == want
    finally:
        T.set_compute_dtype(torch.bfloat16)


@pytest.mark.parametrize("case", ["generator", "discriminator", "pix2pix"])
def test_accumulate_doubles_every_gradient(case):
    """backward into fresh gradient tensors, then a second backward of the same context with accumulate=True: every gradient is exactly twice the
    first (x + x is exact in fp32, and a backward is bit-reproducible)"""
    make, kw, _ = HOOK_CASES[case]
    core, params, forward, backward = make(ops.DT_BF16)
    ctx = forward()
    grads = _fresh(params)
    backward(ctx, grads, **kw)
    torch.cuda.synchronize()
    first = {k: v.clone() for k, v in grads.items()}
    backward(ctx, grads, accumulate=True, **kw)
    torch.cuda.synchronize()
    for k in params:
        assert torch.isfinite(first[k]).all(), k
        assert torch.equal(grads[k], first[k] + first[k]), k
    assert any(first[k].abs().max().item() > 0 for k in params)


@pytest.mark.parametrize("case", ["discriminator", "pix2pix"])
def test_input_gradient_without_parameter_gradients(case):
    """grads=None, need_input_grad=True (the generator step) returns the bits of the input gradient that comes with parameter gradients requested"""
    make, _, _ = HOOK_CASES[case]
    core, params, forward, backward = make(ops.DT_BF16)
    ctx = forward()
    with_grads = backward(ctx, _fresh(params), need_input_grad=True)
    alone = backward(ctx, None, need_input_grad=True)
    torch.cuda.synchronize()
    assert alone.shape == with_grads.shape and alone.abs().max().item() > 0
    assert torch.equal(alone, with_grads)
