"""CycleGAN's residual trunk on the HIP kernels: ResidualBlock, nets.ResNetTrunkCore and GeneratorResNet against tests/cyclegan_ref.py (a float64
restatement in plain torch.nn.functional) and against the module's own torch path.

Every block is compared on its own and stage by stage, as tests/test_gpu_10_networks.py compares the layers of the U-Net: the restatement gets the
ENGINE's stored input of the block, the engine's InstanceNorm statistics (so the variance needs no tolerance and a ReLU mask is decided by identical
numbers) and the engine's gradient of the block's output, and continues every stage from the tensor the engine stored there -- the two convolution
outputs and the activation on the way forward, their three gradients on the way back. All nine results are checked: four forward stages, three stored
gradients, the input gradient (with the accumulate onto the skip gradient) and the four parameter gradients.

  fp32, bf16x3: the bounds test_gpu_10_networks.py applies to UNetDown / UNetUp in fp32 mode -- max |error| 2e-5 forward, 5e-5 input gradient, 2e-4
                parameter gradients (stored gradients: the input-gradient bound). bf16x3 drops the lo x lo term of every product (up to
                2^-16 |a b|); a restatement that multiplies exactly is 3.5e-5 / 7e-4 away from it over a whole block at these shapes (measured),
                so the restatement forms its convolutions from the same split operands (cyclegan_ref._ConvX3).
  bf16:         the project's layer bounds against the bf16-storage model (README: 6.5e-5 forward, 3.0e-3 backward, rel-L2): the restatement rounds
                where the engine stores (after each convolution, after the activation, after the add, the padded gradient in the fold pass's
                scratch) and continues every stage from the engine's stored tensor.
A bias in front of an InstanceNorm has a gradient that cancels to rounding noise, in the restatement as in the engine: a ratio of two noises says
nothing, so in bf16 its error is measured against what the sum is formed from, the per-channel sums of |gradient entering the convolution|.
"""
import pytest
import torch

import tfc_gan_amd as T
from oracle import tfcgan_oracle as O
from tests import cyclegan_ref as R
from tfc_gan_amd import nets, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
MODES = [pytest.param(torch.float32, id="fp32"), pytest.param("bf16x3", id="bf16x3"), pytest.param(torch.bfloat16, id="bf16")]
ABS_FWD, ABS_GX, ABS_GP = 2e-5, 5e-5, 2e-4                       # fp32 / bf16x3: tests/test_gpu_10_networks.py::test_blocks_vs_reference_goldens
BF_FWD, BF_BWD = 6.5e-5, 3.0e-3                                  # bf16: the project's layer bounds (README)


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    T.set_compute_dtype(torch.bfloat16)


def _nchw(v):
    return v.t[..., v.coff:v.coff + v.C].permute(0, 3, 1, 2).to(F64).contiguous()


def _rel(got, want):
    return ((got.to(F64) - want.to(F64)).norm() / want.to(F64).norm().clamp_min(1e-300)).item()


def _gauss(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float32) * scale).to(DEV)


def _is_bf16(dtype):
    return dtype == torch.bfloat16


def check_block(tag, dtype, saved, g_out, dgrads, params, got_out, got_gx, got_gp):
    """one residual block of the engine against the restatement, stage by stage. saved: (x, raw1, st1, a1, raw2, st2) as the core stored them; g_out: the
    engine's gradient of the block's output (NCHW float64); dgrads: the engine's stored gradients {raw1, a1, raw2} (Views); params: [w1, b1, w2, b2];
    got_*: the engine's output, input gradient and parameter gradients. Every stage continues from the engine's stored tensor, forward and backward."""
    x_e, raw1, st1, a1, raw2, st2 = saved
    bf = _is_bf16(dtype)
    x = _nchw(x_e).requires_grad_(True)
    ps = [p.detach().to(F64).clone().requires_grad_(True) for p in params]
    force = {"raw1": _nchw(raw1), "a1": _nchw(a1), "raw2": _nchw(raw2)}
    gforce = {k: _nchw(v) for k, v in dgrads.items()}
    seen = {}
    store = "bf16" if bf else ("bf16x3" if dtype == "bf16x3" else None)
    st = R.residual_block(x, *ps, store=store, stats=(st1.float(), st2.float()), force=force, gforce=gforce, seen=seen)
    gx, *gp = torch.autograd.grad(st["out"], [x] + ps, g_out)
    fwd = [("raw1", force["raw1"], st["raw1"]), ("a1", force["a1"], st["a1"]), ("raw2", force["raw2"], st["raw2"]), ("out", got_out, st["out"])]
    rnd = R._bf if bf else (lambda v: v)
    bwd = [("d_raw2", gforce["raw2"], rnd(seen["raw2"])), ("d_a1", gforce["a1"], rnd(seen["a1"])), ("d_raw1", gforce["raw1"], rnd(seen["raw1"])),
           ("gx", got_gx, rnd(gx))]
    wts = [("w1", got_gp[0], gp[0]), ("w2", got_gp[2], gp[2])]
    bias = [("b1", got_gp[1], gp[1], gforce["raw1"]), ("b2", got_gp[3], gp[3], gforce["raw2"])]
    if bf:
        res = {k: (_rel(a, b), BF_FWD) for k, a, b in fwd}
        res.update({k: (_rel(a, b), BF_BWD) for k, a, b in bwd + wts})
        res.update({k: (((a.to(F64) - b).norm() / d.abs().sum((0, 2, 3)).norm()).item(), BF_BWD) for k, a, b, d in bias})
        what = "rel-L2"
    else:
        amax = lambda a, b: (a.to(F64) - b).abs().max().item()  # noqa: E731
        res = {k: (amax(a, b), ABS_FWD) for k, a, b in fwd}
        res.update({k: (amax(a, b), ABS_GX) for k, a, b in bwd})
        res.update({k: (amax(a, b), ABS_GP) for k, a, b in wts + [t[:3] for t in bias]})
        what = "max |error|"
    print("\n".join(f"  {tag} {k:6s} {what} {v:.3e} (bound {b})" for k, (v, b) in res.items()))
    assert all(v <= b for v, b in res.values()), (tag, {k: v for k, (v, b) in res.items() if v > b})


@pytest.mark.parametrize("dtype", MODES)
@pytest.mark.parametrize("hw", [(8, 16), (9, 17)], ids=["8x16", "9x17"])
def test_residual_block_module(hw, dtype):
    """ResidualBlock(32) on its own through autograd, fp32 NCHW in and out: forward, input gradient and the four parameter gradients"""
    T.set_compute_dtype(dtype)
    H, W = hw
    blk = O.init_weights_portable(T.ResidualBlock(32), seed=71, std=0.05).to(DEV)
    x = _gauss((2, 32, H, W), 72)
    go = _gauss((2, 32, H, W), 73)
    if _is_bf16(dtype):                                           # what crosses the module boundary is stored in bf16: start from representable values
        x, go = x.bfloat16().float(), go.bfloat16().float()
    x.requires_grad_(True)
    core = blk._core_for(DEV)
    core.debug = {}
    y = blk(x)
    y.backward(go)
    torch.cuda.synchronize()
    assert y.shape == x.shape and y.dtype == torch.float32
    names = nets.res_block_keys("")
    sd = dict(blk.named_parameters())
    dbg = core.debug
    check_block(f"ResidualBlock {H}x{W}", dtype, dbg["ctx"].blocks[0], go.to(F64), {k: dbg[f"0.d_{k}"] for k in ("raw1", "a1", "raw2")},
                [sd[k] for k in names], y.detach(), x.grad, [sd[k].grad for k in names])


@pytest.mark.parametrize("dtype", MODES)
def test_resnet_trunk_core_two_blocks(dtype):
    """nets.ResNetTrunkCore with 2 blocks on raw NHWC buffers: every block's forward, input gradient (the accumulate onto the skip gradient included) and
    parameter gradients; the gradients of a second call with accumulate=True are twice the first's"""
    dt = ops.dt_of(dtype)
    C, N, H, W = 32, 2, 9, 17
    core = nets.ResNetTrunkCore(dt, C, 2)
    names = core.param_names()
    assert names == [f"{b}.block.{i}.{s}" for b in (0, 1) for i in (1, 5) for s in ("weight", "bias")]
    params = {k: _gauss((C, C, 3, 3) if k.endswith("weight") else (C,), 80 + i, 0.05) for i, k in enumerate(names)}
    core.set_params(params)
    core.debug = {}
    xv = ops.View(_gauss((N, C, H, W), 90).permute(0, 2, 3, 1).contiguous().to(ops.torch_dtype(dt)), C)
    out, ctx = core.forward(xv)
    g0 = _gauss((N, C, H, W), 91).permute(0, 2, 3, 1).contiguous().to(ops.torch_dtype(dt))
    grads = {k: torch.full_like(v, 7.0) for k, v in params.items()}
    fired = []
    g_in = core.backward(ctx, ops.View(g0.clone(), C), grads, hook=fired.append)
    torch.cuda.synchronize()
    assert fired == core.backward_order()
    dbg = core.debug
    for b in (1, 0):
        keys = nets.res_block_keys(f"{b}.")
        blk_out = _nchw(ctx.blocks[b + 1][0]) if b == 0 else _nchw(out)
        check_block(f"trunk block {b}", dtype, ctx.blocks[b], _nchw(dbg[f"{b}.g_out"]), {k: dbg[f"{b}.d_{k}"] for k in ("raw1", "a1", "raw2")},
                    [params[k] for k in keys], blk_out, _nchw(dbg[f"{b}.g_in"]), [grads[k] for k in keys])
    assert torch.equal(g_in.t, dbg["0.g_in"].t)
    first = {k: v.clone() for k, v in grads.items()}
    core.backward(ctx, ops.View(g0.clone(), C), grads, accumulate=True)
    torch.cuda.synchronize()
    for k in names:
        assert torch.allclose(grads[k], 2 * first[k], rtol=1e-6, atol=1e-7), k


def _generators(hw, n_blocks=2):
    T.set_compute_dtype(torch.float32)
    H, W = hw
    g_hip = O.init_weights_portable(T.GeneratorResNet((3, H, W), n_blocks), seed=75, std=0.05).to(DEV)
    g_ref = T.GeneratorResNet((3, H, W), n_blocks, trunk="torch").to(DEV)
    g_ref.load_state_dict(g_hip.state_dict())
    return g_hip, g_ref


def _fwd_bwd(g, x0, go):
    g.zero_grad(set_to_none=True)
    x = x0.clone().requires_grad_(True)
    y = g(x)
    y.backward(go)
    torch.cuda.synchronize()
    return y.detach(), x.grad, {k: p.grad.clone() for k, p in g.named_parameters()}


@pytest.mark.parametrize("hw", [(32, 32), (40, 72)], ids=["32x32", "40x72"])
def test_generator_resnet_hip_trunk_vs_torch_trunk(hw):
    """GeneratorResNet((3, H, W), 2), fp32 mode: trunk="hip" against trunk="torch" with the same state_dict. The stem and the head are the same torch code on
    both sides, so the difference is the trunk's and the block bounds apply: output, input gradient, every parameter gradient. Two forward + backward
    runs from the same state give equal bits.
    The gradient of the output is Gaussian at 1e-3, the scale tests/test_gpu_10_networks.py gives the gradient of a whole generator's image (a loss
    averaged over pixels). The absolute bounds say little about gradients of that size, so every tensor that does not cancel to noise (all but the
    biases in front of an InstanceNorm) is held to REL_L2 = 1e-4 as well: two fp32 evaluations of ~20 layers in sequence, each a sum of up to 2304
    products (2^-24 x sqrt(2304) = 3e-6 per layer, forward and backward), and a partner whose 3 x 3 convolutions may take a Winograd route."""
    REL_L2 = 1e-4
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        g_hip, g_ref = _generators(hw)
        x0, go = _gauss((2, 3) + hw, 76), _gauss((2, 3) + hw, 77, 1e-3)
        y, gx, gp = _fwd_bwd(g_hip, x0, go)
        y_r, gx_r, gp_r = _fwd_bwd(g_ref, x0, go)
        assert y.shape == (2, 3) + hw and y.dtype == torch.float32
        err = {"out": ((y - y_r).abs().max().item(), ABS_FWD), "gx": ((gx - gx_r).abs().max().item(), ABS_GX)}
        assert set(gp) == set(gp_r) == set(dict(g_hip.named_parameters()))
        for k in gp:
            err[k] = ((gp[k] - gp_r[k]).abs().max().item(), ABS_GP)
        print("\n".join(f"  {k:28s} max |error| {v:.3e} (bound {b})" for k, (v, b) in err.items()))
        assert all(v <= b for v, b in err.values()), {k: v for k, (v, b) in err.items() if v > b}
        n = g_hip.num_residual_blocks
        real = ["out", "gx", f"model.{19 + n}.bias"] + [k for k in gp if k.endswith("weight")]
        rel = {k: _rel(a, b) for k, a, b in [("out", y, y_r), ("gx", gx, gx_r)] + [(k, gp[k], gp_r[k]) for k in real[2:]]}
        print("\n".join(f"  {k:28s} rel-L2 {v:.3e} (bound {REL_L2})" for k, v in rel.items()))
        assert all(v <= REL_L2 for v in rel.values()), {k: v for k, v in rel.items() if v > REL_L2}
        y2, gx2, gp2 = _fwd_bwd(g_hip, x0, go)
        moved = [k for k, u, v in [("out", y, y2), ("gx", gx, gx2)] + [(k, gp[k], gp2[k]) for k in gp] if not torch.equal(u, v)]
        assert not moved, ("two runs from the same state differ in", moved)
    finally:
        torch.backends.cudnn.deterministic = prev


def test_generator_resnet_checkpoints(tmp_path):
    """save_checkpoint then load_clean_state round-trips; a state dict with a missing trunk key is refused as torch refuses it"""
    g_hip, _ = _generators((32, 32))
    path = str(tmp_path / "G_AB.pth")
    T.save_checkpoint(g_hip, path)
    g2 = T.load_clean_state(T.GeneratorResNet((3, 32, 32), 2), path)
    sd, sd2 = g_hip.state_dict(), g2.state_dict()
    assert list(sd) == list(sd2)
    for k in sd:
        assert torch.equal(sd[k].cpu(), sd2[k].cpu()), k
    bad = {k: v for k, v in sd.items() if k != "model.10.block.5.weight"}
    with pytest.raises(RuntimeError, match="Missing key.*model.10.block.5.weight"):
        T.GeneratorResNet((3, 32, 32), 2).load_state_dict(bad)
