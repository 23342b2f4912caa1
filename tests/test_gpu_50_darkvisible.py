"""GPU tests of the DarkVisible step (TFC-STN/TFCGAN_STN21_Eur_DarkVisible.py, "DV"): the mixed-mode warp against torch's own two calls, the plain
pix2pix PatchGAN (Pix2PixDiscriminator on TFC_OP_CONV2) against its torch restatement in fp64 and, in bf16, layer by layer against the bf16-storage
restatement, and DarkVisibleStep against the step composed from the script's own definitions (tests/golden/train_step_darkvisible.npz)."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tfc_gan_amd as T
from oracle import tfcgan_oracle as O
from tests import conv_exact as X
from tests import pix2pix_ref as R
from tfc_gan_amd import stn21

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rnd(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32))


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.fixture(autouse=True)
def _bf16_default_afterwards():
    yield
    T.set_compute_dtype(torch.bfloat16)


# ---- warp ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.filterwarnings("ignore:Since version 1.3.0, affine_grid behavior has changed for unit-size grids")     # the H = 1 case, on purpose
@pytest.mark.parametrize("N,C,H,W", [(3, 3, 5, 7), (1, 1, 2, 2), (2, 1, 1, 6)])
def test_affine_warp_mixed_mode_vs_torch(N, C, H, W):
    """sample_align_corners=False (grid align_corners=True, sampling align_corners=False: DV:205-206) against torch in fp64 on the CPU: forward and the
    gradients w.r.t. theta and src, at the bounds of test_affine_warp_forward_backward_vs_torch; a 1-pixel axis behaves as torch's does"""
    src = rnd((N, C, H, W), 1)
    ident = torch.tensor([[1.0, 0, 0], [0, 1.0, 0]])
    theta = ident[None] + rnd((N, 2, 3), 2, 0.3)
    go = rnd((N, C, H, W), 3)
    s64, t64 = src.double().requires_grad_(True), theta.double().requires_grad_(True)
    want = R.mixed_warp(s64, t64, sample_align_corners=False)
    gsrc, gth = torch.autograd.grad(want, (s64, t64), go.double())
    s2, t2 = src.to(DEV).requires_grad_(True), theta.to(DEV).requires_grad_(True)
    got = T.affine_warp(s2, t2, sample_align_corners=False)
    g2s, g2t = torch.autograd.grad(got, (s2, t2), go.to(DEV))
    e_f = (got.cpu().double() - want.detach()).abs().max().item()
    e_s = (g2s.cpu().double() - gsrc).abs().max().item()
    e_t = (g2t.cpu().double() - gth).abs().max().item()
    print(f"warp {N, C, H, W}: forward {e_f:.3e}, d src {e_s:.3e}, d theta {e_t:.3e} (|d theta| max {gth.abs().max().item():.3e})")
    assert e_f <= 2e-4 * max(1.0, want.abs().max().item())
    assert e_s <= 1e-4 * max(1.0, gsrc.abs().max().item())
    assert e_t <= 2e-3 * max(1.0, gth.abs().max().item()), (g2t.cpu(), gth)
    # the module forms carry the convention
    w = T.Warp(sample_align_corners=False)(t2.detach() - ident.to(DEV), s2.detach())
    assert torch.equal(w, got.detach())


def test_affine_warp_default_mode_keeps_its_bits():
    """sample_align_corners=True IS affine_warp as it was: the same entry points, the same bits, forward and backward; and the two conventions differ"""
    src, theta, go = rnd((3, 3, 5, 7), 1), torch.tensor([[1.0, 0, 0], [0, 1.0, 0]])[None] + rnd((3, 2, 3), 2, 0.3), rnd((3, 3, 5, 7), 3)

    def run(*extra, **kw):
        s, t = src.to(DEV).requires_grad_(True), theta.to(DEV).requires_grad_(True)
        y = T.affine_warp(s, t, *extra, **kw)
        return (y.detach(),) + torch.autograd.grad(y, (s, t), go.to(DEV))
    base, explicit, mixed = run(), run(sample_align_corners=True), run(sample_align_corners=False)
    # d src is the library's one scatter through float atomics (include/tfc_gan.h): the order of its additions, and so its last bits, may differ from
    # run to run -- at most 35 x 16 taps of |go w| <= 8 land on one source pixel, so 1e-4 is far above any reordering and far below a wrong tap
    assert torch.equal(base[0], explicit[0]) and torch.equal(base[2], explicit[2]) and (base[1] - explicit[1]).abs().max().item() <= 1e-4
    assert torch.equal(T.Warp()(theta.to(DEV) - torch.tensor([[1.0, 0, 0], [0, 1.0, 0]], device=DEV), src.to(DEV)), base[0])
    assert (base[0] - mixed[0]).abs().max().item() > 0.1          # up to half a pixel at the borders
    # the entry points that take the convention, called with sample_align_corners = 1: the bits of the old pair, forward and backward
    from tfc_gan_amd import ops
    lib, p = ops.lib(), ops._p
    s, t, g = src.to(DEV), theta.to(DEV).reshape(-1, 6).contiguous(), go.to(DEV)
    out, dth, dsrc = torch.empty_like(s), torch.empty((3, 6), device=DEV), torch.empty_like(s)
    assert lib.tfc_affine_warp_mode_fwd(ops.stream_ptr(), p(s), p(t), p(out), 3, 3, 5, 7, 1) == 0, lib.tfc_last_error()
    assert lib.tfc_affine_warp_mode_bwd(ops.stream_ptr(), p(s), p(t), p(g), p(dth), p(dsrc), 3, 3, 5, 7, 1, ops.part_ws(torch.device(DEV))) == 0, lib.tfc_last_error()
    torch.cuda.synchronize()
    assert torch.equal(out, base[0]) and torch.equal(dth.reshape(3, 2, 3), base[2]) and (dsrc - base[1]).abs().max().item() <= 1e-4


# ---- the discriminator ------------------------------------------------------------------------------------------------------------------------------
CONVS = (0, 2, 5, 8, 12)


def test_pix2pix_discriminator_fp32_vs_torch_fp64():
    """N = 2, 32 x 32, fp32 parity mode against the torch restatement in fp64: logits (the bar of test_discriminator_logits_vs_golden_fp32), the five
    weight gradients, the bias gradient of block 1 and the gradient of img_A (the per-element bars of test_blocks_vs_reference_goldens, relative to the
    tensor's largest element where that exceeds 1, and the rel-L2 bar of the fp32 step); the biases of blocks 2-4 get exact zeros"""
    T.set_compute_dtype(torch.float32)
    Dr = O.init_weights_portable(R.Pix2PixRef(), seed=31)
    D = T.Pix2PixDiscriminator((3, 32, 32))
    D.load_state_dict(Dr.state_dict())
    D = D.to(DEV)
    Dr = Dr.double()
    a, b, go = rnd((2, 3, 32, 32), 1, 0.5), rnd((2, 3, 32, 32), 2, 0.5), rnd((2, 1, 2, 2), 3)
    a64 = a.double().requires_grad_(True)
    want = Dr(a64, b.double())
    (want * go.double()).sum().backward()
    ag = a.to(DEV).requires_grad_(True)
    got = D(ag, b.to(DEV))
    assert got.shape == (2, 1, 2, 2) and got.dtype == torch.float32
    (got * go.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    e = (got.detach().cpu().double() - want.detach()).abs().max().item()
    print(f"logits: max err {e:.3e} of max {want.abs().max().item():.3e}")
    assert e <= 2e-5 * want.abs().max().item()

    def check(tag, g, w, per_elem):
        err, r = (g.cpu().double() - w).abs().max().item(), rel(g.cpu(), w)
        print(f"  {tag:16s} max err {err:.3e} (|ref| max {w.abs().max().item():.3e}), rel-L2 {r:.3e}")
        assert err <= per_elem * max(1.0, w.abs().max().item()), (tag, err)
        assert r <= 1e-2, (tag, r)
    for i in CONVS:
        check(f"model.{i}.weight", D.model[i].weight.grad, Dr.model[i].weight.grad, 2e-4)
    check("model.0.bias", D.model[0].bias.grad, Dr.model[0].bias.grad, 2e-4)
    check("img_A", ag.grad, a64.grad, 5e-5)
    for i in (2, 5, 8):
        assert torch.equal(D.model[i].bias.grad, torch.zeros_like(D.model[i].bias)), i
        assert Dr.model[i].bias.grad.abs().max().item() <= 1e-9 * Dr.model[i].weight.grad.abs().max().item()      # zero up to fp64 round-off


def _nchw(v):
    return v.t[..., v.coff:v.coff + v.C].permute(0, 3, 1, 2).float().cpu()


def test_pix2pix_discriminator_bf16_layers_teacher_forced_vs_storage_restatement():
    """bf16, N = 2, 64 x 64: every block and the head against the bf16-storage restatement of that layer, fed with the ENGINE's stored input, the engine's
    statistics and the engine's incoming gradient: forward <= 5e-4, backward <= 5e-3 rel-L2 (the project's bars, no per-layer exceptions)"""
    FWD, BWD = 5e-4, 5e-3
    rb, rw, rg = O._RoundBoth.apply, O._RoundFwd.apply, O._RoundBwd.apply
    Dr = O.init_weights_portable(R.Pix2PixRef(), seed=32)
    names = T.nets.p2p_param_names()
    sd = Dr.state_dict()
    params = {k: sd[k].clone().to(DEV) for k in names}
    N, S = 2, 64
    a, b = rnd((N, 3, S, S), 4, 0.5).clamp(-1, 1), rnd((N, 3, S, S), 5, 0.5).clamp(-1, 1)
    g_log = rnd((N, S // 16, S // 16), 6, 1e-2)
    core = T.nets.Pix2PixCore(T.ops.DT_BF16)
    core.set_params(params)
    core.debug = {}
    logits, ctx = core.forward(a.to(DEV), b.to(DEV))
    gl = T.ops.new_act(N, S // 16, S // 16, 8, T.ops.DT_BF16, DEV, zero=True)
    gl.t[..., 0] = g_log.to(DEV).to(torch.bfloat16)
    grads = {k: torch.full_like(v, 7.0) for k, v in params.items()}                  # overwritten, not accumulated
    gimg = core.backward(ctx, gl, grads, need_input_grad=True)
    torch.cuda.synchronize()
    dbg = core.debug
    worst = [0.0, 0.0]

    def check(tag, got, want, tol, slot):
        r = rel(got, want)
        worst[slot] = max(worst[slot], r)
        print(f"  {tag:36s} rel-L2 {r:.3e}")
        assert r <= tol, (tag, r)

    for bi, (i, cin, cout, norm) in enumerate(core.blocks()):
        W = sd[f"model.{i}.weight"].clone().requires_grad_(True)
        bias = sd[f"model.{i}.bias"].clone().requires_grad_(True)
        x = _nchw(ctx.ins[bi])[:, :cin].clone().requires_grad_(True)
        z = F.conv2d(x, rw(W), bias, stride=2, padding=1)
        raw_e = _nchw(ctx.raw[bi])
        y_e = _nchw(ctx.ins[bi + 1]) if bi < 3 else _nchw(ctx.p4)
        g_out = _nchw(dbg[f"b{bi}.g_out"])
        if norm:
            check(f"block{bi} conv2+bias fwd", raw_e, O._bf(z.detach()), FWD, 0)
            zt = rb(z + (raw_e - z).detach())                          # teacher forcing: continue from the ENGINE's stored conv output
            y = F.leaky_relu(X.EngineStatsNorm.apply(zt, ctx.stats[bi].cpu(), 1e-5), 0.2)
            check(f"block{bi} norm+leaky fwd", y_e, O._bf(y.detach()), FWD, 0)
            gW, gb, gx, gz = torch.autograd.grad(y, [W, bias, x, zt], g_out)
            assert torch.equal(grads[f"model.{i}.bias"], torch.zeros_like(grads[f"model.{i}.bias"])), "a bias in front of InstanceNorm: exact zeros"
            # torch's value there: the sum of the bf16-ROUNDED conv-output gradient, whose exact sum is zero -- at most 2^-9 |g| of rounding per element
            assert (gb.abs() <= 2.0 ** -8 * gz.abs().sum((0, 2, 3))).all()
        else:
            zg = rg(z)
            y = F.leaky_relu(zg, 0.2)
            check(f"block{bi} conv2+bias+leaky fwd", raw_e, O._bf(y.detach()), FWD, 0)
            gW, gb, gx, gz = torch.autograd.grad(y, [W, bias, x, z], g_out)
            check(f"block{bi} bias grad", grads[f"model.{i}.bias"].cpu(), gb, BWD, 1)
        check(f"block{bi} d_raw", _nchw(dbg[f"b{bi}.d_raw"]), O._bf(gz), BWD, 1)
        check(f"block{bi} wgrad", grads[f"model.{i}.weight"].cpu(), gW, BWD, 1)
        if bi > 0:
            check(f"block{bi} dgrad", _nchw(dbg[f"b{bi - 1}.g_out"]), O._bf(gx), BWD, 1)
        else:
            check("block0 image gradient", gimg.cpu(), O._bf(gx[:, :3]), BWD, 1)
    Wh = sd["model.12.weight"].clone().requires_grad_(True)
    xh = _nchw(ctx.p4).clone().requires_grad_(True)
    lg = rb(F.conv2d(F.pad(xh, (1, 0, 1, 0)), Wh, padding=1))
    glb = g_log.to(torch.bfloat16).float().reshape(N, 1, S // 16, S // 16)
    check("head fwd", logits.t[..., 0].float().cpu().reshape(N, 1, S // 16, S // 16), lg.detach(), FWD, 0)
    gWh, gxh = torch.autograd.grad(lg, [Wh, xh], glb)
    check("head wgrad", grads["model.12.weight"].cpu(), gWh, BWD, 1)
    check("head dgrad", _nchw(dbg["b3.g_out"]), O._bf(gxh), BWD, 1)
    print("worst forward", worst[0], "worst backward", worst[1])
    # the module and the whole-network restatement agree end to end at the bf16 level
    D = T.Pix2PixDiscriminator((3, S, S))
    D.load_state_dict(sd)
    D = D.to(DEV)
    T.set_compute_dtype(torch.bfloat16)
    with torch.no_grad():
        e2e = rel(D(a.to(DEV), b.to(DEV)).cpu(), R.forward_bf16(Dr, a, b))
    print("module vs bf16-storage restatement, logits rel-L2", e2e)
    assert e2e <= 2e-2


def test_pix2pix_discriminator_surface():
    """compute_dtype per module, the operand streams follow an in-place weight update, a size that is no multiple of 16 is refused, and "bf16x3" runs"""
    T.set_compute_dtype(torch.bfloat16)
    D = O.init_weights_portable(T.Pix2PixDiscriminator((3, 32, 32)), seed=33).to(DEV)
    a, b = rnd((1, 3, 32, 32), 1, 0.5).to(DEV), rnd((1, 3, 32, 32), 2, 0.5).to(DEV)
    with torch.no_grad():
        y0 = D(a, b)
        D.compute_dtype = torch.float32
        y32 = D(a, b)
        D.compute_dtype = "bf16x3"
        yx3 = D(a, b)
        D.compute_dtype = None
        assert not torch.equal(y0, y32) and rel(y0, y32) <= 3e-2
        assert rel(yx3, y32) <= 1e-4
        D.model[12].weight.mul_(2.0)                              # _version moves: the core re-reads the weights
        assert rel(D(a, b), 2.0 * y0) <= 1e-2
        with pytest.raises(T.TfcError, match="multiples of 16"):
            D(a[..., :24], b[..., :24])


# ---- the step -----------------------------------------------------------------------------------------------------------------------------------------
def _portable_dv(dtype):
    """DarkVisibleStep with the weights of tests/golden/train_step_darkvisible.npz: init_weights_portable seeds 101..105 in the fixture's module order,
    the last localiser layer scaled for a visible warp"""
    T.set_compute_dtype(dtype)
    st = T.DarkVisibleStep((3, 256, 256), lpips=None, device=DEV)
    for i, m in enumerate((st.G1, st.G2, st.D1, st.D2, st.net)):
        O.init_weights_portable(m, seed=101 + i)                  # writes through the parameter views into the flat buffers
    with torch.no_grad():
        st.net.fc_loc[6].weight.mul_(4.0)
        st.net.fc_loc[6].bias.copy_(torch.tensor([0.03, -0.02, 0.04, 0.02, -0.03, -0.05], device=DEV))
    st._bump()
    st.G1.eval(); st.G2.eval(); st.net.eval(); st.D1.train(); st.D2.train()
    return st


def test_darkvisible_step_vs_reference_golden(golden):
    """one step in the fp32 parity mode, N = 1, against the step composed from DV's own definitions (tests/golden/make_golden_darkvisible.py), at the
    bars of test_stn21_step_vs_reference_golden: the eight losses 3e-4, the images 2e-3, the gradients 2e-2 rel-L2 (fp32 gradients of an N = 1 step:
    activation knife-edge flips), the Adam deltas; the bias gradient of a block in front of InstanceNorm is exactly zero where torch has noise.
    Measured on the MI355X: losses <= 7e-6 relative, images <= 1.2e-4, G1 / G2 / localiser gradients 2.3e-3 .. 3.0e-3, D1.model.12 7e-6,
    D2.model.0.bias 4.3e-3, D2.model.8.weight[::16, ::16] 1.99e-2. The last is ONE LeakyReLU decision: 31 of the slice's 32 output channels agree to
    3e-5, channel 368 is off by 1.1e-1 (the signature of one element of its normalised 16 x 16 plane taking the other slope). The figure is the
    same to four digits with the HIP localiser, whose theta differs, and the engine's sums have a fixed order; on random inputs the discriminator
    agrees with torch fp64 to 4e-6 (test_pix2pix_discriminator_fp32_vs_torch_fp64)."""
    g = golden("train_step_darkvisible")
    st = _portable_dv(torch.float32)
    assert st.lr == 1e-4 and st.net.patch_size == 16 and st.net.warp.sample_align_corners is False
    assert [k for k, _ in st.net.state_dict().items()] == [str(k) for k in g["net_keys"]]
    assert list(st.D1.state_dict().keys()) == [str(k) for k in g["d_keys"]]
    before = {"G2.final": st.G2.final[2].weight.detach().clone(), "net.fc6": st.net.fc_loc[6].weight.detach().clone(),
              "D1.head": st.D1.model[12].weight.detach().clone()}
    A, B = O.synthetic_pairs(1, seed=105)
    out = st.step(A.to(DEV), B.to(DEV))
    torch.cuda.synchronize()
    assert set(out) == {"loss_G", "loss_GAN", "recon_loss", "perc_loss", "loss_FFT", "loss_D", "loss_D1", "loss_D2", "fake_B", "fake_A", "warped_B"}
    for k in ("loss_G", "loss_GAN", "recon_loss", "perc_loss", "loss_FFT", "loss_D", "loss_D1", "loss_D2"):
        w = float(g[k])
        print(f"  {k:12s} {float(out[k]):.7g} (reference {w:.7g})")
        assert abs(float(out[k]) - w) <= 3e-4 * max(1.0, abs(w)), (k, float(out[k]), w)
    for k, got in (("warped_sub", out["warped_B"]), ("fake_A_sub", out["fake_A"]), ("fake_B_sub", out["fake_B"])):
        err = (got.cpu()[:, :, ::8, ::8] - torch.from_numpy(g[k])).abs().max().item()
        print(f"  {k:12s} max err {err:.3e}")
        assert err <= 2e-3, (k, err)
    gv, dv = st.gflat.grad_views, st.dflat.grad_views
    checks = [("g_G1_down1", gv["G1.down1.model.0.weight"]), ("g_G2_down1", gv["G2.down1.model.0.weight"]), ("g_fc6", gv["net.fc_loc.6.weight"]),
              ("g_fc6_bias", gv["net.fc_loc.6.bias"]), ("g_fc0", gv["net.fc_loc.0.weight"][::64, ::256]), ("g_D1_head", dv["D1.model.12.weight"]),
              ("g_D2_b0", dv["D2.model.0.bias"]), ("g_D2_w8", dv["D2.model.8.weight"][::16, ::16])]
    for k, got in checks:
        r = rel(got.cpu(), torch.from_numpy(g[k]))
        print(f"  {k:12s} rel-L2 {r:.3e}")
        assert r <= 2e-2, (k, r)
    assert torch.equal(dv["D2.model.8.bias"], torch.zeros_like(dv["D2.model.8.bias"]))
    assert np.abs(g["g_D2_b8"]).max() <= 1e-5 * float(g["g_D2_w8_absmax"])          # the reference's value there: rounding noise
    for k, now, key in (("d_G2_final", st.G2.final[2].weight, "G2.final"), ("d_fc6", st.net.fc_loc[6].weight, "net.fc6"),
                        ("d_D1_head", st.D1.model[12].weight, "D1.head")):
        delta = (now.detach() - before[key]).cpu()
        # the first Adam step moves every weight by ~lr * sign(g): only entries whose gradient is at round-off level may differ
        frac = ((delta - torch.from_numpy(g[k])).abs() > 2e-5).float().mean().item()
        print(f"  {k:12s} fraction off {frac:.3e}")
        assert frac <= 2e-2, (k, frac)


@pytest.fixture(scope="module")
def lpips_crit():
    torch.manual_seed(11)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return T.LPIPS().to(DEV)


# parameters that the step's losses do not depend on: theta_emb is declared and never used (DV:157), a bias in front of InstanceNorm has a zero gradient
INERT = ("net.theta_emb.", "model.2.bias", "model.5.bias", "model.8.bias")


@pytest.mark.parametrize("localiser", ["torch", "hip"])
def test_darkvisible_step_batch4_bf16(localiser, lpips_crit):
    """batch 4, bf16, patch_size=64, with the LPIPS term: every parameter of the five networks that a loss depends on moves (the others stay bit for
    bit), all outputs are finite, loss_FFT changes no gradient (gflat.grad is torch.equal with the term computed and with it skipped), and with the
    HIP localiser two steps from the same state leave torch.equal gradient buffers"""
    T.set_compute_dtype(torch.bfloat16)
    A, B = T.synthetic_pairs(4, seed=23)
    A, B = A.to(DEV), B.to(DEV)

    def run(fft):
        torch.manual_seed(7)
        st = T.DarkVisibleStep((3, 256, 256), lpips=lpips_crit, device=DEV, seed=3, localiser=localiser, patch_size=64, fft=fft)
        before = {k: v.detach().clone() for flat in (st.gflat, st.dflat) for k, v in flat.views.items()}
        out = st.step(A, B)
        torch.cuda.synchronize()
        return st, out, before
    st, out, before = run(True)
    for k, v in out.items():
        assert torch.isfinite(v).all(), k
    assert out["loss_FFT"].item() > 0 and out["perc_loss"].item() > 0 and out["recon_loss"].item() > 0 and out["loss_D"].item() > 0
    assert abs(out["loss_G"].item() - (out["loss_GAN"] + out["recon_loss"] + out["perc_loss"] + out["loss_FFT"]).item()) <= 1e-3 * out["loss_G"].item()
    assert abs(out["loss_D"].item() - 0.5 * (out["loss_D1"] + out["loss_D2"]).item()) <= 1e-6
    assert out["fake_B"].shape == out["fake_A"].shape == out["warped_B"].shape == (4, 3, 256, 256)
    assert out["warped_B"].abs().max().item() <= 1.5625 + 1e-5
    assert list(st.gflat.views)[0].startswith("G2.") and list(st.gflat.views)[-1].startswith("G1.")     # gradient-completion order: G2, localiser, G1
    assert torch.isfinite(st.gflat.grad).all() and torch.isfinite(st.dflat.grad).all()
    for flat in (st.gflat, st.dflat):
        for k, v in flat.views.items():
            if any(s in k for s in INERT):
                assert torch.equal(before[k], v), f"{k} moved"
            else:
                assert not torch.equal(before[k], v), f"{k} did not move"
    st2, out2, _ = run(False)
    assert out2["loss_FFT"].item() == 0.0
    assert torch.equal(st2.gflat.grad, st.gflat.grad), "loss_FFT changed a generator-side gradient"
    assert torch.equal(st2.dflat.grad, st.dflat.grad)
    if localiser == "hip":
        st3, out3, _ = run(True)
        assert torch.equal(st3.gflat.grad, st.gflat.grad) and torch.equal(st3.dflat.grad, st.dflat.grad)
        assert torch.equal(st3.gflat.data, st.gflat.data) and torch.equal(out3["loss_G"], out["loss_G"])


def test_darkvisible_step_refuses_bf16x3():
    T.set_compute_dtype("bf16x3")
    with pytest.raises(ValueError, match="bf16x3"):
        T.DarkVisibleStep((3, 256, 256), device=DEV, patch_size=64)
