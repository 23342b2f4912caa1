"""bf16x3 compute mode on the GPU: fp32 storage, convolutions as three bf16 products of split operands (tfc_igemm_kernel<tfc_x3_t>,
tfc_wgrad_x3_kernel).

- every op and pass of the convolution family against float64 on the CPU, normwise relative error <= B (tests/bf16x3_cases.py, checked on the
  arithmetic itself in tests/test_bf16x3_host.py); plain bf16 or a dropped cross term miss B by 10x or more
- the generator against the reference golden and the fp32 oracle with north_star's bar (L1 <= 1e-4)
- the training step against the reference goldens with the fp32 mode's tolerances, its bit determinism, no leakage between modes, full size"""
import numpy as np
import pytest
import torch

import tfc_gan_amd as T
from oracle import tfcgan_oracle as O
from tests import bf16x3_cases as C
from tests.conv_exact import ref_dw, ref_dx, ref_fwd
from tfc_gan_amd import ops
from tfc_gan_amd.ops import DT_BF16X3, OP_CONV3, View

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
X3 = "bf16x3"


def t(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(autouse=True)
def _restore_default():
    yield
    T.set_compute_dtype(torch.bfloat16)


def _view(x_nchw, C_):
    """float NCHW (CPU) -> fp32 NHWC View on the GPU, pitch pad8(C), padding channels zero"""
    N, _, H, W = x_nchw.shape
    buf = torch.zeros((N, H, W, ops.pad8(C_)), dtype=torch.float32, device=DEV)
    buf[..., :C_] = x_nchw.permute(0, 2, 3, 1).to(DEV, torch.float32)
    return View(buf, C_)


def _nchw(v):
    return v.t[..., v.coff:v.coff + v.C].double().cpu().permute(0, 3, 1, 2)


def _randn(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g)


def _check(tag, err):
    print(f"  {tag:44s} rel {err:.3e}  (B {C.B:.3e})")
    assert err <= C.B, (tag, err)


@pytest.mark.parametrize("case", C.CASES, ids=[c.name for c in C.CASES])
def test_conv_family_vs_fp64(case):
    dt = DT_BF16X3
    op, Cin, Cout, H, N = case.op, case.Cin, case.Cout, case.H, case.N
    seed = 100 + Cin + 7 * Cout + op
    x = _randn((N, Cin, H, H), seed)
    w = _randn(C.weight_shape(case), seed + 1)
    if op == OP_CONV3:
        w[:, :, 3, :] = 0
        w[:, :, :, 3] = 0
    x64, w64 = x.double(), w.double()
    y64 = ref_fwd(op, x64, w64)
    OH = y64.shape[2]
    wd = w.to(DEV).contiguous()
    if "f" in case.passes:
        bias = _randn((Cout,), seed + 2) if case.flags in ("bias", "tanh") else None
        want = y64 + (bias.double().view(1, -1, 1, 1) if bias is not None else 0)
        pk = ops.pack_weight(dt, op, 0, wd, Cin, Cout)
        base = _randn(tuple(y64.shape), seed + 3) if case.flags == "accum" else torch.zeros(y64.shape)
        yv = _view(base, Cout)
        stats = torch.zeros((N, Cout, 2), dtype=torch.float32, device=DEV) if case.flags == "stats" else None
        flags = ops.EP_ACCUM if case.flags == "accum" else 0
        ops.conv_fwd(dt, op, _view(x, Cin), Cin, Cout, pk, yv, bias=None if bias is None else bias.to(DEV), stats=stats, flags=flags)
        torch.cuda.synchronize()
        got = _nchw(yv)
        _check(f"{case.name} forward", C.rel(got - base.double(), want))
        if stats is not None:
            g32 = got.float()
            amax = g32.abs().max().item()
            assert torch.allclose(stats[..., 0].cpu(), g32.double().sum((2, 3)).float(), rtol=1e-3, atol=1e-5 * OH * OH * amax)
            assert torch.allclose(stats[..., 1].cpu(), (g32.double() ** 2).sum((2, 3)).float(), rtol=1e-3, atol=1e-5 * OH * OH * amax ** 2)
        if case.flags == "tanh":
            out = torch.full((N, Cout, OH, OH), 7.0, dtype=torch.float32, device=DEV)
            ops.conv_fwd(dt, op, _view(x, Cin), Cin, Cout, pk, None, bias=bias.to(DEV), out_nchw=out)
            torch.cuda.synchronize()
            # tanh is 1-Lipschitz: the pre-activation bound carries over to the stored values
            err = (out.cpu().double() - torch.tanh(want)).norm().item() / want.norm().item()
            _check(f"{case.name} forward, bias + tanh NCHW", err)
            assert torch.isfinite(out).all() and out.abs().max().item() <= 1.0
    if "d" in case.passes:
        dy = _randn(tuple(y64.shape), seed + 4)
        want = ref_dx(op, tuple(x.shape), w64, dy.double())
        base = _randn(tuple(x.shape), seed + 5) if case.flags == "accum" else torch.zeros(x.shape)
        dxv = _view(base, Cin)
        pk1 = ops.pack_weight(dt, op, 1, wd, Cin, Cout)
        ops.conv_dgrad(dt, op, _view(dy, Cout), N, H, H, Cin, Cout, pk1, dxv, accumulate=case.flags == "accum")
        torch.cuda.synchronize()
        _check(f"{case.name} dgrad", C.rel(_nchw(dxv) - base.double(), want))
    if "w" in case.passes:
        dy = _randn(tuple(y64.shape), seed + 6)
        want = ref_dw(op, x64, tuple(w.shape), dy.double())
        dw = torch.full(tuple(w.shape), 3.0, dtype=torch.float32, device=DEV)
        ws = ops.conv_wgrad(dt, op, _view(x, Cin), _view(dy, Cout), Cin, Cout, dw)
        torch.cuda.synchronize()
        _check(f"{case.name} wgrad", C.rel(dw.cpu(), want))
        base = _randn(tuple(w.shape), seed + 7)
        dw2 = base.to(DEV).contiguous()
        ops.conv_wgrad(dt, op, _view(x, Cin), _view(dy, Cout), Cin, Cout, dw2, accumulate=True, ws=ws)
        torch.cuda.synchronize()
        _check(f"{case.name} wgrad, accumulating", C.rel(dw2.cpu().double() - base.double(), want))
        nbytes = ops.lib().tfc_conv_wgrad_ws_bytes(op, Cin, Cout)
        acc = ws[nbytes - ((16 * Cin * Cout * 4 + 255) & ~255):]
        assert not acc.any(), "the weight-gradient accumulator must be left all-zero"


def test_generator_l1_vs_golden(golden):
    """north_star in bf16x3: the assertions of test_generator_l1_vs_golden_fp32 (tests/test_gpu_10_networks.py)"""
    T.set_compute_dtype(X3)
    g = golden("generator_fwd")
    A, _ = O.synthetic_pairs(1, seed=11)
    G = O.init_weights_portable(T.GeneratorUNet((3, 256, 256)), seed=3).to(DEV).eval()
    with torch.no_grad():
        fake = G(A.to(DEV)).cpu()
    assert fake.shape == (1, 3, 256, 256) and fake.dtype == torch.float32
    l1 = (fake[:, :, ::8, ::8] - t(g["fake_sub"])).abs().mean().item()
    print(f"bf16x3 generator L1 vs golden {l1:.3e}")
    assert l1 <= 1e-4, l1
    assert (fake[0, :, 0, :] - t(g["fake_row0"])).abs().max().item() <= 5e-5
    assert abs(fake.abs().mean().item() - float(g["fake_absmean"])) <= 1e-5


def test_generator_batch2_vs_oracle():
    """batch 2 at full resolution against the fp32 oracle: L1 <= 1e-4 (the bf16 mode sits near 5e-3 here)"""
    T.set_compute_dtype(X3)
    A, _ = O.synthetic_pairs(2, seed=12)
    Gc = O.init_weights_portable(O.GeneratorUNet((3, 256, 256)), seed=3).eval()
    with torch.no_grad():
        want = Gc(A)
    G = T.GeneratorUNet((3, 256, 256))
    G.load_state_dict(Gc.state_dict())
    G = G.to(DEV).eval()
    with torch.no_grad():
        got = G(A.to(DEV)).cpu()
    l1 = (got - want).abs().mean().item()
    print(f"bf16x3 generator (batch 2) L1 vs fp32 oracle {l1:.3e}")
    assert l1 <= 1e-4, l1


def test_train_step_vs_reference_golden(golden):
    """_train_step_compare of tests/test_gpu_10_networks.py with the fp32 mode's tolerances, Adam deltas and d_u3 included"""
    g = golden("train_step")
    T.set_compute_dtype(X3)
    G = O.init_weights_portable(T.GeneratorUNet((3, 256, 256)), seed=61).to(DEV).eval()
    D = O.init_weights_portable(T.Discriminator1((3, 256, 256)), seed=62).to(DEV).train()
    gb = {k: v.clone() for k, v in G.state_dict().items()}
    db = {k: v.clone() for k, v in D.state_dict().items()}
    A, B = O.synthetic_pairs(1, seed=63)
    ts = T.TrainStep(G, D, compute_dtype=X3)
    out = ts.step(A.to(DEV), B.to(DEV), neg_idx=g["neg_idx"].tolist())
    torch.cuda.synchronize()
    for k in ("loss_G", "loss_GAN_g", "loss_triplet_patch", "loss_FFT", "loss_D"):
        want = float(g[k])
        print(f"  {k} {float(out[k]):.6g} want {want:.6g}")
        assert abs(float(out[k]) - want) <= 2e-4 * max(1.0, abs(want)), (k, float(out[k]), want)
    l1 = (out["fake_B"].cpu()[:, :, ::8, ::8] - t(g["fake_sub"])).abs().mean().item()
    print(f"  fake_B subsample L1 {l1:.3e}")
    assert l1 <= 1e-4

    def close(got, want, tol=1e-2):
        want = t(want).double()
        rel = ((got.cpu().double() - want).norm() / want.norm()).item()
        print(f"  grad rel-L2 error {rel:.3e} (tol {tol})")
        return rel <= tol

    assert close(ts.gflat.grad_views["down1.model.0.weight"], g["g_grad_down1"])
    assert close(ts.gflat.grad_views["up3.model.0.weight"][::16, ::16], g["g_grad_up3"])
    assert close(ts.dflat.grad_views["model.13.weight"], g["d_grad_head"])
    assert close(ts.dflat.grad_views["model.0.bias"], g["d_grad_b0"])
    assert close(ts.dflat.grad_views["model.3.parametrizations.weight.original"][::8, ::8], g["d_grad_w3"])
    for key, ref in (("final.2.weight", g["g_delta_final_w"]), ("down1.model.0.weight", g["g_delta_down1"])):
        got = (G.state_dict()[key] - gb[key]).cpu()
        assert (got - t(ref)).abs().mean().item() <= 2e-6, key
    got = (D.state_dict()["model.13.weight"] - db["model.13.weight"]).cpu()
    assert (got - t(g["d_delta_head"])).abs().mean().item() <= 2e-6
    assert torch.allclose(D.state_dict()["model.3.parametrizations.weight.0._u"].cpu(), t(g["d_u3"]), atol=1e-4)


def test_glo16_train_step_vs_reference_golden(golden):
    """test_glo16_train_step_fp32_vs_reference_golden's checks in bf16x3"""
    g = golden("train_step_glo16")
    T.set_compute_dtype(X3)
    G = O.init_weights_portable(T.GeneratorUNet((3, 256, 256)), seed=61).to(DEV).eval()
    D = O.init_weights_portable(T.Discriminator1((3, 256, 256)), seed=62).to(DEV).train()
    w0 = G.state_dict()["final.2.weight"].clone()
    A, B = O.synthetic_pairs(1, seed=64)
    ts = T.TrainStep(G, D, compute_dtype=X3, fft_mode="global")
    out = ts.step(A.to(DEV), B.to(DEV), neg_idx=g["neg_idx"].tolist())
    torch.cuda.synchronize()
    for k in ("loss_G", "loss_GAN_g", "loss_triplet_patch", "loss_FFT", "loss_Amp", "loss_Pha", "loss_D"):
        want = float(g[k])
        tol = 5e-4 if k in ("loss_Pha", "loss_FFT") else 2e-4
        assert abs(float(out[k]) - want) <= tol * max(1.0, abs(want)), (k, float(out[k]), want)
    assert (out["fake_B"].cpu()[:, :, ::8, ::8] - t(g["fake_sub"])).abs().mean().item() <= 1e-4
    want = t(g["g_grad_down1"]).double()
    rel = ((ts.gflat.grad_views["down1.model.0.weight"].cpu().double() - want).norm() / want.norm()).item()
    assert rel <= 1e-2, rel
    got = (G.state_dict()["final.2.weight"] - w0).cpu()
    assert (got - t(g["g_delta_final_w"])).abs().mean().item() <= 2e-6


def test_step_is_bit_deterministic_on_one_and_two_streams():
    """test_step_is_bit_deterministic_on_one_and_two_streams in bf16x3: no float atomics (the weight gradients reduce fixed-order slabs)"""
    T.set_compute_dtype(X3)
    runs = []
    prev = T.set_wgrad_stream(True)
    try:
        for on in (True, True, False):
            T.set_wgrad_stream(on)
            G = O.init_weights_portable(T.GeneratorUNet((3, 256, 256)), seed=71).to(DEV)
            D = O.init_weights_portable(T.Discriminator1((3, 256, 256)), seed=72).to(DEV)
            A, B = O.synthetic_pairs(2, seed=73)
            A, B = A.to(DEV), B.to(DEV)
            ts = T.TrainStep(G, D, compute_dtype=X3)
            ts.step(A, B)
            out2 = ts.step(A, B)
            torch.cuda.synchronize()
            runs.append({"g_grad": ts.gflat.grad.clone(), "d_grad": ts.dflat.grad.clone(), "g_w": ts.gflat.data.clone(), "d_w": ts.dflat.data.clone(),
                         "fake": out2["fake_B"].clone(), "sn": torch.cat([b.flatten() for b in ts.dbufs.values()]).clone(),
                         "losses": torch.stack([out2[k].reshape(()).float() for k in sorted(out2) if k != "fake_B"]).clone()})
    finally:
        T.set_wgrad_stream(prev)
    ref = runs[0]
    assert torch.isfinite(ref["g_grad"]).all() and ref["g_grad"].abs().max().item() > 0 and ref["d_grad"].abs().max().item() > 0
    for what, other in (("two streams, run to run", runs[1]), ("two streams vs one stream", runs[2])):
        for k in ref:
            assert torch.equal(ref[k], other[k]), (what, k, (ref[k].double() - other[k].double()).abs().max().item())


def _module_run(mod, xs, go):
    xs = [x.clone().requires_grad_(True) for x in xs]
    mod.zero_grad(set_to_none=True)
    y = mod(*xs)
    y.backward(go)
    return [y.detach().clone()] + [x.grad.clone() for x in xs] + [p.grad.clone() for p in mod.parameters()]


@pytest.mark.parametrize("other", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_no_leakage_between_modes(other):
    """forward + backward of UNetDown / UNetUp / GeneratorUNet in `other`, then bf16x3, then `other` again in one process: the two `other` runs are
    torch.equal (operand streams and pack caches do not bleed between modes), and the bf16x3 run really differs from them"""
    torch.manual_seed(5)
    down = O.init_weights_portable(T.UNetDown(64, 128), 21).to(DEV).eval()
    up = O.init_weights_portable(T.UNetUp(128, 64), 23).to(DEV).eval()
    x_d = torch.randn(2, 64, 32, 32, device=DEV)
    x_u, skip = torch.randn(2, 128, 15, 15, device=DEV), torch.randn(2, 64, 30, 30, device=DEV)
    G = O.init_weights_portable(T.GeneratorUNet((3, 256, 256)), seed=3).to(DEV).eval()
    A, _ = O.synthetic_pairs(1, seed=11)
    A = A.to(DEV)
    results = []
    for mode in (other, X3, other):
        T.set_compute_dtype(mode)
        r = []
        yd = down(x_d)
        r += _module_run(down, [x_d], torch.ones_like(yd) * 0.01)
        yu = up(x_u, skip)
        r += _module_run(up, [x_u, skip], torch.ones_like(yu) * 0.01)
        G.compute_dtype = mode
        with torch.no_grad():
            r.append(G(A).clone())
        torch.cuda.synchronize()
        results.append(r)
    a, x3, b = results
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), i
    assert not torch.equal(a[0].float(), x3[0].float())


def test_full_size_batch32_and_stn21_refusal():
    """a batch-32 PATCH-16 step and a batch-32 GLO-16 step at 256 x 256 give finite losses; STN21Step and the HIP ViT refuse the mode"""
    T.set_compute_dtype(X3)
    N = 32
    A, B = O.synthetic_pairs(N, seed=99)
    A, B = A.to(DEV), B.to(DEV)
    for fft_mode in ("patch", "global"):
        torch.manual_seed(0)
        G = T.GeneratorUNet((3, 256, 256)).to(DEV)
        D = T.Discriminator1((3, 256, 256)).to(DEV)
        G.apply(T.weights_init_normal)
        D.apply(T.weights_init_normal)
        ts = T.TrainStep(G, D, compute_dtype=X3, fft_mode=fft_mode)
        out = ts.step(A, B)
        torch.cuda.synchronize()
        fake = out["fake_B"]
        assert fake.shape == (N, 3, 256, 256) and torch.isfinite(fake).all()
        for k, v in out.items():
            if k != "fake_B":
                assert np.isfinite(float(v)), (fft_mode, k)
        del ts, G, D
    with pytest.raises(ValueError, match="bf16x3"):
        T.STN21Step(device=DEV)
    from tfc_gan_amd import vit
    with pytest.raises(ValueError, match="bf16x3"):
        vit._dt()
