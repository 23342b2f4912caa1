"""GPU tests of the edge-mask configuration MASK-4 (TFCGAN_multigpu_patchFFT_experiment.py "4X"): the mask operator of csrc/mask.hip forward and
backward against the fp64 restatement tests/mask_ref.py, the plane packer, and TrainStep(patches=4, mask=True) against the fixture lifted from the
script (tests/golden/make_golden_mask.py).

Tolerances of the operator: 8x the error the SAME restatement run in fp32 on the CPU shows against fp64 for that input (computed here, printed; the
factor allows for a different summation order). The backward of this operator puts a single-pixel spike on the argmin of |laplacian| (and on the
argmax, and on the argmax of the blurred plane); two correct fp32 implementations agree on those positions only when the extremum is separated from
its runner-up by more than their round-off, so every case first asserts, from the restatement, that it is (the seeds were chosen so), or makes the
ties exact (a block of zeros; two identical samples). Nothing is skipped or widened around it.
"""
import functools

import numpy as np
import pytest
import torch

import tfc_gan_amd as T
from oracle import tfcgan_oracle as O
from tests import mask_ref as R
from tfc_gan_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (N, H, W), seed, a 24 x 24 block of exact zeros (mn = 0 with 18 x 18 exact ties per sample, sign = 0 there: saturated flat regions)
CASES = {"n1_8x8": ((1, 8, 8), 0, False),            # smaller than any tile; both reflect folds hit the same pixels
         "n3_19x37": ((3, 19, 37), 2, False),        # odd and ragged
         "n1_70x130": ((1, 70, 130), 2, False),      # several tiles with remainders both ways
         "n2_256x256": ((2, 256, 256), 0, True)}     # the product's shape
SMALL = ("n1_8x8", "n3_19x37", "n1_70x130")


def rel_l2(got, want):
    want = want.double()
    return ((got.double() - want).norm() / want.norm()).item()


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs and references of one case, computed once: fp64 forward / backward of the restatement, and the fp32-CPU error of each against fp64"""
    (N, H, W), seed, zeros = CASES[name]
    g = torch.Generator().manual_seed(seed)
    img = torch.tanh(torch.randn(N, 3, H, W, generator=g))
    dout = torch.randn(N, 1, H, W, generator=g)
    if zeros:
        img[:, :, 100:124, 60:84] = 0
    parts = R.mask_parts(img.double())
    L, Bl = parts["L"].flatten().sort().values, parts["Bl"].flatten().sort().values
    m64, g64 = parts["mask"], R.mask_vjp(img.double(), dout.double())
    m32, g32 = R.mask_maker(img), R.mask_vjp(img, dout)
    return {"img": img, "dout": dout, "mask64": m64, "grad64": g64, "L": L, "Bl": Bl, "zeros": zeros,
            "err_fwd": (m32.double() - m64).abs().max().item(), "err_bwd": rel_l2(g32, g64)}


def assert_separated(c, small):
    """the two largest |lap| and the two largest blurred values differ by more than 1e-4 relative; at the small shapes the smallest |lap| and its gap
    to the next exceed 1e-5 (at 256 x 256 the minimum is an exact 0 attained on the block of zeros)"""
    L, Bl = c["L"], c["Bl"]
    assert (L[-1] - L[-2]) / L[-1] > 1e-4 and (Bl[-1] - Bl[-2]) / Bl[-1] > 1e-4
    if small:
        assert L[0] > 1e-5 and L[1] - L[0] > 1e-5
    else:
        assert c["zeros"] and L[0] == 0 and (L == 0).sum() >= 2 * 18 * 18


# ---- the operator ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_mask_forward_vs_fp64_restatement(name):
    c = case(name)
    assert_separated(c, name in SMALL)
    got = T.mask_maker(c["img"].to(DEV)).cpu()
    err = (got.double() - c["mask64"]).abs().max().item()
    print(f"  {name}: forward max-abs error {err:.3e} (fp32 CPU restatement {c['err_fwd']:.3e}, tol 8x)")
    assert got.shape == c["mask64"].shape and got.dtype == torch.float32
    assert err <= 8 * c["err_fwd"]
    assert got.max().item() == 1.0                                  # Bl / max(Bl)


@pytest.mark.parametrize("name", list(CASES))
def test_mask_backward_random_upstream_vs_fp64_autograd(name):
    """a random upstream gradient (no L1 sign in the way) through the extrema, the abs, both adjoints and the grayscale transpose"""
    c = case(name)
    assert_separated(c, name in SMALL)
    ctx = ops.mask_fwd(c["img"].to(DEV))
    got = ops.mask_bwd(ctx, dout=c["dout"].to(DEV)).cpu()
    err = rel_l2(got, c["grad64"])
    print(f"  {name}: backward rel-L2 error {err:.3e} (fp32 CPU restatement {c['err_bwd']:.3e}, tol 8x)")
    assert err <= 8 * c["err_bwd"]
    if c["zeros"]:                                                  # mn = 0 on the zero block: ties counted, sign(0) = 0 keeps d/dmn off it
        assert ctx.ws[0].item() == 0.0 and ctx.ws[2].item() == float((c["L"] == 0).sum())


def test_mask_operator_matches_the_lifted_reference_fixture(golden):
    """the same kernels against the outputs of the script's own mask_maker (lifted, on the kornia stand-in, in double) and autograd through it"""
    g = golden("mask_maker")
    for name in ("n1_8x8", "n3_19x37"):
        c = case(name)
        assert np.abs(c["mask64"].numpy() - g[f"mask_{name}"]).max() <= 1e-12          # the restatement IS what the fixture was made from
        ctx = ops.mask_fwd(c["img"].to(DEV))
        got_m, got_g = ops.mask_scale(ctx).cpu(), ops.mask_bwd(ctx, dout=c["dout"].to(DEV)).cpu()
        assert (got_m.double() - torch.as_tensor(g[f"mask_{name}"])).abs().max().item() <= 8 * c["err_fwd"]
        assert rel_l2(got_g, torch.as_tensor(g[f"grad_{name}"])) <= 8 * c["err_bwd"]


def test_mask_ties_split_evenly():
    """two identical samples in one batch: every extremum is attained twice, the gradient through it must be autograd's even split"""
    c = case("n3_19x37")
    img = torch.cat([c["img"][:1], c["img"][:1]])
    dout = torch.cat([c["dout"][:1], c["dout"][1:2]])               # different upstream gradients on the two copies
    parts = R.mask_parts(img.double())
    L, Bl = parts["L"].flatten().sort().values, parts["Bl"].flatten().sort().values
    assert L[0] == L[1] and L[-1] == L[-2] and Bl[-1] == Bl[-2]     # exact ties in the reference
    assert L[2] - L[1] > 1e-5 and (L[-2] - L[-3]) / L[-1] > 1e-4 and (Bl[-2] - Bl[-3]) / Bl[-1] > 1e-4
    g64 = R.mask_vjp(img.double(), dout.double())
    err32 = rel_l2(R.mask_vjp(img, dout), g64)
    ctx = ops.mask_fwd(img.to(DEV))
    got = ops.mask_bwd(ctx, dout=dout.to(DEV)).cpu()
    err = rel_l2(got, g64)
    print(f"  ties: backward rel-L2 error {err:.3e} (fp32 CPU restatement {err32:.3e}, tol 8x); tie counts {ctx.ws[2:6].tolist()}")
    assert ctx.ws[2].item() == 2.0 and ctx.ws[3].item() == 2.0 and ctx.ws[5].item() == 2.0
    assert err <= 8 * err32
    # without the split (the whole d/dM, d/dmx, d/dmn on each copy) the error is of order one: the bound above would not hold
    same = ops.mask_bwd(ops.mask_fwd(img.to(DEV)), dout=torch.cat([dout[:1], dout[:1]]).to(DEV)).cpu()
    assert torch.equal(same[0], same[1])


@pytest.mark.parametrize("name", SMALL)
def test_mask_l1_loss_and_gradient(name):
    """scale * mean|mask(fake) - mask(real)| and its gradient. The loss differs from fp64 by at most the sum of the two masks' forward errors, each
    held to 8x its fp32-CPU error above (plus the rounding of the result). The gradient is compared in relative L2 at 8x the fp32-CPU error: a sign
    flip at a near-zero difference would move one pixel, and the case asserts that no difference is that near zero."""
    c = case(name)
    (N, H, W), seed, _ = CASES[name]
    real = torch.tanh(torch.randn(N, 3, H, W, generator=torch.Generator().manual_seed(seed + 107)))      # chosen so that the assertion below holds
    scale = 0.5
    m_f, m_r = c["mask64"], R.mask_maker(real.double())
    assert (m_f - m_r).abs().min().item() > 1e-5
    err_r = (R.mask_maker(real).double() - m_r).abs().max().item()
    loss64, grad64 = R.mask_l1_grad(c["img"].double(), real.double(), scale)
    _, grad32 = R.mask_l1_grad(c["img"], real, scale)
    err32 = rel_l2(grad32, grad64)
    loss, grad = T.mask_l1_loss(c["img"].to(DEV), real.to(DEV), scale=scale)
    tol_loss = scale * 8 * (c["err_fwd"] + err_r) + 2.0 ** -22 * loss64.item()
    err = rel_l2(grad.cpu(), grad64)
    print(f"  {name}: loss {loss.item():.8g} (fp64 {loss64.item():.8g}, tol {tol_loss:.2e}); gradient rel-L2 error {err:.3e} (fp32 CPU {err32:.3e}, tol 8x)")
    assert abs(loss.item() - loss64.item()) <= tol_loss
    assert err <= 8 * err32
    only, none = T.mask_l1_loss(c["img"].to(DEV), real.to(DEV), scale=scale, want_grad=False)
    assert none is None and torch.equal(only, loss)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_pack_nhwc8_plane_vs_torch(dtype):
    dt = ops.dt_of(dtype)
    for (N, H, W) in ((2, 10, 18), (1, 64, 64)):
        g = torch.Generator().manual_seed(7)
        x, plane = torch.randn(N, 3, H, W, generator=g).to(DEV), torch.rand(N, 1, H, W, generator=g).to(DEV)
        div = torch.tensor([0.73], device=DEV)
        for d in (None, div):
            p = plane if d is None else plane / d
            want = torch.cat([x, p, torch.zeros(N, 4, H, W, device=DEV)], 1).permute(0, 2, 3, 1).contiguous().to(dtype)
            got = ops.pack_nhwc8_plane(dt, x, plane, d)
            assert got.t.dtype == dtype and tuple(got.t.shape) == (N, H, W, 8)
            assert torch.equal(got.t, want)
    with pytest.raises(T.TfcError):
        ops.pack_nhwc8_plane(dt, x, plane[:, :, :-1])


def test_mask_is_bit_reproducible():
    c = case("n2_256x256")
    img, dout = c["img"].to(DEV), c["dout"].to(DEV)
    runs = []
    for _ in range(2):
        ctx = ops.mask_fwd(img)
        runs.append((ops.mask_scale(ctx), ops.mask_bwd(ctx, dout=dout), T.mask_l1_loss(img, img.flip(0))))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][2][0], runs[1][2][0]) and torch.equal(runs[0][2][1], runs[1][2][1])


def test_mask_argument_checks_return_errors_without_launching():
    lib = ops.lib()
    assert lib.tfc_mask_ws_bytes(1, 7, 8) == 0 and lib.tfc_mask_ws_bytes(1, 8, 7) == 0 and lib.tfc_mask_ws_bytes(0, 8, 8) == 0
    assert lib.tfc_mask_ws_bytes(2, 256, 256) == 64 + 16 * 2 * 16 * 4
    img = torch.zeros(1, 3, 8, 8, device=DEV)
    lap, bl, ws = torch.full((64,), 5.0, device=DEV), torch.full((64,), 5.0, device=DEV), torch.zeros(64, device=DEV)
    s = ops.stream_ptr()
    for (N, H, W) in ((1, 7, 8), (1, 8, 7), (0, 8, 8), (70000, 8, 8)):
        assert lib.tfc_mask_fwd(s, img.data_ptr(), lap.data_ptr(), bl.data_ptr(), ws.data_ptr(), N, H, W) != 0
    assert lib.tfc_mask_fwd(s, img.data_ptr() + 4, lap.data_ptr(), bl.data_ptr(), ws.data_ptr(), 1, 8, 8) != 0     # misaligned
    assert lib.tfc_mask_fwd(s, img.data_ptr(), None, bl.data_ptr(), ws.data_ptr(), 1, 8, 8) != 0
    assert lib.tfc_mask_bwd(s, lap.data_ptr(), bl.data_ptr(), ws.data_ptr(), None, None, 1.0, None, None, None, 1, 8, 8) != 0     # neither dout nor ref
    assert lib.tfc_mask_bwd(s, lap.data_ptr(), bl.data_ptr(), ws.data_ptr(), lap.data_ptr(), lap.data_ptr(), 1.0, None, None, None, 1, 8, 8) != 0   # both
    assert lib.tfc_mask_bwd(s, lap.data_ptr(), bl.data_ptr(), ws.data_ptr(), lap.data_ptr(), None, 1.0, None, None, None, 1, 8, 8) != 0   # nothing to do
    assert lib.tfc_pack_nhwc8_plane(s, 7, img.data_ptr(), lap.data_ptr(), None, ws.data_ptr(), 1, 8, 8) != 0
    assert lib.tfc_pack_nhwc8_plane(s, 0, img.data_ptr(), lap.data_ptr(), None, ws.data_ptr(), 1, 3, 3) != 0       # H*W % 4
    torch.cuda.synchronize()
    assert bool((lap == 5.0).all()) and bool((bl == 5.0).all()) and not ws.any()          # nothing ran
    with pytest.raises(T.TfcError, match="H, W >= 8"):
        T.mask_maker(torch.zeros(1, 3, 7, 9, device=DEV))
    with pytest.raises(T.TfcError, match="forward-only"):
        T.mask_maker(torch.zeros(1, 3, 8, 8, device=DEV, requires_grad=True))
    with pytest.raises(T.TfcError):
        ops.mask_bwd(ops.mask_fwd(torch.rand(1, 3, 8, 8, device=DEV)), dout=torch.zeros(1, 1, 8, 9, device=DEV))


# ---- the step -------------------------------------------------------------------------------------------------------------------------------------
def mask_nets(seed_g=61, seed_d=62):
    G = O.init_weights_portable(T.GeneratorUNet((3, 256, 256), mask=True), seed=seed_g).to(DEV).eval()
    D = O.init_weights_portable(T.Discriminator1((3, 256, 256)), seed=seed_d).to(DEV).train()
    return G, D


def t(a):
    return torch.as_tensor(np.asarray(a))


def close(got, want, tol=1e-2):
    want = t(want).double()
    r = ((got.cpu().double() - want).norm() / want.norm()).item()
    print(f"  grad rel-L2 error {r:.3e} (tol {tol})")
    return r <= tol


LOG_KEYS = {"loss_G", "loss_GAN_g", "loss_triplet_patch", "loss_FFT", "loss_Amp", "loss_Pha", "loss_D", "fake_B", "loss_mask"}


def run_step(dtype, lambda_mask, g=None, extra=None, nets=None):
    T.set_compute_dtype(dtype)
    try:
        G, D = nets or mask_nets()
        before = ({k: v.clone() for k, v in G.state_dict().items()}, {k: v.clone() for k, v in D.state_dict().items()})
        A, B = O.synthetic_pairs(2, seed=465)
        kw = dict(T.mask_weights(), lambda_mask=lambda_mask)
        ts = T.TrainStep(G, D, compute_dtype=dtype, patches=4, mask=True, **kw)
        out = ts.step(A.to(DEV), B.to(DEV), neg_idx=[3, 0, 2, 1] if g is None else g["neg_idx"].tolist(), extra_loss_G=extra)
        torch.cuda.synchronize()
    finally:
        T.set_compute_dtype(torch.bfloat16)
    return G, D, ts, out, before


def test_mask4_train_step_fp32_run_a_vs_reference_golden(golden):
    """run (a) of the fixture (the mask feeds G, its loss term weighted 0) in fp32 compute mode: the checks and tolerances of
    test_patch4_train_step_fp32_vs_reference_golden (losses 2e-4, gradient tensors 1e-2 relative L2, Adam deltas 2e-6, u). Pins the mask-fed
    4-channel generator end to end; robust because only the VALUES of the extrema reach it."""
    g = golden("train_step_mask4")
    G, D, ts, out, (gb, db) = run_step(torch.float32, 0.0, g)
    assert set(out) == LOG_KEYS
    for k in ("loss_G", "loss_GAN_g", "loss_triplet_patch", "loss_FFT", "loss_D"):
        want = float(g[k])
        print(f"  {k}: {float(out[k]):.7g} (reference {want:.7g})")
        assert abs(float(out[k]) - want) <= 2e-4 * max(1.0, abs(want)), (k, float(out[k]), want)
    assert float(out["loss_mask"]) == 0.0                           # the term is switched off, not computed
    assert (out["fake_B"].cpu()[:, :, ::8, ::8] - t(g["fake_sub"])).abs().mean().item() <= 1e-4
    assert close(ts.gflat.grad_views["down1.model.0.weight"], g["g_grad_down1"])          # all 4 input channels
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


def test_mask4_train_step_fp32_run_b_vs_reference_golden(golden):
    """run (b): the script's 0.5 * loss_mask. Every loss including loss_mask at 2e-4, fake, and the discriminator's gradients and update (the
    generator's gradients of this run carry the argmin spike and are pinned by the wiring test below instead)"""
    g = golden("train_step_mask4")
    G, D, ts, out, (gb, db) = run_step(torch.float32, 0.5, g)
    assert set(out) == LOG_KEYS
    for k in ("loss_G", "loss_GAN_g", "loss_triplet_patch", "loss_FFT", "loss_mask", "loss_D"):
        want = float(g["b_" + k])
        print(f"  {k}: {float(out[k]):.7g} (reference {want:.7g})")
        assert abs(float(out[k]) - want) <= 2e-4 * max(1.0, abs(want)), (k, float(out[k]), want)
    assert (out["fake_B"].cpu()[:, :, ::8, ::8] - t(g["b_fake_sub"])).abs().mean().item() <= 1e-4
    assert close(ts.dflat.grad_views["model.13.weight"], g["b_d_grad_head"])
    assert close(ts.dflat.grad_views["model.0.bias"], g["b_d_grad_b0"])
    assert close(ts.dflat.grad_views["model.3.parametrizations.weight.original"][::8, ::8], g["b_d_grad_w3"])
    got = (D.state_dict()["model.13.weight"] - db["model.13.weight"]).cpu()
    assert (got - t(g["b_d_delta_head"])).abs().mean().item() <= 2e-6
    assert torch.allclose(D.state_dict()["model.3.parametrizations.weight.0._u"].cpu(), t(g["b_d_u3"]), atol=1e-4)


def test_mask4_gradient_wiring_against_the_pluggable_term():
    """the step's own mask term against the same kernels plugged in as extra_loss_G from the same state: the two differ only in the order of two
    additions into the gradient of fake. No cross-implementation argmin agreement is needed. And the term must reach the generator at all."""
    _, _, ts1, out1, _ = run_step(torch.float32, 0.5)
    _, _, ts2, out2, _ = run_step(torch.float32, 0.0, extra=lambda f, b: T.mask_l1_loss(f, b, scale=0.5))
    _, _, ts3, out3, _ = run_step(torch.float32, 0.0)
    assert torch.equal(out1["fake_B"], out2["fake_B"]) and torch.equal(out1["fake_B"], out3["fake_B"])
    lg1, lg2 = float(out1["loss_G"]), float(out2["loss_G"])
    assert abs(lg1 - lg2) <= 1e-6 * abs(lg1), (lg1, lg2)
    assert abs(float(out1["loss_mask"]) * 0.5 - float(out2["loss_extra_g"])) <= 1e-7
    r12 = rel_l2(ts2.gflat.grad, ts1.gflat.grad)
    print(f"  own term vs plugged term: generator gradient rel-L2 difference {r12:.3e}")
    assert r12 <= 1e-6
    moved = {k: rel_l2(ts1.gflat.grad_views[k], ts3.gflat.grad_views[k]) for k in ("down1.model.0.weight", "up3.model.0.weight", "final.2.weight")}
    print(f"  with vs without the term: {moved}")
    assert max(moved.values()) > 1e-3


@pytest.mark.parametrize("dtype", [torch.bfloat16, "bf16x3"])
def test_mask4_train_step_bf16_losses(golden, dtype):
    """run (b) in the bf16 and bf16x3 compute modes: losses within the project's bf16 step bound (3e-2 relative). The mask kernels are fp32 in every
    mode; what varies is the generated image they are applied to."""
    g = golden("train_step_mask4")
    _, _, ts, out, _ = run_step(dtype, 0.5, g)
    for k in ("loss_G", "loss_GAN_g", "loss_triplet_patch", "loss_FFT", "loss_mask", "loss_D"):
        want = float(g["b_" + k])
        print(f"  {k}: {float(out[k]):.7g} (reference {want:.7g})")
        assert abs(float(out[k]) - want) <= 3e-2 * max(1.0, abs(want)), (k, float(out[k]), want)
    assert torch.isfinite(ts.gflat.grad).all() and ts.gflat.grad.abs().max().item() > 0


def test_mask4_step_is_bit_deterministic_on_one_and_two_streams():
    """two MASK-4 steps from the same state (bf16, N = 2): the same bits run to run on two streams and against the one-stream schedule, in every
    parameter, gradient and loss"""
    runs = []
    prev = T.set_wgrad_stream(True)
    try:
        for on in (True, True, False):
            T.set_wgrad_stream(on)
            G, D = mask_nets(71, 72)
            A, B = O.synthetic_pairs(2, seed=73)
            A, B = A.to(DEV), B.to(DEV)
            ts = T.TrainStep(G, D, compute_dtype=torch.bfloat16, patches=4, mask=True, **T.mask_weights())
            ts.step(A, B)
            out2 = ts.step(A, B)
            torch.cuda.synchronize()
            runs.append({"g_w": ts.gflat.data.clone(), "d_w": ts.dflat.data.clone(), "g_grad": ts.gflat.grad.clone(), "d_grad": ts.dflat.grad.clone(),
                         "fake": out2["fake_B"].clone(),
                         "losses": torch.stack([out2[k].reshape(()).float() for k in sorted(out2) if out2[k].numel() == 1]).clone()})
    finally:
        T.set_wgrad_stream(prev)
    ref = runs[0]
    assert torch.isfinite(ref["losses"]).all() and ref["g_grad"].abs().max().item() > 0
    for what, other in (("two streams, run to run", runs[1]), ("two streams vs one stream", runs[2])):
        for k in ref:
            assert torch.equal(ref[k], other[k]), (what, k)


def test_mask_generator_forward_and_refusals(golden):
    g = golden("mask_maker")
    G, D = mask_nets()
    assert list(G.state_dict().keys()) == list(g["g_keys"]) and tuple(G.down1.model[0].weight.shape) == (64, 4, 4, 4)
    A, B = O.synthetic_pairs(2, seed=465)
    A = A.to(DEV)
    T.set_compute_dtype(torch.float32)
    try:
        with torch.no_grad():
            mask_A = T.mask_maker(A)
            fake = G(A, mask_A)
        err32 = (R.mask_maker(A.cpu()).double() - R.mask_maker(A.cpu().double())).abs().max().item()
        assert (mask_A.cpu()[:, :, ::4, ::4].double() - t(g["mask_A_sub"])).abs().max().item() <= 8 * err32
        run = golden("train_step_mask4")
        assert (fake.cpu()[:, :, ::8, ::8] - t(run["fake_sub"])).abs().mean().item() <= 1e-4
        with pytest.raises(T.TfcError, match="TrainStep"):
            G(A, mask_A)                                            # under autograd
        with torch.no_grad(), pytest.raises(T.TfcError, match="mask_A"):
            G(A)
        plain = T.GeneratorUNet((3, 256, 256)).to(DEV)
        with torch.no_grad(), pytest.raises(T.TfcError, match="mask=True"):
            plain(A, mask_A=mask_A)
    finally:
        T.set_compute_dtype(torch.bfloat16)
    # TrainStep's refusals
    plain_G = T.GeneratorUNet((3, 256, 256)).to(DEV)
    lab_G = T.GeneratorUNet((3, 256, 256), labels=3).to(DEV)
    lab_D = T.Discriminator1((3, 256, 256), aux_classes=(2, 4, 3)).to(DEV)
    for bad in (lambda: T.TrainStep(G, D, patches=16, mask=True), lambda: T.TrainStep(plain_G, D, patches=4, mask=True),
                lambda: T.TrainStep(G, D, patches=4), lambda: T.TrainStep(lab_G, lab_D, patches=4, mask=True, labels="real"),
                lambda: T.TrainStep(G, D, patches=4, mask=True, batch_invariant=True)):
        with pytest.raises(T.TfcError):
            bad()
    with pytest.raises(T.TfcError, match="mutually exclusive"):
        T.GeneratorUNet((3, 256, 256), labels=3, mask=True)
