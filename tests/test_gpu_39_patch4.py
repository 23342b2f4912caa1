"""GPU tests of the 4-patch configurations PATCH-4 / GLO-4 (TFCGAN_multigpu_patchFFT.py = "4P", TFCGAN_multigpu_globalFFT.py = "4G"): the triplet head on
the 2x2 grid of 128x128 patches (tfc_patch_triplet, grid 2), the S = 128 spectra (128-point LDS FFT with a radix-2 last pass, and the direct DFT that
cross-checks it) and TrainStep(patches=4), against tests/patch4_ref.py and the fixtures of tests/golden/make_golden_patch4.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import tfc_gan_amd as T
from oracle import tfcgan_oracle as O
from tests import patch4_ref as R4
from tfc_gan_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEG = [2, 1, 0, 2]                                                  # the fixture's indices (r_k == k at k = 1)


def t(a):
    return torch.from_numpy(np.asarray(a))


@functools.lru_cache(maxsize=None)
def triplet_case():
    """inputs at N = 3 (N = 1: sample 0) and, per N, the CPU fp32 loss / gradient plus the float64 restatement of the same formula"""
    fk, rl = O.synthetic_pairs(3, seed=431)
    fk = torch.tanh(fk * 1.5)
    ref = {}
    for n in (1, 3):
        out = []
        for dtype in (None, torch.float64):
            f = fk[:n].clone().requires_grad_(True)
            loss = R4.patch_triplet_loss(f, rl[:n], NEG, dtype=dtype)
            loss.backward()
            out += [loss.detach(), f.grad if dtype is None else f.grad.double()]
        ref[n] = out
    return fk, rl, ref


# ---- triplet head ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 3])
def test_triplet4_vs_ref_and_golden(golden, N):
    """N = 1: 1536 rows in 384 workgroups, four rows in flight per wave -> the unrolled row slots 1..3 lie past the end. N = 3: 4608 rows on the
    512-workgroup cap -> second trip of the grid-stride loop with a ragged tail. Tolerances of test_triplet16_vs_oracle_and_golden.
    (Against a float64 restatement: see the printed errors -- the GPU's 128-term row sums are no further from it than torch's CPU fp32 ones.)"""
    g = golden("triplet4")
    assert g["neg_idx"].tolist() == NEG
    fk, rl, ref = triplet_case()
    want, wgrad, want64, wgrad64 = ref[N]
    loss, dfake = ops.patch_triplet(fk[:N].to(DEV), rl[:N].to(DEV), NEG)
    got = dfake.cpu()
    print(f"N={N}: |loss - f64| gpu {abs(loss.item() - want64.item()):.3e} cpu-fp32 {abs(want.item() - want64.item()):.3e};  "
          f"max|grad - f64| gpu {(got.double() - wgrad64).abs().max().item():.3e} cpu-fp32 {(wgrad.double() - wgrad64).abs().max().item():.3e} "
          f"(max|g| {wgrad.abs().max().item():.3e})")
    tag = "n1" if N == 1 else "n3"
    assert abs(loss.item() - float(g["loss_" + tag])) < 2e-6 and abs(loss.item() - want.item()) < 2e-6
    assert (got - wgrad).abs().max().item() < 1e-9 + 1e-5 * wgrad.abs().max().item()
    assert torch.allclose(got[:, :, ::4, ::4], t(g["gfake_sub_" + tag]), atol=1e-9, rtol=1e-4)


def test_triplet4_properties_and_surface():
    fk, rl, ref = triplet_case()
    f3, r3 = fk.to(DEV), rl.to(DEV)
    # r_k == k for every k: each hinge is exactly the margin and the gradient vanishes (and IS written: the buffer starts as garbage)
    l1, d1 = ops.patch_triplet(f3, r3, [0, 1, 2, 3])
    assert abs(l1.item() - 1.0) < 1e-6 and d1.abs().max().item() == 0.0
    # grid 4 through the new entry point IS the 16-patch kernel
    neg16 = [3, 3, 7, 0, 4, 9, 15, 2, 8, 8, 1, 12, 5, 13, 6, 10]
    l16, d16 = ops.patch16_triplet(f3, r3, neg16)
    l4, d4 = ops.patch_triplet(f3, r3, neg16)
    assert torch.equal(l16, l4) and torch.equal(d16, d4)
    # no gradient asked for
    l0, d0 = ops.patch_triplet(f3, r3, NEG, want_grad=False)
    assert d0 is None and abs(l0.item() - ref[3][0].item()) < 2e-6
    # autograd surface
    f2 = f3.clone().requires_grad_(True)
    T.ContrastiveLoss(patches=4)(f2, r3, NEG).backward()
    assert torch.allclose(f2.grad.cpu(), ref[3][1], atol=1e-9, rtol=1e-4)
    f2 = f3.clone().requires_grad_(True)
    T.patch_triplet_loss(f2, r3, NEG).backward()
    assert torch.allclose(f2.grad.cpu(), ref[3][1], atol=1e-9, rtol=1e-4)
    drawn = T.ContrastiveLoss(patches=4)(f3, r3)                   # np.random.randint(4) per patch, as 4P:477-480
    assert np.isfinite(drawn.item())
    # three-tensor form on 128 x 128 patches = nn.TripletMarginLoss on one patch
    a, p, n = (x[:2].contiguous() for x in (T.make_4_patches(f3)[0], T.make_4_patches(r3)[0], T.make_4_patches(r3)[3]))
    a = a.clone().requires_grad_(True)
    got = T.ContrastiveLoss()(a, p, n)
    got.backward()
    ac = a.detach().cpu().requires_grad_(True)
    want = torch.nn.TripletMarginLoss(margin=1.0, p=2)(ac, p.cpu(), n.cpu())
    want.backward()
    assert abs(got.item() - want.item()) < 1e-5                    # total * 4 - 3: four times the 2e-6 of the head, plus the subtraction
    assert torch.allclose(a.grad.cpu(), ac.grad, atol=1e-9, rtol=1e-4)
    # the same form on 64 x 64 patches (the 16-patch kernel, total * 16 - 15): the gradient reaches the anchor there too
    a, p, n = (x[:2].contiguous() for x in (T.make_16_patches(f3)[0], T.make_16_patches(r3)[0], T.make_16_patches(r3)[9]))
    a = a.clone().requires_grad_(True)
    got = T.ContrastiveLoss()(a, p, n)
    got.backward()
    ac = a.detach().cpu().requires_grad_(True)
    want = torch.nn.TripletMarginLoss(margin=1.0, p=2)(ac, p.cpu(), n.cpu())
    want.backward()
    assert abs(got.item() - want.item()) < 4e-5                    # sixteen times the 2e-6 of the head, plus the subtraction
    assert a.grad is not None and torch.allclose(a.grad.cpu(), ac.grad, atol=1e-9, rtol=1e-4)


def test_triplet4_sample0_bits_do_not_depend_on_the_batch():
    """dfake of sample 0 at N = 3 against dfake of that sample alone, torch.equal. The loss is a batch MEAN, so the N = 3 gradient carries a factor
    1/3 that the N = 1 gradient does not; the N = 3 call therefore passes gscale = 3, and the kernel's single factor gscale / (4 N C 128) is
    rounded once on the host -- 3 / 4608 and 1 / 1536 are the same real number, hence the same float. What is left to differ is the row
    arithmetic itself (which wave, which of the four row slots, which trip of the grid-stride loop carries a row): it must not."""
    fk, rl, _ = triplet_case()
    _, d3 = ops.patch_triplet(fk.to(DEV), rl.to(DEV), NEG, gscale=3.0)
    _, d1 = ops.patch_triplet(fk[:1].to(DEV), rl[:1].to(DEV), NEG)
    assert d1.abs().max().item() > 0 and torch.equal(d3[:1], d1)
    _, d3b = ops.patch_triplet(fk.to(DEV), rl.to(DEV), NEG)           # and at gscale = 1: the same hinge masks, values / 3 to rounding
    assert torch.equal(d3b[:1] == 0, d1 == 0) and torch.allclose(d3b[:1] * 3.0, d1, rtol=3e-7, atol=0.0)


def test_triplet4_rejects_bad_arguments():
    x = torch.zeros(1, 3, 256, 256, device=DEV)
    with pytest.raises(T.TfcError):
        ops.patch_triplet(x, x, [0, 1, 2, 4])                      # index out of range
    with pytest.raises(T.TfcError):
        ops.patch_triplet(x, x, [0, -1, 2, 3])
    with pytest.raises(T.TfcError):
        ops.patch_triplet(x, x, [0] * 9)                           # the 3x3 grid the reference never built
    loss = torch.empty(1, device=DEV)
    idx = (ctypes.c_int * 16)(*([0] * 16))
    for grid in (1, 3, 8):
        rc = ops.lib().tfc_patch_triplet(ops.stream_ptr(), x.data_ptr(), x.data_ptr(), idx, grid, 1, 3, loss.data_ptr(), None, 1.0)
        assert rc != 0 and b"grid" in ops.lib().tfc_last_error()
        with pytest.raises(T.TfcError):
            _lib.check(rc, "tfc_patch_triplet")
    ts_args = (T.GeneratorUNet((3, 256, 256)).to(DEV), T.Discriminator1((3, 256, 256)).to(DEV))
    with pytest.raises(T.TfcError):
        T.TrainStep(*ts_args, patches=9)
    ts = T.TrainStep(*ts_args, patches=4)
    with pytest.raises(T.TfcError):
        ts.step(x, x, neg_idx=list(range(16)))                     # 16 indices for the 4-patch step


# ---- spectra at S = 128 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wx,wy,N,shift", [(2, 2, 1, False), (2, 2, 3, True), (1, 1, 1, True)])
def test_fft128_matches_direct_dft_and_numpy(golden, wx, wy, N, shift):
    """the 128-point LDS FFT (three radix-4 passes + one radix-2 pass; NB = 65 leaves a ragged last column block) against the direct-DFT kernel
    and numpy's float64 rfft2 of the same uint8 luma: the bounds of test_fft_path_matches_direct_dft_and_numpy at S = 64 / 256.
    Phase is compared where amp > 1e-3 * max(amp); with these inputs that leaves out 9.7 - 10.4 % of the bins of a window (numpy,
    patch4_ref.masked_share; the DC bin sets the maximum), asserted <= 12 %."""
    x = R4.spectrum_inputs(N).to(DEV)
    img = x if (wx, wy) == (2, 2) else T.make_4_patches(x)[2]      # (1,1): a non-contiguous 128 x 128 view
    assert (wx, wy) == (2, 2) or not img.is_contiguous()
    a1, p1 = ops.fft_spectrum(img, 128, wx, wy, shift=shift)
    a0, p0 = ops.fft_spectrum(img, 128, wx, wy, shift=shift, direct=True)
    assert a1.shape == (N * wx * wy, 128, 65)
    scale = a0.max().item()
    err = (a1 - a0).abs().max().item()
    big = a0 > 1e-3 * scale                                        # phase of a near-zero bin is noise in any arithmetic
    share = 1.0 - big.flatten(1).float().mean(dim=1)
    dp = (p1 - p0).abs()
    dp = torch.minimum(dp, 2 * np.pi - dp)
    print(f"fft vs direct: amp {err / scale:.3e} of max, phase {dp[big].max().item():.3e} rad, masked share {share.min().item():.4f} .. {share.max().item():.4f}")
    assert err <= 2e-6 * scale
    assert share.max().item() <= 0.12
    assert dp[big].max().item() <= 2e-3
    # numpy float64 on window 0 of image 0
    luma = R4.luma_of(img[0, :, :128, :128].cpu())
    f = np.fft.rfft2(luma)
    if shift:
        f = np.fft.fftshift(f)
    want = torch.from_numpy(np.abs(f).astype(np.float32))
    assert (a1[0].cpu() - want).abs().max().item() <= 4e-6 * scale
    # the four self-conjugate bins: Im = +0, so the phase is exactly 0 or pi
    ky, kx = ([64, 0], [32, 31]) if shift else ([0, 64], [0, 64])  # fftshift: ky -> (ky + 64) % 128, kx -> (kx + 32) % 65
    for pha in (p1, p0):
        corner = pha[:, ky][:, :, kx]
        assert bool(((corner == 0.0) | (corner == float(np.float32(np.pi)))).all())
    if (wx, wy) == (1, 1):
        # the public surface on a view, against the reference's own fft_components (forms of test_fft_spectrum_vs_oracle_and_golden)
        gp = golden("fft_patch128")
        ff, _ = O.synthetic_pairs(1, seed=441)
        ff = (torch.tanh(ff * 2.0) * 0.999).to(DEV)
        amp, pha = T.fft_components(T.make_4_patches(ff)[2])
        a_ref, p_ref = t(gp["amp2"]), t(gp["pha2"])
        assert amp.shape == (1, 1, 128, 65)
        assert (amp.cpu() - a_ref).abs().max().item() <= 2e-6 * a_ref.max().item() + 2e-2
        dphi = (pha.cpu() - p_ref).abs()
        dphi = torch.minimum(dphi, 2 * np.pi - dphi)
        assert (dphi * a_ref).max().item() <= 0.05


def test_fft128_losses_and_spectra_vs_golden(golden):
    gp = golden("fft_patch128")
    ff, rr = O.synthetic_pairs(1, seed=441)
    ff = (torch.tanh(ff * 2.0) * 0.999).to(DEV)
    rr = rr.to(DEV)
    loss, la, lp = T.patch_fft_loss(ff, rr, patches=4)
    assert abs(loss.item() - float(gp["loss_fft"])) <= 2e-4 * float(gp["loss_fft"])          # tolerances of the 16-patch test
    assert abs(la.item() - float(gp["loss_amp"])) <= 1e-4 * float(gp["loss_amp"]) and abs(lp.item() - float(gp["loss_pha"])) <= 2e-3
    z, _, _ = T.patch_fft_loss(ff, ff, patches=4)
    assert z.item() == 0.0                                          # identical images -> exactly zero
    both = T.calculate_ffts(*T.make_4_patches(ff), *T.make_4_patches(rr))
    assert abs(both.item() - loss.item()) <= 2e-4 * loss.item()
    # the 16-patch default is what it was
    l16, _, _ = T.patch_fft_loss(ff, rr)
    l16b, _, _ = T.patch_fft_loss(ff, rr, patches=16)
    assert torch.equal(l16, l16b)
    # sample_spectra / make_spectra on 128 x 128 (4P:254-259, :291-301), tolerance of test_sample_spectra_and_mse_spec_vs_reference_goldens
    sp, _ = O.synthetic_pairs(2, seed=481)
    sp = (torch.tanh(sp * 1.2) * 0.999 + 1e-3)[:, :, 128:, :128].to(DEV)
    spec = T.sample_spectra(sp).cpu()
    assert spec.shape == (2, 1, 128, 128)
    assert (spec[:, :, ::4, ::4] - t(gp["spec_sub"])).abs().max().item() <= 2e-3
    assert (spec[1, 0, 7, :] - t(gp["spec_row7"])).abs().max().item() <= 2e-3
    assert abs(spec.mean().item() - float(gp["spec_mean"])) <= 1e-4
    one = T.FFT_Components(sp[0].contiguous()).make_spectra().cpu()
    assert torch.equal(one, spec[0, 0])
    a1, _ = T.FFT_Components(sp[0].contiguous()).make_components()
    assert a1.shape == (128, 65)
    # log-magnitude metrics accept the 128 x 65 half spectra
    amp_a, _ = ops.fft_spectrum(ff, 128, 2, 2, shift=False)
    amp_b, _ = ops.fft_spectrum(rr, 128, 2, 2, shift=False)
    assert ops.logmag_mse(amp_a, amp_a).abs().max().item() == 0.0 and bool((ops.logmag_mse(amp_a, amp_b, absolute=True) > 0).all())


def test_spectrum_still_rejects_other_sizes():
    x = torch.zeros(1, 3, 512, 512, device=DEV)
    for S in (32, 512):
        assert ops.lib().tfc_fft_spectrum_ws_bytes(S, 1) == 0
        with pytest.raises(T.TfcError):
            ops.fft_spectrum(x, S, 1, 1, direct=True)
        with pytest.raises(T.TfcError):
            ops.fft_spectrum(x, S, 1, 1)                            # the FFT path (no scratch size exists for S)
        ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)   # ... and with a scratch pointer given
        amp = torch.empty((1, S, S // 2 + 1), device=DEV)
        rc = ops.lib().tfc_fft_spectrum(ops.stream_ptr(), x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), 3, S, 1, 1, 1,
                                        amp.data_ptr(), amp.clone().data_ptr(), 0, ws.data_ptr())
        assert rc != 0
    assert ops.lib().tfc_fft_spectrum_ws_bytes(128, 3) == 3 * 65 * 128 * 8


# ---- steps ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,seed,mode", [("train_step_patch4", 465, "patch"), ("train_step_glo4", 466, "global")])
def test_patch4_train_step_fp32_vs_reference_golden(golden, tag, seed, mode):
    """TrainStep(patches=4) at N = 1 in fp32 compute mode against one step of the networks lifted from the 4-patch scripts: the checks and tolerances
    of test_train_step_fp32_vs_reference_golden (losses 2e-4, gradient tensors 1e-2 relative L2 -- the knife-edge scale explained there --, Adam
    deltas 2e-6)"""
    g = golden(tag)
    T.set_compute_dtype(torch.float32)
    try:
        G = O.init_weights_portable(T.GeneratorUNet((3, 256, 256)), seed=61).to(DEV).eval()
        D = O.init_weights_portable(T.Discriminator1((3, 256, 256)), seed=62).to(DEV).train()
        gb = {k: v.clone() for k, v in G.state_dict().items()}
        db = {k: v.clone() for k, v in D.state_dict().items()}
        A, B = O.synthetic_pairs(1, seed=seed)
        ts = T.TrainStep(G, D, compute_dtype=torch.float32, fft_mode=mode, patches=4)
        out = ts.step(A.to(DEV), B.to(DEV), neg_idx=g["neg_idx"].tolist())
        torch.cuda.synchronize()
    finally:
        T.set_compute_dtype(torch.bfloat16)
    assert set(out) == {"loss_G", "loss_GAN_g", "loss_triplet_patch", "loss_FFT", "loss_Amp", "loss_Pha", "loss_D", "fake_B"}     # the log keys of PATCH-16
    for k in ("loss_G", "loss_GAN_g", "loss_triplet_patch", "loss_FFT", "loss_D"):
        want = float(g[k])
        print(f"  {k}: {float(out[k]):.7g} (reference {want:.7g})")
        assert abs(float(out[k]) - want) <= 2e-4 * max(1.0, abs(want)), (k, float(out[k]), want)
    assert (out["fake_B"].cpu()[:, :, ::8, ::8] - t(g["fake_sub"])).abs().mean().item() <= 1e-4

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


def test_patch4_step_is_bit_deterministic_on_one_and_two_streams():
    """two PATCH-4 steps from the same state (bf16, N = 2, negatives drawn by shared_neg_idx(patches=4)): the same bits run to run on two streams and
    against the one-stream schedule, as test_step_is_bit_deterministic_on_one_and_two_streams shows for PATCH-16"""
    runs = []
    prev = T.set_wgrad_stream(True)
    try:
        for on in (True, True, False):
            T.set_wgrad_stream(on)
            G = O.init_weights_portable(T.GeneratorUNet((3, 256, 256)), seed=71).to(DEV)
            D = O.init_weights_portable(T.Discriminator1((3, 256, 256)), seed=72).to(DEV)
            A, B = O.synthetic_pairs(2, seed=73)
            A, B = A.to(DEV), B.to(DEV)
            ts = T.TrainStep(G, D, compute_dtype=torch.bfloat16, patches=4)
            ts.step(A, B)
            out2 = ts.step(A, B)
            torch.cuda.synchronize()
            runs.append({"g_w": ts.gflat.data.clone(), "d_w": ts.dflat.data.clone(), "g_grad": ts.gflat.grad.clone(), "d_grad": ts.dflat.grad.clone(),
                         "fake": out2["fake_B"].clone(),
                         "losses": torch.stack([out2[k].reshape(()).float() for k in sorted(out2) if k != "fake_B"]).clone()})
    finally:
        T.set_wgrad_stream(prev)
    ref = runs[0]
    assert torch.isfinite(ref["losses"]).all() and ref["g_grad"].abs().max().item() > 0
    for what, other in (("two streams, run to run", runs[1]), ("two streams vs one stream", runs[2])):
        for k in ref:
            assert torch.equal(ref[k], other[k]), (what, k)
