"""CPU side of the 4-patch configurations (PATCH-4 / GLO-4, TFCGAN_multigpu_patchFFT.py = "4P" / TFCGAN_multigpu_globalFFT.py = "4G"): the torch / numpy
restatement tests/patch4_ref.py against the fixtures made from the reference's own (lifted) definitions by tests/golden/make_golden_patch4.py, and
the host-side pieces of the package (patch views, index map, negative-index draw). No GPU."""
import numpy as np
import pytest
import torch

import tfc_gan_amd as T
from oracle import tfcgan_oracle as O
from tests import patch4_ref as R4


@pytest.fixture(autouse=True)
def host_independent_cpu_numerics():
    """the CPU numerics the fixtures were made with (tests/test_oracle_golden.py does the same)"""
    threads, mkldnn = torch.get_num_threads(), torch.backends.mkldnn.enabled
    torch.set_num_threads(8)
    torch.backends.mkldnn.enabled = False
    yield
    torch.set_num_threads(threads)
    torch.backends.mkldnn.enabled = mkldnn


def t(a):
    return torch.from_numpy(np.asarray(a))


def test_ref_triplet4_reproduces_the_fixture(golden):
    g = golden("triplet4")
    neg = g["neg_idx"].tolist()
    fk, rl = O.synthetic_pairs(3, seed=431)
    fk = torch.tanh(fk * 1.5)
    for n, tag in ((3, "n3"), (1, "n1")):
        f = fk[:n].clone().requires_grad_(True)
        loss = R4.patch_triplet_loss(f, rl[:n], neg)
        loss.backward()
        assert abs(loss.item() - float(g["loss_" + tag])) < 2e-6                                   # tolerances of test_triplet16_vs_oracle_and_golden
        assert torch.allclose(f.grad[:, :, ::4, ::4], t(g["gfake_sub_" + tag]), atol=1e-9, rtol=1e-4)
        if n == 3:
            assert abs(f.grad.abs().mean().item() - float(g["gfake_absmean_n3"])) <= 1e-4 * float(g["gfake_absmean_n3"])
    # the patch whose negative is itself contributes exactly the margin
    assert neg[1] == 1 and abs(float(g["per_patch_n3"][1]) - 1.0) < 1e-6


def test_ref_fft128_reproduces_the_fixture(golden):
    g = golden("fft_patch128")
    ff, rr = O.synthetic_pairs(1, seed=441)
    ff = torch.tanh(ff * 2.0) * 0.999
    amp, pha = R4.fft_components(R4.make_4_patches(ff)[2])
    assert amp.shape == (1, 1, 128, 65)
    a_ref, p_ref = t(g["amp2"]), t(g["pha2"])
    # numpy float64 rfft2 on both sides, cast to float32: equal up to that cast
    assert (amp - a_ref).abs().max().item() <= 1.2e-7 * a_ref.max().item()
    dphi = (pha - p_ref).abs()
    dphi = torch.minimum(dphi, 2 * np.pi - dphi)
    assert (dphi * a_ref).max().item() <= 1e-6 * a_ref.max().item()
    loss, la, lp = R4.patch_fft_loss(ff, rr)
    assert abs(float(loss) - float(g["loss_fft"])) <= 1e-6 * float(g["loss_fft"])
    assert abs(float(la) - float(g["loss_amp"])) <= 1e-6 * float(g["loss_amp"]) and abs(float(lp) - float(g["loss_pha"])) <= 1e-6
    sp, _ = O.synthetic_pairs(2, seed=481)
    sp = (torch.tanh(sp * 1.2) * 0.999 + 1e-3)[:, :, 128:, :128]
    spec = R4.sample_spectra(sp)
    assert spec.shape == (2, 1, 128, 128)
    assert (spec[:, :, ::4, ::4] - t(g["spec_sub"])).abs().max().item() <= 1e-5
    assert (spec[1, 0, 7, :] - t(g["spec_row7"])).abs().max().item() <= 1e-5
    assert abs(spec.mean().item() - float(g["spec_mean"])) <= 1e-5


@pytest.mark.parametrize("tag,seed,mode", [("train_step_patch4", 465, "patch"), ("train_step_glo4", 466, "global")])
def test_ref_train_step_reproduces_the_fixture(golden, tag, seed, mode):
    """one step of 4P:455-541 / 4G:454-530 restated on the oracle's networks against the step of the lifted networks (tolerances of
    tests/test_oracle_golden.py::test_train_step)"""
    g = golden(tag)
    G = O.init_weights_portable(O.GeneratorUNet((3, 256, 256)), seed=61).eval()
    D = O.init_weights_portable(O.Discriminator1((3, 256, 256)), seed=62).train()
    gb = {k: v.clone() for k, v in G.state_dict().items()}
    db = {k: v.clone() for k, v in D.state_dict().items()}
    A, B = O.synthetic_pairs(1, seed=seed)
    out = R4.train_step(G, D, A, B, g["neg_idx"].tolist(), fft_mode=mode)
    for k in ("loss_G", "loss_GAN_g", "loss_triplet_patch", "loss_FFT", "loss_Amp", "loss_Pha", "loss_D"):
        assert abs(float(out[k]) - float(g[k])) <= 1e-5 * max(1.0, abs(float(g[k]))), k
    assert torch.allclose(out["fake_B"][:, :, ::8, ::8], t(g["fake_sub"]), atol=2e-6)
    assert torch.allclose(G.state_dict()["final.2.weight"] - gb["final.2.weight"], t(g["g_delta_final_w"]), atol=1e-6)
    assert torch.allclose(G.state_dict()["down1.model.0.weight"] - gb["down1.model.0.weight"], t(g["g_delta_down1"]), atol=1e-6)
    assert torch.allclose(D.state_dict()["model.13.weight"] - db["model.13.weight"], t(g["d_delta_head"]), atol=1e-6)
    assert torch.allclose(D.state_dict()["model.3.parametrizations.weight.0._u"], t(g["d_u3"]), atol=1e-5)


def test_make_4_patches_views_and_index_map():
    B = torch.arange(3 * 256 * 256, dtype=torch.float32).reshape(1, 3, 256, 256)
    patches = T.make_4_patches(B)
    assert len(patches) == 4 and all(tuple(p.shape) == (1, 3, 128, 128) for p in patches)
    assert all(p.untyped_storage().data_ptr() == B.untyped_storage().data_ptr() for p in patches)      # views, not copies
    first = [int(p[0, 0, 0, 0]) for p in patches]
    assert first == [0, 128, 32768, 32896]
    assert [T.patch_first_flat_index(k, grid=2) for k in range(4)] == first
    assert [T.patch_first_flat_index(k, 256, 2) for k in range(4)] == first
    for p, q in zip(patches, R4.make_4_patches(B)):
        assert torch.equal(p, q)
    patches[3][0, 0, 0, 0] = -1.0                                                                       # writes through to the image
    assert B[0, 0, 128, 128].item() == -1.0
    # the 16-patch map is what it was
    assert [T.patch_first_flat_index(k) for k in range(5)] == [0, 64, 128, 192, 16384] and T.patch_first_flat_index(15) == 49344
    # the CPU pieces of the wider surface
    st = T.stitch_patches(B, B, patches=4)
    assert st.shape == (1, 12, 256, 128) and torch.equal(st[:, 3:6, :128], patches[1]) and torch.equal(st[:, 3:6, 128:], patches[1])
    assert torch.equal(T.stitch_patches(B, B, patches=16), T.stitch_16_patches(B, B))


def test_shared_neg_idx_default_is_unchanged_and_patches4_is_deterministic():
    sn = T.parallel.shared_neg_idx
    # the parent commit's values, computed there and written down
    assert sn(1) == [2, 2, 12, 6, 15, 0, 14, 14, 0, 11, 14, 13, 2, 5, 4, 4]
    assert sn(7, 0) == [12, 0, 3, 12, 9, 12, 8, 7, 14, 13, 14, 15, 0, 1, 9, 8]
    assert sn(1000, 77) == [9, 0, 8, 0, 2, 9, 4, 14, 11, 4, 4, 11, 11, 7, 12, 15]
    assert sn(7, 0, patches=16) == sn(7, 0)
    for step, seed in ((1, 1234), (7, 0), (1000, 77)):
        four = sn(step, seed, patches=4)
        assert len(four) == 4 and all(isinstance(v, int) and 0 <= v < 4 for v in four)
        assert four == sn(step, seed, patches=4)
    assert len({tuple(sn(s, 5, patches=4)) for s in range(1, 40)}) > 10                                 # a draw per step, not a constant


def test_cpu_tensors_and_bad_lengths_are_refused():
    x = torch.zeros(1, 3, 256, 256)
    with pytest.raises(T.TfcError):
        T.ops.patch_triplet(x, x, [0, 1, 2, 3])                       # CPU tensors: no fallback
    with pytest.raises(T.TfcError):
        T.ops.patch_triplet(x, x, [0, 1, 2])                          # neither 4 nor 16 indices


def test_share_of_bins_the_phase_comparison_leaves_out():
    """the S = 128 spectrum test on the GPU compares phases where amp > 1e-3 * max(amp) and allows that mask to drop at most 12 % of a window's
    bins: numpy float64 on the very inputs of that test gives 9.6 - 10.4 % per window (the DC bin sets the maximum)"""
    for wx, wy, N in ((2, 2, 1), (2, 2, 3), (1, 1, 1)):
        share = R4.masked_share(R4.spectrum_inputs(N), wx, wy)
        assert share.shape == (N * wx * wy,)
        assert 0.096 <= share.min() and share.max() <= 0.104, (wx, wy, N, share.min(), share.max())
