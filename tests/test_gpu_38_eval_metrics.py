"""Evaluation metrics on the GPU (tfc_gan_amd.metrics, csrc/metrics.hip) against the float64 numpy / scipy restatements of
tests/eval_metrics_ref.py. The kernels' sums are exact integers and only the fp64 finalisers round, so the bounds are those of the restatements:

    SSIM   abs <= 1e-9   uniform_filter's float64 rounding is ~1e-11 on second moments <= 65025; the denominators are >= C1 C2 ~ 380
    PSNR   abs <= 1e-9 dB vs float64; <= 1e-4 dB vs the script's float32 form (its pairwise float32 mean carries ~1e-6 relative = ~4e-6 dB)
    Bhatt  the 512-bin histogram EQUAL to np.histogramdd's; distance abs <= 1e-9 where d >= 0.05 (d = sqrt(1 - bc) amplifies the rounding of bc
           by 1 / (2 d)); an identical pair gives d <= 1e-7
    NCC    abs <= 1e-9 vs float64, <= 1e-4 vs the float32 form; b = 255 - a gives -1 to 1e-12; a constant image gives NaN
    MI     the 20 x 20 joint histogram EQUAL to np.histogram2d's; MI abs <= 1e-12

Shapes: 7 x 7 (a single SSIM window), 8 x 9, 37 x 53 (ragged tiles in both directions, window overhang at every edge), 256 x 256; N = 3 seeded images:
uniform noise, a smooth gradient plus noise, one pair with fake = real.
"""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tfc_gan_amd as T
from tests import eval_metrics_ref as R
from tfc_gan_amd import metrics as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(7, 7), (8, 9), (37, 53), (256, 256)]
IDS = ["7x7", "8x9", "37x53", "256x256"]


def make_pairs(H, W, channels=None):
    """(real, fake): uint8 [3,H,W] or [3,H,W,C]: noise against noise of another range, gradient + noise twice, an identical pair"""
    rng = np.random.default_rng(1000 * H + W + (channels or 0))
    shp = (H, W) if channels is None else (H, W, channels)
    yy, xx = np.mgrid[0:H, 0:W]
    grad = 30.0 + 150.0 * (yy / max(H - 1, 1)) + 50.0 * (xx / max(W - 1, 1))
    if channels is not None:
        assert channels == 3
        grad = np.stack([grad, 230.0 - grad, 0.5 * grad + 40.0], axis=-1)
    real = [rng.integers(0, 256, shp), np.clip(grad + rng.integers(-12, 13, shp), 0, 255), rng.integers(0, 256, shp)]
    fake = [rng.integers(0, 192, shp), np.clip(0.8 * grad + 25.0 + rng.integers(-12, 13, shp), 0, 255), real[2]]
    return np.stack(real).astype(np.uint8), np.stack(fake).astype(np.uint8)


_CACHE = {}


def gray_case(shape):
    """(real, fake) gray pairs of a shape and their restated metrics, computed once"""
    if shape not in _CACHE:
        real, fake = make_pairs(*shape)
        ref = {name: np.array([fn(real[i], fake[i]) for i in range(3)]) for name, fn in
               [("ssim", R.ssim_2d), ("ssim_columns", R.ssim_columns), ("psnr", R.psnr), ("psnr_f32", R.psnr_literal_f32), ("ncc", R.ncc),
                ("ncc_f32", R.ncc_literal_f32)]}
        _CACHE[shape] = (real, fake, ref)
    return _CACHE[shape]


def report(name, got, want):
    err = np.abs(np.asarray(got) - np.asarray(want))
    print(f"{name}: max abs error {np.nanmax(err):.3e}")
    return err


def gpu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_ssim_both_window_modes(shape):
    real, fake, ref = gray_case(shape)
    got = M.ssim(gpu(real), gpu(fake)).cpu().numpy()
    got_c = M.ssim(gpu(real), gpu(fake), columns_as_channels=True).cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (3,)
    assert report("ssim 7x7", got, ref["ssim"]).max() <= 1e-9
    assert report("ssim 7x1", got_c, ref["ssim_columns"]).max() <= 1e-9
    assert abs(got[2] - 1.0) <= 1e-12 and abs(got_c[2] - 1.0) <= 1e-12               # fake = real
    half = M.ssim(gpu(real), gpu(fake), data_range=128).cpu().numpy()                  # data_range reaches C1, C2
    assert report("ssim range 128", half, [R.ssim_2d(real[i], fake[i], 128.0) for i in range(3)]).max() <= 1e-9


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_psnr_and_ncc_from_the_integer_moments(shape):
    real, fake, ref = gray_case(shape)
    p = M.psnr(gpu(real), gpu(fake)).cpu().numpy()
    assert report("psnr vs float64", p, ref["psnr"]).max() <= 1e-9
    assert report("psnr vs float32 literal", p, ref["psnr_f32"]).max() <= 1e-4
    assert p[2] == 100.0
    r = M.ncc(gpu(real), gpu(fake)).cpu().numpy()
    assert report("ncc vs float64", r, ref["ncc"]).max() <= 1e-9
    assert report("ncc vs float32 literal", r, ref["ncc_f32"]).max() <= 1e-4
    neg = M.ncc(gpu(real), gpu(255 - real)).cpu().numpy()
    assert report("ncc of the negative", neg, -np.ones(3)).max() <= 1e-12
    const = np.full_like(real, 9)
    assert np.isnan(M.ncc(gpu(const), gpu(fake)).cpu().numpy()).all() and np.isnan(M.ncc(gpu(real), gpu(const)).cpu().numpy()).all()
    # the moments themselves are exact
    mom = T.ops.pair_moments(gpu(real), gpu(fake))[0].cpu().numpy()
    a, b = real.reshape(3, -1).astype(np.int64), fake.reshape(3, -1).astype(np.int64)
    want = np.stack([a.sum(1), b.sum(1), (a * a).sum(1), (b * b).sum(1), (a * b).sum(1), ((a - b) ** 2).sum(1), a.min(1), a.max(1), b.min(1), b.max(1)], 1)
    assert np.array_equal(mom, want)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bhattacharyya_histogram_equal_and_distance(shape):
    real, fake = make_pairs(*shape, channels=3)
    h = M.color_histogram(gpu(real)).cpu().numpy()
    assert np.array_equal(h.reshape(3, 8, 8, 8), np.stack([R.color_hist(real[i]) for i in range(3)]))
    hf = M.color_histogram(gpu(fake)).cpu().numpy()
    assert np.array_equal(hf.reshape(3, 8, 8, 8), np.stack([R.color_hist(fake[i]) for i in range(3)]))
    want = np.array([R.bhattacharyya(real[i], fake[i]) for i in range(3)])
    assert (want[:2] >= 0.05).all(), want                                              # the images are chosen so: the bound below applies
    got = M.bhattacharyya(gpu(real), gpu(fake)).cpu().numpy()
    assert report("bhattacharyya", got[:2], want[:2]).max() <= 1e-9
    assert got[2] <= 1e-7 and want[2] <= 1e-7
    # colour PSNR (the script's PSNR runs on the RGB arrays) and the two colour layouts
    p = M.psnr(gpu(real), gpu(fake)).cpu().numpy()
    assert report("colour psnr", p, [R.psnr(real[i], fake[i]) for i in range(3)]).max() <= 1e-9
    real_chw, fake_chw = gpu(real.transpose(0, 3, 1, 2)), gpu(fake.transpose(0, 3, 1, 2))
    assert torch.equal(M.psnr(real_chw, fake_chw).cpu(), torch.from_numpy(p))
    assert torch.equal(M.bhattacharyya(real_chw, fake_chw).cpu(), torch.from_numpy(got))
    assert np.array_equal(M.color_histogram(real_chw).cpu().numpy(), h)
    # a gray image counts as R = G = B
    g = real[..., 0]
    assert np.array_equal(M.color_histogram(gpu(g)).cpu().numpy(), M.color_histogram(gpu(np.repeat(g[..., None], 3, -1))).cpu().numpy())


def mi_images(H, W):
    """pairs for the joint histogram: full-range noise; levels 3 .. 203 (a range of 200: every tenth level sits on a bin edge up to rounding);
    a constant image; a two-level image; the gradient pair"""
    rng = np.random.default_rng(77 * H + W)
    real, fake, _ = gray_case((H, W))
    lim = rng.integers(3, 204, (H, W))
    lim.flat[0], lim.flat[-1] = 3, 203                                               # min and max are hit, the max exactly on the last edge
    a = [rng.integers(0, 256, (H, W)), lim, np.full((H, W), 77), np.where(rng.integers(0, 2, (H, W)) > 0, 200, 10), real[1], real[2]]
    b = [rng.integers(0, 256, (H, W)), rng.integers(40, 141, (H, W)), rng.integers(0, 256, (H, W)), lim, fake[1], fake[2]]
    return np.stack(a).astype(np.uint8), np.stack(b).astype(np.uint8)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_mutual_information_joint_histogram_equal(shape):
    a, b = mi_images(*shape)
    for edges in sorted({"float64", R.NATIVE_EDGES}):
        want_h = np.stack([R.joint_hist(a[i], b[i], edges=edges) for i in range(len(a))])
        got_h = M.joint_histogram(gpu(a), gpu(b), edges=edges).cpu().numpy()
        assert np.array_equal(got_h, want_h), (edges, np.argwhere(got_h != want_h)[:5])
        got = M.mutual_information(gpu(a), gpu(b), edges=edges).cpu().numpy()
        want = np.array([R.mutual_information(want_h[i]) for i in range(len(a))])
        assert report(f"mutual information ({edges} edges)", got, want).max() <= 1e-12
        assert got[2] == 0.0                                                             # the constant image
    if R.NATIVE_EDGES == "float32":                                                      # the literal call on this numpy
        lit = np.stack([np.histogram2d(R.pixels_f32(a[i]).ravel(), R.pixels_f32(b[i]).ravel(), bins=20)[0] for i in range(len(a))])
        assert np.array_equal(M.joint_histogram(gpu(a), gpu(b), edges="float32").cpu().numpy(), lit.astype(np.int64))


def all_metrics(real, fake):
    return torch.stack([M.psnr(real, fake), M.ssim(real, fake), M.ssim(real, fake, columns_as_channels=True), M.bhattacharyya(real, fake),
                        M.ncc(real, fake), M.mutual_information(real, fake)])


@pytest.mark.parametrize("shape", [(37, 53), (256, 256)], ids=["37x53", "256x256"])
def test_batch_invariance_and_determinism(shape):
    rng = np.random.default_rng(5)
    real, fake = gpu(rng.integers(0, 256, (13,) + shape, dtype=np.uint8)), gpu(rng.integers(0, 200, (13,) + shape, dtype=np.uint8))
    full = all_metrics(real, fake)
    assert torch.equal(full, all_metrics(real, fake))                                    # two calls, same bits
    assert torch.equal(full[:, :3], all_metrics(real[:3], fake[:3]))
    for i in (0, 2, 12):
        assert torch.equal(full[:, i:i + 1], all_metrics(real[i:i + 1], fake[i:i + 1])), i
    assert torch.equal(full[:, 10:13], all_metrics(real[10:13].clone(), fake[10:13].clone()))


def test_non_contiguous_views_are_handled():
    real, fake, ref = gray_case((37, 53))
    wide_r, wide_f = gpu(np.pad(real, ((0, 0), (2, 3), (5, 6)))), gpu(np.pad(fake, ((0, 0), (2, 3), (5, 6))))
    vr, vf = wide_r[:, 2:39, 5:58], wide_f[:, 2:39, 5:58]                                # row and image strides of the padded buffer
    assert not vr.is_contiguous()
    assert torch.equal(all_metrics(vr, vf), all_metrics(gpu(real), gpu(fake)))
    tr, tf = gpu(real.transpose(0, 2, 1)).transpose(1, 2), gpu(fake.transpose(0, 2, 1)).transpose(1, 2)   # unit stride along H, not W
    assert tr.stride(2) != 1
    assert torch.equal(all_metrics(tr, tf), all_metrics(gpu(real), gpu(fake)))
    every_other = all_metrics(gpu(real)[::2], gpu(fake)[::2])
    assert torch.equal(every_other, all_metrics(gpu(real), gpu(fake))[:, ::2])
    assert report("cpu arrays are copied over", M.ssim(real, fake).cpu().numpy(), ref["ssim"]).max() <= 1e-9


def test_errors_are_loud():
    ok = gpu(np.zeros((2, 16, 16), dtype=np.uint8))
    with pytest.raises((T.TfcError, AssertionError), match="smaller than"):
        M.ssim(ok[:, :6], ok[:, :6])
    with pytest.raises((T.TfcError, AssertionError), match="smaller than"):
        M.ssim(ok[:, :, :6], ok[:, :, :6])
    M.ssim(ok[:, :, :6], ok[:, :, :6], columns_as_channels=True)                        # 7 x 1 windows fit 16 x 6
    for fn in (M.psnr, M.ssim, M.bhattacharyya, M.ncc, M.mutual_information):
        with pytest.raises((T.TfcError, AssertionError), match="uint8"):
            fn(ok.float(), ok)
        with pytest.raises((T.TfcError, AssertionError), match="same shape"):
            fn(ok, ok[:, :15])
    with pytest.raises((T.TfcError, AssertionError), match="gray"):
        M.ssim(ok[..., None].expand(2, 16, 16, 3), ok[..., None].expand(2, 16, 16, 3))
    with pytest.raises((T.TfcError, AssertionError), match="colour"):
        M.psnr(ok[..., None].expand(2, 16, 16, 2), ok[..., None].expand(2, 16, 16, 2))


def test_to_uint8_is_the_save_image_arithmetic():
    x = torch.tensor([-1.5, -1.0, -0.999, 0.0, 0.5, 1.0 - 1e-3, 1.0, 2.0], device="cuda")
    want = [0, 0, 0, 128, 191, 255, 255, 255]                                         # trunc(clamp((x + 1) / 2, 0, 1) * 255 + 0.5)
    assert M.to_uint8(x).tolist() == want and M.to_uint8(x).dtype == torch.uint8
    assert M.to_uint8(torch.tensor([0.0, 0.25, 1.0]), lo=0.0, hi=1.0).tolist() == [0, 64, 255]
    g = M.to_gray(gpu(np.array([[[[10, 10, 10], [255, 0, 0], [0, 255, 0], [0, 0, 255]]]], dtype=np.uint8)))
    assert g.tolist() == [[[10, 76, 150, 29]]]


def test_eval_accumulator_equals_direct_calls():
    real, fake = make_pairs(37, 53, channels=3)
    realA, _ = make_pairs(37, 53)
    real, fake, realA = gpu(np.concatenate([real, real[::-1]])), gpu(np.concatenate([fake, fake[::-1]])), gpu(np.concatenate([realA, realA]))
    acc = M.EvalAccumulator()
    acc.update(real[:4], fake[:4], realA[:4])
    acc.update(real[4:], fake[4:], realA[4:])
    res = acc.result()
    rg, fg = M.to_gray(real), M.to_gray(fake)
    want = {"psnr": M.psnr(real, fake), "ssim": M.ssim(rg, fg), "ssim_columns": M.ssim(rg, fg, columns_as_channels=True),
            "bhattacharyya": M.bhattacharyya(real, fake), "ncc": M.ncc(realA, fg), "mi": M.mutual_information(realA, fg)}
    assert set(res) == set(want)
    for k, v in want.items():
        assert np.array_equal(res[k]["values"], v.cpu().numpy()), k
        assert res[k]["mean"] == float(v.cpu().numpy().mean())
    plain = M.EvalAccumulator()
    plain.update(real, fake)
    assert set(plain.result()) == {"psnr", "ssim", "ssim_columns", "bhattacharyya"}


def test_evaluate_cli_writes_the_direct_values(tmp_path):
    from PIL import Image
    real, fake = make_pairs(16, 24, channels=3)
    real, fake = np.concatenate([real, real[:, ::-1]]), np.concatenate([fake, fake[:, ::-1]])
    os.mkdir(tmp_path / "real_B")
    os.mkdir(tmp_path / "fake_B")
    order = [4, 0, 5, 2, 1, 3]                                                        # file numbers, not listing order, pair the images
    for i, num in enumerate(order):
        Image.fromarray(real[i]).save(tmp_path / "real_B" / f"{num}_real_B.png")
        Image.fromarray(fake[i]).save(tmp_path / "fake_B" / f"img{num}_fake_B.png")
    out = tmp_path / "scores.csv"
    run = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-m", "tfc_gan_amd.evaluate", "--real", str(tmp_path / "real_B"), "--fake",
                          str(tmp_path / "fake_B"), "--csv", str(out)], cwd=ROOT, capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    rows = list(csv.DictReader(open(out)))
    assert [r["number"] for r in rows] == ["0", "1", "2", "3", "4", "5"]
    r, f = gpu(real), gpu(fake)
    rg, fg = M.to_gray(r), M.to_gray(f)
    want = {"psnr": M.psnr(r, f), "ssim": M.ssim(rg, fg), "ssim_columns": M.ssim(rg, fg, columns_as_channels=True), "bhattacharyya": M.bhattacharyya(r, f),
            "ncc": M.ncc(rg, fg), "mi": M.mutual_information(rg, fg)}
    for row in rows:
        i = order.index(int(row["number"]))
        assert row["real"] == f"{row['number']}_real_B.png" and row["fake"] == f"img{row['number']}_fake_B.png"
        for k, v in want.items():
            assert float(row[k]) == float(v[i]), (row["number"], k)
    assert "psnr: mean" in run.stdout
