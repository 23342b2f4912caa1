"""Evaluation metrics, host side (no GPU): the numpy / scipy restatements the GPU tests are held against (tests/eval_metrics_ref.py) agree with the
closed forms of the metrics, and the C ABI of the metric kernels is declared on both sides."""
import os

import numpy as np

from tests import eval_metrics_ref as R
from tfc_gan_amd import _lib

METRIC_SYMBOLS = {"tfc_pair_moments_ws_bytes", "tfc_pair_moments_u8", "tfc_ssim_ws_bytes", "tfc_ssim_u8", "tfc_hist_u8_color", "tfc_hist_u8_joint",
                  "tfc_mi_bin_lut", "tfc_bhattacharyya", "tfc_mutual_information"}


def images():
    rng = np.random.default_rng(7)
    return rng.integers(0, 256, (37, 53), dtype=np.uint8), rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)


def test_identical_images_closed_forms():
    gray, colour = images()
    assert R.psnr(colour, colour) == 100.0 and R.psnr_literal_f32(colour, colour) == 100.0
    assert abs(R.ssim_2d(gray, gray) - 1.0) <= 1e-12 and abs(R.ssim_columns(gray, gray) - 1.0) <= 1e-12
    assert R.bhattacharyya(colour, colour) <= 1e-7
    assert abs(R.ncc(gray, gray) - 1.0) <= 1e-12 and abs(R.ncc_literal_f32(gray, gray) - 1.0) <= 1e-4


def test_psnr_of_a_known_mse():
    a = np.zeros((8, 9), dtype=np.uint8)
    b = np.full((8, 9), 5, dtype=np.uint8)                          # mse = 25: 20 log10(255 / 5)
    assert abs(R.psnr(a, b) - 20 * np.log10(51.0)) <= 1e-12
    assert abs(R.psnr_literal_f32(a, b) - 20 * np.log10(51.0)) <= 1e-5


def test_ncc_of_the_negative_and_of_a_constant():
    gray, _ = images()
    assert abs(R.ncc(gray, 255 - gray) + 1.0) <= 1e-12
    # 0 / 0 where the variance is exactly zero. (In floating point that needs a mean without rounding error -- an all-zero image; the mean of
    # another constant can be an ulp off and the restatement then returns noise. The kernel's integer moments give NaN for every constant.)
    assert np.isnan(R.ncc(np.zeros_like(gray), gray))


def test_ssim_column_form_differs_from_the_2d_form_and_both_lie_in_range():
    gray, _ = images()
    other = np.random.default_rng(8).integers(0, 256, gray.shape, dtype=np.uint8)
    s2, s1 = R.ssim_2d(gray, other), R.ssim_columns(gray, other)
    assert -1.0 <= s2 <= 1.0 and -1.0 <= s1 <= 1.0 and s1 != s2
    # one window: the map has a single valid value, which the formula gives directly from the window's moments
    x, y = gray[:7, :7].astype(np.float64), other[:7, :7].astype(np.float64)
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    cov = ((x - x.mean()) * (y - y.mean())).sum() / 48
    want = (2 * x.mean() * y.mean() + c1) * (2 * cov + c2) / ((x.mean() ** 2 + y.mean() ** 2 + c1) * (x.var(ddof=1) + y.var(ddof=1) + c2))
    assert abs(R.ssim_2d(gray[:7, :7], other[:7, :7]) - want) <= 1e-9


def test_mutual_information_closed_forms():
    gray, _ = images()
    const = np.full_like(gray, 77)
    for edges in {"float64", R.NATIVE_EDGES}:
        h = R.joint_hist(const, gray, edges=edges)
        assert h.sum() == gray.size and np.count_nonzero(h.sum(axis=1)) == 1      # a constant image fills one row of the joint histogram
        assert R.mutual_information(h) == 0.0
        two = np.where(gray > 127, 200, 10).astype(np.uint8)
        h2 = R.joint_hist(two, two, edges=edges)                                     # two levels against themselves: MI = the entropy of the split
        p = np.array([(two == 10).mean(), (two == 200).mean()])
        assert abs(R.mutual_information(h2) + (p * np.log(p)).sum()) <= 1e-12
    # the literal call (float32 pixels into np.histogram2d as installed) is the restatement with this numpy's native edge dtype
    lit, _, _ = np.histogram2d(R.pixels_f32(gray).ravel(), R.pixels_f32(255 - gray).ravel(), bins=20)
    assert np.array_equal(lit.astype(np.int64), R.joint_hist(gray, 255 - gray, edges=R.NATIVE_EDGES))


def test_bhattacharyya_histogram_is_the_shift_by_five():
    _, colour = images()
    h = R.color_hist(colour)
    want = np.zeros((8, 8, 8), dtype=np.int64)
    np.add.at(want, tuple((colour.reshape(-1, 3) >> 5).T), 1)
    assert np.array_equal(h, want)
    assert R.bhattacharyya(colour, colour // 2) >= 0.05


def test_metric_prototypes_are_declared_on_both_sides():
    assert METRIC_SYMBOLS <= set(_lib.PROTOTYPES)
    assert "metrics.hip" in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, "metrics.hip"))
    block = open(_lib.PUBLIC_HEADER).read().split("/* ---- evaluation metrics ---- */")[1]
    assert METRIC_SYMBOLS <= set(_lib.parse_header(block.split("#ifdef __cplusplus")[0])[0])     # declared in the header's metrics section
    lib = _lib.load()
    for name in METRIC_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.tfc_abi_version() == 3


def test_metric_entry_points_refuse_bad_arguments_loudly():
    lib = _lib.load()
    assert lib.tfc_ssim_u8(None, 1, 64, 8, 1, 64, 8, 1, 6, 8, 7, 7, 255.0, 8, 8) != 0
    assert b"smaller than" in lib.tfc_last_error()
    assert lib.tfc_ssim_u8(None, 1, 64, 8, 1, 64, 8, 1, 8, 8, 5, 5, 255.0, 8, 8) != 0
    assert b"supported" in lib.tfc_last_error()
    assert lib.tfc_pair_moments_u8(None, 1, 8, 1, 8, (1 << 23) + 1, 1, 8, 8, None, None) != 0
    assert lib.tfc_ssim_ws_bytes(3, 256, 256, 7, 7) == 3 * 4 * 16 * 8 and lib.tfc_ssim_ws_bytes(3, 6, 256, 7, 7) == 0
    assert lib.tfc_pair_moments_ws_bytes(2, 65537) == 2 * 2 * 10 * 8
