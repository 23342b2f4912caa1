"""CPU restatements of the reference's evaluation metrics, in numpy / scipy only: a helper of the evaluation-metric tests, not a test.

The reference computes these with cv2 and scikit-image, which are not installed where this suite runs, so its scripts cannot be run to produce
goldens (and nothing under tests/golden/ belongs to these metrics). Each function below is written from the PUBLISHED definition of the library
call the script makes, with the script line cited; none copies reference text. Images are uint8 numpy arrays.

    psnr / psnr_literal_f32        TFC-GAN-FFT/eval/Devcom/evaluation_psnr_ssim.py:56-64 (calculate_psnr)
    ssim_2d / ssim_columns         evaluation_psnr_ssim.py:119 (skimage.metrics.structural_similarity; Wang et al. 2004, uniform 7-window variant)
    color_hist / bhattacharyya     TFC-GAN-FFT/eval/Devcom/evaluation_bhatt.py:55-61 (cv2.calcHist, cv2.normalize, cv2.compareHist)
    ncc / ncc_literal_f32          TFC-STN/evaluation/calc_NCC.py:44-64
    joint_hist / mutual_information TFC-STN/evaluation/calc_MI.py:58-82
"""
import numpy as np
from scipy.ndimage import uniform_filter


# ---- PSNR ----------------------------------------------------------------------------------------------------------------------------------------
def psnr(real, fake):
    """float64 throughout: the exact mean of the squared differences"""
    mse = np.mean((real.astype(np.float64) - fake.astype(np.float64)) ** 2)
    return 100.0 if mse == 0 else float(20 * np.log10(255.0 / np.sqrt(mse)))


def psnr_literal_f32(real, fake):
    """the script's own precision: float32 arrays (:48, :60), so np.mean is a pairwise float32 sum"""
    mse = np.mean((np.array(real, dtype=np.float32) - np.array(fake, dtype=np.float32)) ** 2)
    return 100.0 if mse == 0 else float(20 * np.log10(255 / np.sqrt(mse)))


# ---- SSIM ----------------------------------------------------------------------------------------------------------------------------------------
def _ssim_map(x, y, size, data_range):
    """structural_similarity's map for a uniform window of `size` (per axis): local means by uniform_filter in float64, SAMPLE covariance
    (cov_norm = NP / (NP - 1), the default use_sample_covariance=True), K1 = 0.01, K2 = 0.03"""
    X, Y = x.astype(np.float64), y.astype(np.float64)
    NP = float(np.prod(size))
    cov_norm = NP / (NP - 1)
    ux, uy = uniform_filter(X, size=size), uniform_filter(Y, size=size)
    uxx, uyy, uxy = uniform_filter(X * X, size=size), uniform_filter(Y * Y, size=size), uniform_filter(X * Y, size=size)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))


def ssim_2d(real, fake, data_range=255.0):
    """the 2-D metric: 7 x 7 window, the map cropped by (7 - 1) // 2 = 3 on every side (so uniform_filter's border mode never shows), float64 mean"""
    return float(_ssim_map(real, fake, (7, 7), data_range)[3:-3, 3:-3].mean(dtype=np.float64))


def ssim_columns(real, fake, data_range=255.0):
    """the script's literal call: multichannel=True on a 2-D image makes the LAST axis the channel axis, so every column is a 1-D signal with a
    7-window, cropped by 3 at both ends; the result is the mean over channels of equal-sized means = the mean over (H - 6) * W values"""
    return float(_ssim_map(real, fake, (7, 1), data_range)[3:-3, :].mean(dtype=np.float64))


# ---- Bhattacharyya -------------------------------------------------------------------------------------------------------------------------------
def color_hist(img):
    """cv2.calcHist([img], [0, 1, 2], None, [8, 8, 8], [0, 256, 0, 256, 0, 256]) as integer counts [8, 8, 8]; img: [H, W, 3]"""
    h, _ = np.histogramdd(img.reshape(-1, 3).astype(np.float64), bins=(8, 8, 8), range=((0, 256),) * 3)
    return h.astype(np.int64)


def bhattacharyya(real, fake):
    """cv2.compareHist(HISTCMP_BHATTACHARYYA): sqrt(max(1 - sum sqrt(h1 h2) / sqrt(sum h1 sum h2), 0)), written on the L2-normalised histograms
    cv2.normalize leaves (the scale divides out; computed here literally, in float64 where cv2 holds float32 histograms)"""
    h1, h2 = color_hist(real).astype(np.float64).ravel(), color_hist(fake).astype(np.float64).ravel()
    h1, h2 = h1 / np.sqrt(np.sum(h1 * h1)), h2 / np.sqrt(np.sum(h2 * h2))
    return float(np.sqrt(max(1.0 - np.sum(np.sqrt(h1 * h2)) / np.sqrt(np.sum(h1) * np.sum(h2)), 0.0)))


# ---- NCC -----------------------------------------------------------------------------------------------------------------------------------------
def _ncc(x, y):
    def norm_data(d):
        return (d - np.mean(d)) / np.std(d, ddof=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float((1.0 / (x.size - 1)) * np.sum(norm_data(x) * norm_data(y)))


def ncc(a, b):
    return _ncc(a.astype(np.float64) / 255.0, b.astype(np.float64) / 255.0)


def ncc_literal_f32(a, b):
    """the script's own precision: ToTensor's float32 pixels (:36-39), float32 mean / std / sum"""
    return _ncc(a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255))


# ---- mutual information --------------------------------------------------------------------------------------------------------------------------
def pixels_f32(a):
    """ToTensor: uint8 -> float32 / 255"""
    return a.astype(np.float32) / np.float32(255)


NATIVE_EDGES = "float32" if int(np.__version__.split(".")[0]) >= 2 else "float64"


def joint_hist(a, b, bins=20, edges="float64"):
    """np.histogram2d(IM1.ravel(), IM2.ravel(), bins=20) of calc_MI.py:59 on ToTensor's float32 pixels, as integer counts.
    edges="float64": numpy 1.x (the reference's era) promoted the float32 min / max against Python floats BY VALUE, so np.linspace produced float64
    edges and the float32 pixels were compared with them in float64; handing np.histogram2d the same pixel VALUES widened to float64 reproduces
    exactly that on every numpy. edges="float32": the literal call on numpy >= 2 (NEP 50 keeps float32) -- only meaningful when NATIVE_EDGES says so."""
    x, y = pixels_f32(a).ravel(), pixels_f32(b).ravel()
    if edges == "float64":
        x, y = x.astype(np.float64), y.astype(np.float64)
    else:
        assert NATIVE_EDGES == "float32", "float32 edges cannot be produced by numpy 1.x"
    h, _, _ = np.histogram2d(x, y, bins=bins)
    return h.astype(np.int64)


def mutual_information(hgram):
    """calc_MI.py:72-82 on a joint histogram"""
    joint = hgram / float(np.sum(hgram))
    independent = np.outer(np.sum(joint, axis=1), np.sum(joint, axis=0))      # product of the marginals
    seen = joint > 0
    return float(np.sum(joint[seen] * np.log(joint[seen] / independent[seen])))
