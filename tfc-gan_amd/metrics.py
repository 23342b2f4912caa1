"""Evaluation metrics on the GPU: what the reference reads off saved PNGs with its offline scripts, computed on uint8 images that are already on the card.

    psnr, ssim           TFC-GAN-FFT/eval/<set>/evaluation_psnr_ssim.py (calculate_psnr :56-64, structural_similarity :119)
    bhattacharyya        TFC-GAN-FFT/eval/<set>/evaluation_bhatt.py:45-61 (cv2.calcHist 8 x 8 x 8 + compareHist(HISTCMP_BHATTACHARYYA))
    ncc                  TFC-STN/evaluation/calc_NCC.py:44-64
    mutual_information   TFC-STN/evaluation/calc_MI.py:58-82
    (the spectrum pair mse_spec / other_spec lives in losses.py)

Every sum over pixels is an integer sum and the finalisers are fp64 adding in a fixed order (csrc/metrics.hip): the values are
bit-reproducible and a pair's value does not depend on the batch it is computed in. Each function returns an [N] float64 CUDA tensor and does not
synchronise. Inputs are uint8 tensors or arrays: [N,H,W] gray, or [N,H,W,3] / [N,3,H,W] colour where the metric is defined on colour (a 4-D input
whose last dimension is 3 is read as [N,H,W,3]); CPU inputs are copied to the GPU; anything else raises.
"""
import numpy as np
import torch

from . import ops


def _u8(x, name):
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    assert t.dtype == torch.uint8, f"{name}: uint8 images expected, got {t.dtype} (to_uint8() converts generator output)"
    assert t.dim() in (3, 4), f"{name}: [N,H,W] gray or [N,H,W,3] / [N,3,H,W] colour expected, got shape {tuple(t.shape)}"
    return t if t.is_cuda else t.to("cuda", non_blocking=True)


def _layout(t, name):
    if t.dim() == 3:
        return "gray"
    if t.shape[-1] == 3:
        return "hwc"
    assert t.shape[1] == 3, f"{name}: a colour batch is [N,H,W,3] or [N,3,H,W], got shape {tuple(t.shape)}"
    return "chw"


def _pair(a, b, names, gray_only):
    a, b = _u8(a, names[0]), _u8(b, names[1])
    assert a.shape == b.shape, f"{names[0]} {tuple(a.shape)} and {names[1]} {tuple(b.shape)} must have the same shape"
    if gray_only:
        assert a.dim() == 3, f"this metric is defined on gray images [N,H,W], got shape {tuple(a.shape)} (to_gray() converts)"
    else:
        _layout(a, names[0])
    assert a.shape[0] > 0, "empty batch"
    return a, b


def to_uint8(x, lo=-1.0, hi=1.0):
    """Generator-range float images -> the uint8 a saved PNG would hold: trunc(clamp((x - lo) / (hi - lo), 0, 1) * 255 + 0.5), the published
    arithmetic of torchvision.utils.save_image(normalize=True, value_range=(lo, hi)). torchvision is not available to this project's tests:
    PARITY UNPINNED. Plain torch (not a hot path); shape and device are kept."""
    x = torch.as_tensor(x).float()
    return ((x - lo) / max(hi - lo, 1e-5)).clamp_(0.0, 1.0).mul_(255.0).add_(0.5).clamp_(0.0, 255.0).to(torch.uint8)


def to_gray(rgb):
    """uint8 colour [N,H,W,3] or [N,3,H,W] -> uint8 gray [N,H,W] with the integer formula (4899 R + 9617 G + 1868 B + 8192) >> 14: a restatement of
    cv2.cvtColor(COLOR_BGR2GRAY)'s fixed-point path (evaluation_psnr_ssim.py:92-93). cv2 is not available to this project's tests: PARITY UNPINNED;
    exact where R = G = B (thermal images), whatever the coefficients. Gray input is returned as it is."""
    t = _u8(rgb, "rgb")
    lay = _layout(t, "rgb")
    if lay == "gray":
        return t
    r, g, b = (t.unbind(-1) if lay == "hwc" else t.unbind(1))
    return ((4899 * r.int() + 9617 * g.int() + 1868 * b.int() + 8192) >> 14).to(torch.uint8)


def psnr(real, fake):
    """calculate_psnr: 100 where the images are equal, else 20 log10(255 / sqrt(mse)), mse over every element (colour or gray)."""
    a, b = _pair(real, fake, ("real", "fake"), gray_only=False)
    return ops.pair_moments(a, b, want_ncc=False)[1]


def ssim(real, fake, columns_as_channels=False, data_range=255):
    """skimage.metrics.structural_similarity on uint8 gray images: 7 x 7 uniform window, K1 0.01, K2 0.03, sample covariance, mean over the map
    cropped by 3 pixels. columns_as_channels=True is the reference's literal call (multichannel=True on a 2-D image, evaluation_psnr_ssim.py:119:
    every column is a 1-D channel): a 7 x 1 window, 3 rows cropped at the top and bottom, the mean over (H - 6) * W values."""
    a, b = _pair(real, fake, ("real", "fake"), gray_only=True)
    return ops.ssim_u8(a, b, 7, 1 if columns_as_channels else 7, data_range)


def color_histogram(img):
    """the 8 x 8 x 8 histogram of cv2.calcHist([img], [0, 1, 2], None, [8, 8, 8], [0, 256] * 3): int32 [N,512], bin (c0 >> 5, c1 >> 5, c2 >> 5)"""
    t = _u8(img, "img")
    return ops.hist_color(t, _layout(t, "img"))


def bhattacharyya(real, fake):
    """cv2.compareHist(HISTCMP_BHATTACHARYYA) of the two 8 x 8 x 8 colour histograms (gray images count as R = G = B)."""
    a, b = _pair(real, fake, ("real", "fake"), gray_only=False)
    lay = _layout(a, "real")
    return ops.bhattacharyya(ops.hist_color(a, lay), ops.hist_color(b, lay))


def ncc(a, b):
    """normalised cross-correlation = Pearson's r with ddof = 1 (gray). NaN where an image is constant, as the reference's 0 / 0."""
    a, b = _pair(a, b, ("a", "b"), gray_only=True)
    return ops.pair_moments(a, b, want_psnr=False)[2]


def _edge_f32(edges):
    assert edges in ("float64", "float32"), "edges: \"float64\" or \"float32\""
    return edges == "float32"


def joint_histogram(a, b, bins=20, edges="float64"):
    """np.histogram2d(a / 255, b / 255, bins) on float32 pixels, as int32 [N,bins,bins]. edges="float64": numpy 1.x, where linspace over float32
    scalars gives float64 edges (the reference's era); "float32": numpy >= 2, which keeps the pixels' dtype."""
    a, b = _pair(a, b, ("a", "b"), gray_only=True)
    assert 1 <= int(bins) <= 32, "bins: 1 .. 32"
    mom = ops.pair_moments(a, b, want_psnr=False, want_ncc=False)[0]
    return ops.joint_hist(a, b, mom, int(bins), _edge_f32(edges))


def mutual_information(a, b, bins=20, edges="float64"):
    """mutual information of the bins x bins joint histogram of two gray images (calc_MI.py): sum over non-zero cells of pxy log(pxy / (px py))."""
    return ops.mutual_information(joint_histogram(a, b, bins, edges))


class EvalAccumulator:
    """Validation-loop accumulator: update() queues the kernels of one batch and returns at once; result() is the single host synchronisation.

    update(real_u8, fake_u8, real_A_u8=None): psnr and bhattacharyya on the images as given (colour or gray), ssim and ssim_columns (the reference's
    literal 7 x 1 form) on their gray versions; with real_A_u8 also ncc and mi between gray(real_A) and gray(fake) -- the STN21 scripts' pairing.
    result(): {metric: {"mean": float, "values": float64 numpy array in update order}}."""

    def __init__(self, bins=20):
        self.bins = bins
        self.parts = {}

    def update(self, real_u8, fake_u8, real_A_u8=None):
        rg, fg = to_gray(real_u8), to_gray(fake_u8)
        got = {"psnr": psnr(real_u8, fake_u8), "ssim": ssim(rg, fg), "ssim_columns": ssim(rg, fg, columns_as_channels=True),
               "bhattacharyya": bhattacharyya(real_u8, fake_u8)}
        if real_A_u8 is not None:
            ag = to_gray(real_A_u8)
            got["ncc"] = ncc(ag, fg)
            got["mi"] = mutual_information(ag, fg, self.bins)
        assert not self.parts or set(got) == set(self.parts), "every update of one accumulator must pass (or omit) real_A_u8 alike"
        for k, v in got.items():
            self.parts.setdefault(k, []).append(v)

    def result(self):
        if not self.parts:
            return {}
        keys = list(self.parts)
        table = torch.stack([torch.cat(self.parts[k]) for k in keys]).cpu().numpy()      # the one synchronisation
        return {k: {"mean": float(table[i].mean()), "values": table[i]} for i, k in enumerate(keys)}
