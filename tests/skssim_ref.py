"""The reference of the scikit-image SSIM call (include/ex4d_loss.h: ex4d_frame_skssim; ex4dgs_amd/evaluate.frame_skssim), shared by
tests/test_cpu_skssim.py and tests/test_gpu_skssim.py.

render.py:78-79 of the reference calls sk_ssim(render, gt, data_range=R, multichannel=True, channel_axis=0) with R = 1 (SKSSIM) and
R = 2 (SKSSIM2).  scikit-image is not installed, so structural_similarity (0.22 and later: `multichannel` is ignored, channel_axis=0
holds, win_size 7, uniform filter, sample covariance, 3-pixel crop, mean of the channel means) is RESTATED here in float64 with
scipy.ndimage.uniform_filter, and cross-checked by an independent formulation without scipy (sliding_window_view means over the valid
windows).  A reference is computed once per case and shared (lru_cache); callers do not modify what they get."""
import functools

import numpy as np
from scipy import ndimage

from tests import metrics_ref as mr
from tests import skssim_cases as sc

WIN, PAD = 7, 3
NP = WIN * WIN
COV_NORM = NP / (NP - 1.0)


def _s_map(ux, uy, uxx, uyy, uxy, R, dtype):
    vx, vy, vxy = dtype(COV_NORM) * (uxx - ux * ux), dtype(COV_NORM) * (uyy - uy * uy), dtype(COV_NORM) * (uxy - ux * uy)
    C1, C2 = dtype((0.01 * R) ** 2), dtype((0.03 * R) ** 2)
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def skssim(image, gt, R, dtype=np.float64):
    """structural_similarity of [3,H,W] arrays at data_range R, evaluated in `dtype` (the mean in float64, as scikit-image forms it)."""
    image, gt = np.asarray(image).astype(dtype), np.asarray(gt).astype(dtype)
    C, H, W = image.shape
    if H < WIN or W < WIN:
        raise ValueError("win_size exceeds image extent")
    means = []
    for c in range(C):
        X, Y = image[c], gt[c]
        f = lambda a: ndimage.uniform_filter(a, size=WIN)
        S = _s_map(f(X), f(Y), f(X * X), f(Y * Y), f(X * Y), R, dtype)
        means.append(S[PAD:H - PAD, PAD:W - PAD].mean(dtype=np.float64))
    return float(np.mean(means))


def skssim_windows(image, gt, R):
    """The same quantity without scipy: float64 means over every valid 7x7 window."""
    image, gt = np.asarray(image, np.float64), np.asarray(gt, np.float64)
    view = lambda a: np.lib.stride_tricks.sliding_window_view(a, (WIN, WIN), axis=(1, 2)).mean(axis=(3, 4))
    S = _s_map(view(image), view(gt), view(image * image), view(gt * gt), view(image * gt), R, np.float64)
    return float(S.mean(axis=(1, 2)).mean())


def both(image, gt, clamp=False, dtype=np.float64):
    """(SKSSIM, SKSSIM2) of float32 numpy [3,H,W] inputs."""
    image = mr.clamp01(image) if clamp else np.asarray(image)
    return skssim(image, gt, 1, dtype), skssim(image, gt, 2, dtype)


def pair(kind, H, W):
    """The inputs of a case: "pair" (metrics_ref.make_pair), "low" (the low-variance pair), "u8" / "u8_1.7" (make_pair's image against
    the decoded bytes through frames.gt_lut() / gt_lut(1.7))."""
    from ex4dgs_amd.frames import gt_lut
    if kind == "low":
        return sc.low_variance_pair(H, W)
    image, gt = mr.make_pair(H, W)
    if kind != "pair":
        gt = mr.looked_up(mr.make_bytes(H, W), gt_lut(1.7) if kind == "u8_1.7" else gt_lut())
    return image, gt


@functools.lru_cache(maxsize=None)
def case(kind, H, W, clamp):
    """The float64 reference (SKSSIM, SKSSIM2) of a case."""
    return both(*pair(kind, H, W), clamp)


def within_bar(row, ref, what=""):
    """row: the four values of a result row; ref: (SKSSIM, SKSSIM2) in float64.  Prints each figure, then asserts."""
    e = abs(row[0] - ref[0]), abs(row[1] - ref[1])
    print(what, f"SKSSIM {e[0]:.3g} SKSSIM2 {e[1]:.3g}")
    assert e[0] <= sc.TOL and e[1] <= sc.TOL, (what, e)
    assert row[2] == 0 and row[3] == 0, (what, list(row))
