"""Shapes and inputs of the scikit-image SSIM call's tiling-edge cases (include/ex4d_loss.h: ex4d_frame_skssim / _u8), shared by
tests/test_cpu_skssim.py (a float32 evaluation against the float64 reference: the bar must be reachable on exactly these inputs) and
tests/test_gpu_skssim.py (the HIP kernel against the float64 reference).

The numbers restate the layout of frame_skssim_kernel in ex4dgs_amd/csrc/ex4d_loss.hip: strips of SW = 64 output columns and segments
of SEG = 48 output rows tile the OUTPUT domain (H - 6) x (W - 6); a workgroup reads SW + 6 image columns and rows_out + 6 image rows,
RPI = 4 image rows per iteration; the strips x segments work items are dealt to 8 XCDs and the grid is padded to a multiple of 8."""
import numpy as np

from tests import loss_cases

SW, SEG, RPI, HALO, WIN = 64, 48, 4, 3, 7
TOL = loss_cases.TOL_LOSS            # 1e-6 absolute: the bar the project holds the mean SSIM of frame_metrics to


def work_items(H, W):
    return ((W - 2 * HALO + SW - 1) // SW) * ((H - 2 * HALO + SEG - 1) // SEG)


def blocks(H, W):
    return 8 * ((work_items(H, W) + 7) // 8)


def last_rows_out(H):
    Ho = H - 2 * HALO
    return Ho - SEG * ((Ho - 1) // SEG)


SMALLEST = ((WIN, WIN), (WIN, 30), (30, WIN))                         # one position; one output row; one output column
STRIP_EDGE = ((9, SW + 2 * HALO), (9, SW + 2 * HALO + 1))             # output width exactly 64 and 65 (W = 70, 71)
SEGMENT_EDGE = ((SEG + 2 * HALO, 20), (SEG + 2 * HALO + 1, 20))       # output height exactly one segment and one more (H = 54, 55)
NARROW_STRIP_W = SW + 2 * HALO + 2                                    # W = 72: a second strip of 2 output columns, narrower than the halo
# one height per value of (rows of the last segment + 6) % RPI, two segments, with the narrow second strip
REMAINDER = tuple((SEG + 2 * HALO + r, NARROW_STRIP_W) for r in (2, 3, 4, 5))
# 1, 7, 8, 9, 17 (strips), 17 (segments) work items: the XCD map with and without padded workgroups
WORK_ITEM_SHAPES = ((40, 50), (12, 2 * HALO + 6 * SW + 5), (60, 2 * HALO + 3 * SW + 1), (106, 196), (10, 2 * HALO + 16 * SW + 2),
                    (2 * HALO + 16 * SEG + 1, 12))
WORK_ITEMS = (1, 7, 8, 9, 17, 17)
ODD = ((53, 139),)
TRANSPOSED = (71, 61)
SHAPES = SMALLEST + STRIP_EDGE + SEGMENT_EDGE + REMAINDER + WORK_ITEM_SHAPES + ODD + (TRANSPOSED, TRANSPOSED[::-1])
LOW_VARIANCE_SHAPE = (53, 139)
assert len(set(SHAPES)) == len(SHAPES)
assert tuple(work_items(H, W) for H, W in WORK_ITEM_SHAPES) == WORK_ITEMS
assert sorted((last_rows_out(H) + 2 * HALO) % RPI for H, _ in REMAINDER) == [0, 1, 2, 3]
assert all(H - 2 * HALO > SEG and 0 < W - 2 * HALO - SW < HALO for H, W in REMAINDER)
assert all(H >= WIN and W >= WIN for H, W in SHAPES)


def low_variance_pair(H, W):
    """A piecewise-constant ground truth (16 x 16 blocks) and the image = gt + noise of sigma 0.002: where uxx - ux^2 cancels worst."""
    rng = np.random.default_rng(H * 7 + W)
    coarse = rng.random((3, (H + 15) // 16, (W + 15) // 16), dtype=np.float32) * np.float32(0.8) + np.float32(0.1)
    gt = np.ascontiguousarray(np.repeat(np.repeat(coarse, 16, axis=1), 16, axis=2)[:, :H, :W])
    image = (gt + np.float32(0.002) * rng.standard_normal((3, H, W)).astype(np.float32)).astype(np.float32)
    return image, gt
