"""Shapes and inputs of the fused L1 + SSIM loss's tiling-edge sweep, shared by tests/test_gpu_loss_edges.py (HIP kernel
against the float64 oracle) and tests/test_cpu_oracle_and_host.py (float32 oracle against the float64 oracle: the bars must be
reachable on exactly these inputs).

The numbers restate the layout of ex4dgs_amd/csrc/ex4d_loss.hip: a workgroup owns a strip of SW = 64 output columns (+ 10 halo
columns) and walks a segment of SEG = 48 output rows, RPI = 4 image rows per iteration through a ring of 16 rows; channels run
in groups of CG = 3; the strips x segments work items are dealt to 8 XCDs and the grid is padded to a multiple of 8."""
import numpy as np

SW, SEG, CG = 64, 48, 3

# heights: one segment of 1 .. 11 rows, both sides of SEG, last segments of 1 .. 11 rows, and every value of (rows_out + 10) % 4
# in the last segment (rows_out = H - 48 k: 1, 4, 5, 6, 10, 11 and 37 .. 48)
HEIGHTS = (1, 5, 6, 10, 11, 37, 38, 39, 43, 44, 47, 48, 49, 52, 53, 54, 58, 59, 96, 97, 106)
# widths: narrower than the halo, both sides of a strip, a second strip narrower than / as wide as / wider than the halo
WIDTHS = (1, 5, 6, 11, 63, 64, 65, 69, 70, 74, 127, 128, 129, 138)
CHANNELS = (1, 2, 4, 5, 6, 7)                    # besides 3: a short only group, two groups (short / full last), three groups
CHANNEL_SHAPES = ((49, 65), (5, 64), (97, 129))
# work-item counts 1, 7, 8, 9, 17 (twice: 17 strips, 17 segments): the XCD map with and without padded workgroups
WORK_ITEM_SHAPES = ((3, 40, 50), (3, 30, 400), (3, 49, 256), (3, 100, 190), (3, 20, 1030), (3, 769, 10))
WORK_ITEMS = (1, 7, 8, 9, 17, 17)

LAMBDAS = (0.2, 0.7)

# the bars of _check_loss (tests/test_gpu_parity.py) for input that is not flat
TOL_LOSS, TOL_L1, TOL_SSIM, TOL_GRAD_REL, TOL_GRAD_ABS = 1e-6, 1e-6, 1e-5, 1e-5, 1e-9


def work_items(H, W):
    return ((W + SW - 1) // SW) * ((H + SEG - 1) // SEG)


def sweep_shapes():
    """Every (C, H, W) of the sweep, in a fixed order, without repeats."""
    out = [(3, H, W) for H in HEIGHTS for W in WIDTHS]
    out += [(C, H, W) for C in CHANNELS for (H, W) in CHANNEL_SHAPES]
    out += list(WORK_ITEM_SHAPES)
    assert len(set(out)) == len(out)
    return out


def make_pair(shape):
    """(image, gt) of test_fused_loss_vs_oracle_shapes: uniform gt, image = clip(gt + 0.15 n), one exact zero of x - y."""
    rng = np.random.default_rng(sum(shape))
    gt = rng.random(shape, dtype=np.float32)
    image = np.clip(gt + 0.15 * rng.standard_normal(shape), 0, 1).astype(np.float32)
    image[0, 0, 0] = gt[0, 0, 0]                   # |x - y| has a zero: sign(0) = 0 like torch.abs
    return image, gt


def errors(got, ref):
    """Achieved errors of dict(loss, l1_errors, ssim_errors, grad) `got` against the float64 oracle's `ref`; the gradient's as a
    multiple of its bar TOL_GRAD_REL * gmax + TOL_GRAD_ABS (relative to gmax alone it is meaningless at image == gt, gmax ~ 0)."""
    gmax = float(np.abs(ref["grad"]).max())
    d = lambda k: float(np.abs(np.asarray(got[k], np.float64) - ref[k]).max())
    return dict(loss=abs(float(got["loss"]) - ref["loss"]), l1_errors=d("l1_errors"), ssim_errors=d("ssim_errors"),
                grad=d("grad"), grad_bar=TOL_GRAD_REL * gmax + TOL_GRAD_ABS, gmax=gmax)


def assert_within_bars(e, scale=1.0, what=""):
    assert e["loss"] < scale * TOL_LOSS, (what, "loss", e)
    assert e["l1_errors"] <= scale * TOL_L1, (what, "l1_errors", e)
    assert e["ssim_errors"] <= scale * TOL_SSIM, (what, "ssim_errors", e)
    assert e["grad"] <= scale * e["grad_bar"], (what, "grad", e)
