"""numpy float32 restatement of ex4d_densify_stats_merge (include/ex4d_densify.h): the left fold, in rank order, of the ranks' pending
statistics blocks into the running total of a group -- and the inputs that take every branch of it.  The checker of the HIP kernel
(tests/test_gpu_stats_merge.py, tests/test_gpu_dist_density.py); its own properties are pinned by tests/test_cpu_stats_merge.py.

A block is [9, n] float32, rows in EX4D_STAT_* order; pending is [W, 9, n], block w from rank w.
"""
import numpy as np

ROWS = 9
GRAD_ACCUM, DENOM, ERROR_ACCUM, SSIM_ACCUM, ERROR_DENOM, MAX_RADII, MIN_RADII, ERROR_MIN, ERROR_MIN_T = range(ROWS)
SUM_ROWS = (GRAD_ACCUM, DENOM, ERROR_ACCUM, SSIM_ACCUM, ERROR_DENOM)
INIT = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1000.0, 1000.0, -1.0], np.float32)


def neutral(n, W=None):
    """A block (W blocks) at the initial values."""
    b = np.repeat(INIT[:, None], n, axis=1)
    return b.copy() if W is None else np.repeat(b[None], W, axis=0).copy()


def fold(total, pending):
    """The total after it took pending[0], pending[1], ... in that order (a new array)."""
    t = np.array(total, np.float32, copy=True)
    pending = np.asarray(pending, np.float32)
    assert t.shape[0] == ROWS and pending.shape[1:] == t.shape
    with np.errstate(all="ignore"):
        for d in pending:
            for r in SUM_ROWS:
                t[r] = t[r] + d[r]                                           # float32 add
            t[MAX_RADII] = np.where(d[MAX_RADII] > t[MAX_RADII], d[MAX_RADII], t[MAX_RADII])
            t[MIN_RADII] = np.where(d[MIN_RADII] < t[MIN_RADII], d[MIN_RADII], t[MIN_RADII])
            take = t[ERROR_MIN] > d[ERROR_MIN]                               # strict: a tie keeps what is there, a NaN is never taken
            t[ERROR_MIN_T] = np.where(take, d[ERROR_MIN_T], t[ERROR_MIN_T])
            t[ERROR_MIN] = np.where(take, d[ERROR_MIN], t[ERROR_MIN])
    return t


KINDS = 12


def make_case(W, n, seed=0):
    """(total [9, n], pending [W, 9, n]) of plausible statistics in which column i is of kind i % KINDS -- together every branch of the
    fold: 0, 11 plain values; 1 every rank neutral; 2 all ranks tie on an error minimum below the total's, with different timestamps (rank 0's
    must win); 3 the ranks tie with the total's minimum (the total keeps its timestamp); 4 a NaN in a sum row of one rank; 5 a NaN error
    minimum in one rank's block (never taken) beside a smaller finite one in another; 6 a NaN error minimum in the total (never replaced);
    7 +inf and -inf meeting in a sum row, inf radii; 8 -0.0 in the deltas' sum rows and in the max / min rows; 9 NaN radii in a delta and in
    the total; 10 only the last rank has seen the Gaussian."""
    rng = np.random.default_rng(1000 * W + 7 * n + seed)
    f = lambda *s: rng.random(s, dtype=np.float32)

    def block(*lead):
        b = np.empty(lead + (ROWS, n), np.float32)
        b[..., GRAD_ACCUM, :] = f(*lead, n) * 3e-3
        b[..., DENOM, :] = rng.integers(0, 40, lead + (n,))
        b[..., ERROR_ACCUM, :] = f(*lead, n) * 5 - 1                        # the error channels' ratio may be negative
        b[..., SSIM_ACCUM, :] = f(*lead, n) * 7
        b[..., ERROR_DENOM, :] = rng.integers(0, 40, lead + (n,))
        b[..., MAX_RADII, :] = rng.integers(0, 300, lead + (n,))
        b[..., MIN_RADII, :] = rng.integers(1, 1001, lead + (n,))
        b[..., ERROR_MIN, :] = np.round(f(*lead, n) * 8) / 8                # coarse: ties between ranks happen by themselves too
        b[..., ERROR_MIN_T, :] = rng.integers(0, 300, lead + (n,))
        return b

    total, pending = block(), block(W)
    kind = np.arange(n) % KINDS
    last = W - 1
    for r in range(ROWS):
        pending[:, r, kind == 1] = INIT[r]
        pending[:last, r, kind == 10] = INIT[r]
    k = kind == 2
    total[ERROR_MIN, k] = 0.75
    pending[:, ERROR_MIN, k] = 0.25
    pending[:, ERROR_MIN_T, k] = 100.0 + np.arange(W, dtype=np.float32)[:, None]
    k = kind == 3
    total[ERROR_MIN, k], total[ERROR_MIN_T, k] = 0.5, 7.0
    pending[:, ERROR_MIN, k] = 0.5
    pending[:, ERROR_MIN_T, k] = 200.0 + np.arange(W, dtype=np.float32)[:, None]
    k = kind == 4
    pending[W // 2, GRAD_ACCUM, k] = np.nan
    pending[0, SSIM_ACCUM, k] = np.nan
    k = kind == 5
    total[ERROR_MIN, k] = 0.875
    pending[:, ERROR_MIN, k] = 1.0
    pending[0, ERROR_MIN, k], pending[0, ERROR_MIN_T, k] = np.nan, 55.0
    if W > 1:
        pending[last, ERROR_MIN, k], pending[last, ERROR_MIN_T, k] = 0.125, 66.0
    k = kind == 6
    total[ERROR_MIN, k], total[ERROR_MIN_T, k] = np.nan, 9.0
    k = kind == 7
    pending[0, ERROR_ACCUM, k] = np.inf
    pending[last, ERROR_ACCUM, k] = -np.inf if W > 1 else np.inf
    total[SSIM_ACCUM, k] = -np.inf
    pending[0, MAX_RADII, k] = np.inf
    pending[last, MIN_RADII, k] = -np.inf
    k = kind == 8
    for r in SUM_ROWS + (MAX_RADII, MIN_RADII):
        pending[:, r, k] = -0.0
    total[MAX_RADII, k] = 0.0
    total[MIN_RADII, k] = 0.0
    k = kind == 9
    pending[0, MAX_RADII, k] = np.nan
    pending[last, MIN_RADII, k] = np.nan
    total[MAX_RADII, k & ((np.arange(n) // KINDS) % 2 == 1)] = np.nan
    return total, pending
