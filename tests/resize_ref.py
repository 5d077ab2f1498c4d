"""PIL's 8-bit Image.resize restated in numpy (include/ex4d_loss.h, "RESIZING"): the coefficient tables in Python floats (IEEE doubles,
one rounding per operation: nothing here can fuse), the two passes in int64.  tests/test_cpu_resize.py holds it to Pillow's own
bytes (tests/golden/resize.npz, and the installed Pillow where there is one); the GPU tests compare the kernels with it."""
import math

import numpy as np

BITS = 22
FILTERS = {"bilinear": 2, "bicubic": 3, "box": 4}          # PIL's resample numbers = EX4D_FILTER_*


def _bilinear(x):
    x = -x if x < 0.0 else x
    return 1.0 - x if x < 1.0 else 0.0


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bicubic(x):
    a = -0.5
    x = -x if x < 0.0 else x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_FILTER = {"bilinear": (_bilinear, 1.0), "box": (_box, 0.5), "bicubic": (_bicubic, 2.0)}


def coefficients(n_in, n_out, resample="bilinear"):
    """(ksize, xmin [out], n [out], k [out, ksize] int64) of one axis."""
    f, s = _FILTER[resample]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    sup = s * fs
    ksize = int(math.ceil(sup)) * 2 + 1
    ss = 1.0 / fs
    xmins, ns, ks = np.zeros(n_out, np.int64), np.zeros(n_out, np.int64), np.zeros((n_out, ksize), np.int64)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - sup + 0.5), 0)               # int() truncates towards zero, as (int) does
        xmax = min(int(center + sup + 0.5), n_in)
        n = xmax - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        xmins[xx], ns[xx] = xmin, n
        for x, v in enumerate(w):
            ks[xx, x] = int(v * float(1 << BITS) + 0.5) if v >= 0 else int(v * float(1 << BITS) - 0.5)
    return ksize, xmins, ns, ks


def table_words(n_in, n_out, resample="bilinear"):
    """The words ex4d_resize_u8_table writes: ksize, then per output element xmin, n and ksize coefficients."""
    ksize, xmins, ns, ks = coefficients(n_in, n_out, resample)
    body = np.concatenate([xmins[:, None], ns[:, None], ks], axis=1)
    return np.concatenate([[ksize], body.reshape(-1)]).astype(np.int32)


def accumulate(src, n_out, resample="bilinear"):
    """One pass along axis 0 of src (uint8 [in, ...]): the un-shifted, un-clamped int64 accumulators [out, ...]."""
    ksize, xmins, ns, ks = coefficients(src.shape[0], n_out, resample)
    s64 = src.astype(np.int64)
    acc = np.full((n_out,) + src.shape[1:], 1 << (BITS - 1), np.int64)
    for xx in range(n_out):
        lo, n = int(xmins[xx]), int(ns[xx])
        k = ks[xx, :n].reshape((n,) + (1,) * (src.ndim - 1))
        acc[xx] += (s64[lo:lo + n] * k).sum(axis=0)
    return acc


def _pass(src, n_out, resample):
    acc = accumulate(src, n_out, resample)
    assert np.abs(acc).max() < 2 ** 31, "the kernels accumulate in int32"
    return np.clip(acc >> BITS, 0, 255).astype(np.uint8)


def resize(src, out_hw, resample="bilinear", parts=False):
    """src uint8 [H_in, W_in, C] -> uint8 [H_out, W_out, C]: horizontal pass, byte intermediate, vertical pass; a pass whose sizes are
    equal is skipped.  parts=True also returns the intermediate."""
    H_out, W_out = out_hw
    mid = src
    if src.shape[1] != W_out:
        mid = np.ascontiguousarray(_pass(np.ascontiguousarray(src.transpose(1, 0, 2)), W_out, resample).transpose(1, 0, 2))
    out = mid if mid.shape[0] == H_out else _pass(mid, H_out, resample)
    out = np.ascontiguousarray(out).copy()
    return (out, mid) if parts else out
