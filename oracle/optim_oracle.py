"""CPU oracle of the RAdam step -- TEST INFRASTRUCTURE ONLY (tests/, smoke, bench cpu legs).

The reference optimises with `torch.optim.RAdam(l, lr=0.001)` (scene/c_gaussian_model.py:449; stepped at train.py:250);
torch is a third-party dependency (environment.yml:10 pins pytorch=2.1.2) whose source is not under /root/reference, so
this restates its documented algorithm (torch.optim.RAdam docs; _single_tensor_radam op order) in numpy float32 with the
scalar coefficients in Python doubles.  Pinned by tests/golden/radam.npz = parameter trajectories of torch.optim.RAdam
itself (the torch installed in the build container, CPU) over 12 steps that cross the rho_t > 5 switch at step 6.

The float32 operations and their grouping are those of radam_update in ex4dgs_amd/csrc/ex4d_optim.hip (built without
contraction, every operation correctly rounded, denormals kept), the scalars those of its fill_coefficients: the kernel is
expected to give these BITS (tests/test_gpu_optim_edges.py), NaN sign and payload aside.
"""
import math
from collections import namedtuple

import numpy as np

f32 = np.float32
FLT_MAX = f32(3.402823466e+38)

Coefficients = namedtuple("Coefficients", "w1 beta2 w2 bc1 lr sqrt_bc2 rect eps rectified")


def radam_coefficients(step, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """The per-tensor scalars of one step as the kernel receives them: formed in Python doubles (math.sqrt where the host code
    calls std::sqrt, ** where it calls std::pow), cast to float32 where they meet a tensor.  rect is 0 when not rectified."""
    st = float(step)
    rho_inf = 2.0 / (1.0 - beta2) - 1.0
    bc1 = 1.0 - beta1 ** st
    bc2 = 1.0 - beta2 ** st
    rho_t = rho_inf - 2.0 * st * beta2 ** st / bc2
    rectified = rho_t > 5.0
    rect = math.sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t)) if rectified else 0.0
    return Coefficients(f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2), f32(bc1), f32(lr), f32(math.sqrt(bc2)), f32(rect), f32(eps),
                        bool(rectified))


def sanitize(g):
    """torch.nan_to_num with its defaults, as include/ex4d_optim.h defines the flag: NaN -> 0, then clamped to +-FLT_MAX."""
    g = np.where(np.isnan(g), f32(0), g).astype(f32)
    return np.minimum(np.maximum(g, -FLT_MAX), FLT_MAX)


def radam_step(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, nan_to_num=False):
    """One step, in place on float32 arrays p, m, v; `step` is the count after the increment.  Returns whether it was rectified."""
    c = radam_coefficients(step, lr, beta1, beta2, eps)
    if nan_to_num:
        g = sanitize(g)
    with np.errstate(all="ignore"):                  # the value-edge cases overflow and make NaN on purpose
        m += c.w1 * (g - m)
        v *= c.beta2
        v += (c.w2 * g) * g
        mhat = m / c.bc1
        if c.rectified:
            adaptive = c.sqrt_bc2 / (np.sqrt(v) + c.eps)
            p -= ((mhat * c.lr) * adaptive) * c.rect
        else:
            p -= mhat * c.lr
    return c.rectified


def dense_from_windows(rows, K, C, windows):
    """The dense float32 [rows, K, C] gradient of windows = [(first, block[rows, count, C]), ...]: zeros, plus the windows in index
    order, each clipped to the keyframes [0, K) (keyframe k takes block[:, k - first])."""
    dense = np.zeros((rows, K, C), f32)
    for first, block in windows:
        block = np.asarray(block, f32).reshape(rows, -1, C)
        lo, hi = max(0, first), min(K, first + block.shape[1])
        if lo < hi:
            dense[:, lo:hi] += block[:, lo - first:hi - first]
    return dense
