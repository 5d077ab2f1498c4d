"""numpy restatement of the reference's motion regularisers (train.py:155-168) and of their hand-derived adjoint, the CPU check of
ex4dgs_amd.regularizers / ex4d_radam_step_sliced_reg (include/ex4d_regularizers.h):

    static = mean_i        log(|_xyz_disp[i]| + 0.001)
    motion = mean_{i,k>=1} |_xyz_motion[i,0] - _xyz_motion[i,k]|
    rot    = mean_{i,k>=1} 1 - <r_k, r_{k-1}> / max(|r_k|, 1e-6) / max(|r_{k-1}|, 1e-6)

Every function takes `dtype` (np.float32: the arithmetic of the kernels, keyframe 0's sum in ascending k; np.float64: the reference
value the GPU tests compare against).  Pinned against the reference's own lines by tests/golden/regularizers.npz.
"""
import numpy as np


def _norm(x, dtype):
    x = x.astype(dtype)
    s = x[..., 0] * x[..., 0]
    for j in range(1, x.shape[-1]):
        s = s + x[..., j] * x[..., j]
    return np.sqrt(s)


def values(xyz_disp, xyz_motion, rotation_motion, dtype=np.float64):
    """The three unweighted means (0 for a mean over nothing)."""
    out = [dtype(0), dtype(0), dtype(0)]
    if xyz_disp is not None and xyz_disp.shape[0]:
        out[0] = np.log(_norm(xyz_disp, dtype) + dtype(0.001)).mean(dtype=dtype)
    if xyz_motion is not None and xyz_motion.shape[0] and xyz_motion.shape[1] > 1:
        p = xyz_motion.astype(dtype)
        out[1] = _norm(p[:, :1] - p[:, 1:], dtype).mean(dtype=dtype)
    if rotation_motion is not None and rotation_motion.shape[0] and rotation_motion.shape[1] > 1:
        r = rotation_motion.astype(dtype)
        n = np.maximum(_norm(r, dtype), dtype(1e-6))
        out[2] = (dtype(1) - (r[:, 1:] * r[:, :-1]).sum(-1, dtype=dtype) / n[:, 1:] / n[:, :-1]).mean(dtype=dtype)
    return out


def mean_abs_terms(xyz_disp, xyz_motion, rotation_motion):
    """mean |term| of the three sums in float64: the scale the 1e-6 bar of the loss values is relative to."""
    f8 = np.float64
    out = [0.0, 0.0, 0.0]
    if xyz_disp.shape[0]:
        out[0] = float(np.abs(np.log(_norm(xyz_disp, f8) + 0.001)).mean())
    if xyz_motion.shape[0] and xyz_motion.shape[1] > 1:
        p = xyz_motion.astype(f8)
        out[1] = float(_norm(p[:, :1] - p[:, 1:], f8).mean())
        r = rotation_motion.astype(f8)
        n = np.maximum(_norm(r, f8), 1e-6)
        out[2] = float(np.abs(1.0 - (r[:, 1:] * r[:, :-1]).sum(-1) / n[:, 1:] / n[:, :-1]).mean())
    return out


def loss(xyz_disp, xyz_motion, rotation_motion, weights, dtype=np.float64):
    v = values(xyz_disp, xyz_motion, rotation_motion, dtype)
    return sum(dtype(w) * x for w, x in zip(weights, v))


def _coefs(Ns, Nd, K, weights, dtype):
    cs = dtype(weights[0] / Ns) if Ns else dtype(0)
    pairs = Nd * (K - 1)
    return cs, (dtype(weights[1] / pairs) if pairs else dtype(0)), (dtype(weights[2] / pairs) if pairs else dtype(0))


def _safe_div(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(b == 0, np.zeros_like(a), a / np.where(b == 0, np.ones_like(b), b))


def grad_static(xyz_disp, coef, dtype=np.float32):
    d = xyz_disp.astype(dtype)
    n = _norm(d, dtype)
    s = _safe_div(coef / (n + dtype(0.001)), n)              # 0 where |d| = 0 (torch's norm backward)
    return d * s[:, None]


def grad_motion(xyz_motion, coef, dtype=np.float32):
    """dL/dp_k = -u_k for k >= 1, dL/dp_0 = sum_k u_k (ascending k), u_k = coef (p_0 - p_k) / |p_0 - p_k| (0 where they coincide)."""
    p = xyz_motion.astype(dtype)
    g = np.zeros_like(p)
    K = p.shape[1]
    if K < 2 or p.shape[0] == 0:
        return g
    d = p[:, :1] - p[:, 1:]
    u = d * _safe_div(np.full(d.shape[:2], coef, dtype), _norm(d, dtype))[..., None]
    g[:, 1:] = -u
    for k in range(K - 1):
        g[:, 0] += u[:, k]
    return g


def _rot_pair(a, b, coef, dtype):
    """d/da of -coef <a,b> / max(|a|,1e-6) / max(|b|,1e-6)"""
    na, nb = _norm(a, dtype), _norm(b, dtype)
    ca, cb = np.maximum(na, dtype(1e-6)), np.maximum(nb, dtype(1e-6))
    dot = a[..., 0] * b[..., 0]
    for j in range(1, 4):
        dot = dot + a[..., j] * b[..., j]
    inv = (coef / ca) / cb
    live = na >= dtype(1e-6)                                 # clamp_min passes no gradient to a norm below the clamp
    t = np.where(live, _safe_div((dot * inv) / ca, np.where(live, na, np.ones_like(na))), np.zeros_like(na))
    return a * t[..., None] - b * inv[..., None]


def grad_rot(rotation_motion, coef, dtype=np.float32):
    r = rotation_motion.astype(dtype)
    g = np.zeros_like(r)
    if r.shape[1] < 2 or r.shape[0] == 0:
        return g
    g[:, 1:] += _rot_pair(r[:, 1:], r[:, :-1], coef, dtype)      # the pair with k-1 first
    g[:, :-1] += _rot_pair(r[:, :-1], r[:, 1:], coef, dtype)     # then the pair with k+1
    return g


def grads(xyz_disp, xyz_motion, rotation_motion, weights, dtype=np.float32):
    """Gradients of loss(): (g_xyz_disp, g_xyz_motion, g_rotation_motion)."""
    Nd, K = xyz_motion.shape[0], xyz_motion.shape[1]
    cs, cm, cr = _coefs(xyz_disp.shape[0], Nd, K, weights, dtype)
    return grad_static(xyz_disp, cs, dtype), grad_motion(xyz_motion, cm, dtype), grad_rot(rotation_motion, cr, dtype)


def grad_scales(xyz_disp, xyz_motion, rotation_motion, weights):
    """Per entry, in float64: A = the sum of the magnitudes of the terms added into the entry with their parts UN-cancelled, and n =
    the number of terms.  The float32 bar of the GPU test is (16 + n) 2^-24 A."""
    f8 = np.float64
    Nd, K = xyz_motion.shape[0], xyz_motion.shape[1]
    cs, cm, cr = (abs(c) for c in _coefs(xyz_disp.shape[0], Nd, K, weights, f8))
    d = xyz_disp.astype(f8)
    n = _norm(d, f8)
    A_s = np.abs(d) * _safe_div(cs / (n + 0.001), n)[:, None]
    p = xyz_motion.astype(f8)
    A_m, n_m = np.zeros_like(p), np.ones(p.shape, np.int64)
    if K > 1 and Nd:
        dd = p[:, :1] - p[:, 1:]
        u = np.abs(dd) * _safe_div(np.full(dd.shape[:2], cm), _norm(dd, f8))[..., None]
        A_m[:, 1:] = u
        A_m[:, 0] = u.sum(1)
        n_m[:, 0] = K - 1
    r = rotation_motion.astype(f8)
    A_r, n_r = np.zeros_like(r), np.ones(r.shape, np.int64)
    if K > 1 and Nd:
        def pair(a, b):
            na, nb = _norm(a, f8), _norm(b, f8)
            ca, cb = np.maximum(na, 1e-6), np.maximum(nb, 1e-6)
            first = np.abs(b) / (ca * cb)[..., None]
            second = np.where((na >= 1e-6)[..., None],
                              (np.abs(a * b).sum(-1) / (ca * ca * cb))[..., None] * np.abs(a) * _safe_div(np.ones_like(na), na)[..., None], 0.0)
            return cr * (first + second)
        A_r[:, 1:] += pair(r[:, 1:], r[:, :-1])
        A_r[:, :-1] += pair(r[:, :-1], r[:, 1:])
        n_r[:, 1:-1] = 2
    return (A_s, np.ones(A_s.shape, np.int64)), (A_m, n_m), (A_r, n_r)


def scatter_windows(shape, windows, dtype=np.float32):
    """Dense keyframe gradient [rows,K,C] of windows [(first, grad [rows,count,C]), ...], added in index order."""
    g = np.zeros(shape, dtype)
    for first, w in windows:
        g[:, first:first + w.shape[1]] += w.astype(dtype)
    return g
