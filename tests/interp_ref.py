"""Shared by tests/golden/make_golden_interp.py, tests/test_cpu_interp.py and tests/test_gpu_interp.py: the layout of
tests/golden/model_getters_interp.npz (the reference's CGaussianModel under interp_type 'linear' and 'pchip', captured in float32 AND
float64), a numpy restatement of the two position interpolators and of their adjoints in either precision, the branch census of the
pchip slopes, and the comparison at the bars of tests/attr_states.py (FWD_BAR 1e-6 absolute; GRAD_BAR 1e-5 * max(1, |reference|inf of
the family); NaN and infinities in the same places).  Everything but the dynamic positions (slerp, opacity window, scales, static rows)
is oracle/model_oracle.py with the configuration's own time shift.

pchip per component (utils/interpolations.py:65-77): a = y[k+1]-y[k], b = y[k]-y[k-1], s = y[k+1]-y[k-1] (its own subtraction),
m_k = a*b > 0 ? (a*b)/s*2 : 0, m_k1 likewise one keyframe on; p = h00 y[k] + h10 m_k + h01 y[k+1] + h11 m_k1.  The adjoint is what
autograd forms: the quotient is differentiated where the comparison drops it, so s == 0 gives NaN on the keyframes it touches.
"""
import os

import numpy as np

from tests import attr_states as st

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_getters_interp.npz")

FWD_BAR, GRAD_BAR, VAR_PAD = st.FWD_BAR, st.GRAD_BAR, st.VAR_PAD
NAMES, STATIC, DYNAMIC, OUTPUTS = st.NAMES, st.STATIC, st.DYNAMIC, st.OUTPUTS
INTERP_CODE = {"cube": 0, "linear": 1, "pchip": 2}

# (duration, interval, time_pad); time_shift = time_pad for linear, time_pad + interval for pchip; K = ceil((duration + time_shift +
# 2 time_pad + 1) / interval) + 3.  The reference's getters assert -time_shift <= t <= duration + time_shift.
#   lin_b   shift 3, K 15: t = -3 (k 0, delta 0), 0 (k 0, .6), 4.5 (k 1, .5), 27 (k 6, 0), 53 (k 11, .2: the last index the assertion admits)
#   lin_a   shift 2, K 34 (N3V; cube has shift 12, K 35): t = -2 (k 0, 0), 0 (k 0, .2), 8 (k 1, 0), 137.5 (k 13, .95), 302 (k 30, .4)
#   pchip_b shift 8, K 16: t = -3 (k 1, the first index with a keyframe before it, delta 0), 0 (k 1, .6), 4.5 (k 2, .5), 27 (k 7, 0),
#           58 (k 13 = K-3, .2: the last the assertion admits)
CONFIGS = {
    "lin_b": dict(interp="linear", duration=50, interval=5, time_pad=3, time_shift=3, K=15, timestamps=(-3, 0, 4.5, 27, 53)),
    "lin_a": dict(interp="linear", duration=300, interval=10, time_pad=2, time_shift=2, K=34, timestamps=(-2, 0, 8, 137.5, 302)),
    "pchip_b": dict(interp="pchip", duration=50, interval=5, time_pad=3, time_shift=8, K=16, timestamps=(-3, 0, 4.5, 27, 58)),
}
# Track families of _xyz_motion (per component; signs of the steps y[j+1]-y[j]); the patterns hold at every keyframe index, the phase
# is the row's slot (+ the component for `mixed`), so every timestamp sees every branch:
#   ordinary      random walk
#   monotone      all steps of one sign: both slopes kept
#   mixed         step signs + + - repeating, phase slot + component: the three components of a row take the three branches
#                 {m_k dropped, m_k1 dropped, both dropped}
#   zigzag        alternating signs, unequal sizes: both dropped, s != 0
#   flat          every other step exactly 0: a == 0 or b == 0 with s != 0 (finite gradients)
#   constant      all keyframes equal: s == 0 for both slopes, NaN on all four keyframes
#   pingpong      u, v, u, v, ...: y[k+1] == y[k-1] != y[k] for both slopes, NaN on all four
#   pingpong_one  u, v, u, w, ...: exactly one of the two slopes has s == 0, NaN on three keyframes
#   ratio         monotone with step sizes 1, r, 1, r, ..., log10 r stratified over [-6, 0): |a|/|b| from 1e-6 to 1e6
FAMILIES = ("ordinary", "monotone", "mixed", "zigzag", "flat", "constant", "pingpong", "pingpong_one", "ratio")
CENSUS = ("both_kept", "mk_dropped", "mk1_dropped", "both_dropped", "a_zero", "b_zero", "s_zero_both", "s_zero_one")
ROW_CENSUS = ("three_branches", "nan_gradient")
MIN_ROWS_PER_BRANCH = 8
SUBNORMAL = float(np.finfo(np.float32).tiny)


def shapes(cfg):
    """(first keyframe of the position window relative to k, its length)."""
    return (0, 2) if CONFIGS[cfg]["interp"] == "linear" else (-1, 4)


def sliced(cfg):
    return {"_xyz_motion": shapes(cfg), "_rotation_motion": (0, 2)}


def time_index(cfg, t):
    c = CONFIGS[cfg]
    tp = t + c["time_shift"]
    return int(tp // c["interval"]), (tp % c["interval"]) / c["interval"], tp / c["interval"]


def weights_of(cfg, t, dtype=np.float32):
    """The four host scalars the kernels get in h00, h10, h01, h11 (Python doubles, cast)."""
    d = time_index(cfg, t)[1]
    if CONFIGS[cfg]["interp"] == "linear":
        w = (1 - d, 0.0, d, 0.0)
    else:
        w = (2 * d ** 3 - 3 * d ** 2 + 1, d ** 3 - 2 * d ** 2 + d, -2 * d ** 3 + 3 * d ** 2, d ** 3 - d ** 2)
    return tuple(dtype(x) for x in w)


tkey = st.tkey


def load():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def params(z, cfg, dtype=np.float32):
    return {n: z[f"{cfg}/param/{n}"].astype(dtype) for n in NAMES}


def weights(z, cfg, dtype=np.float32):
    return {k: z[f"{cfg}/weight/{k}"].astype(dtype) for k in OUTPUTS}


def slice_grads(grads, cfg, t):
    """Dense keyframe gradients [Nd,K,C] -> the window the fixture stores; everything outside it must be exactly zero."""
    k = time_index(cfg, t)[0]
    out = dict(grads)
    for n, (first, count) in sliced(cfg).items():
        g = np.asarray(grads[n])
        lo = k + first
        rest = np.delete(g, np.arange(lo, lo + count), axis=1)
        assert not rest.any() and not np.isnan(rest).any(), f"{n}: gradient outside keyframes {lo}..{lo + count - 1}"
        out[n] = g[:, lo:lo + count]
    return out


# ---------------------------------------------------------------------------------------------- the position interpolators, numpy
def _slope(before, at, after, two):
    a, b, s = after - at, at - before, after - before
    p = a * b
    with np.errstate(all="ignore"):
        q = p / s * two
    return np.where(p > 0, q, np.zeros_like(q)), (a, b, s, p)


def position_forward(y, k, w, interp):
    """Dynamic positions [Nd,3] from keyframes y [Nd,K,3] in y's precision, in the reference's operation order; w = weights_of(...)."""
    h00, h10, h01, h11 = (y.dtype.type(x) for x in w)
    if interp == "linear":
        return y[:, k] * h00 + y[:, k + 1] * h01
    assert interp == "pchip"
    two = y.dtype.type(2)
    mk, _ = _slope(y[:, k - 1], y[:, k], y[:, k + 1], two)
    mk1, _ = _slope(y[:, k], y[:, k + 1], y[:, k + 2], two)
    return h00 * y[:, k] + h10 * mk + h01 * y[:, k + 1] + h11 * mk1


def _slope_adjoint(state, keep_grad, two):
    a, b, s, p = state
    with np.errstate(all="ignore"):
        g_q = np.where(p > 0, keep_grad, np.zeros_like(keep_grad)) * two
        g_p = g_q / s
        g_s = -g_q * ((p / s) / s)
        return g_p * b, g_p * a, g_s          # gradients of a, b, s


def position_backward(y, k, w, g, interp):
    """The gradient window [Nd, 2 or 4, 3] of dL/d(dynamic positions) = g [Nd,3], as autograd forms it."""
    h00, h10, h01, h11 = (y.dtype.type(x) for x in w)
    g = g.astype(y.dtype)
    if interp == "linear":
        return np.stack([g * h00, g * h01], 1)
    two = y.dtype.type(2)
    _, s0 = _slope(y[:, k - 1], y[:, k], y[:, k + 1], two)
    _, s1 = _slope(y[:, k], y[:, k + 1], y[:, k + 2], two)
    ga0, gb0, gs0 = _slope_adjoint(s0, h10 * g, two)
    ga1, gb1, gs1 = _slope_adjoint(s1, h11 * g, two)
    with np.errstate(invalid="ignore"):
        return np.stack([-gb0 - gs0, h00 * g + (gb0 - ga0) + (-gb1 - gs1), h01 * g + (ga0 + gs0) + (gb1 - ga1), ga1 + gs1], 1)


def run_restatement(P, W, cfg, t):
    """(outputs, sliced gradients) in the fixture's layout, float32: the positions by the functions above, the rest by model_oracle."""
    from oracle import model_oracle as mo
    c = CONFIGS[cfg]
    kw = dict(duration=c["duration"], interval=c["interval"], time_shift=c["time_shift"], var_pad=VAR_PAD)
    full = st.with_features(P)
    Ns = P["_xyz"].shape[0]
    k = time_index(cfg, t)[0]
    w = weights_of(cfg, t)
    with np.errstate(all="ignore"):
        o = mo.forward(full, t, **kw)
        N = o["means3D"].shape[0]
        g = mo.backward(full, t, dict(means3D=W["xyz"], rotations=W["rot"], opacities=W["opa"], scales=W["scl"],
                                      shs=np.zeros((N, 16, 3), np.float32)), **kw)
    xyz = o["means3D"].copy()
    xyz[Ns:] = position_forward(P["_xyz_motion"], k, w, c["interp"])
    outs = dict(xyz=xyz, rot=o["rotations"], opa=o["opacities"], scl=o["scales"])
    grads = {n: g[n] for n in NAMES}
    first, count = shapes(cfg)
    dense = np.zeros_like(P["_xyz_motion"])
    dense[:, k + first:k + first + count] = position_backward(P["_xyz_motion"], k, w, W["xyz"][Ns:], c["interp"])
    grads["_xyz_motion"] = dense
    return outs, slice_grads(grads, cfg, t)


def run_getters(P, W, cfg, t):
    """The torch getters of ex4dgs_amd.scene.DynamicGaussians + autograd on the CPU -> (outputs, sliced gradients)."""
    import torch
    from ex4dgs_amd.scene import DynamicGaussians
    c = CONFIGS[cfg]
    tp = {n: torch.tensor(v).requires_grad_(True) for n, v in st.with_features(P).items()}
    m = DynamicGaussians(tp, duration=c["duration"], interval=c["interval"], time_pad=c["time_pad"], var_pad=VAR_PAD, interp_type=c["interp"])
    vals = dict(xyz=m.get_xyz_at_t(t), rot=m.get_rotation_at_t(t), opa=m.get_opacity_at_t(t), scl=m.get_scaling())
    loss = sum((vals[k] * torch.tensor(W[k])).sum() for k in OUTPUTS)
    grads = torch.autograd.grad(loss, [tp[n] for n in NAMES])
    return {k: v.detach().numpy() for k, v in vals.items()}, slice_grads({n: g.numpy() for n, g in zip(NAMES, grads)}, cfg, t)


# ---------------------------------------------------------------------------------------------- census
def census(P, cfg, t):
    """({branch: bool[Nd,3]}, {row branch: bool[Nd]}) of the pchip slopes at timestamp t, on the float32 keyframes themselves."""
    y = P["_xyz_motion"].astype(np.float32)
    k = time_index(cfg, t)[0]
    two = np.float32(2)
    _, (a0, b0, s0, p0) = _slope(y[:, k - 1], y[:, k], y[:, k + 1], two)
    _, (a1, b1, s1, p1) = _slope(y[:, k], y[:, k + 1], y[:, k + 2], two)
    k0, k1 = p0 > 0, p1 > 0
    comp = dict(both_kept=k0 & k1, mk_dropped=~k0 & k1, mk1_dropped=k0 & ~k1, both_dropped=~k0 & ~k1 & (s0 != 0) & (s1 != 0),
                a_zero=(a0 == 0) & (s0 != 0), b_zero=(b0 == 0) & (s0 != 0), s_zero_both=(s0 == 0) & (s1 == 0), s_zero_one=(s0 == 0) ^ (s1 == 0))
    kind = np.where(k0 & k1, 0, np.where(~k0 & k1, 1, np.where(k0 & ~k1, 2, 3)))
    three = (kind[:, 0] != kind[:, 1]) & (kind[:, 1] != kind[:, 2]) & (kind[:, 0] != kind[:, 2])
    return comp, dict(three_branches=three, nan_gradient=((s0 == 0) | (s1 == 0)).any(1))


def subnormal_products(P, cfg):
    """bool[Nd]: rows with a product a*b that is not zero but inside float32's subnormal range, at any timestamp and component (the
    comparison a*b > 0 is then at the mercy of flush-to-zero)."""
    y = P["_xyz_motion"].astype(np.float32)
    bad = np.zeros(y.shape[0], bool)
    for t in CONFIGS[cfg]["timestamps"]:
        k = time_index(cfg, t)[0]
        for j in (k, k + 1):
            with np.errstate(under="ignore"):
                p = (y[:, j + 1] - y[:, j]) * (y[:, j] - y[:, j - 1])
            bad |= ((p != 0) & (np.abs(p) < SUBNORMAL)).any(1)
    return bad


# ---------------------------------------------------------------------------------------------- comparison
def _row_max(a):
    return a.reshape(a.shape[0], -1).max(axis=1) if a.shape[0] else np.zeros(0)


def check(z, cfg, t, outs, grads, scale=1.0, rows=None, static_rows=None):
    """Outputs (dict xyz/rot/opa/scl, static rows first) and gradients (dict by name, keyframe gradients as windows; None entries are
    skipped) against the float32 reference of (cfg, t).  Returns (worst, failures) like attr_states.check: worst[(family, tensor)] =
    (error, bar, ratio); failures = [(family, tensor, fixture row (static: -1 - row), error, bar)], NaN / infinity mismatches included."""
    fam = z[f"{cfg}/family"]
    Ns_all = z[f"{cfg}/param/_xyz"].shape[0]
    rows = np.arange(fam.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64)
    static_rows = np.arange(Ns_all) if static_rows is None else np.asarray(static_rows, dtype=np.int64)
    key = f"{cfg}/{tkey(t)}"
    worst, failures = {}, []

    def compare(tensor, got, r32, families, relative, rowid):
        got = np.asarray(got)
        assert got.shape == r32.shape, (tensor, got.shape, r32.shape)
        finite = np.isfinite(r32)
        with np.errstate(invalid="ignore"):
            special_bad = np.where(finite, ~np.isfinite(got), ~((got == r32) | (np.isnan(got) & np.isnan(r32))))
            err = _row_max(np.where(finite & np.isfinite(got), np.abs(got.astype(np.float64) - r32), 0.0))
        mag = np.where(finite, np.abs(r32), 0.0)
        for name, idx in families.items():
            if idx.size == 0:
                continue
            bar = GRAD_BAR * max(1.0, float(mag[idx].max())) if relative else FWD_BAR
            ratio = err[idx] / bar
            j = int(ratio.argmax())
            worst[(name, tensor)] = (float(err[idx][j]), float(bar), float(ratio[j]))
            failures.extend((name, tensor, int(rowid[idx[i]]), float(err[idx][i]), float(bar)) for i in np.nonzero(ratio > scale)[0])
        failures.extend(("non-finite", tensor, int(rowid[i]), float("nan"), 0.0) for i in np.nonzero(_row_max(special_bad))[0])

    dyn_fams = {name: np.nonzero(fam[rows] == i)[0] for i, name in enumerate(FAMILIES)}
    static_fam = {"static": np.arange(static_rows.size)}
    all_rows = np.concatenate([static_rows, Ns_all + rows])
    for k in OUTPUTS:
        fams = dict(static_fam)
        fams.update({name: static_rows.size + idx for name, idx in dyn_fams.items()})
        compare(k, outs[k], z[f"{key}/{k}"][all_rows], fams, False, np.concatenate([-1 - static_rows, rows]))
    for n in NAMES:
        if grads is None or grads.get(n) is None:
            continue
        sel = static_rows if n in STATIC else rows
        compare(n, grads[n], z[f"{key}/grad/{n}"][sel], static_fam if n in STATIC else dyn_fams, True, -1 - static_rows if n in STATIC else rows)
    return worst, failures


format_failures = st.format_failures
