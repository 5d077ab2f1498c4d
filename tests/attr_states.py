"""Shared by tests/golden/make_golden_attr_states.py, tests/test_cpu_attr_states.py and tests/test_gpu_attr_states.py: the layout of
tests/golden/model_getters_states.npz (keyframe states that training creates, captured from the reference's CGaussianModel in float32
AND float64), the bars the fused attribute kernels are held to on it, the branch census and the threshold margins.

Bars (per family, per tensor, per timestamp; the float32 reference is what everything is compared with):
  forward    1e-6 absolute
  gradients  1e-5 * max(1, |reference|inf over the finite entries of that family's rows)
  opposite families (keyframes q, -q and perturbations of it): the reference's own float32 result moves against its float64 result
      there (the blend of two nearly cancelling vectors is renormalised), so the bar is per row: the bar above plus
      NOISE_MARGIN = 4 times that row's max |reference float32 - reference float64| of the same tensor.  Both come from the fixture.
Entries where the reference is NaN or infinite must be NaN / the same infinity in the result; everything else must be finite.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_getters_states.npz")

FAMILIES = ("ordinary", "identical", "near_parallel", "opposite_exact", "opposite_perturbed", "window_conversion", "window_underflow",
            "window_clone_split")
OPPOSITE = ("opposite_exact", "opposite_perturbed")
# (duration, interval, time_pad), keyframe count and timestamps; time_shift = time_pad + interval ('cube' interpolation).
# "a": K = 35; t = 0, 3, 8, 137, 299 give delta = .2, .5, 0, .9, .1 with k = 1, 1, 2, 14, 31 and tau = 1.2, 1.5, 2.0, 14.9, 31.1; t = 308 is k = 32 = K-3.
# "b": K = 16; time_pad 3, so that the last usable keyframe index k = K-3 = 13 (t = 57) still passes the reference getters' own
#      assertion t <= duration + time_shift = 58 (with time_pad 2 it would need t = 58 > 57).  t = 4.5 gives delta = .5, tau = 2.5.
CONFIGS = {
    "a": dict(duration=300, interval=10, time_pad=2, K=35, timestamps=(0, 3, 8, 137, 299, 308)),
    "b": dict(duration=50, interval=5, time_pad=3, K=16, timestamps=(0, 4.5, 27, 57)),
}
VAR_PAD = 3
STATIC = ("_xyz", "_xyz_disp", "_rotation", "_opacity", "_scaling")
DYNAMIC = ("_xyz_motion", "_rotation_motion", "_opacity_motion", "_opacity_duration_center", "_opacity_duration_var", "_scaling_motion")
NAMES = STATIC + DYNAMIC                       # the feature tensors are a plain copy: checked bit for bit against torch.cat, not stored
OUTPUTS = ("xyz", "rot", "opa", "scl")
SLICED = {"_xyz_motion": (-1, 4), "_rotation_motion": (0, 2)}      # first keyframe relative to k, number of keyframes with a gradient

FWD_BAR = 1e-6
GRAD_BAR = 1e-5
NOISE_MARGIN = 4.0
THRESHOLD_MARGIN = 1e-6          # no float64 dot product this close to +-(1 - 1e-4)
HI, LO, FLOOR = 1 - 1e-4, -1 + 1e-4, 1e-4
CENSUS = ("clamped_high", "clamped_low", "clamp_inside", "psum_clamped", "fallback", "window_inside", "window_before", "window_after",
          "tie", "tau_on_centre", "overflow", "underflow")
MIN_ROWS_PER_BRANCH = 8
# The clamp of the weight sum can never bind: with omega in [acos(1-1e-4), pi - acos(1-1e-4)] and delta in [0, 1),
#   p0 + p1 = (sin((1-delta) omega) + sin(delta omega)) / sin(omega) = cos((1 - 2 delta) omega / 2) / cos(omega / 2) >= 1,
# so no input reaches `p_sum < 1e-4` (nor `acos < 1e-4`, `sin < 1e-4`): the census records 0 rows there and the tests assert that.
UNREACHABLE = ("psum_clamped",)


def time_index(cfg, t):
    c = CONFIGS[cfg]
    tp = t + c["time_pad"] + c["interval"]
    return int(tp // c["interval"]), (tp % c["interval"]) / c["interval"], tp / c["interval"]


def tkey(t):
    return f"t{t:g}"


def load():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def params(z, cfg, dtype=np.float32):
    return {n: z[f"{cfg}/param/{n}"].astype(dtype) for n in NAMES}


def weights(z, cfg, dtype=np.float32):
    return {k: z[f"{cfg}/weight/{k}"].astype(dtype) for k in OUTPUTS}


def family_rows(z, cfg):
    """{family: indices of its dynamic rows}."""
    fam = z[f"{cfg}/family"]
    return {name: np.nonzero(fam == i)[0] for i, name in enumerate(FAMILIES)}


def slice_grads(grads, cfg, t):
    """Dense keyframe gradients [Nd,K,C] -> the slices the fixture stores; asserts that everything outside them is exactly zero."""
    k = time_index(cfg, t)[0]
    out = dict(grads)
    for n, (first, count) in SLICED.items():
        g = np.asarray(grads[n])
        lo = k + first
        rest = np.delete(g, np.arange(lo, lo + count), axis=1)
        assert not rest.any() and not np.isnan(rest).any(), f"{n}: gradient outside keyframes {lo}..{lo + count - 1}"
        out[n] = g[:, lo:lo + count]
    return out


def _row_max(a):
    return a.reshape(a.shape[0], -1).max(axis=1) if a.shape[0] else np.zeros(0)


def check(z, cfg, t, outs, grads, scale=1.0, rows=None, static_rows=None):
    """Compares outputs (dict xyz/rot/opa/scl, static rows first) and gradients (dict by parameter name, keyframe gradients sliced) with
    the float32 reference of (cfg, t).  rows / static_rows: the fixture rows the compared rows were taken from (default: all, in order).
    Returns (worst, failures): worst[(family, tensor)] = (largest error, its bar, error / bar) and failures, a list of
    (family, tensor, fixture row (static rows as -1 - row), error, bar) for every row outside scale * bar or with NaN / infinity in a different place."""
    fam = z[f"{cfg}/family"]
    Ns_all = z[f"{cfg}/param/_xyz"].shape[0]
    rows = np.arange(fam.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64)
    static_rows = np.arange(Ns_all) if static_rows is None else np.asarray(static_rows, dtype=np.int64)
    key = f"{cfg}/{tkey(t)}"
    worst, failures = {}, []

    def compare(tensor, got, r32, r64, families, project_bar_rel, rowid):
        got = np.asarray(got)
        assert got.shape == r32.shape, (tensor, got.shape, r32.shape)
        finite = np.isfinite(r32)
        with np.errstate(invalid="ignore"):
            special_bad = np.where(finite, ~np.isfinite(got), ~((got == r32) | (np.isnan(got) & np.isnan(r32))))
        err = _row_max(np.where(finite, np.abs(got.astype(np.float64) - r32), 0.0))
        noise = _row_max(np.where(finite & np.isfinite(r64), np.abs(r32.astype(np.float64) - r64), 0.0))
        mag = np.where(finite, np.abs(r32), 0.0)
        for name, idx in families.items():
            if idx.size == 0:
                continue
            bar = (GRAD_BAR * max(1.0, float(mag[idx].max())) if project_bar_rel else FWD_BAR) * np.ones(idx.size)
            if name in OPPOSITE:
                bar = bar + NOISE_MARGIN * noise[idx]
            ratio = err[idx] / bar
            j = int(ratio.argmax())
            worst[(name, tensor)] = (float(err[idx][j]), float(bar[j]), float(ratio[j]))
            for i in np.nonzero(ratio > scale)[0]:
                failures.append((name, tensor, int(rowid[idx[i]]), float(err[idx][i]), float(bar[i])))
        failures.extend(("non-finite", tensor, int(rowid[i]), float("nan"), 0.0) for i in np.nonzero(_row_max(special_bad))[0])

    dyn_fams = {name: np.nonzero(fam[rows] == i)[0] for i, name in enumerate(FAMILIES)}
    static_fam = {"static": np.arange(static_rows.size)}
    all_rows = np.concatenate([static_rows, Ns_all + rows])
    for k in OUTPUTS:
        r32, r64 = z[f"{key}/{k}"][all_rows], z[f"{key}/f64/{k}"][all_rows]
        fams = dict(static_fam)
        fams.update({name: static_rows.size + idx for name, idx in dyn_fams.items()})
        compare(k, outs[k], r32, r64, fams, False, np.concatenate([-1 - static_rows, rows]))
    for n in NAMES:
        if grads is None or grads.get(n) is None:
            continue
        sel = static_rows if n in STATIC else rows
        compare(n, grads[n], z[f"{key}/grad/{n}"][sel], z[f"{key}/f64/grad/{n}"][sel], static_fam if n in STATIC else dyn_fams, True,
                -1 - static_rows if n in STATIC else rows)
    return worst, failures


def format_failures(failures, limit=12):
    return "; ".join(f"{f}/{n} row {r}: {e:.3g} > {b:.3g}" for f, n, r, e, b in failures[:limit]) + (f" (+{len(failures) - limit} more)" if len(failures) > limit else "")


# ---------------------------------------------------------------------------------------------- census and margins (float64 numpy)
def slerp_state(q1, q2, delta):
    """The decisions of the reference's slerp on float64 copies of two keyframes: raw dot product, the weight sum before its clamp and
    the L1 norm of the blend that the zero-vector fallback tests."""
    q1, q2 = np.asarray(q1, np.float64), np.asarray(q2, np.float64)
    v1 = q1 / np.linalg.norm(q1, axis=-1, keepdims=True)
    v2 = q2 / np.linalg.norm(q2, axis=-1, keepdims=True)
    raw = (v1 * v2).sum(-1)
    om = np.maximum(np.arccos(np.clip(raw, LO, HI)), FLOOR)
    s = np.maximum(np.sin(om), FLOOR)
    p0, p1 = np.sin((1 - delta) * om) / s, np.sin(delta * om) / s
    ps = np.maximum(p0 + p1, FLOOR)
    blend = np.abs(v1 * (p0 / ps)[:, None] + v2 * (p1 / ps)[:, None]).sum(-1)
    return raw, p0 + p1, blend


def census(P, cfg, t):
    """{branch: bool[Nd]} for the dynamic rows of parameter dict P at timestamp t, decided in float64 on the float32 parameters
    (the window tests on the float32 values themselves: they are comparisons of stored numbers with the float32 tau)."""
    k, delta, tau = time_index(cfg, t)
    q = P["_rotation_motion"]
    raw, ps_raw, blend = slerp_state(q[:, k], q[:, k + 1], delta)
    c = P["_opacity_duration_center"][:, :, 0].astype(np.float32)
    v = P["_opacity_duration_var"][:, :, 0].astype(np.float32)
    tau = np.float32(tau)
    after = (tau > c).any(1)
    sel = np.where(after, v[:, 1], v[:, 0])
    with np.errstate(over="ignore"):
        e = np.exp(sel.astype(np.float32))
    inside = (c[:, 0] - tau) * (c[:, 1] - tau) < 0
    return dict(clamped_high=raw > HI, clamped_low=raw < LO, clamp_inside=(raw >= LO) & (raw <= HI), psum_clamped=ps_raw < FLOOR,
                fallback=~(blend > FLOOR), window_inside=inside, window_before=~after & ~inside, window_after=after & ~inside,
                tie=c[:, 0] == c[:, 1], tau_on_centre=(c == tau).any(1), overflow=np.isinf(e), underflow=e == 0)


def margin_violations(P, cfg):
    """bool[Nd]: rows whose float64 dot product is within THRESHOLD_MARGIN of a clamp bound, whose weight sum is within it of its floor,
    or whose blend norm is within a factor 2 of the fallback threshold (a float32 evaluation could then take the other branch than the
    float64 one, and the fixture's own two precisions would disagree by a branch instead of by rounding), at any timestamp."""
    bad = np.zeros(P["_rotation_motion"].shape[0], bool)
    for t in CONFIGS[cfg]["timestamps"]:
        k, delta, _ = time_index(cfg, t)
        raw, ps_raw, blend = slerp_state(P["_rotation_motion"][:, k], P["_rotation_motion"][:, k + 1], delta)
        bad |= (np.abs(raw - HI) < THRESHOLD_MARGIN) | (np.abs(raw - LO) < THRESHOLD_MARGIN) | (np.abs(ps_raw - FLOOR) < THRESHOLD_MARGIN)
        bad |= (blend > FLOOR / 2) & (blend < FLOOR * 2)
    return bad


# ---------------------------------------------------------------------------------------------- the two CPU restatements
_FEATURE_SHAPES = {"_features_dc": (1, 3), "_features_rest": (15, 3), "_features_dc_motion": (1, 3), "_features_rest_motion": (15, 3)}


def with_features(P, fill=0.0):
    """P plus constant feature tensors (the fixture does not store features)."""
    full = dict(P)
    for n, s in _FEATURE_SHAPES.items():
        rows = P["_xyz_motion" if "motion" in n else "_xyz"].shape[0]
        full[n] = np.full((rows,) + s, fill, np.float32)
    return full


def run_oracle(P, W, cfg, t):
    """oracle/model_oracle.py (numpy float32) -> (outputs, sliced gradients) in the fixture's layout."""
    from oracle import model_oracle as mo
    c = CONFIGS[cfg]
    kw = dict(duration=c["duration"], interval=c["interval"], time_shift=c["time_pad"] + c["interval"], var_pad=VAR_PAD)
    full = with_features(P)
    with np.errstate(all="ignore"):
        o = mo.forward(full, t, **kw)
        N = o["means3D"].shape[0]
        g = mo.backward(full, t, dict(means3D=W["xyz"], rotations=W["rot"], opacities=W["opa"], scales=W["scl"],
                                      shs=np.zeros((N, 16, 3), np.float32)), **kw)
    outs = dict(xyz=o["means3D"], rot=o["rotations"], opa=o["opacities"], scl=o["scales"])
    return outs, slice_grads({n: g[n] for n in NAMES}, cfg, t)


def run_getters(P, W, cfg, t):
    """The torch getters of ex4dgs_amd.scene.DynamicGaussians + autograd on the CPU -> (outputs, sliced gradients)."""
    import torch
    from ex4dgs_amd.scene import DynamicGaussians
    c = CONFIGS[cfg]
    tp = {n: torch.tensor(v).requires_grad_(True) for n, v in with_features(P).items()}
    m = DynamicGaussians(tp, duration=c["duration"], interval=c["interval"], time_pad=c["time_pad"], var_pad=VAR_PAD)
    vals = dict(xyz=m.get_xyz_at_t(t), rot=m.get_rotation_at_t(t), opa=m.get_opacity_at_t(t), scl=m.get_scaling())
    loss = sum((vals[k] * torch.tensor(W[k])).sum() for k in OUTPUTS)
    grads = torch.autograd.grad(loss, [tp[n] for n in NAMES])
    return {k: v.detach().numpy() for k, v in vals.items()}, slice_grads({n: g.numpy() for n, g in zip(NAMES, grads)}, cfg, t)
