"""Generates tests/golden/model_getters_states.npz by importing the REFERENCE's CGaussianModel on the CPU (like make_golden.py: third-party
modules stubbed, Tensor.cuda the identity): the per-frame getters and their autograd gradients on the keyframe states that training
creates and that seeded random parameters never reach, in float32 AND with the same reference code run in float64 (parameters cast up).

Two configurations (tests/attr_states.py CONFIGS): (duration, interval, time_pad) = (300, 10, 2) with K = 35 and (50, 5, 3) with K = 16; the
last timestamp of each lies past the duration and reaches the last usable keyframe index k = K-3.  Dynamic row families, shuffled so
that a wrong row index shows (every row tagged in `<cfg>/family`, names in `families`):
  ordinary            as tests/golden/param_gen.py
  identical           all K keyframe quaternions equal, unnormalised, norms 0.3..3   (scene/c_gaussian_model.py:1189, a Gaussian turned dynamic)
  near_parallel       constant angle between neighbouring keyframes, 0.1x..10x acos(1 - 1e-4) = 0.01414, keyframe norms 0.5..2
  opposite_exact      keyframes q, -q, q, ... bit-exact negations
  opposite_perturbed  keyframes (-1)^j q_j with the angle between q_j and q_j+1 0.1x..10x 0.01414: the lower clamp bound from both sides
  window_conversion   centres / log-widths by the formulas of :1180-1187 for t_min over [0, duration]: clamped centres, log-widths up to
                      duration + time_pad (exp overflows float32 above 88.7), a centre exactly on tau for some rows
  window_underflow    log-widths in [-150, -88]: exp underflows to 0 or to a subnormal, the width is var_min / 2.36
  window_clone_split  log-widths exactly 2, centres clamped as :944-945 / :1006-1007 leave them: c0 == c1 on either bound and inside,
                      tau exactly on a centre, c0 > c1
Rows too close to a decision threshold (tests/attr_states.py margin_violations), and rows on which this repository's two CPU restatements
(oracle/model_oracle.py, the torch getters of ex4dgs_amd/scene.py) do not sit within HALF of the bar the GPU tests use, are redrawn:
no test excludes a row.  The file also holds the branch census per timestamp (`<cfg>/<t>/census/<branch>`, bool per dynamic row).

Run:  python tests/golden/make_golden_attr_states.py      (needs the reference checkout; byte-stable from run to run)
"""
import io
import math
import os
import sys
import zipfile

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from make_golden import _stub_modules  # noqa: E402
from tests import attr_states as st  # noqa: E402

COUNTS = {
    "a": dict(static=12, ordinary=24, identical=24, near_parallel=24, opposite_exact=16, opposite_perturbed=24, window_conversion=24,
              window_underflow=12, window_clone_split=24),
    "b": dict(static=4, ordinary=4, identical=4, near_parallel=4, opposite_exact=4, opposite_perturbed=4, window_conversion=4,
              window_underflow=2, window_clone_split=8),
}
EXACT_TAUS = {"a": (1.5, 2.0), "b": (2.5, 7.0)}        # tau of t = 3, 8 and of t = 4.5, 27: exact in float32
THRESHOLD_ANGLE = math.acos(1 - 1e-4)
SEED = 20240


def _unit_pair(rng):
    a = rng.standard_normal(4)
    a /= np.linalg.norm(a)
    b = rng.standard_normal(4)
    b -= a * (a @ b)
    b /= np.linalg.norm(b)
    return a, b


def _stratified(rng, slot, n, lo, hi):
    """The slot-th of n strata of [lo, hi), at a random place inside it: both sides of a threshold in the middle are populated."""
    return lo + (hi - lo) * (slot + rng.random()) / n


def draw_row(cfg, family, slot, n, rng):
    """One dynamic row: dict of float32 arrays without the leading row dimension."""
    c = st.CONFIGS[cfg]
    K, dur, itv, pad = c["K"], c["duration"], c["interval"], c["time_pad"]
    shift = pad + itv
    N = rng.standard_normal
    row = dict(_xyz_motion=np.cumsum(0.2 * N((K, 3)), 0), _rotation_motion=N((K, 4)), _opacity_motion=N(1),
               _opacity_duration_center=np.sort(2 + rng.random((2, 1)) * (K - 5), 0), _opacity_duration_var=N((2, 1)),
               _scaling_motion=0.3 * N(3) - 2)
    j = np.arange(K)[:, None]
    if family == "identical":
        a, _ = _unit_pair(rng)
        row["_rotation_motion"] = np.repeat((a * math.exp(_stratified(rng, slot, n, math.log(0.3), math.log(3.0))))[None], K, 0)
    elif family in ("near_parallel", "opposite_perturbed"):
        a, b = _unit_pair(rng)
        ang = THRESHOLD_ANGLE * 10 ** _stratified(rng, slot, n, -1.0, 1.0)
        q = (np.cos(j * ang) * a + np.sin(j * ang) * b) * np.exp(rng.uniform(math.log(0.5), math.log(2.0), (K, 1)))
        row["_rotation_motion"] = q * (-1.0) ** j if family == "opposite_perturbed" else q
    elif family == "opposite_exact":
        a, _ = _unit_pair(rng)
        q = (a * math.exp(_stratified(rng, slot, n, math.log(0.3), math.log(3.0)))).astype(np.float32)
        row["_rotation_motion"] = np.where(j % 2 == 0, q, -q)
    elif family == "window_conversion":
        # c_gaussian_model.py:1180-1187 in float32 tensor arithmetic; t_min is the timestamp of the smallest error, an integer frame
        special = {"a": (6.0, 6.0, 16.0, 16.0), "b": (1.0,)}[cfg]        # (t_min / 2 + shift) / interval exactly on the tau of t = 3, 8 (a) / 4.5 (b)
        t_min = special[slot] if slot < len(special) else float(round(_stratified(rng, slot, n, 0, dur)))
        t = torch.full((1, 1), t_min)
        centre = torch.stack([torch.ones(1, 1) * (t * 1 / 2 + shift) / itv, torch.ones(1, 1) * ((dur + t.clamp_min(0) * 1) / 2 + shift) / itv],
                             dim=1).clamp((0 + shift + 1) / itv, (shift + dur - 1) / itv)
        var = torch.stack([torch.ones(1, 1) * (t + pad), torch.ones(1, 1) * (dur - t + pad)], dim=1)
        row["_opacity_duration_center"], row["_opacity_duration_var"] = centre[0].numpy(), var[0].numpy()
    elif family == "window_underflow":
        # exp() is exactly 0 in float32 below -103.3 and subnormal between that and -87.3: two rows in three are drawn from the first range
        row["_opacity_duration_var"] = -(104 + 46 * rng.random((2, 1))) if slot % 3 else -(88 + 15 * rng.random((2, 1)))
    elif family == "window_clone_split":
        lo, hi = np.float32((shift + 1) / itv), np.float32((shift + dur - 1) / itv)
        exact = EXACT_TAUS[cfg]
        kind = slot % 8
        inner = np.float32(rng.uniform(lo + 1, hi - 1))
        if kind == 0:
            c0 = c1 = lo
        elif kind == 1:
            c0 = c1 = hi
        elif kind == 2:
            c0 = c1 = inner
        elif kind == 3:
            c0 = c1 = np.float32(exact[(slot // 8) % 2])
        elif kind == 4:
            c0, c1 = np.float32(exact[(slot // 8) % 2]), min(inner + np.float32(3), hi)
        elif kind == 5:
            c0, c1 = lo, np.float32(exact[(slot // 8) % 2])
        else:
            # a parent's centres jittered by a third of their distance and clamped (:944-945); kind 6 keeps the draws that cross
            parent = np.sort(2 + rng.random(2) * (K - 5)).astype(np.float32)
            length = max(abs(parent[1] - parent[0]) / 3, 2 / itv)
            c0, c1 = np.clip(parent + length * N(2), lo, hi).astype(np.float32)
            if kind == 6 and c0 < c1:
                c0, c1 = c1, c0
        row["_opacity_duration_center"] = np.array([[c0], [c1]], np.float32)
        row["_opacity_duration_var"] = np.full((2, 1), 2.0)
    return {k: np.asarray(v, np.float32) for k, v in row.items()}


def static_rows(Ns, rng):
    N = rng.standard_normal
    return dict(_xyz=N((Ns, 3)), _xyz_disp=0.1 * N((Ns, 3)), _rotation=N((Ns, 4)), _opacity=N((Ns, 1)), _scaling=0.3 * N((Ns, 3)) - 2)


def capture(P, W, cfg, dtype):
    """Outputs and autograd gradients of the reference's getters at every timestamp of cfg, parameters and weights cast to dtype."""
    from scene.c_gaussian_model import CGaussianModel
    c = st.CONFIGS[cfg]
    pc = CGaussianModel(3, c["duration"], c["interval"], c["time_pad"], interp_type="cube", rot_interp_type="slerp", var_pad=st.VAR_PAD)
    assert pc.time_shift == c["time_pad"] + c["interval"]
    for n in st.NAMES:
        setattr(pc, n, torch.tensor(P[n]).to(dtype).requires_grad_(True))
    out = {}
    for t in c["timestamps"]:
        vals = dict(xyz=pc.get_xyz_at_t(t), rot=pc.get_rotation_at_t(t), opa=pc.get_opacity_at_t(t), scl=pc.get_scaling())
        loss = sum((vals[k] * torch.tensor(W[k]).to(dtype)).sum() for k in st.OUTPUTS)
        grads = torch.autograd.grad(loss, [getattr(pc, n) for n in st.NAMES])
        grads = st.slice_grads({n: g.numpy() for n, g in zip(st.NAMES, grads)}, cfg, t)
        sub = "" if dtype == torch.float32 else "f64/"
        for k, v in vals.items():
            assert v.dtype == dtype
            out[f"{cfg}/{st.tkey(t)}/{sub}{k}"] = v.detach().numpy()
        for n, g in grads.items():
            out[f"{cfg}/{st.tkey(t)}/{sub}grad/{n}"] = g
        k = st.time_index(cfg, t)[0]
        for n, (first, count) in st.SLICED.items():        # which keyframes the stored slices of the keyframe gradients are
            out[f"{cfg}/{st.tkey(t)}/grad_slices/{n}"] = np.arange(k + first, k + first + count)
    return out


def build_config(cfg, rng):
    c, counts = st.CONFIGS[cfg], COUNTS[cfg]
    layout = [(f, i, counts[f]) for f in st.FAMILIES for i in range(counts[f])]
    layout = [layout[i] for i in rng.permutation(len(layout))]
    rows = [draw_row(cfg, f, i, n, rng) for f, i, n in layout]
    Ns, Nd = counts["static"], len(layout)
    S = {k: v.astype(np.float32) for k, v in static_rows(Ns, rng).items()}
    N = Ns + Nd
    W = {k: rng.standard_normal((N, d)).astype(np.float32) for k, d in zip(st.OUTPUTS, (3, 4, 1, 3))}
    redrawn = 0
    for attempt in range(50):
        P = dict(S)
        P.update({n: np.stack([r[n] for r in rows]) for n in st.DYNAMIC})
        out = {f"{cfg}/family": np.array([st.FAMILIES.index(f) for f, _, _ in layout], np.int8)}
        out.update({f"{cfg}/param/{n}": P[n] for n in st.NAMES})
        out.update({f"{cfg}/weight/{k}": W[k] for k in st.OUTPUTS})
        out.update(capture(P, W, cfg, torch.float32))
        out.update(capture(P, W, cfg, torch.float64))
        bad = st.margin_violations(P, cfg)
        if bad.any():
            print(f"  config {cfg} round {attempt}: too close to a threshold: rows", np.nonzero(bad)[0].tolist())
        for t in c["timestamps"]:
            for run in (st.run_oracle, st.run_getters):
                outs, grads = run(P, W, cfg, t)
                for fam, tensor, row, err, bar in st.check(out, cfg, t, outs, grads, scale=0.5)[1]:
                    assert row >= 0, ("a static row misses half its bar", fam, tensor, row, err, bar)
                    print(f"  config {cfg} round {attempt}: {run.__name__} t={t:g} {fam}/{tensor} row {row}: {err:.3g} > half of {bar:.3g}")
                    bad[row] = True
        if not bad.any():
            break
        for i in np.nonzero(bad)[0]:
            f, slot, n = layout[i]
            rows[i] = draw_row(cfg, f, slot, n, rng)
            redrawn += 1
    else:
        raise RuntimeError("rows still violate the margins after 50 rounds of redrawing")
    for t in c["timestamps"]:
        for name, mask in st.census(P, cfg, t).items():
            out[f"{cfg}/{st.tkey(t)}/census/{name}"] = mask
    return out, redrawn


def save(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same bytes on every run."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED, 9)


def main():
    _stub_modules()
    torch.set_default_dtype(torch.float32)
    rng = np.random.default_rng(SEED)
    out = {"families": np.array(st.FAMILIES), "seed": np.array(SEED)}
    for cfg in st.CONFIGS:
        arrays, redrawn = build_config(cfg, rng)
        out.update(arrays)
        fam = arrays[f"{cfg}/family"]
        print(f"config {cfg}: {fam.size} dynamic rows", {f: int((fam == i).sum()) for i, f in enumerate(st.FAMILIES)}, f"{redrawn} redrawn")
        for t in st.CONFIGS[cfg]["timestamps"]:
            print(f"  t={t:g}", {b: int(arrays[f'{cfg}/{st.tkey(t)}/census/{b}'].sum()) for b in st.CENSUS})
    path = os.path.join(OUT, "model_getters_states.npz")
    save(path, out)
    print("model_getters_states.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
