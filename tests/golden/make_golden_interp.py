"""Generates tests/golden/model_getters_interp.npz by importing the REFERENCE's CGaussianModel on the CPU (like make_golden_attr_states.py:
third-party modules stubbed, Tensor.cuda the identity) with interp_type 'linear' and 'pchip': the per-frame getters and their autograd
gradients of all parameters, in float32 AND with the same reference code run in float64 (parameters cast up).

Configurations, timestamps, track families and the census: tests/interp_ref.py.  Rows are shuffled and tagged (`<cfg>/family`).  Rows
with a product a*b inside float32's subnormal range, and rows on which this repository's two CPU restatements (tests/interp_ref.py,
the torch getters of ex4dgs_amd/scene.py) do not sit within HALF of the bar the GPU tests use, are redrawn: no test excludes a row.

Run:  python tests/golden/make_golden_interp.py      (needs the reference checkout; byte-stable from run to run)
"""
import math
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from make_golden import _stub_modules  # noqa: E402
from make_golden_attr_states import save, static_rows  # noqa: E402
from tests import interp_ref as ir  # noqa: E402

COUNTS = {
    "lin_b": dict(static=8, ordinary=24, monotone=4, mixed=6, zigzag=4, flat=4, constant=8, pingpong=4, pingpong_one=4, ratio=6),
    "lin_a": dict(static=4, ordinary=24, monotone=0, mixed=0, zigzag=0, flat=0, constant=8, pingpong=0, pingpong_one=0, ratio=0),
    "pchip_b": dict(static=8, ordinary=16, monotone=16, mixed=24, zigzag=8, flat=16, constant=8, pingpong=8, pingpong_one=16, ratio=24),
}
SEED = 20251


def draw_track(family, slot, n, K, rng):
    """_xyz_motion [K,3] of one row."""
    j = np.arange(K)[:, None]
    c = np.arange(3)[None, :]
    size = 0.05 + 0.3 * rng.random((K, 3))
    sign = rng.choice([-1.0, 1.0], (1, 3))
    start = rng.standard_normal((1, 3))
    if family == "ordinary":
        steps = 0.2 * rng.standard_normal((K, 3))
    elif family == "monotone":
        steps = sign * size
    elif family == "mixed":
        steps = sign * size * np.where((j + slot + c) % 3 == 2, -1.0, 1.0)
    elif family == "zigzag":
        steps = sign * size * (-1.0) ** j
    elif family == "flat":
        steps = sign * size * ((j + slot) % 2 == 0)
    elif family == "constant":
        return np.repeat(start, K, 0).astype(np.float32)
    elif family in ("pingpong", "pingpong_one"):
        u, v, w = (rng.standard_normal((1, 3)).astype(np.float32) for _ in range(3))
        w = np.where(w == v, w + 1, w)
        third = w if family == "pingpong_one" else v
        jj = (j + slot) % 4
        return np.where(jj % 2 == 0, u, np.where(jj == 1, v, third)).astype(np.float32)
    elif family == "ratio":
        r = 10 ** (-6 * (1 - (slot + rng.random()) / n))
        steps = sign * np.where((j + slot) % 2 == 0, 1.0, r) * (0.5 + rng.random((K, 3)))
    else:
        raise KeyError(family)
    track = start + np.cumsum(steps, 0) - steps          # y[0] = start; y[j+1] - y[j] = steps[j]
    if family == "flat":                                 # exact repeats: the zero step must survive the cast
        track = track.astype(np.float32)
        flat = np.nonzero(((np.arange(K - 1) + slot) % 2 != 0))[0]
        track[flat + 1] = track[flat]
    return track.astype(np.float32)


def draw_row(cfg, family, slot, n, rng):
    K = ir.CONFIGS[cfg]["K"]
    N = rng.standard_normal
    row = dict(_xyz_motion=draw_track(family, slot, n, K, rng), _rotation_motion=N((K, 4)), _opacity_motion=N(1),
               _opacity_duration_center=np.sort(2 + rng.random((2, 1)) * (K - 5), 0), _opacity_duration_var=N((2, 1)),
               _scaling_motion=0.3 * N(3) - 2)
    return {k: np.asarray(v, np.float32) for k, v in row.items()}


def capture(P, W, cfg, dtype):
    from scene.c_gaussian_model import CGaussianModel
    c = ir.CONFIGS[cfg]
    pc = CGaussianModel(3, c["duration"], c["interval"], c["time_pad"], interp_type=c["interp"], rot_interp_type="slerp", var_pad=ir.VAR_PAD)
    assert pc.time_shift == c["time_shift"]
    assert c["K"] == math.ceil((c["duration"] + pc.time_shift + c["time_pad"] * 2 + 1) / c["interval"]) + 3
    for n in ir.NAMES:
        setattr(pc, n, torch.tensor(P[n]).to(dtype).requires_grad_(True))
    out = {}
    for t in c["timestamps"]:
        vals = dict(xyz=pc.get_xyz_at_t(t), rot=pc.get_rotation_at_t(t), opa=pc.get_opacity_at_t(t), scl=pc.get_scaling())
        loss = sum((vals[k] * torch.tensor(W[k]).to(dtype)).sum() for k in ir.OUTPUTS)
        grads = torch.autograd.grad(loss, [getattr(pc, n) for n in ir.NAMES])
        grads = ir.slice_grads({n: g.numpy() for n, g in zip(ir.NAMES, grads)}, cfg, t)
        sub = "" if dtype == torch.float32 else "f64/"
        for k, v in vals.items():
            assert v.dtype == dtype
            out[f"{cfg}/{ir.tkey(t)}/{sub}{k}"] = v.detach().numpy()
        for n, g in grads.items():
            out[f"{cfg}/{ir.tkey(t)}/{sub}grad/{n}"] = g
    return out


def build_config(cfg, rng):
    c, counts = ir.CONFIGS[cfg], COUNTS[cfg]
    layout = [(f, i, counts[f]) for f in ir.FAMILIES for i in range(counts[f])]
    layout = [layout[i] for i in rng.permutation(len(layout))]
    rows = [draw_row(cfg, f, i, n, rng) for f, i, n in layout]
    Ns, Nd = counts["static"], len(layout)
    S = {k: v.astype(np.float32) for k, v in static_rows(Ns, rng).items()}
    W = {k: rng.standard_normal((Ns + Nd, d)).astype(np.float32) for k, d in zip(ir.OUTPUTS, (3, 4, 1, 3))}
    redrawn = 0
    for attempt in range(50):
        P = dict(S)
        P.update({n: np.stack([r[n] for r in rows]) for n in ir.DYNAMIC})
        out = {f"{cfg}/family": np.array([ir.FAMILIES.index(f) for f, _, _ in layout], np.int8)}
        out.update({f"{cfg}/param/{n}": P[n] for n in ir.NAMES})
        out.update({f"{cfg}/weight/{k}": W[k] for k in ir.OUTPUTS})
        out.update(capture(P, W, cfg, torch.float32))
        out.update(capture(P, W, cfg, torch.float64))
        bad = ir.subnormal_products(P, cfg) if c["interp"] == "pchip" else np.zeros(Nd, bool)
        if bad.any():
            print(f"  config {cfg} round {attempt}: subnormal products: rows", np.nonzero(bad)[0].tolist())
        for t in c["timestamps"]:
            for run in (ir.run_restatement, ir.run_getters):
                outs, grads = run(P, W, cfg, t)
                for fam, tensor, row, err, bar in ir.check(out, cfg, t, outs, grads, scale=0.5)[1]:
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
        raise RuntimeError("rows still miss their bars after 50 rounds of redrawing")
    if c["interp"] == "pchip":
        for t in c["timestamps"]:
            comp, row = ir.census(P, cfg, t)
            for name, mask in {**comp, **row}.items():
                out[f"{cfg}/{ir.tkey(t)}/census/{name}"] = mask
    return out, redrawn


def main():
    _stub_modules()
    torch.set_default_dtype(torch.float32)
    rng = np.random.default_rng(SEED)
    out = {"families": np.array(ir.FAMILIES), "seed": np.array(SEED)}
    for cfg in ir.CONFIGS:
        arrays, redrawn = build_config(cfg, rng)
        out.update(arrays)
        fam = arrays[f"{cfg}/family"]
        print(f"config {cfg}: {fam.size} dynamic rows", {f: int((fam == i).sum()) for i, f in enumerate(ir.FAMILIES)}, f"{redrawn} redrawn")
        if ir.CONFIGS[cfg]["interp"] == "pchip":
            for t in ir.CONFIGS[cfg]["timestamps"]:
                print(f"  t={t:g}", {b: arrays[f'{cfg}/{ir.tkey(t)}/census/{b}'].sum(0).tolist() for b in ir.CENSUS + ir.ROW_CENSUS})
    path = os.path.join(OUT, "model_getters_interp.npz")
    save(path, out)
    print("model_getters_interp.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
