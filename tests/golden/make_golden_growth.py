"""Generates tests/golden/growth.npz and growth.json by importing the REFERENCE's CGaussianModel on CPU (like make_golden_densify.py:
third-party modules stubbed, Tensor.cuda the identity, device= stripped from torch.zeros / torch.ones and, for expand_duration,
torch.arange) and driving its own extract_dynamic_points_from_static, expand_duration, adjust_temp_opa, mark_error and
get_errorneous_timestamp.

Every model is seeded, takes one real RAdam step (non-zero moments and step counts) and two iterations of the train.py:199-216
statistics block before the call.  Cases (K = 35 unless said; `extract` has Ns = 48, Nd = 12, `first` Ns = 48, the three
selection cases Ns = 40, Nd = 2; the others Ns = 4, Nd = 8, the early-outs Nd = 2: the file stays under the size limit for a fixture):
  extract        extraction into an existing dynamic set, percentile 0.8
  first          the first extraction: Nd = 0, duration 5 (so max_dur = 5 and K = 6), percentile 0.9
  motion         motion_thres * extent selects rows below the threshold
  minmotion      min_motion_thres * extent rejects rows above the threshold
  unseen         error_min_timestamp < 0 rejects rows above the threshold
  early_short / early_static / early_fits        expand_duration through each early-out
  expand         a real expansion, K 35 -> 38 (avg = 4), centres on both sides of the new end and of the old end
  expand_small   K 5 -> 7 (avg = K - 2 = 3)
  adjust         adjust_temp_opa: centres on both sides of both bands, vars on both sides of 0.5 and 1
The script ASSERTS that every visible row's score, recomputed in float64, is farther than 1e-5 (relative) from the float64 threshold,
so the selection is decided with margin and the tests demand it exactly.
Run:  python tests/golden/make_golden_growth.py      (needs the reference checkout)
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden import REF, _stub_modules  # noqa: E402
from make_golden_densify import D_STATS, S_STATS, _iteration, _record  # noqa: E402

CAM = (0.3, -0.2, 2.5)


def _model(Ns, Nd, seed, duration=300, K=None):
    from arguments import OptimizationParams
    from scene.c_gaussian_model import CGaussianModel
    g = torch.Generator().manual_seed(seed)
    R = lambda *s: torch.randn(*s, generator=g)
    pc = CGaussianModel(3, duration, 10, 2, interp_type="cube", rot_interp_type="slerp")
    if K is None:
        K = math.ceil((duration + pc.time_shift + 2 * pc.time_pad + 1) / pc.interval) + 3
    P = dict(_xyz=R(Ns, 3), _xyz_disp=0.1 * R(Ns, 3), _rotation=R(Ns, 4), _opacity=2.5 * R(Ns, 1) - 1, _scaling=math.log(0.01) + 0.8 * R(Ns, 3),
             _features_dc=R(Ns, 1, 3), _features_rest=0.2 * R(Ns, 15, 3))
    if Nd > 0:
        pc.keyframe_num = K
        P.update(_xyz_motion=torch.cumsum(0.2 * R(Nd, K, 3), 1), _rotation_motion=R(Nd, K, 4), _opacity_motion=2.5 * R(Nd, 1) - 1,
                 _opacity_duration_center=torch.sort(2 + torch.rand(Nd, 2, 1, generator=g) * (K - 5), dim=1)[0],
                 _opacity_duration_var=R(Nd, 2, 1), _scaling_motion=math.log(0.01) + 0.8 * R(Nd, 3),
                 _features_dc_motion=R(Nd, 1, 3), _features_rest_motion=0.2 * R(Nd, 15, 3))
    else:                                               # an all-static scene: empty 1-D tensors, keyframe_num still 0
        P.update({k: torch.empty(0) for k in ("_xyz_motion", "_rotation_motion", "_opacity_motion", "_opacity_duration_center",
                                              "_opacity_duration_var", "_scaling_motion", "_features_dc_motion", "_features_rest_motion")})
    return pc, g, P


def _setup(pc, g, P):
    from arguments import OptimizationParams
    R = lambda *s: torch.randn(*s, generator=g)
    Ns, Nd = P["_xyz"].shape[0], P["_xyz_motion"].shape[0]
    for k, v in P.items():
        setattr(pc, k, torch.nn.Parameter(v.contiguous()))
    pc.max_radii2D = torch.zeros(Ns)
    pc.min_radii2D = torch.ones(Ns) * 1000
    pc.motion_max_radii2D = torch.zeros(Nd)
    pc.motion_min_radii2D = torch.ones(Nd) * 1000
    pc.spatial_lr_scale = 1.0
    pc.training_setup(OptimizationParams(argparse.ArgumentParser()))
    for grp in pc.optimizer.param_groups:
        p = grp["params"][0]
        p.grad = R(*p.shape) if p.numel() else torch.zeros_like(p)
    pc.optimizer.step()
    pc.optimizer.zero_grad(set_to_none=True)


def _margin(pc, vis, cam, percentile):
    """The smallest relative distance of a visible row's float64 score from the float64 threshold."""
    d, x = pc._xyz_disp.detach().double()[vis], pc._xyz.detach().double()[vis]
    s = d.norm(dim=-1) / ((x - cam.double()).norm(dim=-1) ** 2 + 0.000001)
    u = s / (s.max() + 0.000001)
    theta = torch.quantile(u, percentile)
    return float(((u - theta).abs() / theta.abs()).min()), u, theta


def _extract_case(out, case, seed, Ns, Nd, duration, kw):
    pc, g, P = _model(Ns, Nd, seed, duration=duration)
    _setup(pc, g, P)
    for j, t in enumerate((7.0, 123.0) if duration > 100 else (1.0, 3.0)):
        _iteration(pc, g, t, {}, "unused")
    vis = torch.rand(Ns, generator=g) > 0.2
    cam = torch.tensor(CAM)
    percentile = kw.get("percentile", 0.98)
    margin, u, theta = _margin(pc, vis, cam, percentile)
    assert margin > 1e-5, (case, margin, "change the seed, not the bar")
    n = pc._xyz_disp.detach().norm(dim=-1)[vis]
    seen = pc.xyz_error_min_timestamp.squeeze()[vis] >= 0
    extent = kw.get("extent", 1.0)
    above = u > theta
    if case == "motion":
        assert ((~above) & (n > kw["motion_thres"] * extent)).any(), case
    if case == "minmotion":
        assert (above & ~(n > kw["min_motion_thres"] * extent)).any() and (above & (n > kw["min_motion_thres"] * extent)).any(), case
    if case == "unseen":
        assert (above & ~seen).any() and (above & seen).any(), case
    _record(pc, out, f"{case}/pre")
    out[f"{case}/vis"], out[f"{case}/cam"] = vis.numpy(), cam.numpy()
    ns0 = pc._xyz.shape[0]
    pc.extract_dynamic_points_from_static(cam, 0.0, vis, **kw)
    _record(pc, out, f"{case}/post")
    cfg = dict(kw, duration=pc.duration, keyframe_num=pc.keyframe_num, margin=margin, selected=ns0 - pc._xyz.shape[0], theta64=float(theta))
    assert cfg["selected"] > 0 and pc._xyz_motion.shape[1] == pc.keyframe_num, (case, cfg)
    out[f"{case}/cfg"] = np.array(json.dumps(cfg))


def _expand_case(out, case, seed, Ns, Nd, duration, K, arg, expect, centers=None):
    pc, g, P = _model(Ns, Nd, seed, duration=duration, K=K)
    if centers is not None and Nd > 0:
        lo, hi = centers
        P["_opacity_duration_center"] = torch.sort(lo + torch.rand(Nd, 2, 1, generator=g) * (hi - lo), dim=1)[0]
    _setup(pc, g, P)
    _record(pc, out, f"{case}/pre")
    got = pc.expand_duration(arg)
    assert got is expect, (case, got)
    _record(pc, out, f"{case}/post")
    out[f"{case}/cfg"] = np.array(json.dumps(dict(duration_before=duration, argument=arg, returned=got, duration_after=pc.duration,
                                                 keyframes=int(pc._xyz_motion.shape[1]) if Nd else 0)))
    return pc


def _timestamps(seed):
    """A seeded sequence of mark_error / get_errorneous_timestamp calls on the reference: interleaved, an interval marked once among
    intervals marked often (the tenth-of-the-most-frequent rule), zero losses, pops until nothing is left."""
    from scene.c_gaussian_model import CGaussianModel
    rng = np.random.default_rng(seed)
    pc = CGaussianModel(3, 300, 10, 2, interp_type="cube", rot_interp_type="slerp")
    ops = []
    for _ in range(400):
        if rng.random() < 0.04:
            ops.append(["pop", pc.get_errorneous_timestamp()])
            continue
        t = float(rng.integers(0, 300)) if rng.random() < 0.9 else float(rng.integers(0, 3) * 10)
        loss = float(np.float32(rng.random() * (0.2 if t < 150 else 0.05))) if rng.random() < 0.9 else 0.0
        pc.mark_error(loss, t)
        ops.append(["mark", loss, t])
    for _ in range(40):
        ops.append(["pop", pc.get_errorneous_timestamp()])
    assert ops[-1][1] is None and sum(1 for o in ops if o[0] == "pop" and o[1] is not None) > 20
    return ops


def main():
    _stub_modules()
    real = {n: getattr(torch, n) for n in ("zeros", "ones", "arange")}
    strip = lambda f: (lambda *a, **k: f(*a, **{kk: vv for kk, vv in k.items() if kk != "device"}))
    out = {}
    try:
        torch.zeros, torch.ones, torch.arange = strip(real["zeros"]), strip(real["ones"]), strip(real["arange"])
        _extract_case(out, "extract", 21, 48, 12, 300, dict(extent=1.0, percentile=0.8))
        _extract_case(out, "first", 22, 48, 0, 5, dict(extent=1.0, percentile=0.9))
        _extract_case(out, "motion", 40, 40, 2, 300, dict(extent=1.0, motion_thres=0.15))
        _extract_case(out, "minmotion", 41, 40, 2, 300, dict(extent=1.0, percentile=0.45, min_motion_thres=0.12))
        _extract_case(out, "unseen", 42, 40, 2, 300, dict(extent=1.0, percentile=0.55))
        _expand_case(out, "early_short", 31, 4, 2, 300, None, 100, False)
        _expand_case(out, "early_static", 32, 4, 0, 300, None, 400, False)
        _expand_case(out, "early_fits", 33, 4, 2, 300, None, 301, False)
        pc = _expand_case(out, "expand", 34, 4, 8, 300, None, 330, True, centers=(28.0, 34.0))
        assert pc._xyz_motion.shape[1] == 38
        pc = _expand_case(out, "expand_small", 35, 4, 8, 3, 5, 20, True, centers=(0.5, 3.5))
        assert pc._xyz_motion.shape[1] == 7
        pc, g, P = _model(4, 8, 36)
        c = torch.sort(2.0 + torch.rand(8, 2, 1, generator=g) * 28.0, dim=1)[0]
        c[:5] = torch.tensor([[0.8, 5.0], [1.0, 1.3], [30.0, 32.0], [31.5, 32.5], [0.9, 31.8]]).view(5, 2, 1)      # outside one band, the other, both
        P["_opacity_duration_center"] = c
        v = 1.5 * torch.randn(8, 2, 1, generator=g)
        v[:5] = torch.tensor([[0.7, 0.7], [1.9, -0.3], [2.3, 0.8], [-0.8, 1.05], [0.6, 0.3]]).view(5, 2, 1)       # doubled from below 1, from above 1, and below 0.5
        P["_opacity_duration_var"] = v
        _setup(pc, g, P)
        c, v = pc._opacity_duration_center.detach(), pc._opacity_duration_var.detach()
        assert (c < 1.4).any() and (c > 31.0).any() and ((c > 1.4) & (c < 31.0)).any() and (v < 0.5).any() and ((v > 0.5) & (v < 1)).any() and (v > 1).any()
        _record(pc, out, "adjust/pre")
        pc.adjust_temp_opa()
        _record(pc, out, "adjust/post")
    finally:
        torch.zeros, torch.ones, torch.arange = real["zeros"], real["ones"], real["arange"]
    path = os.path.join(OUT, "growth.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(OUT, "growth.json"), "w") as f:
        json.dump({"interval": 10, "timestamps": _timestamps(7)}, f)
    return len(out), os.path.getsize(path)


if __name__ == "__main__":
    torch.set_default_dtype(torch.float32)
    torch.cuda.empty_cache = lambda: None
    print("growth:", main(), "(keys, bytes)", REF)
