"""Generates tests/golden/densify.npz by importing the REFERENCE's CGaussianModel on CPU (like make_golden.py: third-party modules
stubbed, Tensor.cuda the identity, device="cuda" stripped from torch.zeros / torch.ones, which build_rotation and the densify code call).
torch.normal and torch.randn_like are patched in-process to record the standard-normal draws of every densify call.

Cases (K = 35): seeded small models, one real training_setup + one RAdam step, two iterations of the train.py:199-216 statistics block at
two timestamps (e0 on both sides of 0.01 and of 0), then
  default        densify_and_prune with the default thresholds
  screen         max_screen_size set and percent_dense 0.5: clones selected for split
  staticonly     Nd == 0
  invisible / small / nan   prune_invisible, prune_small, prune_nan_points (one NaN row per group)
Run:  python tests/golden/make_golden_densify.py      (needs the reference checkout)
"""
import argparse
import json
import math
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden import REF, _stub_modules  # noqa: E402

S_STATS = ("xyz_gradient_accum", "denom", "xyz_error_accum", "xyz_ssim_error_accum", "error_denom", "max_radii2D", "min_radii2D",
           "xyz_error_min", "xyz_error_min_timestamp")
D_STATS = ("motion_xyz_gradient_accum", "motion_denom", "motion_xyz_error_mean", "motion_xyz_ssim_error_accum", "motion_error_denom",
           "motion_max_radii2D", "motion_min_radii2D", "motion_xyz_error_min", "motion_xyz_error_min_timestamp")
GROUPS = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation",
          "xyz_disp": "_xyz_disp", "motion_xyz": "_xyz_motion", "motion_f_dc": "_features_dc_motion", "motion_f_rest": "_features_rest_motion",
          "motion_scaling": "_scaling_motion", "motion_opacity": "_opacity_motion", "motion_opacity_center": "_opacity_duration_center",
          "motion_opacity_var": "_opacity_duration_var", "motion_rotation": "_rotation_motion"}
DRAW_ORDER = ("clone_c1", "clone_c0", "static_split_z", "split_z", "split_c1", "split_c0")


def _model(Ns, Nd, seed):
    from arguments import OptimizationParams
    from scene.c_gaussian_model import CGaussianModel
    g = torch.Generator().manual_seed(seed)
    R = lambda *s: torch.randn(*s, generator=g)
    pc = CGaussianModel(3, 300, 10, 2, interp_type="cube", rot_interp_type="slerp")
    K = math.ceil((300 + pc.time_shift + 2 * pc.time_pad + 1) / pc.interval) + 3
    pc.keyframe_num = K
    P = dict(_xyz=R(Ns, 3), _xyz_disp=0.1 * R(Ns, 3), _rotation=R(Ns, 4), _opacity=2.5 * R(Ns, 1) - 1, _scaling=math.log(0.01) + 0.8 * R(Ns, 3),
             _features_dc=R(Ns, 1, 3), _features_rest=0.2 * R(Ns, 15, 3),
             _xyz_motion=torch.cumsum(0.2 * R(Nd, K, 3), 1), _rotation_motion=R(Nd, K, 4), _opacity_motion=2.5 * R(Nd, 1) - 1,
             _opacity_duration_center=torch.sort(2 + torch.rand(Nd, 2, 1, generator=g) * (K - 5), dim=1)[0],
             _opacity_duration_var=R(Nd, 2, 1), _scaling_motion=math.log(0.01) + 0.8 * R(Nd, 3),
             _features_dc_motion=R(Nd, 1, 3), _features_rest_motion=0.2 * R(Nd, 15, 3))
    for k, v in P.items():
        setattr(pc, k, torch.nn.Parameter(v.contiguous()))
    pc.max_radii2D = torch.zeros(Ns)
    pc.min_radii2D = torch.ones(Ns) * 1000
    pc.motion_max_radii2D = torch.zeros(Nd)
    pc.motion_min_radii2D = torch.ones(Nd) * 1000
    pc.spatial_lr_scale = 1.0
    op = OptimizationParams(argparse.ArgumentParser())
    pc.training_setup(op)
    for grp in pc.optimizer.param_groups:                      # one real RAdam step: non-zero moments and step counts
        p = grp["params"][0]
        p.grad = R(*p.shape) if p.numel() else torch.zeros_like(p)
    pc.optimizer.step()
    pc.optimizer.zero_grad(set_to_none=True)
    return pc, g, K


def _iteration(pc, g, t, out, tag):
    """train.py:199-216 with opt.l1_accum on and iteration < densify_until_iter."""
    N = pc._xyz.shape[0] + pc._xyz_motion.shape[0]
    radii = torch.randint(0, 4, (N,), generator=g, dtype=torch.int32) * torch.randint(0, 12, (N,), generator=g, dtype=torch.int32)
    vg = 4e-4 * torch.rand(N, 3, generator=g) * torch.randn(N, 3, generator=g).sign()
    e0 = torch.rand(N, generator=g) * 0.03 * (torch.rand(N, generator=g) > 0.2)          # zeros, (0, 0.01] and (0.01, 0.03)
    eg = torch.stack([e0, torch.rand(N, generator=g) * 0.02, torch.rand(N, generator=g) * 0.02], -1)
    out[f"{tag}/radii"], out[f"{tag}/vgrad"], out[f"{tag}/egrad"], out[f"{tag}/timestamp"] = radii.numpy(), vg.numpy(), eg.numpy(), np.float32(t)
    vp, ve = types.SimpleNamespace(grad=vg), types.SimpleNamespace(grad=eg)
    pc.mark_prune_stats(radii, ve)
    ns = pc._xyz.shape[0]
    vis = radii > 0
    pc.max_radii2D[vis[:ns]] = torch.max(pc.max_radii2D[vis[:ns]], radii[:ns][vis[:ns]])
    pc.motion_max_radii2D[vis[ns:]] = torch.max(pc.motion_max_radii2D[vis[ns:]], radii[ns:][vis[ns:]])
    pc.add_densification_stats(vp, vis[:ns], vis[ns:], ns)
    pc.add_l1_ssim_stats(ve, vis[:ns], vis[ns:], ns, t)


def _record(pc, out, tag):
    for grp in pc.optimizer.param_groups:
        k = GROUPS[grp["name"]]
        p = grp["params"][0]
        out[f"{tag}/param/{k}"] = p.detach().numpy().copy()
        st = pc.optimizer.state.get(p)
        if st:
            out[f"{tag}/m/{k}"] = st["exp_avg"].numpy().copy()
            out[f"{tag}/v/{k}"] = st["exp_avg_sq"].numpy().copy()
            out[f"{tag}/step/{k}"] = np.float32(st["step"])
    for k in S_STATS + D_STATS:
        out[f"{tag}/stats/{k}"] = getattr(pc, k).numpy().copy()


def main():
    _stub_modules()
    real = {n: getattr(torch, n) for n in ("zeros", "ones", "normal", "randn_like")}
    strip = lambda f: (lambda *a, **k: f(*a, **{kk: vv for kk, vv in k.items() if kk != "device"}))
    rec = []
    gen = {"g": None}

    def normal(mean, std, *a, **k):
        z = torch.randn(std.shape, generator=gen["g"])
        rec.append(z)
        return mean + std * z

    def randn_like(x, *a, **k):
        z = torch.randn(x.shape, generator=gen["g"])
        rec.append(z)
        return z

    out = {}
    cases = {"default": (32, 16, 11, dict()), "screen": (32, 16, 12, dict(max_screen_size=20, max_dynamic_screen_size=20, percent_dense=0.5, extent=0.1)),
             "staticonly": (32, 0, 13, dict()), "invisible": (16, 8, 14, None), "small": (16, 8, 15, None), "nan": (16, 8, 16, None)}
    try:
        torch.zeros, torch.ones = strip(real["zeros"]), strip(real["ones"])
        torch.normal, torch.randn_like = normal, randn_like
        for case, (Ns, Nd, seed, cfg) in cases.items():
            pc, g, K = _model(Ns, Nd, seed)
            gen["g"] = g
            for j, t in enumerate((7.0, 123.0)):
                _iteration(pc, g, t, out, f"{case}/A{j}")
                for k in S_STATS + D_STATS:
                    out[f"{case}/A{j}/stats/{k}"] = getattr(pc, k).numpy().copy()
            if case == "nan":
                with torch.no_grad():
                    pc._xyz[3, 1] = float("nan")
                    pc._xyz_motion[5, 17, 2] = float("nan")
            _record(pc, out, f"{case}/pre")
            if cfg is not None:
                cfg = dict(dict(max_grad=0.0002, max_dgrad=0.0002, min_opacity=0.01, min_motion_opacity=0.01, extent=1.0, max_screen_size=None,
                                max_dynamic_screen_size=None, s_max_ssim=0.5, s_l1_thres=0.1, d_max_ssim=0.5, d_l1_thres=0.1, percent_dense=0.01), **cfg)
                pc.percent_dense = cfg["percent_dense"]
                rec.clear()
                pc.densify_and_prune(cfg["max_grad"], cfg["max_dgrad"], cfg["min_opacity"], cfg["min_motion_opacity"], cfg["extent"],
                                     cfg["max_screen_size"], cfg["max_dynamic_screen_size"], s_max_ssim=cfg["s_max_ssim"], s_l1_thres=cfg["s_l1_thres"],
                                     d_max_ssim=cfg["d_max_ssim"], d_l1_thres=cfg["d_l1_thres"])
                order = DRAW_ORDER if Nd > 0 else ("static_split_z",)
                assert len(rec) == len(order), (case, len(rec))
                for k, z in zip(order, rec):
                    out[f"{case}/draw/{k}"] = z.numpy().reshape(-1, 3) if k.endswith("_z") else z.numpy().reshape(-1)
                out[f"{case}/cfg"] = np.array(json.dumps(cfg))
            else:
                {"invisible": pc.prune_invisible, "small": pc.prune_small, "nan": pc.prune_nan_points}[case]()
            _record(pc, out, f"{case}/post")
    finally:
        torch.zeros, torch.ones, torch.normal, torch.randn_like = real["zeros"], real["ones"], real["normal"], real["randn_like"]
    path = os.path.join(OUT, "densify.npz")
    np.savez_compressed(path, **out)
    return len(out), os.path.getsize(path)


if __name__ == "__main__":
    torch.set_default_dtype(torch.float32)
    torch.cuda.empty_cache = lambda: None
    print("densify:", main(), "(keys, bytes)", REF)
