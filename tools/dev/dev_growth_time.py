"""Times the growth of the dynamic set at config-3 sizes (0.8 M static + 0.2 M dynamic Gaussians, K = 35, 2 % of the visible static
rows selected): the HIP `extract_dynamic_points`, `expand_duration` and `adjust_temp_opa` (ex4dgs_amd.growth) against the reference's
torch composition (restated in tests/growth_ref.py) on the same GPU, both editing a torch.optim.RAdam's state.  Wall clock around a
call that ends in a device synchronise, median of the repeats after a warm-up run, the two alternating.  Prints one JSON line and
writes it to profiles/growth_time_cfg3.json (or the path given as the first argument)."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from ex4dgs_amd import densify, growth  # noqa: E402
from ex4dgs_amd.scene import make_scene  # noqa: E402
from tests import densify_ref as D  # noqa: E402
from tests import growth_ref as R  # noqa: E402

PEAK = 8.0e12
REPS = 5


def main():
    dev = torch.device("cuda:0")
    model, cam, _ = make_scene("cfg3", device=dev)
    ns, nd = model.num_static, model.num_dynamic
    K = model._xyz_motion.shape[1]
    g = torch.Generator(device=dev).manual_seed(0)
    base = {k: getattr(model, k).detach().clone() for k in model.PARAM_NAMES}
    mom = {k: (torch.randn(v.shape, device=dev, generator=g) * 1e-3, torch.rand(v.shape, device=dev, generator=g) * 1e-6) for k, v in base.items()}
    stats0 = densify.DensityStats(model)
    stats0.static[8] = torch.rand(ns, device=dev, generator=g) * 300          # every row seen
    stats0.dynamic[8] = torch.rand(nd, device=dev, generator=g) * 300
    vis = torch.rand(ns, device=dev, generator=g) < 0.9
    center = cam.camera_center.to(dev)
    rm = lambda: {"interval": model.interval, "time_shift": model.time_shift, "time_pad": model.time_pad, "duration": 300}
    holder = {}

    def reset():
        model.duration = 300
        for k, v in base.items():
            setattr(model, k, torch.nn.Parameter(v.clone()))
        opt = torch.optim.RAdam([{"params": [getattr(model, k)], "lr": 1e-3} for k in model.PARAM_NAMES])
        for k in model.PARAM_NAMES:
            opt.state[getattr(model, k)] = {"step": torch.tensor(1.0), "exp_avg": mom[k][0].clone(), "exp_avg_sq": mom[k][1].clone()}
        stats = densify.DensityStats(model)
        stats.static, stats.dynamic = stats0.static.clone(), stats0.dynamic.clone()
        holder["opt"], holder["stats"] = opt, stats

    def ref_state():
        st = {"params": {k: v.clone() for k, v in base.items()}, "m": {k: mom[k][0].clone() for k in base}, "v": {k: mom[k][1].clone() for k in base},
              "stats": {}}
        for names, blk in ((D.S_STATS, stats0.static), (D.D_STATS, stats0.dynamic)):
            for i, k in enumerate(names):
                st["stats"][k] = blk[i].clone() if k.endswith("radii2D") else blk[i].clone().view(-1, 1)
        holder["ref"] = st

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    calls = {
        "extract": (lambda: growth.extract_dynamic_points(model, holder["stats"], holder["opt"], center, 0.0, vis, 5.0),
                    lambda: R.extract(holder["ref"], rm(), center, vis, 5.0)),
        "expand_duration": (lambda: growth.expand_duration(model, holder["opt"], 330), lambda: R.expand_duration(holder["ref"], rm(), 330)),
        "adjust_temp_opa": (lambda: growth.adjust_temp_opa(model, holder["opt"]), lambda: R.adjust_temp_opa(holder["ref"], rm())),
    }
    result = {"config": "cfg3", "static": ns, "dynamic": nd, "K": K, "device": torch.cuda.get_device_name(0), "reps": REPS, "visible": int(vis.sum())}
    for name, (hip, ref) in calls.items():
        th, tr = [], []
        for rep in range(REPS + 1):                     # the first pair warms both up
            reset()
            dt, out = clock(hip)
            ref_state()
            dr, rout = clock(ref)
            if rep:
                th.append(dt)
                tr.append(dr)
        th.sort()
        tr.sort()
        result[f"{name}_ms"] = round(th[len(th) // 2] * 1e3, 3)
        result[f"{name}_ms_min_max"] = [round(th[0] * 1e3, 3), round(th[-1] * 1e3, 3)]
        result[f"{name}_torch_composition_ms"] = round(tr[len(tr) // 2] * 1e3, 3)
        if name == "extract":
            sel = out["dynamic"]["clone"]
            result["selected"] = sel
            assert sel == int(rout["mask"].sum()), (sel, int(rout["mask"].sum()))
            srow = sum(base[k][0].numel() for k in densify.STATIC_NAMES) * 4 * 3 + 36
            drow = sum(base[k][0].numel() for k in densify.DYNAMIC_NAMES) * 4 * 3 + 36
            moved = srow * (ns + ns - sel) + drow * (nd + nd + sel) + ns * (24 + 1 + 4 * 6 + 32)
            result["extract_bytes"] = moved
            result["extract_hbm_fraction"] = round(moved / (th[len(th) // 2]) / PEAK, 3)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "growth_time_cfg3.json")
    with open(path, "w") as f:
        f.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
