"""Times adaptive density control at config 3 (1.0 M Gaussians, 20 % dynamic, K = 35): the HIP `DensityStats.update` and
`densify_and_prune` (ex4dgs_amd.densify) against the reference's torch composition (restated in tests/densify_ref.py) on the same GPU.
Prints one JSON line: microseconds / milliseconds, the bytes each moves and the fraction of the MI355X HBM peak (8 TB/s)."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ex4dgs_amd import densify  # noqa: E402
from ex4dgs_amd.scene import make_scene  # noqa: E402
from tests import densify_ref as R  # noqa: E402

PEAK = 8.0e12


def timed(fn, reps, setup=None):
    ts = []
    for _ in range(reps):
        if setup:
            setup()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    dev = torch.device("cuda:0")
    model, _, _ = make_scene("cfg3", device=dev)
    ns, nd = model.num_static, model.num_dynamic
    P = ns + nd
    g = torch.Generator(device=dev).manual_seed(0)
    radii = torch.randint(0, 20, (P,), device=dev, generator=g, dtype=torch.int32)
    vg = 1e-3 * torch.randn(P, 3, device=dev, generator=g)
    eg = torch.rand(P, 3, device=dev, generator=g) * 0.02
    stats = densify.DensityStats(model)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        stats.update(radii, vg, eg, 5.0)
    n = 200
    ev0.record()
    for _ in range(n):
        stats.update(radii, vg, eg, 5.0)
    ev1.record()
    torch.cuda.synchronize()
    upd_us = ev0.elapsed_time(ev1) * 1e3 / n
    ref_st = R.init_stats(ns, nd, dev)
    ref_upd_us = timed(lambda: R.update(ref_st, radii, vg, eg, 5.0), 20) * 1e6
    upd_bytes = P * (4 + 12 + 12 + 2 * 9 * 4)

    cfg = dict(max_grad=0.0002, max_dgrad=0.0002, min_opacity=0.01, min_motion_opacity=0.01, extent=5.0)
    base = {k: getattr(model, k).detach().clone() for k in model.PARAM_NAMES}
    base_stats = (stats.static.clone(), stats.dynamic.clone())
    holder = {}

    def reset():
        for k, v in base.items():
            setattr(model, k, torch.nn.Parameter(v.clone()))
        opt = torch.optim.RAdam([{"params": [getattr(model, k)], "lr": 1e-3} for k in model.PARAM_NAMES])
        for k in model.PARAM_NAMES:
            p = getattr(model, k)
            opt.state[p] = {"step": torch.tensor(1.0), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
        stats.static, stats.dynamic = base_stats[0].clone(), base_stats[1].clone()
        holder["opt"] = opt

    def run():
        holder["out"] = densify.densify_and_prune(model, stats, holder["opt"], **cfg, generator=torch.Generator(device=dev).manual_seed(1))
    dp_ms = timed(run, 5, reset) * 1e3
    out = holder["out"]
    rows_in = {"static": ns, "dynamic": nd}
    rowbytes = {"static": sum(base[k][0].numel() for k in densify.STATIC_NAMES) * 4 * 3 + 36,
                "dynamic": sum(base[k][0].numel() for k in densify.DYNAMIC_NAMES) * 4 * 3 + 36}
    dp_bytes = sum(rowbytes[gk] * (rows_in[gk] + out[gk]["rows"]) for gk in rowbytes)

    def ref_run():
        st = {"params": {k: v.clone() for k, v in base.items()}, "m": {k: torch.zeros_like(v) for k, v in base.items()},
              "v": {k: torch.zeros_like(v) for k, v in base.items()},
              "stats": {k: getattr(stats, k).clone() for k in R.S_STATS + R.D_STATS}}
        holder["ref"] = st
    reset()
    run()
    draws = out["draws"]
    ref_times = []
    for _ in range(3):
        reset()
        ref_st = {"params": {k: v.clone() for k, v in base.items()}, "m": {k: torch.zeros_like(v) for k, v in base.items()},
                  "v": {k: torch.zeros_like(v) for k, v in base.items()},
                  "stats": {k: x.clone() for k, x in zip(R.S_STATS + R.D_STATS, list(base_stats[0]) + list(base_stats[1]))}}
        for k in ref_st["stats"]:
            if not k.endswith("radii2D"):
                ref_st["stats"][k] = ref_st["stats"][k].view(-1, 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        R.densify_and_prune(ref_st, {"interval": model.interval, "time_shift": model.time_shift, "duration": model.duration},
                            cfg["max_grad"], cfg["max_dgrad"], cfg["min_opacity"], cfg["min_motion_opacity"], cfg["extent"], None, None, draws)
        torch.cuda.synchronize()
        ref_times.append(time.perf_counter() - t0)
    ref_dp_ms = sorted(ref_times)[1] * 1e3
    print(json.dumps({
        "config": "cfg3", "P": P, "static": ns, "dynamic": nd, "device": torch.cuda.get_device_name(0),
        "update_us": round(upd_us, 2), "update_torch_composition_us": round(ref_upd_us, 1), "update_bytes": upd_bytes,
        "update_hbm_fraction": round(upd_bytes / (upd_us * 1e-6) / PEAK, 3),
        "densify_and_prune_ms": round(dp_ms, 3), "densify_and_prune_torch_composition_ms": round(ref_dp_ms, 2),
        "densify_and_prune_bytes": dp_bytes, "densify_and_prune_hbm_fraction": round(dp_bytes / (dp_ms * 1e-3) / PEAK, 3),
        "counts": {k: out[k] for k in ("static", "dynamic")}}))


if __name__ == "__main__":
    main()
