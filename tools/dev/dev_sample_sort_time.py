"""Stage time of the sample depth sort (option "depth_sort_sample") against the other depth sorts, on the profiler's `depth_sort` stage
(ex4d_profile_enable), and the frame time of a forward replayed from a hipGraph with the option on and off.
    python tools/dev/dev_sample_sort_time.py [--out profiles/sample_sort_time.json] [--window 1.0] [--rounds 3]
Windows of at least `--window` seconds, the variants alternating round by round; per variant the median over the windows of the window's
mean.  Scenes: cfg3 (1.0 M, spread in depth), cfg3c (1.0 M, clustered), cfg3 with a third of the Gaussians at exactly 10 m (a wall),
cfg2 (100 k) for the graph."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import helpers as h                      # noqa: E402
from tests.test_gpu_round4 import _raw_forward      # noqa: E402
from ex4dgs_amd import _C, build                    # noqa: E402

VARIANTS = (("sample", dict(depth_sort_sample=1, depth_sort_msd=3)), ("msd_forced", dict(depth_sort_sample=0, depth_sort_msd=2)),
            ("default_auto", dict(depth_sort_sample=0, depth_sort_msd=3)), ("lsd", dict(depth_sort_sample=0, depth_sort_msd=0)))


def wall_scene(P):
    ins, st = h.scene_inputs("cfg3", P=P, t=137)
    g = torch.Generator().manual_seed(3)
    m = ins["means3D"]
    on = torch.rand(P, generator=g) < 1.0 / 3.0
    z = torch.where(on, torch.full((P,), 10.0), m[:, 2])
    s = (z / m[:, 2]).unsqueeze(1)
    m = m * s
    m[:, 2] = z
    ins["means3D"], ins["scales"] = m.contiguous(), (ins["scales"] * s).contiguous()
    return ins, st


def set_options(opts):
    for k, v in opts.items():
        _C.set_option(k, v)


def stage_windows(ins, st, window, rounds):
    """{variant: {stage: median over windows of the window's mean, in microseconds}}"""
    ins = {k: v.cuda() for k, v in ins.items()}
    per = {name: [] for name, _ in VARIANTS}
    for r in range(rounds + 1):                       # (round 0 warms up: not recorded)
        for name, opts in VARIANTS:
            set_options(opts)
            for _ in range(3):
                _raw_forward(ins, st)
            torch.cuda.synchronize()
            _C.profile_enable(True)
            agg, n, t0 = {}, 0, time.perf_counter()
            while time.perf_counter() - t0 < (window if r else 0.2):
                _raw_forward(ins, st)
                torch.cuda.synchronize()
                for k, ms in _C.profile_read(0):
                    agg[k] = agg.get(k, 0.0) + ms
                n += 1
            _C.profile_enable(False)
            if r:
                w = {k: v / n * 1e3 for k, v in agg.items()}
                w["forward"] = sum(w.values())
                w["frames"] = n
                w["trips"] = _C.get_option("depth_sort_trips")
                per[name].append(w)
    return {name: {k: round(statistics.median(w.get(k, 0.0) for w in ws), 2) for k in ("depth_sort", "scan_tiles", "forward", "frames", "trips")}
            for name, ws in per.items()}


def graph_windows(window, rounds):
    """frame time (microseconds) of cfg2's asynchronous forward replayed from a graph: default options (the LSD sort under capture) and the sample sort"""
    ins, st = h.scene_inputs("cfg2", dir_scale=0.0)
    ins = {k: v.cuda() for k, v in ins.items()}
    s, sync = _raw_forward(ins, st)
    cap = int(1.5 * int(sync[0]))
    graphs = {}
    for name, opts in (("default_auto", VARIANTS[2][1]), ("sample", VARIANTS[0][1])):
        set_options(opts)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _raw_forward(ins, st, settings=s, instance_capacity=cap, assume_no_flow=True)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            keep = _raw_forward(ins, st, settings=s, instance_capacity=cap, assume_no_flow=True)
        graphs[name] = (g, keep)
    per = {name: [] for name in graphs}
    for r in range(rounds + 1):
        for name, (g, _) in graphs.items():
            n, t0 = 0, time.perf_counter()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            while time.perf_counter() - t0 < (window if r else 0.2):
                for _ in range(50):
                    g.replay()
                torch.cuda.synchronize()
                n += 50
            e1.record()
            torch.cuda.synchronize()
            if r:
                per[name].append(e0.elapsed_time(e1) / n * 1e3)
    return {name: round(statistics.median(v), 2) for name, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_sort_time.json"))
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--P", type=int, default=1_000_000)
    a = ap.parse_args()
    build.build()
    _C.load()
    saved = {k: _C.get_option(k) for k in ("depth_sort_sample", "depth_sort_msd")}
    out = dict(unit="microseconds", window_seconds=a.window, rounds=a.rounds, P=a.P, device=torch.cuda.get_device_name(0))
    try:
        for label, scene in (("cfg3", lambda: h.scene_inputs("cfg3", P=a.P, t=137)), ("cfg3c", lambda: h.scene_inputs("cfg3c", P=a.P, t=137)),
                             ("cfg3_wall_third_at_10m", lambda: wall_scene(a.P))):
            ins, st = scene()
            out[label] = stage_windows(ins, st, a.window, a.rounds)
            print(label, json.dumps(out[label]), flush=True)
        out["cfg2_graph_replay_frame"] = graph_windows(a.window, a.rounds)
        print("cfg2 graph", json.dumps(out["cfg2_graph_replay_frame"]), flush=True)
    finally:
        set_options(saved)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
