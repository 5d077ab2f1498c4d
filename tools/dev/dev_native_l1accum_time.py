"""Times the compiled trainer's l1_accum iteration at config 3 (0.8 M static + 0.2 M dynamic Gaussians, K = 35, 1352 x 1014) and writes
profiles/native_l1accum_cfg3.json (or the path given with --out).  Wall clock around blocks of iterations that end in a device
synchronise, after a warm-up; the variants alternate block by block, the median block and the spread over the blocks are recorded.

  (a) NativeTrainer.step as it was (ex4d_trainer_step), with this tree's library and -- with --parent-lib PATH, a libex4d_hip.so built
      from the parent commit -- with the parent's, both loaded into this process, on two copies of the model, alternating.  "Nothing
      changed" holds when the two medians differ by less than the spread of either.
  (b) the same trainer with l1_accum + statistics + NaN census + report() every iteration.
  (c) what a user composes for the same work without it: FrameTrainer + l1_ssim_loss(acc=) + DensityStats.update + the reference's
      isnan().any() gate of prune_nan_points + loss.item()  ("c_gated"), and with densify.prune_nan_points itself called every
      iteration as train.py:253 does ("c_prune_every_iteration": it re-gathers every tensor each time).
  (d) one begin_density_control -> densify_and_prune -> rebind_parameters cycle with a NativeTrainer (destroy + create + write), and
      the same densify_and_prune with a FrameTrainer (which keeps its workspace) for comparison.
"""
import argparse
import contextlib
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from ex4dgs_amd import _abi, densify  # noqa: E402
from ex4dgs_amd.loss import l1_ssim_loss  # noqa: E402
from ex4dgs_amd.native_trainer import NativeTrainer  # noqa: E402
from ex4dgs_amd.scene import CONFIGS, make_scene  # noqa: E402
from ex4dgs_amd.trainer import FrameTrainer  # noqa: E402

TIMES = (0, 137, 299, 41, 250)


def bind(path):
    """A second library in this process, bound from the prototype table as far as it has the names (the parent lacks the new ones)."""
    lib = ctypes.CDLL(path)
    for _, protos in _abi.PROTOTYPES.values():
        for name, restype, argtypes, _ in protos:
            if hasattr(lib, name):
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = restype, list(argtypes)
    return lib


@contextlib.contextmanager
def using(lib):
    """Calls of ex4dgs_amd go to `lib` inside the block (None: the tree's own library)."""
    if lib is None:
        yield
        return
    own, _abi._lib = _abi.load(), lib
    try:
        yield
    finally:
        _abi._lib = own


def block(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(TIMES[i % len(TIMES)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def summary(samples):
    s = sorted(samples)
    return {"ms": round(statistics.median(s), 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4), "blocks": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "native_l1accum_cfg3.json"))
    ap.add_argument("--P", type=int, default=None, help="Gaussians (default: config 3's 1.0 M)")
    ap.add_argument("--steps", type=int, default=40, help="iterations per block")
    ap.add_argument("--blocks", type=int, default=6)
    args = ap.parse_args()
    dev = "cuda"
    cfg = CONFIGS["cfg3"]

    def scene():
        m, cam, bg = make_scene("cfg3", P=args.P, device=dev, fused=True)
        return m, cam.to(dev), bg.to(dev)
    (m_new, cam, bg), (m_b, _, _), (m_c, _, _) = scene(), scene(), scene()
    gt = torch.rand(3, cfg.height, cfg.width, device=dev)
    lrs = {n: 1e-7 for n in m_new.PARAM_NAMES}
    kw = dict(optimizer=True, lrs=lrs, near=cfg.min_depth, far=cfg.max_depth)
    result = {"config": "cfg3", "static": m_new.num_static, "dynamic": m_new.num_dynamic, "K": int(m_new._xyz_motion.shape[1]),
              "device": torch.cuda.get_device_name(0), "steps_per_block": args.steps}

    variants = {}
    n_new = NativeTrainer(m_new, cam, **kw)
    variants["a_step_this_commit"] = (None, lambda t: n_new.step(cam, bg, t, gt))
    if args.parent_lib:
        parent = bind(args.parent_lib)
        m_old, _, _ = scene()
        with using(parent):
            n_old = NativeTrainer(m_old, cam, **kw)
        variants["a_step_parent_commit"] = (parent, lambda t: n_old.step(cam, bg, t, gt))
    n_b = NativeTrainer(m_b, cam, **kw)
    stats_b = densify.DensityStats(m_b)

    def native_full(t):
        n_b.step(cam, bg, t, gt, l1_accum=True, stats=stats_b, nan_census=True)
        loss, nan_s, nan_d = n_b.report()
        assert loss > 0 and not (nan_s or nan_d)
    variants["b_native_l1accum_stats_census_report"] = (None, native_full)

    f_c = FrameTrainer(m_c, optimizer=True, lrs=lrs)
    stats_c = densify.DensityStats(m_c)
    kept = []

    def upstream(out):
        loss, _, _, hook = l1_ssim_loss(out["render"], gt, 0.2, acc=out["acc"])
        kept[:] = [loss.detach()]
        return [loss, out["opticalflow"]], [None, hook]

    def composed(t, prune_every=False):
        out = f_c.step(cam, bg, t, upstream, near=cfg.min_depth, far=cfg.max_depth)
        stats_c.update(out["radii"].int().contiguous(), out["viewspace_points"].grad, out["viewspace_l1points"].grad, t)
        if prune_every:
            f_c.flush()                                          # (a prune drops a pending update: apply it first)
            densify.prune_nan_points(m_c, stats_c, f_c)
        elif bool(torch.isnan(m_c._xyz).any()) or bool(torch.isnan(m_c._xyz_motion).any()):
            f_c.flush()
            densify.prune_nan_points(m_c, stats_c, f_c)
        assert kept[0].item() > 0
    variants["c_gated"] = (None, composed)

    for lib, fn in variants.values():                            # warm-up: every variant, every timestamp
        with using(lib):
            block(fn, 2 * len(TIMES))
    samples = {k: [] for k in variants}
    for _ in range(args.blocks):
        for k, (lib, fn) in variants.items():
            with using(lib):
                samples[k].append(block(fn, args.steps))
    for k, s in samples.items():
        result[k] = summary(s)
    if args.parent_lib:
        with using(parent):                                      # its handle goes back to the library that made it
            n_old.close()
    if args.parent_lib:
        a, b = result["a_step_this_commit"], result["a_step_parent_commit"]
        spread = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
        result["a_difference_ms"] = round(a["ms"] - b["ms"], 4)
        result["a_spread_ms"] = round(spread, 4)
        result["a_within_spread"] = abs(a["ms"] - b["ms"]) <= spread
    block(lambda t: composed(t, True), 2)
    result["c_prune_every_iteration"] = summary([block(lambda t: composed(t, True), 5) for _ in range(3)])

    # (d) one density-control cycle; statistics of a few real iterations, thresholds of the reference's defaults
    def cycle(trainer, model, stats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = densify.densify_and_prune(model, stats, trainer, 0.0002, 0.0002, 0.005, 0.005, 5.0, generator=torch.Generator(device=dev).manual_seed(0))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out
    n_b.step(cam, bg, 7, gt, l1_accum=True, stats=stats_b, apply_optimizer=False)
    f_c.flush()
    rows = (m_b.num_static, m_b.num_dynamic)
    bytes_before = n_b.bytes()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n_b.begin_density_control()
    torch.cuda.synchronize()
    read_ms = (time.perf_counter() - t0) * 1e3
    ms_native, out = cycle(n_b, m_b, stats_b)
    ms_frame, _ = cycle(f_c, m_c, stats_c)
    result["d_density_control_cycle"] = {
        "native_ms": round(ms_native, 3), "frame_trainer_ms": round(ms_frame, 3), "moments_read_alone_ms": round(read_ms, 3),
        "rows_before": list(rows), "rows_after": [m_b.num_static, m_b.num_dynamic], "cloned": out["static"]["clone"] + out["dynamic"]["clone"],
        "split": out["static"]["split"] + out["dynamic"]["split"], "workspace_bytes_before": bytes_before, "cycles_timed": 1}
    native_full(0)                                               # the rebound trainer runs
    with open(args.out, "w") as f:
        f.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
