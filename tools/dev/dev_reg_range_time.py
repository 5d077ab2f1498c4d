"""Times the regulariser gradient of an element range (ex4d_reg_backward_range) at config 3 (0.8 M static + 0.2 M dynamic, K = 35) on
one GPU, per tensor (_xyz_disp, _xyz_motion, _rotation_motion), every call the bare C entry in accumulate mode:
  * ex4d_reg_backward, dense, of the PARENT build (--parent-lib: a libex4d_hip.so built from the parent commit) and of this build,
  * ex4d_reg_backward_range over the whole element range,
  * ex4d_reg_backward_range over the rank-0 shard of 2 and of 8 ranks (dist.shard_range, align 4).
Device events around windows of at least a second each, the variants taking turns, three rounds.  The one condition: the full-range
call is not slower than the parent's dense call on the same tensor by more than twice the spread of the parent's own windows.  The
shard times and their ratio to the full range are recorded without a bar.  Writes profiles/reg_range_time_cfg3.json (--out)."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from ex4dgs_amd import _abi, regularizers as reg  # noqa: E402
from ex4dgs_amd.dist import shard_range  # noqa: E402
from ex4dgs_amd.scene import make_scene  # noqa: E402

W3 = (1e-4, 1e-4, 1e-3)
WINDOW_S = 1.0
ROUNDS = 3


def events_us(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def alternate(fns):
    """Per fn the times per launch of ROUNDS windows of >= WINDOW_S each, the fns taking turns."""
    launches = []
    for fn in fns:
        events_us(fn, 20)                                         # warm-up
        launches.append(max(50, int(1.1 * WINDOW_S * 1e6 / events_us(fn, 200))))
    ts = [[] for _ in fns]
    for _ in range(ROUNDS):
        for i, fn in enumerate(fns):
            ts[i].append(events_us(fn, launches[i]))
    return ts, launches


def parent_backward(path):
    """ex4d_reg_backward of another build of the library, bound from the same prototype table."""
    lib = C.CDLL(path)
    _, restype, argtypes, _ = next(p for p in _abi.PROTOTYPES["ex4d_regularizers.h"][1] if p[0] == "ex4d_reg_backward")
    lib.ex4d_reg_backward.restype, lib.ex4d_reg_backward.argtypes = restype, list(argtypes)
    return lib.ex4d_reg_backward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libex4d_hip.so of the parent commit (default: none, the parent columns are left out)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reg_range_time_cfg3.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model, _, _ = make_scene("cfg3", device=dev, fused=True)
    Ns, Nd, K = model.num_static, model.num_dynamic, model._xyz_motion.shape[1]
    tensors = {"_xyz_disp": (reg.REG_STATIC, model._xyz_disp.detach(), W3[0], 0),
               "_xyz_motion": (reg.REG_MOTION, model._xyz_motion.detach(), W3[1], 1),
               "_rotation_motion": (reg.REG_ROT, model._rotation_motion.detach(), W3[2], 2)}
    parent = parent_backward(args.parent_lib) if args.parent_lib else None
    lib = _abi.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    report = {"config": "cfg3", "static": Ns, "dynamic": Nd, "K": K, "device": torch.cuda.get_device_name(0), "weights": W3,
              "window_seconds": WINDOW_S, "rounds": ROUNDS, "parent_lib": bool(parent), "tensors": {}}
    ok = True
    for name, (kind, p, w, slot) in tensors.items():
        n = p.numel()
        g = torch.zeros_like(p)
        params, grads, ws = [None] * 3, [None] * 3, [0.0] * 3
        params[slot], grads[slot], ws[slot] = p, g, w
        # every variant is the bare C call with its arguments made once: the same host path for all (the small tensor is launch-bound)
        a = [_abi.ptr(params[0]), _abi.ptr(grads[0]), Ns, _abi.ptr(params[1]), _abi.ptr(grads[1]), _abi.ptr(params[2]), _abi.ptr(grads[2]), Nd, K,
             ws[0], ws[1], ws[2], None, 1, stream]
        variants = {"dense": lambda a=a: lib.ex4d_reg_backward(*a)}
        if parent is not None:
            variants["parent_dense"] = lambda a=a: parent(*a)
        shards = {"range_full": (0, n), "range_rank0_of_2": shard_range(n, 0, 2)[:2], "range_rank0_of_8": shard_range(n, 0, 8)[:2]}
        for key, (lo, hi) in shards.items():
            b = [kind, p.data_ptr(), p.shape[0], K, lo, hi, g.data_ptr() + 4 * lo, w, 1, stream]
            variants[key] = lambda b=b: lib.ex4d_reg_backward_range(*b)
        assert all(fn() == 0 for fn in variants.values()), (name, lib.ex4d_reg_last_error())
        ts, launches = alternate(list(variants.values()))
        row = {"elements": n}
        for key, t, l in zip(variants, ts, launches):
            row[key] = {"median_us": round(sorted(t)[len(t) // 2], 2), "windows_us": [round(x, 2) for x in t], "launches_per_window": l}
        for key, (lo, hi) in shards.items():
            row[key]["elements"] = hi - lo
            row[key]["ratio_to_full"] = round(row[key]["median_us"] / row["range_full"]["median_us"], 3)
        base = row.get("parent_dense", row["dense"])
        spread = max(base["windows_us"]) - min(base["windows_us"])
        row["condition"] = {"baseline": "parent_dense" if parent is not None else "dense", "baseline_spread_us": round(spread, 2),
                            "full_minus_baseline_us": round(row["range_full"]["median_us"] - base["median_us"], 2),
                            "met": bool(row["range_full"]["median_us"] <= base["median_us"] + 2 * spread)}
        ok = ok and row["condition"]["met"]
        report["tensors"][name] = row
    report["condition_full_range_not_slower_than_parent_dense"] = ok
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print(json.dumps(report))


if __name__ == "__main__":
    main()
