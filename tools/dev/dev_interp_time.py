"""Times the fused attribute kernels under the three position interpolators at config 3 (1.0 M Gaussians, Nd = 200 k dynamic, K = 35)
on one GPU: forward, dense backward and sliced backward, each with the [N,16,3] SH block (the whole op) and without it (what the
trainers run: the rasterizer reads the four feature tensors where they are).  cube, linear and pchip take turns in windows of at
least a second between device events; the median window per interpolator is reported with its min / max.

--parent-lib PATH: a libex4d_hip.so built from the parent commit's sources (a checkout of it, `python -m ex4dgs_amd.build`).  Its cube
path -- the entry points without _ex, the only ones it has -- is timed the same way in processes of its own, alternating with
processes of this tree's library (parent, ours, parent, ours): the spread between the parent's own runs is what this tree's cube
times have to sit inside, since the cube instantiation is meant to be the same code.

The entry points are called through ctypes directly (the table of ex4dgs_amd/_abi.py cannot bind a library that lacks the new ones).
One model serves all three interpolators: the timestamp is valid for each (k = 13 or 14 of K = 35), and the kernels' time does not
depend on which keyframes they read.  Prints one JSON line; --out writes it to a file as well."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

INTERPS = ("cube", "linear", "pchip")
OPS = ("forward", "forward_no_sh", "backward_dense", "backward_sliced", "backward_sliced_no_sh")
WINDOW_S, ROUNDS, T = 1.0, 3, 137.0


def child(legacy):
    import torch
    from ex4dgs_amd import _abi, attributes as attr
    from ex4dgs_amd.scene import make_scene
    dev = torch.device("cuda:0")
    lib = C.CDLL(_abi.library_path())
    model, _, _ = make_scene("cfg3", device=dev)
    params = [getattr(model, n).contiguous() for n in attr.PARAM_ORDER]
    Ns, Nd, K = model.num_static, model.num_dynamic, model._xyz_motion.shape[1]
    N = Ns + Nd
    g = torch.Generator().manual_seed(1)
    f32 = dict(dtype=torch.float32, device=dev)
    outs = [torch.empty(N, 3, **f32), torch.empty(N, 4, **f32), torch.empty(N, 1, **f32), torch.empty(N, 3, **f32), torch.empty(N, 16, 3, **f32)]
    gin = [torch.randn(N, c, generator=g).to(dev) for c in (3, 4, 1, 3)] + [torch.randn(N, 16, 3, generator=g).to(dev)]
    gout = [torch.empty_like(p) for p in params]
    slices = {7: torch.empty(Nd, 4, 3, **f32), 8: torch.empty(Nd, 2, 4, **f32)}
    byname = dict(zip(attr.PARAM_ORDER, params))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    hint = (C.c_int32 * 4)()

    def calls(interp):
        shift = model.time_pad if interp == "linear" else model.time_pad + model.interval
        scal = attr.time_scalars(T, Ns, Nd, K, model.duration, model.interval, shift, model.var_pad, interp) if not legacy else \
            attr.time_scalars(T, Ns, Nd, K, model.duration, model.interval, shift, model.var_pad)
        head = [C.byref(scal)] + ([] if legacy else [C.c_int32(attr.INTERP_TYPES[interp])])
        sfx = "" if legacy else "_ex"
        bwd_in = ([] if legacy else [ptr(byname["_xyz_motion"])]) + [ptr(byname[n]) for n in attr._BWD_INPUTS]
        fwd = getattr(lib, "ex4d_attributes_forward" + sfx)
        bwd = getattr(lib, "ex4d_attributes_backward" + sfx)
        bws = getattr(lib, "ex4d_attributes_backward_sliced" + sfx)
        p15, o4 = [ptr(p) for p in params], [ptr(o) for o in outs[:4]]
        g4, gd = [ptr(x) for x in gin[:4]], [ptr(x) for x in gout]
        gs = [ptr(slices.get(i, x)) for i, x in enumerate(gout)]
        feat = [attr.PARAM_ORDER.index(n) for n in attr.FEATURE_NAMES]
        gs_no = [None if i in feat else x for i, x in enumerate(gs)]

        def checked(fn, *a):
            def run():
                if fn(*a) != 0:
                    raise RuntimeError(lib.ex4d_attributes_last_error())
            return run
        return {"forward": checked(fwd, *head, *p15, *o4, ptr(outs[4]), stream),
                "forward_no_sh": checked(fwd, *head, *p15, *o4, None, stream),
                "backward_dense": checked(bwd, *head, *bwd_in, *g4, ptr(gin[4]), *gd, stream),
                "backward_sliced": checked(bws, *head, *bwd_in, *g4, ptr(gin[4]), *gs, hint, stream),
                "backward_sliced_no_sh": checked(bws, *head, *bwd_in, *g4, None, *gs_no, hint, stream)}

    lib.ex4d_attributes_last_error.restype = C.c_char_p

    def window(fn, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches          # us per call

    interps = ("cube",) if legacy else INTERPS
    table = {i: calls(i) for i in interps}
    result = {}
    for op in OPS:
        fns = [table[i][op] for i in interps]
        est = max(window(fn, 20) for fn in fns)               # warm-up, and the launches a one-second window takes
        est = max(est, max(window(fn, 200) for fn in fns))
        launches = int(WINDOW_S * 1e6 / est) + 1
        ts = [[] for _ in fns]
        for _ in range(ROUNDS):
            for j, fn in enumerate(fns):
                ts[j].append(window(fn, launches))
        result[op] = {i: {"median_us": round(sorted(t)[len(t) // 2], 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2), "launches_per_window": launches}
                      for i, t in zip(interps, ts)}
    print(json.dumps({"library": "parent" if legacy else "this tree", "device": torch.cuda.get_device_name(0), "static": Ns, "dynamic": Nd, "K": K,
                      "window_s": WINDOW_S, "rounds": ROUNDS, "us_per_call": result}))


def run_child(legacy, lib):
    env = dict(os.environ)
    if lib:
        env["EX4D_HIP_LIB"] = lib
    else:
        env.pop("EX4D_HIP_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "legacy" if legacy else "ours"], env=env, capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise RuntimeError(f"child failed ({out.returncode}): {out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=("ours", "legacy"))
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        return child(a.child == "legacy")
    runs = []
    if a.parent_lib:
        for _ in range(2):
            runs.append(run_child(True, os.path.abspath(a.parent_lib)))
            runs.append(run_child(False, None))
    else:
        runs.append(run_child(False, None))
    ours = [r for r in runs if r["library"] == "this tree"]
    parent = [r for r in runs if r["library"] == "parent"]
    summary = {}
    for op in OPS:
        med = lambda r, i: r["us_per_call"][op][i]["median_us"]
        cube = [med(r, "cube") for r in ours]
        row = {"cube_us": cube, "linear_us": [med(r, "linear") for r in ours], "pchip_us": [med(r, "pchip") for r in ours],
               "linear_over_cube": round(sum(med(r, "linear") for r in ours) / sum(cube), 3),
               "pchip_over_cube": round(sum(med(r, "pchip") for r in ours) / sum(cube), 3)}
        if parent:
            lo = min(r["us_per_call"][op]["cube"]["min_us"] for r in parent)
            hi = max(r["us_per_call"][op]["cube"]["max_us"] for r in parent)
            row.update(parent_cube_us=[med(r, "cube") for r in parent], parent_cube_window_range_us=[lo, hi],
                       cube_inside_parent_spread=bool(all(lo <= c <= hi for c in cube)))
        summary[op] = row
    doc = {"config": "cfg3", "timestamp": T, "summary": summary, "runs": runs}
    text = json.dumps(doc)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
