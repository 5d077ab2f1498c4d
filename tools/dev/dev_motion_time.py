"""Times the displacement kernels (ex4dgs_amd.motion) at config 3 (0.8 M static + 0.2 M dynamic Gaussians, K = 35) on one GPU against
the same results composed from the ops the library had before them: two attributes.forward_raw(with_shs=False) calls plus a torch
subtraction (world) or a float32 torch projection with the depth rule (screen); for the gradients, the autograd surfaces of both.

Per operation the variants take turns in windows of at least a second between device events (ROUNDS windows each); the median window
is reported with its min / max.  Operations:
  fwd_world, fwd_screen        one launch into a preallocated output  |  the composition
  bwd_world, bwd_screen        one launch: g_xyz, g_xyz_disp and the two keyframe windows (no counterpart: the composition has no backward
                               of its own)
  grad_world, grad_screen      forward + backward through motion.displacement, dense [Nd,K,3] keyframe gradient included  |  forward +
                               backward through two attributes.evaluate_attributes(with_shs=False) and the torch ops
Bytes moved are what the algorithm needs, from the shapes: forward 24 B read per static row, 8 keyframe rows (96 B) per dynamic row, 12 B
written per row; backward 12 B of g_out per row, the positions again in screen space, 24 B written per static row and two windows
(96 B) per dynamic row.  Share of peak = bytes / time / 8 TB/s.  Prints one JSON line; --out writes it to a file as well."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

WINDOW_S, ROUNDS, T0, T1, NEAR, PEAK = 1.0, 3, 137.0, 150.0, 0.2, 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--window", type=float, default=WINDOW_S)
    a = ap.parse_args()
    import torch
    from ex4dgs_amd import attributes as attr, motion
    from ex4dgs_amd.scene import make_scene
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    model, cam, _ = make_scene("cfg3", device=dev)
    cam = cam.to(dev)
    names = attr.PARAM_ORDER
    params = [getattr(model, n).detach().contiguous() for n in names]
    Ns, Nd, K = model.num_static, model.num_dynamic, model._xyz_motion.shape[1]
    N = Ns + Nd
    kw = dict(interp_type=model.interp_type, duration=model.duration, interval=model.interval, time_shift=model.time_shift, var_pad=model.var_pad)
    s0, s1 = (attr.time_scalars(t, Ns, Nd, K, model.duration, model.interval, model.time_shift, model.var_pad, model.interp_type) for t in (T0, T1))
    xyz3 = (params[0], params[1], params[7])
    out = torch.empty(N, 3, device=dev)
    g_out = torch.randn(N, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    vm, pm, W, H = cam.world_view_transform, cam.full_proj_transform, cam.image_width, cam.image_height

    def project(x):
        h = x @ pm[:3] + pm[3]
        inv_w = 1.0 / (h[:, 3] + 0.0000001)
        return torch.stack([((h[:, 0] * inv_w + 1.0) * W - 1.0) * 0.5, ((h[:, 1] * inv_w + 1.0) * H - 1.0) * 0.5, x @ vm[:3, 2] + vm[3, 2]], 1)

    def screen(x0, x1):
        q0, q1 = project(x0), project(x1)
        behind = (q0[:, 2] <= NEAR) | (q1[:, 2] <= NEAR)
        return torch.where(behind[:, None], torch.zeros_like(q0), q1 - q0)

    def composed_fwd(space):
        x0, x1 = attr.forward_raw(s0, params, False, model.interp_type)[0], attr.forward_raw(s1, params, False, model.interp_type)[0]
        return x1 - x0 if space == "world" else screen(x0, x1)

    leaves = {n: p.clone().requires_grad_(True) for n, p in zip(names, params)}

    def zero():
        for p in leaves.values():
            p.grad = None

    def ours_grad(space):
        zero()
        d = motion.displacement(leaves, T0, T1, space=space, camera=cam, near=NEAR, **kw)
        (d * g_out).sum().backward()

    def composed_grad(space):
        zero()
        x0 = attr.evaluate_attributes(leaves, T0, with_shs=False, **kw)[0]
        x1 = attr.evaluate_attributes(leaves, T1, with_shs=False, **kw)[0]
        d = x1 - x0 if space == "world" else screen(x0, x1)
        (d * g_out).sum().backward()

    # the two agree before they are timed
    for space in ("world", "screen"):
        mine = motion.displacement_raw(s0, s1, *xyz3, space=space, camera=cam, near=NEAR, interp_type=model.interp_type)
        theirs = composed_fwd(space)
        err = float((mine - theirs).abs().max() / theirs.abs().max().clamp_min(1.0))
        assert err < 1e-4, (space, err)
        ours_grad(space)
        g = leaves["_xyz_motion"].grad.clone()
        composed_grad(space)
        gerr = float((g - leaves["_xyz_motion"].grad).abs().max() / g.abs().max().clamp_min(1.0))
        assert gerr < 1e-4, (space, gerr)

    ops = {}
    for space in ("world", "screen"):
        sp = dict(space=space, camera=cam, near=NEAR, interp_type=model.interp_type)
        ops[f"fwd_{space}"] = {"kernel": (lambda sp=sp: motion.displacement_raw(s0, s1, *xyz3, out=out, **sp)),
                               "composition": (lambda space=space: composed_fwd(space))}
        ops[f"bwd_{space}"] = {"kernel": (lambda sp=sp: motion.displacement_backward_raw(s0, s1, *xyz3, g_out, **sp))}
        ops[f"grad_{space}"] = {"kernel": (lambda space=space: ours_grad(space)), "composition": (lambda space=space: composed_grad(space))}
    fwd_bytes = Ns * (24 + 12) + Nd * (96 + 12)
    bytes_moved = {"fwd_world": fwd_bytes, "fwd_screen": fwd_bytes, "bwd_world": Ns * (12 + 24) + Nd * (12 + 96),
                   "bwd_screen": Ns * (12 + 24 + 24) + Nd * (12 + 96 + 96)}

    def window(fn, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches          # us per call

    result = {}
    for op, variants in ops.items():
        row = {}
        launches = {}
        for v, fn in variants.items():
            window(fn, 5)                                     # warm-up
            launches[v] = int(a.window * 1e6 / window(fn, 50)) + 1
        ts = {v: [] for v in variants}
        for _ in range(ROUNDS):
            for v, fn in variants.items():                    # the variants alternate
                ts[v].append(window(fn, launches[v]))
        for v, t in ts.items():
            row[v] = {"median_us": round(sorted(t)[len(t) // 2], 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2),
                      "launches_per_window": launches[v]}
        if "composition" in row:
            row["composition_over_kernel"] = round(row["composition"]["median_us"] / row["kernel"]["median_us"], 2)
        if op in bytes_moved:
            row["bytes"] = bytes_moved[op]
            row["share_of_8TBps_peak"] = round(bytes_moved[op] / (row["kernel"]["median_us"] * 1e-6) / PEAK, 4)
        result[op] = row
    doc = {"config": "cfg3", "device": torch.cuda.get_device_name(0), "static": Ns, "dynamic": Nd, "K": K, "interp_type": model.interp_type,
           "t0": T0, "t1": T1, "window_s": a.window, "rounds": ROUNDS, "us_per_call": result}
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
