"""Times the uint8 ground-truth path at config 3's image size (1352 x 1014) and writes profiles/frames_time_cfg3.json (or --out).

  1. Loss forward + backward, device events around blocks of launches, the variants alternating in rounds within this process:
       (a) the float entries on a resident float32 [3,H,W] ground truth;
       (b) the _u8 entries on the same frame as uint8 [H,W,3] (the table in the kernel arguments, copied to LDS per workgroup);
       (c) (a) plus the torch composition that turns the uint8 frame into that float tensor: lut[gt8.long()].permute(2,0,1).contiguous().
     Condition: (b) <= (c).  (b) - (a) is recorded as it comes out.
  2. With --parent-lib PATH (a libex4d_hip.so built from the parent commit): (a) alone in SEPARATE processes, this tree's library and
     the parent's alternating (each child is this script with --float-only and EX4D_HIP_LIB set).  Condition: this tree's median is not
     above the parent's by more than the spread (max - min) of the parent's own runs, which is recorded beside it.
  3. Getting a frame to the device, wall clock per NativeTrainer.step iteration (blocks that end in a device synchronise), as the
     added time over the resident case:
       resident   FrameStore.get(i) of a frame uploaded before the clock starts;
       stream     FrameStream(depth=2): frame n + 1 is pushed (pinned copy + asynchronous upload) before step n is enqueued;
       reference  a pageable float32 tensor with the reference's strides ((1, 3W, 3): permuted HWC) and .cuda() per iteration, made
                  contiguous on the device for the float step.
     No condition; these go into README / DESIGN.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from ex4dgs_amd import _abi  # noqa: E402
from ex4dgs_amd.frames import FrameStore, FrameStream, gt_lut  # noqa: E402
from ex4dgs_amd.loss import _WINDOW  # noqa: E402

H, W = 1014, 1352
DEV = "cuda"
LAMBDA = 0.2


def summary(samples, digits=4):
    s = sorted(samples)
    return {"ms": round(statistics.median(s), digits), "min_ms": round(s[0], digits), "max_ms": round(s[-1], digits), "blocks": len(s)}


class Loss:
    """Preallocated buffers and the three variants of one forward + backward."""

    def __init__(self):
        g = torch.Generator().manual_seed(1)
        f32 = dict(dtype=torch.float32, device=DEV)
        self.lut = gt_lut()
        self.lut_dev = self.lut.to(DEV)
        self.img = torch.rand(3, H, W, generator=g).to(DEV)
        self.gt8 = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
        self.gtf = self.lut_dev[self.gt8.long()].permute(2, 0, 1).contiguous()
        self.loss, self.l1e, self.sse = torch.empty(1, **f32), torch.empty(H, W, **f32), torch.empty(H, W, **f32)
        self.dmaps, self.grad = torch.empty(9, H, W, **f32), torch.empty(3, H, W, **f32)
        self.scratch = torch.empty(_abi.load().ex4d_l1_ssim_scratch_floats(H, W), **f32)
        self.gl = torch.ones(1, **f32)

    def a_float(self, gtf=None):
        gtf = self.gtf if gtf is None else gtf
        with _abi.stream(self.img.device) as s:
            _abi.call("ex4d_l1_ssim_forward", 3, H, W, self.img.data_ptr(), gtf.data_ptr(), LAMBDA, _WINDOW.ctypes.data, self.loss.data_ptr(),
                      self.l1e.data_ptr(), self.sse.data_ptr(), self.dmaps.data_ptr(), self.scratch.data_ptr(), s)
            _abi.call("ex4d_l1_ssim_backward", 3, H, W, self.img.data_ptr(), gtf.data_ptr(), LAMBDA, _WINDOW.ctypes.data, self.dmaps.data_ptr(),
                      self.gl.data_ptr(), self.grad.data_ptr(), s)

    def b_u8(self):
        with _abi.stream(self.img.device) as s:
            _abi.call("ex4d_l1_ssim_forward_u8", H, W, self.img.data_ptr(), self.gt8.data_ptr(), 3, self.lut.data_ptr(), LAMBDA, _WINDOW.ctypes.data,
                      self.loss.data_ptr(), self.l1e.data_ptr(), self.sse.data_ptr(), self.dmaps.data_ptr(), self.scratch.data_ptr(), s)
            _abi.call("ex4d_l1_ssim_backward_u8", H, W, self.img.data_ptr(), self.gt8.data_ptr(), 3, self.lut.data_ptr(), LAMBDA, _WINDOW.ctypes.data,
                      self.dmaps.data_ptr(), self.gl.data_ptr(), self.grad.data_ptr(), s)

    def c_composed(self):
        self.a_float(self.lut_dev[self.gt8.long()].permute(2, 0, 1).contiguous())


def event_block(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def rounds(variants, steps, blocks):
    for fn in variants.values():
        event_block(fn, 10)
    samples = {k: [] for k in variants}
    for _ in range(blocks):
        for k, fn in variants.items():
            samples[k].append(event_block(fn, steps))
    return {k: summary(s) for k, s in samples.items()}


def float_only(args):
    # the parent's library lacks the new names: bind what it has (load() would insist on the whole table)
    lib = ctypes.CDLL(_abi.library_path())
    for _, protos in _abi.PROTOTYPES.values():
        for name, restype, argtypes, _ in protos:
            if hasattr(lib, name):
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = restype, list(argtypes)
    _abi._lib = lib
    L = Loss()
    print(json.dumps({"float_only": rounds({"a": L.a_float}, args.steps, args.blocks)["a"], "lib": _abi.library_path()}))


def across_processes(args):
    runs = {"this": [], "parent": []}
    for _ in range(args.processes):
        for who, lib in (("parent", args.parent_lib), ("this", None)):
            env = dict(os.environ)
            env.pop("EX4D_HIP_LIB", None)
            if lib:
                env["EX4D_HIP_LIB"] = os.path.abspath(lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--float-only", "--steps", str(args.steps), "--blocks", str(args.blocks)],
                                 env=env, capture_output=True, text=True, timeout=300)
            if out.returncode:
                raise RuntimeError(f"{who}: child failed ({out.returncode}): {out.stderr[-400:]}")
            runs[who].append(json.loads(out.stdout.strip().splitlines()[-1])["float_only"]["ms"])
    this, parent = statistics.median(runs["this"]), statistics.median(runs["parent"])
    spread = max(runs["parent"]) - min(runs["parent"])
    return {"this_ms": runs["this"], "parent_ms": runs["parent"], "this_median_ms": round(this, 4), "parent_median_ms": round(parent, 4),
            "parent_spread_ms": round(spread, 4), "difference_ms": round(this - parent, 4), "not_slower_than_parent_beyond_its_spread": this - parent <= spread}


def arrival(args):
    import time
    from ex4dgs_amd.native_trainer import NativeTrainer
    from ex4dgs_amd.scene import CONFIGS, make_scene
    cfg = CONFIGS["cfg3"]
    assert (cfg.height, cfg.width) == (H, W)
    model, cam, bg = make_scene("cfg3", P=args.P, device=DEV, fused=True)
    cam, bg = cam.to(DEV), bg.to(DEV)
    nt = NativeTrainer(model, cam, optimizer=True, lrs={n: 1e-7 for n in model.PARAM_NAMES}, near=cfg.min_depth, far=cfg.max_depth)
    n_frames = 8
    g = torch.Generator().manual_seed(2)
    host = [torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8) for _ in range(n_frames)]
    host_f32 = [(f / 255.0).permute(2, 0, 1) for f in host]              # pageable, stride (1, 3W, 3): what the reference's loader returns
    assert host_f32[0].stride() == (1, 3 * W, 3) and not host_f32[0].is_pinned()
    store = FrameStore(n_frames, H, W, device=DEV)
    for i, f in enumerate(host):
        store.put(i, f)
    fs = FrameStream(H, W, depth=2, device=DEV)
    times = (0, 137, 299, 41, 250)

    def resident(steps):
        for i in range(steps):
            nt.step(cam, bg, times[i % 5], store.get(i % n_frames))

    def stream(steps):
        fs.push(host[0])
        for i in range(steps):
            if i + 1 < steps:
                fs.push(host[(i + 1) % n_frames])
            nt.step(cam, bg, times[i % 5], fs.pop())

    def reference(steps):
        for i in range(steps):
            nt.step(cam, bg, times[i % 5], host_f32[i % n_frames].cuda().contiguous())

    def block(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    variants = {"resident": resident, "stream_depth2": stream, "reference_pageable_f32": reference}
    for fn in variants.values():
        block(fn, 10)
    samples = {k: [] for k in variants}
    for _ in range(args.blocks):
        for k, fn in variants.items():
            samples[k].append(block(fn, args.iterations))
    out = {k: summary(s) for k, s in samples.items()}
    for k in ("stream_depth2", "reference_pageable_f32"):
        out[k]["added_ms_over_resident"] = round(out[k]["ms"] - out["resident"]["ms"], 4)
    out["gaussians"] = model.num_static + model.num_dynamic
    out["iterations_per_block"] = args.iterations
    out["frame_bytes_u8"], out["frame_bytes_f32"], out["store_bytes"] = H * W * 3, H * W * 12, store.bytes()
    nt.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_time_cfg3.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--float-only", action="store_true", help="(child of measurement 2) time the float entries of the loaded library and print one JSON line")
    ap.add_argument("--steps", type=int, default=50, help="forward + backward pairs per block")
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--processes", type=int, default=4, help="measurement 2: processes per library")
    ap.add_argument("--iterations", type=int, default=40, help="measurement 3: trainer iterations per block")
    ap.add_argument("--P", type=int, default=None, help="Gaussians of measurement 3 (default: config 3's 1.0 M)")
    ap.add_argument("--skip-arrival", action="store_true")
    args = ap.parse_args()
    if args.float_only:
        return float_only(args)
    result = {"image": [H, W], "device": torch.cuda.get_device_name(0), "pairs_per_block": args.steps,
              "table_placement": "kernel arguments (1 KB by value) -> LDS, one load per thread per workgroup"}
    L = Loss()
    loss = rounds({"a_float": L.a_float, "b_u8_stride3": L.b_u8, "c_float_plus_torch_conversion": L.c_composed}, args.steps, args.blocks)
    loss["b_minus_a_ms"] = round(loss["b_u8_stride3"]["ms"] - loss["a_float"]["ms"], 4)
    loss["b_not_above_c"] = loss["b_u8_stride3"]["ms"] <= loss["c_float_plus_torch_conversion"]["ms"]
    result["1_loss_forward_backward"] = loss
    del L
    torch.cuda.synchronize()
    if args.parent_lib:
        result["2_float_entries_against_parent"] = across_processes(args)
    if not args.skip_arrival:
        result["3_frame_arrival_per_iteration"] = arrival(args)
    with open(args.out, "w") as f:
        f.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
