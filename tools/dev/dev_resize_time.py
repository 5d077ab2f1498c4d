"""Times the on-device resize of decoded frames at config 3's frame (2028 x 2704 -> 1014 x 1352, bilinear) and writes
profiles/resize_time_cfg3.json (or --out).  First the output is compared with the numpy restatement (tests/resize_ref.py): a resize
that is not PIL's bytes is not timed.

  a. The two kernels of ex4d_resize_u8 by device events, in --windows windows of at least --window-s seconds each; the share of the
     HBM peak the 37.0 MB of algorithmic traffic then amounts to (16.45 read + 8.23 written, 8.23 read + 4.11 written), and the spread.
  b. Alternating with (a), window by window in the same process: the nearest torch composition (float, interpolate(mode="bilinear",
     antialias=True), round, byte).  NOT bit-equal to PIL (the share of differing bytes is recorded): a yardstick for time only.
  c. Wall clock per NativeTrainer.step at config 3, blocks that end in a device synchronise:
       stream_full_resolution   FrameStream(source_size=...) fed [2028,2704,3] frames: pinned copy, 16.4 MB upload, resize on the copy stream;
       stream_pre_resized       the same stream fed [1014,1352,3] frames (the path before this tool's feature);
       host_pil_resize          the same with PIL's Image.resize on the host in front of each push (where PIL imports; its time is this
                                machine's CPU, stated beside it).
  d. With --parent-lib PATH (a libex4d_hip.so of the parent commit): the float loss forward + backward at 1352 x 1014 in separate
     processes, this tree's library and the parent's alternating, exactly as tools/dev/dev_frames_time.py measures it (its code is
     used).  "Unchanged" = the difference of the medians is inside the spread of the parent's own runs.
"""
import argparse
import json
import math
import os
import platform
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dev_frames_time as ft  # noqa: E402
from ex4dgs_amd import frames  # noqa: E402
from tests import resize_ref  # noqa: E402

H_IN, W_IN, H, W = 2028, 2704, 1014, 1352
DEV = "cuda"
HBM_PEAK = 8.0e12                                           # bytes / s, MI355X
TRAFFIC = (H_IN * W_IN + 2 * H_IN * W + H * W) * 3          # 37.0 MB


def check(src_host):
    want = resize_ref.resize(src_host.numpy(), (H, W))
    got = frames.resize_u8(src_host.to(DEV), plan=frames.resize_plan((H_IN, W_IN), (H, W), device=DEV)).cpu().numpy()
    bad = int((got != want).sum())
    if bad:
        raise RuntimeError(f"{bad} bytes differ from the restatement: not timed")
    return want


def torch_nearest(src):
    x = src.permute(2, 0, 1)[None].float()
    y = torch.nn.functional.interpolate(x, size=(H, W), mode="bilinear", antialias=True)
    return y.round().clamp(0, 255).byte()[0].permute(1, 2, 0).contiguous()


def kernels(args, src_host, want):
    src = src_host.to(DEV)
    plan = frames.resize_plan((H_IN, W_IN), (H, W), device=DEV)
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=DEV)
    variants = {"a_resize_u8": lambda: frames.resize_u8(src, out=out, plan=plan), "b_torch_interpolate_antialias_NOT_bit_equal": lambda: torch_nearest(src)}
    steps = {}
    for k, fn in variants.items():
        ft.event_block(fn, 5)
        steps[k] = max(10, math.ceil(args.window_s * 1e3 / ft.event_block(fn, 20)))
    samples = {k: [] for k in variants}
    for _ in range(args.windows):
        for k, fn in variants.items():
            samples[k].append(ft.event_block(fn, steps[k]))
    res = {k: dict(ft.summary(s), calls_per_window=steps[k]) for k, s in samples.items()}
    a = res["a_resize_u8"]
    a["algorithmic_bytes"] = TRAFFIC
    a["share_of_hbm_peak"] = round(TRAFFIC / (a["ms"] * 1e-3) / HBM_PEAK, 4)
    a["spread_ms"] = round(a["max_ms"] - a["min_ms"], 4)
    differing = float((torch_nearest(src).cpu().numpy() != want).mean())
    res["b_torch_interpolate_antialias_NOT_bit_equal"]["share_of_bytes_that_differ_from_pil"] = round(differing, 4)
    return res


def arrival(args):
    from ex4dgs_amd.native_trainer import NativeTrainer
    from ex4dgs_amd.scene import CONFIGS, make_scene
    cfg = CONFIGS["cfg3"]
    assert (cfg.height, cfg.width) == (H, W)
    model, cam, bg = make_scene("cfg3", P=args.P, device=DEV, fused=True)
    cam, bg = cam.to(DEV), bg.to(DEV)
    nt = NativeTrainer(model, cam, optimizer=True, lrs={n: 1e-7 for n in model.PARAM_NAMES}, near=cfg.min_depth, far=cfg.max_depth)
    n_frames = 4
    g = torch.Generator().manual_seed(2)
    full = [torch.randint(0, 256, (H_IN, W_IN, 3), generator=g, dtype=torch.uint8) for _ in range(n_frames)]
    small = [torch.from_numpy(resize_ref.resize(f.numpy(), (H, W))) for f in full]
    fs = frames.FrameStream(H, W, depth=2, device=DEV, source_size=(H_IN, W_IN))
    times = (0, 137, 299, 41, 250)
    try:
        from PIL import Image
    except ImportError:
        Image = None

    def pil(f):
        return torch.from_numpy(np.asarray(Image.fromarray(f.numpy()).resize((W, H), resample=2)))

    def run(source):
        def block(steps):
            fs.push(source(0))
            for i in range(steps):
                if i + 1 < steps:
                    fs.push(source((i + 1) % n_frames))
                nt.step(cam, bg, times[i % 5], fs.pop())
        return block

    variants = {"stream_full_resolution": run(lambda i: full[i]), "stream_pre_resized": run(lambda i: small[i])}
    if Image is not None:
        variants["host_pil_resize"] = run(lambda i: pil(full[i]))

    def block(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    for fn in variants.values():
        block(fn, 6)
    samples = {k: [] for k in variants}
    for _ in range(args.blocks):
        for k, fn in variants.items():
            samples[k].append(block(fn, args.iterations))
    out = {k: ft.summary(s) for k, s in samples.items()}
    for k in out:
        if k != "stream_pre_resized":
            out[k]["added_ms_over_pre_resized"] = round(out[k]["ms"] - out["stream_pre_resized"]["ms"], 4)
    if Image is None:
        out["host_pil_resize"] = "not measured: PIL does not import here"
    else:
        t0 = time.perf_counter()
        for i in range(n_frames):
            pil(full[i])
        out["host_pil_resize"]["pil_resize_alone_ms"] = round((time.perf_counter() - t0) / n_frames * 1e3, 2)
        out["host_pil_resize"]["cpu"] = platform.processor() or platform.machine()
    out["gaussians"] = model.num_static + model.num_dynamic
    out["iterations_per_block"] = args.iterations
    out["source_frame_bytes"], out["frame_bytes"] = H_IN * W_IN * 3, H * W * 3
    nt.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_time_cfg3.json"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=50, help="measurement d: forward + backward pairs per block")
    ap.add_argument("--blocks", type=int, default=5, help="measurements c and d: blocks")
    ap.add_argument("--processes", type=int, default=4, help="measurement d: processes per library")
    ap.add_argument("--iterations", type=int, default=30, help="measurement c: trainer iterations per block")
    ap.add_argument("--P", type=int, default=None, help="Gaussians of measurement c (default: config 3's 1.0 M)")
    ap.add_argument("--skip-arrival", action="store_true")
    args = ap.parse_args()
    result = {"source": [H_IN, W_IN], "image": [H, W], "resample": "bilinear", "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK}
    src_host = torch.randint(0, 256, (H_IN, W_IN, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    want = check(src_host)
    result["equals_the_restatement"] = True
    result["ab_kernels"] = kernels(args, src_host, want)
    result["c_trainer_step_wall_clock"] = "not measured" if args.skip_arrival else arrival(args)
    torch.cuda.synchronize()
    result["d_loss_against_parent"] = ft.across_processes(args) if args.parent_lib else "not measured"
    with open(args.out, "w") as f:
        f.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
