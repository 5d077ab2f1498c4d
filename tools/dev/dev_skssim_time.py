"""Times scikit-image's SSIM of one rendered view (evaluate.frame_skssim: SKSSIM and SKSSIM2 from one pass) at config 3's image size
(1352 x 1014) and writes profiles/skssim_time_cfg3.json (or --out).

In ONE process, the variants alternating in rounds, device events around windows of launches that last at least --window seconds each,
after a warm-up:
  sk_float   evaluate.frame_skssim on float32 [3,H,W] ground truth (two launches);
  sk_u8      the same on uint8 [H,W,3] ground truth through the default table;
  torch      a torch composition of the same metric on the GPU: one avg_pool2d(..., 7, stride=1) over the stacked five product maps
             x, y, xx, yy, xy, the sample covariances and S for both data ranges, two means (results stay on the device);
  metrics    evaluate.frame_metrics without out_u8, for scale.
Condition: sk_float is faster than torch by more than the spread (max - min over the windows) of either; the ratio is recorded.
With --parent-lib PATH (a libex4d_hip.so built from the parent commit): frame_metrics and the training loss's forward + backward, which
share a source file with the new kernel, in SEPARATE processes, this tree's library and the parent's alternating (each child is this
script with --child and EX4D_HIP_LIB set).  Condition: this tree's median is not above the parent's by more than the spread
(max - min) of the parent's own runs, which is recorded beside it.
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from ex4dgs_amd import _abi, evaluate  # noqa: E402
from ex4dgs_amd.frames import gt_lut  # noqa: E402
from ex4dgs_amd.loss import _WINDOW  # noqa: E402

H, W = 1014, 1352
DEV = "cuda"
HW = H * W
LAMBDA = 0.2
# bytes per pixel read by the call: float32 [3,H,W] = 12, uint8 [H,W,3] = 3 (nothing per pixel is written)
ALGORITHMIC_BYTES = {"sk_float": (12 + 12) * HW, "sk_u8": (12 + 3) * HW, "metrics": (12 + 12) * HW}


class Score:
    def __init__(self, sk=True):
        g = torch.Generator().manual_seed(1)
        f32 = dict(dtype=torch.float32, device=DEV)
        lib = _abi._lib if _abi._lib is not None else _abi.load()
        self.img = (torch.rand(3, H, W, generator=g) * 1.2 - 0.1).to(DEV)
        self.gt8 = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
        self.gtf = gt_lut().to(DEV)[self.gt8.long()].permute(2, 0, 1).contiguous()
        self.row = torch.empty(8, dtype=torch.float64, device=DEV)
        self.scratch = torch.empty(lib.ex4d_frame_metrics_scratch_floats(H, W), **f32)
        if sk:
            self.row_sk = torch.empty(4, dtype=torch.float64, device=DEV)
            self.scratch_sk = torch.empty(lib.ex4d_frame_skssim_scratch_floats(H, W), **f32)
        # the training loss, forward + backward (as tools/dev/dev_frames_time.py times it)
        self.loss, self.l1e, self.sse = torch.empty(1, **f32), torch.empty(H, W, **f32), torch.empty(H, W, **f32)
        self.dmaps, self.grad = torch.empty(9, H, W, **f32), torch.empty(3, H, W, **f32)
        self.loss_scratch = torch.empty(lib.ex4d_l1_ssim_scratch_floats(H, W), **f32)
        self.gl = torch.ones(1, **f32)

    def sk_float(self):
        evaluate.frame_skssim(self.img, self.gtf, row=self.row_sk, scratch=self.scratch_sk)

    def sk_u8(self):
        evaluate.frame_skssim(self.img, self.gt8, row=self.row_sk, scratch=self.scratch_sk)

    def torch_composition(self):
        with torch.no_grad():
            x, y = self.img, self.gtf
            u = F.avg_pool2d(torch.stack([x, y, x * x, y * y, x * y]), 7, stride=1)        # [5,3,H-6,W-6]: valid windows only
            ux, uy, uxx, uyy, uxy = u
            k = 49.0 / 48.0
            vx, vy, vxy = k * (uxx - ux * ux), k * (uyy - uy * uy), k * (uxy - ux * uy)
            out = []
            for R in (1.0, 2.0):
                C1, C2 = (0.01 * R) ** 2, (0.03 * R) ** 2
                S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
                out.append(S.mean(dim=(1, 2)).mean())
        return out

    def metrics(self):
        evaluate.frame_metrics(self.img, self.gtf, row=self.row, scratch=self.scratch)

    def loss_fwd_bwd(self):
        with _abi.stream(self.img.device) as s:
            _abi.call("ex4d_l1_ssim_forward", 3, H, W, self.img.data_ptr(), self.gtf.data_ptr(), LAMBDA, _WINDOW.ctypes.data, self.loss.data_ptr(),
                      self.l1e.data_ptr(), self.sse.data_ptr(), self.dmaps.data_ptr(), self.loss_scratch.data_ptr(), s)
            _abi.call("ex4d_l1_ssim_backward", 3, H, W, self.img.data_ptr(), self.gtf.data_ptr(), LAMBDA, _WINDOW.ctypes.data, self.dmaps.data_ptr(),
                      self.gl.data_ptr(), self.grad.data_ptr(), s)


def event_block(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def summary(samples, steps, digits=4):
    s = sorted(samples)
    return {"ms": round(statistics.median(s), digits), "min_ms": round(s[0], digits), "max_ms": round(s[-1], digits),
            "spread_ms": round(s[-1] - s[0], digits), "windows": len(s), "calls_per_window": steps,
            "shortest_window_s": round(s[0] * steps / 1e3, 3)}


def windows(variants, window, n):
    """Alternating windows of at least `window` seconds; the call count of a window comes from a 500-call probe plus a tenth."""
    steps = {}
    for k, fn in variants.items():
        event_block(fn, 10)
        steps[k] = max(10, math.ceil(1.1 * window * 1e3 / event_block(fn, 500)))
    samples = {k: [] for k in variants}
    for _ in range(n):
        for k, fn in variants.items():
            samples[k].append(event_block(fn, steps[k]))
    times = {k: summary(s, steps[k]) for k, s in samples.items()}
    for k, t in times.items():
        assert t["shortest_window_s"] >= window, (k, t)
    return times


def child(args):
    # the parent's library lacks the new names: bind what it has (load() would insist on the whole table)
    lib = ctypes.CDLL(_abi.library_path())
    for _, protos in _abi.PROTOTYPES.values():
        for name, restype, argtypes, _ in protos:
            if hasattr(lib, name):
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = restype, list(argtypes)
    _abi._lib = lib
    S = Score(sk=False)
    times = windows({"metrics": S.metrics, "loss_fwd_bwd": S.loss_fwd_bwd}, args.window, args.windows)
    print(json.dumps({"child": {k: t["ms"] for k, t in times.items()}, "lib": _abi.library_path()}))


def across_processes(args):
    runs = {who: {"metrics": [], "loss_fwd_bwd": []} for who in ("this", "parent")}
    for _ in range(args.processes):
        for who, lib in (("parent", args.parent_lib), ("this", None)):
            env = dict(os.environ)
            env.pop("EX4D_HIP_LIB", None)
            if lib:
                env["EX4D_HIP_LIB"] = os.path.abspath(lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--window", str(args.child_window), "--windows", "3"],
                                 env=env, capture_output=True, text=True, timeout=300)
            if out.returncode:
                raise RuntimeError(f"{who}: child failed ({out.returncode}): {out.stderr[-400:]}")
            got = json.loads(out.stdout.strip().splitlines()[-1])["child"]
            for k in got:
                runs[who][k].append(got[k])
    result = {}
    for k in ("metrics", "loss_fwd_bwd"):
        this, parent = statistics.median(runs["this"][k]), statistics.median(runs["parent"][k])
        spread = max(runs["parent"][k]) - min(runs["parent"][k])
        result[k] = {"this_ms": runs["this"][k], "parent_ms": runs["parent"][k], "this_median_ms": round(this, 4), "parent_median_ms": round(parent, 4),
                     "parent_spread_ms": round(spread, 4), "difference_ms": round(this - parent, 4),
                     "not_slower_than_parent_beyond_its_spread": this - parent <= spread}
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skssim_time_cfg3.json"))
    ap.add_argument("--window", type=float, default=1.0, help="seconds of launches per timed window, at least")
    ap.add_argument("--windows", type=int, default=5, help="windows per variant")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--processes", type=int, default=4, help="--parent-lib: processes per library")
    ap.add_argument("--child-window", type=float, default=0.5, help="--parent-lib: seconds per window in a child (three windows per variant)")
    ap.add_argument("--child", action="store_true", help="(child of --parent-lib) time frame_metrics and the loss of the loaded library, print one JSON line")
    args = ap.parse_args()
    if args.child:
        return child(args)
    S = Score()
    # the variants agree on what they compute before anything is timed
    S.sk_float()
    a = S.row_sk.cpu().tolist()
    b = [float(v) for v in S.torch_composition()]
    S.sk_u8()
    c = S.row_sk.cpu().tolist()
    assert abs(a[0] - b[0]) < 1e-5 and abs(a[1] - b[1]) < 1e-5 and a[2:] == [0.0, 0.0] and c == a, (a, b, c)
    times = windows({"sk_float": S.sk_float, "torch": S.torch_composition, "sk_u8": S.sk_u8, "metrics": S.metrics}, args.window, args.windows)
    sk, tc = times["sk_float"], times["torch"]
    result = {"image": [H, W], "device": torch.cuda.get_device_name(0), "window_seconds_at_least": args.window, "times": times,
              "values": {"sk_float": a[:2], "torch": b},
              "sk_float_against_torch": {"torch_minus_sk_ms": round(tc["ms"] - sk["ms"], 4), "ratio": round(tc["ms"] / sk["ms"], 2),
                                         "sk_faster_by_more_than_either_spread": tc["ms"] - sk["ms"] > max(sk["spread_ms"], tc["spread_ms"])},
              "algorithmic_bytes": ALGORITHMIC_BYTES,
              "GBps_of_algorithmic_bytes": {k: round(v / times[k]["ms"] / 1e6, 1) for k, v in ALGORITHMIC_BYTES.items()}}
    if args.parent_lib:
        result["against_parent_in_separate_processes"] = across_processes(args)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
