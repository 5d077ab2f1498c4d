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
With --parent-lib PATH (a libex4d_hip.so built from the parent commit): every call of ex4d_loss.hip's rolling window -- the training
loss's forward + backward, frame_metrics and frame_skssim, each on float32 and on uint8 ground truth -- in SEPARATE processes, this
tree's library and the parent's alternating (each child is this script with --child and EX4D_HIP_LIB set).  Condition: this tree's
median is not above the parent's by more than the spread (max - min) of the parent's own runs, which is recorded beside it.  And the
BITS: one more child per library (--child --digests) hashes every output buffer of those calls, pre-filled with NaN, at the tiling-edge
shapes of the tests, at this image size and on a pair with NaN and +-inf pixels; every digest of this tree equals the parent's.
--ab: only that comparison (nothing else is timed); profiles/loss_walk_ab.json is `--ab --parent-lib PATH --out` of it.
"""
import argparse
import hashlib
import json
import math
import os
import statistics
import subprocess
import sys

import numpy as np
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


class LossBuffers:
    """The caller's buffers of the training loss's forward + backward through the C ABI, every output pre-filled with NaN."""
    OUTPUTS = ("loss", "l1_errors", "ssim_errors", "dmaps", "grad_img")

    def __init__(self, C, H, W):
        nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
        self.loss, self.l1_errors, self.ssim_errors, self.dmaps, self.grad_img = nan(1), nan(H, W), nan(H, W), nan(3 * C, H, W), nan(C, H, W)
        self.scratch = nan(_abi.load().ex4d_l1_ssim_scratch_floats(H, W))
        self.grad_loss = torch.ones(1, dtype=torch.float32, device=DEV)

    def forward_backward(self, img, gt, lam):
        """gt: float32 [C,H,W], or uint8 [H,W,3|4] through the default table."""
        C, H, W = img.shape
        u8 = gt.dtype == torch.uint8
        head = (H, W, img.data_ptr(), gt.data_ptr(), gt.shape[2], None) if u8 else (C, H, W, img.data_ptr(), gt.data_ptr())
        with _abi.stream(img.device) as s:
            _abi.call("ex4d_l1_ssim_forward" + "_u8" * u8, *head, lam, _WINDOW.ctypes.data, self.loss.data_ptr(), self.l1_errors.data_ptr(),
                      self.ssim_errors.data_ptr(), self.dmaps.data_ptr(), self.scratch.data_ptr(), s)
            _abi.call("ex4d_l1_ssim_backward" + "_u8" * u8, *head, lam, _WINDOW.ctypes.data, self.dmaps.data_ptr(), self.grad_loss.data_ptr(),
                      self.grad_img.data_ptr(), s)


class Score:
    def __init__(self):
        g = torch.Generator().manual_seed(1)
        f32 = dict(dtype=torch.float32, device=DEV)
        lib = _abi.load()
        self.img = (torch.rand(3, H, W, generator=g) * 1.2 - 0.1).to(DEV)
        self.gt8 = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
        self.gtf = gt_lut().to(DEV)[self.gt8.long()].permute(2, 0, 1).contiguous()
        self.row = torch.empty(8, dtype=torch.float64, device=DEV)
        self.scratch = torch.empty(lib.ex4d_frame_metrics_scratch_floats(H, W), **f32)
        self.row_sk = torch.empty(4, dtype=torch.float64, device=DEV)
        self.scratch_sk = torch.empty(lib.ex4d_frame_skssim_scratch_floats(H, W), **f32)
        self.loss = LossBuffers(3, H, W)

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

    def metrics_u8(self):
        evaluate.frame_metrics(self.img, self.gt8, row=self.row, scratch=self.scratch)

    def loss_fwd_bwd(self):
        self.loss.forward_backward(self.img, self.gtf, LAMBDA)

    def loss_fwd_bwd_u8(self):
        self.loss.forward_backward(self.img, self.gt8, LAMBDA)

    def against_parent(self):
        """The six variants of --parent-lib."""
        return {"loss_fwd_bwd": self.loss_fwd_bwd, "loss_fwd_bwd_u8": self.loss_fwd_bwd_u8, "metrics": self.metrics,
                "metrics_u8": self.metrics_u8, "sk_float": self.sk_float, "sk_u8": self.sk_u8}


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


def digests():
    """{case and buffer: sha256} of every output buffer of the rolling window's calls, each pre-filled with NaN (out_u8: with 0xA5): the
    loss at every shape of tests/loss_cases.sweep_shapes() (uint8 ground truth at the three-channel ones, 3 and 4 bytes per pixel), both
    LAMBDAS; frame_metrics at tests/metrics_ref.SHAPES, its four flag combinations; frame_skssim at tests/skssim_cases.SHAPES, with and
    without the clamp; all of them on this module's 1352 x 1014 pair, the two scoring calls on a pair with NaN and +-inf pixels."""
    from tests import loss_cases, metrics_ref, skssim_cases
    out = {}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)

    def put(key, t):
        out[key] = hashlib.sha256(t.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()

    def loss(key, img, gt, lambdas=loss_cases.LAMBDAS):
        for lam in lambdas:
            b = LossBuffers(*img.shape)
            b.forward_backward(img, gt, lam)
            for name in LossBuffers.OUTPUTS:
                put(f"loss {key} lambda={lam} {name}", getattr(b, name))

    def metrics(key, img, gt):
        for clamp in (False, True):
            for quant in ("round", "trunc"):
                row = torch.full((8,), float("nan"), dtype=torch.float64, device=DEV)
                out_u8 = torch.full((img.shape[1], img.shape[2], 3), 0xA5, dtype=torch.uint8, device=DEV)
                evaluate.frame_metrics(img, gt, clamp=clamp, quant=quant, out_u8=out_u8, row=row)
                put(f"metrics {key} clamp={clamp} quant={quant} row", row)
                put(f"metrics {key} clamp={clamp} quant={quant} out_u8", out_u8)

    def skssim(key, img, gt):
        for clamp in (False, True):
            row = torch.full((4,), float("nan"), dtype=torch.float64, device=DEV)
            evaluate.frame_skssim(img, gt, clamp=clamp, row=row)
            put(f"skssim {key} clamp={clamp} row", row)

    def both_kinds(call, shape, image, gt):
        """float ground truth, and the decoded bytes of tests/metrics_ref.make_bytes at 3 and 4 bytes per pixel"""
        call(f"{shape} float", image, dev(gt))
        for stride in (3, 4):
            call(f"{shape} u8 stride={stride}", image, dev(metrics_ref.make_bytes(shape[-2], shape[-1], stride)))

    for shape in loss_cases.sweep_shapes():
        image, gt = loss_cases.make_pair(shape)
        if shape[0] == 3:
            both_kinds(loss, shape, dev(image), gt)
        else:
            loss(f"{shape} float", dev(image), dev(gt))
    for call, shapes in ((metrics, metrics_ref.SHAPES), (skssim, skssim_cases.SHAPES)):
        for shape in shapes:
            image, gt = metrics_ref.make_pair(*shape)
            both_kinds(call, shape, dev(image), gt)
    S = Score()
    for kind, gt in (("float", S.gtf), ("u8", S.gt8)):
        loss(f"{(3, H, W)} {kind}", S.img, gt, (LAMBDA,))
        metrics(f"{(H, W)} {kind}", S.img, gt)
        skssim(f"{(H, W)} {kind}", S.img, gt)
    shape = skssim_cases.LOW_VARIANCE_SHAPE
    image, gt = metrics_ref.make_pair(*shape)
    image[0, 10, 10], image[1, 20, 70], image[2, 52, 138], gt[1, 30, 5], gt[2, 0, 64] = np.nan, np.inf, -np.inf, np.nan, np.inf
    for call in (metrics, skssim):
        call(f"{shape} non-finite float", dev(image), dev(gt))
        call(f"{shape} non-finite u8", dev(image), dev(metrics_ref.make_bytes(*shape)))
    return out


def child(args):
    if args.digests:
        print(json.dumps({"digests": digests(), "lib": _abi.library_path()}))
        return
    times = windows(Score().against_parent(), args.window, args.windows)
    print(json.dumps({"child": {k: t["ms"] for k, t in times.items()}, "lib": _abi.library_path(), "device": torch.cuda.get_device_name(0)}))


def run_child(lib, *options):
    """This script with --child in a process of its own, on `lib` (None: this tree's library); the JSON line it prints."""
    env = dict(os.environ)
    env.pop("EX4D_HIP_LIB", None)
    if lib:
        env["EX4D_HIP_LIB"] = os.path.abspath(lib)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", *options], env=env, capture_output=True, text=True, timeout=300)
    if out.returncode:
        raise RuntimeError(f"child on {lib or 'this tree'} failed ({out.returncode}): {out.stderr[-400:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def across_processes(args):
    runs, device = {"this": {}, "parent": {}}, None
    for _ in range(args.processes):
        for who, lib in (("parent", args.parent_lib), ("this", None)):
            got = run_child(lib, "--window", str(args.child_window), "--windows", "3")
            device = got["device"]
            print(who, got["child"], file=sys.stderr, flush=True)
            for k, ms in got["child"].items():
                runs[who].setdefault(k, []).append(ms)
    result = {"device": device}
    for k in runs["this"]:
        this, parent = statistics.median(runs["this"][k]), statistics.median(runs["parent"][k])
        spread = max(runs["parent"][k]) - min(runs["parent"][k])
        result[k] = {"this_ms": runs["this"][k], "parent_ms": runs["parent"][k], "this_median_ms": round(this, 4), "parent_median_ms": round(parent, 4),
                     "parent_spread_ms": round(spread, 4), "difference_ms": round(this - parent, 4),
                     "not_slower_than_parent_beyond_its_spread": this - parent <= spread}
    return result


def digests_against_parent(args):
    this, parent = run_child(None, "--digests")["digests"], run_child(args.parent_lib, "--digests")["digests"]
    differing = sorted(k for k in set(this) | set(parent) if this.get(k) != parent.get(k))
    print("digests:", len(this), "buffers,", len(differing), "differ", differing[:20], file=sys.stderr, flush=True)
    return {"buffers": len(this), "differing": differing, "all_equal": not differing and len(this) > 0,
            "sha256_of_the_digests": hashlib.sha256(json.dumps(this, sort_keys=True).encode()).hexdigest()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skssim_time_cfg3.json"))
    ap.add_argument("--window", type=float, default=1.0, help="seconds of launches per timed window, at least")
    ap.add_argument("--windows", type=int, default=5, help="windows per variant")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--processes", type=int, default=4, help="--parent-lib: processes per library")
    ap.add_argument("--child-window", type=float, default=0.5, help="--parent-lib: seconds per window in a child (three windows per variant)")
    ap.add_argument("--ab", action="store_true", help="--parent-lib: only the comparison with the parent's library, times and digests")
    ap.add_argument("--child", action="store_true", help="(child of --parent-lib) time the six variants on the loaded library, print one JSON line")
    ap.add_argument("--digests", action="store_true", help="(with --child) hash the output buffers instead")
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.ab:
        result = {"image": [H, W], "processes_per_library": args.processes, "child_window_seconds_at_least": args.child_window,
                  "digests_against_parent": digests_against_parent(args), "against_parent_in_separate_processes": across_processes(args)}
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
        print(json.dumps(result))
        return
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
