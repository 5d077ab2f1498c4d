"""Times the scoring of one rendered view at config 3's image size (1352 x 1014) and writes profiles/metrics_time_cfg3.json (or --out).

For both kinds of ground truth (float32 [3,H,W] planes; uint8 [H,W,3] bytes through the default table), in ONE process, the variants
alternating in rounds, device events around windows of launches that last at least --window seconds each, after a warm-up:
  (a) evaluate.frame_metrics with out_u8: L1, MSE, PSNR, SSIM and the 8-bit frame from one pass (two launches);
  (b) what the library offered for the same outputs before: loss.psnr + loss.ssim + loss.l1_loss + torch's save_image quantisation
      (mul, add_, clamp_, to(uint8), permute, contiguous), with the torch conversion lut[gt8.long()].permute(2,0,1).contiguous() in
      front for byte ground truth.
Condition: (a) is faster than (b) by more than the spread (max - min over the windows) of either.  The algorithmic bytes of each are
recorded beside the times (tensor reads and writes of every kernel of the composition, counted once each; no cache effects).
With --training-loss-check the training loss's own times against the parent build (dev_frames_time.py, measurement 2) are copied in.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from ex4dgs_amd import _abi, evaluate, loss  # noqa: E402
from ex4dgs_amd.frames import gt_lut  # noqa: E402

H, W = 1014, 1352
DEV = "cuda"
HW = H * W

# bytes per pixel of each step: float32 [3,H,W] = 12, uint8 [H,W,3] = 3, int64 [H,W,3] = 24
BYTES = {
    "a_float": {"frame_metrics": 12 + 12 + 3},
    "a_u8": {"frame_metrics": 12 + 3 + 3},
    "b_float": {"psnr (sub, pow, mean)": 36 + 24 + 12, "ssim (fused forward at lambda 1: reads 24, dmaps 36, error maps 8)": 24 + 36 + 8,
                "l1_loss (sub, abs, mean)": 36 + 24 + 12, "quantisation (mul, add_, clamp_, to, permute+contiguous)": 24 + 24 + 24 + 15 + 6},
    "conversion": {"lut[gt8.long()].permute.contiguous (long, index, contiguous)": 3 + 24 + 24 + 12 + 24},
}


def algorithmic_bytes():
    per_pixel = {k: sum(v.values()) for k, v in BYTES.items()}
    per_pixel["b_u8"] = per_pixel["b_float"] + per_pixel.pop("conversion")
    return {k: v * HW for k, v in per_pixel.items()}, BYTES


class Score:
    def __init__(self):
        g = torch.Generator().manual_seed(1)
        self.lut_dev = gt_lut().to(DEV)
        self.img = (torch.rand(3, H, W, generator=g) * 1.2 - 0.1).to(DEV)
        self.gt8 = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(DEV)
        self.gtf = self.lut_dev[self.gt8.long()].permute(2, 0, 1).contiguous()
        self.row = torch.empty(8, dtype=torch.float64, device=DEV)
        self.out = torch.empty(H, W, 3, dtype=torch.uint8, device=DEV)
        self.scratch = torch.empty(_abi.load().ex4d_frame_metrics_scratch_floats(H, W), dtype=torch.float32, device=DEV)

    def a_float(self):
        evaluate.frame_metrics(self.img, self.gtf, out_u8=self.out, row=self.row, scratch=self.scratch)

    def a_u8(self):
        evaluate.frame_metrics(self.img, self.gt8, out_u8=self.out, row=self.row, scratch=self.scratch)

    def b_float(self, gtf=None):
        gtf = self.gtf if gtf is None else gtf
        with torch.no_grad():
            psnr = loss.psnr(self.img.unsqueeze(0), gtf.unsqueeze(0))
            ssim = loss.ssim(self.img.unsqueeze(0), gtf.unsqueeze(0))
            l1 = loss.l1_loss(self.img, gtf)
            frame = self.img.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()
        return psnr, ssim, l1, frame

    def b_u8(self):
        return self.b_float(self.lut_dev[self.gt8.long()].permute(2, 0, 1).contiguous())


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
            "spread_ms": round(s[-1] - s[0], digits), "windows": len(s), "calls_per_window": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_time_cfg3.json"))
    ap.add_argument("--window", type=float, default=1.0, help="seconds of launches per timed window, at least")
    ap.add_argument("--windows", type=int, default=5, help="windows per variant")
    ap.add_argument("--training-loss-check", default=None, help="a result file of `dev_frames_time.py --parent-lib ... --skip-arrival` from the same "
                    "session: the training loss's own times against the parent build, recorded beside these")
    args = ap.parse_args()
    S = Score()
    variants = {"a_float": S.a_float, "b_float": S.b_float, "a_u8": S.a_u8, "b_u8": S.b_u8}
    # the two agree on what they compute before anything is timed
    S.a_float()
    psnr, ssim, l1, frame = S.b_float()
    row = S.row.cpu().tolist()
    assert abs(row[0] - float(l1)) < 1e-5 and abs(row[2] - float(psnr)) < 1e-3 and abs(row[3] - float(ssim)) < 1e-5 and torch.equal(frame, S.out)
    steps = {}
    for k, fn in variants.items():                 # warm-up, and the number of calls that fills a window
        event_block(fn, 10)
        # sized from a probe long enough to run at the steady rate (a short probe overstates the time per call), with a margin
        steps[k] = max(10, math.ceil(1.1 * args.window * 1e3 / event_block(fn, 500)))
    samples = {k: [] for k in variants}
    for _ in range(args.windows):
        for k, fn in variants.items():
            samples[k].append(event_block(fn, steps[k]))
    times = {k: summary(s, steps[k]) for k, s in samples.items()}
    for k, s in samples.items():
        times[k]["shortest_window_s"] = round(min(s) * steps[k] / 1e3, 3)
        assert times[k]["shortest_window_s"] >= args.window, (k, times[k])
    total, breakdown = algorithmic_bytes()
    result = {"image": [H, W], "device": torch.cuda.get_device_name(0), "window_seconds_at_least": args.window, "times": times,
              "algorithmic_bytes": total, "algorithmic_bytes_per_pixel": breakdown}
    for kind in ("float", "u8"):
        a, b = times["a_" + kind], times["b_" + kind]
        result[kind] = {"b_minus_a_ms": round(b["ms"] - a["ms"], 4), "speedup": round(b["ms"] / a["ms"], 2),
                        "a_faster_by_more_than_either_spread": b["ms"] - a["ms"] > max(a["spread_ms"], b["spread_ms"]),
                        "a_GBps_of_algorithmic_bytes": round(total["a_" + kind] / a["ms"] / 1e6, 1)}
    if args.training_loss_check:
        with open(args.training_loss_check) as f:
            check = json.load(f)
        result["training_loss_against_parent"] = {"tool": "tools/dev/dev_frames_time.py --parent-lib", "1_loss_forward_backward": check["1_loss_forward_backward"],
                                                  "2_float_entries_against_parent": check["2_float_entries_against_parent"]}
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
