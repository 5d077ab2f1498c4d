"""Captures tests/golden/metrics.npz from the reference checkout: what the reference's OWN psnr, ssim and l1_loss give for a seeded
render against a decoded 8-bit frame, and the 8-bit pixels its viewer path makes of that render.

    python tests/golden/make_golden_metrics.py /path/to/reference

Nothing of the reference is copied: utils/image_utils.py and utils/loss_utils.py are imported (third-party imports they do not need
here are stubbed when missing), and the byte conversion of train.py is cut out of the file at capture time -- the expression inside
`net_image_bytes = memoryview(...)` up to its `.cpu()` -- compiled and evaluated on the seeded render.  Runs on the CPU.

Recorded, for the RGB [53,139,3] image of frames.npz as ground truth under im_scale 1.0 and 1.7 (frames.gt_lut: bit for bit the
reference loader's floats, tests/test_cpu_frames.py) and a seeded float32 [3,53,139] render that reaches below 0 and above 1:
  render                      the render
  im_scales                   (1.0, 1.7)
  {psnr,ssim,l1}_{k}          float32, the render as it is       (render.py:76-77 call forms; l1_loss as train.py:347)
  {psnr,ssim,l1}_clamped_{k}  float32, torch.clamp(render, 0, 1) (train.py:342-348)
  bytes_trunc                 uint8 [53,139,3], train.py:101
"""
import importlib
import os
import re
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "metrics.npz")
SCALES = (1.0, 1.7)


def reference_functions(ref):
    try:                                             # utils/loss_utils.py imports it; none of the three functions uses it
        importlib.import_module("scipy")
    except ImportError:
        sys.modules["scipy"] = types.ModuleType("scipy")
    sys.path.insert(0, ref)
    from utils.image_utils import psnr
    from utils.loss_utils import l1_loss, ssim
    lines = [l for l in open(os.path.join(ref, "train.py")).read().splitlines() if "net_image_bytes = memoryview(" in l]
    assert len(lines) == 1, "anchor `net_image_bytes = memoryview(` not found once in the reference's train.py"
    m = re.search(r"memoryview\((.*)\.cpu\(\)\.numpy\(\)\)\s*$", lines[0])
    assert m and "clamp" in m.group(1) and "255" in m.group(1) and "net_image" in m.group(1)
    return psnr, ssim, l1_loss, compile(m.group(1), "reference_train_net_image_bytes", "eval")


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("EX4D_REFERENCE", "")
    assert ref and os.path.exists(os.path.join(ref, "train.py")), "usage: make_golden_metrics.py <reference checkout>"
    sys.path.insert(0, ROOT)
    from ex4dgs_amd.frames import gt_lut
    psnr, ssim, l1_loss, to_bytes = reference_functions(ref)
    torch.set_num_threads(1)
    u8 = np.load(os.path.join(HERE, "frames.npz"))["rgb_u8"]
    H, W, _ = u8.shape
    rng = np.random.default_rng(77)
    base = gt_lut(1.0).numpy()[u8.astype(np.int64)].transpose(2, 0, 1)
    render = (np.float32(1.4) * np.clip(base + 0.15 * rng.standard_normal(base.shape), 0, 1).astype(np.float32) - np.float32(0.2)).astype(np.float32)
    assert render.min() < 0 and render.max() > 1 and render.shape == (3, H, W)
    out = {"render": render, "im_scales": np.array(SCALES, np.float64)}
    with torch.no_grad():
        x = torch.from_numpy(render)
        for k, im_scale in enumerate(SCALES):
            gt = gt_lut(im_scale)[torch.from_numpy(u8).long()].permute(2, 0, 1).contiguous()
            for tag, image in (("", x), ("_clamped", torch.clamp(x, 0.0, 1.0))):
                out[f"psnr{tag}_{k}"] = np.float32(psnr(image.unsqueeze(0), gt.unsqueeze(0)).mean().item())
                out[f"ssim{tag}_{k}"] = np.float32(ssim(image.unsqueeze(0), gt.unsqueeze(0)).item())
                out[f"l1{tag}_{k}"] = np.float32(l1_loss(image, gt).mean().item())
        b = eval(to_bytes, {"torch": torch, "net_image": x})
        assert b.dtype == torch.uint8 and tuple(b.shape) == (H, W, 3)
        out["bytes_trunc"] = b.numpy()
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
