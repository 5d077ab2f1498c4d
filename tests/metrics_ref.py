"""The reference of the view-scoring call (include/ex4d_loss.h: ex4d_frame_metrics; ex4dgs_amd/evaluate.py), shared by
tests/test_cpu_metrics.py and tests/test_gpu_metrics.py: float64 on the CPU, its shapes, inputs and bars.

  L1, SSIM map   oracle.loss_oracle.l1_ssim (utils/loss_utils.py:22-25, :47-81)
  MSE, PSNR      restated from utils/image_utils.py:14-19: mse = mean((a - b)^2), psnr = 20 log10(1 / sqrt(mse))
  clamp          train.py:342: torch.clamp(render, 0.0, 1.0)
  bytes          train.py:101: (torch.clamp(image, min=0, max=1.0) * 255).byte(), and torchvision's save_image (render.py:75) --
                 torchvision is not installed, so its line is RESTATED here: image.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)
A reference is computed once per (shape, ground truth, clamp) and shared (lru_cache); callers do not modify what they get."""
import functools
import math

import numpy as np
import torch

from oracle import loss_oracle
from tests import loss_cases

# ---- shapes: the smallest image, a window larger than the image, exactly one segment x one strip, one row / column more, the golden
# image's odd H W, several iterations of the ring; the three shapes of loss_cases whose 17 / 17 / 9 work items exercise the XCD map
# with and without padded workgroups; and, from loss_cases.HEIGHTS, one height per value of (rows_out + 10) % 4 in the last segment
FIXED = ((1, 1), (7, 5), (48, 64), (49, 65), (53, 139), (97, 129))
WORK_ITEM = tuple((H, W) for (C, H, W) in loss_cases.WORK_ITEM_SHAPES if (C, H, W) in ((3, 20, 1030), (3, 769, 10), (3, 100, 190)))
REMAINDER_WIDTH = 69             # a second strip narrower than the halo (loss_cases.WIDTHS)


def _last_rows_out(H):
    return H - loss_cases.SEG * ((H - 1) // loss_cases.SEG)


def _remainder_shapes():
    out = {}
    for H in loss_cases.HEIGHTS:
        if H > loss_cases.SEG:
            out.setdefault((_last_rows_out(H) + 10) % 4, (H, REMAINDER_WIDTH))
    assert sorted(out) == [0, 1, 2, 3] and REMAINDER_WIDTH in loss_cases.WIDTHS
    return tuple(out[r] for r in range(4))


REMAINDER = _remainder_shapes()
SHAPES = FIXED + WORK_ITEM + REMAINDER
assert len(WORK_ITEM) == 3 and len(set(SHAPES)) == len(SHAPES)

TOL = loss_cases.TOL_LOSS        # rows 0, 1, 3: the project's bar for these means, absolute


def psnr_bar(mse_ref, psnr_ref):
    """The MSE bar carried through the logarithm (d psnr / d mse = -(10 / ln 10) / mse) plus a few float32 ulps of the value."""
    return (10.0 / math.log(10.0)) * TOL / mse_ref + 4.0 * 2.0 ** -23 * abs(psnr_ref)


# ---- inputs
def make_pair(H, W):
    """loss_cases.make_pair with the image stretched to [-0.2, 1.2], so that the clamp decides something."""
    image, gt = loss_cases.make_pair((3, H, W))
    image = (np.float32(1.4) * image - np.float32(0.2)).astype(np.float32)
    image[0, 0, 0] = gt[0, 0, 0]
    return image, gt


def make_bytes(H, W, stride=3):
    """The float ground truth of make_pair as decoded bytes [H,W,stride] (a fourth byte is noise that is never read)."""
    _, gt = make_pair(H, W)
    u8 = np.ascontiguousarray(np.rint(gt * 255.0).astype(np.uint8).transpose(1, 2, 0))
    if stride == 4:
        noise = np.random.default_rng(H * 1000 + W).integers(0, 256, size=(H, W, 1), dtype=np.uint8)
        u8 = np.ascontiguousarray(np.concatenate([u8, noise], axis=2))
    return u8


def looked_up(u8, lut):
    """float32 [3,H,W]: what the table makes of decoded bytes (lut: CPU float32 [256] tensor)."""
    return lut.numpy()[u8[..., :3].astype(np.int64)].transpose(2, 0, 1).copy()


# ---- the reference
def clamp01(image):
    return torch.clamp(torch.from_numpy(np.asarray(image)), 0.0, 1.0).numpy()                      # train.py:342


def metrics(image, gt, clamp=False, dtype=torch.float64):
    """dict(l1, mse, psnr, ssim, nonfinite) of float32 numpy [3,H,W] inputs, evaluated in `dtype`."""
    image = clamp01(image) if clamp else np.asarray(image)
    with torch.enable_grad():                        # (the oracle differentiates; callers may sit under no_grad)
        r = loss_oracle.l1_ssim(image, gt, 0.0, dtype=dtype)
    x, y = torch.tensor(image, dtype=dtype), torch.tensor(np.asarray(gt), dtype=dtype)
    mse = ((x - y) ** 2).reshape(1, -1).mean(1, keepdim=True)                                      # image_utils.py:14-15
    psnr = 20 * torch.log10(1.0 / torch.sqrt(mse))                                                 # :17-19
    return dict(l1=float(torch.abs(x - y).mean()), mse=float(mse), psnr=float(psnr), ssim=float(torch.from_numpy(r["ssim_map"]).mean()),
                nonfinite=int((~np.isfinite(image)).sum()))


def quant_trunc(image):
    """train.py:101, as [H,W,3] uint8."""
    return (torch.clamp(torch.from_numpy(np.asarray(image)), min=0, max=1.0) * 255).byte().permute(1, 2, 0).contiguous().numpy()


def quant_round(image):
    """torchvision.utils.save_image's conversion (restated, see the module docstring), as [H,W,3] uint8."""
    return torch.from_numpy(np.asarray(image)).clone().mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous().numpy()


def within_bars(row, ref, what=""):
    """row: the eight values of a result row; ref: metrics(...) in float64.  Prints each figure, then asserts."""
    e = dict(l1=abs(row[0] - ref["l1"]), mse=abs(row[1] - ref["mse"]), psnr=abs(row[2] - ref["psnr"]), ssim=abs(row[3] - ref["ssim"]))
    bar = psnr_bar(ref["mse"], ref["psnr"])
    print(what, {k: f"{v:.3g}" for k, v in e.items()}, f"psnr bar {bar:.3g}")
    assert e["l1"] <= TOL and e["mse"] <= TOL and e["ssim"] <= TOL, (what, e)
    assert e["psnr"] <= bar, (what, e, bar)
    assert row[4] == ref["nonfinite"] and tuple(row[5:8]) == (0.0, 0.0, 0.0), (what, list(row))


@functools.lru_cache(maxsize=None)
def case(H, W, gt_kind, clamp):
    """The float64 reference of shape (H, W); gt_kind: "float", "u8" (default table) or "u8_1.7" (frames.gt_lut(1.7))."""
    from ex4dgs_amd.frames import gt_lut
    image, gt = make_pair(H, W)
    if gt_kind != "float":
        gt = looked_up(make_bytes(H, W), gt_lut(1.7) if gt_kind == "u8_1.7" else gt_lut())
    return metrics(image, gt, clamp)
