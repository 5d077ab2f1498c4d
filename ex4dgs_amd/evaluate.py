"""Scoring rendered views on the GPU: the reference's render.py:64-123 (render_set) and train.py:313-362 (training_report).

One fused HIP pass per view (include/ex4d_loss.h: ex4d_frame_metrics / _u8) gives L1, MSE, PSNR and SSIM of a float32 [3,H,W] render
against its ground truth -- float32 [3,H,W], or the decoded frame as uint8 [H,W,3|4] (ex4dgs_amd.frames) through `lut=` -- and,
optionally, the render as 8-bit pixels [H,W,3].  The results land in one row of a device table, so a whole set is read back once.

    row = frame_metrics(image, gt)                          # device float64 [8]: L1, MSE, PSNR, SSIM, non-finite count, 0, 0, 0
    ev = Evaluator(n_views, H, W, keep_frames=True)
    ev.score(i, image, store.get(i), name="0007.png", lut=lut)      # enqueues; reads nothing back
    mean, per_view = ev.report()                            # the one read-back; dicts with the keys SSIM, PSNR, L1
    evaluate_set(model, cameras, store, lut=lut, background=bg, near=near, far=far, out_dir=model_path, save_img=True)
    sk = frame_skssim(image, gt)                            # device float64 [4]: SKSSIM, SKSSIM2, non-finite positions, 0
    evaluate_set(..., skssim=True)                          # the report gains the keys SKSSIM and SKSSIM2

`clamp=True` scores clamp(image, 0, 1) as train.py:342 does; render.py:76-77 scores the render as it is.  8-bit pixels:
quant="round" is torchvision's save_image (render.py:75: mul(255).add_(0.5).clamp_(0, 255).to(uint8)), quant="trunc" is
train.py:101 ((clamp(image, 0, 1) * 255).byte()).  A NaN pixel becomes 0 (torch leaves that conversion unspecified).

SKSSIM and SKSSIM2 (render.py:78-79: scikit-image's structural_similarity at data_range 1 and 2, the D-SSIM of the dynamic-scene
papers) are a 7x7 box-window SSIM over the positions whose window lies inside the image: one more fused pass
(ex4d_frame_skssim / _u8) gives both, in a row of its own, as scikit-image 0.22 and later read the reference's call.  They are an
option, off by default: `Evaluator(..., skssim=True)`, `evaluate_set(..., skssim=True)`; without it the keys, the tables and the
launches are what they were.

OUT OF SCOPE: the LPIPS and LPIPSVGG entries of render.py:80-81 (pretrained networks, which this project does not have) and "times"
(that is `bench.py --forward-only`).  Those keys are ABSENT from what is returned and written, not zero.  No CPU fallback.
"""
import json
import os

import numpy as np
import torch

from . import _abi
from .loss import _WINDOW

METRICS_CLAMP = 1            # EX4D_METRICS_CLAMP
METRICS_QUANT_TRUNC = 2      # EX4D_METRICS_QUANT_TRUNC
ROW = 8                      # doubles per result row
L1, MSE, PSNR, SSIM, NONFINITE = range(5)
_QUANT = {"round": 0, "trunc": METRICS_QUANT_TRUNC}
SK_ROW = 4                   # doubles per result row of frame_skssim
SKSSIM, SKSSIM2, SK_NONFINITE = range(3)
SK_WINDOW = 7                # EX4D_SKSSIM_WINDOW


def metrics_flags(clamp=False, quant="round"):
    if quant not in _QUANT:
        raise RuntimeError(f"quant is 'round' (save_image) or 'trunc' (train.py:101), not {quant!r}")
    return (METRICS_CLAMP if clamp else 0) | _QUANT[quant]


def _check_pair(image, gt, lut, what):
    """The refusals frame_metrics and frame_skssim share; returns (H, W, device)."""
    if not isinstance(image, torch.Tensor) or not image.is_cuda:
        raise RuntimeError(f"image is not on a ROCm GPU: {what} has no CPU fallback")
    if image.dim() != 3 or image.shape[0] != 3 or image.dtype != torch.float32:
        raise RuntimeError("image must be a float32 [3,H,W] tensor (render.py scores RGB)")
    _, H, W = image.shape
    dev = image.device
    if not isinstance(gt, torch.Tensor) or gt.device != dev:
        raise RuntimeError("gt must be a tensor on the image's ROCm device")
    if gt.dtype == torch.uint8:
        if gt.dim() != 3 or gt.shape[2] not in (3, 4) or tuple(gt.shape[:2]) != (H, W):
            raise RuntimeError("uint8 gt must be [H,W,3] or [H,W,4] for a [3,H,W] image")
        if lut is not None and (not isinstance(lut, torch.Tensor) or lut.device.type != "cpu" or lut.dtype != torch.float32 or tuple(lut.shape) != (256,)):
            raise RuntimeError("lut must be a CPU float32 [256] tensor (frames.gt_lut)")
    elif gt.dtype == torch.float32:
        if lut is not None:
            raise RuntimeError("lut= belongs to uint8 ground truth; a float gt already holds its values")
        if gt.shape != image.shape:
            raise RuntimeError("float gt must be float32 [3,H,W], the image's shape")
    else:
        raise RuntimeError(f"gt must be float32 [3,H,W] or uint8 [H,W,3|4], not {gt.dtype}")
    return H, W, dev


def frame_metrics(image, gt, *, lut=None, clamp=False, quant="round", out_u8=None, row=None, scratch=None):
    """Scores one view: enqueues the two kernels on the current stream and returns the device float64 [8] row (`row`, or a new one).
    gt: float32 [3,H,W], or uint8 [H,W,3|4] with `lut` (CPU float32 [256], default frames.gt_lut(): u / 255) giving the bytes their
    values.  out_u8: a uint8 tensor of H*W*3 contiguous elements (any storage offset) that receives the image as [H,W,3] pixels.
    `scratch`: float32, at least ex4d_frame_metrics_scratch_floats(H, W) elements (allocated when absent)."""
    lib = _abi.load()
    flags = metrics_flags(clamp, quant)
    H, W, dev = _check_pair(image, gt, lut, "frame_metrics")
    if out_u8 is not None and (not isinstance(out_u8, torch.Tensor) or out_u8.dtype != torch.uint8 or out_u8.device != dev
                               or out_u8.numel() != H * W * 3 or not out_u8.is_contiguous()):
        raise RuntimeError("out_u8 must be a contiguous uint8 tensor of H*W*3 elements on the image's device")
    if row is None:
        row = torch.empty(ROW, dtype=torch.float64, device=dev)
    elif not isinstance(row, torch.Tensor) or row.dtype != torch.float64 or row.device != dev or row.numel() != ROW or not row.is_contiguous():
        raise RuntimeError("row must be a contiguous float64 [8] tensor on the image's device")
    need = lib.ex4d_frame_metrics_scratch_floats(H, W)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.float32, device=dev)
    elif not isinstance(scratch, torch.Tensor) or scratch.dtype != torch.float32 or scratch.device != dev or scratch.numel() < need or not scratch.is_contiguous():
        raise RuntimeError(f"scratch must be a contiguous float32 tensor of at least {need} elements on the image's device")
    image, gt = image.contiguous(), gt.contiguous()
    with _abi.stream(dev) as stream:
        if gt.dtype == torch.uint8:
            lut = None if lut is None else lut.contiguous()
            _abi.call("ex4d_frame_metrics_u8", H, W, image.data_ptr(), gt.data_ptr(), gt.shape[2], _abi.ptr(lut), _WINDOW.ctypes.data, flags,
                      _abi.ptr(out_u8), row.data_ptr(), scratch.data_ptr(), stream)
        else:
            _abi.call("ex4d_frame_metrics", H, W, image.data_ptr(), gt.data_ptr(), _WINDOW.ctypes.data, flags, _abi.ptr(out_u8),
                      row.data_ptr(), scratch.data_ptr(), stream)
    return row


def frame_skssim(image, gt, *, lut=None, clamp=False, row=None, scratch=None):
    """scikit-image's SSIM of one view at data_range 1 and 2 (render.py:78-79): enqueues the two kernels on the current stream and
    returns the device float64 [4] row (`row`, or a new one): SKSSIM, SKSSIM2, the number of scored positions whose value is not
    finite, 0.  image, gt, lut and clamp as in frame_metrics; H, W >= 7 (a 7x7 window).  `scratch`: float32, at least
    ex4d_frame_skssim_scratch_floats(H, W) elements (allocated when absent)."""
    lib = _abi.load()
    H, W, dev = _check_pair(image, gt, lut, "frame_skssim")
    if H < SK_WINDOW or W < SK_WINDOW:
        raise RuntimeError(f"image is {H} x {W}: win_size exceeds image extent (H, W >= {SK_WINDOW})")
    if row is None:
        row = torch.empty(SK_ROW, dtype=torch.float64, device=dev)
    elif not isinstance(row, torch.Tensor) or row.dtype != torch.float64 or row.device != dev or row.numel() != SK_ROW or not row.is_contiguous():
        raise RuntimeError("row must be a contiguous float64 [4] tensor on the image's device")
    need = lib.ex4d_frame_skssim_scratch_floats(H, W)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.float32, device=dev)
    elif not isinstance(scratch, torch.Tensor) or scratch.dtype != torch.float32 or scratch.device != dev or scratch.numel() < need or not scratch.is_contiguous():
        raise RuntimeError(f"scratch must be a contiguous float32 tensor of at least {need} elements on the image's device")
    image, gt = image.contiguous(), gt.contiguous()
    flags = METRICS_CLAMP if clamp else 0
    with _abi.stream(dev) as stream:
        if gt.dtype == torch.uint8:
            lut = None if lut is None else lut.contiguous()
            _abi.call("ex4d_frame_skssim_u8", H, W, image.data_ptr(), gt.data_ptr(), gt.shape[2], _abi.ptr(lut), flags, row.data_ptr(),
                      scratch.data_ptr(), stream)
        else:
            _abi.call("ex4d_frame_skssim", H, W, image.data_ptr(), gt.data_ptr(), flags, row.data_ptr(), scratch.data_ptr(), stream)
    return row


def aggregate(rows, names, sk_rows=None):
    """(mean, per_view) of render.py:98-118 from the [N,8] result rows and the views' names -- a pure host function.  The reference
    collects float32 scalars in lists and forms `torch.tensor(list).mean().item()` / `torch.tensor(list).tolist()`: a float32 tensor,
    its float32 mean, widened to Python floats.  L1 is train.py:347's quantity under the same arithmetic.  sk_rows: the [N,4] rows of
    frame_skssim; the results gain the keys SKSSIM and SKSSIM2 (render.py:100-101, :113-114) under the same arithmetic."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, ROW)
    names = list(names)
    if len(names) != rows.shape[0]:
        raise RuntimeError(f"{rows.shape[0]} rows, {len(names)} names")
    cols = {"SSIM": rows[:, SSIM], "PSNR": rows[:, PSNR], "L1": rows[:, L1]}
    if sk_rows is not None:
        sk_rows = np.asarray(sk_rows, dtype=np.float64).reshape(-1, SK_ROW)
        if sk_rows.shape[0] != rows.shape[0]:
            raise RuntimeError(f"{rows.shape[0]} rows, {sk_rows.shape[0]} sk_rows")
        cols.update(SKSSIM=sk_rows[:, SKSSIM], SKSSIM2=sk_rows[:, SKSSIM2])
    lists = {k: torch.tensor([float(np.float32(v)) for v in col], dtype=torch.float32) for k, col in cols.items()}
    mean = {k: t.mean().item() for k, t in lists.items()}
    per_view = {k: {name: v for v, name in zip(t.tolist(), names)} for k, t in lists.items()}
    return mean, per_view


class Evaluator:
    """Scores a set of n_views views of H x W: one float64 [N,8] table, one scratch buffer and, with keep_frames, one uint8 [N,H,W,3]
    tensor of the 8-bit renders -- allocated here, nothing per view.  Rows that were never scored hold NaN.  With skssim it also owns
    a float64 [N,4] table and a second scratch buffer for frame_skssim, and `score` enqueues both calls (H, W >= 7)."""

    def __init__(self, n_views, H, W, keep_frames=False, device="cuda", skssim=False):
        if n_views <= 0 or H <= 0 or W <= 0:
            raise RuntimeError("Evaluator: n_views, H, W > 0")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("Evaluator lives on a ROCm device (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev
        self.n_views, self.H, self.W = int(n_views), int(H), int(W)
        self.table = torch.full((self.n_views, ROW), float("nan"), dtype=torch.float64, device=self.device)
        self.scratch = torch.empty(_abi.load().ex4d_frame_metrics_scratch_floats(self.H, self.W), dtype=torch.float32, device=self.device)
        self.frames = torch.zeros((self.n_views, self.H, self.W, 3), dtype=torch.uint8, device=self.device) if keep_frames else None
        self.names = [None] * self.n_views
        self.quant = "round"
        self.table_sk = self.scratch_sk = None
        if skssim:
            if self.H < SK_WINDOW or self.W < SK_WINDOW:
                raise RuntimeError(f"Evaluator(skssim=True): H, W >= {SK_WINDOW}")
            self.table_sk = torch.full((self.n_views, SK_ROW), float("nan"), dtype=torch.float64, device=self.device)
            self.scratch_sk = torch.empty(_abi.load().ex4d_frame_skssim_scratch_floats(self.H, self.W), dtype=torch.float32, device=self.device)

    def score(self, i, image, gt, name=None, lut=None, clamp=False):
        """Enqueues the scoring of view i on the current stream (all calls of one Evaluator share its scratch: one stream).  Reads
        nothing back."""
        if not 0 <= i < self.n_views:
            raise RuntimeError(f"view {i} of {self.n_views}")
        if tuple(image.shape[1:]) != (self.H, self.W):
            raise RuntimeError(f"image is {list(image.shape)}, the Evaluator was made for [3,{self.H},{self.W}]")
        frame_metrics(image, gt, lut=lut, clamp=clamp, quant=self.quant, out_u8=None if self.frames is None else self.frames[i],
                      row=self.table[i], scratch=self.scratch)
        if self.table_sk is not None:
            frame_skssim(image, gt, lut=lut, clamp=clamp, row=self.table_sk[i], scratch=self.scratch_sk)
        self.names[i] = str(i) if name is None else name

    def frame(self, i):
        """The 8-bit [H,W,3] render of view i (a view of the stored tensor; keep_frames=True)."""
        if self.frames is None:
            raise RuntimeError("Evaluator(keep_frames=True) stores the 8-bit frames")
        return self.frames[i]

    def rows(self):
        """The one read-back: the [N,8] table as a CPU float64 tensor (synchronises with the current stream)."""
        return self.table.cpu()

    def rows_sk(self):
        """The [N,4] table of frame_skssim as a CPU float64 tensor (skssim=True)."""
        if self.table_sk is None:
            raise RuntimeError("Evaluator(skssim=True) scores SKSSIM and SKSSIM2")
        return self.table_sk.cpu()

    def report(self):
        """(mean, per_view) of the views scored so far, in view order; with skssim both tables come back in one transfer."""
        done = [i for i, n in enumerate(self.names) if n is not None]
        names = [self.names[i] for i in done]
        if self.table_sk is None:
            return aggregate(self.rows()[done].numpy(), names)
        both = torch.cat([self.table, self.table_sk], dim=1).cpu()
        return aggregate(both[done, :ROW].numpy(), names, both[done, ROW:].numpy())


def write_report(out_dir, mean, per_view):
    """mean_metrics.json and all_metrics.json as render.py:108-121 writes them (indent=True)."""
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "mean_metrics.json"), "w") as fp:
        json.dump(mean, fp, indent=True)
    with open(os.path.join(out_dir, "all_metrics.json"), "w") as fp:
        json.dump(per_view, fp, indent=True)


def evaluate_set(model, cameras, frames, *, lut=None, pipe=None, background, near, far, interval=1, clamp=False, out_dir=None,
                 save_img=False, skssim=False):
    """render_set of render.py:64-123: renders every `interval`-th camera, scores it against frames.get(i) (a frames.FrameStore) or
    frames[i] (a list of tensors), reads the table back once and returns (mean, per_view, evaluator).  A camera's name is its
    `image_name` (scene/cameras.py), or its index as %05d.png.  out_dir: the two JSON files; save_img: out_dir/renders/<image_name>
    through PIL from the 8-bit frames (needs out_dir).  skssim: also SKSSIM and SKSSIM2 (render.py:78-79), from the same read-back."""
    from .render import render
    if save_img and out_dir is None:
        raise RuntimeError("save_img needs out_dir")
    picked = [i for i in range(len(cameras)) if i % interval == 0]
    if not picked:
        raise RuntimeError("no camera to score")
    H, W = int(cameras[picked[0]].image_height), int(cameras[picked[0]].image_width)
    ev = Evaluator(len(picked), H, W, keep_frames=save_img, device=background.device, skssim=skssim)
    with torch.no_grad():
        for k, i in enumerate(picked):
            cam = cameras[i]
            gt = frames.get(i) if hasattr(frames, "get") else frames[i]
            image = render(cam, model, pipe, background, near=near, far=far, sync=False)["render"]
            ev.score(k, image, gt, name=getattr(cam, "image_name", None) or f"{i:05d}.png", lut=lut, clamp=clamp)
        mean, per_view = ev.report()
    if out_dir is not None:
        write_report(out_dir, mean, per_view)
    if save_img:
        from PIL import Image
        os.makedirs(os.path.join(out_dir, "renders"), exist_ok=True)
        host = ev.frames.cpu().numpy()
        for k, name in enumerate(ev.names):
            Image.fromarray(host[k], "RGB").save(os.path.join(out_dir, "renders", name))
    return mean, per_view, ev
