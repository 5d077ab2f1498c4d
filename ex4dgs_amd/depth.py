"""Supervising the rendered depth: the fused inverse-depth loss with a per-frame scale-and-shift fit (include/ex4d_loss.h, "DEPTH";
ex4dgs_amd/csrc/ex4d_depth.hip).

render(...)["depth"] is the alpha-normalised mean depth, float32 [1,H,W].  The reference's data layer carries the ground truth as a
16-bit inverse-depth map (scene/dataset_readers.py:45 depth_path, utils/general_utils.py:32-36 load_depth).  Monocular inverse depth is
known only up to a scale and a shift, so the loss fits both per frame, on the device, and keeps the fit out of the gradient.

    loss = depth_loss(out["depth"], gt_invdepth, acc=out["acc"])
    loss.backward()                                   # reaches the Gaussians through the rasterizer's grad_out_depth

    g = v * code_scale,  valid = v finite and v > 0,  m = valid and (no acc or acc > 0)
    x = 1 / depth,  r = x - (s g + o),  rho = |r|  ("l1")   or   sqrt(r^2 + eps^2)  ("charbonnier")
    loss = sum m w rho / max(sum m, 1),   w = acc (a constant) or 1
    align="fit": (s, o) the unweighted least-squares fit of s g + o to x over m (float64 sums; s = 0, o = mean x where the ground truth
    is constant or fewer than two pixels count), detached;  align="given": s = scale, o = offset

`gt`: torch.uint16 or torch.int16 (the same bits) codes, or torch.float32 values, [H,W] on the device at render resolution.
`depth_loss_raw` / `depth_loss_backward_raw` are the launches themselves; `depth_metrics` returns the device float64 [6] row (loss, pixels
in the mask, s, o, RMSE of r, mask pixels whose depth is not finite or <= 0) for scoring test views with one read-back per set;
`decode_invdepth` is the decode and the validity in torch ops, CPU or GPU.  The kernels have no CPU fallback.
"""
import torch

from . import _abi, _pixel_loss as _pl
from ._abi import ptr as _ptr
from ._pixel_loss import KINDS, PIXELS_PER_LANE, THREADS, FOLD, kind_code, CODE_DTYPES as _CODE_DTYPES  # noqa: F401 (this module's names too)

ALIGNS = {"given": 0, "fit": 1}               # EX4D_DEPTH_ALIGN_*
GT_U16, GT_F32 = 0, 1                         # EX4D_DEPTH_GT_*
ROW = 6


def align_code(align):
    if align not in ALIGNS:
        raise ValueError(f"unknown align {align!r}: one of {sorted(ALIGNS)}")
    return ALIGNS[align]


def gt_type(gt):
    if gt.dtype in _CODE_DTYPES:
        return GT_U16
    if gt.dtype == torch.float32:
        return GT_F32
    raise RuntimeError("gt must be a torch.uint16 or torch.int16 tensor of codes, or a torch.float32 tensor of values")


def decode_invdepth(gt, code_scale=1.0):
    """(g float32, valid bool), both of gt's shape: the raw value (the code as a float, or the float itself) times float32(code_scale),
    one rounding, and where it is a measurement: finite and > 0."""
    if gt_type(gt) == GT_U16:
        v = (gt.view(torch.int16).to(torch.int32) & 0xFFFF).to(torch.float32)
    else:
        v = gt
    g = v * torch.tensor(float(code_scale), dtype=torch.float32, device=v.device)
    return g, torch.isfinite(v) & (v > 0)


def _check(out_depth, gt, acc):
    _pl.require_device(out_depth, "out_depth", "depth")
    if out_depth.dim() not in (2, 3) or (out_depth.dim() == 3 and out_depth.shape[0] != 1) or out_depth.dtype != torch.float32 \
            or not out_depth.is_contiguous():
        raise RuntimeError("out_depth must be a contiguous float32 [H,W] or [1,H,W] tensor (the rasterizer's depth output)")
    H, W = int(out_depth.shape[-2]), int(out_depth.shape[-1])
    if (gt.dtype not in _CODE_DTYPES and gt.dtype != torch.float32) or gt.dim() != 2 or tuple(gt.shape) != (H, W) \
            or gt.device != out_depth.device or not gt.is_contiguous():
        raise RuntimeError("gt must be a contiguous torch.uint16, torch.int16 or torch.float32 [H,W] tensor on out_depth's device")
    _pl.check_acc(acc, H, W, out_depth.device, "out_depth")
    return H, W


def new_scratch(H, W, device):
    return torch.empty(_abi.load().ex4d_depth_loss_scratch_bytes(H, W), dtype=torch.uint8, device=device)


def depth_loss_raw(out_depth, gt, code_scale=1.0, align="fit", scale=1.0, offset=0.0, kind="l1", eps=1e-3, acc=None, loss=None, row=None,
                   scratch=None):
    """The forward's launches on the current stream (four for "fit", two for "given").  Returns (loss float32 [1], row float64 [6]) on
    the device; `loss`, `row` and `scratch` (new_scratch(H, W, device)) are allocated when absent and fully written either way.  No
    autograd."""
    code, how = kind_code(kind), align_code(align)
    H, W = _check(out_depth, gt, acc)
    dev = out_depth.device
    need = _abi.load().ex4d_depth_loss_scratch_bytes(H, W)
    loss, row, scratch = _pl.forward_outputs(loss, row, scratch, ROW, need, torch.uint8, "bytes", dev, "out_depth")
    with _abi.stream(dev) as stream:
        _abi.call("ex4d_depth_loss_forward", H, W, out_depth.data_ptr(), gt.data_ptr(), gt_type(gt), float(code_scale), _ptr(acc), how,
                  float(scale), float(offset), code, float(eps), loss.data_ptr(), row.data_ptr(), scratch.data_ptr(), stream)
    return loss, row


def depth_loss_backward_raw(out_depth, gt, row, grad_loss, code_scale=1.0, align="fit", kind="l1", eps=1e-3, acc=None, out=None):
    """The backward's launch on the current stream: `row` is the forward's row of the same inputs (its count, s and o are read on the
    device: the fit is a constant), `grad_loss` a device float32 [1].  Returns grad_depth of out_depth's shape (`out`, or a new tensor:
    every element is written)."""
    code, how = kind_code(kind), align_code(align)
    H, W = _check(out_depth, gt, acc)
    dev = out_depth.device
    _pl.check_row(row, ROW, dev, "out_depth")
    _pl.check_grad_loss(grad_loss, dev, "out_depth")
    out = _pl.gradient_output(out, out_depth, lambda o: o.numel() == H * W, "[H,W] or [1,H,W]", "out_depth")
    with _abi.stream(dev) as stream:
        _abi.call("ex4d_depth_loss_backward", H, W, out_depth.data_ptr(), gt.data_ptr(), gt_type(gt), float(code_scale), _ptr(acc), how,
                  code, float(eps), row.data_ptr(), grad_loss.data_ptr(), out.data_ptr(), stream)
    return out


class _DepthLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out_depth, gt, code_scale, align, scale, offset, kind, eps, acc):
        depth = out_depth.contiguous()
        acc = None if acc is None else acc.detach().contiguous()
        loss, row = depth_loss_raw(depth, gt, code_scale, align, scale, offset, kind, eps, acc)
        ctx.call = (gt, float(code_scale), align, kind, float(eps), acc)
        ctx.save_for_backward(depth, row)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g_loss):
        depth, row = ctx.saved_tensors
        gt, code_scale, align, kind, eps, acc = ctx.call
        g = g_loss.reshape(1).to(torch.float32).contiguous()
        return (depth_loss_backward_raw(depth, gt, row, g, code_scale, align, kind, eps, acc),) + (None,) * 8


def depth_loss(out_depth, gt, code_scale=1.0, align="fit", scale=1.0, offset=0.0, kind="l1", eps=1e-3, acc=None):
    """The scalar loss of the module docstring for a rendered [H,W] or [1,H,W] depth and its inverse-depth ground truth; differentiable
    in `out_depth` only (`acc`, the rasterizer's [1,H,W] or [H,W] accumulated alpha, masks and weighs the pixels as a constant; the
    fit of align="fit" is detached)."""
    kind_code(kind)
    align_code(align)
    _pl.require_device(out_depth, "out_depth", "depth")
    return _DepthLoss.apply(out_depth, gt, code_scale, align, scale, offset, kind, eps, acc)


def depth_metrics(out_depth, gt, code_scale=1.0, align="fit", scale=1.0, offset=0.0, row=None, scratch=None):
    """Scores one view: enqueues the forward on the current stream and returns the device float64 [6] row (`row`, or a new one): the
    unweighted L1 loss, the number of pixels with a measurement, s and o as used, the RMSE of the residual over them, the number of them
    whose rendered depth is not finite or <= 0.  Rows of a set of views can live in one [n,6] table and be read back once."""
    return depth_loss_raw(out_depth.detach().contiguous(), gt, code_scale, align, scale, offset, "l1", 0.0, None, row=row, scratch=scratch)[1]
