"""Supervising the rendered motion: the fused flow loss on 16-bit encoded ground truth (include/ex4d_loss.h, "FLOW";
ex4dgs_amd/csrc/ex4d_flow.hip).

render(..., flow_to=t1)["opticalflow"] is the rendered motion in pixels, float32 [3,H,W] (u, v, depth change).  The reference's data
layer carries the ground truth as a 16-bit three-channel image (utils/general_utils.py:39-53 read_opticalflow / decode_flow,
scene/cameras.py:85,102 opticalflow_path): u and v offset by 2^15 and scaled by 2^8, the third word above 2^15 where the pixel is
valid.  The kernels decode those words on load; the float flow image and its mask are never formed.

    loss = flow_loss(out["opticalflow"], encoded, flow_scale, kind="charbonnier", eps=1e-3, acc=out["acc"])
    loss.backward()                                   # reaches _xyz, _xyz_disp and _xyz_motion through the render

    g = (float)(code - 32768) / 256 * flow_scale,  m = code2 > 32768,  r = (flow_u - g_u, flow_v - g_v)
    rho = |r_u| + |r_v|  ("l1")   or   sqrt(r_u^2 + r_v^2 + eps^2)  ("charbonnier")
    loss = sum m w rho / max(sum m, 1),   w = acc (a constant) or 1

`encoded`: torch.uint16 or torch.int16 (the same bits) [H,W,3|4] on the device, at render resolution; `flow_scale` carries
read_opticalflow's resolution[1] / rows.  `flow_loss_raw` / `flow_loss_backward_raw` are the launches themselves; `flow_metrics`
returns the device float64 [4] row (loss, valid pixels, mean end-point error, non-finite valid pixels) for scoring test views with one
read-back per set; `decode_flow` is the reference's decode in torch ops, CPU or GPU.  The kernels have no CPU fallback.
"""
import torch

from . import _abi, _pixel_loss as _pl
from ._abi import ptr as _ptr
from ._pixel_loss import KINDS, PIXELS_PER_LANE, THREADS, FOLD, kind_code, CODE_DTYPES as _CODE_DTYPES  # noqa: F401 (this module's names too)

ROW = 4


def _words(encoded):
    """The codes as int32 in 0..65535, for either dtype."""
    if encoded.dtype not in _CODE_DTYPES:
        raise RuntimeError("encoded flow must be a torch.uint16 or torch.int16 tensor [H,W,3|4]")
    if encoded.dim() != 3 or encoded.shape[2] not in (3, 4):
        raise RuntimeError("encoded flow must be [H,W,3] or [H,W,4]")
    return encoded.view(torch.int16).to(torch.int32) & 0xFFFF


def decode_flow(encoded, flow_scale=1.0):
    """(flow float32 [H,W,2], mask float32 [H,W]) of decode_flow (utils/general_utils.py:49-53) times read_opticalflow's flow_scale
    (:45), with the reference's bits: the subtraction and the division are exact in float32, the product rounds once."""
    words = _words(encoded)
    flow = (words[..., :2] - 32768).to(torch.float32) / 256.0
    flow = flow * torch.tensor(float(flow_scale), dtype=torch.float32, device=flow.device)
    return flow, (words[..., 2] > 32768).to(torch.float32)


def _check(out_flow, encoded, acc):
    _pl.require_device(out_flow, "out_flow", "flow")
    if out_flow.dim() != 3 or out_flow.shape[0] != 3 or out_flow.dtype != torch.float32 or not out_flow.is_contiguous():
        raise RuntimeError("out_flow must be a contiguous float32 [3,H,W] tensor (the rasterizer's opticalflow output)")
    H, W = int(out_flow.shape[1]), int(out_flow.shape[2])
    if encoded.dtype not in _CODE_DTYPES or encoded.dim() != 3 or encoded.shape[2] not in (3, 4) or tuple(encoded.shape[:2]) != (H, W) \
            or encoded.device != out_flow.device or not encoded.is_contiguous():
        raise RuntimeError("encoded flow must be a contiguous torch.uint16 or torch.int16 [H,W,3|4] tensor on out_flow's device")
    _pl.check_acc(acc, H, W, out_flow.device, "out_flow")
    return H, W


def new_scratch(H, W, device):
    return torch.empty(_abi.load().ex4d_flow_loss_scratch_floats(H, W), dtype=torch.float32, device=device)


def flow_loss_raw(out_flow, encoded, flow_scale=1.0, kind="charbonnier", eps=1e-3, acc=None, loss=None, row=None, scratch=None):
    """The forward's two launches on the current stream.  Returns (loss float32 [1], row float64 [4]) on the device; `loss`, `row` and
    `scratch` (new_scratch(H, W, device)) are allocated when absent and fully written either way.  No autograd."""
    code = kind_code(kind)
    H, W = _check(out_flow, encoded, acc)
    dev = out_flow.device
    need = _abi.load().ex4d_flow_loss_scratch_floats(H, W)
    loss, row, scratch = _pl.forward_outputs(loss, row, scratch, ROW, need, torch.float32, "elements", dev, "out_flow")
    with _abi.stream(dev) as stream:
        _abi.call("ex4d_flow_loss_forward", H, W, out_flow.data_ptr(), encoded.data_ptr(), int(encoded.shape[2]), float(flow_scale),
                  _ptr(acc), code, float(eps), loss.data_ptr(), row.data_ptr(), scratch.data_ptr(), stream)
    return loss, row


def flow_loss_backward_raw(out_flow, encoded, row, grad_loss, flow_scale=1.0, kind="charbonnier", eps=1e-3, acc=None, out=None):
    """The backward's launch on the current stream: `row` is the forward's row of the same inputs, `grad_loss` a device float32 [1].
    Returns grad_flow [3,H,W] (`out`, or a new tensor: every element is written)."""
    code = kind_code(kind)
    H, W = _check(out_flow, encoded, acc)
    dev = out_flow.device
    _pl.check_row(row, ROW, dev, "out_flow")
    _pl.check_grad_loss(grad_loss, dev, "out_flow")
    out = _pl.gradient_output(out, out_flow, lambda o: tuple(o.shape) == (3, H, W), "[3,H,W]", "out_flow")
    with _abi.stream(dev) as stream:
        _abi.call("ex4d_flow_loss_backward", H, W, out_flow.data_ptr(), encoded.data_ptr(), int(encoded.shape[2]), float(flow_scale),
                  _ptr(acc), code, float(eps), row.data_ptr(), grad_loss.data_ptr(), out.data_ptr(), stream)
    return out


class _FlowLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out_flow, encoded, flow_scale, kind, eps, acc):
        flow = out_flow.contiguous()
        acc = None if acc is None else acc.detach().contiguous()
        loss, row = flow_loss_raw(flow, encoded, flow_scale, kind, eps, acc)
        ctx.call = (encoded, float(flow_scale), kind, float(eps), acc)
        ctx.save_for_backward(flow, row)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g_loss):
        flow, row = ctx.saved_tensors
        encoded, flow_scale, kind, eps, acc = ctx.call
        g = g_loss.reshape(1).to(torch.float32).contiguous()
        return flow_loss_backward_raw(flow, encoded, row, g, flow_scale, kind, eps, acc), None, None, None, None, None


def flow_loss(out_flow, encoded, flow_scale=1.0, kind="charbonnier", eps=1e-3, acc=None):
    """The scalar loss of the module docstring for a rendered [3,H,W] flow and its encoded ground truth; differentiable in `out_flow`
    only (`acc`, the rasterizer's [1,H,W] or [H,W] accumulated alpha, weighs the pixels as a constant)."""
    kind_code(kind)
    _pl.require_device(out_flow, "out_flow", "flow")
    return _FlowLoss.apply(out_flow, encoded, flow_scale, kind, eps, acc)


def flow_metrics(out_flow, encoded, flow_scale=1.0, row=None, scratch=None):
    """Scores one view: enqueues the forward on the current stream and returns the device float64 [4] row (`row`, or a new one):
    the unweighted L1 loss, the number of valid pixels, the mean end-point error over them, the number of them whose rendered flow is
    not finite.  Rows of a set of views can live in one [n,4] table and be read back once."""
    return flow_loss_raw(out_flow.detach().contiguous(), encoded, flow_scale, "l1", 0.0, None, row=row, scratch=scratch)[1]
