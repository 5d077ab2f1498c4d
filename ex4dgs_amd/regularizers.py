"""The motion regularisers of the reference's training loop (train.py:155-168) on the HIP library (include/ex4d_regularizers.h):

    w = regularizer_weights(opt, iteration, gaussians._xyz_motion.shape[0])
    loss += motion_regularizers(gaussians._xyz_disp, gaussians._xyz_motion, gaussians._rotation_motion, *w)

replaces the three `if opt.*_reg > 0 ...` blocks: one forward launch pair and one backward launch per tensor instead of ~20
element-wise torch kernels and their autograd graph over the keyframe tensors.  Works with torch.optim.RAdam and FusedRAdam.
trainer.FrameTrainer(regularizers=...) goes further: with sliced keyframe gradients the two keyframe terms are formed inside the
optimizer step (optim.radam_step_sliced_reg_raw) and their dense gradient never exists.  On several ranks the term is added once per
optimizer step, last, to the gradient summed over ranks and views; backward_range_raw is the gradient of one term
over the element range a rank of the sharded optimizer owns.
No CPU fallback: everything here needs the HIP library and a ROCm device.
"""
import torch

from . import _abi
from ._abi import ptr

EXPORTS = _abi.exports("ex4d_regularizers.h")


def _get(opt, name):
    return opt[name] if isinstance(opt, dict) else getattr(opt, name)


def regularizer_weights(opt, iteration, num_dynamic, views=1):
    """The gates of train.py:156, :159, :163: (static_reg, motion_reg, rot_reg) as they act at `iteration` (0.0 = term off).
    opt: the reference's OptimizationParams (or a dict of its fields).
    views: multiplies the three weights.  A FrameTrainer adds the term once per optimizer step, to the gradient summed over N ranks x k
    views, where the reference adds one term per view: views = N * k restores the reference's balance of data and regulariser.
    The result depends on replicated values only (num_dynamic is the same on every rank), so every rank gets the same weights -- which
    multi-rank training requires and does not check."""
    late_static = iteration > _get(opt, "progressive_growing_steps") + _get(opt, "make_dynamic_interval")
    late_motion = iteration > _get(opt, "progressive_growing_steps") * _get(opt, "extract_every") + _get(opt, "make_dynamic_interval")
    s, m, r = (float(_get(opt, n)) * views for n in ("static_reg", "motion_reg", "rot_reg"))
    return (s if s > 0 and late_static else 0.0,
            m if m > 0 and late_motion and num_dynamic > 0 else 0.0,
            r if r > 0 and late_motion and num_dynamic > 0 else 0.0)


def _check_inputs(xyz_disp, xyz_motion, rotation_motion):
    dev = None
    for t, tail in ((xyz_disp, (3,)), (xyz_motion, None), (rotation_motion, None)):
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(f"regularizers: tensor on {t.device}: the motion regularisers only run on a ROCm GPU (no CPU fallback)")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError("regularizers: parameters must be contiguous float32")
        dev = t.device
    if dev is None:
        raise RuntimeError("regularizers: no tensor given")
    Ns = xyz_disp.shape[0] if xyz_disp is not None else 0
    if xyz_disp is not None and tuple(xyz_disp.shape[1:]) != (3,):
        raise RuntimeError("regularizers: _xyz_disp must be [Ns, 3]")
    Nd, K = 0, 1
    for t, Cc in ((xyz_motion, 3), (rotation_motion, 4)):
        if t is None:
            continue
        if t.dim() != 3 or t.shape[2] != Cc:
            raise RuntimeError(f"regularizers: keyframe tensor must be [Nd, K, {Cc}]")
        if Nd and (t.shape[0], t.shape[1]) != (Nd, K):
            raise RuntimeError("regularizers: _xyz_motion and _rotation_motion disagree on [Nd, K]")
        Nd, K = t.shape[0], t.shape[1]
    return dev, Ns, Nd, K


def forward_raw(xyz_disp, xyz_motion, rotation_motion, weights, out=None, scratch=None):
    """ex4d_reg_forward on the current stream: float32[4] on the device = (static mean, motion mean, rot mean, weighted sum).
    out / scratch: reusable buffers (scratch: new_scratch(device))."""
    dev, Ns, Nd, K = _check_inputs(xyz_disp, xyz_motion, rotation_motion)
    if out is None:
        out = torch.empty(4, dtype=torch.float32, device=dev)
    if scratch is None:
        scratch = new_scratch(dev)
    with _abi.stream(dev) as stream:
        _abi.call("ex4d_reg_forward", ptr(xyz_disp), Ns, ptr(xyz_motion), ptr(rotation_motion), Nd, K, float(weights[0]), float(weights[1]),
                  float(weights[2]), out.data_ptr(), scratch.data_ptr(), stream)
    return out


def new_scratch(device):
    return torch.empty(_abi.load().ex4d_reg_scratch_bytes() // 8, dtype=torch.float64, device=device)


def backward_raw(xyz_disp, xyz_motion, rotation_motion, weights, grads, upstream=None, accumulate=False):
    """ex4d_reg_backward on the current stream.  grads: (g_xyz_disp, g_xyz_motion, g_rotation_motion), None = skip that tensor;
    upstream: one-element float32 device tensor multiplied into the gradients (None = 1); accumulate: add instead of write."""
    dev, Ns, Nd, K = _check_inputs(xyz_disp, xyz_motion, rotation_motion)
    for g, p in zip(grads, (xyz_disp, xyz_motion, rotation_motion)):
        if g is not None and (p is None or g.shape != p.shape or g.dtype != torch.float32 or not g.is_contiguous() or g.device != p.device):
            raise RuntimeError("regularizers: a gradient must be contiguous float32 of its parameter's shape, on its device")
    with _abi.stream(dev) as stream:
        _abi.call("ex4d_reg_backward", ptr(xyz_disp), ptr(grads[0]), Ns, ptr(xyz_motion), ptr(grads[1]), ptr(rotation_motion), ptr(grads[2]), Nd, K,
                  float(weights[0]), float(weights[1]), float(weights[2]), ptr(upstream), int(bool(accumulate)), stream)


REG_MOTION, REG_ROT, REG_STATIC = 1, 2, 3      # kinds of backward_range_raw (1 and 2: optim.REG_MOTION / REG_ROT)


def backward_range_raw(kind, param, lo, hi, grad, weight, accumulate=True):
    """ex4d_reg_backward_range on the current stream: one term's gradient over the flat element range [lo, hi) of `param`, the bits
    backward_raw gives those elements.  kind: REG_MOTION (param [rows,K,3]), REG_ROT ([rows,K,4]) or REG_STATIC ([rows,3]); param: the
    WHOLE tensor (the mean counts its rows); grad: contiguous float32 of hi - lo elements on param's device, grad[0] belongs to element
    lo (e.g. a view of a rank's gradient shard); accumulate: add (the default: the term joins a summed gradient) instead of write."""
    d, m, r = (param if kind == k else None for k in (REG_STATIC, REG_MOTION, REG_ROT))
    if d is None and m is None and r is None:
        raise RuntimeError(f"regularizers: unknown kind {kind} (REG_MOTION, REG_ROT, REG_STATIC)")
    dev, Ns, Nd, K = _check_inputs(d, m, r)
    lo, hi = int(lo), int(hi)                      # (a range outside the tensor is refused by the library, with its text)
    if grad is None or grad.dtype != torch.float32 or not grad.is_contiguous() or grad.device != param.device or grad.numel() != max(hi - lo, 0):
        raise RuntimeError("regularizers: the gradient must be contiguous float32 of hi - lo elements, on its parameter's device")
    with _abi.stream(dev) as stream:
        _abi.call("ex4d_reg_backward_range", int(kind), ptr(param), Ns if kind == REG_STATIC else Nd, K, lo, hi, ptr(grad), float(weight),
                  int(bool(accumulate)), stream)


class _MotionRegularizers(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz_disp, xyz_motion, rotation_motion, static_reg, motion_reg, rot_reg):
        ctx.weights = (float(static_reg), float(motion_reg), float(rot_reg))
        ctx.save_for_backward(xyz_disp, xyz_motion, rotation_motion)
        return forward_raw(xyz_disp.detach(), xyz_motion.detach(), rotation_motion.detach(), ctx.weights)[3]

    @staticmethod
    def backward(ctx, grad_out):
        params = [p.detach() for p in ctx.saved_tensors]
        grads = [torch.empty_like(p) if need else None for p, need in zip(params, ctx.needs_input_grad[:3])]
        up = grad_out.detach().to(torch.float32).reshape(1).contiguous()
        backward_raw(*params, ctx.weights, grads, upstream=up, accumulate=False)
        return grads[0], grads[1], grads[2], None, None, None


def motion_regularizers(xyz_disp, xyz_motion, rotation_motion, static_reg, motion_reg, rot_reg):
    """static_reg * mean log(|_xyz_disp| + 0.001) + motion_reg * mean |_xyz_motion[:, :1] - _xyz_motion[:, 1:]| + rot_reg * mean(1 - cos of
    neighbouring _rotation_motion keyframes, norms clamped at 1e-6): the sum train.py:155-168 adds to the loss, as a 0-d tensor with
    autograd.  Weights as regularizer_weights returns them (0 = term off; an empty dynamic set contributes 0)."""
    return _MotionRegularizers.apply(xyz_disp, xyz_motion, rotation_motion, static_reg, motion_reg, rot_reg)
