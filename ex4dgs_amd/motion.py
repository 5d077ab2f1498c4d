"""Per-Gaussian displacement between two timestamps, in the world or on the screen (include/ex4d_attributes.h, "Motion";
ex4dgs_amd/csrc/ex4d_motion.hip): where each Gaussian goes between t0 and t1.

`displacement(params, t0, t1, space=...)` is a torch.autograd.Function over `_xyz`, `_xyz_disp` and `_xyz_motion` and returns
[Ns+Nd,3], static rows first:

  space="world"   x(t1) - x(t0); x(t) carries the bits attributes.forward_raw gives means3D at that timestamp.
  space="screen"  (u1 - u0, v1 - v0, z1 - z0) for `camera`: the pixel position and view depth the rasterizer's preprocess computes
                  for that mean, bit for bit.  Rows at or behind `near` at either timestamp are exact zeros (and get zero gradients).
                  Fed to the rasterizer as dir3D -- render(..., flow_to=t1) does -- the composited `opticalflow` is in pixels.

One HIP launch each way, no host read-back; no CPU fallback.  `displacement_raw` / `displacement_backward_raw` are the launches
themselves: the backward hands the keyframe gradient back as two windows ([Nd,4,3] each, [Nd,2,3] under linear) and the host hint
(first0, count, first1, count) -- what optim.radam_step_sliced takes as two windows of `_xyz_motion` -- and `dense_from_windows`
builds the dense [Nd,K,3] gradient from them with torch ops.
"""
import ctypes as C

import torch

from . import _abi
from ._abi import ptr as _ptr
from .attributes import interp_code, sliced_shapes, time_scalars

SPACES = {"world": 0, "screen": 1}            # EX4D_MOTION_*
PARAM_NAMES = ("_xyz", "_xyz_disp", "_xyz_motion")


def space_code(space):
    if space not in SPACES:
        raise ValueError(f"unknown space {space!r}: one of {sorted(SPACES)}")
    return SPACES[space]


def _check(tensors):
    dev = tensors[0].device
    if not tensors[0].is_cuda:
        raise RuntimeError(f"parameters are on {dev}: the displacement kernels only run on a ROCm GPU (no CPU fallback)")
    for x in tensors:
        if x.dtype != torch.float32 or x.device != dev or not x.is_contiguous():
            raise RuntimeError("all tensors must be contiguous float32 tensors on the same ROCm device")
    return dev


def _validate(space, camera):
    if space_code(space) == SPACES["screen"] and camera is None:
        raise ValueError("space='screen' needs a camera")


def _view(space, camera, near, dev):
    """(viewmatrix, projmatrix, W, H, min_depth) of the call; the matrices are the [4,4] tensors the rasterizer takes."""
    if space_code(space) == SPACES["world"]:
        return None, None, 0, 0, 0.0
    vm = camera.world_view_transform.to(device=dev, dtype=torch.float32).contiguous()
    pm = camera.full_proj_transform.to(device=dev, dtype=torch.float32).contiguous()
    return vm, pm, int(camera.image_width), int(camera.image_height), float(near)


def displacement_raw(scal0, scal1, xyz, xyz_disp, xyz_motion, space="world", camera=None, near=0.2, interp_type="cube", out=None):
    """One launch of ex4d_motion_forward on the current stream (scal0, scal1: attributes.time_scalars of t0 and t1 for the same
    interp_type).  out: optional [Ns+Nd,3] buffer (any contents: every row is written).  No autograd."""
    interp = interp_code(interp_type)
    _validate(space, camera)
    dev = _check([xyz, xyz_disp, xyz_motion])
    vm, pm, W, H, min_depth = _view(space, camera, near, dev)
    N = scal0.Ns + scal0.Nd
    if out is None:
        out = torch.empty(N, 3, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (N, 3):
        raise RuntimeError(f"out must have the shape {(N, 3)}")
    _check([out] + [m for m in (vm, pm) if m is not None])
    with _abi.stream(dev) as stream:
        _abi.call("ex4d_motion_forward", C.byref(scal0), C.byref(scal1), interp, SPACES[space], _ptr(xyz), _ptr(xyz_disp), _ptr(xyz_motion),
                  _ptr(vm), _ptr(pm), W, H, min_depth, _ptr(out), stream)
    return out


def displacement_backward_raw(scal0, scal1, xyz, xyz_disp, xyz_motion, g_out, space="world", camera=None, near=0.2, interp_type="cube"):
    """One launch of ex4d_motion_backward on the current stream.  Returns (g_xyz[Ns,3], g_xyz_disp[Ns,3], g_win0, g_win1, hint): the
    windows are [Nd,4,3] ([Nd,2,3] under linear), hint = (first0, count, first1, count) on the host."""
    interp = interp_code(interp_type)
    _validate(space, camera)
    dev = _check([xyz, xyz_disp, xyz_motion])
    vm, pm, W, H, min_depth = _view(space, camera, near, dev)
    N = scal0.Ns + scal0.Nd
    g_out = g_out.contiguous()
    if tuple(g_out.shape) != (N, 3):
        raise RuntimeError(f"g_out must have the shape {(N, 3)}")
    _check([g_out] + [m for m in (vm, pm) if m is not None])
    f32 = dict(dtype=torch.float32, device=dev)
    window = (scal0.Nd,) + sliced_shapes(interp_type)["_xyz_motion"]
    g_xyz, g_disp = torch.empty(scal0.Ns, 3, **f32), torch.empty(scal0.Ns, 3, **f32)
    g_win0, g_win1 = torch.empty(window, **f32), torch.empty(window, **f32)
    hint = (C.c_int32 * 4)()
    with _abi.stream(dev) as stream:
        _abi.call("ex4d_motion_backward", C.byref(scal0), C.byref(scal1), interp, SPACES[space], _ptr(xyz), _ptr(xyz_disp), _ptr(xyz_motion),
                  _ptr(vm), _ptr(pm), W, H, min_depth, _ptr(g_out), _ptr(g_xyz), _ptr(g_disp), _ptr(g_win0), _ptr(g_win1), hint, stream)
    return g_xyz, g_disp, g_win0, g_win1, tuple(int(v) for v in hint)


def dense_from_windows(g_win0, g_win1, hint, K):
    """The dense [Nd,K,3] keyframe gradient: zeros, window 0, then window 1 added -- summed in that order where they overlap."""
    first0, count0, first1, count1 = hint
    dense = torch.zeros(g_win0.shape[0], K, 3, dtype=g_win0.dtype, device=g_win0.device)
    if g_win0.shape[0]:
        dense[:, first0:first0 + count0] = g_win0
        dense[:, first1:first1 + count1] += g_win1
    return dense


class _Displacement(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scal0, scal1, space, camera, near, interp_type, xyz, xyz_disp, xyz_motion):
        p = [x.contiguous() for x in (xyz, xyz_disp, xyz_motion)]
        ctx.call = (scal0, scal1, space, camera, near, interp_type)
        ctx.save_for_backward(*p)
        return displacement_raw(scal0, scal1, *p, space=space, camera=camera, near=near, interp_type=interp_type)

    @staticmethod
    def backward(ctx, g_out):
        scal0, scal1, space, camera, near, interp_type = ctx.call
        xyz, xyz_disp, xyz_motion = ctx.saved_tensors
        g_xyz, g_disp, g_win0, g_win1, hint = displacement_backward_raw(scal0, scal1, xyz, xyz_disp, xyz_motion, g_out, space=space,
                                                                        camera=camera, near=near, interp_type=interp_type)
        return (None,) * 6 + (g_xyz, g_disp, dense_from_windows(g_win0, g_win1, hint, scal0.K).reshape(xyz_motion.shape))


def displacement(params, t0, t1, *, space="world", camera=None, near=0.2, interp_type="cube", duration=300, interval=10, time_shift=12,
                 var_pad=3):
    """params: mapping with `_xyz`, `_xyz_disp`, `_xyz_motion` (more entries are ignored); the other arguments as in
    attributes.evaluate_attributes (`time_shift` is the model's own: time_pad for linear, time_pad + interval otherwise).  Returns the
    [Ns+Nd,3] displacement from t0 to t1 (module docstring); differentiable in the three tensors.  pchip keeps the reference's quirk
    (NaN keyframe gradients where y[k+1] == y[k-1])."""
    _validate(space, camera)
    xyz, xyz_disp, xyz_motion = (params[n] for n in PARAM_NAMES)
    Ns, Nd = xyz.shape[0], xyz_motion.shape[0]
    K = xyz_motion.shape[1] if Nd > 0 else 0
    scal0 = time_scalars(t0, Ns, Nd, K, duration, interval, time_shift, var_pad, interp_type)
    scal1 = time_scalars(t1, Ns, Nd, K, duration, interval, time_shift, var_pad, interp_type)
    return _Displacement.apply(scal0, scal1, space, camera, float(near), interp_type, xyz, xyz_disp, xyz_motion)
