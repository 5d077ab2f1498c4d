"""ctypes mirror of include/ex4d_trainer.h: the compiled host path of one training iteration.

    attributes -> render (SplitSH) -> L1+SSIM -> rasterizer backward -> attribute backward (sliced) -> RAdam
    (train.py:124-153, :244-255 of the reference for one view), sequenced in C++ on the current stream with a persistent workspace.

Same kernels as trainer.FrameTrainer + loss.l1_ssim_loss, without the Python / autograd / allocator work per iteration (one ctypes
call instead of ~40 tensor operations).  Single process; for N ranks use FrameTrainer (it owns the gradient exchange).
No CPU fallback: the library and a ROCm device are required.
"""
import ctypes as C
import math

import torch

from . import _abi
from . import attributes as attr
from ._abi import Ex4dTrainerConfig, load as _lib
from .loss import _WINDOW
from .trainer import reference_lrs

EXPORTS = _abi.exports("ex4d_trainer.h")


class NativeTrainer:
    """model: scene.DynamicGaussians on a ROCm device (its 15 parameter tensors are updated in place).  cam: the image size and field
    of view are fixed at construction; step() takes any camera of that size."""

    def __init__(self, model, cam, optimizer=True, lrs=None, lambda_dssim=0.2, near=0.2, far=300.0, betas=(0.9, 0.999), eps=1e-8,
                 spatial_lr_scale=1.0):
        """lrs: per-parameter learning rates overriding the reference table (trainer.reference_lrs(spatial_lr_scale));
        near / far default to the reference's dataset.near / dataset.far (arguments/__init__.py:74-75).  This is the render +
        L1/SSIM + RAdam core of the iteration (include/ex4d_trainer.h: SCOPE): the motion regularisers are off until set_regularizers
        gives them weights; no l1_accum hook, no densification."""
        self.model = model
        self.names = list(attr.PARAM_ORDER)
        self.params = [getattr(model, n) for n in self.names]
        dev = self.params[0].device
        if dev.type != "cuda":
            raise RuntimeError("NativeTrainer needs the model on a ROCm device (no CPU fallback)")
        for n, p in zip(self.names, self.params):
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                raise RuntimeError(f"{n} must be a contiguous float32 tensor on {dev}")
        self.device = dev
        self.H, self.W = int(cam.image_height), int(cam.image_width)
        cfg = Ex4dTrainerConfig()
        cfg.Ns, cfg.Nd = model.num_static, model.num_dynamic
        cfg.K = model._xyz_motion.shape[1] if model.num_dynamic else 0
        cfg.W, cfg.H, cfg.sh_degree = self.W, self.H, model.active_sh_degree
        cfg.tanfovx, cfg.tanfovy, cfg.kernel_size = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), model.kernel_size
        cfg.min_depth, cfg.max_depth = near, far
        cfg.duration, cfg.interval, cfg.time_shift, cfg.var_pad = model.duration, model.interval, model.time_shift, model.var_pad
        cfg.lambda_dssim = lambda_dssim
        cfg.window = (C.c_float * 11)(*[float(x) for x in _WINDOW])
        lrs = dict(reference_lrs(spatial_lr_scale), **(lrs or {}))
        cfg.lr = (C.c_double * 15)(*[float(lrs[n]) for n in self.names])
        cfg.beta1, cfg.beta2, cfg.eps, cfg.optimizer = betas[0], betas[1], eps, int(bool(optimizer))
        self.cfg = cfg
        lib = _lib()
        ptrs = (C.c_void_p * 15)(*[_abi.ptr(p) for p in self.params])
        with torch.cuda.device(dev):
            self.handle = lib.ex4d_trainer_create(C.byref(cfg), ptrs)
        if not self.handle:                    # a pointer, not a status: NULL is the refusal
            raise RuntimeError(lib.ex4d_trainer_last_error().decode())
        self.num_rendered = 0

    def step(self, cam, bg, t, gt_image):
        """One iteration on the current stream (asynchronous apart from the rasterizer's instance-count read-back)."""
        if int(cam.image_height) != self.H or int(cam.image_width) != self.W:
            raise RuntimeError("camera size differs from the one the trainer was built for")
        if tuple(gt_image.shape) != (3, self.H, self.W) or gt_image.dtype != torch.float32 or not gt_image.is_contiguous() or gt_image.device != self.device:
            raise RuntimeError(f"gt_image must be a contiguous float32 [3,{self.H},{self.W}] tensor on {self.device}")
        R = C.c_int32(0)
        with _abi.stream(self.device) as stream:
            _abi.call("ex4d_trainer_step", self.handle, float(t), cam.world_view_transform.data_ptr(), cam.full_proj_transform.data_ptr(),
                      cam.camera_center.data_ptr(), bg.data_ptr(), gt_image.data_ptr(), stream, C.byref(R))
        self.num_rendered = R.value
        if self.cfg.optimizer:
            torch.autograd.graph.increment_version(self.params)

    def set_lrs(self, lrs):
        """Learning rates from the next step on (dict name -> value; unnamed groups keep theirs): the reference's update_learning_rate."""
        cur = {n: self.cfg.lr[i] for i, n in enumerate(self.names)}
        cur.update(lrs)
        arr = (C.c_double * 15)(*[float(cur[n]) for n in self.names])
        _abi.call("ex4d_trainer_set_lr", self.handle, arr)
        self.cfg.lr = arr

    def set_sh_degree(self, degree):
        """Active SH degree from the next step on (oneupSHdegree, train.py:113-114)."""
        _abi.call("ex4d_trainer_set_sh_degree", self.handle, int(degree))
        self.cfg.sh_degree = int(degree)
        self.model.active_sh_degree = int(degree)

    def set_async(self, on=True):
        """Asynchronous rasterizer forward (no instance-count read-back in the middle of the frame; include/ex4d_trainer.h):
        same parameters as the synchronous path -- a frame that overflows its capacity is re-run before the optimizer step."""
        _abi.call("ex4d_trainer_set_async", self.handle, int(bool(on)))

    def set_regularizers(self, static_reg=0.0, motion_reg=0.0, rot_reg=0.0):
        """Weights of the motion regularisers (train.py:155-168) from the next step on, as regularizers.regularizer_weights returns them
        for the iteration (a 3-tuple as the first argument works too); all 0 = off.  output('reg') holds their values."""
        if isinstance(static_reg, (tuple, list)):
            static_reg, motion_reg, rot_reg = static_reg
        _abi.call("ex4d_trainer_set_regularizers", self.handle, float(static_reg), float(motion_reg), float(rot_reg))

    def replays(self):
        return int(_lib().ex4d_trainer_replays(self.handle))

    def output(self, what):
        """Copies of the trainer's outputs of the last step: 'loss', 'render', 'radii', 'viewspace_grad', 'depth', 'acc', 'reg' (the
        regularisers' three means and their weighted sum)."""
        idx = {"loss": 0, "render": 1, "radii": 2, "viewspace_grad": 3, "depth": 4, "acc": 5, "reg": 6}[what]
        P = self.cfg.Ns + self.cfg.Nd
        shape, dtype = {0: ((1,), torch.float32), 1: ((3, self.H, self.W), torch.float32), 2: ((P,), torch.int32), 3: ((P, 3), torch.float32),
                        4: ((1, self.H, self.W), torch.float32), 5: ((1, self.H, self.W), torch.float32), 6: ((4,), torch.float32)}[idx]
        return self._read(idx, shape, dtype)

    def grad(self, name):
        """Copy of the gradient of parameter `name` of the last step (slices [Nd,4,3] / [Nd,2,4] for the two keyframe tensors) and the
        slice hint (xyz first keyframe, 4, rotation first keyframe, 2)."""
        i = self.names.index(name)
        hint = (C.c_int32 * 4)()
        _lib().ex4d_trainer_grad(self.handle, i, hint)
        p = self.params[i]
        shape = (p.shape[0],) + attr.SLICED_SHAPES[name] if name in attr.SLICED_SHAPES else tuple(p.shape)
        return self._read(100 + i, shape, torch.float32), tuple(int(x) for x in hint)

    def _read(self, what, shape, dtype):
        out = torch.empty(shape, dtype=dtype, device=self.device)
        if out.numel():
            with _abi.stream(self.device) as stream:
                _abi.call("ex4d_trainer_read", self.handle, what, out.data_ptr(), out.numel() * out.element_size(), stream)
        return out

    def bytes(self):
        return int(_lib().ex4d_trainer_bytes(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            _lib().ex4d_trainer_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
