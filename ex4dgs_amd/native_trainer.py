"""ctypes mirror of include/ex4d_trainer.h: the compiled host path of one training iteration.

    attributes -> render (SplitSH) -> L1+SSIM -> rasterizer backward -> attribute backward (sliced) -> RAdam
    (train.py:124-153, :244-255 of the reference for one view), sequenced in C++ on the current stream with a persistent workspace.

Same kernels as trainer.FrameTrainer + loss.l1_ssim_loss, without the Python / autograd / allocator work per iteration (one ctypes
call instead of ~40 tensor operations).  Single process; for N ranks use FrameTrainer (it owns the gradient exchange).
No CPU fallback: the library and a ROCm device are required.

The reference's default schedule through the same call (ex4d_trainer_step_ex):

    stats = densify.DensityStats(model)
    native.step(cam, bg, t, gt, l1_accum=True, stats=stats, nan_census=True,
                apply_optimizer=not densify_now)         # train.py densifies before optimizer.step(): that update is dropped
    loss, nan_s, nan_d = native.report()                 # the iteration's one wait
    if nan_s or nan_d: densify.prune_nan_points(model, stats, native)
    if densify_now:    densify.densify_and_prune(model, stats, native, ...)          # also the prunes and ex4dgs_amd.growth

Density control replaces the model's tensors: densify / growth carry the trainer's moments and step count into a new native handle
(begin_density_control / rebind_parameters).
"""
import ctypes as C
import math

import torch

from . import _abi
from . import attributes as attr
from ._abi import Ex4dTrainerConfig, Ex4dTrainerReport, Ex4dTrainerStepOptions, load as _lib
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
        gives them weights; the l1_accum hook, the densification statistics and the NaN census are options of step()."""
        self.model = model
        self.names = list(attr.PARAM_ORDER)
        self.H, self.W = int(cam.image_height), int(cam.image_width)
        cfg = Ex4dTrainerConfig()
        cfg.W, cfg.H, cfg.sh_degree = self.W, self.H, model.active_sh_degree
        cfg.tanfovx, cfg.tanfovy, cfg.kernel_size = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), model.kernel_size
        cfg.min_depth, cfg.max_depth = near, far
        cfg.lambda_dssim = lambda_dssim
        cfg.window = (C.c_float * 11)(*[float(x) for x in _WINDOW])
        lrs = dict(reference_lrs(spatial_lr_scale), **(lrs or {}))
        cfg.lr = (C.c_double * 15)(*[float(lrs[n]) for n in self.names])
        cfg.beta1, cfg.beta2, cfg.eps, cfg.optimizer = betas[0], betas[1], eps, int(bool(optimizer))
        self.cfg = cfg
        self.handle = None
        self._async, self._reg_w = False, (0.0, 0.0, 0.0)
        self._moments, self._steps = None, 0
        self.interp_type = getattr(model, "interp_type", "cube")     # kept like the SH degree: every new handle is told again
        attr.interp_code(self.interp_type)
        self._create()
        self.num_rendered = 0

    def _create(self):
        """A native handle over the model's current tensors: Ns, Nd, K and the model's time constants are read now."""
        model, cfg = self.model, self.cfg
        self.params = [getattr(model, n) for n in self.names]
        dev = self.params[0].device
        if dev.type != "cuda":
            raise RuntimeError("NativeTrainer needs the model on a ROCm device (no CPU fallback)")
        for n, p in zip(self.names, self.params):
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                raise RuntimeError(f"{n} must be a contiguous float32 tensor on {dev}")
        self.device = dev
        cfg.Ns, cfg.Nd = model.num_static, model.num_dynamic
        cfg.K = model._xyz_motion.shape[1] if model.num_dynamic else 0
        cfg.duration, cfg.interval, cfg.time_shift, cfg.var_pad = model.duration, model.interval, model.time_shift, model.var_pad
        lib = _lib()
        ptrs = (C.c_void_p * 15)(*[_abi.ptr(p) for p in self.params])
        with torch.cuda.device(dev):
            self.handle = lib.ex4d_trainer_create(C.byref(cfg), ptrs)
        if not self.handle:                    # a pointer, not a status: NULL is the refusal
            raise RuntimeError(lib.ex4d_trainer_last_error().decode())
        _abi.call("ex4d_trainer_set_interp", self.handle, attr.interp_code(self.interp_type))

    def step(self, cam, bg, t, gt_image, *, l1_accum=False, stats=None, densify_stats=True, prune_stats=True, apply_optimizer=True,
             nan_census=False, lut=None):
        """One iteration on the current stream (asynchronous apart from the rasterizer's instance-count read-back).
        l1_accum: the error hook of train.py:148-153 -- output('error_grad') is viewspace_l1points.grad, output('hook') the hook tensor.
        stats: a densify.DensityStats updated by this frame as DensityStats.update(radii, viewspace_grad, error_grad, t,
        densify_stats=, prune_stats=, l1_accum=) would (its blocks are looked up at every call: density control replaces them).
        apply_optimizer=False: gradients and statistics only -- the iteration train.py densifies in, whose optimizer.step() skips every
        replaced tensor; the step count does not advance.  nan_census: report() tells whether _xyz / _xyz_motion hold a NaN after the
        step.  All defaults: the plain ex4d_trainer_step.
        gt_image may be the frame as decoded: a contiguous uint8 [H,W,3|4] device tensor (frames.FrameStore.get / FrameStream.pop)
        with lut (CPU float32 [256], frames.gt_lut(im_scale); None: u / 255) -- ex4d_trainer_step_u8, the same iteration.  The frame
        must keep its content until the step's work on the stream is done."""
        if int(cam.image_height) != self.H or int(cam.image_width) != self.W:
            raise RuntimeError("camera size differs from the one the trainer was built for")
        u8 = gt_image.dtype == torch.uint8
        if u8:
            if gt_image.dim() != 3 or tuple(gt_image.shape[:2]) != (self.H, self.W) or gt_image.shape[2] not in (3, 4) \
                    or not gt_image.is_contiguous() or gt_image.device != self.device:
                raise RuntimeError(f"uint8 gt_image must be a contiguous [{self.H},{self.W},3|4] tensor on {self.device}")
            if lut is not None and (lut.device.type != "cpu" or lut.dtype != torch.float32 or tuple(lut.shape) != (256,) or not lut.is_contiguous()):
                raise RuntimeError("lut must be a contiguous CPU float32 [256] tensor (frames.gt_lut)")
        elif lut is not None:
            raise RuntimeError("lut= belongs to uint8 ground truth; a float gt_image already holds its values")
        elif tuple(gt_image.shape) != (3, self.H, self.W) or gt_image.dtype != torch.float32 or not gt_image.is_contiguous() or gt_image.device != self.device:
            raise RuntimeError(f"gt_image must be a contiguous float32 [3,{self.H},{self.W}] tensor on {self.device}")
        self._moments = None
        R = C.c_int32(0)
        args = (self.handle, float(t), cam.world_view_transform.data_ptr(), cam.full_proj_transform.data_ptr(),
                cam.camera_center.data_ptr(), bg.data_ptr(), gt_image.data_ptr())
        plain = not l1_accum and stats is None and apply_optimizer and not nan_census
        if not plain:
            from .densify import GRAD_STATS, L1_STATS, PRUNE_STATS
            o = Ex4dTrainerStepOptions()
            o.l1_accum, o.skip_optimizer, o.nan_census = int(bool(l1_accum)), int(not apply_optimizer), int(bool(nan_census))
            if stats is not None:
                ns, nd = stats.static.shape[1], stats.dynamic.shape[1]
                if (ns, nd) != (self.cfg.Ns, self.cfg.Nd) or stats.static.device != self.device or stats.dynamic.device != self.device \
                        or not stats.static.is_contiguous() or not stats.dynamic.is_contiguous():
                    raise RuntimeError(f"stats holds {ns} + {nd} rows, the trainer {self.cfg.Ns} + {self.cfg.Nd} (contiguous blocks on {self.device})")
                # composed as DensityStats.update composes them
                o.stats_flags = (GRAD_STATS if densify_stats else 0) | (PRUNE_STATS if (prune_stats and l1_accum) else 0) | \
                                (L1_STATS if (densify_stats and l1_accum) else 0)
                o.stats_s, o.stats_d = _abi.ptr(stats.static), _abi.ptr(stats.dynamic)
        with _abi.stream(self.device) as stream:
            if u8:
                _abi.call("ex4d_trainer_step_u8", *args, int(gt_image.shape[2]), _abi.ptr(lut), stream, C.byref(R), None if plain else C.byref(o))
            elif plain:
                _abi.call("ex4d_trainer_step", *args, stream, C.byref(R))
            else:
                _abi.call("ex4d_trainer_step_ex", *args, stream, C.byref(R), C.byref(o))
        self.num_rendered = R.value
        if self.cfg.optimizer and apply_optimizer:
            torch.autograd.graph.increment_version(self.params)

    def report(self):
        """(loss, nan_static, nan_dynamic) of the last step that took an option: waits for that step (the iteration's one
        synchronisation, in place of loss.item() and prune_nan_points' count read-back).  The flags are 0 without nan_census."""
        r = Ex4dTrainerReport()
        _abi.call("ex4d_trainer_report", self.handle, C.byref(r))
        return float(r.loss), int(r.nan_static), int(r.nan_dynamic)

    # ---- density control and growth (ex4dgs_amd.densify / .growth call these two; the moments travel as torch tensors)
    def steps(self):
        """RAdam's step count."""
        n = C.c_int64(0)
        _abi.call("ex4d_trainer_get_step", self.handle, C.byref(n))
        return int(n.value)

    def moments(self):
        """{name: (exp_avg, exp_avg_sq)} copies of the optimizer state ({name: None} without an optimizer)."""
        if not self.cfg.optimizer:
            return {n: None for n in self.names}
        return {n: (self._read(200 + i, tuple(p.shape), torch.float32), self._read(300 + i, tuple(p.shape), torch.float32))
                for i, (n, p) in enumerate(zip(self.names, self.params))}

    def write_moment(self, name, which, value):
        """exp_avg (which = 0) or exp_avg_sq (1) of parameter `name` from a device tensor of the parameter's shape."""
        i = self.names.index(name)
        p = self.params[i]
        if tuple(value.shape) != tuple(p.shape) or value.dtype != torch.float32 or value.device != self.device or not value.is_contiguous():
            raise RuntimeError(f"moment of {name}: a contiguous float32 {tuple(p.shape)} tensor on {self.device}")
        if value.numel():
            with _abi.stream(self.device) as stream:
                _abi.call("ex4d_trainer_write", self.handle, (200, 300)[which] + i, value.data_ptr(), value.numel() * 4, stream)

    def begin_density_control(self):
        """Before densify / growth replaces the model's tensors: the moments and the step count as torch tensors / an int.  Nothing is
        pending in a NativeTrainer (the step that precedes density control ran with apply_optimizer=False)."""
        self._moments, self._steps = self.moments(), (self.steps() if self.cfg.optimizer else 0)
        return self._moments

    def rebind_parameters(self, moments=None):
        """After the model's tensors were replaced: a new native handle over them (Ns, Nd, K re-read; the whole workspace is freed
        and allocated again), the moments written back (moments: {name: (exp_avg, exp_avg_sq)} for the new rows; None: zeros), the
        step count, learning rates, SH degree, asynchronous mode and regulariser weights as they were."""
        steps = self.steps() if self.cfg.optimizer else 0
        self.close()
        self._moments = None
        self._create()
        if self.cfg.optimizer:
            for n in self.names:
                pair = (moments or {}).get(n)
                if pair is not None:
                    self.write_moment(n, 0, pair[0])
                    self.write_moment(n, 1, pair[1])
            _abi.call("ex4d_trainer_set_step", self.handle, steps)
        if self._async:
            _abi.call("ex4d_trainer_set_async", self.handle, 1)
        if any(self._reg_w):
            _abi.call("ex4d_trainer_set_regularizers", self.handle, *self._reg_w)

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

    def set_interp(self, interp_type):
        """The position interpolator ('cube', 'linear', 'pchip') of the steps to come; the constructor takes it from the model, so this
        is for a handle that has not stepped yet -- afterwards the native side refuses (the model's time_shift and keyframe window
        belong to one interpolator)."""
        _abi.call("ex4d_trainer_set_interp", self.handle, attr.interp_code(interp_type))
        self.interp_type = interp_type

    def set_async(self, on=True):
        """Asynchronous rasterizer forward (no instance-count read-back in the middle of the frame; include/ex4d_trainer.h):
        same parameters as the synchronous path -- a frame that overflows its capacity is re-run before the optimizer step."""
        _abi.call("ex4d_trainer_set_async", self.handle, int(bool(on)))
        self._async = bool(on)

    def set_regularizers(self, static_reg=0.0, motion_reg=0.0, rot_reg=0.0):
        """Weights of the motion regularisers (train.py:155-168) from the next step on, as regularizers.regularizer_weights returns them
        for the iteration (a 3-tuple as the first argument works too); all 0 = off.  output('reg') holds their values."""
        if isinstance(static_reg, (tuple, list)):
            static_reg, motion_reg, rot_reg = static_reg
        _abi.call("ex4d_trainer_set_regularizers", self.handle, float(static_reg), float(motion_reg), float(rot_reg))
        self._reg_w = (float(static_reg), float(motion_reg), float(rot_reg))

    def replays(self):
        return int(_lib().ex4d_trainer_replays(self.handle))

    def output(self, what):
        """Copies of the trainer's outputs of the last step: 'loss', 'render', 'radii', 'viewspace_grad', 'depth', 'acc', 'reg' (the
        regularisers' three means and their weighted sum), 'error_grad' ([P,3]: viewspace_l1points.grad of an l1_accum step) and
        'hook' ([3,H,W]: stack([acc[0], l1_errors, ssim_errors]) of an l1_accum step)."""
        idx = {"loss": 0, "render": 1, "radii": 2, "viewspace_grad": 3, "depth": 4, "acc": 5, "reg": 6, "error_grad": 7, "hook": 8}[what]
        P = self.cfg.Ns + self.cfg.Nd
        shape, dtype = {0: ((1,), torch.float32), 1: ((3, self.H, self.W), torch.float32), 2: ((P,), torch.int32), 3: ((P, 3), torch.float32),
                        4: ((1, self.H, self.W), torch.float32), 5: ((1, self.H, self.W), torch.float32), 6: ((4,), torch.float32),
                        7: ((P, 3), torch.float32), 8: ((3, self.H, self.W), torch.float32)}[idx]
        return self._read(idx, shape, dtype)

    def grad(self, name):
        """Copy of the gradient of parameter `name` of the last step (slices [Nd,4,3] / [Nd,2,4] for the two keyframe tensors) and the
        slice hint (xyz first keyframe, 4, rotation first keyframe, 2); under 'linear' the position slices are [Nd,2,3] and the hint
        says 2."""
        i = self.names.index(name)
        hint = (C.c_int32 * 4)()
        _lib().ex4d_trainer_grad(self.handle, i, hint)
        p = self.params[i]
        window = attr.sliced_shapes(self.interp_type)
        shape = (p.shape[0],) + window[name] if name in window else tuple(p.shape)
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
