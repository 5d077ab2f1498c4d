"""Fused RAdam: a torch.optim.Optimizer with the constructor, param-group and state layout of
`torch.optim.RAdam` -- what the reference builds at scene/c_gaussian_model.py:449 and steps at train.py:250 -- whose
step() is ONE HIP launch over every parameter tensor (include/ex4d_optim.h) instead of ~10 element-wise passes per tensor.

State per parameter: {"step": float32 CPU scalar tensor, "exp_avg", "exp_avg_sq"} -- the same keys and shapes as
torch.optim.RAdam, so the reference's densification code that edits optimizer state in place
(c_gaussian_model.py: replace_tensor_to_optimizer / _prune_optimizer / cat_tensors_to_optimizer) works unchanged.
No CPU fallback: parameters must live on a ROCm device.
"""
import ctypes as C

import torch

from . import _abi
from ._abi import Ex4dRadamSlicedRegTensor, Ex4dRadamSlicedTensor, Ex4dRadamTensor

EXPORTS = _abi.exports("ex4d_optim.h")
REG_NONE, REG_MOTION, REG_ROT = 0, 1, 2
MAX_WINDOWS = _abi.RADAM_MAX_WINDOWS
MAX_SLICED = 4
MAX_TENSORS = 32


def _launch(descs, struct, entry, limit, betas, eps, device):
    """`entry` over descs (a list of `struct`), at most `limit` per call, on device's current stream; a refused call raises its text."""
    with _abi.stream(device) as stream:
        for i in range(0, len(descs), limit):
            chunk = descs[i:i + limit]
            _abi.call(entry, (struct * len(chunk))(*chunk), len(chunk), betas[0], betas[1], eps, stream)


def radam_step_raw(items, betas, eps, device):
    """One fused launch (per <= 32 tensors) over raw element ranges.  items: iterable of
    (param_ptr, grad_ptr, exp_avg_ptr, exp_avg_sq_ptr, numel, lr, step[, nan_to_num]) -- plain device pointers, so a range may be a
    whole tensor or a rank's shard of one (RAdam is element-wise: updating ranges separately gives bit-identical results).
    nan_to_num = 1 reads the gradient through torch.nan_to_num (train.py:244-247 does that to _opacity_duration_var.grad)."""
    descs = [Ex4dRadamTensor(int(it[0]), int(it[1]), int(it[2]), int(it[3]), int(it[4]), float(it[5]), int(it[6]), int(it[7]) if len(it) > 7 else 0, 0)
             for it in items if it[4] > 0]
    _launch(descs, Ex4dRadamTensor, "ex4d_radam_step", MAX_TENSORS, betas, eps, device)


def _sliced_descs(items, reg=False):
    """The descriptors of the sliced item tuples (radam_step_sliced_raw; reg: radam_step_sliced_reg_raw); tensors without rows are left out."""
    descs = []
    for it in items:
        p, m, v, rows, K, Cc, lr, step, windows = it[:9]
        first_dev = it[9] if len(it) > 9 else None
        if rows <= 0:
            continue
        if len(windows) > MAX_WINDOWS:
            raise RuntimeError(f"at most {MAX_WINDOWS} gradient windows per tensor and step")
        if first_dev is None and any(w[0] is None for w in windows):
            raise RuntimeError("radam_step_sliced_raw: a window without a host position needs first_dev (SliceGather.first_device_ptr())")
        first = (C.c_int32 * 8)(*([(0 if w[0] is None else int(w[0])) for w in windows] + [0] * (8 - len(windows))))
        count = (C.c_int32 * 8)(*([w[1] for w in windows] + [0] * (8 - len(windows))))
        grad = (C.c_void_p * 8)(*([int(w[2]) for w in windows] + [None] * (8 - len(windows))))
        d = Ex4dRadamSlicedTensor(int(p), int(m), int(v), int(rows), int(K), int(Cc), float(lr), int(step), len(windows), first, count, grad,
                                  int(first_dev) if first_dev else None)
        if reg:
            kind, weight, reg_rows = it[10:]
            d = Ex4dRadamSlicedRegTensor(d, int(kind), 0, float(weight), int(reg_rows))
        descs.append(d)
    return descs


def radam_step_sliced_raw(items, betas, eps, device):
    """ex4d_radam_step_sliced over keyframe tensors [rows, K, C] with windowed gradients.  items: iterable of
    (param_ptr, exp_avg_ptr, exp_avg_sq_ptr, rows, K, C, lr, step, windows[, first_dev_ptr]) with windows = [(first, count, grad_ptr), ...]
    (<= 8), grad_ptr -> [rows, count, C] floats; first_dev_ptr (optional): device int32 array of the windows' first keyframes, read by
    the kernel instead of the host values (no device -> host round trip when the positions were gathered from other ranks).
    Bit-identical to radam_step_raw on the dense gradient the windows add up to."""
    _launch(_sliced_descs(items), Ex4dRadamSlicedTensor, "ex4d_radam_step_sliced", MAX_SLICED, betas, eps, device)


def sliced_reg_rows(K, Cc):
    """Rows of a [rows, K, C] tensor one workgroup of ex4d_radam_step_sliced_reg owns; 0: K is too large for the fused step."""
    return int(_abi.load().ex4d_radam_sliced_reg_rows(int(K), int(Cc)))


def radam_step_sliced_reg_raw(items, betas, eps, device):
    """ex4d_radam_step_sliced_reg: radam_step_sliced_raw with a motion regulariser's gradient (train.py:159-168) formed inside the
    kernel from each Gaussian's own row and added to the windows last.  items: the tuples of radam_step_sliced_raw with first_dev_ptr
    present (None = host positions) followed by (reg_kind, reg_weight, reg_rows): REG_NONE / REG_MOTION ([rows,K,3]) / REG_ROT
    ([rows,K,4]), the term's weight of this step and the model's full dynamic count Nd (the mean is over Nd (K-1) terms; `rows` may
    be a row range).  Bit-identical to radam_step_raw on (windows scattered into zeros + regularizers.backward_raw(accumulate=1))."""
    _launch(_sliced_descs(items, reg=True), Ex4dRadamSlicedRegTensor, "ex4d_radam_step_sliced_reg", MAX_SLICED, betas, eps, device)


class FusedRAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        if weight_decay != 0:
            raise ValueError("FusedRAdam: weight_decay is not used by the reference (c_gaussian_model.py:449) and is not implemented")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError("FusedRAdam: invalid hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        batches = {}                               # (device, betas, eps) -> (descriptor, the gradient it points into)
        touched = []                               # tensors the library writes: their autograd version counters are bumped below
        f32 = torch.float32
        for group in self.param_groups:
            key_tail = (tuple(group["betas"]), float(group["eps"]))
            lr = float(group["lr"])
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue                       # like torch: tensors without a gradient keep their step count
                if not p.is_cuda:
                    raise RuntimeError(f"parameter on {p.device}: FusedRAdam only runs on a ROCm GPU (no CPU fallback)")
                if p.dtype != f32 or g.dtype != f32 or g.is_sparse or not p.is_contiguous():
                    raise RuntimeError("FusedRAdam: parameters and gradients must be dense contiguous float32")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=f32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                step_t = state["step"]
                step_t += 1
                if not g.is_contiguous():
                    g = g.contiguous()
                m, v = state["exp_avg"], state["exp_avg_sq"]
                if not (m.is_contiguous() and v.is_contiguous()):
                    raise RuntimeError("FusedRAdam: optimizer state must be contiguous")
                batches.setdefault((p.device,) + key_tail, []).append(
                    (Ex4dRadamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, int(step_t.item()), 0, 0), g))
                touched += (p, m, v)
        for (dev, betas, eps), items in batches.items():       # (a gradient made contiguous above lives in `batches` until here)
            _launch([d for d, _ in items], Ex4dRadamTensor, "ex4d_radam_step", MAX_TENSORS, betas, eps, dev)
        # the library wrote through raw pointers: tell autograd the tensors changed (version counters), exactly what the
        # in-place torch ops of torch.optim.RAdam do -- caches keyed on parameter versions depend on it
        if touched:
            torch.autograd.graph.increment_version(touched)
        return loss
