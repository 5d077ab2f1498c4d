"""Growth of the dynamic set (include/ex4d_densify.h, ex4d_growth_*): extract_dynamic_points_from_static, expand_duration and
adjust_temp_opa of the reference's CGaussianModel (scene/c_gaussian_model.py:1147-1358) on the HIP library, with the matching edits
of the optimizer state, and the error-timestamp bookkeeping that picks the extraction timestamp (:1299-1328).

    stats = densify.DensityStats(model)
    errors = ErrorTimestamps(model.interval)
    errors.mark(loss, timestamp)                                                             # every iteration
    extract_dynamic_points(model, stats, opt, cam.camera_center, errors.pop(), vis, extent)  # every extraction interval
    expand_duration(model, opt, duration)
    adjust_temp_opa(model, opt)

`opt` is as in ex4dgs_amd.densify: torch.optim.RAdam / FusedRAdam over the reference's 15 groups, a trainer.FrameTrainer, a
native_trainer.NativeTrainer, or None.
No CPU fallback: everything runs on a ROCm device.  DESIGN.md section 7 lists the quirks kept.
"""
import ctypes as C
import math

import torch
import torch.distributed as dist

from . import _abi
from ._abi import Ex4dDensifyApplyGroup, Ex4dGrowthAppend, Ex4dGrowthClassify, Ex4dGrowthTensor, ptr
from .densify import (DYNAMIC_NAMES, STATIC_NAMES, COUNT_NAMES, RULE_COPY, _apply, _broadcast, _desc, _opt_state, _prepare, _rebind,
                      _same_on_every_rank)

GROW_COPY, GROW_ZERO, GROW_XYZ, GROW_ROTATION, GROW_CENTER, GROW_VAR, GROW_STATS = range(7)
MAX_TENSORS = 28
SELECT_THETA, SELECT_MAX, SELECT_COUNT = 0, 1, 2
MIN_KEYFRAMES = 4          # the cubic keyframe interpolation reads four keyframes

_f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))     # a Python number as torch sets it against a float32 tensor
_NEW_ROW_RULES = {"_xyz_motion": GROW_XYZ, "_rotation_motion": GROW_ROTATION, "_opacity_duration_center": GROW_CENTER,
                  "_opacity_duration_var": GROW_VAR}
_STATIC_SOURCE = {"_opacity_motion": "_opacity", "_scaling_motion": "_scaling", "_features_dc_motion": "_features_dc",
                  "_features_rest_motion": "_features_rest"}


class ErrorTimestamps:
    """mark_error / get_errorneous_timestamp (:1299-1328): the summed loss and the count per keyframe interval; pop() returns the
    middle of the interval with the largest mean loss among those seen more than a tenth as often as the most frequent one SO FAR
    (the running maximum follows the dict's insertion order, as the reference's loop does), and forgets that interval.

    shared=True (several ranks, each marking the losses of its own views): mark() logs locally; sync() gathers the ranks' logs and
    replays them in (mark index, rank) order -- the i-th marks of ranks 0 .. W-1, then the (i+1)-th -- so every rank holds the dict,
    insertion order included, of one process that saw the views in that order.  pop() syncs first; both are collective calls.  A loss
    travels as a float64 (a Python float, or a tensor's item())."""

    def __init__(self, interval, shared=False, group=None):
        self.interval = interval
        self.errors = {}
        self.shared, self.group = bool(shared), group
        self._log = []

    def mark(self, loss, timestamp):
        if self.shared:
            self._log.append((float(loss), timestamp))
        else:
            self._apply(loss, timestamp)

    def _apply(self, loss, timestamp):
        idx = timestamp // self.interval
        total, count = self.errors.get(idx, (0, 0))
        self.errors[idx] = (total + loss, count + 1) if count else (loss, 1)

    def sync(self):
        if not self.shared:
            return
        logs = [self._log]
        if dist.is_initialized() and dist.get_world_size(self.group) > 1:
            logs = [None] * dist.get_world_size(self.group)
            dist.all_gather_object(logs, self._log, group=self.group)
        self._log = []
        for i in range(max(len(l) for l in logs)):
            for l in logs:
                if i < len(l):
                    self._apply(*l[i])

    def pop(self):
        self.sync()
        best_loss, best_idx, most = 0, 0, 0
        for idx, (total, count) in self.errors.items():
            most = max(most, count)
            if total / count > best_loss and count > most * 0.1:
                best_loss, best_idx = total / count, idx
        if best_loss == 0:
            return None
        del self.errors[best_idx]
        return (best_idx + 0.5) * self.interval


def first_keyframe_count(model, max_dur):
    """The keyframe count the first extraction gives an all-static model (:1166): ceil((max_dur + 2 time_shift + 1) / interval) + 3."""
    return math.ceil((max_dur + model.time_shift * 2 + 1) / model.interval) + 3


def quantile_threshold(score, percentile):
    """The radix select behind extract_dynamic_points on its own: score float32 [n] on the device, entries with a sign bit absent.
    Returns the device tensor [theta, max, count as int32 bits, 0] with theta = torch.quantile(s / (s.max() + 1e-6), percentile) bit
    for bit (NaN when a score is NaN or none is present).  No synchronisation."""
    if not score.is_cuda or score.dtype != torch.float32 or not score.is_contiguous() or score.dim() != 1:
        raise RuntimeError("quantile_threshold: a contiguous float32 vector on the device")
    result = torch.empty(4, dtype=torch.float32, device=score.device)
    scratch = torch.empty(int(_abi.load().ex4d_growth_select_scratch_bytes()), dtype=torch.uint8, device=score.device)
    with _abi.stream(score.device) as stream:
        _abi.call("ex4d_growth_select", ptr(score), score.numel(), float(percentile), result.data_ptr(), scratch.data_ptr(), stream)
    return result


def _classify(model, stats, cam, vis, percentile, motion_abs, min_abs):
    """scores -> threshold -> selected rows and the static prune's destination map.  Returns (map, plan counts, selected, counts_out,
    result), all on the device."""
    device = model._xyz.device
    ns = model.num_static
    lib = _abi.load()
    score = torch.empty(ns, dtype=torch.float32, device=device)
    result = torch.empty(4, dtype=torch.float32, device=device)
    sel_scratch = torch.empty(int(lib.ex4d_growth_select_scratch_bytes()), dtype=torch.uint8, device=device)
    g = Ex4dGrowthClassify()
    mp = torch.empty(max(ns, 1), 8, dtype=torch.int32, device=device)
    counts = torch.empty(8, dtype=torch.int32, device=device)
    selected = torch.empty(max(ns, 1), dtype=torch.int32, device=device)
    counts_out = torch.empty(2, dtype=torch.int32, device=device)
    scratch = torch.empty(max(int(lib.ex4d_densify_scratch_bytes(ns)), 1), dtype=torch.uint8, device=device)
    xyz, disp = model._xyz.detach(), model._xyz_disp.detach()
    g.n, g.score, g.result, g.disp, g.stats = ns, ptr(score), result.data_ptr(), ptr(disp), ptr(stats.static)
    g.motion_abs, g.min_abs = motion_abs, min_abs
    g.map, g.counts, g.selected, g.counts_out, g.scratch = mp.data_ptr(), counts.data_ptr(), selected.data_ptr(), counts_out.data_ptr(), scratch.data_ptr()
    with _abi.stream(device) as stream:
        _abi.call("ex4d_growth_scores", ptr(xyz), ptr(disp), ptr(vis), cam.data_ptr(), ns, ptr(score), stream)
        _abi.call("ex4d_growth_select", ptr(score), ns, percentile, result.data_ptr(), sel_scratch.data_ptr(), stream)
        _abi.call("ex4d_growth_classify", C.byref(g), stream)
    return mp, counts, selected, counts_out, result


def _append(descs, args, device):
    with _abi.stream(device) as stream:
        for i in range(0, len(descs), MAX_TENSORS):
            chunk = descs[i:i + MAX_TENSORS]
            _abi.call("ex4d_growth_append", (Ex4dGrowthTensor * len(chunk))(*chunk), len(chunk), C.byref(args), stream)


def extract_dynamic_points(model, stats, opt, viewpoint_loc, timestamp, vis_filter, extent, percentile=0.98, motion_thres=1000.0,
                           min_motion_thres=1e-6, max_dur=None, src=0):
    """CGaussianModel.extract_dynamic_points_from_static (:1147): the visible static rows whose normalised motion score is above its
    `percentile` quantile (or whose displacement is above motion_thres * extent), that move at all (min_motion_thres * extent) and
    have been seen (error-min timestamp >= 0) become dynamic rows, appended after the existing ones in ascending source order, and
    leave the static set.  `timestamp` is accepted and unused, as in the reference.  vis_filter: bool / uint8 [Ns] on the device.

    One read-back (the counts).  Returns {"static": counts, "dynamic": counts (keyed by densify.COUNT_NAMES; "clone" of the dynamic
    group counts the new rows), "threshold": the quantile as a float, "visible": the visible rows}.  With no visible row the reference
    raises inside max / quantile; here the call changes nothing and returns zero counts.  With visible rows and none selected the
    state keeps its values except the dynamic accumulators, which are reset as the reference resets them ("reset grad anyway");
    an all-static model stays as it is.
    Several ranks sharing `stats` (DensityStats(shared=True)): the statistics are merged first, and the camera position and the
    visibility filter are those of rank `src`, broadcast -- every rank extracts the same rows."""
    _prepare(opt, stats)
    device = model._xyz.device
    ns, nd = model.num_static, model.num_dynamic
    max_dur = model.duration if max_dur is None else max(float(max_dur), model.interval)
    if vis_filter.dtype == torch.bool:
        vis_filter = vis_filter.view(torch.uint8)
    if not vis_filter.is_cuda or vis_filter.dtype != torch.uint8 or not vis_filter.is_contiguous() or tuple(vis_filter.shape) != (ns,):
        raise RuntimeError("extract_dynamic_points: vis_filter must be a contiguous bool / uint8 [Ns] tensor on the device")
    cam = _broadcast(torch.as_tensor(viewpoint_loc, dtype=torch.float32).reshape(3).to(device).contiguous(), stats, src)
    vis_filter = _broadcast(vis_filter.clone(), stats, src) if getattr(stats, "shared", False) else vis_filter
    zero = {"static": dict(zip(COUNT_NAMES, [ns] + [0] * 6 + [ns])), "dynamic": dict(zip(COUNT_NAMES, [nd] + [0] * 6 + [nd])),
            "threshold": float("nan"), "visible": 0}
    if ns == 0:
        return zero
    mp, counts, selected, counts_out, result = _classify(model, stats, cam, vis_filter, _f32(percentile), _f32(motion_thres * extent),
                                                         _f32(min_motion_thres * extent))
    back = torch.tensor(_same_on_every_rank(torch.cat([counts_out, result.view(torch.int32)]), stats, "extract_dynamic_points"),
                        dtype=torch.int32)                                                 # the one read-back
    n_new, keep = int(back[0]), int(back[1])
    theta, visible = float(back[2:3].view(torch.float32)), int(back[2 + SELECT_COUNT])
    if visible == 0:
        return zero
    out = {"static": dict(zip(COUNT_NAMES, [keep] + [0] * 6 + [keep])), "dynamic": dict(zip(COUNT_NAMES, [nd, n_new] + [0] * 5 + [nd + n_new])),
           "threshold": theta, "visible": visible}
    if n_new == 0 and nd == 0:
        return out
    K = model._xyz_motion.shape[1] if nd > 0 else first_keyframe_count(model, max_dur)
    if K < MIN_KEYFRAMES:
        raise RuntimeError(f"extract_dynamic_points: {K} keyframes; the keyframe interpolation needs at least {MIN_KEYFRAMES}")
    names = {n: getattr(model, n) for n in STATIC_NAMES + DYNAMIC_NAMES}
    moments = _opt_state(opt, names)
    new_params, new_moments, descs_s, descs_d, hold = {}, {}, [], [], []

    # static side: the prune, through the density-control gather (a map in its layout, every tensor a copy)
    for n in STATIC_NAMES:
        src = names[n].detach()
        dst = torch.empty((keep,) + tuple(src.shape[1:]), dtype=src.dtype, device=device)
        descs_s.append(_desc(src, dst, ns, keep))
        new_params[n] = dst
        pair = []
        for m in moments[n] or ():
            md = torch.empty_like(dst)
            descs_s.append(_desc(m, md, ns, keep))
            pair.append(md)
        new_moments[n] = tuple(pair) if pair else None
    block_s = torch.empty(9, keep, dtype=torch.float32, device=device)
    descs_s.append(_desc(stats.static, block_s, ns, keep, RULE_COPY, 0, planes=9))

    # dynamic side: old rows copied, one new row per selected static row
    rows = nd + n_new
    shapes = {"_xyz_motion": (K, 3), "_rotation_motion": (K, 4)}
    for n in DYNAMIC_NAMES:
        old = names[n].detach()
        tail = shapes.get(n, tuple(old.shape[1:]) if nd > 0 else tuple(getattr(model, _STATIC_SOURCE[n]).shape[1:]) if n in _STATIC_SOURCE else (2, 1))
        dst = torch.empty((rows,) + tail, dtype=torch.float32, device=device)
        width = dst[0].numel() if rows else 1
        rule = _NEW_ROW_RULES.get(n, GROW_COPY)
        src0 = {GROW_XYZ: model._xyz, GROW_ROTATION: model._rotation, GROW_COPY: getattr(model, _STATIC_SOURCE.get(n, "_xyz"))}.get(rule)
        src1 = model._xyz_disp if rule == GROW_XYZ else None
        hold += [src0, src1]
        descs_d.append(Ex4dGrowthTensor(ptr(old) if nd else None, ptr(dst), ptr(src0.detach()) if src0 is not None else None,
                                        ptr(src1.detach()) if src1 is not None else None, nd, width, rule))
        new_params[n] = dst
        pair = []
        for m in moments[n] or ():
            md = torch.empty_like(dst)
            descs_d.append(Ex4dGrowthTensor(ptr(m) if nd else None, ptr(md), None, None, nd, width, GROW_ZERO))
            pair.append(md)
        new_moments[n] = tuple(pair) if pair else None
    block_d = torch.empty(9, rows, dtype=torch.float32, device=device)
    descs_d.append(Ex4dGrowthTensor(ptr(stats.dynamic) if nd else None, ptr(block_d), None, None, nd, 1, GROW_STATS))
    a = Ex4dGrowthAppend()
    a.selected, a.n_new, a.n_static, a.stats, a.K = selected.data_ptr(), n_new, ns, ptr(stats.static), K
    a.interval, a.max_dur, a.b_scale = _f32(model.interval), _f32(max_dur), _f32(1 + model.interval / max_dur)
    a.time_shift, a.time_pad = _f32(model.time_shift), _f32(model.time_pad)
    a.center_lo, a.center_hi = _f32((model.time_shift + 1) / model.interval), _f32((model.time_shift + max_dur - 1) / model.interval)
    _append(descs_d, a, device)                                # reads the static tensors: before they are replaced
    group = Ex4dDensifyApplyGroup()
    group.map = mp.data_ptr()
    group.split_div = 1.6
    _apply(descs_s, [group, Ex4dDensifyApplyGroup()], device)
    _rebind(model, opt, new_params, new_moments)
    stats._resized(block_s, block_d)
    return out


def _replace(model, opt, new_params):
    """replace_tensor_to_optimizer (:672-691): the tensors swapped in, both moments of each zeroed where it has state, step kept."""
    names = {n: getattr(model, n) for n in STATIC_NAMES + DYNAMIC_NAMES}
    moments = _opt_state(opt, names)
    for n, t in new_params.items():
        if moments[n] is not None:
            moments[n] = (torch.zeros_like(t), torch.zeros_like(t))
    _rebind(model, opt, new_params, moments)


def expand_duration(model, opt, duration):
    """CGaussianModel.expand_duration (:1243): the keyframe tracks lengthened to cover `duration` + 1 frames.  The new keyframes of
    _xyz_motion and _rotation_motion continue from the last one in steps of d, the mean over the last avg = min(K - 2, 4) keyframes
    of their offset from the keyframe before them (lin_interp_last: one subtrahend for all of them, as the reference slices it);
    _opacity_duration_var[:, 1] becomes 1 where a centre lies within half an interval of the new end, the centres are capped at the
    OLD end.  All four tensors get zeroed moments.  Returns whether anything was expanded; the three early-outs are the reference's."""
    duration = int(duration) + 1
    if duration <= model.duration:
        return False
    nd = model.num_dynamic
    if nd == 0:
        model.duration = duration
        return False
    K = model._xyz_motion.shape[1]
    K2 = math.ceil((duration + model.time_shift + model.time_pad * 2 + 1) / model.interval) + 3
    if K2 - K < 1:
        model.duration = duration
        return False
    _prepare(opt)
    device = model._xyz_motion.device
    avg = min(K - 2, 4)
    shift_i = model.time_shift / model.interval
    new = {}
    with _abi.stream(device) as stream:
        for n, c in (("_xyz_motion", 3), ("_rotation_motion", 4)):
            src = getattr(model, n).detach()
            new[n] = torch.empty(nd, K2, c, dtype=torch.float32, device=device)
            _abi.call("ex4d_growth_extrapolate", ptr(src), ptr(new[n]), nd, K, K2, c, avg, stream)
        center, var = model._opacity_duration_center.detach(), model._opacity_duration_var.detach()
        new["_opacity_duration_center"], new["_opacity_duration_var"] = torch.empty_like(center), torch.empty_like(var)
        _abi.call("ex4d_growth_expand_opacity", ptr(center), ptr(var), ptr(new["_opacity_duration_center"]), ptr(new["_opacity_duration_var"]), nd,
                  _f32(shift_i), _f32((duration + model.time_shift) / model.interval - 0.5),
                  _f32((model.time_shift + model.duration - 1) / model.interval), stream)
    model.duration = duration            # before the optimizer rebinds: a NativeTrainer reads the model's time constants when it does
    _replace(model, opt, new)
    if hasattr(model, "_drop_fused_cache"):
        model._drop_fused_cache()
    return True


def adjust_temp_opa(model, opt, max_dur=None):
    """CGaussianModel.adjust_temp_opa (:1330): the duration centres clamped 0.2 intervals inside [start, max_dur]; the log-width on the
    side where either centre of a row was outside becomes max(var, 1) * 2; wherever the OLD var is below 0.5 it becomes 0.5 instead.
    Both tensors get zeroed moments.  No dynamic rows: nothing happens."""
    max_dur = model.duration if max_dur is None else float(max_dur)
    nd = model.num_dynamic
    if nd == 0:
        return
    _prepare(opt)
    device = model._xyz_motion.device
    center, var = model._opacity_duration_center.detach(), model._opacity_duration_var.detach()
    new = {"_opacity_duration_center": torch.empty_like(center), "_opacity_duration_var": torch.empty_like(var)}
    with _abi.stream(device) as stream:
        _abi.call("ex4d_growth_adjust_opacity", ptr(center), ptr(var), ptr(new["_opacity_duration_center"]), ptr(new["_opacity_duration_var"]), nd,
                  _f32(model.time_shift / model.interval + 0.2), _f32((max_dur + model.time_shift) / model.interval - 0.2), stream)
    _replace(model, opt, new)
