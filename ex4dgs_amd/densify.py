"""Adaptive density control (include/ex4d_densify.h): the per-iteration densification statistics and densify_and_prune /
prune_invisible / prune_small / prune_nan_points of the reference's CGaussianModel (scene/c_gaussian_model.py:715-1145, :1229),
on the HIP library, with the matching edits of the optimizer state.

    stats = DensityStats(model)
    stats.update(radii, viewspace_points.grad, viewspace_l1points_grad_or_None, timestamp)     # every iteration: one launch
    densify_and_prune(model, stats, opt, max_grad, max_dgrad, 0.01, 0.01, extent, ...)         # every densification_interval

`opt` is a torch.optim.Optimizer over the reference's 15 groups (FusedRAdam or torch.optim.RAdam: state re-keyed to the new
parameter objects, `step` kept, moments gathered / zero for new rows), a trainer.FrameTrainer (m / v remapped, its buffers rebuilt,
the pending gradients dropped -- train.py densifies before optimizer.step(), whose replaced parameters have no .grad), a
native_trainer.NativeTrainer (its moments read out, a new native handle over the new tensors, moments and step count written back; run
the step before it with apply_optimizer=False), or None.
Random draws are inputs: by default torch.randn on the device (optionally from `generator`), in the reference's draw order; `noise`
hands in explicit draws.  No CPU fallback: everything runs on a ROCm device.

Several ranks (a FrameTrainer with exchange "allreduce" or "sharded", parameters replicated): DensityStats(model, shared=True) on every
rank; update() then accumulates the rank's own views, and every call here that changes the rows first merges the ranks' statistics
(DensityStats.sync), checks that the ranks planned the same counts and uses rank 0's draws -- every rank ends with the same bits.
"""
import ctypes as C

import torch
import torch.distributed as dist

from . import _abi
from ._abi import Ex4dDensifyApplyGroup, Ex4dDensifyPlanGroup, Ex4dDensifyTensor, ptr
from .attributes import PARAM_ORDER

EXPORTS = _abi.exports("ex4d_densify.h")

PRUNE_STATS, GRAD_STATS, L1_STATS = 1, 2, 4
PLAN_DENSIFY, PLAN_PRUNE_INVISIBLE, PLAN_PRUNE_SMALL, PLAN_PRUNE_NAN = 0, 1, 2, 3
RULE_COPY, RULE_ZERO_NEW, RULE_CONST_NEW, RULE_CHILD_SCALING, RULE_CHILD_XYZ, RULE_CENTER, RULE_STATS = range(7)
MAX_TENSORS = 24
MERGE_CHUNK, MERGE_MAX_BLOCKS = 1024, 1024      # DN_MERGE_CHUNK, DN_MERGE_MAX_BLOCKS of ex4d_densify.hip: Gaussians per workgroup and trip, grid cap
COUNT_NAMES = ("keep", "clone", "keep_clone", "split", "split_clone", "keep_child", "keep_child_clone", "rows")

STATIC_NAMES, DYNAMIC_NAMES = PARAM_ORDER[:7], PARAM_ORDER[7:]       # the static tensors come first
# rows of the [9, N] statistics block (EX4D_STAT_*) and the reference's attribute names for them
STAT_ROWS = ("gradient_accum", "denom", "error_accum", "ssim_error_accum", "error_denom", "max_radii2D", "min_radii2D", "error_min",
             "error_min_timestamp")
STAT_INIT = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1000.0, 1000.0, -1.0)
STATIC_STAT_NAMES = ("xyz_gradient_accum", "denom", "xyz_error_accum", "xyz_ssim_error_accum", "error_denom", "max_radii2D", "min_radii2D",
                     "xyz_error_min", "xyz_error_min_timestamp")
DYNAMIC_STAT_NAMES = ("motion_xyz_gradient_accum", "motion_denom", "motion_xyz_error_mean", "motion_xyz_ssim_error_accum", "motion_error_denom",
                      "motion_max_radii2D", "motion_min_radii2D", "motion_xyz_error_min", "motion_xyz_error_min_timestamp")
# [N] (radii) versus [N, 1] (everything else) views, as the reference allocates them (c_gaussian_model.py:408-428, :843-844)
_FLAT_STATS = ("max_radii2D", "min_radii2D")


def densify_thresholds(iteration, opt):
    """train.py:219-223: the (s_max_ssim, s_l1_thres, d_max_ssim, d_l1_thres) of the densify call at `iteration`.  opt: an object or
    mapping with densification_interval, error_base_prune_steps, ssim_prune_every, l1_prune_every, s_max_ssim, s_l1_thres, d_max_ssim,
    d_l1_thres (the reference's OptimizationParams)."""
    g = (lambda k: opt[k]) if isinstance(opt, dict) else (lambda k: getattr(opt, k))
    late = iteration > g("error_base_prune_steps")
    ssim_on = late and iteration % (g("densification_interval") * g("ssim_prune_every")) == 0
    l1_on = late and iteration % (g("densification_interval") * g("l1_prune_every")) == 0
    return (g("s_max_ssim") if ssim_on else 0, g("s_l1_thres") if l1_on else 100,
            g("d_max_ssim") if ssim_on else 0, g("d_l1_thres") if l1_on else 100)


class DensityStats:
    """The densification statistics of a scene.DynamicGaussians (c_gaussian_model.py:408-428 initial values): one [9, Ns] and one
    [9, Nd] float32 block; the reference-named attributes (xyz_gradient_accum, motion_min_radii2D, ...) are views of them.

    shared=True (several ranks, each seeing its own views): update() accumulates into a PENDING block per group that starts at
    STAT_INIT, and sync() all-gathers the ranks' pending blocks and folds them, in rank order, into `static` / `dynamic`
    (ex4d_densify_stats_merge) -- afterwards the totals are bit-identical on every rank and the pending blocks are at STAT_INIT again.
    The reference-named attributes read the totals: they are valid after sync().  densify_and_prune, the prunes and
    growth.extract_dynamic_points sync first, so a pending block is never remapped; after a resize it is fresh at the new size."""

    def __init__(self, model, device=None, shared=False, group=None):
        device = device or model._xyz.device
        self.shared, self.group = bool(shared), group
        self.static = self._fresh(model.num_static, device)
        self.dynamic = self._fresh(model.num_dynamic, device)
        self.pending_static = self._fresh(model.num_static, device) if self.shared else None
        self.pending_dynamic = self._fresh(model.num_dynamic, device) if self.shared else None

    @staticmethod
    def _fresh(n, device):
        return torch.tensor(STAT_INIT, dtype=torch.float32, device=device).view(9, 1).repeat(1, n).contiguous()

    def __getattr__(self, name):
        for names, key in ((STATIC_STAT_NAMES, "static"), (DYNAMIC_STAT_NAMES, "dynamic")):
            if name in names:
                row = self.__dict__[key][names.index(name)]
                return row if any(name.endswith(f) for f in _FLAT_STATS) else row.view(-1, 1)
        raise AttributeError(name)

    def update(self, radii, viewspace_grad, error_grad, timestamp, *, densify_stats=True, prune_stats=True, l1_accum=True):
        """One iteration of train.py:199-216: mark_prune_stats (when l1_accum and prune_stats) and, when densify_stats (iteration <
        densify_until_iter), max_radii2D + add_densification_stats + add_l1_ssim_stats (the latter when l1_accum).  radii int32 [P];
        viewspace_grad = dL/dmeans2D [P, 3]; error_grad = the (e0, e1, e2) hook gradient [P, 3] (None: no error statistics).
        shared: into the pending blocks."""
        ns, nd = self.static.shape[1], self.dynamic.shape[1]
        flags = (GRAD_STATS if densify_stats else 0) | (PRUNE_STATS if (prune_stats and l1_accum) else 0) | \
                (L1_STATS if (densify_stats and l1_accum) else 0)
        if error_grad is None:
            flags &= ~(PRUNE_STATS | L1_STATS)
        if ns + nd == 0 or flags == 0:
            return
        for t, w in ((radii, 1), (viewspace_grad, 3)) + (((error_grad, 3),) if error_grad is not None else ()):
            if not t.is_cuda or not t.is_contiguous() or t.shape[0] != ns + nd or (w > 1 and tuple(t.shape[1:]) != (w,)):
                raise RuntimeError("DensityStats.update: inputs must be contiguous device tensors with one row per Gaussian")
        if radii.dtype != torch.int32 or viewspace_grad.dtype != torch.float32 or (error_grad is not None and error_grad.dtype != torch.float32):
            raise RuntimeError("DensityStats.update: radii int32, gradients float32")
        blocks = (self.pending_static, self.pending_dynamic) if self.shared else (self.static, self.dynamic)
        with _abi.stream(radii.device) as stream:
            _abi.call("ex4d_densify_stats", ptr(blocks[0]), ns, ptr(blocks[1]), nd, radii.data_ptr(), viewspace_grad.data_ptr(),
                      ptr(error_grad), float(timestamp), flags, stream)

    def sync(self, group=None, force=False):
        """shared: folds every rank's pending blocks into the totals and resets them.  A collective call: every rank of the group makes
        it at the same point.  Per group of rows one all-gather of the [9, n] pending blocks (all_gather_into_tensor on RCCL, the list
        form on gloo) and one launch.  In a world of one no collective is issued -- the pending block alone is folded in -- unless
        `force` (or EX4D_FORCE_COLLECTIVES=1) asks for it: the one-rank collective and the kernel with W = 1, as several ranks run
        them.  Not shared: nothing to do."""
        if not self.shared:
            return
        from .dist import _backend, _forced
        group = self.group if group is None else group
        world = dist.get_world_size(group) if dist.is_initialized() else 1
        collective = dist.is_initialized() and (world > 1 or _forced(force))
        for total, pending in ((self.static, self.pending_static), (self.dynamic, self.pending_dynamic)):
            n = total.shape[1]
            if n == 0:
                continue
            if collective:
                gathered = torch.empty(world, 9, n, dtype=torch.float32, device=total.device)
                if _backend(group) == "nccl":
                    dist.all_gather_into_tensor(gathered, pending, group=group)
                else:
                    dist.all_gather([gathered[r] for r in range(world)], pending, group=group)
            else:
                gathered = pending.clone().view(1, 9, n)
            merge_stats(total, gathered, pending)

    def _resized(self, static, dynamic):
        """The blocks of a new row count (the pending ones were merged before the rows moved: fresh)."""
        self.static, self.dynamic = static, dynamic
        if self.shared:
            self.pending_static = self._fresh(static.shape[1], static.device)
            self.pending_dynamic = self._fresh(dynamic.shape[1], dynamic.device)


def merge_stats(total, pending, own=None):
    """ex4d_densify_stats_merge on tensors: total [9, n] takes the blocks pending [W, 9, n] in order; own [9, n] (optional) is reset to
    STAT_INIT.  Contiguous float32 device tensors; no synchronisation."""
    for t in (total, pending) + ((own,) if own is not None else ()):
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError("merge_stats: contiguous float32 tensors on the device")
    n = total.shape[-1]
    if tuple(total.shape) != (9, n) or pending.dim() != 3 or tuple(pending.shape[1:]) != (9, n) or (own is not None and tuple(own.shape) != (9, n)):
        raise RuntimeError("merge_stats: total [9, n], pending [W, 9, n], own [9, n]")
    with _abi.stream(total.device) as stream:
        _abi.call("ex4d_densify_stats_merge", ptr(total), ptr(pending), pending.shape[0], n, ptr(own), stream)


# ---------------------------------------------------------------------------------------------------- several ranks
def _rank_group(stats):
    """(group, world) when the statistics are shared among several ranks, else (None, 1)."""
    if getattr(stats, "shared", False) and dist.is_initialized():
        world = dist.get_world_size(stats.group)
        if world > 1:
            return stats.group, world
    return None, 1


def _same_on_every_rank(values, stats, what):
    """`values` (an integer device tensor, e.g. the plan counts) read back -- after ONE fixed-size collective, the minimum over the
    ranks of (values, -values), when several ranks share the statistics: a rank whose replica planned different counts would size
    its tensors and the following collectives differently.  Every rank raises the same RuntimeError then."""
    group, world = _rank_group(stats)
    if world == 1:
        return values.cpu().tolist()
    v = values.reshape(-1).to(torch.int64)
    both = torch.cat([v, -v])
    dist.all_reduce(both, op=dist.ReduceOp.MIN, group=group)
    both = both.cpu()
    lo, hi = both[:v.numel()], -both[v.numel():]
    if not torch.equal(lo, hi):
        raise RuntimeError(f"{what}: the ranks' replicas disagree (minimum over ranks {lo.tolist()}, maximum {hi.tolist()}): "
                           "their parameters or statistics are no longer identical")
    return lo.to(values.dtype).view(values.shape).tolist()


def _broadcast(t, stats, src=0):
    group, world = _rank_group(stats)
    if world > 1:
        dist.broadcast(t, src=dist.get_global_rank(group, src) if group is not None else src, group=group)
    return t


# ---------------------------------------------------------------------------------------------------- optimizer adapters
def _opt_state(opt, params):
    """{name: (exp_avg, exp_avg_sq) or None} of the optimizer for the current parameter objects."""
    from .native_trainer import NativeTrainer
    from .trainer import FrameTrainer
    if opt is None:
        return {n: None for n in params}
    if isinstance(opt, NativeTrainer):
        state = opt._moments if opt._moments is not None else opt.begin_density_control()
        return {n: state[n] for n in params}
    if isinstance(opt, FrameTrainer):
        if not getattr(opt, "optimizer", False):
            return {n: None for n in params}
        idx = {n: i for i, n in enumerate(opt.names)}
        if opt.mode == "sharded":                  # the owned ranges move with the rows: the moments whole, gathered from their owners
            full = opt.opt.full_moments()
            return {n: full[idx[n]] for n in params}
        return {n: (opt.m[idx[n]], opt.v[idx[n]]) for n in params}
    out = {}
    for n, p in params.items():
        st = opt.state.get(p, None)
        out[n] = (st["exp_avg"], st["exp_avg_sq"]) if st and "exp_avg" in st else None
    return out


def _rebind(model, opt, new_params, new_moments):
    from .native_trainer import NativeTrainer
    from .trainer import FrameTrainer
    old = {n: getattr(model, n) for n in new_params}
    fresh = {}
    for n, t in new_params.items():
        o = old[n]
        p = torch.nn.Parameter(t, requires_grad=o.requires_grad) if isinstance(o, torch.nn.Parameter) else t.requires_grad_(o.requires_grad)
        fresh[n] = p
        setattr(model, n, p)
    if hasattr(model, "_drop_fused_cache"):
        model._drop_fused_cache()
    if opt is None:
        return
    if isinstance(opt, (FrameTrainer, NativeTrainer)):
        opt.rebind_parameters(new_moments)
        return
    for group in opt.param_groups:
        for k, p in enumerate(group["params"]):
            name = next((n for n, o in old.items() if o is p), None)
            if name is None:
                continue
            st = opt.state.pop(p, None)
            group["params"][k] = fresh[name]
            if st is not None:
                if new_moments.get(name) is not None:
                    st["exp_avg"], st["exp_avg_sq"] = new_moments[name]
                opt.state[fresh[name]] = st


def _prepare(opt, stats=None):
    from .native_trainer import NativeTrainer
    from .trainer import FrameTrainer
    if isinstance(opt, FrameTrainer) and opt.mode != "none" and opt.world > 1 and stats is not None and not getattr(stats, "shared", False):
        raise RuntimeError("density control on a multi-rank FrameTrainer needs DensityStats(model, shared=True): every rank would decide on the "
                           "statistics of its own views and the replicas would part")
    if isinstance(opt, (FrameTrainer, NativeTrainer)):
        opt.begin_density_control()
    if stats is not None:
        stats.sync()                               # shared statistics: the decision below reads the merged totals, on every rank the same


# ---------------------------------------------------------------------------------------------------- plan + apply
def _plan(mode, stats_block, n, device, scaling=None, opacity=None, xyz=None, thr=None):
    g = Ex4dDensifyPlanGroup()
    g.n = n
    mp = torch.empty(max(n, 1), 8, dtype=torch.int32, device=device)
    counts = torch.zeros(8, dtype=torch.int32, device=device)
    scratch = torch.empty(max(int(_abi.load().ex4d_densify_scratch_bytes(n)), 1), dtype=torch.uint8, device=device)
    g.stats, g.map, g.counts, g.scratch = ptr(stats_block), mp.data_ptr(), counts.data_ptr(), scratch.data_ptr()
    if scaling is not None:
        g.scaling, g.opacity = ptr(scaling), ptr(opacity)
    if xyz is not None:
        g.xyz, g.xyz_width = ptr(xyz), (xyz[0].numel() if n else 1)
    for k, v in (thr or {}).items():
        setattr(g, k, v)
    with _abi.stream(device) as stream:
        _abi.call("ex4d_densify_plan", mode, C.byref(g), stream)
    return mp, counts, scratch


def _apply(descs, groups, device):
    garr = (Ex4dDensifyApplyGroup * 2)(*groups)
    with _abi.stream(device) as stream:
        for i in range(0, len(descs), MAX_TENSORS):
            chunk = descs[i:i + MAX_TENSORS]
            _abi.call("ex4d_densify_apply", (Ex4dDensifyTensor * len(chunk))(*chunk), len(chunk), garr, stream)


def _desc(src, dst, rows, dst_rows, rule=RULE_COPY, group=0, planes=1, aux0=None, aux1=None, value=0.0):
    width = src.numel() // max(rows * planes, 1) if rows else 1
    return Ex4dDensifyTensor(ptr(src), ptr(dst), rows, dst_rows, width, planes, rule, group, ptr(aux0), ptr(aux1), float(value), 0)


def _gather(model, stats, opt, plans, counts, rules, groups, names_by_group):
    """Allocates every new tensor, runs the multi-tensor gather, swaps the tensors into model / stats / optimizer."""
    device = model._xyz.device
    moments = _opt_state(opt, {n: getattr(model, n) for g in names_by_group for n in g})
    descs, new_params, new_moments, keep = [], {}, {}, []
    new_blocks = [stats.static, stats.dynamic]
    for gi, names in enumerate(names_by_group):
        rows_src = (model.num_static, model.num_dynamic)[gi]
        rows_dst = int(counts[gi][7])
        for n in names:
            src = getattr(model, n).detach()
            dst = torch.empty((rows_dst,) + tuple(src.shape[1:]), dtype=src.dtype, device=device)
            rule, aux0, aux1, value = rules.get(n, (RULE_COPY, None, None, 0.0))
            descs.append(_desc(src, dst, rows_src, rows_dst, rule, gi, 1, aux0, aux1, value))
            new_params[n] = dst
            mom = moments.get(n)
            if mom is not None:
                pair = []
                for m in mom:
                    md = torch.empty_like(dst)
                    descs.append(_desc(m, md, rows_src, rows_dst, RULE_ZERO_NEW if rules else RULE_COPY, gi))
                    pair.append(md)
                new_moments[n] = tuple(pair)
            else:
                new_moments[n] = None
        blk = (stats.static, stats.dynamic)[gi]
        nb = torch.empty(9, rows_dst, dtype=torch.float32, device=device)
        descs.append(_desc(blk, nb, rows_src, rows_dst, RULE_STATS if rules else RULE_COPY, gi, planes=9))
        new_blocks[gi] = nb
        keep.append(blk)
    _apply(descs, groups, device)
    _rebind(model, opt, new_params, new_moments)
    stats._resized(*new_blocks)


def _groups(plans, counts, noise=None, model=None):
    out = []
    for gi in range(2):
        g = Ex4dDensifyApplyGroup()
        if plans[gi] is not None:
            g.map = plans[gi][0].data_ptr()
            c = counts[gi]
            g.child_stride = int(c[5] + c[6])
            g.n_split = int(c[3] + c[4])
        g.split_div = 1.6
        if model is not None:
            g.min_len = 2 / model.interval
            g.center_lo = (model.time_shift + 1) / model.interval
            g.center_hi = (model.time_shift + model.duration - 1) / model.interval
        if noise is not None:
            for k in ("split_z", "split_c1", "split_c0", "clone_c1", "clone_c0"):
                t = noise[gi].get(k)
                # an empty draw tensor is never read (its count is 0): a valid one-element stand-in keeps the pointer checks simple
                setattr(g, k, ptr(t) if t is not None and t.numel() else ptr(_dummy(plans[0][0].device)))
        out.append(g)
    return out


_DUMMY = {}


def _dummy(device):
    if device not in _DUMMY:
        _DUMMY[device] = torch.zeros(4, device=device)
    return _DUMMY[device]


def _draws(counts, has_dynamic, device, generator=None, noise=None, stats=None):
    """The standard-normal draws of one densify call, in the reference's order: clone centre jitter (c1, c0) of the dynamic rows,
    static split samples, dynamic split samples, their centre jitter (c1, c0).  `noise` (a dict with the keys of the returned one)
    overrides; its shapes are checked against the counts.  Several ranks sharing `stats`: rank 0 draws (its `noise` and `generator`
    count), the others receive its draws in one broadcast."""
    nc_d = int(counts[1][1])
    ns_s, ns_d = int(counts[0][3] + counts[0][4]), int(counts[1][3] + counts[1][4])
    shapes = {"clone_c1": (nc_d,), "clone_c0": (nc_d,), "static_split_z": (2 * ns_s, 3), "split_z": (2 * ns_d, 3),
              "split_c1": (2 * ns_d,), "split_c0": (2 * ns_d,)}
    order = ("clone_c1", "clone_c0", "static_split_z", "split_z", "split_c1", "split_c0") if has_dynamic else ("static_split_z",)
    out = {}
    group, world = _rank_group(stats)
    drawing = world == 1 or dist.get_rank(group) == 0
    for k in order:
        if not drawing:
            t = torch.empty(shapes[k], dtype=torch.float32, device=device)
        elif noise is not None and k in noise:
            t = noise[k].to(device=device, dtype=torch.float32).contiguous().reshape(shapes[k])
        else:
            t = torch.randn(shapes[k], device=device, generator=generator)
        out[k] = t
    if world > 1:
        flat = _broadcast(torch.cat([out[k].reshape(-1) for k in order]), stats)
        off = 0
        for k in order:
            out[k] = flat[off:off + out[k].numel()].view(shapes[k]).clone()
            off += out[k].numel()
    for k in shapes:
        out.setdefault(k, torch.zeros(shapes[k], device=device))
    return out


def densify_and_prune(model, stats, opt, max_grad, max_dgrad, min_opacity, min_motion_opacity, extent, max_screen_size=None,
                      max_dynamic_screen_size=None, s_max_ssim=0.5, s_l1_thres=0.1, d_max_ssim=0.5, d_l1_thres=0.1, percent_dense=0.01,
                      generator=None, noise=None):
    """CGaussianModel.densify_and_prune (:1019): clone, split, postfix resets, prune -- one plan per group, ONE read-back of the
    counts, one multi-tensor gather.  Returns {"static": counts, "dynamic": counts, "draws": the draws used} with counts keyed by
    COUNT_NAMES.  Nd == 0: the dynamic state is left untouched (densification_postfix_onlystatic)."""
    _prepare(opt, stats)
    device = model._xyz.device
    ns, nd = model.num_static, model.num_dynamic
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))
    common = dict(dense_scale=f32(percent_dense * extent), big_scale=f32(0.1 * extent))
    thr_s = dict(common, grad_thr=f32(max_grad), use_screen=int(bool(max_screen_size)), screen_size=f32(max_screen_size or 0),
                 min_opacity=f32(min_opacity), l1_thres=f32(s_l1_thres), max_ssim=f32(s_max_ssim))
    thr_d = dict(common, grad_thr=f32(max_dgrad), use_screen=int(bool(max_dynamic_screen_size)), screen_size=f32(max_dynamic_screen_size or 0),
                 min_opacity=f32(min_motion_opacity), l1_thres=f32(d_l1_thres), max_ssim=f32(d_max_ssim))
    plans = [_plan(PLAN_DENSIFY, stats.static, ns, device, model._scaling.detach(), model._opacity.detach(), thr=thr_s),
             _plan(PLAN_DENSIFY, stats.dynamic, nd, device, model._scaling_motion.detach(), model._opacity_motion.detach(), thr=thr_d)
             if nd > 0 else None]
    counts = _same_on_every_rank(torch.stack([plans[0][1], plans[1][1] if plans[1] is not None else torch.zeros_like(plans[0][1])]),
                                 stats, "densify_and_prune")                                 # the one read-back
    draws = _draws(counts, nd > 0, device, generator, noise, stats)
    noise_g = [{"split_z": draws["static_split_z"]},
               {k: draws[k] for k in ("split_z", "split_c1", "split_c0", "clone_c1", "clone_c0")}]
    groups = _groups(plans, counts, noise_g, model)
    rules = {"_xyz": (RULE_CHILD_XYZ, model._rotation.detach(), model._scaling.detach(), 1.0),
             "_scaling": (RULE_CHILD_SCALING, None, None, 0.0),
             "_xyz_motion": (RULE_CHILD_XYZ, model._rotation_motion.detach(), model._scaling_motion.detach(), 2.0),
             "_scaling_motion": (RULE_CHILD_SCALING, None, None, 0.0),
             "_opacity_duration_center": (RULE_CENTER, None, None, 0.0),
             "_opacity_duration_var": (RULE_CONST_NEW, None, None, 2.0)}
    names = [STATIC_NAMES, DYNAMIC_NAMES if nd > 0 else ()]
    _gather(model, stats, opt, plans, counts, rules, groups, names)
    return {"static": dict(zip(COUNT_NAMES, counts[0])), "dynamic": dict(zip(COUNT_NAMES, counts[1])), "draws": draws}


def _prune(mode, model, stats, opt):
    _prepare(opt, stats)
    device = model._xyz.device
    ns, nd = model.num_static, model.num_dynamic
    plans = [_plan(mode, stats.static, ns, device, xyz=model._xyz.detach()),
             _plan(mode, stats.dynamic, nd, device, xyz=model._xyz_motion.detach()) if nd > 0 else None]
    counts = _same_on_every_rank(torch.stack([plans[0][1], plans[1][1] if plans[1] is not None else torch.zeros_like(plans[0][1])]),
                                 stats, "prune")
    groups = _groups(plans, counts)
    # prune_points returns before the dynamic half when it is empty (c_gaussian_model.py:737-738)
    _gather(model, stats, opt, plans, counts, {}, groups, [STATIC_NAMES, DYNAMIC_NAMES if nd > 0 else ()])
    return {"static": dict(zip(COUNT_NAMES, counts[0])), "dynamic": dict(zip(COUNT_NAMES, counts[1]))}


def prune_invisible(model, stats, opt):
    """:1074: static and dynamic rows whose error-min timestamp is < 0 (the duration test at :1078-1081 is computed and discarded)."""
    return _prune(PLAN_PRUNE_INVISIBLE, model, stats, opt)


def prune_small(model, stats, opt):
    """:1087: rows whose min_radii2D is < 5."""
    return _prune(PLAN_PRUNE_SMALL, model, stats, opt)


def prune_nan_points(model, stats, opt):
    """:1229: rows with a NaN in _xyz, or anywhere in the K keyframes of _xyz_motion."""
    return _prune(PLAN_PRUNE_NAN, model, stats, opt)
