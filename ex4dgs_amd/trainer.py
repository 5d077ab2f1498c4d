"""One training-iteration core per rank, built from the fused pieces of this package:

    fused attribute evaluation (attributes.forward_raw)            scene/c_gaussian_model.py:170-215,330-375 getters
 -> rasterizer forward + backward (GaussianRasterizer, SplitSH)    gaussian_renderer/__init__.py:19-124, train.py:139-153
 -> fused attribute backward into persistent gradient buffers      (autograd of the getters in the reference)
 -> sum of the 15 model-parameter gradients over the ranks         (the reference is single-process)
 -> optimizer step: replicated fused RAdam or the sharded one      scene/c_gaussian_model.py:430-449, train.py:250

One view (camera, timestamp) per rank per step: views shard round-robin (dist.shard_views), parameters are replicated.  The
attribute backward and the gradient exchange of frame i run on a side stream / the communicator's stream: the four feature gradients
(3/4 of the bytes) go on the wire before the attribute backward starts.  Without an optimizer the whole exchange hides behind the
rasterization of frame i+1; with one (the default of the multi-GPU bench) it has to finish before the optimizer step at the top of step
i+1 and is exposed except for the part beside the attribute backward.
No CPU fallback: everything here needs the HIP library and a ROCm device.
"""
import contextlib
import math

import torch
import torch.distributed as dist

from . import attributes as attr
from . import dist as xdist
from ._C import SplitSH
from .diff_gaussian_rasterization_df import GaussianRasterizationSettings, rasterize_gaussians

def reference_lrs(spatial_lr_scale=1.0):
    """The 15 optimizer groups of CGaussianModel.training_setup (scene/c_gaussian_model.py:430-447) with the default OptimizationParams
    (arguments/__init__.py:93-110); the two position groups carry the initial value of their exponential schedule times
    spatial_lr_scale.  Pinned by tests/golden/training_args.json (captured from the imported reference)."""
    return {"_xyz": 0.00016 * spatial_lr_scale, "_features_dc": 0.0025, "_features_rest": 0.0025 / 20.0, "_opacity": 0.05, "_scaling": 0.005,
            "_rotation": 0.00001, "_xyz_disp": 0.0001,
            "_xyz_motion": 0.00016 * spatial_lr_scale, "_features_dc_motion": 0.0025, "_features_rest_motion": 0.0025 / 20.0,
            "_scaling_motion": 0.005, "_opacity_motion": 0.05, "_opacity_duration_center": 0.001, "_opacity_duration_var": 0.0005,
            "_rotation_motion": 0.001}


# reference group name (c_gaussian_model.py:430-447) -> parameter attribute
REFERENCE_GROUP_NAMES = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
                         "rotation": "_rotation", "xyz_disp": "_xyz_disp", "motion_xyz": "_xyz_motion", "motion_f_dc": "_features_dc_motion",
                         "motion_f_rest": "_features_rest_motion", "motion_scaling": "_scaling_motion", "motion_opacity": "_opacity_motion",
                         "motion_opacity_center": "_opacity_duration_center", "motion_opacity_var": "_opacity_duration_var",
                         "motion_rotation": "_rotation_motion"}
DEFAULT_LRS = reference_lrs(1.0)
# parameters whose gradient the reference passes through nan_to_num before optimizer.step() (train.py:244-247)
NAN_TO_NUM = ("_opacity_duration_var",)


class FrameTrainer:
    """model: scene.DynamicGaussians on a ROCm device.  exchange: "none" | "allreduce" | "sharded" (reduce-scatter + sharded RAdam +
    all-gather; implies optimizer).  optimizer: False | True (replicated fused RAdam when exchange != "sharded")."""

    def __init__(self, model, exchange="none", optimizer=False, lrs=None, overlap=True, group=None, sliced=None, spatial_lr_scale=1.0,
                 force_collectives=False, async_forward=None, views_per_step=1, regularizers=None):
        """lrs: overrides of the reference table reference_lrs(spatial_lr_scale).
        sliced (default: on whenever an optimizer runs, replicated or sharded): the keyframe gradients stay [Nd,4,3] / [Nd,2,4] slices from
        the attribute backward through the exchange into ex4d_radam_step_sliced -- no 196 MB zero fill, no dense read.  Replicated
        optimizer: all-gather of the ranks' windows (16 MB per rank sent instead of 196); sharded optimizer: the keyframe tensors are
        sharded by rows and one all-to-all hands every owner the rows of every rank's window (dist.SliceRowExchange: 14 MB sent per rank
        at 8 ranks).
        force_collectives: issue the exchange's collectives even in a process group of one rank (dist.py: the RCCL-native branches
        run and are checked on a one-GPU box).
        async_forward (default: off since round 6 -- with the synchronous forward's read-back off the caller's stream the two are equal at 1.0 M Gaussians
        and the synchronous one is 8 % faster at 100 k (bench.py --train-core [--sync-forward]); round 5: on for a single rank with exchange "none"): the rasterizer forward runs asynchronously (no instance-count read-back:
        include/ex4d_rasterizer.h Ex4dParams.instance_capacity, under an AsyncFrames policy of the trainer's own); the frame's status is looked at once, right before its gradients are applied, and a frame that overflowed its
        capacity is RE-RUN first -- the parameters are those of the synchronous path.  `replays` counts such re-runs.
        views_per_step = k > 1 (round 6): a rank renders k views per optimizer step; their gradients are added up locally (persistent
        accumulators), exchanged ONCE after the k-th view and applied once -- the batch of a step is N k views, the wire time per view
        1/k of the single-view step's (DESIGN.md section 6 has the projected efficiencies).  Keyframe gradients are dense in this mode (k
        views touch k windows; the sliced optimizer takes one window per rank), the forward is synchronous.
        regularizers (default None: off): the weights (static_reg, motion_reg, rot_reg) of the reference's motion regularisers
        (train.py:155-168) as a 3-tuple, or a callable returning them, asked once per frame -- e.g.
        lambda: regularizers.regularizer_weights(opt, iteration, Nd).  Their gradients join the frame's in the optimizer step: with sliced
        keyframe gradients the two keyframe terms are formed inside ex4d_radam_step_sliced_reg from the rows it updates (no dense
        gradient), _xyz_disp's term is added to its gradient buffer; with dense keyframe gradients all three are added once per optimizer
        step.  last["reg"]: float32[4] on the device = (static, motion, rot mean, weighted sum) at the frame's parameters.
        With an exchange the terms are added once per optimizer step, last, to the gradient summed over ranks and views -- after the
        exchange, never before it: "allreduce" adds them to the reduced buffers / forms them in the fused step over the gathered windows,
        "sharded" hands them to ShardedRAdam.step(reg=...), whose owners add them to their element ranges or rows.  Every rank ends a step
        with the bits of a single-process step fed the reduced gradient.  The weights must be equal on all ranks (nothing checks it;
        regularizer_weights depends on replicated values only), and regularizer_weights(..., views=N k) restores the reference's one term
        per view.  exchange="allreduce" without a process group of several ranks (and without force_collectives) would train with no
        exchange at all: with regularizers that request is still refused (NotImplementedError); ask for exchange="none"."""
        assert exchange in ("none", "allreduce", "sharded")
        self._exchange_asked = exchange
        self.k = int(views_per_step)
        assert self.k >= 1
        if self.k > 1:
            if sliced:
                raise ValueError("views_per_step > 1 accumulates dense keyframe gradients (one gradient window per view and rank): sliced=True does not apply")
            if async_forward:
                raise ValueError("views_per_step > 1 runs the synchronous forward (a re-run frame would be accumulated twice)")
            sliced, async_forward = False, False
        self._acc, self._nacc = None, 0
        self.model = model
        self.regularizers = regularizers
        self._reg_w = self._reg_out = self._reg_scratch = None
        if regularizers is not None:
            if not optimizer:
                raise ValueError("regularizers join the gradients inside the optimizer step: optimizer=True")
            if model.num_dynamic > 0 and self.k == 1:
                from .optim import sliced_reg_rows
                K = model._xyz_motion.shape[1]
                if min(sliced_reg_rows(K, 3), sliced_reg_rows(K, 4)) == 0:     # K too large for the fused step's row staging: dense keyframe gradients
                    if sliced:
                        raise ValueError(f"regularizers with sliced keyframe gradients: K = {K} keyframes do not fit the fused step (sliced=False works)")
                    sliced = False
        self.names = list(attr.PARAM_ORDER)
        self.params = [getattr(model, n) for n in self.names]
        self.device = self.params[0].device
        if self.device.type != "cuda":
            raise RuntimeError("FrameTrainer needs the model on a ROCm device (no CPU fallback)")
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        force = xdist._forced(force_collectives) and dist.is_initialized()
        self.mode = exchange if (self.world > 1 or exchange == "sharded" or force) else "none"
        if regularizers is not None and self.mode != exchange:
            # the part of the former refusal that stays: an exchange was asked for and none takes place (no process group of several
            # ranks, no force_collectives), so weights scaled for N ranks (regularizer_weights(views=)) would act on one rank's gradient
            raise NotImplementedError(f"regularizers on a FrameTrainer with exchange='{exchange}' need a process group of several ranks "
                                      "(or force_collectives): no exchange would take place; ask for exchange='none'")
        self.overlap = overlap
        self.side = torch.cuda.Stream(device=self.device) if overlap else None
        self._group, self._force = group, force
        self.feature_idx = [self.names.index(n) for n in attr.FEATURE_NAMES]
        lrs = dict(reference_lrs(spatial_lr_scale), **(lrs or {}))
        self.lrs = [lrs[n] for n in self.names]
        self.opt = None
        # one gradient window per rank reaches ex4d_radam_step_sliced: more ranks than it takes windows -> dense keyframe gradients
        from .optim import MAX_WINDOWS
        gather_world = self.world if self.mode in ("allreduce", "sharded") else 1      # exchange "none": nothing is summed over ranks, keyframes included
        fits = gather_world <= MAX_WINDOWS
        has_opt = bool(optimizer) or self.mode == "sharded"
        self.sliced = (has_opt and model.num_dynamic > 0 and fits) if sliced is None else bool(sliced)
        if self.sliced and not has_opt:
            raise ValueError("sliced keyframe gradients need an optimizer in the step (plain gradient output is dense)")
        if self.sliced and not fits:
            raise ValueError(f"sliced keyframe gradients take one window per rank, at most {MAX_WINDOWS}")
        # the model's position interpolator sizes the keyframe window: 2 slices under 'linear', 4 under 'cube' and 'pchip'
        self.interp_type = getattr(model, "interp_type", "cube")
        self.sliced_shapes = attr.sliced_shapes(self.interp_type)
        self.kf_idx = [self.names.index(n) for n in self.sliced_shapes] if self.sliced else []
        self._make_grad_buffers()
        # two exchanges: the four feature gradients (3/4 of the bytes) leave the rasterizer backward and are on the wire while the
        # attribute backward still runs; the other parameters follow it
        self.feat_pos = [i for i in self.feature_idx]
        self.rest_pos = [i for i in range(len(self.params)) if i not in self.kf_idx and i not in self.feature_idx]
        self._make_exchanges()
        if self.mode != "sharded" and optimizer:
            self.m = [torch.zeros_like(p) for p in self.params]
            self.v = [torch.zeros_like(p) for p in self.params]
            self.steps = 0
        self.optimizer = bool(optimizer) or self.mode == "sharded"
        # (round 5 made the non-blocking forward the default wherever the class can recover from an overflow by itself; round 6 measured the
        # synchronous forward -- its read-back off the caller's stream now -- equal or faster, and it needs no capacity policy: opt-in again)
        self.async_forward = False if async_forward is None else bool(async_forward)
        self.replays = 0
        self._frame = self._last_args = None
        self._flow = None
        if self.async_forward:
            if self.mode != "none":
                raise ValueError("async_forward re-runs an overflowing frame on its own: single rank, exchange 'none' only")
            from .diff_gaussian_rasterization_df import AsyncFrames
            self._policy = AsyncFrames().enable(headroom=1.25, strict=False)     # this trainer's own: other callers stay synchronous
        self._grads = None
        self._zero_sub = {}
        self.last = {}

    # ------------------------------------------------------------------------------------------
    def _make_grad_buffers(self):
        """The buffers sized by the parameters' rows: pgrad, the persistent gradient buffers of the 11 non-feature parameters (written
        once per step by the attribute backward; the four feature gradients come out of the rasterizer's SplitSH path as fresh tensors
        every step), and kf_gather, the window gathers of the sliced keyframe tensors."""
        self.pgrad = [None if i in self.feature_idx else torch.zeros_like(p) for i, p in enumerate(self.params)]
        self.kf_gather = []
        for i in self.kf_idx:
            shape = (self.params[i].shape[0],) + self.sliced_shapes[self.names[i]]
            self.pgrad[i] = torch.zeros(shape, dtype=torch.float32, device=self.device)
            if self.mode != "sharded":      # replicated optimizer: every rank needs every window (all-gather); sharded: row all-to-all inside ShardedRAdam
                self.kf_gather.append(xdist.SliceGather(shape, self.device, group=self._group, local_only=(self.mode != "allreduce"), force=self._force))

    def _make_exchanges(self):
        """The collectives sized by the parameters: the two gradient exchanges of the replicated modes, or the sharded optimizer with
        its reduce-scatter (a rebuilt one takes over the step counts; its moments are loaded by the caller)."""
        self.exchange_feat = self.exchange = None
        if self.mode == "sharded":
            old = self.opt
            self.opt = xdist.ShardedRAdam(self.params, self.lrs, group=self._group, nan_to_num=[n in NAN_TO_NUM for n in self.names], force=self._force,
                                          sliced={i: self.sliced_shapes[self.names[i]][0] for i in self.kf_idx})
            if old is not None:
                self.opt.steps = list(old.steps)
            self.exchange = self.opt.exchange
        elif self.mode == "allreduce":
            shapes = lambda pos: [self.params[i].shape for i in pos]
            self.exchange_feat = xdist.ParamGradExchange(shapes(self.feat_pos), self.device, mode="allreduce", group=self._group, force=self._force)
            self.exchange = xdist.ParamGradExchange(shapes(self.rest_pos), self.device, mode="allreduce", group=self._group, force=self._force)

    def _settings(self, cam, bg, near, far):
        H, W = int(cam.image_height), int(cam.image_width)
        key = (H, W)
        if key not in self._zero_sub:
            self._zero_sub[key] = torch.zeros(H, W, 2, device=self.device)
        m = self.model
        return GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5), kernel_size=m.kernel_size,
            subpixel_offset=self._zero_sub[key], bg=bg, scale_modifier=1.0, viewmatrix=cam.world_view_transform,
            projmatrix=cam.full_proj_transform, sh_degree=m.active_sh_degree, campos=cam.camera_center, prefiltered=False,
            min_depth=near, max_depth=far, debug=False)

    def finish_exchange(self):
        """Block the current stream on the pending gradient exchange (its results are needed by the optimizer / the caller)."""
        def wait_all():
            if self.exchange_feat is not None:
                self.exchange_feat.wait()
            if self.exchange is not None:
                self.exchange.wait()
            for gth in self.kf_gather:
                gth.wait()
            if self.mode == "sharded":
                for ex in self.opt.row_exchange.values():
                    ex.wait()
        if self.exchange is not None or self.kf_gather:
            if self.side is not None:
                with torch.cuda.stream(self.side):
                    wait_all()
                torch.cuda.current_stream(self.device).wait_stream(self.side)
            else:
                wait_all()

    def exchange_bytes_on_wire(self):
        """Payload bytes one rank contributes to one step's gradient exchange (all collectives of the step)."""
        n = 0
        for ex in (self.exchange_feat, self.exchange):
            if ex is not None:
                n += ex.bytes_on_wire()
        if self.world > 1:
            n += sum(g.bytes_on_wire() for g in self.kf_gather if not g.local_only)
            if self.mode == "sharded":
                n += sum(ex.bytes_on_wire() for ex in self.opt.row_exchange.values())
        return n

    def step(self, cam, bg, t, upstream, near=0.2, far=300.0, flow_to=None):
        """upstream: callable(render dict) -> (list of outputs, list of their gradients), e.g. a loss evaluated with the fused
        L1+SSIM op, or fixed synthetic gradients.  Returns the render dict (tensors of this frame, detached).
        flow_to (default None: a zero dir3D, the step as it always was): a timestamp makes dir3D the screen displacement of every
        Gaussian from t to flow_to for this camera and `near` (motion.displacement_raw), so out["opticalflow"] is the rendered motion in
        pixels and an upstream loss on it (flow.flow_loss) trains `_xyz`, `_xyz_disp` and `_xyz_motion`: dir3D's gradient goes through
        motion.displacement_backward_raw, its two static gradients are added to the attribute backward's, and `_xyz_motion` takes
        three gradient windows in the order attribute window, motion window 0, motion window 1 -- handed to ex4d_radam_step_sliced as
        they are, or added into the dense gradient in that order.  One rank, one view per step: exchange "none" only."""
        if flow_to is not None:
            if self._exchange_asked != "none":
                raise NotImplementedError(f"flow_to on a FrameTrainer with exchange='{self._exchange_asked}': the motion windows of a flow step are "
                                          "not exchanged between ranks; exchange='none' only")
            if self.k != 1:
                raise NotImplementedError(f"flow_to with views_per_step={self.k}: a flow step takes one view per optimizer step")
        # the previous frame's exchange must be complete before this frame's optimizer-updated parameters are read (optimizer on) --
        # without an optimizer it only has to finish before its buffers are overwritten by this frame's attribute backward
        if self.optimizer and self._grads is not None:
            self._apply_optimizer()
        elif self.async_forward:
            self._settle_frame()
        self._last_args = (cam, bg, t, upstream, near, far, flow_to)
        return self._run_frame(cam, bg, t, upstream, near, far, flow_to)

    def _settle_frame(self):
        """async_forward: the pending frame's status; a frame whose tile lists were truncated is run again (with the capacity the policy
        has regrown) until it is whole -- before anybody consumes its gradients."""
        attempts = 0
        while True:
            fr, self._frame = self._frame, None
            if fr is None:
                return
            fr.wait()
            self._policy.poll()                     # (non-strict: counts the invalid frame, regrows the capacity, learns the flow flag)
            if fr.valid:
                return
            if attempts == 3:                       # the frame and three re-runs with regrown capacities were all truncated
                raise RuntimeError(f"a frame stayed invalid after {attempts} re-runs (last: {fr.num_rendered} instances for a capacity of {fr.capacity})")
            attempts += 1
            self.replays += 1
            self._run_frame(*self._last_args)       # leaves the re-run's pending status in self._frame: validated by the next turn of the loop

    def _run_frame(self, cam, bg, t, upstream, near, far, flow_to=None):
        m = self.model
        main = torch.cuda.current_stream(self.device)
        scal = attr.time_scalars(t, m.num_static, m.num_dynamic, m._xyz_motion.shape[1] if m.num_dynamic else 0,
                                 m.duration, m.interval, m.time_shift, m.var_pad, self.interp_type)
        with torch.no_grad():
            xyz, rot, opa, scl, _ = attr.forward_raw(scal, self.params, with_shs=False, interp_type=self.interp_type)
        leaves = [x.requires_grad_(True) for x in (xyz, rot, opa, scl)]
        feats = [self.params[i].detach().requires_grad_(True) for i in self.feature_idx]
        means2D = torch.empty_like(xyz, requires_grad=True)
        if flow_to is None:
            dir3D = torch.zeros_like(xyz, requires_grad=True)
            flow_ctx = contextlib.nullcontext()
        else:
            from . import motion
            from .diff_gaussian_rasterization_df import expect_flow
            scal_to = attr.time_scalars(flow_to, m.num_static, m.num_dynamic, m._xyz_motion.shape[1] if m.num_dynamic else 0,
                                        m.duration, m.interval, m.time_shift, m.var_pad, self.interp_type)
            moving = [self.params[self.names.index(n)] for n in motion.PARAM_NAMES]
            with torch.no_grad():
                dir3D = motion.displacement_raw(scal, scal_to, *moving, space="screen", camera=cam, near=near, interp_type=self.interp_type)
            dir3D.requires_grad_(True)
            flow_ctx = expect_flow()        # never the flow-free compositing kernel an asynchronous policy learned from plain frames
        e = torch.Tensor([])
        st = self._settings(cam, bg, near, far)
        if self.async_forward:
            from .diff_gaussian_rasterization_df import use_policy
            with use_policy(self._policy), flow_ctx:
                color, radii, depth, flow, acc, idx = rasterize_gaussians(leaves[0], means2D, dir3D, SplitSH(*feats), e, leaves[2], leaves[3], leaves[1], e, st)
            self._frame = self._policy.pending[-1] if self._policy.pending else None      # (None: the policy's synchronous seed frame)
        else:
            with flow_ctx:
                color, radii, depth, flow, acc, idx = rasterize_gaussians(leaves[0], means2D, dir3D, SplitSH(*feats), e, leaves[2], leaves[3], leaves[1], e, st)
        out = {"render": color, "depth": depth, "opticalflow": flow, "acc": acc, "radii": radii, "dominent_idxs": idx,
               "viewspace_points": means2D, "viewspace_l1points": dir3D, "visibility_filter": radii > 0}
        outs, gouts = upstream(out)
        torch.autograd.backward(outs, gouts)
        gin = [x.grad for x in leaves]                    # dL/d(means3D, rotations, opacities, scales)
        fgrads = [f.grad for f in feats]
        gdir = None if flow_to is None else (dir3D.grad if dir3D.grad is not None else torch.zeros_like(dir3D))
        # ---- attribute backward + exchange: side stream, overlapping the next frame's rasterization
        if self.side is not None:
            self.side.wait_stream(main)
            for g in gin + fgrads + ([] if gdir is None else [gdir]):
                g.record_stream(self.side)
            ctx = torch.cuda.stream(self.side)
        else:
            ctx = torch.cuda.stream(main)
        with ctx:
            if self.exchange_feat is not None and self.k == 1:
                self.exchange_feat.wait()
                self.exchange_feat.launch(fgrads)            # on the wire before the attribute backward runs
            if self.exchange is not None:
                self.exchange.wait()                       # previous frame's collectives own the persistent buffers until here
            for gth in self.kf_gather:
                gth.wait()
            gout = attr.backward_raw(scal, self.params, (gin[0], gin[1], gin[2], gin[3], None), with_shs=False, out=self.pgrad, sliced=self.sliced,
                                     interp_type=self.interp_type)
            self._flow = None
            if gdir is not None:
                self._flow_backward(scal, scal_to, moving, gdir, cam, near, gout[0] if self.sliced else gout, main)
            windows = None
            if self.sliced:
                gout, hint = gout
                self._hint = hint
                for gth, i, first in zip(self.kf_gather, self.kf_idx, (hint[0], hint[2])):
                    gth.launch(gout[i], first)               # all-gather of this rank's window (a plain copy for one rank)
                if self.mode == "sharded":                   # row all-to-all of the windows (inside the sharded optimizer)
                    windows = {i: (gout[i], first) for i, first in zip(self.kf_idx, (hint[0], hint[2]))}
            grads = [fgrads[self.feature_idx.index(i)] if i in self.feature_idx else gout[i] for i in range(len(self.params))]
            pending = self._submit(grads, windows)
        self.last = {"radii": radii}
        if pending:
            self._note_regularizers()
        return out

    def _flow_backward(self, scal, scal_to, moving, gdir, cam, near, gout, main):
        """dL/d(dir3D) of a flow_to frame back to `_xyz`, `_xyz_disp` and `_xyz_motion` (on the attribute backward's stream, after it):
        the two static gradients are added to the attribute backward's; the two keyframe windows wait for the optimizer step (sliced:
        self._flow, two more windows of `_xyz_motion`) or are added into the dense gradient, window 0 first."""
        from . import motion
        g_xyz, g_disp, g_win0, g_win1, mhint = motion.displacement_backward_raw(scal, scal_to, *moving, gdir, space="screen", camera=cam, near=near,
                                                                                interp_type=self.interp_type)
        ix, idisp, imot = (self.names.index(n) for n in motion.PARAM_NAMES)
        if gout[ix].numel():
            gout[ix].add_(g_xyz)
            gout[idisp].add_(g_disp)
        if not g_win0.shape[0]:
            return
        if self.sliced:
            for w in (g_win0, g_win1):
                w.record_stream(main)                    # consumed by the optimizer step on the caller's stream
            self._flow = (g_win0, g_win1, mhint)
        else:
            first0, count0, first1, count1 = mhint
            gout[imot][:, first0:first0 + count0] += g_win0
            gout[imot][:, first1:first1 + count1] += g_win1

    def _submit(self, grads, windows=None):
        """A view's 15 gradients on their way to the optimizer step: added to the group's accumulators (views_per_step > 1) and, with
        the group's last view, put on the wire (the feature gradients of a single-view step are there already).  windows: the sharded
        optimizer's keyframe windows.  False: accumulated only, no step follows this view."""
        if self.k > 1:
            # views 1 .. k-1 of the group: added to the accumulators, nothing goes on the wire, no optimizer step follows
            if self._acc is None:
                self._acc = [torch.zeros_like(p) for p in self.params]
            if self._nacc == 0:
                if self.exchange_feat is not None:
                    self.exchange_feat.wait()            # (the previous group's collectives own the accumulators until here)
                for a, g_ in zip(self._acc, grads):
                    a.copy_(g_)
            else:
                torch._foreach_add_(self._acc, list(grads))
            self._nacc += 1
            if self._nacc < self.k:
                self._grads = None
                return False
            self._nacc = 0
            grads = self._acc
            if self.exchange_feat is not None:
                self.exchange_feat.launch([grads[i] for i in self.feat_pos])
        self._grads = grads
        if self.exchange is not None:
            if self.exchange_feat is not None:
                self.exchange.launch([grads[i] for i in self.rest_pos])
            else:                                      # sharded: one reduce-scatter over the dense tensors + the window all-to-all
                self.opt.launch_exchange(grads, windows)
        return True

    def _note_regularizers(self):
        """The frame's regulariser weights and loss terms (at the parameters the frame was rendered with), on the main stream."""
        if self.regularizers is None:
            return
        from . import regularizers as reg
        w = self.regularizers() if callable(self.regularizers) else self.regularizers
        self._reg_w = tuple(float(x) for x in w)
        assert len(self._reg_w) == 3
        if self._reg_out is None:
            self._reg_out = torch.empty(4, dtype=torch.float32, device=self.device)
            self._reg_scratch = reg.new_scratch(self.device)
        m = self.model
        self.last["reg"] = reg.forward_raw(m._xyz_disp, m._xyz_motion, m._rotation_motion, self._reg_w, out=self._reg_out, scratch=self._reg_scratch)

    def _drain(self):
        """Everything pending ends on the current stream: an asynchronous frame is settled (re-run if it overflowed), the exchange
        finished, the side stream's attribute backward waited for."""
        if self.async_forward:
            self._settle_frame()
        self.finish_exchange()
        if self.side is not None:
            torch.cuda.current_stream(self.device).wait_stream(self.side)

    def _apply_optimizer(self):
        self._drain()
        # the step's regulariser weights; the terms are added HERE, after the exchange was drained: once per optimizer step, last, to the
        # gradient summed over ranks and views (with views_per_step > 1 the accumulators are what was exchanged)
        w = self._reg_w if self.regularizers is not None and self._reg_w is not None and any(self._reg_w) else None
        if self.mode == "sharded":
            reg = None
            if w is not None:                              # the owner of an element adds its term (dist.ShardedRAdam.step); sliced or dense alike
                from .regularizers import REG_MOTION, REG_ROT, REG_STATIC
                reg = {self.names.index(n): (kind, wt, self.params[self.names.index(n)].shape[0])        # rows: Ns, Nd, Nd -- the means' counts
                       for n, kind, wt in (("_xyz_disp", REG_STATIC, w[0]), ("_xyz_motion", REG_MOTION, w[1]), ("_rotation_motion", REG_ROT, w[2]))}
            self.opt.step(reg=reg)                         # (its exchange was launched by _run_frame: launch_exchange(grads, windows))
        else:
            from .optim import radam_step_raw, radam_step_sliced_raw, radam_step_sliced_reg_raw, REG_MOTION, REG_ROT
            self.steps += 1
            if w is not None:
                # dense gradients take their terms here (added to the frame's gradient buffers, which hold the sums over the ranks in mode
                # "allreduce": ParamGradExchange reduces in place); sliced keyframe tensors in the step below, on every rank's window
                from . import regularizers as reg
                gi = [self._grads[self.names.index(n)] for n in ("_xyz_disp", "_xyz_motion", "_rotation_motion")]
                if self.sliced:
                    gi[1] = gi[2] = None
                m_ = self.model
                reg.backward_raw(m_._xyz_disp, m_._xyz_motion, m_._rotation_motion, w, gi, accumulate=True)
            items = [(p.data_ptr(), g.data_ptr(), mm.data_ptr(), vv.data_ptr(), p.numel(), lr, self.steps, int(self.names[i] in NAN_TO_NUM))
                     for i, (p, g, mm, vv, lr) in enumerate(zip(self.params, self._grads, self.m, self.v, self.lrs)) if i not in self.kf_idx]
            hyper = ((0.9, 0.999), 1e-8, self.device)      # betas, eps: the defaults of the reference's RAdam (c_gaussian_model.py:449)
            radam_step_raw(items, *hyper)
            if self.sliced:
                sl = []
                for gth, i in zip(self.kf_gather, self.kf_idx):
                    p = self.params[i]
                    count, Cc = self.sliced_shapes[self.names[i]]
                    wins = gth.windows(count)
                    if self._flow is not None and self.names[i] == "_xyz_motion":
                        g_win0, g_win1, mhint = self._flow   # a flow_to frame: attribute window, motion window 0, motion window 1, summed in that order
                        wins = wins + [(mhint[0], mhint[1], g_win0.data_ptr()), (mhint[2], mhint[3], g_win1.data_ptr())]
                    item = (p.data_ptr(), self.m[i].data_ptr(), self.v[i].data_ptr(), p.shape[0], p.shape[1], Cc, self.lrs[i], self.steps,
                            wins, gth.first_device_ptr())
                    if w is not None:
                        motion = self.names[i] == "_xyz_motion"
                        item += (REG_MOTION if motion else REG_ROT, w[1] if motion else w[2], p.shape[0])
                    sl.append(item)
                (radam_step_sliced_reg_raw if w is not None else radam_step_sliced_raw)(sl, *hyper)
            torch.autograd.graph.increment_version(self.params)
        self._grads = None

    def flush(self):
        """Finish whatever is pending (exchange, optimizer step of the last frame) on the current stream."""
        if self.optimizer and self._grads is not None:
            self._apply_optimizer()
        else:
            self._drain()

    def begin_density_control(self):
        """Before densify_and_prune / a prune (ex4dgs_amd.densify) replaces the model's tensors: settles a pending asynchronous frame and
        DROPS the pending gradients without applying them -- train.py densifies before optimizer.step(), which then skips every replaced
        parameter (no .grad): that iteration's update is lost and the step count does not advance.  With an exchange ("allreduce",
        "sharded") the pending collectives are waited for first; every rank makes the density-control call at the same iteration, with
        densify.DensityStats(model, shared=True)."""
        if self.k != 1:
            raise NotImplementedError("density control on a FrameTrainer needs views_per_step=1 (the accumulated gradients of a group of views "
                                      "would be dropped half way)")
        self._drain()
        self._grads = None

    def rebind_parameters(self, moments=None):
        """After the model's tensors were replaced (ex4dgs_amd.densify): picks up the new parameters and rebuilds the P-sized buffers
        (gradient buffers, keyframe slice gathers, gradient exchanges, the sharded optimizer with its step counts).  moments: {name: (exp_avg, exp_avg_sq)} remapped to the new rows (None: zeros)."""
        if self._grads is not None:
            raise RuntimeError("rebind_parameters: pending gradients (call begin_density_control first)")
        self.params = [getattr(self.model, n) for n in self.names]
        self._make_grad_buffers()
        self._make_exchanges()
        moments = moments or {}
        pairs = [moments.get(n) for n in self.names]
        if self.mode == "sharded":
            self.opt.load_moments(pairs)
        elif self.optimizer:
            self.m = [pr[0] if pr is not None else torch.zeros_like(p) for pr, p in zip(pairs, self.params)]
            self.v = [pr[1] if pr is not None else torch.zeros_like(p) for pr, p in zip(pairs, self.params)]

    def grads(self):
        """The 15 (summed) parameter gradients of the last frame, valid after flush() when no optimizer consumed them."""
        return dict(zip(self.names, self._grads)) if self._grads is not None else None
