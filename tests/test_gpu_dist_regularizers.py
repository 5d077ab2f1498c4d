"""GPU tests of the motion regularisers on several ranks: two ranks share the box's one GPU and talk over gloo (the pattern of
tests/test_gpu_dist_density.py).  The term is added once per optimizer step, last, to the gradient summed over ranks and views, after
the exchange: every rank ends a step with the same bits, the bits of a single-process step fed the reduced gradient.  Run with `-m gpu`
on an MI355X."""
import os
import subprocess
import sys
import time

import pytest

from tests import helpers as h

pytestmark = pytest.mark.gpu

WORKER_SECONDS = 180

_WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
PART = sys.argv[2]
import numpy as np, torch
import torch.distributed as dist
from ex4dgs_amd import _C, densify, dist as xd
from ex4dgs_amd.scene import make_scene, upstream_grads
from ex4dgs_amd.trainer import FrameTrainer
from ex4dgs_amd.attributes import PARAM_ORDER
from tests import stats_merge_ref as mr

os.environ["LOCAL_RANK"] = "0"                       # both ranks on the box's one GPU
rank, world, local = xd.init_from_env(backend="gloo")
assert world == 2
torch.cuda.set_device(0); _C.load()
DEV = torch.device("cuda", 0)
KEYFRAMES = ("_xyz_motion", "_rotation_motion")
stamps = [0, 100, 200, 299, 41, 88]
bits = lambda t: t.detach().contiguous().view(torch.int32)

def scene():
    return make_scene("cfg3", P=20000, device="cuda", fused=True)

def same_on_ranks(items, what):
    for name, t in items:
        q = t.detach().clone()
        dist.broadcast(q, src=0)
        assert torch.equal(bits(q), bits(t)), (what, name, rank)

def moments(tr):
    if tr.mode == "sharded":
        return [tuple(x.clone() for x in pair) for pair in tr.opt.full_moments()]      # (a collective: every rank calls it)
    return [(a.clone(), b.clone()) for a, b in zip(tr.m, tr.v)]

def steps_of(tr):
    return list(tr.opt.steps) if tr.mode == "sharded" else [tr.steps] * len(tr.params)

def state(tr):
    out = [("param " + n, p) for n, p in zip(tr.names, tr.params)]
    for n, (a, b) in zip(tr.names, moments(tr)):
        out += [("exp_avg " + n, a), ("exp_avg_sq " + n, b)]
    return out

def refuse(*a, **k):
    raise AssertionError("a regularised launch in a step without regularisers")


def rendered(mode):
    # Three steps on the rank's own rendered views, the three terms on.  Up to step 5 RAdam moves a parameter by lr * gradient: a
    # keyframe no window touched has the term alone, weight / (Nd (K-1)) per unit vector, so the keyframe tensors get a learning rate
    # and weights at which three such steps are more than an ulp of their values (of order 10 - 100): 1e-2 * 1e3 / 136 000 = 7e-5.
    lrs = dict({n: 1e-4 for n in PARAM_ORDER}, _xyz_motion=1e-2, _rotation_motion=1e-2)
    W3 = (1e-2, 1e3, 1e3)
    runs = {}
    for key, regs in (("on", W3), ("off", None)):
        model, cam, bg = scene()
        H, W = cam.image_height, cam.image_width
        def upstream(out, H=H, W=W):
            gc, gd, gf, ga = upstream_grads(out["acc"], H, W, device=DEV)
            return [out["render"], out["depth"], out["opticalflow"], out["acc"]], [gc, gd, gf, ga]
        p0 = {n: getattr(model, n).detach().clone() for n in KEYFRAMES}
        tr = FrameTrainer(model, exchange=mode, optimizer=True, lrs=lrs, regularizers=regs)
        assert tr.mode == mode and tr.sliced
        for n in KEYFRAMES:                           # past the 1 MB threshold: really sharded, by rows
            p = getattr(model, n)
            assert p.numel() * 4 >= 1 << 20
            if mode == "sharded":
                i = tr.names.index(n)
                lo, hi = tr.opt.owned[i]
                assert not tr.opt.small[i] and 0 < hi - lo < p.numel() and (hi - lo) % (p.shape[1] * p.shape[2]) == 0
        if mode == "sharded":
            i = tr.names.index("_xyz_disp")           # "small": all-reduced whole and updated by every rank, which adds the whole term
            assert tr.opt.small[i] and tr.opt.owned[i] == (0, model._xyz_disp.numel())
        for k in range(3):
            tr.step(cam, bg, stamps[(2 * k + rank) % len(stamps)], upstream)
            if regs is not None:
                reg4 = tr.last["reg"]
                assert reg4.shape == (4,) and bool(torch.isfinite(reg4).all()) and float(reg4[3]) != 0.0
                same_on_ranks([("last reg", reg4)], f"{mode} step {k}")
        tr.flush(); torch.cuda.synchronize()
        assert steps_of(tr)[0] == 3 and all(bool(torch.isfinite(p).all()) for p in tr.params)
        same_on_ranks(state(tr), f"{mode} regularizers {key}")
        runs[key] = (model, p0)
    # the term reached the step: keyframes no window touched stay where they were without it and move with it
    (on, p0), (off, _) = runs["on"], runs["off"]
    for n in KEYFRAMES:
        still = getattr(off, n) == p0[n]
        frac_still = float(still.float().mean())
        frac_moved = float((getattr(on, n)[still] != p0[n][still]).float().mean())
        print(f"{mode} {n}: {frac_still:.3f} of the entries untouched without regularisers, {frac_moved:.3f} of those moved with them")
        assert frac_still > 0.1 and frac_moved > 0.5, (mode, n, frac_still, frac_moved)
    assert not torch.equal(on._xyz_disp, off._xyz_disp)


def lockstep(variant):
    # "allreduce", "sharded" and a single-process-style reference (exchange "none", dense keyframe gradients, rank 0 only) are fed the
    # same seeded gradients -- rendered frames differ in their last bits from run to run -- and must be bit-equal after every step.
    # The reference is fed the REDUCED gradients: the sums over the ranks (and the group's views), keyframe windows scattered into
    # dense tensors in rank order.  variant: "sliced" | "dense" | "views2".
    W3 = (1e-3, 2e-2, 3e-2)
    LRS = {n: 1e-3 for n in PARAM_ORDER}
    k = 2 if variant == "views2" else 1
    kw = dict(optimizer=True, lrs=LRS, regularizers=W3)
    if variant == "dense":
        kw["sliced"] = False
    if k > 1:
        kw["views_per_step"] = k
    runs = {}
    for mode in ("allreduce", "sharded"):
        model, cam, bg = scene()
        tr = FrameTrainer(model, exchange=mode, **kw)
        assert tr.mode == mode and tr.sliced == (variant == "sliced") and tr.k == k
        runs[mode] = (model, tr, densify.DensityStats(model, shared=True))
    ref = None
    if rank == 0:                                     # nothing of the reference enters a collective
        model, cam, bg = scene()
        tr = FrameTrainer(model, exchange="none", optimizer=True, lrs=LRS, regularizers=W3, sliced=False)
        assert tr.mode == "none" and not tr.sliced
        ref = (model, tr, densify.DensityStats(model))

    def view_grads(tr, step, view):
        g = torch.Generator(device=DEV).manual_seed(1000 * step + 10 * view + rank)
        gs = [torch.randn(p.shape, device=DEV, generator=g) * 1e-3 for p in tr.params]
        wins = {}
        if tr.sliced:
            for i in tr.kf_idx:
                rows, K, C = tr.params[i].shape
                count = tr.sliced_shapes[tr.names[i]][0]
                first = int(torch.randint(0, K - count + 1, (1,), generator=torch.Generator().manual_seed(77 * step + 5 * rank + i)))
                wins[i] = (torch.randn((rows, count, C), device=DEV, generator=g) * 1e-3, first)
        return gs, wins

    def reduced(tr, step):
        # the sums the reference is fed, made by collectives of this test's own
        total = None
        for view in range(k):
            gs, wins = view_grads(tr, step, view)
            for i, (w, first) in wins.items():        # this rank's window as the dense gradient it stands for
                gs[i] = torch.zeros_like(tr.params[i])
                gs[i][:, first:first + w.shape[1]] = w
            if total is None:
                total = gs
            else:
                torch._foreach_add_(total, gs)        # views first (the accumulators), then ranks
        out = []
        for i, g in enumerate(total):
            both = [torch.empty_like(g) for _ in range(world)]
            dist.all_gather(both, g.contiguous())
            out.append(both[0] + both[1])             # rank order
        return out

    def feed(tr, step):
        for view in range(k):
            gs, wins = view_grads(tr, step, view)
            if tr.mode == "allreduce" and k == 1:     # a single-view step has its feature gradients on the wire before the attribute backward
                tr.exchange_feat.launch([gs[i] for i in tr.feat_pos])
                for gth, i in zip(tr.kf_gather, tr.kf_idx):
                    gth.launch(*wins[i])
            pending = tr._submit(gs, wins if tr.mode == "sharded" and tr.sliced else None)
            assert pending == (view == k - 1)
        tr._note_regularizers()
        tr.flush()

    def compare(what):
        (ma, ta, sa), (mb, tb, sb) = runs["allreduce"], runs["sharded"]
        A, B = state(ta), state(tb)
        for (name, a), (_, b) in zip(A, B):
            assert a.shape == b.shape and torch.equal(bits(a), bits(b)), (variant, what, name)
        assert steps_of(ta) == steps_of(tb)
        same_on_ranks(B, what)
        same_on_ranks([("last reg", tb.last["reg"])], what)
        assert torch.equal(bits(ta.last["reg"]), bits(tb.last["reg"]))
        if ref is not None:
            mr_, tr_, _ = ref
            R = [("param " + n, p) for n, p in zip(tr_.names, tr_.params)]
            for n, a, b in zip(tr_.names, tr_.m, tr_.v):
                R += [("exp_avg " + n, a), ("exp_avg_sq " + n, b)]
            for (name, a), (_, b) in zip(B, R):
                assert a.shape == b.shape and torch.equal(bits(a), bits(b)), (variant, what, "single-process reference", name)
            assert steps_of(tb)[0] == tr_.steps

    def step_all(step):
        sums = reduced(runs["sharded"][1], step)
        for mode in runs:
            feed(runs[mode][1], step)
        if ref is not None:
            ref[1]._grads = sums
            ref[1]._note_regularizers()
            ref[1].flush()
        compare(f"step {step}")

    p0 = runs["sharded"][0]._xyz_motion.detach().clone()
    for step in range(1, 4):
        step_all(step)
    assert not torch.equal(runs["sharded"][0]._xyz_motion, p0)
    if k > 1:
        return
    # ---- densify_and_prune with shared statistics: rebuilt exchanges and remapped moments keep the term (the weights are per step)
    def pending_of(n, seed):
        total, pend = mr.make_case(1, n, seed)
        return torch.from_numpy(np.nan_to_num(pend[0], nan=0.5, posinf=3.0, neginf=0.0)).cuda()
    THR = dict(max_grad=2e-4, max_dgrad=2e-4, min_opacity=0.01, min_motion_opacity=0.01, extent=5.0)
    draws = None
    for mode, (model, tr, stats) in runs.items():
        stats.pending_static.copy_(pending_of(model.num_static, 10 + rank))
        stats.pending_dynamic.copy_(pending_of(model.num_dynamic, 20 + rank))
        stats.sync()
        totals = (stats.static.clone(), stats.dynamic.clone())
        rows = model.num_static + model.num_dynamic
        res = densify.densify_and_prune(model, stats, tr, **THR, noise=draws)
        draws = res["draws"]
        assert model.num_static + model.num_dynamic != rows and res["static"]["clone"] > 0 and res["static"]["split"] > 0
    if ref is not None:
        model, tr, stats = ref
        stats.static, stats.dynamic = totals
        densify.densify_and_prune(model, stats, tr, **THR, noise=draws)
        assert model.num_static == runs["sharded"][0].num_static and model.num_dynamic == runs["sharded"][0].num_dynamic
    for step in range(4, 7):
        step_all(step)
    assert steps_of(runs["sharded"][1])[0] == 6


def weights_off():
    # regularizers=None and all-zero weights launch what a trainer built without the keyword launches: fed the same gradients the three
    # are bit-equal, and nothing of the zero-weight one reaches a regularised launch.
    LRS = {n: 1e-3 for n in PARAM_ORDER}
    for mode in ("allreduce", "sharded"):
        trainers = []
        for kw in ({}, dict(regularizers=None), dict(regularizers=(0.0, 0.0, 0.0))):
            model, cam, bg = scene()
            tr = FrameTrainer(model, exchange=mode, optimizer=True, lrs=LRS, **kw)
            assert tr.mode == mode and tr.sliced
            if mode == "sharded" and kw.get("regularizers") is not None:
                tr.opt.sliced_reg_step_fn = tr.opt.reg_range_fn = refuse
            trainers.append(tr)
        for step in range(1, 3):
            for tr in trainers:
                g = torch.Generator(device=DEV).manual_seed(1000 * step + rank)
                gs = [torch.randn(p.shape, device=DEV, generator=g) * 1e-3 for p in tr.params]
                wins = {i: (torch.randn((tr.params[i].shape[0],) + tr.sliced_shapes[tr.names[i]], device=DEV, generator=g) * 1e-3, (3 * step + rank + i) % 7)
                        for i in tr.kf_idx}
                if mode == "allreduce":
                    tr.exchange_feat.launch([gs[i] for i in tr.feat_pos])
                    for gth, i in zip(tr.kf_gather, tr.kf_idx):
                        gth.launch(*wins[i])
                assert tr._submit(gs, wins if mode == "sharded" else None)
                tr._note_regularizers()
                tr.flush()
        S = [state(tr) for tr in trainers]
        for other in S[1:]:
            for (name, a), (_, b) in zip(S[0], other):
                assert torch.equal(bits(a), bits(b)), (mode, name)


if PART in ("allreduce", "sharded"):
    rendered(PART)
elif PART == "off":
    weights_off()
else:
    lockstep(PART)
torch.cuda.synchronize()
dist.barrier(); dist.destroy_process_group()
print("OK", rank)
"""


def _two_ranks(tmp_path, argv, port_base):
    """Both workers under one time limit; if either fails or runs out of time both are killed and nothing more is started."""
    port = port_base + (os.getpid() % 2000)
    procs, logs = [], []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        logs.append(open(tmp_path / f"rank{r}.log", "w+"))
        procs.append(subprocess.Popen([sys.executable] + argv, env=env, stdout=logs[-1], stderr=subprocess.STDOUT, text=True))
    deadline = time.monotonic() + WORKER_SECONDS
    verdict = None
    while verdict is None:
        for p in procs:
            try:
                p.wait(timeout=0.25)
            except subprocess.TimeoutExpired:
                pass
        codes = [p.poll() for p in procs]
        if any(c not in (None, 0) for c in codes):
            verdict = "a worker failed"
        elif all(c == 0 for c in codes):
            verdict = "done"
        elif time.monotonic() > deadline:
            verdict = f"a worker ran longer than {WORKER_SECONDS} s"
    for p in procs:
        if p.poll() is None:
            p.kill()
        p.wait()
    outs = []
    for f in logs:
        f.seek(0)
        outs.append(f.read())
        f.close()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert verdict == "done" and p.returncode == 0 and f"OK {r}" in o, (verdict, r, p.returncode, outs[0][-3000:], outs[1][-3000:])


def _trainer_part(tmp_path, part):
    script = tmp_path / "regularizers_worker.py"
    script.write_text(_WORKER)
    _two_ranks(tmp_path, [str(script), h.ROOT, part], 37700)


@pytest.mark.parametrize("mode", ["allreduce", "sharded"])
def test_two_ranks_train_rendered_frames_with_regularizers(hip_lib, tmp_path, mode):
    """Three rendered steps with the three terms on: the same parameter and moment bits and the same last["reg"] on both ranks, and
    keyframes no window touched moved -- the term reached the step."""
    _trainer_part(tmp_path, mode)


@pytest.mark.parametrize("variant", ["sliced", "dense", "views2"])
def test_both_modes_equal_a_single_process_step_fed_the_reduced_gradient(hip_lib, tmp_path, variant):
    """Fed gradients: "allreduce", "sharded" and the single-process reference bit-equal after each of three steps, across a
    densify_and_prune and three further steps; views_per_step=2 applies the term once per two views."""
    _trainer_part(tmp_path, variant)


def test_two_ranks_with_regularizers_off_launch_what_they_launched_before(hip_lib, tmp_path):
    _trainer_part(tmp_path, "off")


@pytest.mark.parametrize("case", ["dense", "sliced", "off"])
def test_sharded_radam_on_the_device_gives_the_oracles_bits(hip_lib, tmp_path, case):
    """tests/dist_reg_worker.py on GPU tensors with the HIP defaults of every hook: element shards that cut rows and keyframes of tiny
    tensors (_xyz_disp's cut-row shard runs on the device here), against the numpy oracle of tests/test_cpu_dist_regularizers.py."""
    _two_ranks(tmp_path, [os.path.join(h.ROOT, "tests", "dist_reg_worker.py"), h.ROOT, "cuda", case], 39700)
