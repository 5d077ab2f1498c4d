"""GPU tests of multi-rank density control and growth: two ranks share the box's one GPU and talk over gloo (the pattern of
tests/test_gpu_dist.py).  Every rank trains on its own views with shared statistics (densify.DensityStats(shared=True)); after sync()
the totals are the numpy fold (tests/stats_merge_ref.py) of the ranks' pending blocks, and densify_and_prune / prune_invisible /
extract_dynamic_points leave every rank with the same bits -- the bits of a plain single-process call fed the same totals, moments
and draws.  Run with `-m gpu` on an MI355X."""
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
from ex4dgs_amd import _C, densify, growth, dist as xd
from ex4dgs_amd.scene import make_scene, upstream_grads
from ex4dgs_amd.trainer import FrameTrainer
from ex4dgs_amd.attributes import PARAM_ORDER
from tests import stats_merge_ref as mr

os.environ["LOCAL_RANK"] = "0"                       # both ranks on the box's one GPU
rank, world, local = xd.init_from_env(backend="gloo")
assert world == 2
torch.cuda.set_device(0); _C.load()
DEV = torch.device("cuda", 0)
LRS = {n: 1e-4 for n in PARAM_ORDER}
THR = dict(max_grad=1e-6, max_dgrad=1e-6, min_opacity=0.01, min_motion_opacity=0.01, extent=5.0)
stamps = [0, 100, 200, 299, 41, 88]
bits = lambda t: t.detach().contiguous().view(torch.int32)
nbits = lambda a: np.ascontiguousarray(a).view(np.uint32)

def scene():
    return make_scene("cfg3", P=20000, device="cuda", fused=True)

def same_on_ranks(items, what):
    for name, t in items:
        q = t.detach().clone()
        dist.broadcast(q, src=0)
        assert torch.equal(bits(q), bits(t)), (what, name, rank)

def gathered(block):
    out = [torch.empty_like(block) for _ in range(world)]
    dist.all_gather(out, block.clone())
    return torch.stack(out).cpu().numpy()

def moments(tr):
    if tr.mode == "sharded":
        return [tuple(x.clone() for x in pair) for pair in tr.opt.full_moments()]      # (a collective: every rank calls it)
    return [(a.clone(), b.clone()) for a, b in zip(tr.m, tr.v)]

def steps_of(tr):
    return list(tr.opt.steps) if tr.mode == "sharded" else [tr.steps] * len(tr.params)

def state(tr, stats):
    out = [("param " + n, p) for n, p in zip(tr.names, tr.params)]
    for n, (a, b) in zip(tr.names, moments(tr)):
        out += [("exp_avg " + n, a), ("exp_avg_sq " + n, b)]
    return out + [("stats static", stats.static), ("stats dynamic", stats.dynamic), ("pending static", stats.pending_static),
                  ("pending dynamic", stats.pending_dynamic)]

def neutral(block):
    return np.array_equal(nbits(block.cpu().numpy()), nbits(mr.neutral(block.shape[1])))


def trained(mode):
    # A trainer of `mode` after three steps on the rank's own views, its shared statistics (pending) and the step function.
    model, cam, bg = scene()
    H, W = cam.image_height, cam.image_width
    def upstream(out):
        gc, gd, gf, ga = upstream_grads(out["acc"], H, W, device=DEV)
        return [out["render"], out["depth"], out["opticalflow"], out["acc"]], [gc, gd, gf, ga]
    tr = FrameTrainer(model, exchange=mode, optimizer=True, lrs=LRS)
    assert tr.mode == mode and tr.sliced
    if mode == "sharded":                             # at 20 k Gaussians _features_rest is really sharded, the other tensors are "small"
        small = dict(zip(tr.names, tr.opt.small))
        assert not small["_features_rest"] and small["_xyz"] and tr.opt.state_bytes() < 8 * sum(p.numel() for p in tr.params)
    stats = densify.DensityStats(model, shared=True)
    def step(k):
        t = stamps[(2 * k + rank) % len(stamps)]
        out = tr.step(cam, bg, t, upstream)
        stats.update(out["radii"].int().contiguous(), out["viewspace_points"].grad, out["viewspace_l1points"].grad, t)
        return out
    for k in range(3):
        step(k)
    return model, cam, tr, stats, step


def density_control(mode):
    model, cam, tr, stats, step = trained(mode)
    P0 = model.num_static + model.num_dynamic
    # ---- statistics that are not shared are refused before anything is touched: every rank would decide on its own views
    try:
        densify.prune_small(model, densify.DensityStats(model), tr)
    except RuntimeError as e:
        assert "shared=True" in str(e) and tr._grads is not None and model.num_static + model.num_dynamic == P0
    else:
        raise AssertionError("a multi-rank trainer took statistics that are not shared")
    # ---- sync(): the totals are the fold of the two ranks' pending blocks, which this test gathers itself
    assert neutral(stats.static) and not neutral(stats.pending_static)
    before = {k: getattr(stats, k).cpu().numpy() for k in ("static", "dynamic")}
    pend = {k: gathered(getattr(stats, "pending_" + k)) for k in ("static", "dynamic")}
    assert not np.array_equal(nbits(pend["static"][0]), nbits(pend["static"][1])), "the ranks saw different views"
    stats.sync()
    for k in ("static", "dynamic"):
        want = mr.fold(before[k], pend[k])
        assert np.array_equal(nbits(getattr(stats, k).cpu().numpy()), nbits(want)), (mode, k)
        assert neutral(getattr(stats, "pending_" + k)), (mode, k)
    assert float(stats.denom.max()) > 1, "some Gaussian was counted by both ranks"
    # ---- densify_and_prune: a single-process twin is fed the same parameters, totals and moments, and the draws rank 0 makes
    tr.begin_density_control()
    twin_model, _, _ = scene()
    densify._rebind(twin_model, None, {n: p.detach().clone() for n, p in zip(tr.names, tr.params)}, {})
    twin = FrameTrainer(twin_model, exchange="none", optimizer=True, lrs=LRS)
    assert twin.mode == "none"
    mom = moments(tr)
    twin.m, twin.v, twin.steps = [a.clone() for a, _ in mom], [b.clone() for _, b in mom], steps_of(tr)[0]
    twin_stats = densify.DensityStats(twin_model)
    twin_stats.static, twin_stats.dynamic = stats.static.clone(), stats.dynamic.clone()
    steps_before = steps_of(tr)
    res = densify.densify_and_prune(model, stats, tr, **THR)
    twin_res = densify.densify_and_prune(twin_model, twin_stats, twin, **THR, noise=res["draws"])
    P1 = model.num_static + model.num_dynamic
    assert P1 != P0 and P1 == res["static"]["rows"] + res["dynamic"]["rows"], (P0, P1)
    assert res["static"] == twin_res["static"] and res["dynamic"] == twin_res["dynamic"]
    assert steps_of(tr) == steps_before and tr._grads is None
    assert all(a is b for a, b in zip((getattr(model, n) for n in tr.names), tr.params))
    same_on_ranks(state(tr, stats) + [("draw " + k, v) for k, v in res["draws"].items()], mode + " after densify")
    got = state(tr, stats)[:-2]
    ref = [("param " + n, getattr(twin_model, n)) for n in tr.names]
    for n, a, b in zip(tr.names, twin.m, twin.v):
        ref += [("exp_avg " + n, a), ("exp_avg_sq " + n, b)]
    ref += [("stats static", twin_stats.static), ("stats dynamic", twin_stats.dynamic)]
    for (name, a), (_, b) in zip(got, ref):
        assert a.shape == b.shape and torch.equal(bits(a), bits(b)), (mode, name)
    assert stats.pending_static.shape == stats.static.shape and neutral(stats.pending_static) and neutral(stats.pending_dynamic)
    # ---- three more steps: finite, identical on both ranks
    for k in range(3, 6):
        step(k)
    tr.flush(); torch.cuda.synchronize()
    assert steps_of(tr)[0] == steps_before[0] + 3
    assert all(bool(torch.isfinite(p).all()) for p in tr.params)
    same_on_ranks(state(tr, stats)[:-2], mode + " three steps after densify")
    # ---- prune_invisible and extract_dynamic_points(src=0), once each
    rows = model.num_static + model.num_dynamic
    out = densify.prune_invisible(model, stats, tr)
    assert out["static"]["rows"] + out["dynamic"]["rows"] == model.num_static + model.num_dynamic < rows
    assert float(stats.xyz_error_min_timestamp.min()) >= 0 and neutral(stats.pending_static)
    same_on_ranks(state(tr, stats), mode + " after prune_invisible")
    last = step(6)
    ns, nd = model.num_static, model.num_dynamic
    vis = (last["radii"][:ns] > 0).contiguous()
    cam_loc = cam.camera_center
    if rank != 0:                                     # what another rank hands in does not count: rank src's view decides
        vis, cam_loc = torch.zeros_like(vis), torch.tensor([9.0, 9.0, 9.0])
    out = growth.extract_dynamic_points(model, stats, tr, cam_loc, 0.0, vis, 5.0, percentile=0.5, src=0)
    assert out["visible"] > 0 and out["dynamic"]["clone"] > 0, out
    assert model.num_dynamic == nd + out["dynamic"]["clone"] and model.num_static == ns - out["dynamic"]["clone"]
    same_on_ranks(state(tr, stats), mode + " after extract_dynamic_points")
    for k in range(7, 9):
        step(k)
    tr.flush(); torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p).all()) for p in tr.params)
    same_on_ranks(state(tr, stats)[:-2], mode + " two steps after the extraction")
    # ---- expand_duration and adjust_temp_opa need the trainer's rebuilding alone (the sharded keyframe rows get new owner ranges)
    K = model._xyz_motion.shape[1]
    assert growth.expand_duration(model, tr, model.duration + 40) and model._xyz_motion.shape[1] > K
    growth.adjust_temp_opa(model, tr)
    for k in range(9, 11):
        step(k)
    tr.flush(); torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p).all()) for p in tr.params)
    same_on_ranks(state(tr, stats)[:-2], mode + " two steps after expand_duration")
    # ---- replicas that disagree: one rank's threshold perturbed -> different counts -> the same error on both ranks, no hang
    thr = dict(THR) if rank == 0 else dict(THR, max_grad=1e-2, min_opacity=0.5)
    rows = model.num_static + model.num_dynamic
    try:
        densify.densify_and_prune(model, stats, tr, **thr)
    except RuntimeError as e:
        assert "disagree" in str(e), e
        msg = [None] * world
        dist.all_gather_object(msg, str(e))
        assert msg[0] == msg[1]
    else:
        raise AssertionError("a count mismatch between the ranks went unnoticed")
    assert model.num_static + model.num_dynamic == rows


def lockstep():
    # The sharded optimizer against the replicated one through a densify, bit for bit.  The rasterizer backward sums with float atomics,
    # so two trainers that each render their own frames differ in the last bits however right the optimizers are: here both are fed the
    # SAME per-rank gradients (seeded), so every difference would be the optimizers' own -- the exchange, the sharded update, the moments
    # gathered from their owners before the densify and handed to the new owners after it.
    def feed(tr, step):
        g = torch.Generator(device=DEV).manual_seed(1000 * step + rank)
        gs = [torch.randn(p.shape, device=DEV, generator=g) * 1e-3 for p in tr.params]
        if tr.mode == "sharded":
            tr.opt.launch_exchange(gs)
        else:
            tr.exchange_feat.launch([gs[i] for i in tr.feat_pos]); tr.exchange.launch([gs[i] for i in tr.rest_pos])
        tr._grads = gs
        tr.flush()
    def pending_of(n, seed):
        total, pend = mr.make_case(1, n, seed)
        return torch.from_numpy(np.nan_to_num(pend[0], nan=0.5, posinf=3.0, neginf=0.0)).cuda()
    runs = {}
    for mode in ("allreduce", "sharded"):
        model, cam, bg = scene()
        tr = FrameTrainer(model, exchange=mode, optimizer=True, sliced=False, lrs=LRS)
        assert tr.mode == mode and not tr.sliced
        stats = densify.DensityStats(model, shared=True)
        runs[mode] = (model, tr, stats)
    def compare(what):
        (ma, ta, sa), (mb, tb, sb) = runs["allreduce"], runs["sharded"]
        for (name, a), (_, b) in zip(state(ta, sa), state(tb, sb)):
            assert a.shape == b.shape and torch.equal(bits(a), bits(b)), (what, name)
        assert steps_of(ta) == steps_of(tb)
        same_on_ranks(state(tb, sb), what)
    for step in range(1, 4):
        for mode in runs:
            feed(runs[mode][1], step)
        compare(f"step {step}")
    draws = None
    for mode, (model, tr, stats) in runs.items():
        stats.pending_static.copy_(pending_of(model.num_static, 10 + rank))
        stats.pending_dynamic.copy_(pending_of(model.num_dynamic, 20 + rank))
        rows = model.num_static + model.num_dynamic
        res = densify.densify_and_prune(model, stats, tr, max_grad=2e-4, max_dgrad=2e-4, min_opacity=0.01, min_motion_opacity=0.01, extent=5.0,
                                        noise=draws)
        draws = res["draws"]
        assert model.num_static + model.num_dynamic != rows and res["static"]["clone"] > 0 and res["static"]["split"] > 0
    compare("after densify")
    for step in range(4, 7):
        for mode in runs:
            feed(runs[mode][1], step)
        compare(f"step {step}")
    assert steps_of(runs["sharded"][1])[0] == 6


if PART == "lockstep":
    lockstep()
else:
    density_control(PART)
torch.cuda.synchronize()
dist.barrier(); dist.destroy_process_group()
print("OK", rank)
"""


def _two_ranks(tmp_path, part):
    """Both workers under one time limit each; if either fails or runs out of time both are killed and nothing more is started."""
    script = tmp_path / "density_worker.py"
    script.write_text(_WORKER)
    port = 35700 + (os.getpid() % 2000)
    procs, logs = [], []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        logs.append(open(tmp_path / f"rank{r}.log", "w+"))
        procs.append(subprocess.Popen([sys.executable, str(script), h.ROOT, part], env=env, stdout=logs[-1], stderr=subprocess.STDOUT, text=True))
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


@pytest.mark.parametrize("mode", ["allreduce", "sharded"])
def test_two_ranks_density_control_and_growth(hip_lib, tmp_path, mode):
    """One mode end to end on rendered frames.  Two runs that render their own frames differ in the last bits whatever the optimizer (the
    rasterizer backward sums with float atomics: tests/test_gpu_dist.py compares such runs to 2e-3 of the movement), so the sharded
    optimizer is compared with the replicated one bit for bit in test_sharded_equals_replicated_through_a_densify, on gradients that both
    are fed."""
    _two_ranks(tmp_path, mode)


def test_sharded_equals_replicated_through_a_densify(hip_lib, tmp_path):
    _two_ranks(tmp_path, "lockstep")
