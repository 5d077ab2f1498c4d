"""CPU tests of the multi-rank statistics merge: the numpy restatement of ex4d_densify_stats_merge (tests/stats_merge_ref.py) against
the sequential single-process update of tests/densify_ref.py, the shared replay of growth.ErrorTimestamps and the re-sharding of
dist.ShardedRAdam's moments (gloo, world size 2)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import densify_ref as dr
from tests import helpers as h
from tests import stats_merge_ref as mr

def _same_bits(got, ref, what):
    h.assert_same_bits(np.ascontiguousarray(got), np.ascontiguousarray(ref), np.ones(ref.shape, bool), what)


def _blocks(st):
    """The [9, ns] and [9, nd] blocks of a densify_ref statistics dict."""
    return tuple(np.stack([st[k].reshape(-1).numpy() for k in names]).astype(np.float32) for names in (dr.S_STATS, dr.D_STATS))


def _view(ns, nd, seed):
    """One iteration's inputs of DensityStats.update: radii (a third invisible), viewspace gradient, error channels with the decisions'
    edge values (e0 = 0, below the clamp, at 0.01; a NaN; ties of e1 / e0 between views)."""
    g = torch.Generator().manual_seed(seed)
    P = ns + nd
    radii = torch.randint(0, 1200, (P,), generator=g, dtype=torch.int32)
    radii[torch.rand(P, generator=g) < 0.33] = 0
    vgrad = torch.randn(P, 3, generator=g) * 1e-3
    e0 = torch.round(torch.rand(P, generator=g) * 16) / 16
    e0[torch.rand(P, generator=g) < 0.1] = 0.0
    e0[torch.rand(P, generator=g) < 0.05] = 0.01
    e0[torch.rand(P, generator=g) < 0.05] = 5e-5
    e1 = e0 * (torch.round(torch.rand(P, generator=g) * 4) / 4)             # l1 = e1 / e0 on a grid of five values: ties between views
    e2 = torch.rand(P, generator=g)
    egrad = torch.stack([e0, e1, e2], dim=1).contiguous()
    egrad[P // 2, 1] = float("nan")
    return radii, vgrad, egrad


@pytest.mark.parametrize("W", [1, 2, 3, 8])
@pytest.mark.parametrize("n", [1, 5, 64, 257])
def test_neutral_blocks_are_the_identity(W, n):
    total, _ = mr.make_case(W, n)
    total[list(mr.SUM_ROWS)] = np.where(total[list(mr.SUM_ROWS)] == 0, 0.0, total[list(mr.SUM_ROWS)])      # (-0.0 + 0 is +0.0: not a reachable sum)
    got = mr.fold(total, mr.neutral(n, W))
    assert np.array_equal(got.view(np.uint32), total.view(np.uint32))
    assert np.array_equal(mr.fold(total, np.zeros((0, 9, n), np.float32)).view(np.uint32), total.view(np.uint32))


def test_make_case_takes_every_branch():
    total, pending = mr.make_case(3, 257)
    got = mr.fold(total, pending)
    kind = np.arange(257) % mr.KINDS
    assert (got[mr.ERROR_MIN_T, kind == 2] == 100.0).all() and (got[mr.ERROR_MIN, kind == 2] == 0.25).all()      # the lowest rank wins the tie
    assert (got[mr.ERROR_MIN_T, kind == 3] == 7.0).all()                                                       # the total keeps its own on a tie
    assert np.isnan(got[mr.GRAD_ACCUM, kind == 4]).all() and np.isnan(got[mr.SSIM_ACCUM, kind == 4]).all()
    assert (got[mr.ERROR_MIN, kind == 5] == 0.125).all() and (got[mr.ERROR_MIN_T, kind == 5] == 66.0).all()    # the NaN minimum was never taken
    assert np.isnan(got[mr.ERROR_MIN, kind == 6]).all() and (got[mr.ERROR_MIN_T, kind == 6] == 9.0).all()      # a NaN total is never replaced
    assert np.isnan(got[mr.ERROR_ACCUM, kind == 7]).all() and np.isinf(got[mr.MAX_RADII, kind == 7]).all()
    assert np.array_equal(got[:, kind == 1].view(np.uint32), total[:, kind == 1].view(np.uint32))
    one, p1 = mr.make_case(1, 64)
    assert (mr.fold(one, p1)[mr.ERROR_MIN, np.arange(64) % mr.KINDS == 5] == 0.875).all()                       # W = 1: the NaN delta alone, not taken


@pytest.mark.parametrize("W", [1, 2, 3, 8])
def test_one_update_per_rank_equals_the_sequential_run_bit_for_bit(W):
    ns, nd = 301, 77
    seq = dr.init_stats(ns, nd)
    for i in range(3):                                      # a history before the sync: the totals are not at their initial values
        dr.update(seq, *_view(ns, nd, 50 + i), 5.0 + i)
    total = _blocks(seq)
    pend = []
    for w in range(W):
        view, t = _view(ns, nd, 100 + w), 20.0 + w
        own = dr.init_stats(ns, nd)
        dr.update(own, *view, t)
        pend.append(_blocks(own))
        dr.update(seq, *view, t)                            # the single process sees the ranks' views in rank order
    for g, name in enumerate(("static", "dynamic")):
        got = mr.fold(total[g], np.stack([p[g] for p in pend]))
        _same_bits(got, _blocks(seq)[g], f"{name} W={W}")


@pytest.mark.parametrize("W", [2, 3, 8])
def test_several_updates_per_rank_keep_the_order_free_rows(W):
    """The float sums depend on the grouping; the max / min rows, the (error minimum, timestamp) pair and the integer-valued counters
    do not: equal to one process that saw rank 0's views, then rank 1's, ..."""
    ns, nd = 301, 77
    seq = dr.init_stats(ns, nd)
    dr.update(seq, *_view(ns, nd, 49), 4.0)
    total = _blocks(seq)
    pend = []
    for w in range(W):
        own = dr.init_stats(ns, nd)
        for j in range(1 + (w + 1) % 3 + 1):
            view, t = _view(ns, nd, 1000 + 10 * w + j), 30.0 + 10 * w + j
            dr.update(own, *view, t)
            dr.update(seq, *view, t)
        pend.append(_blocks(own))
    rows = [mr.DENOM, mr.ERROR_DENOM, mr.MAX_RADII, mr.MIN_RADII, mr.ERROR_MIN, mr.ERROR_MIN_T]
    for g, name in enumerate(("static", "dynamic")):
        got = mr.fold(total[g], np.stack([p[g] for p in pend]))
        _same_bits(got[rows], _blocks(seq)[g][rows], f"{name} W={W}")
        ref = _blocks(seq)[g]
        for r in (mr.GRAD_ACCUM, mr.ERROR_ACCUM, mr.SSIM_ACCUM):       # regrouped float sums: equal to rounding
            ok = np.isfinite(ref[r])
            assert np.allclose(got[r][ok], ref[r][ok], rtol=1e-5, atol=1e-6), (name, r)


_WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
from ex4dgs_amd import dist as xd
from ex4dgs_amd.growth import ErrorTimestamps
from oracle import optim_oracle

rank, world, local = xd.init_from_env(backend="gloo")
assert world == 2

# ---- ErrorTimestamps(shared=True): the replay in (mark index, rank) order is the dict of one process that saw the views in that order
def marks(r):
    g = np.random.default_rng(3 + r)
    return [(float(g.random()) * (3.0 if i % 4 == r else 1.0), int(g.integers(0, 300))) for i in range(9 if r == 0 else 6)]
interval = 10
shared = ErrorTimestamps(interval, shared=True)
one = ErrorTimestamps(interval)
logs = [marks(0), marks(1)]
def replay(upto_a, upto_b):
    for i in range(upto_a, upto_b):
        for r in range(world):
            if i < len(logs[r]):
                one.mark(*logs[r][i])
for i, (loss, t) in enumerate(logs[rank][:4]):
    shared.mark(loss, t)
shared.sync(); replay(0, 4)
assert list(shared.errors.items()) == list(one.errors.items()), (shared.errors, one.errors)
for loss, t in logs[rank][4:]:
    shared.mark(loss, t)
replay(4, 9)
for k in range(4):                                         # pop() syncs first, then agrees pop after pop
    a, b = shared.pop(), one.pop()
    assert a == b and a is not None, (k, a, b)
    assert list(shared.errors.items()) == list(one.errors.items())

# ---- ShardedRAdam.full_moments / load_moments: the moments whole on every rank, and a new optimizer over remapped rows goes on as the
#      replicated one does
shapes = [(1003, 3), (257, 35, 4), (10, 1), (4099,)]
lrs = [1.6e-4, 1e-3, 5e-2, 5e-3]
g0 = torch.Generator().manual_seed(7)
init = [torch.randn(*s, generator=g0) for s in shapes]
def grads_of(r, step, shp):
    g = torch.Generator().manual_seed(1000 * step + r)
    return [torch.randn(*s, generator=g) * (0.1 + step) for s in shp]
def oracle_step(items, betas, eps, device):
    for p, g, m, v, n, lr, step, sanitize in items:
        optim_oracle.radam_step(p.numpy(), g.numpy().copy(), m.numpy(), v.numpy(), step, lr, betas[0], betas[1], eps)
params = [x.clone() for x in init]
opt = xd.ShardedRAdam(params, lrs, step_fn=oracle_step, small_bytes=256)
assert opt.exchange.small == [False, False, True, False]
ref = [x.clone() for x in init]
m = [torch.zeros_like(x) for x in init]; v = [torch.zeros_like(x) for x in init]
def both_step(step, shp):
    opt.launch_exchange(grads_of(rank, step, shp)); opt.step()
    ga, gb = grads_of(0, step, shp), grads_of(1, step, shp)
    for i in range(len(ref)):
        optim_oracle.radam_step(ref[i].numpy(), (ga[i] + gb[i]).numpy(), m[i].numpy(), v[i].numpy(), step, lrs[i])
for step in range(1, 4):
    both_step(step, shapes)
full = opt.full_moments()
for i in range(len(shapes)):
    assert full[i][0].shape == params[i].shape
    assert torch.equal(full[i][0], m[i]) and torch.equal(full[i][1], v[i]), i          # tails and small tensors included
# rows leave and rows arrive: every tensor keeps a subset of its rows and gains zero-moment rows, as a densify does
keep = [torch.arange(s[0]) % 3 != 1 for s in shapes]
def remap(x, k, fill):
    extra = torch.full((5,) + tuple(x.shape[1:]), fill, dtype=x.dtype)
    return torch.cat([x[k], extra]).contiguous()
params = [remap(p, k, 0.5) for p, k in zip(params, keep)]
ref = [remap(p, k, 0.5) for p, k in zip(ref, keep)]
m = [remap(x, k, 0.0) for x, k in zip(m, keep)]; v = [remap(x, k, 0.0) for x, k in zip(v, keep)]
new_moments = [(remap(a, k, 0.0), remap(b, k, 0.0)) for (a, b), k in zip(full, keep)]
old_steps = list(opt.steps)
opt = xd.ShardedRAdam(params, lrs, step_fn=oracle_step, small_bytes=256)
opt.steps = old_steps
opt.load_moments(new_moments)
shapes2 = [tuple(p.shape) for p in params]
for step in range(4, 7):
    both_step(step, shapes2)
    for i, (a, b) in enumerate(zip(params, ref)):
        assert torch.equal(a, b), (step, i, float((a - b).abs().max()))
opt.load_moments([None] * len(params))
assert all(float(x.abs().max()) == 0 for x in opt.exp_avg + opt.exp_avg_sq)
torch.distributed.barrier(); torch.distributed.destroy_process_group()
print("OK", rank)
"""


def test_shared_error_timestamps_and_moment_resharding_gloo_world2(tmp_path):
    script = tmp_path / "worker_stats_merge.py"
    script.write_text(_WORKER)
    port = 33500 + (os.getpid() % 2000)
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script), h.ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"OK {r}" in o, o
