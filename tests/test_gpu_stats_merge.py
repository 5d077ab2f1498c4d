"""GPU tests of ex4d_densify_stats_merge (include/ex4d_densify.h) against its numpy restatement (tests/stats_merge_ref.py), bit for
bit: every rank count and size class of the kernel -- the last n % 4 Gaussians that go one per thread, rows off the 16-byte phase, the
workgroup's chunk, the grid-stride loop's second trip -- on values that take every branch of the fold, in buffers with guard words on
both sides.  Run with `-m gpu` on an MI355X; every case is a few launches."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import helpers as h
from tests import stats_merge_ref as mr

pytestmark = pytest.mark.gpu

GUARD, GUARD_VALUE = 64, -12345.678
CHUNK, MAX_BLOCKS = 1024, 1024             # densify.MERGE_CHUNK, densify.MERGE_MAX_BLOCKS (asserted below)
SMALL = [0, 1, 3, 4, 5, 63, 64, 65, 66, 67, 255, 256, 257, 258, 259, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 2, CHUNK + 3, 2 * CHUNK + 1]
SECOND_TRIP = CHUNK * MAX_BLOCKS + 3 * CHUNK + 3      # the first three workgroups take a second trip; three Gaussians go one per thread


def _guarded(arr, shift):
    """arr on the device, `shift` floats off a 16-byte boundary, between guard words.  Returns (the view, the whole allocation)."""
    flat = torch.full((GUARD + 4 + arr.size + GUARD,), GUARD_VALUE, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[GUARD + shift:GUARD + shift + arr.size].view(arr.shape)
    view.copy_(torch.from_numpy(arr))
    assert arr.size == 0 or view.data_ptr() % 16 == (4 * shift) % 16
    return view, flat


def _guards_intact(flat, view, what):
    lo = (view.data_ptr() - flat.data_ptr()) // 4
    outside = torch.cat([flat[:lo], flat[lo + view.numel():]])
    assert bool((outside == GUARD_VALUE).all()), (what, "guard words overwritten")


def _run(W, n, with_own=True, seed=0):
    from ex4dgs_amd import densify
    total, pending = mr.make_case(max(W, 1), n, seed)
    pending = pending[:W]
    want = mr.fold(total, pending)
    shifts = ((W + n) % 4, n % 4, (W + 1) % 4)
    t, t_all = _guarded(total, shifts[0])
    p, p_all = _guarded(pending, shifts[1])
    own, own_all = _guarded(pending[0] if W else mr.neutral(n), shifts[2])
    densify.merge_stats(t, p, own if with_own else None)
    torch.cuda.synchronize()
    what = f"W={W} n={n}"
    if n:
        h.assert_same_bits(t, want, np.ones(want.shape, bool), what)
    for flat, view in ((t_all, t), (p_all, p), (own_all, own)):
        _guards_intact(flat, view, what)
    assert np.array_equal(p.cpu().numpy().view(np.uint32), pending.view(np.uint32)), (what, "the gathered blocks are inputs")
    own_want = mr.neutral(n) if (with_own and W) else (pending[0] if W else mr.neutral(n))
    assert np.array_equal(own.cpu().numpy().view(np.uint32), own_want.view(np.uint32)), (what, "own pending block")


@pytest.mark.parametrize("W", [1, 2, 3, 8])
@pytest.mark.parametrize("n", SMALL)
def test_merge_equals_the_fold_bit_for_bit(hip_lib, W, n):
    from ex4dgs_amd import densify
    assert (densify.MERGE_CHUNK, densify.MERGE_MAX_BLOCKS) == (CHUNK, MAX_BLOCKS)
    _run(W, n)


@pytest.mark.parametrize("n", [SECOND_TRIP, SECOND_TRIP - 3])
def test_merge_grid_stride_second_trip(hip_lib, n):
    _run(2, n)


@pytest.mark.parametrize("n", [5, 257, CHUNK + 2])
def test_merge_without_an_own_block_and_with_no_ranks(hip_lib, n):
    _run(3, n, with_own=False)
    _run(0, n)                                   # W = 0: valid, nothing is done -- the own block is not reset either


def test_neutral_pending_blocks_leave_the_total_unchanged(hip_lib):
    from ex4dgs_amd import densify
    for W, n in ((1, 257), (8, CHUNK + 3)):
        total, _ = mr.make_case(W, n)
        rows = list(mr.SUM_ROWS)
        total[rows] = np.where(total[rows] == 0, 0.0, total[rows])
        t = torch.from_numpy(total).cuda()
        own = torch.from_numpy(mr.neutral(n)).cuda()
        densify.merge_stats(t, torch.from_numpy(mr.neutral(n, W)).cuda(), own)
        assert np.array_equal(t.cpu().numpy().view(np.uint32), total.view(np.uint32))
        assert np.array_equal(own.cpu().numpy().view(np.uint32), mr.neutral(n).view(np.uint32))


def test_merge_refuses_bad_arguments_with_the_headers_messages(hip_lib):
    from ex4dgs_amd import _abi
    n, W = 8, 2
    t = torch.zeros(9, n, device="cuda")
    p = torch.zeros(W, 9, n, device="cuda")
    own = torch.zeros(9, n, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    call = lambda *a: _abi.call("ex4d_densify_stats_merge", *a, s)
    for args, text in (((t.data_ptr(), p.data_ptr(), -1, n, None), "negative rank count or size"),
                       ((t.data_ptr(), p.data_ptr(), W, -1, None), "negative rank count or size"),
                       ((None, p.data_ptr(), W, n, None), "null or misaligned block"),
                       ((t.data_ptr(), None, W, n, None), "null or misaligned block"),
                       ((t.data_ptr() + 2, p.data_ptr(), W, n, None), "null or misaligned block"),
                       ((t.data_ptr(), p.data_ptr(), W, n, own.data_ptr() + 1), "null or misaligned block"),
                       ((p.data_ptr(), p.data_ptr(), W, n, None), "must not overlap"),                        # the total given as a gathered block
                       ((p[1].data_ptr(), p.data_ptr(), W, n, None), "must not overlap"),
                       ((t.data_ptr(), p.data_ptr(), W, n, p[1].data_ptr()), "must not overlap"),            # own inside the gathered blocks
                       ((t.data_ptr(), p.data_ptr(), W, n, t.data_ptr()), "must not overlap")):
        with pytest.raises(RuntimeError, match="densify_stats_merge: .*" + text):
            call(*args)
    call(None, None, 0, n, None)                 # W = 0 and n = 0 ask for nothing, pointers included
    call(None, None, W, 0, None)
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0 and float(p.abs().max()) == 0 and float(own.abs().max()) == 0


_RCCL_WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
import torch.distributed as dist
from ex4dgs_amd import _C, densify
from ex4dgs_amd.scene import make_scene
from tests import stats_merge_ref as mr

torch.cuda.set_device(0); _C.load()
dist.init_process_group(backend="nccl", rank=0, world_size=1)          # "nccl" is RCCL on ROCm
model, cam, bg = make_scene("cfg3", P=3001, device="cuda", fused=True)
ns, nd = model.num_static, model.num_dynamic
assert ns > 0 and nd > 0
stats = densify.DensityStats(model, shared=True)
plain = densify.DensityStats(model)
def view(seed):
    g = torch.Generator().manual_seed(seed)
    P = ns + nd
    radii = torch.randint(0, 300, (P,), generator=g, dtype=torch.int32)
    radii[torch.rand(P, generator=g) < 0.3] = 0
    e0 = torch.round(torch.rand(P, generator=g) * 16) / 16
    e = torch.stack([e0, e0 * torch.rand(P, generator=g), torch.rand(P, generator=g)], dim=1).contiguous()
    return radii.cuda(), (torch.randn(P, 3, generator=g) * 1e-3).cuda(), e.cuda()
bits = lambda x: x.detach().cpu().numpy().view(np.uint32)
# two views, an un-forced sync (a world of one: no collective, the pending block alone is folded in), a third view
for i in range(2):
    stats.update(*view(i), 10.0 + i); plain.update(*view(i), 10.0 + i)
assert np.array_equal(bits(stats.static), bits(torch.from_numpy(mr.neutral(ns)))), "update() accumulates into the pending blocks"
stats.sync()
stats.update(*view(2), 12.0)
for key in ("static", "dynamic"):
    assert not np.array_equal(bits(getattr(stats, "pending_" + key)), mr.neutral(getattr(stats, key).shape[1]).view(np.uint32))
before = {k: getattr(stats, k).cpu().numpy() for k in ("static", "dynamic")}
pend = {k: getattr(stats, "pending_" + k).cpu().numpy() for k in ("static", "dynamic")}
stats.sync(force=True)                                              # all_gather_into_tensor in the one-rank group + the kernel with W = 1
torch.cuda.synchronize()
for key in ("static", "dynamic"):
    want = mr.fold(before[key], pend[key][None])
    n = want.shape[1]
    assert np.array_equal(bits(getattr(stats, key)), want.view(np.uint32)), key
    assert np.array_equal(bits(getattr(stats, "pending_" + key)), mr.neutral(n).view(np.uint32)), key
# the reference-named attributes read the totals
assert stats.xyz_gradient_accum.data_ptr() == stats.static[0].data_ptr() and stats.motion_min_radii2D.data_ptr() == stats.dynamic[6].data_ptr()
assert float(stats.denom.sum()) > 0
# shared=False is the object of before: update() writes the totals, sync() does nothing
assert plain.pending_static is None and float(plain.denom.sum()) > 0
keep = bits(plain.static).copy(); plain.sync(force=True); assert np.array_equal(bits(plain.static), keep)
dist.barrier(); dist.destroy_process_group()
print("OK rccl")
"""


def test_shared_density_stats_sync_in_a_forced_one_rank_rccl_group(hip_lib, tmp_path):
    script = tmp_path / "stats_rccl_worker.py"
    script.write_text(_RCCL_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(34700 + (os.getpid() % 2000)), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, str(script), h.ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=180)
    assert r.returncode == 0 and "OK rccl" in r.stdout, r.stdout[-4000:]
