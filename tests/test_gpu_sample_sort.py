"""The sample depth sort (option "depth_sort_sample" = 1) against the host restatement (run with `-m gpu` on an MI355X).

Every frame of tests/depth_sort_cases.py and of tests/sample_sort_cases.py goes through tests/raw_abi.forward on guarded buffers with
the option on, under both tile sorts, both rankings, synchronously and asynchronously; the state buffers hold 0xFF bytes for the
first frame and what the frame before left afterwards.  All comparisons are exact: the depths are the designed bit patterns, the depth
order, the point list, the tile ranges and the sorted tile ids are binning_cases.host_binning's on the frame's own arrays, the six
outputs are bit-equal to the LSD variant's, the guards are intact, "depth_sort_sample_frames" advanced (or, where the planes leave the
frame to the LSD sort, did not), and the device census (ex4d_debug_sample_sort) is sample_sort_cases.restate's on the frame's own keys."""
import numpy as np
import pytest
import torch

from tests import binning_cases as bc
from tests import depth_sort_cases as dc
from tests import helpers as h
from tests import raw_abi
from tests import sample_sort_cases as sc
from tests import test_gpu_buffer_contract as table

pytestmark = pytest.mark.gpu

OUTPUTS = ("color", "radii", "depth", "acc", "flow", "idx")
LSD = dict(depth_sort_msd=0, depth_sort_sample=0, depth_sort_sample_stats=0, binning_tile_ids=1)
SAMPLE = dict(depth_sort_sample=1, depth_sort_sample_stats=1, binning_tile_ids=1)
# tile sort x ranking x synchronous / asynchronous
MATRIX = [(f"rows={r}, rank={k}{', async' if a else ''}", dict(SAMPLE, tile_sort_rows=r, rank_lds_atomics=k), a) for r in (1, 0) for k in (-1, 0) for a in (0, 1)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = (got != want).reshape(got.shape[0], -1).any(1).nonzero()
        i = int(bad[0])
        raise AssertionError(f"{what}: {int(bad.numel())} of {got.shape[0]} differ, first at {i}: got {got[i].tolist()}, expected {want[i].tolist()}")


def _expected(f, W, H):
    hb = bc.host_binning(f["radii"], f["means2D"], f["depths"], W, H)
    hb["dev"] = {k: _dev(hb[k]) for k in ("order", "point_list", "ranges", "tile_ids")}
    return hb


def _frame_keys(f, min_depth, max_depth):
    """(keys by id with the invisible key filled in, invisible key) of a forward's own radii and depths"""
    base, inv, _ = dc.key_frame(min_depth, max_depth)
    bits = np.ascontiguousarray(f["depths"].cpu().numpy(), np.float32).view(np.uint32).astype(np.int64)
    return np.where(f["radii"].cpu().numpy() > 0, (bits - base) & 0xFFFFFFFF, inv), inv


def _applies(P, W, H, min_depth, max_depth):
    return W <= 255 * 16 and H <= 255 * 16 and dc.depth_sort_msd_applies(P, dc.key_frame(min_depth, max_depth)[2])


def _check(f, hb, what, materialised=True):
    R, want = f["num_rendered"], hb["dev"]
    assert f["rc"] == 0 and hb["R"] == R, (what, f.get("error"), hb["R"], R)
    assert f["asked"] == f["expected_bytes"], (what, f["asked"], f["expected_bytes"])
    _equal(f["depth_order"], want["order"], f"{what}: depth_order")
    _equal(f["point_list"][:R], want["point_list"], f"{what}: point_list")
    _equal(f["ranges"], want["ranges"], f"{what}: ranges")
    if materialised:
        _equal(f["tile_ids"][:R], want["tile_ids"], f"{what}: sorted tile ids")
    f["bufs"].assert_guards_intact()


def _run_matrix(name, ins, st, variants, bufs=None, first_state="ones"):
    """the LSD variant, then every (label, options, asynchronous) of `variants` on the same buffers; returns the last forward"""
    from ex4dgs_amd import _C
    W, H, lo, hi = st["image_width"], st["image_height"], st["min_depth"], st["max_depth"]
    P = int(ins["means3D"].shape[0])
    applies = _applies(P, W, H, lo, hi)
    bufs = raw_abi.Buffers() if bufs is None else bufs
    with table.options(LSD):
        lsd = raw_abi.forward(ins, st, bufs, fill="zero", state_fill=first_state)
    assert lsd["rc"] == 0, lsd["error"]
    hb = _expected(lsd, W, H)
    _check(lsd, hb, f"{name} / lsd")
    ref = {k: _bits(lsd[k]).clone() for k in OUTPUTS}
    keys, inv = _frame_keys(lsd, lo, hi)
    R = lsd["num_rendered"]
    f = lsd
    for label, opts, asyn in variants:
        what = f"{name} / {label}"
        with table.options(opts):                          # (setting "depth_sort_sample" clears the frame counter)
            _C.sample_sort_stats(reset=True)
            f = raw_abi.forward(ins, st, bufs, fill="zero", state_fill="stale", instance_capacity=R + 1 if asyn else 0)
            frames, census = _C.get_option("depth_sort_sample_frames"), _C.sample_sort_stats(reset=True)
        _check(f, hb, what)
        if asyn:
            assert f["status"][0] == R and f["status"][1] == 0, (what, f["status"])
        for k in OUTPUTS:
            assert torch.equal(_bits(f[k]), ref[k]), f"{what}: {k} differs from the LSD variant's"
        assert frames == (1 if applies else 0), (what, frames)
        if applies:
            order, want, _ = sc.restate(keys, inv, opts)
            assert census == want, (what, census, want)
        else:
            assert not any(census.values()), (what, census)
    return f, keys, inv


@pytest.mark.parametrize("name", dc.FRAME_NAMES)
def test_depth_sort_frames_on_the_sample_sort(hip_lib, name):
    fr = dc.frame(name)
    ins, st = dc.scene(name)
    ins = {k: v.cuda() for k, v in ins.items()}
    f, keys, inv = _run_matrix(name, ins, st, MATRIX)
    d = dc.designed(fr)
    vis = f["radii"] > 0
    _equal(_bits(f["depths"])[vis], _dev(d["z_by_id"].view(np.int32))[vis], f"{name}: depths vs the designed bit patterns")


@pytest.mark.parametrize("name", sc.FRAME_NAMES)
def test_designed_frames_on_the_sample_sort(hip_lib, name):
    fr = sc.frame(name)
    ins, st = dc.scene_of(fr)
    ins = {k: v.cuda() for k, v in ins.items()}
    extra = [(f"rows={r}, {o}", dict(SAMPLE, tile_sort_rows=r, **o), 0) for o in sc.option_sets(name)[1:] for r in (1, 0)]
    f, keys, inv = _run_matrix(name, ins, st, MATRIX + extra)
    want, winv = sc.designed_keys(fr)
    assert inv == winv and np.array_equal(keys, want), f"{name}: the frame's keys are not the designed ones"
    for opts in sc.option_sets(name):
        memory = sc.restate(keys, inv, opts)[1]["memory"]
        assert (memory > 0) == ((name, opts) in sc.MEMORY_DESIGNED), (name, opts, memory)


def test_walls_cost_no_trip_and_no_bucket_through_memory(hip_lib):
    """The exact-tie wall of the buffer-contract table and the near-tie wall, one after the other on the same buffers, under the default
    "depth_sort_msd" = 3: no bucket through memory, and the auto mode's word stays untouched -- no trip after the frames that follow"""
    from ex4dgs_amd import _C
    bufs = raw_abi.Buffers()
    wall_ins, wall_st = table._scene(table.WALL)
    near_ins, near_st = dc.scene_of(sc.frame("wall_near"))
    opts = dict(SAMPLE, depth_sort_msd=3)
    variants = [("rows, frame 1", opts, 0), ("rows, frame 2", opts, 0), ("pairs, async", dict(opts, tile_sort_rows=0), 1)]
    for n, (name, ins, st) in enumerate([("table wall", wall_ins, wall_st), ("wall_near", near_ins, near_st), ("table wall again", wall_ins, wall_st)]):
        ins = {k: v.cuda() for k, v in ins.items()}
        f, keys, inv = _run_matrix(name, ins, st, variants, bufs=bufs, first_state="ones" if n == 0 else "stale")
        _, census, _ = sc.restate(keys, inv, opts)
        assert census["memory"] == 0 and census["largest"] <= sc.capacity(512), (name, census)
        if n == 0:
            # (14000 Gaussians at one depth, those the frustum keeps: more than any bucket kernel finishes in LDS)
            assert int(np.unique(keys[keys != inv], return_counts=True)[1].max()) > sc.capacity(512), "the table's wall does not exceed the capacity"
    with table.options(opts):
        for ins, st in ((wall_ins, wall_st), (near_ins, near_st), (wall_ins, wall_st)):
            f = raw_abi.forward({k: v.cuda() for k, v in ins.items()}, st, bufs, fill="zero", state_fill="stale")
            assert f["rc"] == 0, f["error"]
        assert (_C.get_option("depth_sort_trips"), _C.get_option("depth_sort_hold"), _C.get_option("depth_sort_sample_frames")) == (0, 0, 3)


def test_option_off_counts_no_frame(hip_lib):
    from ex4dgs_amd import _C
    ins, st = dc.scene_of(sc.frame("p_65"))
    ins = {k: v.cuda() for k, v in ins.items()}
    with table.options(dict(depth_sort_sample=0, depth_sort_sample_stats=1)):
        _C.sample_sort_stats(reset=True)
        f = raw_abi.forward(ins, st, raw_abi.Buffers(), fill="zero", state_fill="ones")
        assert f["rc"] == 0 and _C.get_option("depth_sort_sample_frames") == 0 and not any(_C.sample_sort_stats().values())
    with table.options(dict(depth_sort_sample=1)):
        f = raw_abi.forward(ins, st, raw_abi.Buffers(), fill="zero", state_fill="ones")
        assert f["rc"] == 0 and _C.get_option("depth_sort_sample_frames") == 1


def _wall_at(ins, ids, z):
    """means3D with the Gaussians `ids` moved to depth z along their view rays (identity view: same image position)"""
    m = ins["means3D"].clone()
    m[ids] = m[ids] * (z / m[ids, 2]).unsqueeze(1)
    m[ids, 2] = z
    return m.contiguous()


def test_a_captured_forward_takes_the_sample_sort_and_replays(hip_lib):
    """One asynchronous forward captured into a hipGraph with the option on; replayed three times with means3D rewritten in place, a
    wall of 8000 of 20000 Gaussians moving in depth: each replay equals an eager LSD frame on the same inputs"""
    from ex4dgs_amd import _C
    from tests.test_gpu_round4 import _raw_forward
    ins, st = h.scene_inputs("cfg2", P=20000, dir_scale=0.0)
    ins = {k: v.cuda() for k, v in ins.items()}
    P = 20000
    ids = torch.randperm(P, generator=torch.Generator().manual_seed(3))[:8000].cuda()
    with table.options(LSD):
        s, sync = _raw_forward(dict(ins, means3D=_wall_at(ins, ids, 5.0)), st)
    cap = 2 * int(sync[0]) + 100000
    static = {k: v.clone() for k, v in ins.items()}
    with table.options(dict(depth_sort_sample=1)):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _raw_forward(static, st, settings=s, instance_capacity=cap, assume_no_flow=True)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        before = _C.get_option("depth_sort_sample_frames")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            _, fwd = _raw_forward(static, st, settings=s, instance_capacity=cap, assume_no_flow=True)
        assert _C.get_option("depth_sort_sample_frames") == before + 1, "the captured call did not take the sample sort"
        assert (_C.get_option("depth_sort_trips"), _C.get_option("depth_sort_hold")) == (0, 0)
    for z in (6.0, 9.5, 41.0):
        moved = _wall_at(ins, ids, z)
        static["means3D"].copy_(moved)
        g.replay()
        torch.cuda.synchronize()
        with table.options(LSD):
            _, ref = _raw_forward(dict(ins, means3D=moved), st)
        assert fwd[0].wait().num_rendered == ref[0] and fwd[0].valid, (z, ref[0])
        for i in (1, 2, 6, 7, 8, 9):
            assert torch.equal(_bits(fwd[i]), _bits(ref[i])), f"wall at {z}: output {i} differs from the eager LSD frame's"
        assert torch.equal(_C.geom_views(fwd[3], P)["depth_order"], _C.geom_views(ref[3], P)["depth_order"]), f"wall at {z}: depth order"
