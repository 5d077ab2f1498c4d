"""The tile sorts at every instantiation and edge, against a host sort (run with `-m gpu` on an MI355X).

Every case of tests/binning_cases.py goes through tests/raw_abi.forward on guarded, zero-filled buffers under every option set
(tile_sort_rows x depth_sort_msd, ranking by ballots once per tile-sort chain) and capacity (synchronous; asynchronous at R, R + 1 and on
either side of the row-segment sort's stage choice) that selects another kernel chain.  From the frame's OWN radii, means2D and depths
the host restatement (binning_cases.host_binning: a stable sort, nothing else) gives the depth order, the point list, the tile ranges
and the sorted tile ids the frame must hold, exactly; the radii, tiles_touched and the instance count equal the CPU oracle's, so the
restatement is fed the rects the case was designed for; and the census, recomputed from the frame's own depth order and rects, names
the cells tests/test_cpu_binning_cases.py showed to cover every instantiation and per-block path."""
import numpy as np
import pytest
import torch

from tests import binning_cases as bc
from tests import raw_abi
from tests import test_gpu_buffer_contract as table
from tests.test_cpu_buffer_contract import path_signature

pytestmark = pytest.mark.gpu


def _forward(name, opts, cap, bufs):
    """one frame; every option of BASE_OPTIONS is set for it and restored in the context manager's exit"""
    ins, st = bc.scene(name)
    with table.options(opts):
        f = raw_abi.forward(ins, st, bufs, fill="zero", instance_capacity=int(cap or 0))
    assert f["rc"] == 0, f["error"]
    assert f["asked"] == f["expected_bytes"], (f["asked"], f["expected_bytes"])
    return f


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).cuda()


def _expected(f, W, H, **kw):
    hb = bc.host_binning(f["radii"], f["means2D"], f["depths"], W, H, **kw)
    hb["dev"] = {k: _dev(hb[k]) for k in ("order", "point_list", "ranges", "tile_ids")}
    return hb


def _first_difference(got, want):
    bad = (got != want).reshape(got.shape[0], -1).any(1).nonzero()
    i = int(bad[0])
    return f"{int(bad.numel())} of {got.shape[0]} differ, first at {i}: got {got[i].tolist()}, expected {want[i].tolist()}"


def _assert_equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.equal(got, want), f"{what}: {_first_difference(got, want)}"


@pytest.mark.parametrize("name", bc.CASE_NAMES)
def test_frames_equal_the_host_restatement(hip_lib, name):
    o = bc.oracle_of(name)
    P, W, H, R = o["P"], o["W"], o["H"], o["num_rendered"]
    promised = bc.promised(name)
    o_radii = _dev(o["radii"])
    bufs = raw_abi.Buffers()
    ref = None                         # (visible mask, means2D, depths, restatement) of the first frame
    for i, (label, opts, cap) in enumerate(bc.frames(P, W, H, R)):
        what = f"{name} / {label}"
        opts = dict(opts, geom_debug_arrays=1) if i == 0 else opts
        f = _forward(name, opts, cap, bufs)
        # ---- the frame against the oracle: the rects the case was designed for
        _assert_equal(f["radii"], o_radii, f"{what}: radii vs the oracle")
        assert f["num_rendered"] == R, (what, f["num_rendered"], R)
        if i == 0:
            _assert_equal(f["tiles_touched"], _dev(o["tiles_touched"]), f"{what}: tiles_touched vs the oracle")
        if cap is not None:
            assert f["status"][0] == R and R <= cap and f["status"][1] == 0, (what, f["status"])
        # ---- the frame against the restatement of its own radii, means2D and depths
        vis = f["radii"] > 0
        if ref is None or not (torch.equal(f["means2D"][vis], ref[1]) and torch.equal(f["depths"][vis], ref[2])):
            ref = (vis, f["means2D"][vis].clone(), f["depths"][vis].clone(), _expected(f, W, H))
        hb = ref[3]
        want = hb["dev"]
        assert hb["R"] == R
        _assert_equal(f["depth_order"], want["order"], f"{what}: depth_order")
        _assert_equal(f["point_list"][:R], want["point_list"], f"{what}: point_list")
        _assert_equal(f["ranges"], want["ranges"], f"{what}: ranges")
        if dict(table.BASE_OPTIONS, **opts)["binning_tile_ids"]:
            _assert_equal(f["tile_ids"][:R], want["tile_ids"], f"{what}: sorted tile ids")
        bufs.assert_guards_intact()
        # ---- the census of the frame's own depth order and rects: the cells the CPU test promised
        got = bc.census(P, W, H, f["depth_order"].cpu().numpy(), hb["rects"], dict(table.BASE_OPTIONS, **opts), cap)
        assert got == promised[label], (what, sorted(got ^ promised[label]))


@pytest.mark.parametrize("short", [1, bc.RS_CHUNK + 1], ids=["one_short", "a_block_and_one_short"])
@pytest.mark.parametrize("name,chain", bc.SHORT_CASES, ids=[f"{n}-{c.replace(' ', '_')}" for n, c in bc.SHORT_CASES])
def test_a_capacity_short_of_the_instances(hip_lib, name, chain, short):
    """An asynchronous frame whose capacity is one instance (and: one pass-B block and one instance) short, through each of the three
    tile sorts: the status reports R -- overflowed, not valid --, the outputs are finite, every guard is intact, and the list and
    the ranges are those of the stream the tile sort reads, cut at the capacity (binning_cases.host_binning, capacity=)."""
    o = bc.oracle_of(name)
    P, W, H, R = o["P"], o["W"], o["H"], o["num_rendered"]
    cap = R - short
    assert cap > bc.RS_CHUNK                                               # more than one block is left
    opts = dict(tile_sort_rows=int(chain == "rows"), depth_sort_msd=2, binning_tile_ids=1)
    assert path_signature(P, W, H, bc.MIN_DEPTH, bc.MAX_DEPTH, dict(table.BASE_OPTIONS, **opts), True)[3] == chain
    bufs = raw_abi.Buffers()
    f = _forward(name, opts, cap, bufs)
    assert f["status"][0] == R and f["status"][0] > cap, f["status"]       # num_rendered > capacity: overflowed, the frame is not valid
    for k in ("color", "depth", "acc", "flow"):
        assert bool(torch.isfinite(f[k]).all()), k
    bufs.assert_guards_intact()
    _assert_equal(f["radii"], _dev(o["radii"]), "radii vs the oracle")
    hb = _expected(f, W, H, capacity=cap, form="rows" if chain == "rows" else "pair")
    assert hb["R"] == R and hb["kept"] == cap
    _assert_equal(f["depth_order"], hb["dev"]["order"], "depth_order")
    _assert_equal(f["point_list"][:cap], hb["dev"]["point_list"], f"point_list[:{cap}]")
    _assert_equal(f["ranges"], hb["dev"]["ranges"], "ranges")
    _assert_equal(f["tile_ids"][:cap], hb["dev"]["tile_ids"], "sorted tile ids")
    if short == 1:
        got = bc.census(P, W, H, f["depth_order"].cpu().numpy(), hb["rects"], dict(table.BASE_OPTIONS, **opts), cap)
        assert "cap.R_minus_1" in got
