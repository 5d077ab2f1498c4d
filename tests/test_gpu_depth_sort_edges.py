"""The depth sorts at every key width, digit split and bucket edge, against a host sort (run with `-m gpu` on an MI355X).

Every frame of tests/depth_sort_cases.py goes through tests/raw_abi.forward on guarded buffers, once per option set that selects
another kernel chain or another path inside one (depth_sort_cases.option_sets: LSD / MSD / MSD with the scan kernel, row-segment or
pair tile sort, digit width, workgroup size, local capacity, ranking by ballots, asynchronous frames).  The state buffers hold 0xFF
bytes for the first frame and what the frame before left for every other one: stale bucket sums, starts and histograms are what a
frame finds.  big_grid, whose point is the zero fill of 8704 tile ranges that rides in the LSD sort's last pass, in the bucket kernel
and in the scan kernel, starts every variant from 0xFF bytes: every range must be (0, 0) or correct.  All comparisons are exact:
radii and the instance count equal the CPU oracle's, the depths are the designed bit patterns, the depth order, the point list, the tile ranges and the sorted tile ids are the restatement's
(binning_cases.host_binning on the frame's own radii, means2D and depths), the six outputs of every variant are bit-equal to the LSD
variant's, every guard is intact, and the census recomputed from the frame's own keys is what tests/test_cpu_depth_sort_cases.py
showed to cover every reachable cell."""
import numpy as np
import pytest
import torch

from tests import binning_cases as bc
from tests import depth_sort_cases as dc
from tests import raw_abi
from tests import test_gpu_buffer_contract as table

pytestmark = pytest.mark.gpu

OUTPUTS = ("color", "radii", "depth", "acc", "flow", "idx")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _first_difference(got, want):
    bad = (got != want).reshape(got.shape[0], -1).any(1).nonzero()
    i = int(bad[0])
    return f"{int(bad.numel())} of {got.shape[0]} differ, first at {i}: got {got[i].tolist()}, expected {want[i].tolist()}"


def _assert_equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.equal(got, want), f"{what}: {_first_difference(got, want)}"


def _expected(f, W, H):
    hb = bc.host_binning(f["radii"], f["means2D"], f["depths"], W, H)
    hb["dev"] = {k: _dev(hb[k]) for k in ("order", "point_list", "ranges", "tile_ids")}
    return hb


def _check_against_restatement(f, hb, R, materialised, what):
    want = hb["dev"]
    assert hb["R"] == R
    _assert_equal(f["depth_order"], want["order"], f"{what}: depth_order")
    _assert_equal(f["point_list"][:R], want["point_list"], f"{what}: point_list")
    _assert_equal(f["ranges"], want["ranges"], f"{what}: ranges")
    if materialised:
        _assert_equal(f["tile_ids"][:R], want["tile_ids"], f"{what}: sorted tile ids")


@pytest.mark.parametrize("name", dc.FRAME_NAMES)
def test_frames_equal_the_host_restatement(hip_lib, name):
    fr = dc.frame(name)
    d, o = dc.designed(fr), dc.oracle_of(name)
    P, W, H, R = d["P"], fr.W, fr.H, o["num_rendered"]
    promised = dc.promised(name)
    ins, st = dc.scene(name)
    ins = {k: v.cuda() for k, v in ins.items()}
    o_radii, z_bits = _dev(o["radii"]), _dev(d["z_by_id"].view(np.int32))
    sets = dc.option_sets(fr, dc.keys_of(fr, o["radii"], o["depths"]))
    assert sets[0][1]["depth_sort_msd"] == 0 and not sets[0][2], "the LSD variant comes first: the others are compared with it"
    bufs = raw_abi.Buffers()
    ref, lsd = None, None
    for i, (label, opts, asyn, _) in enumerate(sets):
        what = f"{name} / {label}"
        cap = R + 1 if asyn else 0
        with table.options(opts):
            # (FRESH_STATE: a stale state holds this very frame's tile ranges -- a zero fill that did not happen would not show)
            state = "ones" if i == 0 or name in dc.FRESH_STATE else "stale"
            f = raw_abi.forward(ins, st, bufs, fill="zero", state_fill=state, instance_capacity=cap)
        assert f["rc"] == 0, (what, f["error"])
        assert f["asked"] == f["expected_bytes"], (what, f["asked"], f["expected_bytes"])
        # ---- the frame against the oracle and the design
        _assert_equal(f["radii"], o_radii, f"{what}: radii vs the oracle")
        assert f["num_rendered"] == R, (what, f["num_rendered"], R)
        if asyn:
            assert f["status"][0] == R and f["status"][1] == 0, (what, f["status"])
        vis = f["radii"] > 0
        _assert_equal(_bits(f["depths"])[vis], z_bits[vis], f"{what}: depths vs the designed bit patterns")
        # ---- the frame against the restatement of its own radii, means2D and depths
        if ref is None or not (torch.equal(f["means2D"][vis], ref[0]) and torch.equal(f["depths"][vis], ref[1])):
            ref = (f["means2D"][vis].clone(), f["depths"][vis].clone(), _expected(f, W, H))
        hb = ref[2]
        _check_against_restatement(f, hb, R, dict(table.BASE_OPTIONS, **opts)["binning_tile_ids"], what)
        # ---- every variant against the LSD variant
        if lsd is None:
            lsd = {k: _bits(f[k]).clone() for k in OUTPUTS}
        for k in OUTPUTS:
            assert torch.equal(_bits(f[k]), lsd[k]), f"{what}: {k} differs from the LSD variant's"
        bufs.assert_guards_intact()
        # ---- the census of the frame's own keys: the cells the CPU test promised
        got = dc.census(fr, dc.keys_of(fr, f["radii"].cpu().numpy(), f["depths"].cpu().numpy()), dict(table.BASE_OPTIONS, **opts), asyn)
        assert got == promised[label], (what, sorted(got ^ promised[label]))


@pytest.mark.parametrize("threads", [256, 512])
def test_auto_mode_at_the_capacity_and_one_beyond(hip_lib, threads):
    """depth_sort_msd = 3 (the default): a frame whose largest bucket is exactly the bucket kernel's capacity raises nothing -- after the
    frame that follows it no trip is counted; one Gaussian more in that bucket and the following frame counts one trip and holds the LSD
    sort for 63 more frames.  Both frames equal the restatement whichever sort ran."""
    from ex4dgs_amd import _C
    saved = {k: _C.get_option(k) for k in table.BASE_OPTIONS}
    try:
        for extra, want in ((0, (0, 0)), (1, (1, 63))):
            fr = dc.auto_edge(threads, extra)
            ins, st = dc.scene_of(fr)
            ins = {k: v.cuda() for k, v in ins.items()}
            for k, v in dict(table.BASE_OPTIONS, depth_sort_local_threads=threads, tile_sort_rows=0, binning_tile_ids=1).items():
                _C.set_option(k, v)                               # (setting "depth_sort_msd" resets the hold and the counters)
            assert _C.get_option("depth_sort_msd") == 3 and _C.get_option("depth_sort_trips") == 0 and _C.get_option("depth_sort_hold") == 0
            bufs = raw_abi.Buffers()
            hb = None
            for n in range(2):
                what = f"{fr.name}, frame {n}"
                f = raw_abi.forward(ins, st, bufs, fill="zero", state_fill="ones" if n == 0 else "stale")
                assert f["rc"] == 0, (what, f["error"])
                if n == 0:
                    assert _C.get_option("depth_sort_trips") == 0, "the host looks at the report when the next frame starts"
                    hb = _expected(f, fr.W, fr.H)
                    keys = dc.keys_of(fr, f["radii"].cpu().numpy(), f["depths"].cpu().numpy())
                    k = keys[keys >= 0]
                    assert k.size == int((fr.keys >= 0).sum())
                    assert np.bincount((k - k.min()) >> dc.msd_shift(int(k.max() - k.min()), 9)).max() == threads * dc.DLS_ITEMS + extra
                _check_against_restatement(f, hb, f["num_rendered"], True, what)
                bufs.assert_guards_intact()
            assert (_C.get_option("depth_sort_trips"), _C.get_option("depth_sort_hold")) == want, (fr.name, want)
    finally:
        for k, v in saved.items():
            _C.set_option(k, v)
