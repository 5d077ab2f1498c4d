"""The frames of tests/test_gpu_depth_sort_edges.py, without a GPU: every frame of tests/depth_sort_cases.py realises its plan on the
CPU oracle (depths bit for bit, visibility, rects, and the oracle's lists equal the restatement's -- the unsigned stable host sort and
the reference's 64-bit key sort agree, ties included); the frames reach every cell of the census the host rules make reachable, and
the rules exclude what they are there to exclude; the constants the census restates are those of the sources; the scene builder
factored out of tests/binning_cases.py builds the scenes it built before."""
import os
import re

import numpy as np
import pytest
import torch

from ex4dgs_amd.scene import SceneConfig
from tests import binning_cases as bc
from tests import depth_sort_cases as dc
from tests import helpers as h
from tests.test_cpu_buffer_contract import DLS_IDX_BITS, DLS_MSD_BITS, key_bits
from tests.test_gpu_buffer_contract import BASE_OPTIONS

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ex4dgs_amd", "csrc")


def _u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def negative_depths_rendered():
    """does the CPU oracle render the rows of wide_planes_32 whose depth is below zero?  (all of them or none)"""
    fr = dc.frame("wide_planes_32")
    d, o = dc.designed(fr), dc.oracle_of("wide_planes_32")
    r = o["radii"][d["uncertain_by_id"]] > 0
    assert r.all() or not r.any(), r
    return bool(r.all())


@pytest.mark.parametrize("name", dc.FRAME_NAMES)
def test_frames_realise_their_plan_on_the_oracle(name):
    fr = dc.frame(name)
    d, o = dc.designed(fr), dc.oracle_of(name)
    P = d["P"]
    assert o["P"] == P and key_bits(fr.min_depth, fr.max_depth) == d["key_bits"]
    planned = d["keys_by_id"] >= 0
    unc = d["uncertain_by_id"]
    if unc.any():
        rendered = negative_depths_rendered()
        print(f"{name}: the oracle {'renders' if rendered else 'culls'} the {int(unc.sum())} rows with a depth below zero")
        planned = planned & (rendered | ~unc)
    # ---- depths bit for bit, visibility, rects
    vis = o["radii"] > 0
    assert np.array_equal(vis, planned), f"{int((vis != planned).sum())} rows whose visibility is not the planned one"
    assert np.array_equal(_u32(o["depths"])[vis], _u32(d["z_by_id"])[vis]), "a depth that is not the designed bit pattern"
    keys = dc.keys_of(fr, o["radii"], o["depths"])
    assert np.array_equal(keys[planned], d["keys_by_id"][planned]) and (keys[~planned] == -1).all()
    rects = bc.rects_of(o["radii"], o["means2D"], fr.W, fr.H)
    want = dc.designed_rects(fr, d)
    want[~planned] = 0
    assert np.array_equal(rects, want), f"{int((rects != want).any(1).sum())} rects are not the designed ones"
    # ---- the oracle's lists are the restatement's
    hb = bc.host_binning(o["radii"], o["means2D"], o["depths"], fr.W, fr.H)
    assert hb["R"] == o["num_rendered"]
    assert np.array_equal(hb["tiles_touched"], o["tiles_touched"].astype(np.int64))
    assert np.array_equal(hb["point_list"], o["point_list"].astype(np.int64)), "the unsigned stable host sort and the oracle's 64-bit key sort disagree"
    assert np.array_equal(hb["tile_ids"], (o["keys_sorted"] >> np.uint64(32)).astype(np.int64))
    assert np.array_equal(hb["ranges"], o["ranges"].astype(np.int64))
    # (a full-image rect is in tile 0: the third of the visible rows that has one is listed there in the depth order)
    order_vis = hb["order"][: int(vis.sum())]
    in_tile0 = order_vis[(rects[order_vis, 0] == 0) & (rects[order_vis, 1] == 0) & (rects[order_vis, 2] > 0)]
    s, e = hb["ranges"][0]
    assert np.array_equal(o["point_list"][s:e].astype(np.int64), in_tile0)
    # ---- the order itself: ascending unsigned depth bits, ties in ascending id, invisible rows behind in id order
    ko = keys[hb["order"]]
    nv = int(vis.sum())
    assert (np.diff(ko[:nv]) >= 0).all() and (ko[nv:] == -1).all() and (np.diff(hb["order"][nv:]) > 0).all()
    assert (np.diff(hb["order"][:nv])[np.diff(ko[:nv]) == 0] > 0).all()
    if unc.any() and negative_depths_rendered():
        tail = hb["order"][nv - int(unc.sum()): nv]
        assert unc[tail].all() and (np.diff(d["z_by_id"][tail]) <= 0).all(), "depths below zero sort behind every positive one, descending"


def test_equal_keys_come_in_runs_whose_ids_do_not_ascend():
    """a sort that is not stable shows: the designed order holds runs of equal keys, and inside most of them the ids do not ascend"""
    for name in ("bucket_edges_a", "bucket_edges_b", "bucket_edges_c", "rem_ladder_16", "span27_full"):
        fr = dc.frame(name)
        ids = dc.ids_of(fr)
        same = (fr.keys[1:] == fr.keys[:-1]) & (fr.keys[1:] >= 0)
        assert same.sum() > 50 and (np.diff(ids)[same] < 0).sum() > same.sum() // 4, name
        if name.startswith("bucket"):
            runs = 1 + int((~same).sum())
            assert runs > 300


def test_the_frames_reach_every_reachable_cell():
    reachable, excluded = dc.reachable_cells()
    reached, labels = {}, set()
    for name in dc.FRAME_NAMES:
        per = dc.promised(name)
        labels |= set(per)
        mine = set().union(*per.values())
        new = sorted(mine - set(reached))
        for c in mine:
            reached.setdefault(c, []).append(name)
        fr = dc.frame(name)
        print(f"{name}: P={fr.keys.size} key bits {key_bits(fr.min_depth, fr.max_depth)} frames={len(per)} cells={len(mine)} first here: {', '.join(new) or '-'}")
    unknown = set(reached) - reachable
    assert not unknown, f"cells the host rules do not make reachable, or unnamed: {sorted(unknown)}"
    missing = sorted(reachable - set(reached))
    assert not missing, f"{len(missing)} reachable cells no frame reaches: {missing}"
    # what the rules are there to exclude, shown excluded by the same computation
    for c in ("msd.rem.9.20", "msd.rem.10.20", "msd.digit.9.at.28", "msd.digit.10.at.29"):
        assert c in excluded and c not in reachable, c
    assert not excluded & set(reached)
    assert not any(c.endswith(".20") for c in reachable)
    # every option set of the GPU test ran on some frame
    every = {l for l, _ in dc.CHAINS + dc.PATHS + dc.BALLOTS} | {l + ", asynchronous" for l, _ in dc.ASYNC}
    assert labels == every, sorted(every - labels)


def test_the_rem_ladder_reaches_every_rem_the_rules_allow():
    """9-bit digit: every rem in 0..19; forced 10 bits at 27 key bits: every rem up to what the widest range leaves -- both sets derived
    from the host rule"""
    kb = key_bits(*dc.PLANES27)
    assert kb == 27 and dc.depth_sort_msd_bits(1, kb) == 9
    got = {9: set(), 10: set()}
    for r in range(21):
        fr = dc.frame(f"rem_ladder_{r}")
        k = fr.keys[fr.keys >= 0]
        for bits in (9, 10):
            got[bits].add(dc.msd_shift(int(k.max() - k.min()), bits))
    widest = (1 << kb) - 3
    for bits in (9, 10):
        assert got[bits] == set(range(dc.msd_shift(widest, bits) + 1)), (bits, sorted(got[bits]))
    assert max(got[9]) == 19 and max(got[9]) + dc.IDX_BITS[512] == 32
    # rem 16 and 17: the top remaining bit set in some rows and clear in others, inside one bucket
    for r in (16, 17):
        fr = dc.frame(f"rem_ladder_{r}")
        k = fr.keys[fr.keys >= 0]
        low = (k - k.min()) & ((1 << r) - 1)
        first = ((k - k.min()) >> r) == 0
        assert (low[first] >> (r - 1) == 1).sum() > 10 and (low[first] >> (r - 1) == 0).sum() > 10


def test_planes_and_key_widths():
    assert key_bits(*dc.PLANES27) == 27 and key_bits(*dc.PLANES28) == 28 and key_bits(*dc.PLANES26) == 26
    assert [key_bits(*dc.planes_of_bits(4.0, u)) for u in (100, 510, 511, 131071)] == [7, 9, 10, 18]
    assert [dc.lsd_passes(b) for b in (7, 9, 10, 18, 26, 27, 28, 31, 32)] == [[7], [9], [5, 5], [9, 9], [9, 9, 8], [9, 9, 9], [7, 7, 7, 7], [8, 8, 8, 7], [8, 8, 8, 8]]
    for kb in range(2, 31):
        fr = dc.frame(f"key_width_{kb}")
        assert key_bits(fr.min_depth, fr.max_depth) == kb and 0.0 < fr.min_depth < fr.max_depth == 256.0
    assert key_bits(0.0, 300.0) == 31 and key_bits(-1.0, 3.4e38) == 32 and dc.key_frame(-1.0, 3.4e38)[:2] == (0, 0xFFFFFFFF)
    assert [dc.bucket_pass_widths(r) for r in (9, 10, 16, 17, 19)] == [[9], [5, 5], [8, 8], [9, 8], [7, 6, 6]]


def test_bucket_edges_sit_on_the_capacities():
    """the census of bucket_edges under 256 and 512 threads says which buckets are at, under or over the capacity"""
    per = dict(dc.promised("bucket_edges_a"))
    per.update({"b: " + k: v for k, v in dc.promised("bucket_edges_b").items()})
    per.update({"c: " + k: v for k, v in dc.promised("bucket_edges_c").items()})
    t256 = set().union(*(v for v in per.values() if "msd.threads.256" in v))
    t512 = set().union(*(v for v in per.values() if "msd.threads.512" in v))
    for T, cells in ((256, t256), (512, t512)):
        for c in ("n_lt_64", "n_eq_64_waves", "partial_last_wave", "n_eq_cap"):
            assert f"bucket.lds.{T}.{c}" in cells, (T, c)
        assert f"bucket.mem.{T}.n_eq_cap_plus_1" in cells and f"bucket.scan.{T}.chunks_ge_2" in cells
    for threads in (256, 512):
        for extra in (0, 1):
            fr = dc.auto_edge(threads, extra)
            k = fr.keys[fr.keys >= 0]
            assert np.bincount((k - k.min()) >> dc.msd_shift(int(k.max() - k.min()), 9)).max() == threads * dc.DLS_ITEMS + extra


def test_big_grid_runs_every_kernel_that_clears_the_tile_ranges():
    """the zero fill of the tile ranges rides in the LSD sort's last pass (in front of the row-segment sort), in the scan kernel (LSD or
    MSD with the scan kernel, in front of a pair sort) and in the bucket kernel (MSD, fused scan or row-segment sort), under 256 and
    512 threads: big_grid, every variant of which starts from 0xFF state, has a variant for each, on a grid of 8704 tiles with 3
    Gaussians -- more tiles than one sweep of any of these grids covers"""
    fr = dc.frame("big_grid")
    assert "big_grid" in dc.FRESH_STATE and (fr.W // 16) * (fr.H // 16) == 8704 and fr.keys.size == 3
    # tiles without instances in both halves of the grid, in front of the first tile with instances and behind the last
    r = dc.oracle_of("big_grid")["ranges"].astype(np.int64)
    empty = (r == 0).all(1)
    full = np.flatnonzero(~empty)
    assert full.size == 1 + 16 + 4 and 0 < full[0] and full[-1] < 8703 and empty[:4352].sum() > 4000 and empty[4352:].sum() > 4000 and (full >= 4352).any() and (full < 4352).any()
    per = dc.promised("big_grid")
    chains = {(("lsd" if any(c.startswith("lsd.") for c in cells) else "msd"),
               next((c for c in cells if c.startswith(("lsd.gather.", "msd.scan."))), None),
               next((c for c in cells if c.startswith("msd.threads.")), None)) for cells in per.values()}
    want = {("lsd", "lsd.gather.1", None), ("lsd", "lsd.gather.0", None), ("msd", "msd.scan.fused", "msd.threads.256"),
            ("msd", "msd.scan.fused", "msd.threads.512"), ("msd", "msd.scan.none", "msd.threads.512"), ("msd", "msd.scan.kernel", "msd.threads.512")}
    assert want <= chains, sorted(want - chains, key=str)


def test_through_memory_passes_and_narrow_planes():
    """rem 9, 10 and 19 with a local capacity of 1 and of 64: one, two and three passes through memory, so odd and even; planes up to
    511 ulps apart: rem = 0 in every bucket of the MSD sort, one or two LSD passes"""
    for r, passes in ((9, 1), (10, 2), (19, 3)):
        per = dc.promised(f"rem_ladder_{r}")
        for cap in (1, 64):
            mine = [cells for label, cells in per.items() if f"9 bits, 512 threads, cap {cap}" in label]
            assert mine and all(f"bucket.mem.passes.{passes}" in cells and f"msd.rem.9.{r}" in cells and "msd.watch.raised" in cells for cells in mine), (r, cap)
    for ulps, widths in ((100, "g"), (510, "9"), (511, "g+g"), (131071, "9+9")):
        per = dc.promised(f"narrow_planes_{ulps}")
        assert f"lsd.scatter.{widths}" in per["lsd, rows"] and f"lsd.start_in_b.{len(widths.split('+')) & 1}" in per["lsd, rows"]
        msd = [cells for cells in per.values() if any(c.startswith("msd.rem.") for c in cells)]
        assert msd
        if ulps <= 511:
            assert all({c for c in cells if c.startswith("msd.rem.")} <= {"msd.rem.9.0", "msd.rem.10.0"} for cells in msd)
            assert not any(c.startswith(("bucket.lds.", "bucket.mem.")) for cells in msd for c in cells)


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, source):
    found = re.findall(pattern, source)
    assert len(found) == 1, (pattern, found)
    return found[0]


def test_the_census_constants_are_the_sources():
    b, i = _source("ex4d_binning.hip"), _source("ex4d_internal.h")
    assert int(_one(r"#define DLS_ITEMS (\d+)", b)) == dc.DLS_ITEMS
    assert _one(r"IDX_BITS = \(THREADS == 512 \? (\d+) : (\d+)\)", b) == (str(dc.IDX_BITS[512]), str(dc.IDX_BITS[256]))
    assert int(_one(r"#define DLS_IDX_BITS (\d+)", b)) == DLS_IDX_BITS == max(dc.IDX_BITS.values())
    assert int(_one(r"#define EX4D_DLS_MSD_BITS (\d+)", i)) == DLS_MSD_BITS == 10
    assert int(_one(r"#define RS_SMALL_ITEMS (\d+)", b)) == dc.RS_SMALL_ITEMS
    assert int(_one(r"#define RS_THREADS (\d+)", i)) == 256 and dc.PARTITION_BLOCK == dc.RS_SMALL_ITEMS * 256
    assert _one(r"for \(uint32_t base = 0; base < nranges; base \+= (\d+)u \* RS_THREADS\)", b) == str(dc.RANGE_TRIP // 256)
    assert _one(r"nranges = \(n \+ (\d+)u\) / (\d+)u;", b) == (str(dc.RANGE_PAIR - 1), str(dc.RANGE_PAIR))
    assert int(_one(r"n <= (\d+)u && key_bits - \(narrow - 1\)", b)) == dc.MSD_BITS_COUNT
    assert int(_one(r"n > (\d+)u\) \? 512 : 256", b)) == dc.THREADS_COUNT
    assert _one(r"rs_items_for\(uint32_t n\) \{ return n <= \((\d+)u << (\d+)\) \? RS_SMALL_ITEMS", b) == ("2", "20")
    assert _one(r"rs_max_bits_for\(uint32_t n\) \{ return rs_items_for\(n\) == RS_SMALL_ITEMS \? (\d+) : 8", b) == str(dc.LSD_MAX_DIGIT)
    assert _one(r"if \(rem == (\d+)\) \{ dls_lds_pass<THREADS, 8>", b) == "16" and _one(r"else if \(rem == (\d+)\) \{ dls_lds_pass<THREADS, 9>", b) == "17"


def test_profile_tool_names_the_stage_of_recorded_and_current_sort_kernels():
    """tools/pmc_traffic.py maps a kernel name to a stage by the first matching substring: the names the profiles up to round 6 recorded
    and the names of the folded kernels (digit rule as the last template argument) land in the same stages."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("pmc_traffic", os.path.join(os.path.dirname(CSRC), "..", "tools", "pmc_traffic.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    ns = "void (anonymous namespace)::"
    for name, stage in (("dls_histogram_kernel<8, 512>(unsigned int const*", "depth_sort_msd_histogram"),
                        ("rs_histogram_kernel<8, 512, 1, (anonymous namespace)::DigitRange<512> >(", "depth_sort_msd_histogram"),
                        ("rs_histogram_kernel<16, 1024, 1, (anonymous namespace)::DigitTable<1024> >(", "depth_sort_sample_histogram"),
                        ("rs_histogram_kernel<8, 512, 1>(", "depth_sort_histogram_pass"),
                        ("rs_histogram_kernel<8, 512, 1, (anonymous namespace)::DigitBits<0> >(", "depth_sort_histogram_pass"),
                        ("rs_histogram_kernel<16, 256, 8>(", "tile_sort_histogram_pass"),
                        ("rs_histogram_kernel<16, 256, 8, (anonymous namespace)::DigitBits<0> >(", "tile_sort_histogram_pass"),
                        ("rs_scatter_kernel<8, 512, 3, 9>(", "depth_sort_scatter_pass"),
                        ("rs_scatter_kernel<8, 512, 3, (anonymous namespace)::DigitRange<512> >(", "depth_sort_scatter_pass"),
                        ("rs_scatter_kernel<8, 512, 3, (anonymous namespace)::DigitTable<512> >(", "depth_sort_scatter_pass"),
                        ("rs_scatter_kernel<16, 1024, 3, 10>(", "depth_sort_scatter_pass"),
                        ("rs_scatter_kernel<16, 1024, 3, (anonymous namespace)::DigitTable<1024> >(", "depth_sort_scatter_pass"),
                        ("rs_scatter_kernel<16, 512, 3, (anonymous namespace)::DigitRange<512> >(", "depth_sort_scatter_pass"),
                        ("rs_scatter_kernel<16, 256, 0, (anonymous namespace)::DigitBits<0> >(", "depth_sort_scatter_pass"),
                        ("rs_scatter_kernel<16, 256, 1, (anonymous namespace)::DigitBits<6> >(", "tile_sort_scatter_pass"),
                        ("rs_histogram_kernel<16, 256, 1, (anonymous namespace)::DigitBits<0> >(", "depth_sort_histogram_pass"),
                        ("rs_scatter_kernel<16, 256, 2, 7>(", "tile_sort_scatter_pass"),
                        ("rs_scatter_kernel<16, 256, 2, (anonymous namespace)::DigitBits<7> >(", "tile_sort_scatter_pass"),
                        ("depth_local_sort_kernel<512>(", "depth_sort_bucket_pass"), ("ss_bucket_kernel<512>(", "depth_sort_bucket_pass"),
                        ("ss_splitter_kernel<512>(", "depth_sort_sample_splitters"), ("ts_histogram_kernel(", "tile_sort_histogram_pass_b")):
        assert tool.alias(ns + name) == stage, name


# ------------------------------------------------------------------------------------------------ the factored scene builder
def _scene_as_before(name):
    """binning_cases.scene as it was before build_scene was factored out of it, word for word"""
    c = bc.case(name)
    P = len(c.specs)
    focal = 16.0 * max(c.W, c.H)
    cfg = SceneConfig(f"binning case {name}", P, c.W, c.H, focal, seed=900 + bc.CASE_NAMES.index(name), min_depth=bc.MIN_DEPTH, max_depth=bc.MAX_DEPTH)
    ins, st = h.scene_inputs(cfg, P=P)
    ids = np.random.default_rng(7000 + bc.CASE_NAMES.index(name)).permutation(P)          # the id of the i-th designed Gaussian
    px, py, r, vis = (np.array([s[k] for s in c.specs], np.float64) for k in range(4))
    z = np.where(vis > 0, 5.0 + 0.01 * (np.arange(P) // 2), 1.0).astype(np.float32).astype(np.float64)
    var = np.maximum(((r - 0.5) / 3.0) ** 2 - (0.1 + 0.1 ** 0.5), 0.01)
    m = np.stack([(px + 0.5 - c.W / 2.0) * z / focal, (py + 0.5 - c.H / 2.0) * z / focal, z], -1)
    s = np.repeat((z / focal * np.sqrt(var))[:, None], 3, 1)
    op = np.where(r > 100, 1.0, 0.5)[:, None]
    for k, v in (("means3D", m), ("scales", s), ("opacities", op)):
        t = torch.zeros(ins[k].shape, dtype=torch.float32)
        t[torch.from_numpy(ids)] = torch.from_numpy(v.astype(np.float32))
        ins[k] = t.contiguous()
    ins["rotations"] = torch.tensor([1.0, 0.0, 0.0, 0.0]).repeat(P, 1).contiguous()
    return ins, st


@pytest.mark.parametrize("name", bc.CASE_NAMES)
def test_the_factored_builder_builds_the_binning_cases_as_before(name):
    (a, sa), (b, sb) = bc.scene(name), _scene_as_before(name)
    assert set(a) == set(b) and set(sa) == set(sb)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    for k in sa:
        assert torch.equal(sa[k], sb[k]) if torch.is_tensor(sa[k]) else sa[k] == sb[k], k


def test_signed_and_unsigned_host_orders_differ_only_below_zero():
    """binning_cases.host_depth_order views the depth bits as unsigned words: the same order as the signed view for positive depths,
    and the order of the library's 32-bit key (and of the reference's 64-bit one) for a visible depth below zero"""
    d = np.array([2.0, 1.0, 1.0, 3.0, 0.5], np.float32)
    r = np.array([1, 1, 1, 0, 1])
    assert bc.host_depth_order(r, d).tolist() == [4, 1, 2, 0, 3]
    d[0] = -0.5
    d[4] = -0.25
    assert bc.host_depth_order(r, d).tolist() == [1, 2, 4, 0, 3]
    assert BASE_OPTIONS["depth_sort_msd"] == 3
