"""The sample depth sort's rule on the CPU: tests/sample_sort_cases.py restates it in numpy; here the restated order is a stable sort on
every designed frame, the frames reach every cell of the census, the options behave as include/ex4d_rasterizer.h says, and the rule
keeps the bench scenes' buckets under the bucket kernel's capacity (profiles/sample_sort_census.json)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import depth_sort_cases as dc
from tests import sample_sort_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_FRAMES = sc.FRAME_NAMES + dc.FRAME_NAMES


def _frame(name):
    return sc.frame(name) if name in sc.FRAME_NAMES else dc.frame(name)


def _applies(fr):
    return dc.depth_sort_msd_applies(fr.keys.size, dc.key_frame(fr.min_depth, fr.max_depth)[2])


def test_the_capacity_is_derived():
    assert sc.capacity(256) == 4096 and sc.capacity(512) == 8192 and all(1 << dc.IDX_BITS[t] == sc.capacity(t) for t in (256, 512))
    assert sc.choice({}) == (512, 8192) and sc.choice(dict(depth_sort_local_threads=256, depth_sort_local_cap=64)) == (256, 64)


@pytest.mark.parametrize("name", ALL_FRAMES)
def test_the_restated_order_is_a_stable_sort(name):
    fr = _frame(name)
    if not _applies(fr):
        return                                   # (the planes leave the frame to the LSD sort: nothing of the rule runs)
    keys, inv = sc.designed_keys(fr)
    for opts in sc.option_sets(name) + [dict(depth_sort_local_threads=256)]:
        order, census, paths = sc.restate(keys, inv, opts)
        assert np.array_equal(order, np.argsort(keys, kind="stable")), (name, opts)
        assert sum(census[k] for k in ("empty", "skipped", "packed", "pairs", "memory")) == sc.bins_of(keys.size)


def test_the_table_gives_a_repeated_splitter_a_bucket_of_its_own():
    spl = np.array([5, 5, 9, 12, 12, 12, 40, 40], np.int64)
    ub, distinct = sc.bucket_table(spl)
    assert distinct == 4 and ub.tolist() == [10, 11, 19, 24, 25, 80, 81, 0xFFFFFFFF]
    assert sc.bucket_of(ub, [0, 4, 5, 6, 9, 10, 11, 12, 13, 39, 40]).tolist() == [0, 0, 1, 2, 2, 3, 3, 4, 5, 5, 6]


def test_splitters_follow_from_keys_count_and_invisible_key_alone():
    keys, inv = sc.designed_keys(sc.frame("wall_exact"))
    spl = sc.splitter_list(keys, inv)
    assert spl.size == 512 and (spl[1:] >= spl[:-1]).all() and spl[-2:].tolist() == [inv, inv]
    sample = np.sort(keys[::4])                  # P = 30000: stride ceil(30000 / 8192) = 4, 7500 samples
    assert sc.stride_of(30000) == 4 and sample.size == 7500 and spl[0] == sample[7500 // 511] and spl[509] == sample[510 * 7500 // 511]
    assert (spl == (1 << 23)).sum() > 200        # the wall: a repeated splitter, a bucket of its own
    big = np.arange(1400000)
    assert sc.bins_of(big.size) == 1024 and sc.splitter_list(big, 1 << 27).size == 1024


def test_the_frames_reach_every_census_cell():
    reached, memory_by = {}, []
    for name in ALL_FRAMES:
        fr = _frame(name)
        if not _applies(fr):
            continue
        keys, inv = sc.designed_keys(fr)
        for opts in sc.option_sets(name) if name in sc.FRAME_NAMES else [{}]:
            _, census, _ = sc.restate(keys, inv, opts)
            for k in ("empty", "skipped", "packed", "pairs", "memory"):
                if census[k]:
                    reached.setdefault(k, []).append(name)
            if census["memory"]:
                memory_by.append((name, opts))
                assert census["memory_gaussians"] > sc.choice(opts)[1]
    assert set(reached) == {"empty", "skipped", "packed", "pairs", "memory"}, sorted(reached)
    assert sorted(memory_by, key=str) == sorted(sc.MEMORY_DESIGNED, key=str), memory_by
    # the designed edges: ordinary buckets of exactly the capacity (in LDS) and of one more (through memory)
    keys, inv = sc.designed_keys(sc.frame("cap_edge_64_65"))
    for threads in (256, 512):
        opts = dict(depth_sort_local_cap=64, depth_sort_local_threads=threads)
        order, census, paths = sc.restate(keys, inv, opts)
        n_of = np.bincount(sc.bucket_of(sc.bucket_table(sc.splitter_list(keys, inv))[0], keys))
        assert sorted(int(n_of[b]) for b, p in paths.items() if p != "skipped") == [3, 64, 65]
        assert census["memory"] == 1 and census["memory_gaussians"] == 65 and census["largest"] == 65
    _, census, paths = sc.restate(*sc.designed_keys(sc.frame("periodic_with_the_stride")))
    assert census["largest"] == 8192 and census["memory"] == 0 and census["distinct_splitters"] == 2
    for wall in ("wall_exact", "wall_near", "two_walls"):
        assert sc.restate(*sc.designed_keys(sc.frame(wall)))[1]["memory"] == 0
    assert sc.restate(*sc.designed_keys(sc.frame("sparse_tail")))[1]["pairs"] > 0


def test_a_plain_upper_bound_search_would_not_do():
    """the wall's 14000 Gaussians land in ONE bucket when a key's bucket is the number of splitters <= key: the equality bucket is needed"""
    keys, inv = sc.designed_keys(sc.frame("wall_exact"))
    spl = sc.splitter_list(keys, inv)
    assert np.bincount(np.searchsorted(spl, keys[keys != inv], side="right")).max() >= 14000
    _, census, _ = sc.restate(keys, inv)
    assert census["largest"] < 200


def test_options_and_byte_counts():
    from ex4dgs_amd import _C
    lib = _C.load()
    assert _C.get_option("depth_sort_sample") == 0 and _C.get_option("depth_sort_sample_frames") == 0 and _C.get_option("depth_sort_sample_stats") == 0
    sizes = lambda: ([lib.ex4d_geom_bytes(P) for P in (1, 2049, 30000, 1000000, 2100000)],
                     [lib.ex4d_binning_bytes(R, 1352, 1014) for R in (0, 1, 7000000)], [lib.ex4d_img_bytes(64, 48), lib.ex4d_img_bytes(2048, 1088)])

    def layouts():
        g, b, i = _C.GeomLayout(), _C.BinningLayout(), _C.ImgLayout()
        lib.ex4d_geom_layout(30000, ctypes.byref(g)); lib.ex4d_binning_layout(500000, 1352, 1014, ctypes.byref(b)); lib.ex4d_img_layout(1352, 1014, ctypes.byref(i))
        return [bytes(x) for x in (g, b, i)]
    off = (sizes(), layouts())
    try:
        for name in ("depth_sort_sample", "depth_sort_sample_stats"):
            for bad in (-1, 2, 4):
                with pytest.raises(RuntimeError):
                    _C.set_option(name, bad)
            _C.set_option(name, 1)
            assert _C.get_option(name) == 1
        with pytest.raises(RuntimeError):
            _C.set_option("depth_sort_sample_frames", 0)          # read-only
        assert (sizes(), layouts()) == off
        assert (_C.get_option("depth_sort_msd"), _C.get_option("depth_sort_hold"), _C.get_option("depth_sort_trips")) == (3, 0, 0)
    finally:
        _C.set_option("depth_sort_sample", 0)
        _C.set_option("depth_sort_sample_stats", 0)
    assert (sizes(), layouts()) == off


def _bench_keys(cfg_name):
    """depth keys of a bench scene at t = 0, by id: p_view.z from the means and the view matrix in float32 (no rasterizer: a Gaussian is
    taken as visible where min_depth < z <= max_depth)"""
    from ex4dgs_amd.scene import CONFIGS, make_scene
    cfg = CONFIGS[cfg_name]
    model, cam, _ = make_scene(cfg_name)
    with torch.no_grad():
        m = model.get_xyz_at_t(0).float().cpu().numpy().astype(np.float32)
    V = cam.world_view_transform.cpu().numpy().astype(np.float32)
    z = (m[:, 0] * V[0, 2] + m[:, 1] * V[1, 2] + m[:, 2] * V[2, 2] + V[3, 2]).astype(np.float32)
    base, inv, kb = dc.key_frame(cfg.min_depth, cfg.max_depth)
    assert dc.depth_sort_msd_applies(z.size, kb)
    vis = (z > np.float32(cfg.min_depth)) & (z <= np.float32(cfg.max_depth))
    return np.where(vis, z.view(np.uint32).astype(np.int64) - base, inv), inv


def test_bench_scenes_stay_under_the_capacity():
    out = {}
    for name in ("cfg3", "cfg3c", "cfg5"):
        keys, inv = _bench_keys(name)
        threads, cap = sc.choice({})
        ub, _ = sc.bucket_table(sc.splitter_list(keys, inv))
        b = sc.bucket_of(ub, keys)
        n_of = np.bincount(b, minlength=ub.size)
        prev = np.concatenate([[0], ub[:-1]])
        ordinary = (((ub - 1) >> 1) > ((prev + 1) >> 1)) & (n_of > 0)
        largest, mean = int(n_of[ordinary].max()), float(n_of[ordinary].mean())
        out[name] = dict(P=int(keys.size), visible=int((keys != inv).sum()), buckets=int(ub.size), ordinary_buckets=int(ordinary.sum()),
                         largest=largest, mean=round(mean, 1), largest_to_mean=round(largest / mean, 3), capacity=cap)
        print(name, out[name])
        assert largest <= cap == sc.capacity(threads), (name, out[name])
    path = os.path.join(ROOT, "profiles", "sample_sort_census.json")
    try:
        with open(path, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass                                      # (a read-only checkout: the figures were asserted above)
