"""The constructed density-control cases (tests/densify_cases.py) mean what they say, without a GPU: on every case the torch
restatement (tests/densify_ref.py, pinned to the reference by tests/golden/densify.npz) yields exactly the row counts and the
row-to-row gather that the case list writes down by construction, the list covers the block edges it names, and the restatement run
in float32 sits within HALF of every bar of tests/test_gpu_densify_edges.py against itself in float64 -- so that a HIP kernel as
accurate as the reference passes there with room to spare, and a bar the reference formulation cannot meet shows up here."""
import numpy as np
import pytest
import torch

from tests import densify_cases as dc
from tests import densify_ref as R

COPIED = ("_xyz_disp", "_rotation", "_opacity", "_features_dc", "_features_rest", "_rotation_motion", "_opacity_motion", "_features_dc_motion",
          "_features_rest_motion")


def check_against_expectations(post, pre, maps, counts, what):
    """The restatement's result `post` of a densify call on `pre` equals the numpy gather through the expected maps, bit for bit,
    for everything that is copied, zeroed or set to a constant; returns nothing.  maps / counts: (static, dynamic)."""
    eq = lambda a, b, k: dc.assert_same(a.numpy(), b, f"{what}: {k}")
    for gi, (names, stat_names) in enumerate(((R.STATIC, R.S_STATS), (R.DYNAMIC, R.D_STATS))):
        mp, cnt = maps[gi], counts[gi]
        if gi == 1 and pre["params"]["_xyz_motion"].shape[0] == 0:
            continue
        for k in names:
            assert post["params"][k].shape[0] == cnt[dc.ROWS], (what, k, post["params"][k].shape, cnt)
            if k in COPIED:
                eq(post["params"][k], dc.gather_expected(pre["params"][k].numpy(), mp, cnt), k)
            if k == "_opacity_duration_var":
                eq(post["params"][k], dc.gather_expected(pre["params"][k].numpy(), mp, cnt, new=2.0), k)
            for mk in ("m", "v"):
                if pre[mk] is not None:
                    eq(post[mk][k], dc.gather_expected(pre[mk][k].numpy(), mp, cnt, new=0.0), f"{mk} {k}")
        for k, init in zip(stat_names[:7], R.INIT[:7]):
            eq(post["stats"][k], np.full(post["stats"][k].shape, init, np.float32), k)
        eq(post["stats"][stat_names[7]], dc.gather_expected(pre["stats"][stat_names[7]].numpy(), mp, cnt, new=("child", 1000.0)), stat_names[7])
        eq(post["stats"][stat_names[8]], dc.gather_expected(pre["stats"][stat_names[8]].numpy(), mp, cnt, new=("child", -1.0)), stat_names[8])


@pytest.mark.parametrize("config", ["A", "B"])
def test_cases_match_their_expectations_and_float32_sits_within_half_of_every_bar(config):
    worst = {k: 0.0 for k in dc.TRANSFORMED}
    for c in dc.cases():
        if c.config != config:
            continue
        sc, dy = dc.layout(config, c.static), dc.layout(config, c.dynamic)
        pre = dc.make_state(sc, dy, c.seed, config=config)
        counts = dc.expected_counts(sc, config), dc.expected_counts(dy, config)
        maps = dc.expected_map(sc, config), dc.expected_map(dy, config)
        draws = dc.make_draws(counts[0], counts[1], c.seed)
        r32 = dc.run_restatement(pre, config, draws)
        check_against_expectations(r32, pre, maps, counts, c.name)
        r64 = dc.run_restatement(pre, config, draws, torch.float64)
        for k in dc.TRANSFORMED:
            e = dc.transformed_error_over_bar(r32["params"][k].numpy(), r64["params"][k].numpy())
            assert e <= 0.5, (c.name, k, e)
            worst[k] = max(worst[k], e)
    print(f"configuration {config}: float32 restatement against float64, worst error / bar:", worst)


def test_prune_cases_match_their_expectations():
    for c in dc.prune_cases():
        sc, dy = dc.layout("P", c.static), dc.layout("P", c.dynamic)
        counts = dc.expected_counts(sc, "P"), dc.expected_counts(dy, "P")
        maps = dc.expected_map(sc, "P"), dc.expected_map(dy, "P")
        for kind in dc.PRUNE_KINDS:
            pre = dc.make_prune_state(kind, sc, dy, c.seed)
            post = dc.clone_state(pre)
            R.prune(post, kind)
            for gi, (names, stat_names) in enumerate(((R.STATIC, R.S_STATS), (R.DYNAMIC, R.D_STATS))):
                if gi == 1 and not dy:
                    continue
                for grp, keys in (("params", names), ("m", names), ("v", names), ("stats", stat_names)):
                    for k in keys:
                        dc.assert_same(post[grp][k].numpy(), dc.gather_expected(pre[grp][k].numpy(), maps[gi], counts[gi]), f"{c.name} {kind}: {grp} {k}")
            if kind == "nan" and dy:
                x = pre["params"]["_xyz_motion"].view(len(dy), -1)
                gone = np.array([k == "gone" for k in dy])
                assert x.shape[1] == 105 and torch.equal(x.isnan().any(dim=1), x[:, -1].isnan()) and not x[:, :-1].isnan().any()
                assert np.array_equal(x[:, -1].isnan().numpy(), gone)


def _block_sums(flags):
    pad = (-len(flags)) % dc.BLOCK
    f = np.concatenate([flags, np.zeros(pad, np.int64)]).reshape(-1, dc.BLOCK)
    return np.stack([((f >> k) & 1).sum(axis=1) for k in range(7)], axis=1)            # [blocks, 7]


def test_cases_cover_the_edges_they_name():
    for config in ("A", "B"):
        specs = dc.layout_specs(config)
        in_cases = {c.static for c in dc.cases() if c.config == config} | {c.dynamic for c in dc.cases() if c.config == config}
        assert set(specs) <= in_cases                                         # every layout is run through the whole call too
        for c in dc.cases():
            assert c.static != c.dynamic                                         # the two groups of a case never share a layout
        # every class uniform over a full block, at one block, at a block and a partial one, and at 257 blocks
        for name in dc.CLASSES[config]:
            assert {n for k, cl, n in (s for s in specs if s[0] == "uniform") if cl == name} >= set(dc.SMALL) | {65537}
        # block counts 1, 2, 256, 257, 513: one block per scan thread, two with idle threads, three
        blocks = {(dc.spec_rows(s) + dc.BLOCK - 1) // dc.BLOCK for s in specs}
        assert blocks >= {1, 2, 3, 16, 17, 256, 257, 513}
        assert {dc.scan_per(dc.spec_rows(s)) for s in specs} == {1, 2, 3}
        assert {dc.spec_rows(s) for s in specs} == set(dc.ROW_COUNTS)
        # a needle at 0, 255, 256 and N - 1, below and above one scan thread's worth of blocks
        for n in (513, 65537):
            assert {s[4] for s in specs if s[0] == "needle" and s[3] == n} == {0, 255, 256, n - 1}
        # runs: the class changes at every multiple of 256, and one row either side of a boundary between two scan threads
        for n in (4097, 65537, 131073):
            per, cuts = dc.scan_per(n), set(dc.run_boundaries(n))
            assert set(range(256, n, 256)) <= cuts and {256 * per * (1 if per > 1 else 4) + d for d in (-1, 0, 1)} <= cuts
            names = np.array(dc.layout(config, ("runs", n)))
            assert set((np.nonzero(names[1:] != names[:-1])[0] + 1).tolist()) == cuts
    # each of the seven packed counters reaches 256 -- the one value that needs the ninth bit -- in some block: with 8-bit fields
    # the count would carry into the next counter (the last one: out of the word), and either shows in `counts`
    seen = set()
    for config in ("A", "B"):
        for s in dc.layout_specs(config):
            if dc.spec_rows(s) <= 4097:
                seen |= set(np.nonzero((_block_sums(dc.class_flags(config, dc.layout(config, s))) == 256).any(axis=0))[0].tolist())
    assert seen == set(range(7)), seen
    # quad saturates CLONE, SPLIT, SPLIT_CLONE, KEEP_CHILD and KEEP_CHILD_CLONE at once while KEEP and KEEP_CLONE stay 0
    assert _block_sums(dc.class_flags("B", dc.uniform("quad", 256))).tolist() == [[0, 256, 0, 256, 256, 256, 256]]
    assert _block_sums(dc.class_flags("A", dc.uniform("clone", 256))).tolist() == [[256, 256, 256, 0, 0, 0, 0]]
    # the rows-out column of the class tables
    want = {"A": dict(keep=1, gone=0, clone=2, clone_gone=0, split=2, split_gone=0, nan_grad=1, big_quiet=1, at_thr=2, below_thr=1, nan_scale=1),
            "B": dict(keep=1, gone=0, clone=2, clone_gone=0, nan_grad=1, quad=4, split_kids_gone=0, split_gone=0, nan_scale=1)}
    for config, table in want.items():
        assert {k: dc.rows_out(v.flags) for k, v in dc.CLASSES[config].items()} == table
    # the prunes: the same block edges
    ps = dc.prune_layout_specs()
    assert {dc.scan_per(dc.spec_rows(s)) for s in ps} == {1, 2, 3} and {s[4] for s in ps if s[0] == "needle"} == {0, 255, 256, 512}


def test_thresholds_sit_where_the_class_tables_say():
    # at_thr / below_thr: the decision itself, as the kernel's fabsf(g) >= grad_thr against a float32 threshold must make it
    thr = torch.tensor(dc.GRAD_THR, dtype=torch.float32)
    at = torch.tensor([[float(np.float32(dc.GRAD_THR))]]) / 1
    below = torch.tensor([[float(np.nextafter(np.float32(dc.GRAD_THR), np.float32(0)))]]) / 1
    assert bool(torch.norm(at, dim=-1) >= dc.GRAD_THR) and not bool(torch.norm(below, dim=-1) >= dc.GRAD_THR)
    assert float(at) == float(thr) and float(below) < float(thr)
    assert bool(torch.norm(at.double(), dim=-1) >= dc.f32(dc.GRAD_THR)) and not bool(torch.norm(at.double(), dim=-1) >= dc.GRAD_THR)
    # torch.max propagates a NaN whichever column holds it: the nan_scale rows are neither selected nor pruned
    for col in range(3):
        s = torch.full((1, 3), -5.0)
        s[0, col] = float("nan")
        assert torch.exp(s).max(dim=1).values.isnan().all()
    # every finite scale keeps a factor 1.3 from the thresholds it meets (the children of quad: 1.067 from big)
    for config, dense, big in (("A", 0.01, None), ("B", 0.2, 0.1)):
        for name, k in dc.CLASSES[config].items():
            for s in ([k.scale] if k.scale != "nan" else []):
                for t in (dense, big) if big else (dense,):
                    assert max(s / t, t / s) >= 1.3, (config, name, s, t)
                if big and (k.flags & dc.SPLIT):
                    assert max(s / 1.6 / big, big / (s / 1.6)) >= 1.06, (config, name)


STAT_SHAPES = ((1, 0), (255, 257), (256, 256), (257, 1), (65537, 300))


def test_float32_gradient_accum_sits_within_half_of_its_bar():
    worst = [0.0, 0.0, 0.0]
    for ns, nd in STAT_SHAPES:
        for start in ("fresh", "prefilled"):
            st32 = R.init_stats(ns, nd) if start == "fresh" else dc.make_stats_prefill(ns, nd, ns + nd)
            st64 = {k: v.double() for k, v in st32.items()}
            for j, (radii, vg, eg, ts) in enumerate(dc.make_frames(ns, nd, ns + 3 * nd)):
                R.update(st32, radii, vg, eg, ts)
                R.update(st64, radii, vg.double(), eg.double(), ts)
                for k in ("xyz_gradient_accum", "motion_xyz_gradient_accum"):
                    e = dc.grad_accum_error_over_bar(st32[k].numpy(), st64[k].numpy(), j + 1)
                    assert e <= 0.5, (ns, nd, start, j, k, e)
                    worst[j] = max(worst[j], e)
    print("float32 gradient_accum against float64, worst error / (2 n + 1 ulp) after 1 / 2 / 3 updates:", worst)


def test_frames_cover_the_switch_points():
    frames = dc.make_frames(257, 300, 4)
    e0 = frames[0][2][:, 0].numpy()
    for v in dc.E0_SPECIAL[1:]:
        assert (e0 == np.float32(v)).any(), v
    assert np.isnan(e0).any() and (e0 > np.float32(0.01)).any()
    assert all((f[0] <= 0).any() and (f[0] > 0).any() for f in frames)
    # error_min / its timestamp are and are not replaced on the later frames
    st = R.init_stats(257, 300)
    replaced = []
    for radii, vg, eg, ts in frames:
        before = st["xyz_error_min_timestamp"].clone()
        R.update(st, radii, vg, eg, ts)
        replaced.append(st["xyz_error_min_timestamp"] != before)
    assert all(r.any() and not r.all() for r in replaced)
