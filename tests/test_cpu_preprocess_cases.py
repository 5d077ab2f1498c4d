"""The frames of tests/test_gpu_preprocess_paths.py, without a GPU: every frame realises its plan on the CPU oracle -- the frustum test's
verdict and radii > 0 on EVERY row -- the depth planes set onto a Gaussian's own depth cull / keep that Gaussian, the table as a whole
reaches every path of the per-Gaussian kernels with every lane pattern that can occur on it (the cells are spelled out below), the
shared-chunk situations of the split layout occur on staged waves, the oracle's fragile-pixel fraction stays inside compare_forward's
bar, and the census itself (tests/preprocess_cases.py) gives the known answers on hand-written one-wave frames."""
import collections

import numpy as np
import pytest

from tests import helpers as h
from tests import preprocess_cases as pc

NAMES = [c.name for c in pc.RUNNABLE]
MAX_FRAGILE_FRAC = 2e-3                      # compare_forward's default


# ------------------------------------------------------------------ the census on hand-written frames
def _case(P, **kw):
    return pc.Case("hand", P, **kw)


def _census(case, culled=(), invisible=(), **kw):
    frustum = np.ones(case.P, bool)
    frustum[list(culled)] = False
    visible = frustum.copy()
    visible[list(invisible)] = False
    return pc.census(case, frustum, visible, **kw)


def test_census_one_tensor():
    c = _census(_case(64))
    assert c["fwd"] == ["plain12"] and c["bwd_read"] == ["staged"] and c["bwd_store"] == ["staged"]
    assert c["need_classes"] == [{"full"}] and c["rows"].tolist() == [64] and c["last_workgroup_chunks"] == 1 and c["last_wave_rows"] == 64
    # one culled row, one short row, one degree below 3: the predicated loads
    assert _census(_case(64), culled=[5])["fwd"] == ["predicated"]
    assert _census(_case(63))["fwd"] == ["predicated"]
    for D, nvec in ((0, 1), (1, 3), (2, 7), (3, 12)):
        assert pc.nvec_of(D) == nvec
        assert _census(_case(64, D=D))["fwd"] == ["plain12" if D == 3 else "predicated"]
    # a row that passes the frustum test and is not rendered: needed by the forward, dead for the backward
    c = _census(_case(64), culled=[5], invisible=[6])
    assert c["need"][0].sum() == 63 and c["live"][0].sum() == 62 and not c["need"][0, 5] and c["need"][0, 6] and not c["live"][0, 6]
    # predicate off: all ones, whatever is culled -- the plain loads again
    c = _census(_case(64), culled=[5], sh_predicate=0)
    assert c["fwd"] == ["plain12"] and c["need"][0].all() and c["live"][0].sum() == 63
    # prepare_backward: the sums are read, whatever the layout -- but not without SH
    assert _census(_case(64), prepare_backward=1)["bwd_read"] == ["dsums"]
    assert _census(_case(64, layout="colors", M=0), prepare_backward=1)["bwd_read"] == ["no_sh"]
    c = _census(_case(64, D=1, M=4))
    assert (c["fwd"], c["bwd_read"], c["bwd_store"]) == (["unstaged"], ["unstaged"], ["m_not_16"])
    # 5 workgroups and a tail: 1400 = 5 * 256 + 120 -> 2 chunks in the last workgroup, 56 rows in the last wave
    c = _census(_case(1400))
    assert len(c["fwd"]) == 22 and c["last_workgroup_chunks"] == 2 and c["last_wave_rows"] == 56 and c["fwd"][-1] == "predicated"
    assert [_census(_case(P))["last_workgroup_chunks"] for P in (1, 64, 95, 160, 225, 1280, 1343)] == [1, 1, 2, 3, 4, 4, 1]


def test_census_split_layout():
    sp = lambda P, n, **kw: _case(P, layout="split", n_static=n, **kw)
    assert _census(sp(64, 0))["fwd"] == ["split_staged"] and _census(sp(64, 64))["fwd"] == ["split_staged"]
    assert _census(sp(63, 0))["fwd"] == ["split_rows"]                                   # a partial wave
    # n_static = 1: wave 0 straddles, wave 1 starts at dynamic row 63: 63 * 45 floats = 11340 bytes, 12 behind a 16-byte boundary
    c = _census(sp(128, 1))
    assert c["fwd"] == ["split_rows", "split_rows"] and c["bwd_read"] == ["split_rows"] * 2 and c["bwd_store"] == ["rows"] * 2
    # n_static = 4: wave 1 starts at dynamic row 60 (60 * 45 * 4 and 60 * 3 * 4 are multiples of 16), wave 2 holds 4 rows
    c = _census(sp(132, 4))
    assert c["fwd"] == ["split_rows", "split_staged", "split_rows"] and c["bwd_store"] == ["rows", "staged", "rows"]
    assert c["bwd_read"] == ["split_rows", "split_staged", "split_rows"]
    # n_static = 32: wave 1 starts at dynamic row 32; n_static = 2: row 62, 62 * 3 floats = 744 bytes = 16 * 46.5
    assert _census(sp(128, 32))["fwd"] == ["split_rows", "split_staged"] and _census(sp(128, 2))["fwd"] == ["split_rows", "split_rows"]
    # tensors 4 bytes behind a 16-byte boundary: inputs -> nothing is staged; gradients alone -> staged reads, stores row by row
    c = _census(sp(128, 64, in_offset=1))
    assert c["fwd"] == ["split_rows"] * 2 and c["bwd_read"] == ["split_rows"] * 2 and c["bwd_store"] == ["rows"] * 2
    c = _census(sp(128, 64, grad_offset=1))
    assert c["fwd"] == ["split_staged"] * 2 and c["bwd_read"] == ["split_staged"] * 2 and c["bwd_store"] == ["rows"] * 2
    assert _census(sp(128, 64, grad_offset=1), prepare_backward=1)["bwd_read"] == ["dsums"] * 2


def test_pattern_classes_of_known_masks():
    m = pc.PATTERN_MASKS
    assert pc.pattern_classes(m["all"], 64) == {"full"} and pc.pattern_classes(m["none"], 64) == {"empty"}
    assert pc.pattern_classes(m["all"], 1) == {"full"}
    assert pc.pattern_classes(m["lower"], 64) == {"lower_only"} and pc.pattern_classes(m["upper"], 64) == {"upper_only"}
    assert pc.pattern_classes(m["lower"], 32) == {"full"} and pc.pattern_classes(m["upper"], 32) == {"empty"}
    # (a lone row with both neighbours inside the wave is an isolated needed row as well)
    for lane, also in ((0, set()), (31, {"iso_visible_lower"}), (32, {"iso_visible_upper"}), (63, set())):
        assert pc.pattern_classes(m[f"one{lane}"], 64) == {f"single_{lane}"} | also
    assert pc.pattern_classes(m["even"], 64) == {"alternating", "mixed_halves"} == pc.pattern_classes(m["odd"], 64)
    assert pc.pattern_classes(m["even"], 31) == {"alternating"}
    assert pc.pattern_classes(m["third"], 64) == {"every_third", "mixed_halves", "iso_visible_lower", "iso_visible_upper"}
    # (lane 32 between 31 and 33 is an isolated row of the other kind in both patterns)
    assert pc.pattern_classes(m["iso_visible"], 64) == {"iso_visible_lower", "iso_visible_upper", "iso_culled_upper", "mixed_halves"}
    assert pc.pattern_classes(m["iso_culled"], 64) == {"iso_culled_lower", "iso_culled_upper", "iso_visible_upper", "mixed_halves"}
    # lanes 0 and 63 have one neighbour inside the wave: of the three culled lanes only lane 32 is isolated
    assert pc.pattern_classes(m["iso_culled_edges"], 64) == {"iso_culled_upper", "mixed_halves"}
    # a partial wave sees the lanes it has
    assert pc.pattern_classes(m["iso_visible"], 33) == {"iso_visible_lower"}
    assert all(0 < pc.pattern_mask("random", s).sum() == 32 for s in range(4))
    # every isolated needed row of the pattern shares its first 16-byte chunk of the split layout's rest span with the row in front
    assert all((45 * r) % 4 != 0 for r in pc.ISO_VISIBLE)


# ------------------------------------------------------------------ every frame realises its plan
@pytest.mark.parametrize("name", NAMES)
def test_frame_realises_its_plan(name):
    from oracle import oracle
    f = pc.frame(name)
    st = f.settings
    assert f.ins["means3D"].dtype.is_floating_point and tuple(f.ins["means3D"].shape) == (f.case.P, 3)
    marked = oracle.mark_visible(f.ins["means3D"], st["viewmatrix"], st["projmatrix"], st["min_depth"], st["max_depth"])
    bad = np.flatnonzero(marked != f.frustum)
    assert bad.size == 0, ("frustum verdict differs from the plan on rows", bad[:16].tolist(), [pc.CLASS_NAMES[k] for k in f.cls[bad[:16]]])
    o = pc.oracle_forward(name)
    bad = np.flatnonzero((o["radii"] > 0) != f.visible)
    assert bad.size == 0, ("radii > 0 differs from the plan on rows", bad[:16].tolist(), [pc.CLASS_NAMES[k] for k in f.cls[bad[:16]]])
    if f.case.special not in ("min_depth", "max_depth"):
        assert np.array_equal(f.frustum, ~np.isin(f.cls, pc.CULLED)) and np.array_equal(f.visible, f.cls == pc.VIS)
    # (P = 1 cannot hold 8)
    if set(f.case.patterns) == {"none"}:
        assert int(f.visible.sum()) == 0 and o["num_rendered"] == 0
    else:
        assert int(f.visible.sum()) >= min(8, f.case.P), int(f.visible.sum())
    frag = 1.0 - float((o["fragile"] > h.FRAG_EPS).mean())
    assert frag <= MAX_FRAGILE_FRAC, frag
    # every frame is valid input: finite everywhere but the planted NaN coordinates
    nan = np.isnan(f.ins["means3D"].numpy())
    assert np.array_equal(nan.any(1), f.cls == pc.NAN) and (nan.sum(1) <= 1).all()
    for k, v in f.ins.items():
        if v is not None and k != "means3D":
            assert bool(np.isfinite(v.numpy()).all()), k


def test_every_row_class_occurs_and_is_what_it_claims():
    """Over the table: every class on hundreds of rows, and each culled class fails the frustum test for ITS reason alone."""
    count = collections.Counter()
    for name in NAMES:
        f = pc.frame(name)
        st = f.settings
        count.update(f.cls.tolist())
        if f.case.special in ("min_depth", "max_depth"):
            continue
        m = f.ins["means3D"].double().numpy()
        hom = np.concatenate([m, np.ones((f.case.P, 1))], 1)
        z = (hom @ st["viewmatrix"].double().numpy())[:, 2]
        p = hom @ st["projmatrix"].double().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            nx, ny = p[:, 0] / (p[:, 3] + 1e-7), p[:, 1] / (p[:, 3] + 1e-7)
        reasons = np.stack([z <= st["min_depth"], z > st["max_depth"], np.abs(nx) > 1.3, np.abs(ny) > 1.3], -1)
        want = {pc.NEAR: 0, pc.BACK: 0, pc.FAR: 1, pc.XPOS: 2, pc.XNEG: 2, pc.YPOS: 3, pc.YNEG: 3}
        for k, col in want.items():
            rows = f.cls == k
            if k == pc.BACK:          # behind the camera the perspective division flips the signs: only the depth reason is asserted
                assert reasons[rows, 0].all()
                continue
            assert reasons[rows, col].all() and reasons[rows].sum(1).tolist() == [1] * int(rows.sum()), (name, pc.CLASS_NAMES[k])
        for k in pc.INVISIBLE[:4]:
            rows = f.cls == k
            edge = np.abs(nx[rows]) if k in (pc.EDGE_XPOS, pc.EDGE_XNEG) else np.abs(ny[rows])
            assert ((edge > 1.05) & (edge < 1.25)).all() and not reasons[rows].any(), (name, pc.CLASS_NAMES[k])
    assert all(count[k] >= 100 for k in range(len(pc.CLASS_NAMES))), {pc.CLASS_NAMES[k]: count[k] for k in range(len(pc.CLASS_NAMES))}


def test_depth_planes_on_a_gaussians_own_depth():
    lo, hi = (pc.frame(n) for n in pc.THRESHOLD_CASES)
    for f, key in ((lo, "min_depth"), (hi, "max_depth")):
        o = pc.oracle_forward(f.case.name)
        base = h.oracle_forward(f.ins, dict(f.settings, min_depth=pc.MIN_DEPTH, max_depth=pc.MAX_DEPTH))
        d = base["depths"]
        assert d.dtype == np.float32 and f.settings[key] == float(d[f.marked])            # the plane IS the Gaussian's float32 depth
        kept = bool(o["radii"][f.marked] > 0)
        assert kept == (key == "max_depth"), (key, kept)                                  # z <= min_depth culls, z > max_depth does not
        # both sides of the plane are populated, and a Gaussian one float further out is on the other side
        assert 100 <= int((o["radii"] > 0).sum()) <= f.case.P - 100
        order = np.argsort(d, kind="stable")
        at = int(np.flatnonzero(order == f.marked)[0])
        nxt = int(order[at + 1])
        assert d[nxt] > d[f.marked] and bool(o["radii"][nxt] > 0) == (key == "min_depth")


def test_prefiltered_is_refused_on_the_frames_with_one_culled_row():
    for name, row in zip(pc.PREFILTER_CASES, (0, None)):
        f = pc.frame(name)
        row = f.case.P - 1 if row is None else row
        assert np.flatnonzero(~f.frustum).tolist() == [row]
        assert (row % pc.WAVE == 0) if row == 0 else (f.case.P % pc.WAVE != 0 and row // pc.WAVE == (f.case.P - 1) // pc.WAVE)
        with pytest.raises(RuntimeError, match="filtered although prefiltered"):
            h.oracle_forward(f.ins, dict(f.settings, prefiltered=True))


def test_flow_cases():
    f = pc.frame("flow only on unrendered rows")
    carriers = pc.flow_carriers(f)
    assert carriers.sum() >= 100 and not (carriers & f.visible).any() and (carriers & ~f.frustum).any() and (carriers & f.frustum).any()
    assert float(np.abs(pc.oracle_forward(f.case.name)["flow"]).max()) == 0.0
    f = pc.frame("flow on one row of the partial last wave")
    carriers = np.flatnonzero(pc.flow_carriers(f))
    P = f.case.P
    assert carriers.size == 1 and f.visible[carriers[0]] and P % pc.WAVE != 0 and carriers[0] >= P // pc.WAVE * pc.WAVE
    assert float(np.abs(pc.oracle_forward(f.case.name)["flow"]).max()) > 0.0


# ------------------------------------------------------------------ the coverage of the table
def _table():
    cells = {k: collections.Counter() for k in ("fwd", "read", "read_prepared", "store")}
    shared = collections.Counter()
    edges = dict(last_workgroup_chunks=set(), last_wave_rows=set(), P=set(), n_static_mod=set())
    for c in pc.RUNNABLE:
        f = pc.frame(c.name)
        edges["last_workgroup_chunks"].add(pc.census(c, f.frustum, f.visible)["last_workgroup_chunks"])
        edges["last_wave_rows"].add(pc.census(c, f.frustum, f.visible)["last_wave_rows"])
        edges["P"].add(c.P)
        if c.layout == "split":
            edges["n_static_mod"].add("0" if c.n_static == 0 else "P" if c.n_static == c.P else f"64k+{c.n_static % 64}")
        for prepared in (0, 1):
            cs = pc.census(c, f.frustum, f.visible, sh_predicate=1, prepare_backward=prepared)
            for w in range(len(cs["fwd"])):
                for k in cs["live_classes"][w]:
                    cells["read_prepared" if prepared else "read"][(cs["bwd_read"][w], k)] += 1
                if prepared:
                    continue
                for k in cs["need_classes"][w]:
                    cells["fwd"][(cs["fwd"][w], k)] += 1
                for k in cs["live_classes"][w]:
                    cells["store"][(cs["bwd_store"][w], k)] += 1
                if cs["fwd"][w] == "split_staged":
                    for side in ("need", "live"):
                        for k, v in cs["shared"][w][side].items():
                            shared[(side, k)] += int(v)
    return cells, shared, edges


def test_every_path_meets_every_pattern():
    cells, shared, edges = _table()
    P = pc.PATTERN_CLASSES
    want = {
        "fwd": {"plain12": ("full",), "predicated": P, "split_staged": P, "split_rows": P, "unstaged": P, "no_sh": P},
        "read": {"staged": P, "split_staged": P, "split_rows": P, "unstaged": P, "no_sh": P},
        "read_prepared": {"dsums": P, "no_sh": P},
        "store": {"staged": P, "rows": P, "m_not_16": P, "no_sh": P},
    }
    assert want["fwd"] == pc.FWD_CELLS and set(want["store"]) == set(pc.BWD_STORE_PATHS)
    assert set(want["read"]) | set(want["read_prepared"]) == set(pc.BWD_READ_PATHS)
    zero = [(t, path, k) for t, rows in want.items() for path, ks in rows.items() for k in ks if cells[t][(path, k)] < 1]
    assert not zero, zero
    # nothing runs on a path the table does not name
    for t, counter in cells.items():
        assert {path for path, _ in counter} <= set(want[t]), (t, set(counter))
    # the plain loads never see anything but a full mask
    assert {k for (path, k), n in cells["fwd"].items() if path == "plain12" and n} == {"full"}
    for t in want:
        print(t, {path: min(cells[t][(path, k)] for k in ks) for path, ks in want[t].items()})


def test_shared_chunks_of_the_split_layout_occur_on_staged_waves():
    """A 16-byte chunk of the rest / dc span belongs to two neighbouring rows: on waves that go through LDS a needed row follows a culled
    one, a culled row follows a needed one, and lanes 31 and 32 -- the two halves the spans are staged in -- differ; in the forward's
    need mask and in the backward's radii > 0 mask."""
    _, shared, _ = _table()
    for side in ("need", "live"):
        for k in ("visible_after_culled", "culled_after_visible", "halves_differ_at_31_32"):
            assert shared[(side, k)] >= 8, (side, k, shared[(side, k)])


def test_wave_and_workgroup_edges():
    _, _, edges = _table()
    assert edges["last_workgroup_chunks"] == {1, 2, 3, 4}
    assert edges["last_wave_rows"] >= {1, 31, 32, 33, 63, 64}
    assert {1, 64} <= edges["P"] and max(edges["P"]) > 5 * pc.GROUP
    assert edges["n_static_mod"] >= {"0", "P", "64k+0", "64k+4", "64k+1", "64k+32"}
    layouts = {(c.layout, c.D, c.M) for c in pc.CASES}
    assert layouts >= {("cat", 0, 16), ("cat", 1, 16), ("cat", 2, 16), ("cat", 3, 16), ("cat", 1, 4), ("cat", 2, 9), ("cat", 3, 4), ("colors", 3, 0), ("split", 3, 16)}
    assert any(c.cov_precomp for c in pc.CASES) and any(c.in_offset for c in pc.CASES) and any(c.grad_offset for c in pc.CASES)
    # the one frame the argument check refuses: M = 4 coefficients at degree 3 would make the reference read 12 coefficients past each row
    refused = [c for c in pc.CASES if c.refused]
    assert [(c.D, c.M) for c in refused] == [(3, 4)] and (3 + 1) ** 2 > 4
    # the misaligned pair: staged reads with row-by-row stores, and nothing staged at all
    for c in pc.RUNNABLE:
        if c.grad_offset or c.in_offset:
            f = pc.frame(c.name)
            cs = pc.census(c, f.frustum, f.visible)
            full = [w for w in range(len(cs["fwd"])) if cs["rows"][w] == pc.WAVE]
            assert all(cs["bwd_store"][w] == "rows" for w in full)
            assert all(cs["bwd_read"][w] == ("split_staged" if c.grad_offset else "split_rows") for w in full)
