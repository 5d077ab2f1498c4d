"""The cases of tests/test_gpu_composite_fwd_paths.py, without a GPU: the forward census (tests/composite_fwd_cases.py) on hand-written
frames with known answers, and on the CPU oracle's forward of every scene -- the coverage the GPU tests rely on (all 20 cells of the
walk, the clamp of alpha deciding, every group and chunk boundary, every branch of the quadrant cull, exact ties of the largest weight)
depends on the data alone and is asserted here, together with the census's agreement with the oracle itself."""
import json

import numpy as np
import pytest

from tests import composite_fwd_cases as fc
from tests import helpers as h


# ------------------------------------------------------------------ the census on hand-written frames
WIDE = (1e-9, 0.0, 1e-9)          # conic of a Gaussian that is flat over the tile: alpha = w on every pixel
SPOT = (40.0, 0.0, 40.0)          # ... and of one that reaches its own pixel only (a pixel further: alpha = w e^-20)


def _frame(W, H, entries, lists=None):
    """One 16x16 tile whose list holds `entries` = [(mean x, mean y, conic, w)] in this order; lists: quadrant -> staged positions
    (the kernel's qlist / qcount), None = the numpy cull decides."""
    n = len(entries)
    m2 = np.array([[e[0], e[1]] for e in entries], np.float32).reshape(n, 2)
    co = np.array([[*e[2], e[3]] for e in entries], np.float32).reshape(n, 4)
    kw = {}
    if lists is not None:
        ql = np.full(4 * n, 0x7FFFFFFF, np.int64)                 # never-written capacity
        qc = np.zeros(4, np.int64)
        for q, ent in lists.items():
            ql[q * n: q * n + len(ent)] = ent
            qc[q] = len(ent)
        kw = dict(qlist=ql, qcount=qc)
    return fc.census(np.array([[0, n]]), np.arange(n), co, m2, W, H, **kw)


def _nonzero(d):
    return {k: v for k, v in d.items() if v}


def _quadrant_image(c, key, q):
    img = c["per_quadrant"][key]
    return img[8 * (q >> 1): 8 * (q >> 1) + 8, 8 * (q & 1): 8 * (q & 1) + 8]


def test_census_counts_0_1_15_16_17_64():
    wide = [(8.0, 8.0, WIDE, 0.01)] * 64                       # 0.99^64 = 0.53: nobody saturates
    c = _frame(16, 16, wide, {0: [], 1: [5], 2: list(range(15)), 3: list(range(16))})
    assert _nonzero(c["cells"]) == {"noclamp.a.add": 1 + 8 + 8, "noclamp.b.add": 7 + 8}
    assert _nonzero(c["cnt_mod16"]) == {1: 1, 15: 1, 0: 1}
    assert c["chunks"] == 4 and c["chunks_empty_live"] == 1 and c["chunks_multi_group"] == 0 and c["chunks_end_on_a"] == 2
    assert c["quadrants_finished"] == 4 and c["quadrants_unfinished"] == 0 and c["later_chunks"] == 0
    assert c["abandoned_a"] == 0 and c["abandoned_b"] == 0 and c["clamped_pairs"] == 0 and c["weight_ties"] == 0
    p = c["per_quadrant"]
    assert p["chunks"].tolist() == [1, 1, 1, 1] and p["last_live_chunk"].tolist() == [0, 0, 0, 0] and p["staged"].tolist() == [0, 1, 15, 16]
    for q, last, dom in ((0, 0, -1), (1, 6, 5), (2, 15, 0), (3, 16, 0)):           # weights fall with T: the first entry dominates
        assert (_quadrant_image(c, "last", q) == last).all() and (_quadrant_image(c, "dom", q) == dom).all(), q
    # the numpy cull keeps all 64 everywhere, and every entry reaches alpha >= 1/255: what the given lists leave out is counted
    assert c["cull_differs"] == 4 * 64 - 32 and c["cull_missed"] == 4 * 64 - 32 and c["from_kernel_lists"] == 1
    # the mean (8, 8) faces a corner of quadrant 0, a horizontal edge of 1, a vertical edge of 2 and lies inside 3
    assert _nonzero(c["cull"]) == {"corner.kept": 64, "horizontal.kept": 64, "vertical.kept": 64, "inside.kept": 64}
    c = _frame(16, 16, wide, {0: list(range(17)), 1: list(range(64))})
    assert _nonzero(c["cells"]) == {"noclamp.a.add": 9 + 32, "noclamp.b.add": 8 + 32}
    assert _nonzero(c["cnt_mod16"]) == {1: 1, 0: 1} and c["chunks_multi_group"] == 2 and c["chunks_end_on_a"] == 1 and c["chunks_empty_live"] == 2
    assert c["new_dominant_group_ge1"] == 0 and c["pairs_added"] == 64 * (17 + 64)
    json.dumps(fc.report(c, "hand"))
    assert "per_quadrant" not in fc.report(c, "hand")


def test_census_two_chunks_and_the_clamp_variant():
    # 70 entries: a second chunk of 6; w rises by 2 % per entry, faster than T falls (w <= 1.6 %): every entry is a new dominant contributor
    ent = [(8.0, 8.0, WIDE, 0.004 * 1.02 ** k) for k in range(70)]
    c = _frame(16, 16, ent)
    assert _nonzero(c["cells"]) == {"noclamp.a.add": 4 * 35, "noclamp.b.add": 4 * 35}
    assert c["chunks"] == 8 and c["later_chunks"] == 4 and _nonzero(c["cnt_mod16"]) == {0: 4, 6: 4} and c["chunks_end_on_a"] == 0
    assert c["new_dominant_group_ge1"] == 256 * (48 + 0) and c["new_dominant_chunk_ge1"] == 256 * 6
    assert (c["per_quadrant"]["dom"] == 69).all() and (c["per_quadrant"]["dom_at"] == (1, 5)).all() and (c["per_quadrant"]["last"] == 70).all()
    assert c["per_quadrant"]["chunks"].tolist() == [2] * 4 and c["cull_differs"] == 0 and c["cull_missed"] == 0
    # one entry with w > 0.99 in the second chunk: that chunk alone walks the CLAMP variant; alpha = min(0.99, w G) there
    ent[66] = (8.0, 8.0, WIDE, 0.995)
    c = _frame(16, 16, ent)
    assert _nonzero(c["cells"]) == {"noclamp.a.add": 4 * 32, "noclamp.b.add": 4 * 32, "clamp.a.add": 4 * 3, "clamp.b.add": 4 * 3}
    assert c["clamped_pairs"] == 256 and c["clamped_entries"] == 4 and c["clamped_gaussians"] == 1
    assert (c["per_quadrant"]["dom"] == 66).all()


def test_census_saturating_lanes_on_either_set():
    p = (2.0, 2.0)                                               # a pixel of quadrant 0
    spot, wide = (lambda w: (*p, SPOT, w)), (lambda w: (8.0, 8.0, WIDE, w))
    # quadrant 0 stages everything: five spots bring p to T = 0.2^5; the wide entry at j = 5 saturates p while 63 lanes add (rare_add, set
    # b); the spot at j = 6 reaches only the dead p (skip, a); 0.2 x 0.4^k < 1e-4 first at k = 9: eight adds, then every lane saturates at
    # j = 15 (rare_dead, b) with three entries left.  Quadrants 1-3 cull the spots: wide 0.8 at j = 0, eight adds, dead at j = 9 (b)
    ent = [spot(0.8)] * 5 + [wide(0.8), spot(0.8)] + [wide(0.6)] * 12
    c = _frame(16, 16, ent)
    assert c["per_quadrant"]["staged"].tolist() == [19, 13, 13, 13]
    assert _nonzero(c["cells"]) == {"noclamp.a.add": 3 + 4 + 3 * (1 + 4), "noclamp.b.add": 2 + 4 + 3 * 4, "noclamp.b.rare_add": 1, "noclamp.a.skip": 1,
                                    "noclamp.b.rare_dead": 4}
    assert c["abandoned_b"] == 4 and c["abandoned_a"] == 0 and c["chunks_end_on_a"] == 0
    assert c["per_quadrant"]["last"][2, 2] == 5 and c["per_quadrant"]["last"][2, 3] == 15 and c["per_quadrant"]["last"][12, 12] == 15
    # the six spots face a vertical edge of quadrant 1, a horizontal edge of 2 and a corner of 3: culled there
    assert c["cull"]["vertical.culled"] == 6 and c["cull"]["horizontal.culled"] == 6 and c["cull"]["corner.culled"] == 6 and c["cull"]["inside.kept"] == 6 + 13
    # 0.4^10 = 1.05e-4, 0.4^11 < 1e-4: every lane saturates at j = 10 (set a) of 14 entries
    c = _frame(16, 16, [wide(0.6)] * 14)
    assert _nonzero(c["cells"]) == {"noclamp.a.add": 4 * 5, "noclamp.b.add": 4 * 5, "noclamp.a.rare_dead": 4} and c["abandoned_a"] == 4
    assert (c["per_quadrant"]["last"] == 10).all()
    # ... and at the chunk's last entry: dead, but nothing abandoned
    c = _frame(16, 16, [wide(0.6)] * 11)
    assert c["cells"]["noclamp.a.rare_dead"] == 4 and c["abandoned_a"] == 0 and c["chunks_end_on_a"] == 0
    # the lane saturates where nobody else is in range: four spots, a wide entry every lane adds, the spot at j = 5 finishes p alone
    # (rare_skip, set b); one more wide entry in front moves it to j = 6 (set a).  With w > 0.99 somewhere in the chunk: CLAMP variant
    tail = [spot(0.8)] * 4 + [wide(0.8), spot(0.8), wide(0.01)]
    c = _frame(16, 16, tail)
    assert c["cells"]["noclamp.b.rare_skip"] == 1 and c["cells"]["noclamp.a.rare_skip"] == 0 and c["per_quadrant"]["last"][2, 2] == 5
    c = _frame(16, 16, [wide(0.01)] + tail)
    assert c["cells"]["noclamp.a.rare_skip"] == 1 and c["cells"]["noclamp.b.rare_skip"] == 0 and c["per_quadrant"]["last"][2, 2] == 6
    c = _frame(16, 16, tail + [(20.0, 20.0, (0.02, 0.0, 0.02), 0.999)])
    assert c["cells"]["clamp.b.rare_skip"] == 1 and sum(v for k, v in c["cells"].items() if k.startswith("noclamp")) == 0
    assert c["clamped_pairs"] == 0                               # staged with w > 0.99, but w G stays below 0.99 on every pixel
    # a list that goes on behind the dead quadrant: the second chunk is never looked at
    c = _frame(16, 16, [wide(0.6)] * 70)
    assert c["quadrants_unfinished"] == 4 and c["quadrants_finished"] == 0 and c["chunks"] == 4 and c["later_chunks"] == 0
    assert c["per_quadrant"]["last_live_chunk"].tolist() == [0] * 4 and c["abandoned_a"] == 4


def test_census_quadrants_outside_the_image_and_empty_lists():
    wide = [(4.0, 8.0, WIDE, 0.01)] * 3
    c = _frame(8, 16, wide)                                       # W = 8: the right quadrants have no pixel
    assert c["quadrants_outside"] == 2 and c["quadrants_partly_outside"] == 0 and c["chunks"] == 2
    assert c["per_quadrant"]["chunks"].tolist() == [1, 0, 1, 0] and c["per_quadrant"]["last_live_chunk"].tolist() == [0, -1, 0, -1]
    assert c["pairs_added"] == 3 * 128 and c["per_quadrant"]["last"].shape == (16, 8)
    c = _frame(12, 10, wide)                                      # the right quadrants keep 4 columns, the lower ones 2 rows
    assert c["quadrants_outside"] == 0 and c["quadrants_partly_outside"] == 3 and c["pairs_added"] == 3 * 120
    assert c["quadrants_empty_list"] == 0
    c = fc.census(np.array([[0, 0]]), np.zeros(0, np.int64), np.zeros((0, 4), np.float32), np.zeros((0, 2), np.float32), 16, 16)
    assert c["quadrants_empty_list"] == 4 and c["chunks"] == 0 and (c["per_quadrant"]["dom"] == -1).all()
    # a Gaussian below 1/255 is culled even with its mean inside the box (tau = -inf); a conic that is not positive definite is kept
    c = _frame(16, 16, [(4.0, 4.0, WIDE, 0.003), (40.0, 40.0, (1.0, 2.0, 1.0), 0.5)])
    assert c["cull"]["inside.culled"] == 1 and c["cull"]["vertical.culled"] == 1 and c["cull"]["horizontal.culled"] == 1 and c["cull"]["corner.culled"] == 1
    assert c["tau_neg_inf"] == 4 and c["tau_pos_inf"] == 4
    assert c["cull"]["corner.kept"] == 4 and c["per_quadrant"]["staged"].tolist() == [1, 1, 1, 1]


def test_census_exact_ties_need_float32():
    # fl(fl(1/3) 0.75) == 0.25: the second entry's weight equals the first's bit for bit in float32 and the first stays dominant; in
    # float64 the product exceeds 0.25 by 2^-27 -- no tie, and the second entry wins: why the tie frames are replayed in float32
    third = np.float32(1.0) / np.float32(3.0)
    assert np.float32(third * np.float32(0.75)) == np.float32(0.25)
    ent = [(8.0, 8.0, (0.0, 0.0, 0.0), 0.25), (8.0, 8.0, (0.0, 0.0, 0.0), float(third))]
    n = len(ent)
    m2, co = np.array([[e[0], e[1]] for e in ent], np.float32), np.array([[*e[2], e[3]] for e in ent], np.float32)
    a = fc.census(np.array([[0, n]]), np.array([1, 0]), co[::-1].copy(), m2, 16, 16, dtype=np.float32)
    assert a["weight_ties"] == 256 and (a["per_quadrant"]["dom"] == 1).all() and a["dtype"] == "float32"
    b = fc.census(np.array([[0, n]]), np.array([1, 0]), co[::-1].copy(), m2, 16, 16)
    assert b["weight_ties"] == 0 and (b["per_quadrant"]["dom"] == 0).all()


# ------------------------------------------------------------------ the scenes on the CPU oracle
_FWD = {}


def _oracle(name, dir_scale=0.0):
    key = (name, dir_scale)
    if key not in _FWD:
        ins, st = fc.scene_inputs(name, dir_scale)
        o = h.oracle_forward(ins, st)
        _FWD[key] = (o, fc.census_of(o) if dir_scale == 0.0 else None)
    return _FWD[key]


def test_the_scenes_cover_every_path_of_the_walk():
    by_scene = {name: _oracle(name)[1] for name in fc.SCENES}
    fc.assert_coverage(by_scene)
    # what each scene is there for
    assert by_scene["opaque"]["clamped_pairs"] >= 50 and by_scene["opaque"]["clamped_entries"] >= 8
    assert min(by_scene["stack"]["cells"][fc.cell("clamp", s, "rare_skip")] for s in fc.SETS) >= 3
    assert sum(by_scene[k]["cells"][fc.cell("noclamp", s, "rare_skip")] for k in ("deep", "wrap") for s in fc.SETS) >= 4
    assert by_scene["specks"]["chunks_empty_live"] >= 8 and by_scene["specks"]["quadrants_empty_list"] >= 1
    assert by_scene["wrap"]["new_dominant_chunk_ge1"] >= 8 and by_scene["deep"]["new_dominant_group_ge1"] >= 8
    assert by_scene["wrap"]["quadrants_finished"] >= 8 and by_scene["wrap"]["quadrants_unfinished"] >= 8
    for c in by_scene.values():
        assert c["quadrants_outside"] == 23 and c["quadrants_partly_outside"] == 21
        assert c["weight_ties"] == 0 and c["cull_missed"] == 0 and c["cull_differs"] == 0


@pytest.mark.parametrize("name", list(fc.SCENES))
def test_fragile_fraction_is_inside_the_forward_comparisons_cap(name):
    for dir_scale in (0.0, 0.1):
        o = _oracle(name, dir_scale)[0]
        assert float((o["fragile"] <= h.FRAG_EPS).mean()) <= 2e-3, (name, dir_scale)
        # the index comparison of compare_forward leaves out at most 1e-4 of the solid pixels
        solid = o["fragile"] > h.FRAG_EPS
        assert int((solid & (o["idx_margin"] <= h.IDX_BAND)).sum()) <= 1e-4 * solid.sum()


@pytest.mark.parametrize("name", list(fc.SCENES))
def test_census_agrees_with_the_oracle(name):
    """The replay is a restatement: on the pixels whose decisions are not within FRAG_EPS of a threshold its last contributor is the
    oracle's n_contrib and its dominant entry the oracle's idx (where the two largest weights are further apart than float32 rounding)."""
    o, c = _oracle(name)
    solid = o["fragile"] > h.FRAG_EPS
    p = c["per_quadrant"]
    assert np.array_equal(p["last"][solid], o["n_contrib"].astype(np.int64)[solid])
    decided = solid & (o["idx_margin"] > h.IDX_BAND)
    assert np.array_equal(p["dom"][decided], o["idx"][0].astype(np.int64)[decided])
    assert int(decided.sum()) >= 0.999 * solid.sum()
    # the restated cull never drops a pair that reaches alpha >= (1 + 1e-4) / 255
    assert c["cull_missed"] == 0


@pytest.mark.parametrize("name", ["deep", "opaque", "specks"])
def test_only_the_flow_image_depends_on_dir3D(name):
    """What the flow kernel must share bit for bit with the flow-free walks: on the oracle, every output but `flow` has the same bits at
    dir_scale 0 and 0.1."""
    a, b = _oracle(name, 0.0)[0], _oracle(name, 0.1)[0]
    for k in fc.FLOW_INDEPENDENT:
        assert np.array_equal(a[k], b[k]), k
    assert float(np.abs(a["flow"]).max()) == 0.0 and float(np.abs(b["flow"]).max()) > 0.0
    assert set(fc.FLOW_INDEPENDENT) == {"color", "depth", "acc", "idx", "final_T", "n_contrib"}


# ------------------------------------------------------------------ the tie frames
@pytest.mark.parametrize("k", fc.TIE_FILLERS)
def test_tie_frames_tie_exactly_where_they_are_built_to(k):
    op1, op2, w1, w2 = fc.tie_opacities()
    ins, st = fc.tie_inputs(k)
    o = h.oracle_forward(ins, st)
    cx, cy = fc.TIE_CENTRE
    assert st["image_width"] % 2 == 1 and st["image_height"] % 2 == 1
    # the pair sits on the optical axis: the exact integer centre pixel, G = 1
    assert np.array_equal(o["means2D"][[fc.TIE_FIRST, fc.TIE_SECOND]], np.array([[cx, cy]] * 2, np.float32))
    wf, wb = o["conic_opacity"][fc.TIE_FIRST, 3], o["conic_opacity"][fc.TIE_SECOND, 3]
    assert wf == np.float32(w1) and wb == np.float32(w2) and 1.0 / 255.0 < wf < 0.99 and 1.0 / 255.0 < wb < 0.99
    # the oracle's float32 weights: alpha T of the front entry (T = 1) and of the back one (T = 1 - w_front)
    assert np.float32(wb * np.float32(np.float32(1.0) - wf)) == wf and wf > 0
    assert o["idx_margin"][cy, cx] == 0.0 and o["idx"][0, cy, cx] == fc.TIE_FIRST and o["n_contrib"][cy, cx] == k + 2
    assert float(o["fragile"][cy, cx]) > h.FRAG_EPS
    c = fc.census_of(o, dtype=np.float32)
    first, second = fc.tie_positions(o, c)
    want = {0: ((0, 0), (0, 1)), 14: ((0, 14), (0, 15)), 15: ((0, 15), (0, 16)), 63: ((0, 63), (1, 0))}[k]
    assert (first, second) == want
    assert c["weight_ties"] == 1 and c["per_quadrant"]["dom"][cy, cx] == fc.TIE_FIRST
    assert tuple(c["per_quadrant"]["dom_at"][cy, cx]) == first
    solid = o["fragile"] > h.FRAG_EPS
    assert np.array_equal(c["per_quadrant"]["last"][solid], o["n_contrib"].astype(np.int64)[solid])
    assert np.array_equal(c["per_quadrant"]["dom"][solid], o["idx"][0].astype(np.int64)[solid])
    # the fillers are staged for the centre pixel's quadrant and do not reach the centre pixel: T = 1 in front of the pair
    assert c["per_quadrant"]["staged"][fc.tie_quadrant()] == k + 2
