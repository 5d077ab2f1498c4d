"""The cases of tests/test_gpu_composite_variants.py, without a GPU: the census (tests/composite_cases.py) on hand-written frames with
known answers, and the CPU oracle's forward of the two scenes under every support layout -- the properties the GPU tests rely on
(every (sep, extra, gacc) class populated with deep quadrants, single pixels deciding a quadrant's class, quadrants without
contributors, pixels with acc == 0, few fragile pixels) depend on the data alone and are asserted here."""
import numpy as np
import pytest
import torch

from tests import composite_cases as cc
from tests import helpers as h


# ------------------------------------------------------------------ the census on hand-written frames
def _frame(W, H, n, contrib, lists):
    """One 16x16 tile with a list of n entries.  contrib: quadrant -> n_contrib of its pixels (scalar or [8,8]); lists: quadrant -> positions."""
    nc = np.zeros((16, 16), np.int64)
    ql = np.full(4 * n, 0x7FFFFFFF, np.int64)                   # never-written capacity
    qc = np.zeros((1, 4), np.int64)
    for q, v in contrib.items():
        nc[8 * (q >> 1): 8 * (q >> 1) + 8, 8 * (q & 1): 8 * (q & 1) + 8] = v
    for q, ent in lists.items():
        ql[q * n: q * n + len(ent)] = ent
        qc[0, q] = len(ent)
    return dict(n_contrib=nc[:H, :W], ranges=np.array([[0, n]]), qlist=ql, qcount=qc, W=W, H=H)


def _census(fr, acc=None, offsets=None, grads=None, pairs=1):
    W, H = fr["W"], fr["H"]
    acc = np.ones((H, W), np.float32) if acc is None else acc
    grads = [np.ones((3, H, W), np.float32), None, None, None] if grads is None else grads
    return cc.census(fr["n_contrib"], acc, fr["ranges"], fr["qlist"], fr["qcount"], offsets, grads, W, H, pairs)


def _loops(c):
    return {k: v for k, v in c["loops"].items() if v}


def test_census_list_lengths_0_1_16_17_97():
    # q0: no contributor -> early return; q1: one entry; q2: 16 valid of 20 listed (the four at or behind the deepest are dropped);
    # q3: 97 entries = six full batches + a tail of 1, one more than the ring holds
    fr = _frame(16, 16, 97, {0: 0, 1: 1, 2: 16, 3: 97}, {1: [0], 2: list(range(20)), 3: list(range(97))})
    c = _census(fr)
    assert c["early_return"] == 1 and c["outside"] == 0
    assert c["per_quadrant"]["valid"].tolist() == [0, 1, 16, 97]
    assert c["batches"] == 1 + 1 + 7 and c["entries"] == 1 + 16 + 97
    assert {n: k for n, k in c["tail_sizes"].items() if k} == {1: 2}
    assert c["ring_wrap_quadrants"] == 1 and c["ring_wraps"]["sep=1,extra=0,gacc=0"] == 1
    # full batches whose first entry lies below every pixel's last contributor: q2's one and q3's six
    assert _loops(c) == {cc.pairs_name(0, 1): 7, cc.pairs_name(0, 0): 2}
    # 17 entries: a full batch (positions 16 .. 1) and a tail of 1; 96 entries fill the ring exactly and do not wrap it
    fr = _frame(16, 16, 96, {0: 17, 1: 96}, {0: list(range(17)), 1: list(range(96))})
    c = _census(fr, pairs=0)
    assert c["early_return"] == 2 and c["per_quadrant"]["valid"].tolist() == [17, 96, 0, 0]
    assert c["ring_wrap_quadrants"] == 0 and {n: k for n, k in c["tail_sizes"].items() if k} == {1: 1}
    assert _loops(c) == {cc.batch_name(0, 1, 1, 0): 7, cc.batch_name(0, 1, 0, 0): 1}
    # a quadrant with contributors whose list holds nothing in front of its deepest one: no batch at all
    fr = _frame(16, 16, 8, {0: 3}, {0: [5, 6]})
    c = _census(fr)
    assert c["batches"] == 0 and c["entries"] == 0 and c["early_return"] == 3


def test_census_nolast_at_the_batch_boundary_and_outside_pixels():
    one_short = np.full((8, 8), 17); one_short[3, 5] = 16
    deep = np.full((8, 8), 33); deep[0, 0] = 17
    # W = 12: quadrants 1 and 3 keep 4 pixel columns; their outside pixels count as last contributor 0, so no batch is NOLAST there
    fr = _frame(12, 16, 40, {0: 17, 1: 17, 2: one_short, 3: deep},
                {0: list(range(17)), 1: list(range(17)), 2: list(range(17)), 3: list(range(33))})
    c = _census(fr, pairs=0)
    p = c["per_quadrant"]
    assert p["min_last"].tolist() == [17, 0, 16, 0] and p["deepest"].tolist() == [17, 17, 17, 33]
    # q0: first position 16 < 17 -> NOLAST; q2: min_last == the first position -> not; q1, q3: never.  Tails are never NOLAST
    assert _loops(c) == {cc.batch_name(0, 1, 1, 0): 1, cc.batch_name(0, 1, 0, 0): 1 + 2 + 2 + 3}
    # the same deep quadrant inside the image: min_last 17, batches start at 32 (not below 17), 16 (below) and 0 (tail)
    fr = _frame(16, 16, 40, {3: deep}, {3: list(range(33))})
    c = _census(fr, pairs=1)
    assert _loops(c) == {cc.pairs_name(0, 1): 1, cc.pairs_name(0, 0): 2}
    # a gap in the list: positions need not be dense, the first entry of a batch is what counts
    fr = _frame(16, 16, 64, {0: 60}, {0: [0] + list(range(40, 60))})
    c = _census(fr)
    assert c["per_quadrant"]["valid"][0] == 21 and c["tail_sizes"][5] == 1 and _loops(c) == {cc.pairs_name(0, 1): 1, cc.pairs_name(0, 0): 1}


def test_census_classes_gating_and_loop_names():
    W = H = 16
    fr = _frame(W, H, 4, {0: 2, 1: 2, 2: 2, 3: 2}, {q: [0, 1] for q in range(4)})
    acc = np.ones((H, W), np.float32); acc[:8, :8] = 0.0; acc[8:, 8:] = 0.0        # q0 and q3: acc == 0 everywhere
    ones = lambda n: np.ones((n, H, W), np.float32)
    zeros = lambda n: np.zeros((n, H, W), np.float32)
    # flow and dL_dacc everywhere: gated off where acc == 0
    p = _census(fr, acc=acc, grads=[ones(3), zeros(1), ones(3), ones(1)])["per_quadrant"]
    assert p["extra"].tolist() == [False, True, True, False] and p["gacc"].tolist() == [False, True, True, False]
    # a depth gradient is kept (undivided) where acc == 0; negative zero is zero
    gd = zeros(1); gd[0, 2, 3] = 0.5; gd[0, 12, 3] = -0.0
    p = _census(fr, acc=acc, grads=[ones(3), gd, None, None])["per_quadrant"]
    assert p["extra"].tolist() == [True, False, False, False] and not p["gacc"].any()
    # offsets: one moved pixel makes its quadrant non-separable; an offset too small to move a pixel does not (but moves pixel 0)
    off = np.zeros((H, W, 2), np.float32); off[9, 2, 1] = 0.25; off[:8, 8:, :] = 1e-9
    p = _census(fr, offsets=off)["per_quadrant"]
    assert p["sep"].tolist() == [True, False, False, True]       # q1 holds y = 0, where 0 + 1e-9 != 0
    off[0, 8:, 1] = 0.0
    c = _census(fr, offsets=off)
    assert c["per_quadrant"]["sep"].tolist() == [True, True, False, True]
    assert _loops(c) == {cc.pairs_name(0, 0): 3, cc.NOSEP: 1}
    # which loop a class takes under either setting
    assert len(set(cc.ALL_LOOPS)) == 13 and len(cc.LOOPS_PAIRS_ON) == 9 and len(cc.LOOPS_PAIRS_OFF) == 9
    assert set(cc.LOOPS_PAIRS_ON) | set(cc.LOOPS_PAIRS_OFF) == set(cc.ALL_LOOPS)
    for pairs, reach in ((1, cc.LOOPS_PAIRS_ON), (0, cc.LOOPS_PAIRS_OFF)):
        got = {cc.loop_of(s, e, g, n, pairs) for (s, e, g) in cc.CLASSES for n in (0, 1)}
        assert got == set(reach)
    assert cc.loop_of(1, 0, 0, 1, 1) == cc.pairs_name(0, 1) and cc.loop_of(1, 0, 1, 1, 1) == cc.batch_name(0, 1, 1, 1)
    assert cc.loop_of(0, 0, 0, 1, 1) == cc.NOSEP == cc.loop_of(0, 1, 1, 0, 0)
    grads = [ones(3), gd, ones(3), ones(1)]
    a, b = _census(fr, acc=acc, grads=grads, pairs=1), _census(fr, acc=acc, grads=grads, pairs=0)
    assert _loops(a) == {cc.pairs_name(1, 0): 1, cc.batch_name(1, 1, 0, 1): 2, cc.pairs_name(0, 0): 1}
    assert _loops(b) == {cc.batch_name(1, 1, 0, 0): 1, cc.batch_name(1, 1, 0, 1): 2, cc.batch_name(0, 1, 0, 0): 1}
    rep = cc.report(a, "hand")
    assert rep["kind"] == "composite_census" and "per_quadrant" not in rep
    import json
    json.dumps(rep)


def test_quadrant_numbering_matches_the_kernel():
    W, H = 100, 70
    gx = 7
    ids = np.arange(H * W).reshape(H, W)
    q = cc._quads(ids, W, H, -1)
    assert q.shape == (4 * 35, 64)
    for (px, py) in ((0, 0), (13, 10), (99, 69), (48, 32), (95, 63), (96, 64)):
        i = cc.quadrant_of(px, py, W)
        tile, quad = divmod(i, 4)
        lane = (px - ((tile % gx) * 16 + (quad & 1) * 8)) + 8 * (py - ((tile // gx) * 16 + (quad >> 1) * 8))
        assert 0 <= lane < 64 and q[i, lane] == py * W + px
    inside = (q >= 0).any(1)
    assert int(inside.sum()) == 117                      # 7 x 5 tiles: the right quadrants of the last column and the lower ones of the last row lie outside
    assert int((q[cc.quadrant_of(96, 64, W)] >= 0).sum()) == 4 * 6


# ------------------------------------------------------------------ the scenes on the CPU oracle
_FWD = {}


def _oracle(scene, layout):
    """(oracle forward, offsets, gradients after the fragile-pixel mask, quadrant facts) of a case; forwards are shared."""
    cfg, dir_scale = {"deep": (cc.DEEP, cc.DEEP_DIR_SCALE), "wrap": (cc.WRAP, cc.DEEP_DIR_SCALE), "sparse": (cc.SPARSE, 0.1)}[scene]
    sub, grads = layout(cfg.height, cfg.width)
    key = (scene, None if sub is None else sub.numpy().tobytes())
    if key not in _FWD:
        ins, st = h.scene_inputs(cfg, dir_scale=dir_scale)
        _FWD[key] = h.oracle_forward(ins, st, subpixel_offset=sub)
    o = _FWD[key]
    grads = cc.mask_fragile(grads, o["fragile"], h.FRAG_EPS)
    return o, sub, grads, cc.quadrant_facts(o["n_contrib"], o["acc"], sub, grads, cfg.width, cfg.height)


LAYOUTS = {"mixed": cc.mixed, "image_only": cc.image_only, "image_only_null": lambda H, W: cc.image_only(H, W, null=True),
           "single_pixel": cc.single_pixel, "dense": cc.dense}


@pytest.mark.parametrize("scene,layout", [("deep", "mixed"), ("deep", "image_only"), ("deep", "image_only_null"), ("deep", "single_pixel"),
                                          ("wrap", "mixed"), ("wrap", "image_only"), ("sparse", "dense"), ("sparse", "image_only")])
def test_fragile_fraction_is_inside_the_forward_comparisons_cap(scene, layout):
    o, *_ = _oracle(scene, LAYOUTS[layout])
    frac = float((o["fragile"] <= h.FRAG_EPS).mean())
    assert frac <= 2e-3, frac


def test_deep_scene_geometry_and_depth():
    o, _, _, f = _oracle("deep", cc.image_only)
    assert o["W"] == 100 and o["H"] == 70 and o["ranges"].shape[0] == 35
    assert float(np.abs(o["flow"]).max()) == 0.0               # dir3D = 0: the flow-free forward
    assert int(f["inside"].sum()) == 117
    live = f["inside"] & (f["deepest"] > 0)
    assert int((f["deepest"][live] > cc.RING).sum()) >= 58     # most quadrants walk more than the ring holds ...
    assert int((f["min_last"] >= 32).sum()) >= 64              # ... and have full batches in front of every pixel's last contributor
    # image_only: one class, nothing but the colour gradient
    assert f["sep"].all() and not f["extra"].any() and not f["gacc"].any()
    _, _, _, fn = _oracle("deep", LAYOUTS["image_only_null"])
    assert fn["sep"].all() and not fn["extra"].any() and not fn["gacc"].any()


@pytest.mark.parametrize("scene", ["deep", "wrap"])
def test_mixed_fills_every_class_with_deep_quadrants(scene):
    o, sub, grads, f = _oracle(scene, cc.mixed)
    live = f["inside"] & (f["deepest"] > 0)
    walked = cc.walked_lower_bound(o, sub)
    assert (walked <= f["deepest"]).all() and (walked[live] >= 1).all()
    for c in cc.CLASSES:
        m = live & (f["sep"] == bool(c[0])) & (f["extra"] == bool(c[1])) & (f["gacc"] == bool(c[2]))
        assert int(m.sum()) >= 8, (c, int(m.sum()))
        assert int((m & (f["min_last"] >= 32)).sum()) >= 8, (c, int((m & (f["min_last"] >= 32)).sum()))
        assert int((m & (f["deepest"] > cc.RING)).sum()) >= 1, c
        if scene == "wrap":          # lists longer than the ring in every class: what DEEP's quadrant-sized footprints cannot give
            assert int((m & (walked > cc.RING)).sum()) >= 8, (c, int((m & (walked > cc.RING)).sum()))
    # the masks sit on quadrant borders: neighbouring quadrants of one tile differ in class
    codes = (f["sep"].astype(int) + 2 * f["extra"] + 4 * f["gacc"]).reshape(-1, 4)
    assert int((codes.max(1) != codes.min(1)).sum()) >= 20


def test_single_pixels_decide_their_quadrants_class():
    o, sub, grads, f = _oracle("deep", cc.single_pixel)
    special = cc.single_quadrants(o["W"])
    assert len(set(special.values())) == 4
    for name, i in special.items():
        assert f["inside"][i] and f["deepest"][i] >= 16, name
        assert cc.class_at(f, i) == cc.SINGLE_EXPECT[name], (name, cc.class_at(f, i))
    # every other quadrant: colour only at integer positions
    others = np.ones(f["sep"].shape, bool); others[list(special.values())] = False
    assert f["sep"][others].all() and not f["extra"][others].any() and not f["gacc"][others].any()
    # the tiny offset is there and moves nothing
    tx, ty = cc.SINGLE_TINY_ORIGIN
    blk = sub[ty: ty + 8, tx: tx + 8].numpy()
    assert (blk != 0).all() and (np.float32(tx) + blk[..., 0] == np.float32(tx)).all()
    # (the single pixels themselves are not fragile, or the mask would have removed what the case is about)
    for p in (cc.SINGLE_DEPTH_PIXEL, cc.SINGLE_ACC_PIXEL, cc.SINGLE_OFFSET_PIXEL):
        assert o["fragile"][p[1], p[0]] > h.FRAG_EPS and o["acc"].reshape(o["H"], o["W"])[p[1], p[0]] > 0


def test_sparse_scene_has_empty_quadrants_short_lists_and_unlit_pixels():
    o, sub, grads, f = _oracle("sparse", cc.dense)
    live = f["inside"] & (f["deepest"] > 0)
    assert int((f["inside"] & (f["deepest"] == 0)).sum()) >= 1          # the kernel's early return
    assert int(live.sum()) >= 100 and int(f["deepest"][live].max()) < 16  # one tail batch per quadrant at the most
    acc = o["acc"].reshape(o["H"], o["W"])
    assert int((acc == 0).sum()) >= 500
    # dense gradients meet unlit pixels: a quadrant none of whose pixels is lit still takes `extra` (its depth gradient), never `gacc`
    unlit = live & ~cc._quads(acc > 0, o["W"], o["H"], False).any(1)
    assert f["extra"][live].all() and not f["gacc"][unlit].any()
    assert float((o["fragile"] <= h.FRAG_EPS).mean()) == 0.0
