"""Every inner loop of the compositing backward against the CPU oracle (run with `-m gpu` on an MI355X).

composite_bwd_scan_kernel picks one of 13 instantiations per batch of 16 list entries from what the quadrant's 64 pixels carry
(tests/composite_cases.py restates the choice).  The cases below put neighbouring quadrants of one frame into different loops, let single
pixels decide, pass the training loop's colour-only gradients as zeros and as null pointers, and run both settings of
"composite_bwd_pairs"; every case goes through _fwd_bwd of tests/test_gpu_parity.py -- the suite's oracle comparison with its bars
unchanged -- and then proves from the forward's own lists which loops it ran (the census), which is in turn pinned to the kernel's
counters.  tests/test_cpu_composite_cases.py asserts the data-only half of the coverage without a GPU."""
import numpy as np
import pytest
import torch

from tests import composite_cases as cc
from tests import helpers as h
from tests.test_gpu_parity import _fwd_bwd

pytestmark = pytest.mark.gpu

SCENES = {"deep": (cc.DEEP, cc.DEEP_DIR_SCALE), "wrap": (cc.WRAP, cc.DEEP_DIR_SCALE), "sparse": (cc.SPARSE, 0.1)}


def _census_of(g, sub, passed, cfg, pairs):
    return cc.census(g["n_contrib"], g["acc"], g["ranges"], g["qlist"], g["qcount"], sub, passed, cfg.width, cfg.height, pairs)


def _case(scene, layout, pairs, name):
    """Oracle comparison of one case under one setting of composite_bwd_pairs, then the census of what the backward ran."""
    from ex4dgs_amd import _C
    cfg, dir_scale = SCENES[scene]
    sub, grads = layout(cfg.height, cfg.width)
    assert _C.get_option("composite_bwd_pairs") == 1 and _C.get_option("composite_bwd_variant") == 4
    _C.set_option("composite_bwd_pairs", pairs)
    try:
        o, g, ob, gb, rep = _fwd_bwd(cfg, dir_scale=dir_scale, subpixel=sub, grads=lambda o: grads)
    finally:
        _C.set_option("composite_bwd_pairs", 1)
    c = _census_of(g, sub, rep["upstream"], cfg, pairs)
    h.REPORT.append(cc.report(c, f"{cfg.name} x {name}, composite_bwd_pairs={pairs}"))
    return o, g, gb, c


def _ran(c):
    return {k for k, v in c["loops"].items() if v}


@pytest.mark.parametrize("pairs", [1, 0])
@pytest.mark.parametrize("scene", ["deep", "wrap"])
def test_mixed_every_loop_of_the_setting(hip_lib, scene, pairs):
    """Quadrants of all eight (sep, extra, gacc) classes side by side, adding into the same Gaussians' accumulator rows: each of the nine
    loops the setting reaches runs at least 8 batches, full ones in front of every last contributor (NOLAST) and others, ending in tails
    of many sizes.  The two settings reach all 13 instantiations between them.  On WRAP the lists wrap the 96-slot ring in every class
    (DEEP's footprints cover whole quadrants: its compacted lists stay near 65 entries, a few quadrants wrap)."""
    o, g, gb, c = _case(scene, cc.mixed, pairs, "mixed")
    reach = cc.LOOPS_PAIRS_ON if pairs else cc.LOOPS_PAIRS_OFF
    assert len(reach) == 9 and set(cc.LOOPS_PAIRS_ON) | set(cc.LOOPS_PAIRS_OFF) == set(cc.ALL_LOOPS) and len(set(cc.ALL_LOOPS)) == 13
    assert _ran(c) == set(reach), c["loops"]
    for k in reach:
        assert c["loops"][k] >= 8, (k, c["loops"])
    for cls in cc.CLASSES:
        assert c["quadrants"][cc.class_name(cls)] >= 8, c["quadrants"]
        if scene == "wrap":
            assert c["ring_wraps"][cc.class_name(cls)] >= 1, c["ring_wraps"]
    assert c["ring_wrap_quadrants"] >= 1
    assert sum(1 for n, k in c["tail_sizes"].items() if k) >= 8, c["tail_sizes"]
    assert c["early_return"] == 0 and c["outside"] == 23


@pytest.mark.parametrize("scene,pairs,null", [("deep", 1, False), ("deep", 1, True), ("deep", 0, False), ("deep", 0, True), ("wrap", 1, True), ("wrap", 0, False)])
def test_image_only_the_training_loops_case(hip_lib, scene, pairs, null):
    """What FrameTrainer, NativeTrainer and bench.py run: the image's gradient alone (the others zero tensors, or absent).  Only
    EXTRA = false, GACC = false loops run; the sums only the depth and flow gradients feed stay exact zeros."""
    o, g, gb, c = _case(scene, lambda H, W: cc.image_only(H, W, null=null), pairs, "image_only " + ("null" if null else "zeros"))
    want = {cc.pairs_name(0, 0), cc.pairs_name(0, 1)} if pairs else {cc.batch_name(0, 1, 0, 0), cc.batch_name(0, 1, 1, 0)}
    assert _ran(c) == want, c["loops"]
    assert min(c["loops"][k] for k in want) >= 8 and c["ring_wrap_quadrants"] >= (64 if scene == "wrap" else 1)
    acc16 = gb["acc16"].cpu().numpy()
    assert np.abs(acc16[:, 7:10]).max() > 0
    for col in (2, 10, 11, 12):                          # dL_dmean2D.z, dL_ddir
        assert (acc16[:, col] == 0.0).all(), col
    assert (gb["dL_ddir"].cpu().numpy() == 0.0).all()


@pytest.mark.parametrize("pairs", [1, 0])
def test_deep_single_pixels_decide_the_loop(hip_lib, pairs):
    """One pixel with a depth gradient, one with dL_dacc, one moved by a sub-pixel offset: each switches its whole quadrant to another
    loop; offsets too small to move a pixel leave theirs separable."""
    o, g, gb, c = _case("deep", cc.single_pixel, pairs, "single_pixel")
    p = c["per_quadrant"]
    special = cc.single_quadrants(cc.DEEP.width)
    for name, i in special.items():
        assert cc.class_at(p, i) == cc.SINGLE_EXPECT[name] and p["valid"][i] >= 16, (name, cc.class_at(p, i), int(p["valid"][i]))
    assert c["quadrants"] == {cc.class_name(k): (1 if k in ((0, 0, 0), (1, 0, 1), (1, 1, 0)) else 114 if k == (1, 0, 0) else 0) for k in cc.CLASSES}
    assert c["loops"][cc.NOSEP] >= 1 and sum(c["loops"][cc.batch_name(0, 1, n, 1)] for n in (0, 1)) >= 1
    assert sum(c["loops"][cc.loop_of(1, 1, 0, n, pairs)] for n in (0, 1)) >= 1


@pytest.mark.parametrize("layout,pairs,null", [("gated", 1, False), ("gated", 0, False), ("image_only", 1, True), ("image_only", 0, False)])
def test_sparse_early_returns_and_tail_batches_only(hip_lib, layout, pairs, null):
    """A few small Gaussians: quadrants without a contributor return at once, every other list is shorter than one batch.  `gated`:
    all four gradients on every pixel, so dL_dacc and flow gradients meet pixels with acc == 0 (gated off) and depth gradients too (kept,
    undivided)."""
    lay = cc.dense if layout == "gated" else (lambda H, W: cc.image_only(H, W, null=null))
    o, g, gb, c = _case("sparse", lay, pairs, layout + (" null" if null else ""))
    assert c["early_return"] >= 1 and c["batches"] >= 100
    assert c["batches"] == sum(c["tail_sizes"].values()) and c["ring_wrap_quadrants"] == 0
    assert all(v == 0 for k, v in c["loops"].items() if "NOLAST=1" in k)
    assert int((g["acc"] == 0).sum()) >= 500
    if layout == "gated":
        # unlit pixels still decide `extra` through their depth gradient; quadrants without a lit pixel never take `gacc`
        p = c["per_quadrant"]
        lit = cc._quads(g["acc"].cpu().numpy().reshape(cc.SPARSE.height, cc.SPARSE.width) > 0, cc.SPARSE.width, cc.SPARSE.height, False).any(1)
        live = p["inside"] & (p["deepest"] > 0)
        assert p["extra"][live].all() and not p["gacc"][live & ~lit].any() and p["gacc"][live & lit].all()


@pytest.mark.parametrize("scene", ["deep", "wrap"])
def test_census_equals_the_kernels_own_counters(hip_lib, scene):
    """The census is a restatement of the dispatch; the statistics variant of the kernel counts what it did.  Batches and valid entries
    agree exactly on DEEP x mixed and WRAP x mixed, so the coverage asserted above is the kernel's and not the restatement's."""
    from ex4dgs_amd import _C
    cfg, dir_scale = SCENES[scene]
    sub, grads = cc.mixed(cfg.height, cfg.width)
    ins, st = h.scene_inputs(cfg, dir_scale=dir_scale)
    g = h.gpu_forward_raw(ins, st, subpixel_offset=sub)
    _C.bwd_stats(reset=True)
    _C.set_option("composite_bwd_variant", 8)
    try:
        h.gpu_backward_raw(ins, g, grads)
        torch.cuda.synchronize()
        stats = [int(x) for x in _C.bwd_stats(reset=True)]
    finally:
        _C.set_option("composite_bwd_variant", 4)
    c = _census_of(g, sub, grads, cfg, 0)
    rep = cc.report(c, f"{cfg.name} x mixed, composite_bwd_variant=8")
    rep["bwd_stats"] = stats[:2]
    h.REPORT.append(rep)
    assert c["batches"] >= 9 * 8 and c["ring_wrap_quadrants"] >= 1
    assert stats[0] == c["batches"], (stats[0], c["batches"])
    assert stats[1] == c["entries"], (stats[1], c["entries"])
