"""Every path of the compositing forward's walk against the CPU oracle (run with `-m gpu` on an MI355X).

composite_fwd_kernel walks the staged entries of a chunk with hand-scheduled inline assembly: two register sets, two variants (with and
without the v_min of alpha = min(0.99, w G)) in one asm statement, the rare paths Lrare / Ldead / Lgodd and a dominant-index key folded
once per group of 16.  tests/composite_fwd_cases.py restates its control flow (the census) and holds scenes that reach all 20 cells
(variant, set, outcome), the clamp deciding, every group and chunk boundary, every branch of the quadrant cull, and hand-built frames
whose two largest weights tie exactly.  Here every scene goes through _fwd_bwd of tests/test_gpu_parity.py -- the suite's oracle
comparison with its bars unchanged -- on the asm walk (dir3D = 0) and on the flow kernel; the census is then taken on the kernel's own
compacted lists and pinned to them, the quadrant cull is shown conservative, and the three walks (asm, asm with the clamp everywhere,
compiled) and the flow kernel are compared bit for bit.  tests/test_cpu_composite_fwd_cases.py asserts the data-only half without a GPU."""
import numpy as np
import pytest
import torch

from tests import composite_fwd_cases as fc
from tests import helpers as h
from tests.test_gpu_parity import _fwd_bwd

pytestmark = pytest.mark.gpu

SCENE_NAMES = list(fc.SCENES)
_RUN = {}              # (scene, dir_scale) -> (inputs, settings, oracle forward, GPU forward), shared by the tests below
_CENSUS = {}           # scene -> census on the kernel's own lists


def _defaults():
    from ex4dgs_amd import _C
    assert _C.get_option("composite_fwd_asm") == 1 and _C.get_option("composite_clamp_always") == 0
    return _C


def _run(name, dir_scale=0.0):
    """Oracle and GPU forward of a scene under the library's default walk (cached; the oracle comparison below fills the cache too)."""
    key = (name, dir_scale)
    if key not in _RUN:
        _defaults()
        ins, st = fc.scene_inputs(name, dir_scale)
        _RUN[key] = (ins, st, h.oracle_forward(ins, st), h.gpu_forward_raw(ins, st))
    return _RUN[key]


def _kernel_census(name):
    if name not in _CENSUS:
        _, _, o, g = _run(name)
        assert np.array_equal(o["point_list"].astype(np.int64), h.to_np(g["point_list"]).astype(np.int64))
        assert np.array_equal(o["ranges"].astype(np.int64), h.to_np(g["ranges"]).astype(np.int64))
        _CENSUS[name] = fc.census_of(o, g=g)
        h.REPORT.append(fc.report(_CENSUS[name], f"{fc.SCENES[name][0].name}, the kernel's own lists"))
    return _CENSUS[name]


def _valid_lists(g):
    """The valid prefixes of the per-quadrant compacted lists, as one array (quadrant by quadrant) with the quadrant of each entry."""
    ranges = h.to_np(g["ranges"]).astype(np.int64)
    ql, qc = h.to_np(g["qlist"]).astype(np.int64) & 0xFFFFFFFF, h.to_np(g["qcount"]).astype(np.int64).reshape(-1) & 0xFFFFFFFF
    n = ranges[:, 1] - ranges[:, 0]
    start = np.repeat(4 * ranges[:, 0], 4) + np.tile(np.arange(4), len(n)) * np.repeat(n, 4)
    assert (qc <= np.repeat(n, 4)).all()
    quad = np.repeat(np.arange(len(qc)), qc)
    at = np.repeat(start, qc) + (np.arange(int(qc.sum())) - np.repeat(np.cumsum(qc) - qc, qc))
    return ql[at], quad


@pytest.mark.parametrize("dir_scale", [0.0, 0.1])
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_scene_against_the_oracle(hip_lib, name, dir_scale):
    """_fwd_bwd with its bars unchanged: dir_scale = 0 launches the flow-free kernel with the hand-scheduled walk, 0.1 the flow kernel.
    On OPAQUE and STACK the clamp of alpha decides (w G > 0.99 on contributing pairs), in the forward and in the backward's pass-through."""
    _defaults()
    cfg, mutate = fc.SCENES[name]
    o, g, ob, gb, rep = _fwd_bwd(cfg, dir_scale=dir_scale, mutate=mutate)
    ins, st = fc.scene_inputs(name, dir_scale)
    _RUN[(name, dir_scale)] = (ins, st, o, g)
    flow = float(g["flow"].abs().max())
    assert (flow == 0.0) == (dir_scale == 0.0) and (float(np.abs(o["flow"]).max()) == 0.0) == (dir_scale == 0.0)
    if dir_scale == 0.0:
        c = _kernel_census(name)
        if name == "opaque":
            assert c["clamped_pairs"] >= 50, c["clamped_pairs"]


def test_the_kernels_own_lists_cover_every_path(hip_lib):
    """The coverage conditions of tests/test_cpu_composite_fwd_cases.py, on the census of what the kernel staged: all 20 cells, each common
    one at least 8 times per variant and set, every cnt mod 16, empty chunks, chunks ending on set a, abandoned on either set, second
    chunks, the clamp deciding on 50 pairs, every branch of the cull with both outcomes."""
    by_scene = {name: _kernel_census(name) for name in SCENE_NAMES}
    fc.assert_coverage(by_scene)
    assert min(by_scene["stack"]["cells"][fc.cell("clamp", s, "rare_skip")] for s in fc.SETS) >= 1
    assert sum(1 for r in h.REPORT if r.get("kind") == "composite_fwd_census") >= len(SCENE_NAMES)


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_census_is_pinned_to_the_kernel(hip_lib, name):
    """The census replays the kernel's lists; the kernel in turn staged what the replay (with the cull restated in numpy) says it had to:
    per quadrant without a fragile pixel, entries only in chunks that were live, the same number of chunks walked, a non-zero qcount
    wherever the replay staged something -- and the replay's last contributor and dominant entry are the kernel's n_contrib and idx."""
    _, _, o, g = _run(name)
    W, H = o["W"], o["H"]
    ck = _kernel_census(name)
    cn = fc.census_of(o)                                           # the numpy cull instead of qlist / qcount
    fragile_px = int((o["fragile"] <= h.FRAG_EPS).sum())
    fq = fc.fragile_quadrants(o["fragile"], W, H, h.FRAG_EPS)
    assert int(fq.sum()) <= fragile_px
    pk, pn = ck["per_quadrant"], cn["per_quadrant"]
    pos, quad = _valid_lists(g)
    qc = h.to_np(g["qcount"]).astype(np.int64).reshape(-1)
    assert np.array_equal(np.concatenate(pk["lists"] + [np.zeros(0, np.int64)]), pos)          # the census walked these very lists
    solid_q = ~fq
    assert np.array_equal(pk["chunks"][solid_q], pn["chunks"][solid_q])
    assert np.array_equal(pk["last_live_chunk"][solid_q], pn["last_live_chunk"][solid_q])
    # no entry behind the last live chunk; entries only in live chunks (chunks are walked in order: live = 0 .. last_live_chunk)
    keep = solid_q[quad]
    assert (pos[keep] // fc.CHUNK <= pn["last_live_chunk"][quad[keep]]).all()
    assert (qc[solid_q & (pn["staged"] > 0)] > 0).all() and (qc[pn["chunks"] == 0] == 0).all()
    same = sum(1 for i in np.flatnonzero(solid_q) if np.array_equal(pk["lists"][i], pn["lists"][i]))      # reported, not asserted
    # the replay of the kernel's lists gives the kernel's per-pixel state
    solid = o["fragile"] > h.FRAG_EPS
    assert np.array_equal(pk["last"][solid], h.to_np(g["n_contrib"]).astype(np.int64).reshape(H, W)[solid])
    decided = solid & (o["idx_margin"] > h.IDX_BAND)
    assert np.array_equal(pk["dom"][decided], h.to_np(g["idx"]).astype(np.int64).reshape(H, W)[decided])
    h.REPORT.append(dict(kind="composite_fwd_pinned", tag=fc.SCENES[name][0].name, fragile_pixels=fragile_px, fragile_quadrants=int(fq.sum()),
                         quadrants_with_identical_lists=int(same), entries_differing_from_numpy_cull=int(ck["cull_differs"]),
                         staged_by_kernel=int(ck["staged_entries"]), staged_by_numpy_cull=int(cn["staged_entries"])))


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_quadrant_cull_is_conservative(hip_lib, name):
    """Every list position of a walked chunk at which some inside pixel of the quadrant has power <= 0 and alpha >= (1 + 1e-4) / 255 in
    float64 is in the quadrant's compacted list.  (How many entries differ from the numpy restatement of the cull is reported, not asserted.)"""
    ck = _kernel_census(name)
    assert ck["from_kernel_lists"] == 1 and ck["chunks"] >= 100
    assert ck["cull_missed"] == 0, ck["cull_missed"]
    print(f"{name}: {ck['cull_differs']} of {sum(ck['cull'].values())} cull decisions differ from the numpy restatement")


def _same_bits(a, b, keys, what):
    for k in keys:
        assert torch.equal(a[k], b[k]), (what, k)
    pa, qa = _valid_lists(a)
    pb, qb = _valid_lists(b)
    assert np.array_equal(pa, pb) and np.array_equal(qa, qb), (what, "qlist")


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_three_walks_and_the_flow_kernel_same_bits(hip_lib, name):
    """composite_fwd_asm 1 against 0 and composite_clamp_always 0 against 1: colour, depth, acc, idx, final_T, n_contrib, qcount and the
    valid prefixes of qlist agree bit for bit -- on scenes whose census shows both variants, every cell and the clamp deciding.  The flow
    kernel (dir3D != 0) agrees with them on every output that does not depend on dir3D."""
    _C = _defaults()
    ins, st, o, a = _run(name)
    keys = fc.FLOW_INDEPENDENT + ("qcount", "flow")
    try:
        _C.set_option("composite_fwd_asm", 0)
        b = h.gpu_forward_raw(ins, st)
        _C.set_option("composite_fwd_asm", 1)
        _C.set_option("composite_clamp_always", 1)
        c = h.gpu_forward_raw(ins, st)
        _C.set_option("composite_fwd_asm", 0)
        d = h.gpu_forward_raw(ins, st)
    finally:
        _C.set_option("composite_fwd_asm", 1)
        _C.set_option("composite_clamp_always", 0)
    _same_bits(a, b, keys, "compiled walk")
    _same_bits(a, c, keys, "asm walk, clamp everywhere")
    _same_bits(a, d, keys, "compiled walk, clamp everywhere")
    _, _, of, f = _run(name, 0.1)
    _same_bits(a, f, fc.FLOW_INDEPENDENT + ("qcount",), "flow kernel")
    assert float(a["flow"].abs().max()) == 0.0 and float(f["flow"].abs().max()) > 0.0
    _defaults()


@pytest.mark.parametrize("k", fc.TIE_FILLERS)
def test_first_of_two_tied_entries_is_the_dominant_one(hip_lib, k):
    """Two Gaussians on the optical axis whose blending weights at the centre pixel are equal bit for bit, behind k fillers: the tied
    entries sit at j = (0, 1), (14, 15) -- inside one group of the key fold -- (15, 16) -- across two groups -- and at list positions 63
    and 64 -- in two chunks.  idx at the centre pixel is the id of the first one (CR/forward.cu:411-415: strict >) in the asm walk, the
    asm walk with the clamp everywhere, the compiled walk and the flow kernel."""
    _C = _defaults()
    cx, cy = fc.TIE_CENTRE
    ins, st = fc.tie_inputs(k)
    o = h.oracle_forward(ins, st)
    assert o["idx_margin"][cy, cx] == 0.0 and o["idx"][0, cy, cx] == fc.TIE_FIRST
    first, second = fc.tie_positions(o, fc.census_of(o, dtype=np.float32))
    assert first[1] == k % fc.CHUNK and second == ((k + 1) // fc.CHUNK, (k + 1) % fc.CHUNK)
    insf, stf = fc.tie_inputs(k, dir_scale=0.1)
    solid = (o["fragile"] > h.FRAG_EPS) & (o["idx_margin"] > h.IDX_BAND)
    solid[cy, cx] = True
    got = {}
    try:
        for walk, (asm, clamp, flow) in {"asm": (1, 0, False), "asm, clamp everywhere": (1, 1, False), "compiled": (0, 0, False),
                                         "flow kernel": (1, 0, True)}.items():
            _C.set_option("composite_fwd_asm", asm)
            _C.set_option("composite_clamp_always", clamp)
            got[walk] = h.gpu_forward_raw(insf, stf) if flow else h.gpu_forward_raw(ins, st)
    finally:
        _C.set_option("composite_fwd_asm", 1)
        _C.set_option("composite_clamp_always", 0)
    i = fc.tie_quadrant()
    for walk, g in got.items():
        assert np.array_equal(o["point_list"].astype(np.int64), h.to_np(g["point_list"]).astype(np.int64)), walk
        pair = [fc.TIE_FIRST, fc.TIE_SECOND]
        assert np.array_equal(o["conic_opacity"][pair].view(np.uint32), h.to_np(g["conic_opacity"])[pair].view(np.uint32)), walk
        assert (float(g["flow"].abs().max()) > 0.0) == (walk == "flow kernel")
        pos, quad = _valid_lists(g)
        assert np.array_equal(pos[quad == i], np.arange(k + 2)), walk                 # all staged: the tied entries sit where the census put them
        idx = h.to_np(g["idx"]).reshape(fc.TIE_H, fc.TIE_W)
        assert idx[cy, cx] == fc.TIE_FIRST, (walk, k, int(idx[cy, cx]))
        assert int(h.to_np(g["n_contrib"]).reshape(fc.TIE_H, fc.TIE_W)[cy, cx]) == k + 2
        assert np.array_equal(idx[solid], o["idx"][0][solid]), walk
    _defaults()
