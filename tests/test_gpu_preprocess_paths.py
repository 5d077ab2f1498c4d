"""The per-Gaussian kernels (ex4dgs_amd/csrc/ex4d_preprocess.hip) against the CPU oracle on frames the view frustum cuts through (run with
`-m gpu` on an MI355X).

tests/preprocess_cases.py holds the frames -- every row placed by a plan: culled by each plane of the frustum test, passing it with an
empty tile rect, NaN, rendered; lane patterns per wave that put culled and needed rows next to each other in both 32-lane halves; every
SH layout; the wave, workgroup and alignment edges -- and tests/test_cpu_preprocess_cases.py proves on the CPU that each frame realises
its plan and that the table reaches every path with every pattern.  Here each frame runs through the raw C ABI (tests/raw_abi.py) on
NaN-poisoned, guarded buffers under every setting of

    preprocess_sh_predicate {0, 1}  x  preprocess_fast_path {0, 1}  x  prepare_backward {0, 1}

and is compared with ONE oracle forward: helpers.compare_forward (radii on all rows; depth, mean2D, conic, colour and clamp bits bit for
bit on rendered rows; point_list, ranges, num_rendered -- through them the depth keys and the published key range; the images), the eight
settings among each other byte for byte, the direction sums the forward leaves for the backward, and the backward's per-Gaussian stage
bit for bit against oracle.preprocess_backward on the GPU's own accumulators -- for the concatenated and for the split layout."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from tests import helpers as h
from tests import preprocess_cases as pc
from tests import raw_abi

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in pc.RUNNABLE]
GRID = [(pred, fast, prep) for pred in (0, 1) for fast in (0, 1) for prep in (0, 1)]
FILL = "ones"                                  # bytes 0xFF: NaN as a float -- a row nobody wrote cannot pass as a zero
GEOMETRY = ("depths", "means2D", "conic_opacity", "rgb", "clamped")              # per-Gaussian arrays, defined on rendered rows
WHOLE = ("radii", "color", "depth", "acc", "flow", "idx", "point_list", "ranges", "final_T", "n_contrib")


@contextlib.contextmanager
def _options(pred, fast):
    from ex4dgs_amd import _C
    saved = {k: _C.get_option(k) for k in ("preprocess_sh_predicate", "preprocess_fast_path")}
    assert saved == {"preprocess_sh_predicate": 1, "preprocess_fast_path": 1}, saved          # the library's defaults
    try:
        _C.set_option("preprocess_sh_predicate", pred)
        _C.set_option("preprocess_fast_path", fast)
        yield
    finally:
        for k, v in saved.items():
            _C.set_option(k, v)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _forward(f, bufs, prep, **over):
    c = f.case
    g = raw_abi.forward(f.ins, dict(f.settings, **over), bufs, fill=FILL, prepare_backward=bool(prep), n_static=c.n_static if c.layout == "split" else None,
                        split_offset=c.in_offset)
    return g


def _direction_sums(g, P):
    """The [P,9] array the forward leaves for the backward: the last array of the geometry buffer."""
    from ex4dgs_amd import _C
    lay = _C.GeomLayout()
    _C.load().ex4d_geom_layout(P, ctypes.byref(lay))
    off = lay.total - ((36 * P + 255) // 256) * 256
    return g["geomBuffer"][off: off + 36 * P].view(torch.int32).view(P, 9)


def _upstream(o):
    """helpers.upstream_grads, masked on the oracle's fragile pixels as _fwd_bwd of tests/test_gpu_parity.py does."""
    Hh, Ww = o["H"], o["W"]
    grads = h.upstream_grads(torch.from_numpy(o["acc"]), Hh, Ww, seed=3, grad_acc_zero=False)
    solid = torch.from_numpy(o["fragile"] > h.FRAG_EPS)
    return [x * solid[None] for x in grads]


def _check_backward(f, o, g, b, what):
    c = f.case
    P = c.P
    assert b["rc"] == 0, (what, b["error"])
    b["bufs"].assert_guards_intact()
    b["bufs"].assert_guards_intact(raw_abi.STATE_BUFFERS)
    dead = torch.from_numpy(~f.visible)
    for k, t in b["written"].items():
        assert not bool(torch.isnan(t).any()), f"{what}: {k} holds NaN: a row nobody wrote, or one computed from rows that were not loaded"
        assert raw_abi.leftover_fill(t, FILL) == 0, (what, k)
        if t.numel() and k not in raw_abi.SPLIT_GRAD_NAMES:
            rows = t.reshape(P, -1)[dead.to(t.device)]
            assert int((_bits(rows) != 0).sum()) == 0, f"{what}: {k} is not exactly zero on rows with radii == 0"
    h.assert_per_gaussian_stage_bit_exact(o, b)
    if c.layout == "split":
        # the four parts: fully written (checked above: no NaN), exact zeros on rows with radii == 0, and put together they are the
        # [P,16,3] gradient the stage check above has just compared bit for bit with the oracle's
        n = c.n_static
        parts = [b[k] for k in raw_abi.SPLIT_GRAD_NAMES]
        assert [tuple(p.shape) for p in parts] == [(n, 1, 3), (n, 15, 3), (P - n, 1, 3), (P - n, 15, 3)]
        for p, rows in zip(parts, (dead[:n], dead[:n], dead[n:], dead[n:])):
            if p.numel():
                assert int((_bits(p.reshape(p.shape[0], -1)[rows.to(p.device)]) != 0).sum()) == 0, f"{what}: a split gradient part is not zero on a row with radii == 0"
        live = b["dL_dsh"][torch.from_numpy(f.visible).to(b["dL_dsh"].device)]
        if c.D > 0 and live.numel():
            assert float(live[:, 1:(c.D + 1) ** 2].abs().max()) > 0.0            # the rest parts carry gradients at all
        assert float(b["dL_dsh"][:, (c.D + 1) ** 2:].abs().max() if c.D < 3 else 0.0) == 0.0
        # the floats in front of misaligned parts keep their fill
        for k, lead in b["split_grad_lead"].items():
            assert lead.numel() == c.grad_offset and bool(torch.isnan(lead).all()), (what, k)


@pytest.mark.parametrize("name", NAMES)
def test_frame_against_the_oracle_under_every_setting(hip_lib_both, name):
    f = pc.frame(name)
    c = f.case
    P = c.P
    o = pc.oracle_forward(name)
    assert np.array_equal(o["radii"] > 0, f.visible)                              # the plan (tests/test_cpu_preprocess_cases.py)
    vis = torch.from_numpy(f.visible).cuda()
    grads = _upstream(o)
    has_sh = c.layout != "colors"
    bufs = raw_abi.Buffers()
    kept = {}
    for pred, fast, prep in GRID:
        what = f"{name} [predicate {pred}, fast path {fast}, prepare_backward {prep}]"
        with _options(pred, fast):
            g = _forward(f, bufs, prep)
            assert g["rc"] == 0, (what, g["error"])
            bufs.assert_guards_intact()
            h.compare_forward(o, g, tag=what)
            for k in raw_abi.FORWARD_OUTPUTS:
                assert raw_abi.leftover_fill(g[k], FILL) == 0 or k in ("radii", "idx"), (what, k)      # (-1 is a value of idx)
            assert bool((g["radii"] >= 0).all())
            flow_expected = bool((pc.flow_carriers(f) & f.visible).any())
            assert (float(g["flow"].abs().max()) > 0.0) == flow_expected == (float(np.abs(o["flow"]).max()) > 0.0), what
            snap = {k: _bits(g[k]).clone() for k in WHOLE}
            snap.update({k: _bits(g[k])[vis].clone() for k in GEOMETRY if not (k in ("rgb", "clamped") and not has_sh)})
            snap["num_rendered"] = g["num_rendered"]
            if prep and has_sh:
                snap["dsums"] = _direction_sums(g, P)[vis].clone()
                assert not bool(torch.isnan(snap["dsums"].view(torch.float32)).any()), what
            b = raw_abi.backward(g, grads, fill=FILL, prepared=bool(prep), split_grad_offset=c.grad_offset)
            _check_backward(f, o, g, b, what)
        kept[(pred, fast, prep)] = snap
    # all eight settings: byte-identical per-Gaussian arrays and images
    ref = kept[GRID[0]]
    for key, snap in kept.items():
        for k, v in snap.items():
            if k == "dsums":
                continue
            same = (v == ref[k]) if k == "num_rendered" else torch.equal(v, ref[k])
            assert same, f"{name}: {k} differs between settings {GRID[0]} and {key}"
    # ... and the direction sums of rendered rows, between the predicate off and on, the generic and the specialised kernel
    sums = [snap["dsums"] for key, snap in kept.items() if "dsums" in snap]
    assert len(sums) == (4 if has_sh else 0)
    for s in sums[1:]:
        assert torch.equal(s, sums[0]), f"{name}: the direction sums differ between two settings"


@pytest.mark.parametrize("name", pc.THRESHOLD_CASES)
def test_depth_plane_on_a_gaussians_own_depth(hip_lib, name):
    """min_depth equal to a Gaussian's float32 view depth culls it (<=), max_depth equal to it keeps it (> fails) -- under both
    settings of the predicate, whose frustum test runs in another place of the kernel."""
    f = pc.frame(name)
    for pred in (0, 1):
        with _options(pred, 1):
            g = _forward(f, raw_abi.Buffers(), 0)
        assert g["rc"] == 0, g["error"]
        assert bool(g["radii"][f.marked] > 0) == (f.case.special == "max_depth"), (name, pred)
        assert np.array_equal(h.to_np(g["radii"]) > 0, f.visible)


@pytest.mark.parametrize("name", pc.PREFILTER_CASES)
def test_prefiltered_is_refused_when_one_gaussian_is_culled(hip_lib, name):
    """The single culled Gaussian is lane 0 of wave 0 / the last row of a partial last wave: the chunk's flag reaches the host."""
    f = pc.frame(name)
    assert int((~f.frustum).sum()) == 1
    for pred in (0, 1):
        with _options(pred, 1):
            with pytest.raises(RuntimeError, match="filtered although prefiltered"):
                h.gpu_forward_raw(f.ins, dict(f.settings, prefiltered=True))
            g = _forward(f, raw_abi.Buffers(), 0, prefiltered=True)
            assert g["rc"] != 0 and "filtered although prefiltered" in g["error"], (g["rc"], g["error"])
    # the same frames with the culled row taken out pass
    keep = torch.from_numpy(f.frustum)
    ins = {k: (v[keep].contiguous() if v is not None else None) for k, v in f.ins.items()}
    g = h.gpu_forward_raw(ins, dict(f.settings, prefiltered=True))
    assert g["num_rendered"] == pc.oracle_forward(name)["num_rendered"]


def test_fewer_coefficients_than_the_degree_needs_is_refused(hip_lib):
    """shs [P,4,3] at degree 3: the reference would read twelve coefficients past every row.  The library's argument check refuses the
    frame before any kernel runs, and leaves the outputs alone."""
    (c,) = [x for x in pc.CASES if x.refused]
    f = pc.frame(c.name)
    bufs = raw_abi.Buffers()
    g = raw_abi.forward(f.ins, f.settings, bufs, fill=FILL)
    assert g["rc"] != 0 and c.refused in g["error"], (g["rc"], g["error"])
    bufs.assert_guards_intact()
    assert bool(torch.isnan(g["color"]).all()) and bool((g["radii"] == -1).all())
