"""The rasterizer on poisoned, guarded and reused caller buffers (run with `-m gpu` on an MI355X).

include/ex4d_rasterizer.h promises that every output is fully written, that the three state buffers may arrive with any content
and that nothing outside a buffer is touched; `ex4dgs_amd._C` hands the library `torch.empty` memory, so whether a word that is
read before it is written shows depends on what the allocator returns.  Here tests/raw_abi.py drives the C ABI on buffers the
test owns -- [guard | payload | guard], prefilled with zeros, 0xFF bytes (NaN / -1), 0x3C bytes (a small finite float) or left as
the previous frame left them -- over one table of kernel chains (depth sort x tile sort x rect form x digit width x ranking x
synchronous / asynchronous x debug arrays) and inputs.  The forward is deterministic: every frame must be bit-identical to the
same frame on zero-filled buffers, and that one to the path every other test uses.  The backward sums with float atomics: it is
held to the bar two runs of one backward are held to (tests/test_gpu_parity.py: test_backward_reproducible_to_rounding), its
per-Gaussian stage bit-exactly to the oracle's on the GPU's own accumulators.

DESIGN.md ("Written before read") is the audit this table follows; tests/test_cpu_buffer_contract.py checks, without a GPU, that
the table reaches every kernel chain the host code can select."""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

from ex4dgs_amd.scene import CONFIGS, SceneConfig
from tests import helpers as h
from tests import raw_abi

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ the table
# Every option the table touches, at the library's default (ex4d_api.hip); an entry's overrides go on top, and every frame sets them
# all (setting "depth_sort_msd" also resets the auto mode's hold, so which sort a frame takes does not depend on the frames before it).
BASE_OPTIONS = dict(geom_debug_arrays=0, binning_tile_ids=0, depth_sort_msd=3, depth_sort_msd_bits=0, depth_sort_local_cap=0,
                    depth_sort_local_threads=0, tile_sort_rows=1, rank_lds_atomics=-1)
TEST_OPTIONS = dict(geom_debug_arrays=1, binning_tile_ids=1)           # what the `hip_lib` fixture switches on (conftest.py)

# kind: "cfg" (helpers.scene_inputs on a named or literal configuration), "wall" (test_gpu_round5._squeezed: a depth wall),
# "scaled" (cfg1 with every scale x 30: giant rects), "behind" (cfg1 with everything behind the near plane: R = 0)
Scene = namedtuple("Scene", "name kind cfg P t")
Variant = namedtuple("Variant", "name scene extras options")

CFG1 = Scene("cfg1", "cfg", "cfg1", None, 0)
CFG2_1 = Scene("cfg2 P=1", "cfg", "cfg2", 1, 0)
CFG2_2049 = Scene("cfg2 P=2049", "cfg", "cfg2", 2049, 0)
CFG3 = Scene("cfg3 P=12000 t=137", "cfg", "cfg3", 12000, 137)
CFG5 = Scene("cfg5 P=6000 2048x1088", "cfg", "cfg5", 6000, 0)
CFG3C = Scene("cfg3c P=20000", "cfg", "cfg3c", 20000, 0)
SMALL = Scene("128x96", "cfg", SceneConfig("small image", 3000, 128, 96, 110.0, seed=5), None, 0)                     # 48 tiles: the radix pair sort
HUGE = Scene("4112x4112", "cfg", SceneConfig("huge: 4112x4112", 1500, 4112, 4112, 2200.0, seed=31, sigma_px_med=30.0), None, 0)      # 257 x 257 tiles: 8-byte rects
STRIP = Scene("4112x32", "cfg", SceneConfig("strip: 4112x32", 800, 4112, 32, 2200.0, seed=32, sigma_px_med=12.0), None, 0)          # 257 x 2 tiles: 8-byte rects, MSD pair sort
TINY = Scene("131x67", "cfg", SceneConfig("odd image: 131x67", 500, 131, 67, 90.0, seed=7, sigma_px_med=4.0), None, 0)             # partial tiles on both edges
WALL = Scene("depth wall", "wall", "cfg2", 30000, 0)          # 14000 of 30000 Gaussians at one depth: a bucket beyond the LDS capacity
GIANT = Scene("cfg1 scales x 30", "scaled", "cfg1", None, 0)
BEHIND = Scene("cfg1 behind the near plane", "behind", "cfg1", None, 0)

# extras: Ex4dParams fields (prepare_backward, asynchronous -> instance_capacity, assume_no_flow) and input forms (dir: "rand" /
# "zero" / "null"; colors_precomp, cov3D_precomp, sh4 = shs[P,4,3] at degree 1, n_static = split SH, subpixel); bwd = the entry
# also runs through the backward matrix
ASYNC = dict(asynchronous=1)


def _chain(scene):
    """depth sort x digit width x tile sort x synchronous / asynchronous on one scene"""
    out = []
    for msd in (0, 1, 2):
        for bits in ((9, 10) if msd else (0,)):
            for rows in (1, 0):
                for asyn in (0, 1):
                    name = f"{scene.name}: depth_sort_msd={msd}" + (f" bits={bits}" if bits else "") + f" tile_sort_rows={rows}" + (" async" if asyn else "")
                    out.append(Variant(name, scene, dict(ASYNC) if asyn else {}, dict(depth_sort_msd=msd, depth_sort_msd_bits=bits, tile_sort_rows=rows)))
    return out


VARIANTS = [
    # library defaults (auto depth sort, row-segment sort, probed LDS ranking) and the test options
    Variant("cfg1 defaults", CFG1, dict(bwd=1), {}),
    Variant("cfg1 test options", CFG1, dict(bwd=1), TEST_OPTIONS),
    Variant("cfg3 defaults", CFG3, dict(bwd=1), {}),
    Variant("cfg3 test options", CFG3, dict(bwd=1), TEST_OPTIONS),
    # depth sort: buckets through memory, an oversize bucket
    Variant("cfg3 buckets through memory, fused row sort", CFG3, {}, dict(depth_sort_msd=2, depth_sort_local_threads=256, depth_sort_local_cap=64)),
    Variant("cfg3 buckets through memory, fused tile scan", CFG3, {}, dict(depth_sort_msd=2, depth_sort_local_threads=256, depth_sort_local_cap=64, tile_sort_rows=0)),
    Variant("cfg3 buckets through memory, scan kernel", CFG3, {}, dict(depth_sort_msd=1, depth_sort_local_threads=256, depth_sort_local_cap=64, tile_sort_rows=0)),
    Variant("depth wall, MSD sort", WALL, {}, dict(depth_sort_msd=2)),
    Variant("depth wall, MSD sort, fused tile scan from memory", WALL, {}, dict(depth_sort_msd=2, tile_sort_rows=0)),
    Variant("depth wall, auto", WALL, {}, {}),
    # tile sort: pair sorts (the chains below), 8-byte rects, 2048x1088
    Variant("4112x4112 defaults", HUGE, {}, {}),
    Variant("4112x4112 async", HUGE, dict(ASYNC), {}),
    Variant("4112x32 defaults", STRIP, {}, {}),
    Variant("4112x32 async", STRIP, dict(ASYNC), {}),
    Variant("cfg5 defaults", CFG5, dict(bwd=1), {}),
    Variant("cfg5 pair sort", CFG5, {}, dict(tile_sort_rows=0)),
    Variant("cfg5 test options, LSD", CFG5, {}, dict(TEST_OPTIONS, depth_sort_msd=0)),
    # ranking by ballots
    Variant("cfg3 ballots", CFG3, {}, dict(rank_lds_atomics=0)),
    Variant("cfg2 P=2049 ballots, LSD, pair sort", CFG2_2049, {}, dict(rank_lds_atomics=0, depth_sort_msd=0, tile_sort_rows=0)),
    Variant("128x96 ballots, MSD, radix pair sort", SMALL, {}, dict(rank_lds_atomics=0, depth_sort_msd=2, tile_sort_rows=0)),
    # asynchronous forward, with and without flow
    Variant("cfg3 async, with flow", CFG3, dict(ASYNC, bwd=1), {}),
    Variant("cfg3 async, assume_no_flow", CFG3, dict(ASYNC, assume_no_flow=1, dir="zero", bwd=1), {}),
    Variant("cfg3 async, test options, prepare_backward", CFG3, dict(ASYNC, prepare_backward=1), TEST_OPTIONS),
    # inputs
    Variant("cfg1 dir3D NULL", CFG1, dict(dir="null", bwd=1), {}),
    Variant("cfg1 dir3D all 0", CFG1, dict(dir="zero", bwd=1), {}),
    Variant("cfg3 dir3D all 0", CFG3, dict(dir="zero"), {}),
    Variant("cfg1 colors_precomp", CFG1, dict(colors_precomp=1, bwd=1), {}),
    Variant("cfg1 cov3D_precomp", CFG1, dict(cov3D_precomp=1, bwd=1), {}),
    Variant("cfg1 colors_precomp + cov3D_precomp, test options", CFG1, dict(colors_precomp=1, cov3D_precomp=1, bwd=1), TEST_OPTIONS),
    Variant("cfg3 split SH", CFG3, dict(n_static=9001, bwd=1), {}),
    Variant("cfg3 split SH, prepare_backward", CFG3, dict(n_static=9001, prepare_backward=1, bwd=1), {}),
    Variant("cfg1 split SH, empty dynamic part", CFG1, dict(n_static=256, bwd=1), {}),
    Variant("cfg1 split SH, empty static part", CFG1, dict(n_static=0, bwd=1), {}),
    Variant("cfg1 shs[P,4,3] degree 1", CFG1, dict(sh4=1, bwd=1), {}),
    Variant("cfg1 prepare_backward", CFG1, dict(prepare_backward=1, bwd=1), {}),
    Variant("cfg3 prepare_backward", CFG3, dict(prepare_backward=1, bwd=1), {}),
    Variant("cfg1 subpixel_offset", CFG1, dict(subpixel=1, bwd=1), {}),
    Variant("cfg3 subpixel_offset, test options", CFG3, dict(subpixel=1), TEST_OPTIONS),
    # scenes
    Variant("cfg2 P=1", CFG2_1, dict(bwd=1), {}),
    Variant("cfg2 P=1 LSD", CFG2_1, {}, dict(depth_sort_msd=0)),
    Variant("cfg2 P=2049", CFG2_2049, dict(bwd=1), {}),
    Variant("cfg3c", CFG3C, dict(bwd=1), {}),
    Variant("giant rects", GIANT, dict(bwd=1), {}),
    Variant("giant rects, pair sort", GIANT, {}, dict(tile_sort_rows=0)),
    Variant("nothing visible", BEHIND, dict(bwd=1), {}),
    Variant("nothing visible, async, pair sort", BEHIND, dict(ASYNC), dict(tile_sort_rows=0)),
    Variant("131x67", TINY, dict(bwd=1), {}),
    Variant("131x67 test options, LSD, pair sort", TINY, {}, dict(TEST_OPTIONS, depth_sort_msd=0, tile_sort_rows=0)),
] + _chain(CFG2_2049) + _chain(SMALL)
assert len({v.name for v in VARIANTS}) == len(VARIANTS)
BWD_VARIANTS = [v for v in VARIANTS if v.extras.get("bwd")]

# fills of the forward matrix: the four modes of tests/raw_abi.py, and `ones` / `finite` on the outputs alone (state buffers zeroed)
FWD_FILLS = ("zero", "stale", "ones-outputs", "finite-outputs", "ones", "finite")
BWD_FILLS = ("zero", "stale", "ones", "finite")
# test ids by what a fill may reach: `-k "fillzero or fillstale"` (benign), `-k fillouts` (floats only), `-k fillall` (state buffers too)
FILL_ID = {"zero": "fillzero", "stale": "fillstale", "ones-outputs": "fillouts-ones", "finite-outputs": "fillouts-finite", "ones": "fillall-ones",
           "finite": "fillall-finite"}.get
PRIMER = Variant("primer", Scene("cfg2 P=5000", "cfg", "cfg2", 5000, 0), dict(prepare_backward=1), {})        # the frame a `stale` buffer held before


def scene_shape(scene):
    """(P, W, H, min_depth, max_depth) of a table scene without building it (tests/test_cpu_buffer_contract.py)."""
    c = CONFIGS[scene.cfg] if isinstance(scene.cfg, str) else scene.cfg
    return (scene.P if scene.P is not None else c.P), c.width, c.height, c.min_depth, c.max_depth


def capacity_of(scene):
    """instance_capacity of the table's asynchronous entries: comfortably above the frame's count (asserted where it is used)"""
    return 2_400_000 if scene is HUGE else max(400_000, 60 * scene_shape(scene)[0])          # (4112x4112: 0.97 M instances of 1500 Gaussians)


# ------------------------------------------------------------------------------------------------ frames
@functools.lru_cache(maxsize=4)
def _scene(scene):
    if scene.kind == "wall":
        from tests.test_gpu_round5 import _squeezed
        ins, st = _squeezed(scene.P, 6.0, 6.4, 14000)
        return {k: v.cpu() for k, v in ins.items()}, st
    ins, st = h.scene_inputs(scene.cfg, P=scene.P, t=scene.t)
    if scene.kind == "scaled":
        ins["scales"] = ins["scales"] * 30.0
    if scene.kind == "behind":
        ins["means3D"] = ins["means3D"].clone()
        ins["means3D"][:, 2] = 1.0
    return ins, st


def _cov3d(ins):
    """R S^2 R^T from scale / raw quaternion in float64 (tests/test_gpu_parity.py: the precomputed-covariance case)"""
    P = ins["means3D"].shape[0]
    s, q = ins["scales"].numpy().astype(np.float64), ins["rotations"].numpy().astype(np.float64)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                  2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(P, 3, 3)
    S = R * s[:, None, :]
    Sig = S @ S.transpose(0, 2, 1)
    return torch.tensor(np.stack([Sig[:, 0, 0], Sig[:, 0, 1], Sig[:, 0, 2], Sig[:, 1, 1], Sig[:, 1, 2], Sig[:, 2, 2]], -1), dtype=torch.float32)


def frame_inputs(v):
    """(inputs, settings, subpixel offsets, keyword arguments of raw_abi.forward) of a table entry"""
    ins, st = _scene(v.scene)
    ins, st, x = dict(ins), dict(st), v.extras
    P = ins["means3D"].shape[0]
    if x.get("dir") == "null":
        ins["dir3D"] = None
    elif x.get("dir") == "zero":
        ins["dir3D"] = torch.zeros_like(ins["means3D"])
    if x.get("cov3D_precomp"):
        ins["cov3D_precomp"] = _cov3d(ins)
        ins["scales"] = ins["rotations"] = None
    if x.get("colors_precomp"):
        ins["colors_precomp"] = torch.rand(P, 3, generator=torch.Generator().manual_seed(2))
        ins["shs"] = None
    if x.get("sh4"):
        ins["shs"] = ins["shs"][:, :4, :].contiguous()
        st["sh_degree"] = 1
    sub = None
    if x.get("subpixel"):
        sub = torch.rand(st["image_height"], st["image_width"], 2, generator=torch.Generator().manual_seed(5)) - 0.5
    kw = dict(prepare_backward=bool(x.get("prepare_backward")), n_static=x.get("n_static"), assume_no_flow=bool(x.get("assume_no_flow")),
              instance_capacity=capacity_of(v.scene) if x.get("asynchronous") else 0)
    return ins, st, sub, kw


class options:
    """The table's options for one frame; whatever was set before comes back in `finally`."""

    def __init__(self, overrides):
        self.want = dict(BASE_OPTIONS, **overrides)

    def __enter__(self):
        from ex4dgs_amd import _C
        self.saved = {k: _C.get_option(k) for k in self.want}
        for k, val in self.want.items():
            if k == "depth_sort_msd" or self.saved[k] != val:        # (setting the ranking option makes the next forward probe again: only on a change)
                _C.set_option(k, val)

    def __exit__(self, *exc):
        from ex4dgs_amd import _C
        for k, val in self.saved.items():
            if k == "depth_sort_msd" or _C.get_option(k) != val:
                _C.set_option(k, val)


def run_forward(v, bufs, fill, state_fill=None):
    ins, st, sub, kw = frame_inputs(v)
    with options(v.options):
        f = raw_abi.forward(ins, st, bufs, fill=fill, state_fill=state_fill, subpixel_offset=sub, **kw)
    assert f["rc"] == 0, f["error"]
    return f


def _bits(t):
    return t.contiguous().view(torch.int32)


FWD_EXACT = ("color", "radii", "depth", "acc", "flow", "idx", "depth_order", "ranges", "final_T", "n_contrib")


def forward_snapshot(f):
    """What of a forward has to be the same bit for bit whatever its buffers held (clones: the buffers may be reused)."""
    R = f["num_rendered"]
    vis = f["radii"] > 0
    s = {k: _bits(f[k]).clone() for k in FWD_EXACT}
    s.update(num_rendered=R, point_list=_bits(f["point_list"][:R]).clone(), records=_bits(f["records"][vis]).clone(), status=f.get("status"))
    if f["inputs"]["colors_precomp"] is None:
        s["clamped"] = f["clamped"][vis].clone()
    return s


def assert_same_forward(a, ref, what):
    assert a["num_rendered"] == ref["num_rendered"], (what, a["num_rendered"], ref["num_rendered"])
    assert a["status"] == ref["status"], (what, a["status"], ref["status"])
    for k in ref:
        if k not in ("num_rendered", "status"):
            assert a[k].shape == ref[k].shape and torch.equal(a[k], ref[k]), f"{what}: {k} differs from the same frame on zero-filled buffers"


def check_forward_call(f, fill, what, ref=None):
    """Return code (run_forward), requested bytes, guards, no output element left unwritten (ref: the snapshot of the zero-fill run --
    an element whose computed value happens to have the bits of the `finite` pattern has them there as well; raw_abi.leftover_fill)."""
    assert f["asked"] == f["expected_bytes"], (what, f["asked"], f["expected_bytes"])
    touched = set(f["bufs"].touched)
    assert touched >= set(raw_abi.FORWARD_OUTPUTS) | set(raw_abi.STATE_BUFFERS) and (("status" in touched) == (f["params"].instance_capacity > 0))
    f["bufs"].assert_guards_intact()
    if f["params"].instance_capacity > 0:
        assert f["num_rendered"] <= f["params"].instance_capacity // 2, "the table's capacity is not comfortably above this frame's count"
    for k in raw_abi.FORWARD_OUTPUTS:
        if k == "idx" and fill == "ones":
            continue            # -1 is what the call writes where nothing contributed: covered by the bit comparison with the zero-fill run
        left = raw_abi.leftover_fill(f[k], fill, None if ref is None else ref[k])
        assert left == 0, f"{what}: {left} elements of {k} still hold the prefill"


_ZERO_RUN = {}       # variant name -> (snapshot, forward) of its zero-fill run (one entry: the parametrisation is variant-major)


def zero_run(v):
    if v.name not in _ZERO_RUN:
        _ZERO_RUN.clear()
        f = run_forward(v, raw_abi.Buffers(), "zero")
        _ZERO_RUN[v.name] = (forward_snapshot(f), f)
    return _ZERO_RUN[v.name]


def common_path_forward(v):
    """The same frame through ex4dgs_amd._C.rasterize_gaussians, the path every other test takes (helpers.gpu_forward_raw where that
    can express the entry; the same call with the entry's keyword arguments otherwise)."""
    from ex4dgs_amd import _C
    ins, st, sub, kw = frame_inputs(v)
    with options(v.options):
        if not (kw["prepare_backward"] or kw["instance_capacity"] or kw["n_static"] is not None):
            g = h.gpu_forward_raw(ins, st, subpixel_offset=sub)
        else:
            s = h.gpu_settings(st, "cuda", sub)
            e = torch.Tensor([])
            d = lambda k: ins[k].cuda() if ins.get(k) is not None else e
            sh = d("shs")
            if kw["n_static"] is not None:
                sh = _C.SplitSH(*raw_abi._split_parts(sh, kw["n_static"]))
            out = _C.rasterize_gaussians(s.bg, d("means3D"), d("dir3D"), d("colors_precomp"), d("opacities"), d("scales"), d("rotations"),
                                         s.scale_modifier, d("cov3D_precomp"), s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, s.kernel_size,
                                         s.subpixel_offset, s.image_height, s.image_width, sh, s.sh_degree, s.campos, s.prefiltered,
                                         s.min_depth, s.max_depth, s.debug, prepare_backward=kw["prepare_backward"],
                                         instance_capacity=kw["instance_capacity"], assume_no_flow=kw["assume_no_flow"])
            R, color, radii, geom, binning, img, depth, acc, flow, idx = out
            P, H, W = ins["means3D"].shape[0], s.image_height, s.image_width
            g = dict(num_rendered=int(R), color=color, radii=radii, depth=depth, acc=acc, flow=flow, idx=idx)
            g.update(_C.geom_views(geom, P))
            g.update(_C.binning_views(binning, R, W, H))
            g.update(_C.img_views(img, W, H))
            g["inputs"] = dict(colors_precomp=ins.get("colors_precomp"))
            g["status"] = None
        torch.cuda.synchronize()
    g.setdefault("inputs", dict(colors_precomp=ins.get("colors_precomp")))
    g.setdefault("status", None)
    return g


def _report(kind, v, fill, **more):
    h.REPORT.append(dict(kind=kind, tag=f"{v.name} [{fill}]", variant=v.name, fill=fill, options=dict(BASE_OPTIONS, **v.options),
                         extras={k: val for k, val in v.extras.items() if k != "bwd"}, **more))


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("fill", FWD_FILLS, ids=FILL_ID)
@pytest.mark.parametrize("v", VARIANTS, ids=lambda v: v.name)
def test_forward_is_the_same_whatever_the_buffers_held(hip_lib, v, fill):
    """Every (path variant, fill): return code 0, the allocation callbacks asked for ex4d_*_bytes of the frame, every guard intact (six
    outputs, three state buffers, the status words), no output element still holds the prefill, and num_rendered / the six outputs /
    depth_order / point_list[:R] / ranges / final_T / n_contrib / the records (and clamp bits) of visible Gaussians bit-identical to
    the zero-fill run -- which is bit-identical to the same frame through ex4dgs_amd._C (helpers.gpu_forward_raw)."""
    ref, ref_f = zero_run(v)
    what = f"{v.name} [{fill}]"
    if fill == "zero":
        f = ref_f
        g = common_path_forward(v)
        g["num_rendered"] = int(g["num_rendered"])
        snap = forward_snapshot(g)
        snap["status"] = ref["status"]             # (the common path reports the status through a PendingFrame: its count is compared above)
        assert_same_forward(snap, ref, f"{v.name}: raw driver vs ex4dgs_amd._C")
    elif fill == "stale":
        bufs = raw_abi.Buffers()
        p = run_forward(PRIMER, bufs, "zero")
        held = {n: bufs.get(n).base.data_ptr() for n in raw_abi.STATE_BUFFERS}
        f = run_forward(v, bufs, "stale")
        for n in raw_abi.STATE_BUFFERS:            # the storage really is the previous frame's unless it had to grow
            assert (bufs.get(n).base.data_ptr() == held[n]) == (f["asked"][n] <= (p["asked"][n] + 255) // 256 * 256), n
    else:
        out_fill = fill.split("-")[0]
        f = run_forward(v, raw_abi.Buffers(), out_fill, state_fill="zero" if fill.endswith("-outputs") else out_fill)
    check_forward_call(f, fill.split("-")[0], what, ref)
    assert_same_forward(forward_snapshot(f), ref, what)
    _report("buffer_contract_forward", v, fill, P=int(f["params"].P), R=int(f["num_rendered"]), W=int(f["params"].W), H=int(f["params"].H))


@pytest.mark.parametrize("scene", [CFG1, CFG3], ids=lambda s: s.name)
def test_poisoned_buffers_through_the_oracle_comparison(hip_lib_both, monkeypatch, scene):
    """cfg1 and cfg3 (P = 12000, t = 137) with every buffer prefilled with 0xFF bytes, through the whole chain of
    tests/test_gpu_parity.py::_fwd_bwd: compare_forward against the oracle, the oracle's backward on the GPU forward's state, the
    reference's noise floor, the end-to-end comparison, the per-Gaussian stage -- with the bars that chain has."""
    from ex4dgs_amd import _C
    from tests.test_gpu_parity import _fwd_bwd
    bufs = raw_abi.Buffers()
    calls = []

    def fwd(ins, st, device="cuda", subpixel_offset=None):
        f = raw_abi.forward(ins, st, bufs, fill="ones", subpixel_offset=subpixel_offset)
        assert f["rc"] == 0, f["error"]
        check_forward_call(f, "ones", scene.name)
        calls.append("forward")
        return f

    def bwd(ins, f, grads, device="cuda"):
        b = raw_abi.backward(f, grads, fill="ones")
        assert b["rc"] == 0, b["error"]
        bufs.assert_guards_intact()
        calls.append("backward")
        return b
    monkeypatch.setattr(h, "gpu_forward_raw", fwd)
    monkeypatch.setattr(h, "gpu_backward_raw", bwd)
    lean = dict(geom_debug_arrays=_C.get_option("geom_debug_arrays"), binning_tile_ids=_C.get_option("binning_tile_ids"))
    with options(lean):                            # (the fixture's choice of debug arrays, everything else at the library's defaults)
        _fwd_bwd(scene.cfg, P=scene.P, t=scene.t)
    assert calls == ["forward", "backward"]
    h.REPORT.append(dict(kind="buffer_contract_oracle", tag=f"{scene.name} [ones] through _fwd_bwd", variant=scene.name, fill="ones", options=lean))


SEQUENCES = {
    "big, small, big": [Variant("cfg3", CFG3, {}, {}), Variant("131x67", TINY, {}, {}), Variant("cfg2 P=1", CFG2_1, {}, {}), Variant("cfg3 again", CFG3, {}, {})],
    "prepare_backward 1 then 0": [Variant("cfg3 prepare_backward", CFG3, dict(prepare_backward=1), {}), Variant("cfg3", CFG3, {}, {})],
    "MSD-sorted then LSD-sorted": [Variant("cfg3 MSD", CFG3, {}, dict(depth_sort_msd=2)), Variant("cfg3 LSD", CFG3, {}, dict(depth_sort_msd=0)),
                                   Variant("cfg2 P=2049 MSD, scan kernel", CFG2_2049, {}, dict(depth_sort_msd=1, tile_sort_rows=0)),
                                   Variant("cfg2 P=2049 LSD", CFG2_2049, {}, dict(depth_sort_msd=0, tile_sort_rows=0))],
    "defaults then tile_sort_rows=0": [Variant("cfg3", CFG3, {}, {}), Variant("cfg3 pair sort", CFG3, {}, dict(tile_sort_rows=0)),
                                       Variant("cfg3 async", CFG3, dict(ASYNC), {}), Variant("cfg3 again", CFG3, {}, {})],
}


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_stale_sequences(hip_lib, name):
    """Frames of different sizes, options and Ex4dParams one after the other in ONE set of buffers, nothing cleared in between
    (FrameTrainer's arenas, a replayed graph): every frame equals the same frame on fresh zero-filled buffers."""
    bufs = raw_abi.Buffers()
    for i, v in enumerate(SEQUENCES[name]):
        ref = forward_snapshot(run_forward(v, raw_abi.Buffers(), "zero"))
        ptrs = {n: g.base.data_ptr() for n, g in bufs.by_name.items()}
        caps = {n: g.capacity for n, g in bufs.by_name.items()}
        f = run_forward(v, bufs, "stale")
        for n in ptrs:
            if n in bufs.touched and bufs.get(n).nbytes <= caps[n]:
                assert bufs.get(n).base.data_ptr() == ptrs[n], f"{n}: not the storage of the previous frame"
        check_forward_call(f, "stale", f"{name} / frame {i}: {v.name}")
        assert_same_forward(forward_snapshot(f), ref, f"{name} / frame {i}: {v.name}")
        _report("buffer_contract_sequence", v, "stale", sequence=name, frame=i)


# ------------------------------------------------------------------------------------------------ backward
ROW_BAR = 1e-4       # of the row's max, floored at 1: what two runs of one backward are held to (test_backward_reproducible_to_rounding)
BWD_COMPARED = raw_abi.GRAD_NAMES + ("acc16",)


def _upstream(f, seed=4):
    H, W = f["params"].H, f["params"].W
    return [x.cuda() for x in h.upstream_grads(f["acc"].cpu(), H, W, seed=seed, grad_acc_zero=False)]


def assert_rows_close(a, b, what, names=BWD_COMPARED):
    for k in names:
        x, y = a[k], b[k]
        assert x.shape == y.shape, (what, k, x.shape, y.shape)
        if x.numel() == 0:
            continue
        x2, y2 = x.reshape(x.shape[0], -1), y.reshape(y.shape[0], -1)
        scale = y2.abs().amax(dim=1, keepdim=True).clamp_min(1.0)
        err = float(((x2 - y2).abs() / scale).nan_to_num(nan=float("inf")).max())
        assert err < ROW_BAR, f"{what}: {k} differs by {err:.3e} of the row's max (bar {ROW_BAR})"


def check_backward_call(f, b, fill, state_before, what, ref=None):
    """Guards of every output and of the scratch, state buffers untouched, invisible rows exactly zero, nothing left unwritten."""
    assert b["rc"] == 0, b["error"]
    touched = set(b["bufs"].touched)
    assert "scratch" in touched and touched >= set(b["written"])
    b["bufs"].assert_guards_intact()
    b["bufs"].assert_guards_intact(raw_abi.STATE_BUFFERS)
    for n in raw_abi.STATE_BUFFERS:
        assert torch.equal(b["bufs"].get(n).payload, state_before[n]), f"{what}: the backward changed the {n} buffer"
    invisible = f["radii"] <= 0
    for k, t in b["written"].items():
        # (ref: gradients of the zero-fill run -- a computed value may have the bits of the `finite` pattern; raw_abi.leftover_fill)
        left = raw_abi.leftover_fill(t, fill, ref[k] if (ref is not None and k in ref) else None)
        assert left == 0, f"{what}: {left} elements of {k} still hold the prefill"
    for k in raw_abi.GRAD_NAMES:
        t = b[k]
        if t.numel():
            assert int((_bits(t.reshape(t.shape[0], -1)[invisible]) != 0).sum()) == 0, f"{what}: {k} is not exactly zero on rows with radii == 0"


@functools.lru_cache(maxsize=2)
def _oracle_forward(name):
    v = next(x for x in VARIANTS if x.name == name)
    ins, st, sub, kw = frame_inputs(v)
    return h.oracle_forward(ins, st, subpixel_offset=sub)


def run_backward(v, bufs, fill, prepared=None, **kw):
    f = run_forward(v, bufs, fill)
    state_before = {n: bufs.get(n).payload.clone() for n in raw_abi.STATE_BUFFERS}
    with options(v.options):
        b = raw_abi.backward(f, _upstream(f), fill=fill, prepared=bool(v.extras.get("prepare_backward")) if prepared is None else prepared, **kw)
    return f, b, state_before


_ZERO_BWD = {}


def zero_backward(v):
    if v.name not in _ZERO_BWD:
        _ZERO_BWD.clear()
        f, b, _ = run_backward(v, raw_abi.Buffers(), "zero")
        assert b["rc"] == 0, b["error"]
        _ZERO_BWD[v.name] = {k: b[k].clone() for k in BWD_COMPARED + tuple(n for n in raw_abi.SPLIT_GRAD_NAMES if n in b)}
    return _ZERO_BWD[v.name]


@pytest.mark.parametrize("fill", BWD_FILLS, ids=FILL_ID)
@pytest.mark.parametrize("v", BWD_VARIANTS, ids=lambda v: v.name)
def test_backward_is_the_same_whatever_the_buffers_held(hip_lib, v, fill):
    """The backward on the state a forward on equally poisoned buffers left, its outputs and scratch prefilled: guards intact, the
    state buffers bit-unchanged, rows with radii == 0 exactly zero, no element left unwritten, the per-Gaussian stage bit-exact
    against oracle.preprocess_backward on the GPU's own accumulators, accumulators and gradients within the run-to-run bar of the
    zero-fill run (split SH: the four gradient parts, put together)."""
    ref = zero_backward(v)
    what = f"{v.name} [{fill}]"
    bufs = raw_abi.Buffers()
    if fill == "stale":
        pf, pb, _ = run_backward(PRIMER, bufs, "zero")
        assert pb["rc"] == 0, pb["error"]
    f, b, state_before = run_backward(v, bufs, fill)
    check_backward_call(f, b, fill, state_before, what, ref)
    assert_rows_close(b, ref, what)
    o = _oracle_forward(v.name)
    assert np.array_equal(o["radii"], h.to_np(f["radii"]))
    h.assert_per_gaussian_stage_bit_exact(o, b)
    _report("buffer_contract_backward", v, fill, P=int(f["params"].P), R=int(f["num_rendered"]))


@pytest.mark.parametrize("fill", BWD_FILLS, ids=FILL_ID)
def test_null_outputs_and_null_upstream_gradients(hip_lib, fill):
    """dL_dcolors / dL_dcov3D passed as NULL change nothing else; each upstream gradient passed as NULL equals a zero tensor."""
    v = next(x for x in VARIANTS if x.name == "cfg3 defaults")
    bufs = raw_abi.Buffers()
    if fill == "stale":
        run_backward(PRIMER, bufs, "zero")
    f = run_forward(v, bufs, fill)
    grads = _upstream(f)
    state_before = {n: bufs.get(n).payload.clone() for n in raw_abi.STATE_BUFFERS}
    with options(v.options):
        base = raw_abi.backward(f, grads, fill=fill)
        check_backward_call(f, base, fill, state_before, "all outputs", zero_backward(v))
        base = {k: base[k].clone() for k in BWD_COMPARED}
        for null in (("dL_dcolors",), ("dL_dcov3D",), ("dL_dcolors", "dL_dcov3D")):
            b = raw_abi.backward(f, grads, fill=fill, null_outputs=null)
            check_backward_call(f, b, fill, state_before, f"NULL {null}", base)
            assert all(b[n].numel() == 0 and n not in b["written"] for n in null)
            assert_rows_close(b, base, f"NULL {null} [{fill}]", names=[k for k in BWD_COMPARED if k not in null])
        for i, name in enumerate(("dL_dout_color", "dL_dout_depth", "dL_dout_flow", "dL_dout_acc")):
            zeroed = [torch.zeros_like(g) if j == i else g for j, g in enumerate(grads)]
            want = raw_abi.backward(f, zeroed, fill="zero", bufs=_scratch_outputs(bufs))
            got = raw_abi.backward(f, grads, fill=fill, null_grads=(i,))
            check_backward_call(f, got, fill, state_before, f"NULL {name}", want)
            assert_rows_close(got, want, f"NULL {name} [{fill}] vs a zero tensor")
    h.REPORT.append(dict(kind="buffer_contract_null", tag=f"cfg3 NULL outputs / upstream gradients [{fill}]", variant=v.name, fill=fill))


def _scratch_outputs(bufs):
    """A second set of gradient / scratch buffers that shares the forward's state buffers (the reference run of a comparison)."""
    other = raw_abi.Buffers()
    for n in raw_abi.STATE_BUFFERS:
        other.by_name[n] = bufs.get(n)
    return other


@pytest.mark.parametrize("fill", BWD_FILLS, ids=FILL_ID)
@pytest.mark.parametrize("name", ["cfg3 defaults", "cfg3 split SH", "cfg1 test options"])
def test_prepare_backward_mismatch_gives_nan_means3d_and_nothing_else(hip_lib, name, fill):
    """include/ex4d_rasterizer.h, Ex4dParams.prepare_backward: a backward that asks for the forward's SH direction sums on buffers
    whose forward ran with prepare_backward = 0 returns dL_dmeans3D = NaN on every visible Gaussian (the one gradient the sums
    enter) and every other output as the plain backward does -- whatever the buffers held, the sums and the mark of an earlier
    frame with prepare_backward = 1 in the same storage included (`stale`)."""
    v = next(x for x in VARIANTS if x.name == name)
    bufs = raw_abi.Buffers()
    if fill == "stale":
        with_sums = Variant(v.name + ", prepare_backward", v.scene, dict(v.extras, prepare_backward=1), v.options)
        f1, b1, _ = run_backward(with_sums, bufs, "zero")
        assert b1["rc"] == 0 and bool(torch.isfinite(b1["dL_dmeans3D"]).all())          # that frame's sums are there and marked
    f = run_forward(v, bufs, fill)                                                       # prepare_backward = 0
    grads = _upstream(f)
    state_before = {n: bufs.get(n).payload.clone() for n in raw_abi.STATE_BUFFERS}
    with options(v.options):
        plain = raw_abi.backward(f, grads, fill="zero", bufs=_scratch_outputs(bufs), prepared=False)
        assert plain["rc"] == 0, plain["error"]
        plain = {k: plain[k].clone() for k in BWD_COMPARED}
        b = raw_abi.backward(f, grads, fill=fill, prepared=True)
    check_backward_call(f, b, fill, state_before, f"{name} [{fill}]", plain)
    visible = f["radii"] > 0
    assert int(visible.sum()) > 0
    assert bool(torch.isnan(b["dL_dmeans3D"][visible]).all()), "dL_dmeans3D of a visible Gaussian is a number: computed from sums this frame did not store"
    assert not bool(torch.isnan(b["dL_dmeans3D"][~visible]).any())
    others = [k for k in BWD_COMPARED if k != "dL_dmeans3D"]
    for k in others:
        assert not bool(torch.isnan(b[k]).any()), k
    assert_rows_close(b, plain, f"{name} [{fill}]", names=others)
    _report("buffer_contract_mismatch", v, fill)
