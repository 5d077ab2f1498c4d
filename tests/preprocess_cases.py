"""Frames the view frustum cuts through, and a host census of the paths the per-Gaussian kernels take on them; shared by
tests/test_cpu_preprocess_cases.py (every frame realises its plan on the CPU oracle, and the table reaches every path with every lane
pattern) and tests/test_gpu_preprocess_paths.py (the kernels of ex4dgs_amd/csrc/ex4d_preprocess.hip against the oracle on these frames).

A frame is a small synthetic scene (160 x 96 pixels, 1 .. 1400 Gaussians) in which EVERY row of means3D is re-placed: a plan gives each
row one of the classes below, positions are formed in view space in float64, taken back to world space through the inverse of the
camera's viewmatrix and rounded to float32.

    VIS          inside the image (|ndc| <= 0.9), between the depth planes: passes the frustum test and is rendered
    NEAR         view depth min_depth / 2                               culled: p_view.z <= min_depth
    BACK         behind the camera (view depth -2)                       culled: p_view.z <= min_depth
    FAR          view depth 1.5 max_depth                                culled: p_view.z > max_depth
    XPOS / XNEG  ndc x = +-1.45                                          culled: |ndc x| > 1.3
    YPOS / YNEG  ndc y = +-1.45                                          culled: |ndc y| > 1.3
    EDGE_*       ndc x or y in +-[1.12, 1.2], footprint of half a pixel: PASSES the frustum test, its tile rect is empty (radii = 0)
    NAN          one coordinate NaN: every comparison of the frustum test is false, so it PASSES; its pixel position is NaN, which the
                 float -> int conversion maps to 0: an empty tile rect (radii = 0)

So the forward's `need` bit of a row (it passed the frustum test: its SH row is requested) is set for VIS, EDGE_* and NAN, the
backward's `radii > 0` bit for VIS alone.  Which rows of a wave of 64 are which is laid out by a lane pattern per wave (PATTERNS),
rotated through the waves of a frame.

census() restates, from the conditions the kernels branch on (not from their code), which path each wave of a frame takes:

    forward     plain12       one [P,16,3] tensor, degree 3, a full wave whose 64 rows are all needed: twelve plain 16-byte loads
                predicated    one [P,16,3] tensor otherwise: each 16-byte chunk requested if its row is needed, inside the frame
                              and below the degree's length
                split_staged  four tensors (dc / rest, static / dynamic): a full wave inside one part whose spans start on 16 bytes
                split_rows    four tensors otherwise (the wave that straddles n_static, a partial wave, misaligned spans): row by row
                unstaged      [P,M,3] with M != 16
                no_sh         precomputed colours
    bwd read    dsums         the forward left the direction sums (prepare_backward): no SH row is read
                staged        one [P,16,3] tensor, through LDS
                split_staged  four tensors, stageable wave (the forward's condition on the INPUT tensors)
                split_rows    four tensors otherwise: each lane reads its row straight from memory
                unstaged      M != 16: likewise
                no_sh
    bwd store   staged        one [P,16,3] gradient; four gradient parts on a stageable wave whose gradient spans start on 16 bytes
                rows          four gradient parts otherwise
                m_not_16      [P,M,3] with M != 16, one element at a time
                no_sh
"""
import functools
from typing import NamedTuple, Optional

import numpy as np
import torch

from ex4dgs_amd.scene import SceneConfig
from tests import helpers as h

WAVE, GROUP = 64, 256                 # rows per wave, per workgroup
W, H, FOCAL = 160, 96, 90.0
MIN_DEPTH, MAX_DEPTH = 0.5, 60.0
CFG = SceneConfig("preprocess frame", 1400, W, H, FOCAL, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, z_lo=1.0, z_hi=30.0,
                  sigma_px_med=2.5, sigma_px_logstd=0.6, seed=21)

# ------------------------------------------------------------------ row classes
VIS, NEAR, BACK, FAR, XPOS, XNEG, YPOS, YNEG, EDGE_XPOS, EDGE_XNEG, EDGE_YPOS, EDGE_YNEG, NAN = range(13)
CLASS_NAMES = ("VIS", "NEAR", "BACK", "FAR", "XPOS", "XNEG", "YPOS", "YNEG", "EDGE_XPOS", "EDGE_XNEG", "EDGE_YPOS", "EDGE_YNEG", "NAN")
CULLED = (NEAR, BACK, FAR, XPOS, XNEG, YPOS, YNEG)                   # fail the frustum test
INVISIBLE = (EDGE_XPOS, EDGE_XNEG, EDGE_YPOS, EDGE_YNEG, NAN)        # pass it, radii = 0

# ------------------------------------------------------------------ lane patterns of a wave: which of its 64 rows are needed
_LANES = np.arange(WAVE)
ISO_VISIBLE = (2, 17, 31, 33, 46, 61)         # needed rows between two culled ones; none a multiple of 4: in the split layout the first
                                              # 16-byte chunk of each is shared with the culled row in front of it
ISO_CULLED = (1, 16, 31, 33, 47, 62)          # culled rows between two needed ones (their chunks are shared with both neighbours)
ISO_CULLED_EDGES = (0, 32, 63)                # ... at the first lane, the first lane of the upper half, the last lane


def _random_half(seed):
    return np.random.default_rng(seed).permutation(WAVE) < WAVE // 2


PATTERN_MASKS = {
    "all": np.ones(WAVE, bool), "none": np.zeros(WAVE, bool), "lower": _LANES < 32, "upper": _LANES >= 32,
    "one0": _LANES == 0, "one31": _LANES == 31, "one32": _LANES == 32, "one63": _LANES == 63,
    "even": _LANES % 2 == 0, "odd": _LANES % 2 == 1, "third": _LANES % 3 == 0,
    "iso_visible": np.isin(_LANES, ISO_VISIBLE), "iso_culled": ~np.isin(_LANES, ISO_CULLED), "iso_culled_edges": ~np.isin(_LANES, ISO_CULLED_EDGES),
    "random": None,                           # a seeded random half, different in every wave
}
PATTERNS = tuple(PATTERN_MASKS)


def pattern_mask(name, seed):
    return _random_half(seed) if name == "random" else PATTERN_MASKS[name]


# what a mask (the first nrows lanes of a wave) is, by its own properties -- the classes of the census's cell table.  A mask belongs
# to every class whose property it has.
PATTERN_CLASSES = ("full", "empty", "lower_only", "upper_only", "single_0", "single_31", "single_32", "single_63", "alternating",
                   "every_third", "iso_visible_lower", "iso_visible_upper", "iso_culled_lower", "iso_culled_upper", "mixed_halves")


def pattern_classes(mask, nrows):
    m = np.zeros(WAVE, bool)
    m[:nrows] = np.asarray(mask, bool)[:nrows]
    inside = _LANES < nrows
    out = set()
    n = int(m.sum())
    if n == nrows:
        out.add("full")
    if n == 0:
        out.add("empty")
    if nrows > 32 and m[:32].all() and not m[32:].any():
        out.add("lower_only")
    if nrows > 32 and not m[:32].any() and m[32:nrows].all():
        out.add("upper_only")
    if n == 1:
        lane = int(np.flatnonzero(m)[0])
        if lane in (0, 31, 32, 63) and nrows > 1:
            out.add(f"single_{lane}")
    if nrows >= 4 and (np.array_equal(m, inside & (_LANES % 2 == 0)) or np.array_equal(m, inside & (_LANES % 2 == 1))):
        out.add("alternating")
    if nrows >= 4 and np.array_equal(m, inside & (_LANES % 3 == 0)):
        out.add("every_third")
    # isolated rows: both neighbours inside the wave and of the other kind
    left, right = np.roll(m, 1), np.roll(m, -1)
    interior = (_LANES >= 1) & (_LANES + 1 < nrows)
    iso_v, iso_c = interior & m & ~left & ~right, interior & ~m & left & right
    if 0 < n < nrows and not out & {"alternating"}:
        for name, iso in (("iso_visible", iso_v), ("iso_culled", iso_c)):
            if iso[:32].any():
                out.add(name + "_lower")
            if iso[32:].any():
                out.add(name + "_upper")
    if nrows > 32 and 0 < int(m[:32].sum()) < 32 and 0 < int(m[32:nrows].sum()) < nrows - 32:
        out.add("mixed_halves")
    return out


# ------------------------------------------------------------------ the case table
class Case(NamedTuple):
    name: str
    P: int
    layout: str = "cat"                       # "cat": shs [P,M,3]; "split": four tensors; "colors": colors_precomp
    D: int = 3
    M: int = 16
    n_static: Optional[int] = None            # split layout
    rotate: int = 0                           # waves 2 j and 2 j + 1 get patterns[(j + rotate) % len(patterns)] (pairs = False: wave w gets patterns[w % len])
    pairs: bool = True                        # ... the even wave with every needed row rendered, the odd one with invisible rows among them
    patterns: tuple = PATTERNS
    invisible_every: int = 5                  # every n-th needed row (of the odd waves; pairs = False: of all waves) is EDGE_* / NAN instead of VIS (0: none)
    cov_precomp: bool = False                 # cov3D_precomp (the oracle's own cov3D of the frame) instead of scale + rotation
    flow: str = "all"                         # dir3D: "all" rows, "unrendered" = only rows with radii = 0, "last_wave" = one VIS row of the last wave
    special: Optional[str] = None             # "min_depth" / "max_depth": a plane set onto a Gaussian's own depth; "cull_row0" / "cull_last_row"
    in_offset: int = 0                        # split layout: the four input tensors start this many floats into their allocations
    grad_offset: int = 0                      # ... and the four gradient tensors
    refused: Optional[str] = None             # the library refuses the frame with this message (argument check): no kernel runs
    seed: int = 0


def _split(name, P, n_static, **kw):
    return Case(name, P, layout="split", n_static=n_static, **kw)


CASES = (
    # one [P,16,3] tensor: 5 workgroups and a tail of 2 chunks (56 rows in the last); every degree (nvec = 12, 7, 3, 1)
    Case("cat d3 P1400", 1400),
    Case("cat d2 P1400", 1400, D=2, rotate=3),
    Case("cat d1 P1343", 1343, D=1, rotate=11),            # last workgroup: 1 chunk of 63 rows
    Case("cat d0 P1400", 1400, D=0, rotate=7),
    Case("cat d3 P1280 full last workgroup", 1280, rotate=8),
    # the last workgroup holds 1, 2, 3, 4 chunks; the last wave 1, 31, 32, 33, 63 rows
    Case("cat d3 P1", 1, patterns=("all",), invisible_every=0),
    Case("cat d3 P64", 64, patterns=("iso_culled",), pairs=False),
    Case("cat d3 P95 (2 chunks, 31 rows)", 95, patterns=("even", "iso_culled"), pairs=False),
    Case("cat d3 P160 (3 chunks, 32 rows)", 160, patterns=("upper", "iso_visible", "all"), pairs=False),
    Case("cat d3 P225 (4 chunks, 33 rows)", 225, patterns=("lower", "third", "one63", "iso_culled_edges"), pairs=False),
    Case("cat d3 P447 (3 chunks, 63 rows)", 447, rotate=8),
    Case("cat d3 P129 (1 row)", 129, patterns=("random", "odd", "all"), invisible_every=0, pairs=False),
    Case("cat d3 P200 all culled", 200, patterns=("none",)),
    # M != 16
    Case("M4 d1 P1400", 1400, D=1, M=4, rotate=0),
    Case("M9 d2 P1343", 1343, D=2, M=9, rotate=8),
    Case("M4 d3 P95 (fewer coefficients than the degree needs)", 95, D=3, M=4, refused="fewer coefficients than the active degree needs"),
    # no SH, precomputed covariance
    Case("colors_precomp P1400", 1400, layout="colors", M=0, rotate=0),
    Case("colors_precomp P1343", 1343, layout="colors", M=0, rotate=8),
    Case("cov3D_precomp P1400", 1400, cov_precomp=True, rotate=6),
    # four tensors: n_static in {0, P, 64k, 64k+4, 64k+1, 64k+32}
    _split("split n_static 0 P1400", 1400, 0, rotate=1),
    _split("split n_static P P1343", 1343, 1343, rotate=10),
    _split("split n_static 640 P1400", 1400, 640, rotate=13),
    _split("split n_static 644 P1400", 1400, 644, rotate=2),       # boundary wave row by row, later waves staged from row 60 + 64 j
    _split("split n_static 68 P1400", 1400, 68, rotate=9),
    _split("split n_static 641 P1400", 1400, 641, rotate=4),       # every dynamic wave misaligned: row by row
    _split("split n_static 65 P1343", 1343, 65, rotate=0),
    _split("split n_static 1 P1400 d2", 1400, 1, D=2, rotate=8),
    _split("split n_static 672 P1400", 1400, 672, rotate=7),
    _split("split n_static 32 P225 d1", 225, 32, D=1, patterns=("iso_visible", "iso_culled", "random", "lower"), pairs=False),
    _split("split n_static 64 P129 d0", 129, 64, D=0, patterns=("odd", "iso_visible", "all"), pairs=False),
    # staged reads with row-by-row stores, and the reverse: gradient parts / input parts 4 bytes into their allocations
    _split("split n_static 640 P1400, gradient parts misaligned", 1400, 640, rotate=3, grad_offset=1),
    _split("split n_static 640 P1400, input parts misaligned", 1400, 640, rotate=11, in_offset=1),
    # flow
    Case("flow only on unrendered rows", 447, rotate=1, flow="unrendered"),
    Case("flow on one row of the partial last wave", 225, patterns=("lower", "third", "even", "iso_visible"), pairs=False, flow="last_wave"),
    # the depth planes met exactly
    Case("min_depth on a Gaussian's depth", 447, patterns=("all",), invisible_every=0, special="min_depth"),
    Case("max_depth on a Gaussian's depth", 447, patterns=("all",), invisible_every=0, special="max_depth"),
    # one culled Gaussian: lane 0 of wave 0 / the last row of a partial last wave (prefiltered = True must be refused on them)
    Case("one culled row: lane 0 of wave 0", 225, patterns=("all",), invisible_every=0, special="cull_row0"),
    Case("one culled row: the last of a partial last wave", 225, patterns=("all",), invisible_every=0, special="cull_last_row"),
)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
RUNNABLE = tuple(c for c in CASES if c.refused is None)
PREFILTER_CASES = ("one culled row: lane 0 of wave 0", "one culled row: the last of a partial last wave")
THRESHOLD_CASES = ("min_depth on a Gaussian's depth", "max_depth on a Gaussian's depth")


# ------------------------------------------------------------------ the plan of a case
def plan_classes(case):
    """Class of every row, from the lane patterns alone."""
    P = case.P
    cls = np.zeros(P, np.int64)
    n_need = n_cull = 0
    for w in range((P + WAVE - 1) // WAVE):
        name = case.patterns[((w // 2 + case.rotate) if case.pairs else w) % len(case.patterns)]
        swap = case.invisible_every and (w % 2 == 1 or not case.pairs)
        mask = pattern_mask(name, 1000 * case.seed + 7 * len(case.name) + w)
        for lane in range(min(WAVE, P - w * WAVE)):
            i = w * WAVE + lane
            if mask[lane]:
                n_need += 1
                cls[i] = INVISIBLE[(n_need // case.invisible_every) % len(INVISIBLE)] if (swap and n_need % case.invisible_every == 0) else VIS
            else:
                cls[i] = CULLED[n_cull % len(CULLED)]
                n_cull += 1
    if case.special == "cull_row0":
        cls[0] = FAR
    if case.special == "cull_last_row":
        cls[P - 1] = XNEG
    return cls


def _view_positions(cls, z_scene, tanx, tany, rng, min_depth, max_depth):
    """View-space positions [P,3] (float64) of the classes; z_scene: the scene's own depths, kept by every row that stays in range."""
    P = cls.shape[0]
    u, v = rng.uniform(-0.9, 0.9, P), rng.uniform(-0.9, 0.9, P)
    z = np.asarray(z_scene, np.float64).copy()
    edge = rng.uniform(1.12, 1.2, P)
    z[cls == NEAR] = 0.5 * min_depth
    z[cls == BACK] = -2.0
    z[cls == FAR] = 1.5 * max_depth
    u[cls == XPOS], u[cls == XNEG] = 1.45, -1.45
    v[cls == YPOS], v[cls == YNEG] = 1.45, -1.45
    u = np.where(cls == EDGE_XPOS, edge, np.where(cls == EDGE_XNEG, -edge, u))
    v = np.where(cls == EDGE_YPOS, edge, np.where(cls == EDGE_YNEG, -edge, v))
    return np.stack([u * z * tanx, v * z * tany, z], -1)


class Frame(NamedTuple):
    case: Case
    ins: dict
    settings: dict
    cls: np.ndarray            # class per row
    frustum: np.ndarray        # planned verdict of the frustum test per row (the forward's need bit)
    visible: np.ndarray        # planned radii > 0 per row
    marked: Optional[int]      # the row whose depth a plane was set to (threshold cases)


@functools.lru_cache(maxsize=None)
def frame(name):
    case = BY_NAME[name]
    P = case.P
    ins, st = h.scene_inputs(CFG, P=P, sh_degree=case.D, dir_scale=0.1, seed=31 + case.seed)
    cls = plan_classes(case)
    rng = np.random.default_rng(500 + 13 * len(case.name) + case.seed)
    vm = st["viewmatrix"].double().numpy()                     # row-vector convention: p_view = [p, 1] @ vm
    z_scene = (np.concatenate([ins["means3D"].double().numpy(), np.ones((P, 1))], 1) @ vm)[:, 2]
    pv = _view_positions(cls, z_scene, st["tanfovx"], st["tanfovy"], rng, MIN_DEPTH, MAX_DEPTH)
    world = (np.concatenate([pv, np.ones((P, 1))], 1) @ np.linalg.inv(vm))[:, :3]
    # (the camera's position is the translation of inv(vm))
    assert np.allclose(np.linalg.inv(vm)[3, :3], st["campos"].double().numpy(), atol=1e-6)
    means = world.astype(np.float32)
    nan_rows = np.flatnonzero(cls == NAN)
    means[nan_rows, nan_rows % 3] = np.nan
    ins["means3D"] = torch.from_numpy(means).contiguous()
    # rows whose tile rect must be empty: a footprint of half a pixel at their depth
    small = np.isin(cls, INVISIBLE)
    sc = ins["scales"].clone()
    sc[torch.from_numpy(small)] = torch.from_numpy((np.abs(pv[small, 2:3]) * 0.4 / FOCAL).astype(np.float32)).expand(-1, 3)
    ins["scales"] = sc.contiguous()
    frustum, visible = ~np.isin(cls, CULLED), cls == VIS
    marked = None
    if case.M not in (0, 16):
        ins["shs"] = ins["shs"][:, :case.M].contiguous()
    if case.layout == "colors":
        ins["colors_precomp"] = torch.rand(P, 3, generator=torch.Generator().manual_seed(77 + case.seed))
        ins["shs"] = None
    if case.special in ("min_depth", "max_depth") or case.cov_precomp:
        base = h.oracle_forward(ins, st)                     # the frame with its planes where the scene has them
        if case.cov_precomp:
            ins["cov3D_precomp"] = torch.from_numpy(base["cov3D"].copy())
            ins["scales"] = ins["rotations"] = None
        else:
            assert (base["radii"] > 0).all(), "the threshold frames start from a frame in which every Gaussian is rendered"
            d = base["depths"]                               # float32, what the frustum test compares with the planes
            order = np.argsort(d, kind="stable")
            if case.special == "min_depth":
                marked = int(order[P // 3])
                st["min_depth"] = float(d[marked])
                frustum = d > d[marked]                      # the marked Gaussian itself is culled: p_view.z <= min_depth
            else:
                marked = int(order[2 * P // 3])
                st["max_depth"] = float(d[marked])
                frustum = ~(d > d[marked])                   # ... is kept: p_view.z > max_depth fails
            visible = frustum.copy()
    dir3D = ins["dir3D"].clone()
    if case.flow == "unrendered":
        dir3D[torch.from_numpy(visible)] = 0.0
    elif case.flow == "last_wave":
        last = np.flatnonzero(visible & (np.arange(P) >= (P - 1) // WAVE * WAVE))
        assert last.size and P % WAVE, "no rendered row in a partial last wave"
        keep = dir3D[last[-1]].clone()
        dir3D.zero_()
        dir3D[last[-1]] = keep
    ins["dir3D"] = dir3D.contiguous()
    return Frame(case, ins, st, cls, frustum, visible, marked)


@functools.lru_cache(maxsize=None)
def oracle_forward(name):
    """The oracle's forward of a case (left unchanged by everybody)."""
    f = frame(name)
    return h.oracle_forward(f.ins, f.settings)


def flow_carriers(f):
    """Rows whose dir3D is not zero."""
    return (f.ins["dir3D"] != 0).any(1).numpy()


# ------------------------------------------------------------------ census
def nvec_of(D):
    """16-byte chunks of a [16,3] row that hold the coefficients of degree D: 1, 3, 7 (one float past the 27), 12."""
    return ((D + 1) * (D + 1) * 3 + 3) // 4


def split_stageable(first, nrows, n_static, offset):
    """A wave of the split layout goes through LDS when it is full, lies inside one part, and its rest / dc spans start on 16 bytes:
    the spans start r0 * 45 and r0 * 3 floats into tensors that themselves start `offset` floats behind a 16-byte boundary."""
    if nrows != WAVE:
        return False
    if first >= n_static:
        r0 = first - n_static
    elif first + nrows <= n_static:
        r0 = first
    else:
        return False
    return (4 * (r0 * 45 + offset)) % 16 == 0 and (4 * (r0 * 3 + offset)) % 16 == 0


def census(case, frustum, visible, sh_predicate=1, prepare_backward=0):
    """Per wave of the frame: rows, the forward's need mask and the backward's radii > 0 mask (bool [waves, 64]), the three paths,
    the pattern classes of both masks, and -- what the split layout's shared chunks turn on -- whether a needed row follows a
    culled one, a culled row follows a needed one, and whether lanes 31 and 32 differ."""
    P = case.P
    nw = (P + WAVE - 1) // WAVE
    pad = lambda m: np.concatenate([np.asarray(m, bool), np.zeros(nw * WAVE - P, bool)]).reshape(nw, WAVE)
    in_range = pad(np.ones(P, bool))
    need = pad(frustum) if sh_predicate else in_range.copy()
    live = pad(visible)
    rows = in_range.sum(1)
    out = dict(rows=rows, need=need, live=live, fwd=[], bwd_read=[], bwd_store=[], need_classes=[], live_classes=[], shared=[])
    for w in range(nw):
        first, n = w * WAVE, int(rows[w])
        # the forward's request is all ones when the predicate is off -- also on the lanes past the end of the frame
        all_needed = bool(need[w, :n].all()) if sh_predicate else True
        if case.layout == "colors":
            fwd = read = store = "no_sh"
        elif case.M != 16:
            fwd, read, store = "unstaged", "unstaged", "m_not_16"
        elif case.layout == "split":
            stage_in = split_stageable(first, n, case.n_static, case.in_offset)
            fwd = "split_staged" if stage_in else "split_rows"
            read = "split_staged" if stage_in else "split_rows"
            store = "staged" if (stage_in and split_stageable(first, n, case.n_static, case.grad_offset)) else "rows"
        else:
            fwd = "plain12" if (n == WAVE and nvec_of(case.D) == 12 and all_needed) else "predicated"
            read, store = "staged", "staged"
        if prepare_backward and case.layout != "colors":
            read = "dsums"
        out["fwd"].append(fwd); out["bwd_read"].append(read); out["bwd_store"].append(store)
        out["need_classes"].append(pattern_classes(need[w], n))
        out["live_classes"].append(pattern_classes(live[w], n))
        sh = {}
        for key, m in (("need", need[w, :n]), ("live", live[w, :n])):
            sh[key] = dict(visible_after_culled=bool((~m[:-1] & m[1:]).any()), culled_after_visible=bool((m[:-1] & ~m[1:]).any()),
                           halves_differ_at_31_32=bool(n > 32 and m[31] != m[32]))
        out["shared"].append(sh)
    # the wave of the last workgroup that publishes the depth-key range is the one whose ticket is min(chunks of that workgroup, 4) - 1
    out["last_workgroup_chunks"] = nw - (nw - 1) // 4 * 4
    out["last_wave_rows"] = int(rows[-1])
    return out


FWD_PATHS = ("plain12", "predicated", "split_staged", "split_rows", "unstaged", "no_sh")
BWD_READ_PATHS = ("dsums", "staged", "split_staged", "split_rows", "unstaged", "no_sh")
BWD_STORE_PATHS = ("staged", "rows", "m_not_16", "no_sh")
# the cells that must be reached: every pattern class on every path, but plain12, which by its condition only meets full masks
FWD_CELLS = {p: (("full",) if p == "plain12" else PATTERN_CLASSES) for p in FWD_PATHS}
BWD_READ_CELLS = {p: PATTERN_CLASSES for p in BWD_READ_PATHS}
BWD_STORE_CELLS = {p: PATTERN_CLASSES for p in BWD_STORE_PATHS}
