"""Constructed models for adaptive density control whose row classes are known by construction, shared by
tests/test_cpu_densify_cases.py (the cases mean what they say: the restatement tests/densify_ref.py agrees with the expectations
written down here, and in float32 sits within half of every bar against itself in float64) and tests/test_gpu_densify_edges.py
(the HIP kernels of ex4dgs_amd/csrc/ex4d_densify.hip against those expectations and against the float64 restatement).

The numbers restate the layout of ex4d_densify.hip: plan_classify_kernel / plan_map_kernel / densify_stats_kernel work in
workgroups of BLOCK = 256 rows with seven per-block counters packed into 9-bit fields of one 64-bit word (256 is the one value that
needs the ninth bit), and plan_scan_kernel is ONE workgroup whose 256 threads each scan per = ceil(blocks / 256) consecutive
blocks.  The row classes are chosen so that every counter saturates a whole block in some case, and the row counts so that the
scan runs with 1, 2 and 3 blocks per thread, with idle threads and with a partial last block.

A class fixes (gradient, largest scale, opacity logit) of a row.  Every scale is at least a factor 1.3 away from the threshold it
is compared with (the children of `quad`, 0.15 / 1.6 against 0.1: a factor 1.067), the opacities are far from min_opacity, and the
gradients are 0, 5 x the threshold, or exactly at / one float32 below it: no decision can flip on a 1-2 ulp difference of expf.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

from tests import densify_ref as R

BLOCK = 256
SCAN_THREADS = 256
K = 35                                                 # keyframes of duration 300, interval 10, time_pad 2
MODEL = {"interval": 10, "time_shift": 12, "duration": 300}
KEEP, CLONE, KEEP_CLONE, SPLIT, SPLIT_CLONE, KEEP_CHILD, KEEP_CHILD_CLONE = (1 << k for k in range(7))
COUNTERS = ("KEEP", "CLONE_SEL", "KEEP_CLONE", "SPLIT_SEL", "SPLIT_SEL_CLONE", "KEEP_CHILD", "KEEP_CHILD_CLONE")
ROWS = 7                                               # EX4D_CNT_ROWS
TRANSFORMED = ("_xyz", "_scaling", "_xyz_motion", "_scaling_motion", "_opacity_duration_center")
GRAD_THR = 2e-4

_COMMON = dict(max_grad=GRAD_THR, max_dgrad=GRAD_THR, min_opacity=0.01, min_motion_opacity=0.01, extent=1.0, s_max_ssim=0.5, s_l1_thres=0.1,
               d_max_ssim=0.5, d_l1_thres=0.1)
CONFIGS = {"A": dict(_COMMON, max_screen_size=None, max_dynamic_screen_size=None, percent_dense=0.01),
           "B": dict(_COMMON, max_screen_size=20, max_dynamic_screen_size=20, percent_dense=0.2)}     # dense 0.2 > big 0.1

Class = namedtuple("Class", "grad scale logit flags")
# grad: a float, or "nan" (0 / 0 -> 0), "at" (accum = float32(2e-4), denom 1: selected by >=), "below" (its float32 predecessor)
# scale: the largest of the three; "nan": exp(NaN) in one column, the other two as for `clone` / `quad` -- torch.max propagates the
#        NaN, every comparison with it is false, the row is neither selected nor pruned
CLASSES = {
    "A": {"keep": Class(0.0, 0.005, 2.0, KEEP),
          "gone": Class(0.0, 0.005, -9.0, 0),
          "clone": Class(1e-3, 0.005, 2.0, KEEP | CLONE | KEEP_CLONE),
          "clone_gone": Class(1e-3, 0.005, -9.0, CLONE),                  # selected, then pruned: its draws are consumed
          "split": Class(1e-3, 0.05, 2.0, SPLIT | KEEP_CHILD),
          "split_gone": Class(1e-3, 0.05, -9.0, SPLIT),
          "nan_grad": Class("nan", 0.05, 2.0, KEEP),
          "big_quiet": Class(0.0, 0.5, 2.0, KEEP),
          "at_thr": Class("at", 0.005, 2.0, KEEP | CLONE | KEEP_CLONE),
          "below_thr": Class("below", 0.005, 2.0, KEEP),
          "nan_scale": Class(1e-3, "nan", 2.0, KEEP)},
    "B": {"keep": Class(0.0, 0.05, 2.0, KEEP),
          "gone": Class(0.0, 0.05, -9.0, 0),
          "clone": Class(1e-3, 0.05, 2.0, KEEP | CLONE | KEEP_CLONE),
          "clone_gone": Class(1e-3, 0.05, -9.0, CLONE),
          "nan_grad": Class("nan", 0.05, 2.0, KEEP),
          "quad": Class(1e-3, 0.15, 2.0, CLONE | SPLIT | SPLIT_CLONE | KEEP_CHILD | KEEP_CHILD_CLONE),   # four children from one row
          "split_kids_gone": Class(1e-3, 0.5, 2.0, SPLIT),               # children 0.5 / 1.6 > big: pruned, draws consumed
          "split_gone": Class(1e-3, 0.5, -9.0, SPLIT),
          "nan_scale": Class(1e-3, "nan", 2.0, KEEP)},
    # the three prunes: one table, a row either stays or goes
    "P": {"keep": Class(0.0, 0.005, 2.0, KEEP), "gone": Class(0.0, 0.005, 2.0, 0)},
}
NAN_SCALE_OTHERS = {"A": 0.005, "B": 0.15, "P": 0.005}   # the finite columns of nan_scale: `clone` / `quad` were the NaN not there
PRUNE_KINDS = ("invisible", "small", "nan")


def rows_out(flags):
    return sum(1 for b in (KEEP, KEEP_CLONE) if flags & b) + 2 * sum(1 for b in (KEEP_CHILD, KEEP_CHILD_CLONE) if flags & b)


# ------------------------------------------------------------------------------------------------------------------ layouts
def uniform(c, n):
    return [c] * n


def needle(c, background, n, at):
    out = [background] * n
    out[at] = c
    return out


def scan_per(n):
    """Blocks per thread of plan_scan_kernel."""
    nb = (n + BLOCK - 1) // BLOCK
    return (nb + SCAN_THREADS - 1) // SCAN_THREADS


def run_boundaries(n):
    """Where `runs` changes class: every multiple of 256 (every block uniform in one class), and one row either side of every
    third boundary between two scan threads' block ranges (256 * per * t, t = 1, 4, 7, ...; every fourth block where per = 1 makes
    all of them thread boundaries): those blocks start / end with a single row of another class."""
    per = scan_per(n)
    step = BLOCK * per
    cuts = set(range(BLOCK, n, BLOCK))
    for q in range(step if per > 1 else 4 * BLOCK, n, 3 * step if per > 1 else 4 * BLOCK):
        cuts |= {c for c in (q - 1, q + 1) if 0 < c < n}
    return sorted(cuts)


def runs(classes, n):
    cuts = [0] + run_boundaries(n) + [n]
    out = []
    for j in range(len(cuts) - 1):
        out += [classes[j % len(classes)]] * (cuts[j + 1] - cuts[j])
    return out


def alternating(classes, n):
    return [classes[i % len(classes)] for i in range(n)]


def random_layout(classes, n, seed):
    idx = np.random.default_rng(seed).integers(0, len(classes), n)
    return [classes[i] for i in idx]


def layout(config, spec):
    """The class name per row of a layout spec: ("uniform", c, n), ("needle", c, background, n, at), ("runs", n),
    ("alternating", (classes), n), ("random", n, seed); None or n = 0: no rows."""
    if spec is None:
        return []
    names = list(CLASSES[config])
    kind = spec[0]
    if kind == "uniform":
        return uniform(spec[1], spec[2])
    if kind == "needle":
        return needle(*spec[1:])
    if kind == "runs":
        return runs(names, spec[1])
    if kind == "alternating":
        return alternating(spec[1], spec[2])
    if kind == "random":
        return random_layout(names, spec[1], spec[2])
    raise ValueError(spec)


_ROWS_AT = {"uniform": 2, "needle": 3, "runs": 1, "alternating": 2, "random": 1}


def spec_rows(spec):
    return 0 if spec is None else spec[_ROWS_AT[spec[0]]]


# --------------------------------------------------------------------------------------------- expectations by construction
def class_flags(config, classes):
    table = CLASSES[config]
    return np.array([table[c].flags for c in classes], dtype=np.int64)


def counts_of_flags(flags):
    """The eight EX4D_CNT_* of include/ex4d_densify.h."""
    c = [int(((flags >> k) & 1).sum()) for k in range(7)]
    return np.array(c + [c[0] + c[2] + 2 * (c[5] + c[6])], dtype=np.int32)


def map_of_flags(flags):
    """[N, 8] int32, the map layout of include/ex4d_densify.h: dst_orig, dst_clone, dst_child (copy 0), dst_child_of_clone (copy 0),
    clone draw, split draw, split draw of the clone, unused; -1 = none.  Destinations: survivors in row order, then the surviving
    clones, then copy 0 of the children of split originals, of split clones, then copy 1 of both; draws: in row order, a split
    clone's after all split originals'."""
    n = flags.shape[0]
    bit = [((flags >> k) & 1).astype(np.int64) for k in range(7)]
    ex = [np.cumsum(b) - b for b in bit]                                   # exclusive running counts
    tot = [int(b.sum()) for b in bit]
    base = [0, 0, tot[0], 0, tot[3], tot[0] + tot[2], tot[0] + tot[2] + tot[5]]
    col_of_bit = {0: 0, 2: 1, 5: 2, 6: 3, 1: 4, 3: 5, 4: 6}
    out = np.full((n, 8), -1, dtype=np.int32)
    for k, col in col_of_bit.items():
        out[:, col] = np.where(bit[k] == 1, base[k] + ex[k], -1)
    return out


def expected_counts(classes, config="A"):
    return counts_of_flags(class_flags(config, classes))


def expected_map(classes, config="A"):
    return map_of_flags(class_flags(config, classes))


def gather_expected(src, mp, counts, new="copy"):
    """numpy statement of the multi-tensor gather for one [N, ...] array: every destination of a source row copies it (new =
    "copy"), or the new rows (clones, children) hold the constant `new` / the children alone hold `new[1]` where new = ("child", x)."""
    src = np.asarray(src)
    out = np.full((int(counts[ROWS]),) + src.shape[1:], np.nan, dtype=src.dtype)
    stride = int(counts[5] + counts[6])
    clone_val = child_val = None
    if isinstance(new, tuple):
        child_val = new[1]
    elif not isinstance(new, str):
        clone_val = child_val = new
    for col, kind in ((0, "orig"), (1, "clone"), (2, "child"), (3, "child")):
        sel = mp[:, col] >= 0
        dst = mp[sel, col].astype(np.int64)
        for off in ((0, stride) if kind == "child" else (0,)):
            const = clone_val if kind == "clone" else child_val if kind == "child" else None
            if const is None:
                out[dst + off] = src[sel]
            else:
                out[dst + off] = const
    return out


# --------------------------------------------------------------------------------------------------------------- the models
def _class_columns(rng, config, classes):
    """(gradient_accum, denom, scaling [N, 3], opacity logit) float32 of one group."""
    table = CLASSES[config]
    n = len(classes)
    accum, denom = np.zeros(n, np.float32), np.full(n, 4, np.float32)
    ms, logit = np.zeros(n, np.float32), np.zeros(n, np.float32)
    nan_col = np.zeros(n, bool)
    names = np.array(classes) if n else np.zeros(0, "<U1")
    for c in sorted(set(classes)):
        k, sel = table[c], names == c
        if k.grad == "nan":
            accum[sel], denom[sel] = 0, 0
        elif k.grad == "at":
            accum[sel], denom[sel] = np.float32(GRAD_THR), 1
        elif k.grad == "below":
            accum[sel], denom[sel] = np.nextafter(np.float32(GRAD_THR), np.float32(0)), 1
        else:
            accum[sel] = np.float32(k.grad) * np.float32(4)
        if k.scale == "nan":
            ms[sel], nan_col[sel] = NAN_SCALE_OTHERS[config], True
        else:
            ms[sel] = k.scale
        logit[sel] = k.logit
    offs = rng.permuted(np.tile(np.array([0.0, -0.3, -0.7], np.float32), (n, 1)), axis=1)
    scaling = (np.log(ms)[:, None] + offs).astype(np.float32)
    scaling[nan_col[:, None] & (offs == 0)] = np.nan                        # the largest column: whichever of the three it is
    return accum, denom, scaling, logit


def _stats(rng, n, names, accum, denom):
    """Reference-shaped statistics: the two class columns, everything densification_postfix resets filled with values that must
    not matter, error min / timestamp distinct per row."""
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    ts = rng.uniform(0, 300, n)
    ts[rng.random(n) < 0.125] = -1
    cols = [accum, denom, rng.uniform(0, 5, n), rng.uniform(0, 5, n), rng.integers(0, 9, n), rng.integers(0, 60, n), rng.integers(0, 12, n),
            rng.uniform(0, 2, n), ts]
    return {k: f(c) if k.endswith("radii2D") else f(c).view(n, 1) for k, c in zip(names, cols)}


def _shapes(ns, nd):
    return {"_xyz": (ns, 3), "_xyz_disp": (ns, 3), "_rotation": (ns, 4), "_opacity": (ns, 1), "_scaling": (ns, 3), "_features_dc": (ns, 1, 3),
            "_features_rest": (ns, 15, 3), "_xyz_motion": (nd, K, 3), "_rotation_motion": (nd, K, 4), "_opacity_motion": (nd, 1),
            "_opacity_duration_center": (nd, 2, 1), "_opacity_duration_var": (nd, 2, 1), "_scaling_motion": (nd, 3),
            "_features_dc_motion": (nd, 1, 3), "_features_rest_motion": (nd, 15, 3)}


def make_state(static_classes, dynamic_classes, seed, moments=True, config="A"):
    """The state dict of tests/densify_ref.py (float32, CPU) for one class name per row.  Everything that is only copied is random
    and distinct per row; moments are non-zero."""
    rng = np.random.default_rng(seed)
    ns, nd = len(static_classes), len(dynamic_classes)
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    P = {k: rng.standard_normal(s, dtype=np.float32) for k, s in _shapes(ns, nd).items()}
    stats = {}
    for classes, n, names, sc, op in ((static_classes, ns, R.S_STATS, "_scaling", "_opacity"), (dynamic_classes, nd, R.D_STATS, "_scaling_motion", "_opacity_motion")):
        accum, denom, scaling, logit = _class_columns(rng, config, classes)
        P[sc], P[op] = scaling, logit.reshape(n, 1)
        stats.update(_stats(rng, n, names, accum, denom))
    # duration centres inside [1.3, 31.1]: spans below and above 3 * min_len = 0.6, some close enough to an end to be clamped
    c0 = rng.uniform(1.5, 30.5, nd)
    P["_opacity_duration_center"] = np.stack([c0, c0 + rng.uniform(-2, 2, nd) * (rng.random(nd) < 0.7)], axis=1).reshape(nd, 2, 1)
    state = {"params": {k: f(v) for k, v in P.items()}, "m": None, "v": None, "stats": stats}
    if moments:
        # distinct per row like the parameters they are derived from (cheaper than two more random tensors each), never 0
        finite = {k: np.nan_to_num(np.asarray(v, dtype=np.float32), nan=1.0) for k, v in P.items()}
        state["m"] = {k: f(v * np.float32(0.37) + np.float32(3.0)) for k, v in finite.items()}
        state["v"] = {k: f(v * v + np.float32(0.1)) for k, v in finite.items()}
    return state


def make_plan_inputs(config, classes, seed):
    """What ex4d_densify_plan reads of one group: (stats block [9, N], scaling [N, 3], opacity [N]) float32 numpy."""
    rng = np.random.default_rng(seed)
    n = len(classes)
    accum, denom, scaling, logit = _class_columns(rng, config, classes)
    st = _stats(rng, n, R.S_STATS, accum, denom)
    return np.stack([st[k].numpy().reshape(n) for k in R.S_STATS]) if n else np.zeros((9, 0), np.float32), scaling, logit


def make_prune_state(kind, static_classes, dynamic_classes, seed, moments=True):
    """A model of `keep` rows whose "gone" rows one of the three prunes removes: error-min timestamp < 0 (invisible; 0 itself
    stays), min_radii2D < 5 (small; 5 itself stays), a NaN in one coordinate of _xyz / in the LAST keyframe's last coordinate only
    of _xyz_motion (nan: all 105 floats of a dynamic row have to be looked at)."""
    ns, nd = len(static_classes), len(dynamic_classes)
    state = make_state(["keep"] * ns, ["keep"] * nd, seed, moments=moments, config="P")
    rng = np.random.default_rng(seed + 1)
    for classes, n, names, xyz in ((static_classes, ns, R.S_STATS, "_xyz"), (dynamic_classes, nd, R.D_STATS, "_xyz_motion")):
        if n == 0:
            continue
        gone = torch.from_numpy(np.array([c == "gone" for c in classes], dtype=bool))
        st = state["stats"]
        if kind == "invisible":
            ts = torch.from_numpy(rng.uniform(0, 300, n).astype(np.float32))
            ts[::5] = 0.0
            ts[gone] = torch.from_numpy(np.where(rng.random(n) < 0.5, -1.0, -rng.uniform(1e-3, 300, n)).astype(np.float32))[gone]
            st[names[8]] = ts.view(n, 1)
        elif kind == "small":
            r = torch.from_numpy(rng.integers(5, 40, n).astype(np.float32))
            r[::5] = 5.0
            r[gone] = torch.from_numpy(rng.integers(0, 5, n).astype(np.float32))[gone]
            st[names[6]] = r
        else:
            x = state["params"][xyz].view(n, -1)
            col = torch.from_numpy(rng.integers(0, 3, n)) if xyz == "_xyz" else torch.full((n,), x.shape[1] - 1 if n else 0)
            rows = torch.nonzero(gone).view(-1)
            x[rows, col[rows]] = float("nan")
    return state


def make_draws(counts_s, counts_d, seed):
    """Explicit standard-normal draws with the keys and shapes of ex4dgs_amd.densify._draws."""
    g = torch.Generator().manual_seed(seed)
    nc_d = int(counts_d[1])
    ns_s, ns_d = int(counts_s[3] + counts_s[4]), int(counts_d[3] + counts_d[4])
    shapes = {"clone_c1": (nc_d,), "clone_c0": (nc_d,), "static_split_z": (2 * ns_s, 3), "split_z": (2 * ns_d, 3), "split_c1": (2 * ns_d,),
              "split_c0": (2 * ns_d,)}
    return {k: torch.randn(s, generator=g) for k, s in shapes.items()}


E0_SPECIAL = (float("nan"), 0.0, 5e-5, float(np.float32(1e-4)), float(np.float32(0.01)), 0.02, -0.01)


def make_frames(ns, nd, seed, n_frames=3):
    """[(radii int32 [P], vgrad [P, 3], egrad [P, 3], timestamp)] per frame.  radii <= 0 and > 0; view-space gradients over six
    decades; e0 takes the values at which train.py's filters and clamps switch (NaN, 0, below / at the 1e-4 clamp, at / above the
    0.01 gate, negative) and random ones; e1 / e0 falls over the frames for even rows and rises for odd ones, so that error_min and
    its timestamp are and are not replaced on the later frames."""
    rng = np.random.default_rng(seed)
    p = ns + nd
    e0 = rng.uniform(0.011, 0.05, p).astype(np.float32)
    special = rng.random(p) < 0.4
    e0[special] = np.array(E0_SPECIAL, np.float32)[rng.integers(0, len(E0_SPECIAL), p)][special]
    e0[: min(p, len(E0_SPECIAL))] = np.array(E0_SPECIAL, np.float32)[: min(p, len(E0_SPECIAL))]
    base = rng.uniform(0.2, 3.0, p).astype(np.float32)
    out = []
    for j in range(n_frames):
        radii = rng.integers(-1, 40, p).astype(np.int32)
        radii[rng.random(p) < 0.2] = 0
        vgrad = (rng.standard_normal((p, 3)) * 10.0 ** rng.uniform(-7, -1, (p, 1))).astype(np.float32)
        ratio = np.where(np.arange(p) % 2 == 0, base * np.float32(0.7) ** j, base * np.float32(1.3) ** j).astype(np.float32)
        wobble = rng.uniform(0.9, 1.1, p).astype(np.float32) if j else np.ones(p, np.float32)
        e0j = e0 * wobble                                                   # NaN, 0 stay; the special values hold on frame 0
        egrad = np.stack([e0j, e0j * ratio, rng.uniform(0, 0.02, p).astype(np.float32)], axis=1).astype(np.float32)
        out.append((torch.from_numpy(radii), torch.from_numpy(vgrad), torch.from_numpy(egrad), float((7, 3, 11, 5)[j % 4] + 10 * (j // 4))))
    return out


def make_stats_prefill(ns, nd, seed):
    """Reference-shaped statistics to start an update from: half of the rows at their initial values, half arbitrary (distinct
    bits: an update that skips a row of the block must leave exactly these behind)."""
    rng = np.random.default_rng(seed)
    st = R.init_stats(ns, nd)
    for names, n in ((R.S_STATS, ns), (R.D_STATS, nd)):
        arb = _stats(rng, n, names, rng.uniform(0, 1e-2, n), rng.integers(0, 9, n))
        used = torch.from_numpy(rng.random(n) < 0.5)
        for k in names:
            st[k][used] = arb[k][used]
    return st


def to_dtype(state, dtype):
    conv = lambda d: None if d is None else {k: v.to(dtype) for k, v in d.items()}
    return {"params": conv(state["params"]), "m": conv(state["m"]), "v": conv(state["v"]), "stats": conv(state["stats"])}


def clone_state(state):
    conv = lambda d: None if d is None else {k: v.clone() for k, v in d.items()}
    return {k: conv(state[k]) for k in ("params", "m", "v", "stats")}


def f32(x):
    return float(np.float32(x))


def assert_same(got, want, what):
    """NaN-aware exact equality; the slow element-wise report only when it fails."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype or not np.array_equal(got, want, equal_nan=True):
        np.testing.assert_array_equal(got, want, err_msg=what)
        assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)


def run_restatement(state, config, draws, dtype=torch.float32):
    """densify_ref.densify_and_prune on a copy of `state` in `dtype`.  The thresholds go in rounded to float32, as
    ex4dgs_amd.densify hands them to the kernel: in float64 `at_thr` would otherwise sit below an unrounded 2e-4."""
    cfg = CONFIGS[config]
    st = to_dtype(clone_state(state), dtype)
    d = {k: v.to(dtype) for k, v in draws.items()}
    r = lambda x: None if x is None else (x if dtype == torch.float32 else f32(x))
    ext = cfg["extent"]
    R.densify_and_prune(st, MODEL, r(cfg["max_grad"]), r(cfg["max_dgrad"]), r(cfg["min_opacity"]), r(cfg["min_motion_opacity"]), ext,
                        cfg["max_screen_size"], cfg["max_dynamic_screen_size"], d, s_max_ssim=cfg["s_max_ssim"], s_l1_thres=cfg["s_l1_thres"],
                        d_max_ssim=cfg["d_max_ssim"], d_l1_thres=cfg["d_l1_thres"], percent_dense=cfg["percent_dense"])
    return st


# ------------------------------------------------------------------------------------------------------------------- the bars
def transformed_error_over_bar(got, ref64):
    """max of |got - ref| / (1e-6 |ref| + 1e-6 max(1, |ref|_inf)) for one of the five transformed tensors (the bar of
    test_densify_at_one_million_against_restatement), NaN-aware: a NaN of the reference (the nan_scale rows' own scale) must be a
    NaN of `got` and the other way round."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    nan = np.isnan(ref)
    if not np.array_equal(nan, np.isnan(got)):
        return float("inf")
    if nan.all():
        return 0.0
    top = max(1.0, float(np.abs(ref[~nan]).max()))
    bar = 1e-6 * np.abs(ref[~nan]) + 1e-6 * top
    return float((np.abs(got[~nan] - ref[~nan]) / bar).max())


def grad_accum_error_over_bar(got, ref64, n_updates):
    """max of |got - ref| in float32 ulps of the accumulated value, over the bar 2 n + 1 ulps after n updates."""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref64, np.float64).reshape(-1)
    if ref.size == 0:
        return 0.0
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return float((np.abs(got - ref) / ulp).max() / (2 * n_updates + 1))


# ------------------------------------------------------------------------------------------------------------------ the cases
ROW_COUNTS = (1, 2, 255, 256, 257, 511, 512, 513, 4095, 4097, 65536, 65537, 131073)
SMALL = (1, 2, 255, 256, 257, 511, 512, 513)
Case = namedtuple("Case", "name config static dynamic seed")          # static / dynamic: layout specs (dynamic None: Nd = 0)
ALTERNATING = {"A": (("clone", "split"), ("split_gone", "clone", "keep")), "B": (("quad", "keep"), ("clone", "quad", "split_kids_gone")),
               "P": (("keep", "gone"), ("gone", "keep", "keep"))}


def _name(spec):
    return "none" if spec is None else "-".join("+".join(x) if isinstance(x, tuple) else str(x) for x in spec)


def _needles(names, n):
    ats = sorted({a for a in (0, BLOCK - 1, BLOCK, n - 1) if a < n})
    return [("needle", names[(j + n) % len(names)], names[(j + n + 3) % len(names)], n, at) for j, at in enumerate(ats)]


@functools.lru_cache(maxsize=None)
def layout_specs(config):
    """Every layout of a configuration, each run through the plan for both groups: `uniform` (every class) and `needle` at <= 513
    rows and at 65 537; `runs`, `alternating` (period 2 and 3) and `random` at 4097, 65 537 and 131 073; 4095 and 65 536 rows once."""
    names = list(CLASSES[config])
    out = [("uniform", c, n) for n in SMALL + (65537,) for c in names]
    for n in (256, 257, 513, 65537):
        out += _needles(names, n)
    for n in (4097, 65537, 131073):
        out += [("runs", n), ("alternating", ALTERNATING[config][0], n), ("alternating", ALTERNATING[config][1], n), ("random", n, n % 1000)]
    out += [("random", 4095, 5), ("runs", 65536), ("random", 65536, 6)]
    return tuple(out)


# one multi-block mixed case per configuration for the tests that run a single case (FrameTrainer adapter, prefilled destinations)
MIXED = {"A": "A:mixed-65537|65537", "B": "B:mixed-65537|65537"}


@functools.lru_cache(maxsize=None)
def cases():
    """The whole-call cases: every layout of layout_specs("A" / "B") as the static group of one case, with a DIFFERENT layout as the
    dynamic group; the dynamic group (301 floats per row, three tensors each with the moments) stays at <= 65 537 rows and gets every
    small layout, and the large ones listed below."""
    out = []
    for config in ("A", "B"):
        names = list(CLASSES[config])
        specs = layout_specs(config)
        small = [s for s in specs if spec_rows(s) <= 513]
        alt = ALTERNATING[config]
        big_dynamic = [("runs", 65537), ("alternating", alt[1], 4097), ("random", 4097, 78), ("alternating", alt[0], 4097), ("runs", 4097),
                       ("random", 65537, 77), ("alternating", alt[1], 4097)]
        large_dynamic = [("uniform", names[2], 65537), ("uniform", names[5], 65537), _needles(names, 65537)[2], _needles(names, 65537)[3]]
        nbig = 0
        for k, s in enumerate(specs):
            if spec_rows(s) <= 513:
                d = small[(k + len(names) + 1) % len(small)]
            elif s[0] in ("uniform", "needle"):
                d = small[(7 * k) % len(small)]
            else:
                d = next(b for b in big_dynamic[nbig % len(big_dynamic):] + big_dynamic if b[0] != s[0])
                nbig += 1
            out.append(Case(f"{config}:{_name(s)}|{_name(d)}", config, s, d, 1000 + len(out)))
        for b in large_dynamic:                                                # large uniform / needle layouts in the dynamic group
            s = small[(11 * len(out)) % len(small)]
            out.append(Case(f"{config}:{_name(s)}|{_name(b)}", config, s, b, 1000 + len(out)))
        for s in (("uniform", names[2], 1), ("random", 257, 9), ("random", 65537, 10)):      # (N, 0): the static-only path
            out.append(Case(f"{config}:{_name(s)}|none", config, s, None, 1000 + len(out)))
        out.append(Case(MIXED[config], config, ("random", 65537, 91), ("runs", 65537), 1000 + len(out)))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def prune_cases():
    """(name, static spec, dynamic spec, seed) for the three prunes: the "gone" rows placed by the same layouts."""
    P = [("uniform", "keep", 256), ("uniform", "gone", 257), ("needle", "gone", "keep", 513, 0), ("needle", "gone", "keep", 513, 255),
         ("needle", "keep", "gone", 513, 256), ("needle", "gone", "keep", 513, 512), ("runs", 4097), ("random", 4097, 3),
         ("alternating", ALTERNATING["P"][0], 4097), ("alternating", ALTERNATING["P"][1], 513), ("uniform", "gone", 1), ("uniform", "keep", 2)]
    out = [Case(f"P:{_name(s)}|{_name(P[(k + 5) % len(P)])}", "P", s, P[(k + 5) % len(P)], 2000 + k) for k, s in enumerate(P)]
    out += [Case("P:runs-131073|random-65537", "P", ("runs", 131073), ("random", 65537, 4), 2100),
            Case("P:random-65537|runs-65537", "P", ("random", 65537, 5), ("runs", 65537), 2101),
            Case("P:random-257|none", "P", ("random", 257, 6), None, 2102)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def prune_layout_specs():
    out = []
    for c in prune_cases():
        out += [s for s in (c.static, c.dynamic) if s is not None and s not in out]
    return tuple(out + [("random", 131073, 8), ("alternating", ALTERNATING["P"][0], 65537)])


def case_by_name(name):
    return next(c for c in cases() + prune_cases() if c.name == name)
