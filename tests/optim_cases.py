"""Constructed inputs for the fused RAdam steps (ex4dgs_amd/csrc/ex4d_optim.hip) at the edges of their chunk table, slot table,
window arithmetic and step count, shared by tests/test_cpu_optim_cases.py (the cases hit the edges they name; the numpy restatement
oracle/optim_oracle.py they are compared with follows torch.optim.RAdam in float64; none of its coefficients is a rounding accident)
and tests/test_gpu_optim_edges.py (the kernels give the restatement's BITS).

The numbers restate the layout of ex4d_optim.hip: radam_kernel / radam_sliced_kernel work in chunks of CHUNK = 4096 elements (16-byte
accesses when the chunk is full and every pointer aligned, element by element otherwise), a launch carries at most MAX_TENSORS dense
or MAX_SLICED sliced tensors whose workgroups find their slot by a scan over the slots' first chunks, a sliced tensor has at most
MAX_WINDOWS gradient windows, and a workgroup of the regularised step stages R = reg_rows(K, C) whole rows twice in REG_LDS_BYTES of
LDS.  Everything is seeded.  The dense and regularised cases are small (no tensor above ~4 chunks, a launch below 200 k elements);
the sliced case keeps the two keyframe shapes of the existing tests, (1003, 35, 3) = 105 315 and (777, 35, 4) = 108 780 elements
(26 and 27 chunks), so its first launch of four tensors has 214 332 elements.

Expected values never come from the library: `expected_dense` / `expected_sliced` apply oracle/optim_oracle.py to copies.
"""
import functools

import numpy as np

from oracle import optim_oracle as oo

f32 = np.float32
CHUNK = 4096                     # RADAM_CHUNK
MAX_TENSORS = 32                 # EX4D_RADAM_MAX_TENSORS
MAX_SLICED = 4                   # EX4D_RADAM_MAX_SLICED
MAX_WINDOWS = 8                  # EX4D_RADAM_MAX_WINDOWS
REG_LDS_BYTES = 32768
REG_NONE, REG_MOTION, REG_ROT = 0, 1, 2
BETAS = (0.9, 0.999)             # the reference's (torch's defaults)
BETAS_B = (0.9, 0.99)            # a second pair with beta1 > 0.5 (torch's lerp_ keeps its formula)
EPS = 1e-8
GUARD = 0xCAFEF00D               # bit pattern of the padding around the alignment case's views
# the learning rates of the model's parameter groups; the two extremes sit next to each other
LRS = (1.6e-4, 1e-3, 1e-4, 5e-2, 2.5e-3, 5e-3, 1.25e-4)
UNRECTIFIED_STEPS = (1, 5)
RECTIFIED_STEPS = (6, 7, 12, 100, 29999, 30000, 120000)


def reg_rows(K, C):
    """reg_block_rows of ex4d_optim.hip: rows a workgroup stages (p and the regulariser gradient), a multiple of 4 up to 32; 0: no fit."""
    R = REG_LDS_BYTES // (2 * K * C * 4)
    return 32 if R > 32 else R & ~3


def reg_lds_bytes(K, C):
    return 2 * reg_rows(K, C) * K * C * 4


def switch_step(betas):
    """The first step with rho_t > 5 (the rectified update)."""
    t = 1
    while not oo.radam_coefficients(t, 1e-3, betas[0], betas[1], EPS).rectified:
        t += 1
    return t


def _rng(*key):
    return np.random.default_rng([20241, *key])


# ------------------------------------------------------------------------------------------------------------------ dense: slot table
SLOT_NUMELS = (1, 3, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 12293)
ZERO_POSITIONS = (0, 5, 6, MAX_TENSORS - 1)          # numel == 0 descriptors (null pointers) of the C-ABI variant


def slot_step(i):
    """Rectified and unrectified slots alternate."""
    return RECTIFIED_STEPS[(i // 2) % len(RECTIFIED_STEPS)] if i % 2 else UNRECTIFIED_STEPS[(i // 2) % len(UNRECTIFIED_STEPS)]


@functools.lru_cache(maxsize=None)
def slot_tensors(count):
    """`count` dense tensors, each with its own (step, lr, nan_to_num), seeded non-zero state and a gradient that holds one NaN, one
    +inf and one -inf (a one-element tensor: the NaN only).  Returns a tuple of dicts of read-only arrays."""
    out = []
    for i in range(count):
        n = SLOT_NUMELS[i % len(SLOT_NUMELS)]
        r = _rng(1, i)
        t = dict(p=r.standard_normal(n).astype(f32), g=(r.standard_normal(n) * (1e-4 if i % 4 < 2 else 0.1)).astype(f32),
                 m=(r.standard_normal(n) * 1e-2).astype(f32), v=(r.random(n) * 1e-4).astype(f32),
                 step=slot_step(i), lr=LRS[i % len(LRS)], nan_to_num=int(i % 3 == 1), betas=BETAS)
        planted = [n // 2] if n == 1 else [n // 2, n - 1, 0]
        for at, val in zip(planted, (np.nan, np.inf, -np.inf)):
            t["g"][at] = val
        t["planted"] = tuple(planted)
        for k in "pgmv":
            t[k].setflags(write=False)
        out.append(t)
    return tuple(out)


def expected_dense(t, p=None, m=None, v=None, g=None):
    """(p, m, v) after one step of tensor dict t by the restatement (on copies; p, m, v, g override the dict's arrays)."""
    p, m, v = [(t[k] if a is None else a).astype(f32).copy() for k, a in zip("pmv", (p, m, v))]
    oo.radam_step(p, t["g"] if g is None else g, m, v, t["step"], t["lr"], t["betas"][0], t["betas"][1], EPS, nan_to_num=bool(t.get("nan_to_num", 0)))
    return p, m, v


def planted_mask(t):
    """Where an unsanitised tensor may turn NaN: its planted gradient elements.  A sanitised tensor: nowhere."""
    mask = np.zeros(t["p"].shape, bool)
    if not t.get("nan_to_num", 0):
        mask.reshape(-1)[list(t["planted"])] = True
    return mask


# ------------------------------------------------------------------------------------------------------------------ dense: trajectory
TRAJ_NUMEL = CHUNK + 1
LATE_STEPS = (29999, 30000, 30001)


def trajectory_steps(betas):
    """1..8 with the state carried forward from zero; includes the step on each side of the rho_t > 5 switch of `betas`."""
    sw = switch_step(betas)
    return tuple(sorted(set(range(1, 9)) | {sw - 1, sw}))


@functools.lru_cache(maxsize=None)
def trajectory(betas):
    """Two runs of one 4097-element tensor: `early` (zero state, trajectory_steps) and `late` (seeded state, LATE_STEPS).  Each is
    (p0, m0, v0, [(step, lr, g), ...]); every step has its own gradient, some of it zero, and its own learning rate."""
    runs = {}
    for name, steps in (("early", trajectory_steps(betas)), ("late", LATE_STEPS)):
        r = _rng(2, int(betas[1] * 1000), len(steps))
        p0 = r.standard_normal(TRAJ_NUMEL).astype(f32)
        m0 = np.zeros(TRAJ_NUMEL, f32) if name == "early" else (r.standard_normal(TRAJ_NUMEL) * 1e-3).astype(f32)
        v0 = np.zeros(TRAJ_NUMEL, f32) if name == "early" else (r.random(TRAJ_NUMEL) * 1e-6).astype(f32)
        seq = []
        for j, s in enumerate(steps):
            g = (r.standard_normal(TRAJ_NUMEL) * 1e-3).astype(f32)
            g[r.random(TRAJ_NUMEL) < 0.3] = 0                  # elements no frame touched: moved by their momentum alone
            seq.append((s, LRS[j % len(LRS)], g))
        runs[name] = (p0, m0, v0, seq)
    return runs


# ------------------------------------------------------------------------------------------------------------------ dense: alignment
ALIGN_OFFSETS = ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 2, 3, 1))      # floats, for p, g, m, v
ALIGN_NUMELS = (CHUNK, 2 * CHUNK + 5, 3)
ALIGN_FRONT, ALIGN_BACK = 4, 8                       # guard floats before (keeps 16-byte alignment) and after every view


@functools.lru_cache(maxsize=None)
def alignment_tensors():
    out = []
    for i, n in enumerate(ALIGN_NUMELS):
        r = _rng(3, i)
        t = dict(p=r.standard_normal(n).astype(f32), g=(r.standard_normal(n) * 1e-3).astype(f32), m=(r.standard_normal(n) * 1e-3).astype(f32),
                 v=(r.random(n) * 1e-6).astype(f32), step=(7, 5, 100)[i], lr=LRS[i], nan_to_num=0, betas=BETAS, planted=())
        out.append(t)
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------ dense: value edges
# name -> (p, g, m, v); the plants sit in the 16-byte path (the first, full chunk); the one-element tail repeats g_subnormal
EDGE_PLANTS = {
    "zero":          (1.5, 0.0, 0.0, 0.0),            # 0 / (0 + eps): no move, state stays zero
    "neg_zero":      (-0.0, -0.0, 0.0, 0.0),
    "g_subnormal":   (0.25, 1e-40, 0.0, 0.0),         # m = 0.1 g and v stay subnormal / underflow
    "v_subnormal":   (0.25, 0.0, 1e-5, 1e-42),        # sqrt of a subnormal
    "v_at_eps":      (0.25, 0.0, 1e-6, 1e-16),        # sqrt(v) ~ eps
    "g_1e20":        (0.25, 1e20, 0.0, 0.0),
    "g_-1e20":       (0.25, -1e20, 0.0, 0.0),
    "g_1e21":        (0.25, 1e21, 0.0, 0.0),          # (w2 g) g overflows: v = inf, adaptive = 0, no move
    "g_-1e21":       (0.25, -1e21, 0.0, 0.0),
    "g_inf":         (0.25, np.inf, 1e-3, 1e-6),
    "g_-inf":        (0.25, -np.inf, 1e-3, 1e-6),
    "g_nan":         (0.25, np.nan, 1e-3, 1e-6),
    "p_1e30":        (1e30, 1e-3, 1e-3, 1e-6),
    "p_-1e30":       (-1e30, 1e-3, 1e-3, 1e-6),
    "p_1e-30":       (1e-30, 1e-3, 1e-3, 1e-6),
    "m_against_g":   (0.25, 0.3, -0.5, 0.04),
    "g_against_m":   (0.25, -0.3, 0.5, 0.04),
}
EDGE_NUMEL = CHUNK + 1
EDGE_NONFINITE = ("g_inf", "g_-inf", "g_nan")
EDGE_RUNS = tuple((step, flag) for step in (5, 6) for flag in (0, 1))      # (unrectified, rectified) x nan_to_num
EDGE_LR = 1e-3


def edge_index(name, tail=False):
    """Plants sit from element 8 on, five apart (every lane of a 16-byte access gets some); tail: the element past the full chunk."""
    return CHUNK if tail else 8 + 5 * list(EDGE_PLANTS).index(name)


@functools.lru_cache(maxsize=None)
def edge_tensor():
    r = _rng(4)
    n = EDGE_NUMEL
    t = dict(p=r.standard_normal(n).astype(f32), g=(r.standard_normal(n) * 1e-3).astype(f32), m=(r.standard_normal(n) * 1e-3).astype(f32),
             v=(r.random(n) * 1e-6).astype(f32), lr=EDGE_LR, betas=BETAS)
    for name, vals in EDGE_PLANTS.items():
        for k, x in zip("pgmv", vals):
            t[k][edge_index(name)] = x
    for k, x in zip("pgmv", EDGE_PLANTS["g_subnormal"]):
        t[k][CHUNK] = x
    t["planted"] = tuple(edge_index(nm) for nm in EDGE_NONFINITE)
    return t


def edge_run(step, flag):
    return dict(edge_tensor(), step=step, nan_to_num=flag)


# ------------------------------------------------------------------------------------------------------------------ FusedRAdam.step
OPT_PARAMS = 40                                       # two launches


@functools.lru_cache(maxsize=None)
def optimizer_params():
    """40 small parameters in groups of their own learning rate; two steps of gradients, None for some (those keep their step count)."""
    out = []
    for i in range(OPT_PARAMS):
        r = _rng(5, i)
        shape = ((1,), (3,), (7, 3), (5, 7, 4), (257,), (33, 1, 4), (600,), (2, 2))[i % 8]
        grads = [None if (i + 3 * s) % 7 == 2 else (r.standard_normal(shape) * 1e-2).astype(f32) for s in range(2)]
        out.append(dict(p=r.standard_normal(shape).astype(f32), lr=LRS[i % len(LRS)], grads=grads))
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------ sliced
def _windows(r, rows, C, spec):
    """spec: ((first, count), ...) or "=j" for an identical copy of window j (same position, same block)."""
    out = []
    for w in spec:
        if isinstance(w, str):
            out.append(out[int(w[1:])])
        else:
            out.append((w[0], (r.standard_normal((rows, w[1], C)) * 1e-2).astype(f32)))
    return out


# (rows, K, C), step, lr, windows as (first, count)
SLICED_SPECS = (
    ((1003, 35, 3), 5, 1.6e-4, ((0, 4), (2, 4), (17, 4), "=1", (31, 4), (30, 2), (9, 1), (34, 1))),   # 8 windows, two identical
    ((0, 35, 4), 3, 1e-3, ((0, 2),)),                                                                   # no rows: left out
    ((777, 35, 4), 6, 1e-4, ((0, 35), (12, 1), (0, 2), (33, 2))),                                       # count == K, count == 1, both ends
    ((5, 7, 3), 100, 5e-2, ((1, 4), (2, 4), (3, 4))),                                                   # three overlapping, the last ends at K
    ((33, 1, 4), 30000, 2.5e-3, ((0, 1),)),                                                             # K == 1
    ((130, 7, 4), 7, 5e-3, ((6, 1), (0, 3))),                                                           # count == 1 on the last keyframe
    ((1, 35, 3), 1, 1.25e-4, ()),                                                                       # no window: momentum alone
)
# one tensor as an offset row range of a larger one: odd K C and an odd row offset, so the base pointer is not 16-byte aligned
RANGE_TOTAL, RANGE_ROW0, RANGE_ROWS, RANGE_K, RANGE_C = 650, 3, 640, 7, 3


def _sliced_tensor(key, shape, step, lr, spec, total_rows=None, row0=0):
    rows, K, C = shape
    r = _rng(6, *(key if isinstance(key, tuple) else (key,)))
    full = (total_rows if total_rows is not None else rows, K, C)
    return dict(shape=shape, full=full, row0=row0, p=r.standard_normal(full).astype(f32), m=(r.standard_normal(full) * 1e-3).astype(f32),
                v=(r.random(full) * 1e-6).astype(f32), step=step, lr=lr, betas=BETAS, windows=_windows(r, rows, C, spec))


@functools.lru_cache(maxsize=None)
def sliced_tensors(with_range=False):
    """The seven items (six live: the wrapper launches 4 + 2).  with_range: the (5, 7, 3) tensor is replaced by rows [3, 643) of a
    [650, 7, 3] tensor (more than three chunks from an unaligned base)."""
    out = []
    for i, (shape, step, lr, spec) in enumerate(SLICED_SPECS):
        if with_range and shape == (5, 7, 3):
            out.append(_sliced_tensor(100 + i, (RANGE_ROWS, RANGE_K, RANGE_C), step, lr, spec, RANGE_TOTAL, RANGE_ROW0))
        else:
            out.append(_sliced_tensor(i, shape, step, lr, spec))
    return tuple(out)


def expected_sliced(t, grad=None):
    """(p, m, v) of the FULL tensor after one step on its row range: the restatement on dense_from_windows (or on `grad`, the dense
    gradient of the range: the regularised cases pass windows + regulariser); rows outside the range keep their bits."""
    rows, K, C = t["shape"]
    p, m, v = t["p"].copy(), t["m"].copy(), t["v"].copy()
    if rows:
        g = oo.dense_from_windows(rows, K, C, t["windows"]) if grad is None else grad
        sl = slice(t["row0"], t["row0"] + rows)
        q, a, b = p[sl].copy(), m[sl].copy(), v[sl].copy()
        oo.radam_step(q, g.astype(f32), a, b, t["step"], t["lr"], t["betas"][0], t["betas"][1], EPS)
        p[sl], m[sl], v[sl] = q, a, b
    return p, m, v


def window_classes(t):
    """The window classes of the issue that tensor t shows."""
    K = t["shape"][1]
    ws = [(f, b.shape[1]) for f, b in t["windows"]]
    cls = set()
    if len(ws) == MAX_WINDOWS:
        cls.add("eight")
    if len(set(ws)) < len(ws):
        cls.add("identical")
    for f, c in ws:
        cls |= {"count==K"} if c == K else set()
        cls |= {"count==1"} if c == 1 else set()
        cls |= {"first==0"} if f == 0 else set()
        cls |= {"first==K-count"} if f == K - c else set()
    if sum(1 for a in ws for b in ws if a < b and a[0] < b[0] < a[0] + a[1]) >= 2:
        cls.add("overlapping")
    return cls


# ------------------------------------------------------------------------------------------------------------------ first_dev out of range
def outside_positions(K, count):
    """Window positions the host would refuse, legal in device memory: wholly before, partly before, partly past, last keyframe, past."""
    return (-count, -1, K - count + 1, K - 1, K)


@functools.lru_cache(maxsize=None)
def outside_tensors():
    out = []
    for i, (shape, count, step) in enumerate((((130, 35, 3), 4, 6), ((5, 7, 3), 4, 5), ((1100, 2, 4), 2, 100))):
        K = shape[1]
        out.append(_sliced_tensor(200 + i, shape, step, LRS[i], tuple((f, count) for f in outside_positions(K, count))))
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------ regularised step
REG_ROWS_TABLE = {(341, 3): 4, (342, 3): 0, (256, 4): 4, (257, 4): 0, (1, 3): 32, (1, 4): 32}
REG_LIMITS = ((341, 3, REG_MOTION), (256, 4, REG_ROT))
REG_LIMIT_ROWS = (1, 4, 5, 9)
REG_LIMIT_WINDOWS = (1, 3)
REG_WEIGHT = 1e-3
# the mixed launch: a different R per slot, one LDS size (that of the K = 341 slot, which is not the last)
REG_MIXED = (((9, 341, 3), REG_MOTION), ((33, 1, 4), REG_ROT), ((70, 35, 4), REG_ROT), ((37, 2, 3), REG_NONE))


def _keyframes(r, rows, K, C):
    """Keyframe tensors as training has them: positions drifting from keyframe 0, near-unit quaternions."""
    p = r.standard_normal((rows, 1, C)) + np.cumsum((0.05 if C == 3 else 0.1) * r.standard_normal((rows, K, C)), 1)
    if C == 4:
        p /= np.linalg.norm(p, axis=-1, keepdims=True)
    return p.astype(f32)


@functools.lru_cache(maxsize=None)
def reg_tensor(rows, K, C, kind, n_windows, step):
    r = _rng(7, rows, K, C, kind, n_windows)
    count = min(4 if C == 3 else 2, K)
    firsts = [int(r.integers(0, K - count + 1)) for _ in range(n_windows)]
    t = _sliced_tensor((300, rows, K, C, kind, n_windows), (rows, K, C), step, LRS[(rows + n_windows) % len(LRS)], tuple((f, count) for f in firsts))
    t["p"] = _keyframes(r, rows, K, C)
    t["windows"] = [(f, (b * f32(1e-2)).astype(f32)) for f, b in t["windows"]]      # ~1e-4, the size of the regulariser's gradient
    t["kind"], t["weight"], t["reg_rows"] = kind, REG_WEIGHT, rows
    return t


def reg_limit_cases():
    for K, C, kind in REG_LIMITS:
        for i, rows in enumerate(REG_LIMIT_ROWS):
            for nw in REG_LIMIT_WINDOWS:
                yield reg_tensor(rows, K, C, kind, nw, (5, 6, 100, 30000)[i])


def reg_mixed_case():
    return tuple(reg_tensor(s[0], s[1], s[2], kind, 1 + i % 3, (6, 5, 30000, 7)[i]) for i, (s, kind) in enumerate(REG_MIXED))


# ------------------------------------------------------------------------------------------------------------------ every coefficient point
def coefficient_points():
    """Every (step, betas, lr) any case above runs: what test_cpu_optim_cases.py proves free of rounding accidents."""
    pts = set()
    for t in slot_tensors(MAX_TENSORS + 1) + alignment_tensors() + sliced_tensors() + sliced_tensors(True) + outside_tensors() + reg_mixed_case():
        pts.add((t["step"], t["betas"], t["lr"]))
    for t in reg_limit_cases():
        pts.add((t["step"], t["betas"], t["lr"]))
    for betas in (BETAS, BETAS_B):
        for run in trajectory(betas).values():
            pts |= {(s, betas, lr) for s, lr, _ in run[3]}
    pts |= {(s, BETAS, EDGE_LR) for s, _ in EDGE_RUNS}
    for q in optimizer_params():
        pts |= {(s, BETAS, q["lr"]) for s in (1, 2)}
    return sorted(pts)
