"""Scenes, upstream-gradient layouts and a host census of the compositing backward's inner loops, shared by
tests/test_cpu_composite_cases.py (the cases have the properties they are chosen for, on the CPU oracle) and
tests/test_gpu_composite_variants.py (every loop against the oracle, and the census against the kernel's own counters).

The census restates the dispatch of composite_bwd_scan_kernel (ex4dgs_amd/csrc/ex4d_composite.hip): one wave per 8x8 quadrant of a
16x16 tile decides, from its 64 pixels,
    sep        every inside pixel sits at its integer position: float32(px) + offset == float32(px), likewise y
    use_extra  a pixel carries an upstream depth gradient, or (where acc > 0) a flow gradient
    use_gacc   a pixel with acc > 0 carries an upstream dL_dacc
    deepest    max n_contrib (0 outside the image); 0 = nothing to do, the wave returns
    min_last   min n_contrib (0 outside the image)
and walks the entries of its compacted list whose position lies below `deepest`, back to front, in batches of 16 (the last one
possibly shorter) through a ring of 96 slots.  A batch is NOLAST when it is full and the position of its first (= deepest) entry is
below min_last.  Each batch runs one of 13 instantiations, named as below."""
import numpy as np
import torch

from ex4dgs_amd.scene import SceneConfig

TILE, QUAD, BATCH, RING = 16, 8, 16, 96

# 7 x 5 tiles; the last tile column keeps 4 pixel columns (its right quadrants lie outside the image), the last tile row 6 pixel rows.
# Deep tile lists (most quadrants' deepest contributor lies beyond position 96) of Gaussians that cover whole quadrants, so nearly every
# pixel of a step contributes.  Rendered with dir3D = 0 (DEEP_DIR_SCALE), like the training loop's frames.
DEEP = SceneConfig("composite deep", 1500, 100, 70, 60.0, min_depth=0.01, z_lo=0.5, z_hi=40.0, sigma_px_med=5.0, sigma_px_logstd=0.8, seed=7)
DEEP_DIR_SCALE = 0.0
# DEEP's footprints (5 px) cover whole quadrants, so a quadrant's compacted list is about as long as one pixel's list of contributors:
# ~65 entries survive the quadrant cull in front of the deepest contributor, and more Gaussians only saturate the pixels sooner (7 of the
# 117 quadrants walk more than the ring holds, at any P).  WRAP is DEEP with 1.5 px footprints: a quadrant collects the short lists of 64
# pixels that see different Gaussians -- ~140 entries walked per quadrant, past the ring's 96 slots in every (sep, extra, gacc) class.
WRAP = DEEP._replace(name="composite deep, small footprints", P=4000, sigma_px_med=1.5)
# a few small Gaussians: quadrants without any contributor, lists shorter than one batch, pixels with acc == 0
SPARSE = SceneConfig("composite sparse", 60, 100, 70, 60.0, z_lo=4.5, z_hi=30.0, sigma_px_med=2.0, sigma_px_logstd=0.8, seed=8)


def pairs_name(extra, nolast):
    return f"bwd_batch_pairs<EXTRA={int(extra)},NOLAST={int(nolast)}>"


def batch_name(extra, sep, nolast, gacc):
    return f"bwd_batch<EXTRA={int(extra)},SEP={int(sep)},NOLAST={int(nolast)},GACC={int(gacc)}>"


NOSEP = batch_name(1, 0, 0, 1)
PAIRS_LOOPS = tuple(pairs_name(e, n) for e in (0, 1) for n in (0, 1))
SEP_LOOPS = tuple(batch_name(e, 1, n, g) for e in (0, 1) for n in (0, 1) for g in (0, 1))
ALL_LOOPS = PAIRS_LOOPS + SEP_LOOPS + (NOSEP,)                                                   # the 13 instantiations
LOOPS_PAIRS_ON = PAIRS_LOOPS + tuple(batch_name(e, 1, n, 1) for e in (0, 1) for n in (0, 1)) + (NOSEP,)     # what composite_bwd_pairs = 1 reaches
LOOPS_PAIRS_OFF = SEP_LOOPS + (NOSEP,)                                                                     # ... and = 0
CLASSES = tuple((s, e, g) for s in (0, 1) for e in (0, 1) for g in (0, 1))                       # (sep, use_extra, use_gacc)


def loop_of(sep, extra, gacc, nolast, pairs):
    """The instantiation the kernel runs for a batch of a quadrant of class (sep, extra, gacc)."""
    if pairs and sep and not gacc:
        return pairs_name(extra, nolast)
    if not sep:
        return NOSEP
    return batch_name(extra, 1, nolast, gacc)


# ------------------------------------------------------------------ support layouts
def _random(H, W, seed):
    """O(1) random offsets and upstream gradients, dense: colour ~ N(0,1), depth ~ 0.1 N(0,1), flow = (U, |N|, U), acc ~ N(0,1)."""
    g = torch.Generator().manual_seed(4000 + seed)
    off = torch.rand(H, W, 2, generator=g) - 0.5
    gc = torch.randn(3, H, W, generator=g)
    gd = 0.1 * torch.randn(1, H, W, generator=g)
    gf = torch.stack([torch.rand(H, W, generator=g), torch.randn(H, W, generator=g).abs(), torch.rand(H, W, generator=g)], 0)
    ga = torch.randn(1, H, W, generator=g)
    return off, gc, gd, gf, ga


def _xy(H, W):
    y, x = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return x, y


def mixed(H, W, seed=0):
    """Neighbouring quadrants in all eight (sep, extra, gacc) classes: offsets for x >= 48, depth and flow gradients for y >= 32,
    dL_dacc on the quadrants of one colour of a checkerboard.  -> (subpixel_offset [H,W,2], [colour, depth, flow, acc])."""
    off, gc, gd, gf, ga = _random(H, W, seed)
    x, y = _xy(H, W)
    low = (y >= 32).float()
    return off * (x >= 48).float()[..., None], [gc, gd * low[None], gf * low[None], ga * (((x // 8 + y // 8) % 2) == 0).float()[None]]


def image_only(H, W, seed=0, null=False):
    """The training loop's case: a colour gradient alone, the others as zero tensors or (null) absent.  No offsets."""
    _, gc, gd, gf, ga = _random(H, W, seed)
    return None, [gc] + ([None, None, None] if null else [torch.zeros_like(gd), torch.zeros_like(gf), torch.zeros_like(ga)])


def dense(H, W, seed=0):
    """All four gradients on every pixel, no offsets ("gated" on SPARSE: they meet pixels with acc == 0)."""
    _, gc, gd, gf, ga = _random(H, W, seed)
    return None, [gc, gd, gf, ga]


# single_pixel: the pixel that alone carries a depth gradient / dL_dacc / an offset, and the origin of the quadrant whose every pixel carries
# an offset too small to move it.  Four different quadrants, none at x = 0 or y = 0 (0 + 1e-9 != 0).
SINGLE_DEPTH_PIXEL, SINGLE_ACC_PIXEL, SINGLE_OFFSET_PIXEL, SINGLE_TINY_ORIGIN = (13, 10), (35, 21), (61, 44), (80, 48)      # (x, y)
SINGLE_TINY = 1e-9
SINGLE_EXPECT = {"depth": (1, 1, 0), "acc": (1, 0, 1), "offset": (0, 0, 0), "tiny": (1, 0, 0)}


def single_pixel(H, W, seed=0):
    """Classes decided by one pixel: colour everywhere; SINGLE_EXPECT says which class each special quadrant must take."""
    off, gc, gd, gf, ga = _random(H, W, seed)
    x, y = _xy(H, W)
    at = lambda p: ((x == p[0]) & (y == p[1])).float()
    tx, ty = SINGLE_TINY_ORIGIN
    tiny = ((x >= tx) & (x < tx + 8) & (y >= ty) & (y < ty + 8)).float()
    sub = off * at(SINGLE_OFFSET_PIXEL)[..., None] + SINGLE_TINY * tiny[..., None]
    return sub, [gc, gd * at(SINGLE_DEPTH_PIXEL)[None], torch.zeros_like(gf), ga * at(SINGLE_ACC_PIXEL)[None]]


def single_quadrants(W):
    """name -> flat quadrant index (4 * tile + quadrant) of single_pixel's four special quadrants."""
    pts = {"depth": SINGLE_DEPTH_PIXEL, "acc": SINGLE_ACC_PIXEL, "offset": SINGLE_OFFSET_PIXEL, "tiny": SINGLE_TINY_ORIGIN}
    return {k: quadrant_of(px, py, W) for k, (px, py) in pts.items()}


def quadrant_of(px, py, W):
    gx = (W + TILE - 1) // TILE
    return 4 * ((py // TILE) * gx + px // TILE) + 2 * ((py % TILE) // QUAD) + (px % TILE) // QUAD


def walked_lower_bound(o, offsets=None):
    """Per quadrant, the entries in front of its deepest contributor that reach alpha >= 1/255 on one of its pixels (float64 on the
    oracle's forward `o`): these survive the forward's conservative quadrant cull, so the backward walks at least as many."""
    W, H = o["W"], o["H"]
    gx = (W + TILE - 1) // TILE
    nc = _quads(np.asarray(o["n_contrib"]).reshape(H, W).astype(np.int64), W, H, 0)
    co, m2 = o["conic_opacity"].astype(np.float64), o["means2D"].astype(np.float64)
    pl, rg = o["point_list"].astype(np.int64), o["ranges"].astype(np.int64)
    off = np.zeros((H, W, 2)) if offsets is None else _np(offsets).reshape(H, W, 2).astype(np.float64)
    out = np.zeros(nc.shape[0], np.int64)
    for i in np.flatnonzero(nc.max(1) > 0):
        t, q = divmod(int(i), 4)
        ox, oy = (t % gx) * TILE + (q & 1) * QUAD, (t // gx) * TILE + (q >> 1) * QUAD
        ids = pl[rg[t, 0]: rg[t, 0] + nc[i].max()]
        py, px = np.meshgrid(np.arange(oy, min(oy + QUAD, H)), np.arange(ox, min(ox + QUAD, W)), indexing="ij")
        dx = m2[ids, 0][:, None] - (px + off[py, px, 0]).reshape(-1)[None]
        dy = m2[ids, 1][:, None] - (py + off[py, px, 1]).reshape(-1)[None]
        A, B, C, w = (co[ids, k][:, None] for k in range(4))
        power = -0.5 * (A * dx * dx + C * dy * dy) - B * dx * dy
        out[i] = int(((power <= 0) & (np.minimum(0.99, w * np.exp(power)) >= 1.0 / 255.0)).any(1).sum())
    return out


def mask_fragile(grads, fragile, frag_eps):
    """What _fwd_bwd (tests/test_gpu_parity.py) passes on: the gradients with the fragile pixels zeroed; absent ones stay absent."""
    solid = torch.from_numpy(np.asarray(fragile) > frag_eps)
    return [None if x is None else x * solid[None] for x in grads]


# ------------------------------------------------------------------ census
def _np(x):
    return None if x is None else (x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x))


def _quads(a, W, H, fill):
    """[H,W] -> [4 T, 64]: row 4 * tile + quadrant, the kernel's numbering (quadrant = 2 * lower + right); `fill` outside the image."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    full = np.full((gy * TILE, gx * TILE), fill, dtype=a.dtype)
    full[:H, :W] = a
    return full.reshape(gy, 2, QUAD, gx, 2, QUAD).transpose(0, 3, 1, 4, 2, 5).reshape(gy * gx * 4, QUAD * QUAD)


def quadrant_facts(n_contrib, acc, offsets, grads, W, H):
    """Per quadrant (flat index 4 * tile + quadrant): inside (has a pixel in the image), sep, extra, gacc (bool), deepest, min_last.
    grads: [colour, depth [1,H,W], flow [3,H,W], acc [1,H,W]], the last three possibly None (absent = zero)."""
    nc = _np(n_contrib).reshape(H, W).astype(np.int64)
    a = _np(acc).reshape(H, W).astype(np.float32)
    lit = a > 0
    inside = _quads(np.ones((H, W), bool), W, H, False)
    ncq = _quads(nc, W, H, 0)
    moved = np.zeros((H, W), bool)
    if offsets is not None:
        off = _np(offsets).reshape(H, W, 2).astype(np.float32)
        px, py = np.arange(W, dtype=np.float32)[None, :], np.arange(H, dtype=np.float32)[:, None]
        moved = ((px + off[..., 0]).astype(np.float32) != px) | ((py + off[..., 1]).astype(np.float32) != py)
    _, gd, gf, ga = [_np(x) for x in grads]
    extra = np.zeros((H, W), bool)
    if gd is not None:
        extra |= gd.reshape(H, W) != 0
    if gf is not None:
        extra |= (gf.reshape(3, H, W) != 0).any(0) & lit
    gacc = (ga.reshape(H, W) != 0) & lit if ga is not None else np.zeros((H, W), bool)
    return dict(inside=inside.any(1), sep=~_quads(moved, W, H, False).any(1), extra=_quads(extra, W, H, False).any(1),
                gacc=_quads(gacc, W, H, False).any(1), deepest=ncq.max(1), min_last=ncq.min(1))


def census(n_contrib, acc, ranges, qlist, qcount, offsets, grads, W, H, pairs):
    """Which loops the compositing backward runs on this frame, from the forward's state and what the backward is given.
    Returns counts (plain ints: the dict goes into the parity report) and, under "per_quadrant", the arrays of quadrant_facts
    plus `valid` (entries walked) and `code` (sep + 2 extra + 4 gacc)."""
    f = quadrant_facts(n_contrib, acc, offsets, grads, W, H)
    ranges = _np(ranges).astype(np.int64).reshape(-1, 2)
    ql = _np(qlist).astype(np.int64).reshape(-1) & 0xFFFFFFFF
    qc = _np(qcount).astype(np.int64).reshape(-1) & 0xFFFFFFFF
    Q = f["deepest"].shape[0]
    assert Q == 4 * ranges.shape[0] == qc.shape[0], (Q, ranges.shape, qc.shape)
    loops = {k: 0 for k in ALL_LOOPS}
    tails = {n: 0 for n in range(1, BATCH)}
    wraps = {c: 0 for c in CLASSES}
    quads = {c: 0 for c in CLASSES}
    valid_q = np.zeros(Q, np.int64)
    early = outside = batches = entries = 0
    for i in range(Q):
        if not f["inside"][i]:
            outside += 1
            continue
        deepest, min_last = int(f["deepest"][i]), int(f["min_last"][i])
        if deepest == 0:
            early += 1
            continue
        t, q = divmod(i, 4)
        r0, r1 = ranges[t]
        ent = ql[4 * r0 + q * (r1 - r0): 4 * r0 + q * (r1 - r0) + qc[i]]
        walk = ent[ent < deepest][::-1]                      # back to front
        cls = (int(f["sep"][i]), int(f["extra"][i]), int(f["gacc"][i]))
        quads[cls] += 1
        valid_q[i] = len(walk)
        wraps[cls] += len(walk) > RING
        for b in range(0, len(walk), BATCH):
            nb = min(BATCH, len(walk) - b)
            nolast = nb == BATCH and int(walk[b]) < min_last
            loops[loop_of(*cls, nolast, pairs)] += 1
            if nb < BATCH:
                tails[nb] += 1
            batches += 1
            entries += nb
    name = lambda c: f"sep={c[0]},extra={c[1]},gacc={c[2]}"
    per = dict(f, valid=valid_q, code=f["sep"].astype(np.int64) + 2 * f["extra"] + 4 * f["gacc"])
    return dict(pairs=int(bool(pairs)), loops=loops, tail_sizes=tails, quadrants={name(c): int(n) for c, n in quads.items()},
                ring_wraps={name(c): int(n) for c, n in wraps.items()}, ring_wrap_quadrants=int(sum(wraps.values())),
                early_return=int(early), outside=int(outside), batches=int(batches), entries=int(entries), per_quadrant=per)


def class_name(c):
    return f"sep={int(c[0])},extra={int(c[1])},gacc={int(c[2])}"


def class_at(facts, i):
    return (int(facts["sep"][i]), int(facts["extra"][i]), int(facts["gacc"][i]))


def report(c, tag):
    """The census without its arrays, as an entry of helpers.REPORT."""
    return dict(kind="composite_census", tag=tag, **{k: v for k, v in c.items() if k != "per_quadrant"})
