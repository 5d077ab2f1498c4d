"""Designed scenes, a host restatement of the binning and a host census of the tile sorts' instantiations and per-block paths, shared by
tests/test_cpu_binning_cases.py (the restatement equals the CPU oracle's binning on every case; the cases reach every cell of the
census) and tests/test_gpu_binning_edges.py (every kernel chain against the restatement, the census against the frame).

The binning is ex4dgs_amd/csrc/ex4d_rowsort.hip (the row-segment sort: rows_seg_hist_kernel, rows_scan_kernel,
rows_seg_scatter_kernel<NRP, CAP>) and ex4dgs_amd/csrc/ex4d_binning.hip (the pair sorts: rs_histogram_kernel / rs_scatter_kernel in
its modes with the DigitBits rule, ts_histogram_kernel, ts_locate_block; pass B; duplicate_kernel; scan_tiles_local_kernel).  The census restates, from the
host code (ex4d_tile_sort_rows, ex4d_tile_sort_msd, ex4d_tile_sort_pass_b, ex4d_radix_sort_pairs, forward_impl) and from the kernels,
WHICH template instantiation a frame launches and WHICH uniform branch every workgroup takes -- as names, so that a cell nobody
reaches can be printed.

A case is a list of (pixel centre x, pixel centre y, radius, visible) in the depth order it is designed for.  The camera looks down
+z with an identity view and a focal length of 16 image sides, the scales are isotropic: a Gaussian's centre and its radius
ceil(3 sqrt(lambda)) -- hence its tile rect -- are what the list says (the CPU test checks the rects that matter through the census).
The ids are a random permutation of the designed order, and the depths tie in pairs (ties resolve in ascending id)."""
import functools
from collections import namedtuple

import numpy as np
import torch

from ex4dgs_amd.scene import SceneConfig
from tests import helpers as h
from tests.test_cpu_buffer_contract import path_signature, tile_bits
from tests.test_gpu_buffer_contract import BASE_OPTIONS

TILE = 16
ROWA_GAUSS, ROWA_HINTS = 256, 1024            # ex4d_rowsort.hip
RS_CHUNK, SCAN_CHUNK = 4096, 2048             # ex4d_internal.h
MIN_DEPTH, MAX_DEPTH = 4.0, 300.0             # SceneConfig's defaults: 26 key bits, the MSD depth sort applies


# ------------------------------------------------------------------------------------------------ designed scenes
def dot(tx, ty):
    """a 1 x 1 rect: the smallest radius (2) in the centre of tile (tx, ty)"""
    return (16.0 * tx + 8.0, 16.0 * ty + 8.0, 2, True)


def square(px, ty0, k):
    """k rows [ty0, ty0 + k) around the pixel column px, and the k columns around it that the image has: the rect of radius 8k - 6
    centred on a tile corner (k even) or centre (k odd) keeps 6 px of margin to the next tile on either side"""
    return (float(px), 16.0 * ty0 + 8.0 * k, 8 * k - 6, True)


def full(W, H):
    """a rect over the whole image"""
    return (W / 2.0, H / 2.0, max(W, H) + 32, True)


HIDDEN = (8.0, 8.0, 2, False)                 # in front of min_depth: invisible, rect 0, behind every visible Gaussian in the depth order

Case = namedtuple("Case", "name W H specs why")


def _edge(name, gy, P, seed, why):
    """48 px wide, gy tile rows: dots and 2 x 2 squares all over, and one rect whose last row is gy - 1"""
    rng = np.random.default_rng(seed)
    W, H = 48, 16 * gy
    specs = [square(24, gy - 4, 4)]
    while len(specs) < P:
        tx, ty = int(rng.integers(0, 3)), int(rng.integers(0, gy))
        specs.append(square(16, int(rng.integers(0, gy - 1)), 2) if len(specs) % 7 == 3 else dot(tx, ty))
    order = rng.permutation(P)
    return Case(name, W, H, [specs[i] for i in order], why)


def _cap(name, gy, k, hidden, why):
    """16 px wide (one tile column): block 0 = 256 rects k rows high (256 k segments: the stage exactly full for k = CAP / 256),
    block 1 = 255 of them and one of k + 1 rows (one segment too many), block 2 = 256 dots, then `hidden` invisible Gaussians"""
    rng = np.random.default_rng(gy)
    tall = lambda kk: square(8, int(rng.integers(0, gy - kk + 1)), kk)
    specs = [tall(k) for _ in range(256)] + [tall(k) for _ in range(255)] + [tall(k + 1)] + [dot(0, int(rng.integers(0, gy))) for _ in range(256)]
    return Case(name, 16, 16 * gy, specs + [HIDDEN] * hidden, why)


def _gaps():
    rng = np.random.default_rng(12)
    rows = (30, 31, 60, 61)
    return Case("gaps", 48, 1600, [dot(int(rng.integers(0, 3)), rows[int(rng.integers(0, 4))]) for _ in range(300)],
                "tile rows / buckets without instances in front, in runs in the middle and at the end (300 tiles, 9 tile bits: buckets of 32 tiles)")


def _strip():
    rng = np.random.default_rng(13)
    return Case("strip", 1600, 16, [(float(rng.integers(0, 1600)), 8.0, int(rng.integers(2, 200)), True) for _ in range(500)],
                "one tile row, 100 columns: rects clipped to one row, pass B with 7-bit columns")


def _scatter(name, W, H, P, seed, why, last_rows=0):
    """dots and squares of 2..5 tiles all over a W x H image; last_rows > 0: some dots in the last tile rows"""
    rng = np.random.default_rng(seed)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    specs = []
    for i in range(P):
        if i < last_rows:
            specs.append(dot(int(rng.integers(0, gx)), gy - 1 - (i % 3)))
        elif i % 5 == 0:
            k = int(rng.integers(2, 6))
            specs.append(square(int(rng.integers(8, W - 8)), int(rng.integers(0, gy - k + 1)), k))
        else:
            specs.append(dot(int(rng.integers(0, gx)), int(rng.integers(0, gy))))
    order = rng.permutation(P)
    return Case(name, W, H, [specs[i] for i in order], why)


@functools.lru_cache(maxsize=None)
def cases():
    c = [
        _edge("gy64", 64, 2048, 64, "64 tile rows: the last row of NRP = 64; P = SCAN_CHUNK; 192 tiles: the radix pair sort in one 8-bit pass"),
        _edge("gy65", 65, 2049, 65, "65 tile rows: the first of NRP = 128; P = SCAN_CHUNK + 1"),
        _edge("gy128", 128, 4097, 128, "128 tile rows: the last of NRP = 128; P = 2 SCAN_CHUNK + 1; 9 tile bits"),
        _edge("gy129", 129, 255, 129, "129 tile rows: the first of NRP = 256; P = 255: fewer than 4096 instances through the MSD pair sort"),
        _edge("gy255", 255, 257, 255, "255 tile rows: the last the row-segment sort takes; P = 257"),
        _cap("cap1024", 40, 4, 300, "blocks of exactly 1024 and of 1025 segments under CAP = 1024, blocks without segments"),
        _cap("cap2048", 100, 8, 0, "blocks of exactly 2048 and of 2049 segments under CAP = 2048 (2 S > 7 P); three blocks of pass A'"),
        Case("sh9", 4080, 128, [full(4080, 128)] * 256, "256 full-width Gaussians in one block: 2048 segments of 255 words, hint shift 9, "
             "tile rows of 65280 instances (16 blocks of pass B), 8-bit columns"),
        Case("bucket4096", 512, 192, [full(512, 192)] * 64 + [dot(5, 1)] + [full(512, 192)] * 64,
             "tile rows = buckets of 32 tiles with exactly 4096 instances and one with 4097; R = 12 x 4096 + 1"),
        Case("R8192", 512, 256, [full(512, 256)] * 16, "R = 2 x 4096 exactly, P = 16"),
        _gaps(),
        _strip(),
        _scatter("bits12", 320, 1760, 1000, 14, "2200 tiles: 12 tile bits, 6-bit high digit"),
        _scatter("bits14", 528, 4000, 1000, 15, "8250 tiles: 14 tile bits, 7-bit high and low digits"),
        _scatter("bits16", 32, 16 * 32768, 600, 16, "65536 tiles: 16 tile bits, 8-bit digits, 256 buckets the last of which holds instances; "
                 "8-byte rects; plain division in the duplication", last_rows=40),
        _scatter("bits17", 32, 16 * 32769, 600, 17, "65538 tiles: 17 tile bits, the radix pair sort in two passes (9 + 8 bits)", last_rows=40),
        Case("radix8", 256, 256, [full(256, 256)] * 20 + [dot(i % 16, i // 16) for i in range(100)] + [full(256, 256)] * 20,
             "256 tiles: the radix pair sort over more than one block of instances"),
    ]
    assert len({x.name for x in c}) == len(c)
    return tuple(c)


def case(name):
    return next(c for c in cases() if c.name == name)


CASE_NAMES = tuple(c.name for c in cases())
# the multi-block cases of the one-instance-short test: between them they go through all three tile sorts
SHORT_CASES = (("bucket4096", "rows"), ("bucket4096", "msd pair"), ("radix8", "radix pair"))


def build_scene(label, W, H, specs, z, ids, min_depth, max_depth, seed):
    """(inputs, settings) of designed Gaussians: helpers.scene_inputs on a literal SceneConfig with these two planes, then means3D /
    scales / opacities / rotations overwritten.  specs[i] = (pixel centre x, pixel centre y, radius, visible) of the i-th designed
    Gaussian, z[i] its depth (a float32 value; the view is the identity, so it is p_view.z exactly), ids[i] its id."""
    P = len(specs)
    focal = 16.0 * max(W, H)
    cfg = SceneConfig(label, P, W, H, focal, seed=seed, min_depth=min_depth, max_depth=max_depth)
    ins, st = h.scene_inputs(cfg, P=P)
    px, py, r, vis = (np.array([s[k] for s in specs], np.float64) for k in range(4))
    z = np.asarray(z, np.float32).astype(np.float64)
    # radius = ceil(3 sqrt(lambda)), lambda = (focal s / z)^2 + kernel_size + sqrt(0.1): aim at r - 0.5 (the smallest radius is 2)
    var = np.maximum(((r - 0.5) / 3.0) ** 2 - (0.1 + 0.1 ** 0.5), 0.01)
    m = np.stack([(px + 0.5 - W / 2.0) * z / focal, (py + 0.5 - H / 2.0) * z / focal, z], -1)
    # (|z|: the same value for the depths in front of the camera; tests/depth_sort_cases.py has rows with a depth below zero under a
    # negative near plane, whose scales must stay positive)
    s = np.repeat((np.abs(z) / focal * np.sqrt(var))[:, None], 3, 1)
    op = np.where(r > 100, 1.0, 0.5)[:, None]          # the large ones opaque: the compositing behind them ends early
    for k, v in (("means3D", m), ("scales", s), ("opacities", op)):
        t = torch.zeros(ins[k].shape, dtype=torch.float32)
        t[torch.from_numpy(ids)] = torch.from_numpy(v.astype(np.float32))
        ins[k] = t.contiguous()
    # (the generator's quaternions are not unit: a rotation matrix built from one scales the covariance; the identity keeps it isotropic)
    ins["rotations"] = torch.tensor([1.0, 0.0, 0.0, 0.0]).repeat(P, 1).contiguous()
    return ins, st


@functools.lru_cache(maxsize=4)
def scene(name):
    """(inputs, settings) of a case: build_scene with the depths 5 + 0.01 (i // 2) (hidden: 1) between SceneConfig's default planes"""
    c = case(name)
    P = len(c.specs)
    ids = np.random.default_rng(7000 + CASE_NAMES.index(name)).permutation(P)          # the id of the i-th designed Gaussian
    vis = np.array([s[3] for s in c.specs], np.float64)
    z = np.where(vis > 0, 5.0 + 0.01 * (np.arange(P) // 2), 1.0).astype(np.float32)
    return build_scene(f"binning case {name}", c.W, c.H, c.specs, z, ids, MIN_DEPTH, MAX_DEPTH, 900 + CASE_NAMES.index(name))


# ------------------------------------------------------------------------------------------------ the restatement
def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def rects_of(radii, means2D, W, H):
    """getRect (CR/auxiliary.h:46-56) in float32, truncation toward zero, clamped to the grid -> int64 [P,4] = (x0, y0, w, h); zeros for
    radii == 0"""
    radii, m = _np(radii).astype(np.int64), _np(means2D).astype(np.float32).reshape(-1, 2)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    vis = radii > 0
    f = np.float32
    r = np.where(vis, radii, 0).astype(f)
    out = np.zeros((radii.shape[0], 4), np.int64)
    for axis, g in ((0, gx), (1, gy)):
        p = np.where(vis, m[:, axis], f(0))
        lo = np.trunc((p - r) / f(TILE)).astype(np.int64)
        hi = np.trunc((((p + r) + f(TILE)) - f(1)) / f(TILE)).astype(np.int64)
        lo, hi = np.clip(lo, 0, g), np.clip(hi, 0, g)
        out[:, axis], out[:, 2 + axis] = lo, hi - lo
    out[~vis] = 0
    return out


def host_depth_order(radii, depths):
    """tests/test_gpu_round5.py: _host_depth_order, in numpy: stable ascending sort of the visible depths' bit patterns as unsigned
    32-bit words, ties in ascending id, invisible Gaussians behind in id order"""
    radii = _np(radii)
    bits = np.ascontiguousarray(_np(depths), np.float32).view(np.uint32).astype(np.int64)
    return np.argsort(np.where(radii > 0, bits, 1 << 40), kind="stable").astype(np.int64)


def host_binning(radii, means2D, depths, W, H, capacity=None, form="pair"):
    """The binning, plainly: every Gaussian's instances (its rect's tiles, row by row) in depth order, stably sorted by tile id.
    point_list = the instances of tile 0, then tile 1, ...; ranges[t] = (start, end), (0, 0) for a tile without instances.
    capacity (an asynchronous frame whose instance count exceeds it): only the first `capacity` instances of the stream the tile sort
    reads are kept -- form "pair": the duplication's stream (Gaussians in depth order, each rect row by row); form "rows": the
    row-segment partition's (tile row by tile row, inside a row the Gaussians in depth order)."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    rects = rects_of(radii, means2D, W, H)
    order = host_depth_order(radii, depths)
    r = rects[order]
    cnt = r[:, 2] * r[:, 3]
    R, S = int(cnt.sum()), int(r[cnt > 0, 3].sum())
    owner = np.repeat(np.arange(r.shape[0]), cnt)                        # position in the depth order of every instance
    local = np.arange(R) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    w = r[owner, 2]
    row, col = r[owner, 1] + local // np.maximum(w, 1), r[owner, 0] + local % np.maximum(w, 1)
    tile, ids = row * gx + col, order[owner]
    kept = R
    if capacity is not None and capacity < R:
        first = np.argsort(row, kind="stable")[:capacity] if form == "rows" else np.arange(capacity)
        first = np.sort(first)                                            # (back in depth order)
        tile, ids, kept = tile[first], ids[first], int(capacity)
    perm = np.argsort(tile, kind="stable")
    tile_ids, point_list = tile[perm], ids[perm]
    T = gx * gy
    start, end = np.searchsorted(tile_ids, np.arange(T), "left"), np.searchsorted(tile_ids, np.arange(T), "right")
    ranges = np.where((end > start)[:, None], np.stack([start, end], -1), 0)
    return dict(order=order, rects=rects, tiles_touched=rects[:, 2] * rects[:, 3], R=R, S=S, kept=kept, point_list=point_list,
                tile_ids=tile_ids, ranges=ranges)


def oracle_binning(ins, st):
    """The CPU oracle's forward up to the tile ranges (oracle.forward's preprocess and binning stages, the same two calls with the same
    arguments; the compositing, which a 16 Mpx image makes slow, is left out): radii, means2D, depths, tiles_touched, num_rendered,
    point_list, keys_sorted, ranges"""
    import ctypes as C
    from oracle import oracle as o
    L = o.lib()
    f32 = lambda k, d=None: o._np(d.get(k) if d is not None else ins.get(k), np.float32)
    means3D = f32("means3D")
    P, W, H = means3D.shape[0], int(st["image_width"]), int(st["image_height"])
    shs, scales, rotations, opac = f32("shs"), f32("scales"), f32("rotations"), f32("opacities")
    vm, pm, cp = f32("viewmatrix", st), f32("projmatrix", st), f32("campos", st)
    M = shs.shape[1]
    g = dict(radii=np.zeros(P, np.int32), means2D=np.zeros((P, 2), np.float32), depths=np.zeros(P, np.float32), cov3D=np.zeros((P, 6), np.float32),
             rgb=np.zeros((P, 3), np.float32), conic_opacity=np.zeros((P, 4), np.float32), tiles_touched=np.zeros(P, np.uint32),
             clamped=np.zeros((P, 3), np.uint8), point_offsets=np.zeros(P, np.uint32))
    p = o._p
    R = int(L.ex4d_oracle_preprocess(
        C.c_int(P), C.c_int(int(st["sh_degree"])), C.c_int(M), p(means3D), p(scales), C.c_float(st["scale_modifier"]), p(rotations), p(opac), p(shs),
        p(None), p(None), p(vm), p(pm), p(cp), C.c_int(W), C.c_int(H), C.c_float(st["tanfovx"]), C.c_float(st["tanfovy"]), C.c_float(st["kernel_size"]),
        C.c_float(st["min_depth"]), C.c_float(st["max_depth"]), C.c_int(0), p(g["radii"]), p(g["means2D"]), p(g["depths"]), p(g["cov3D"]), p(g["rgb"]),
        p(g["conic_opacity"]), p(g["tiles_touched"]), p(g["clamped"]), p(g["point_offsets"])))
    T = ((W + 15) // 16) * ((H + 15) // 16)
    b = dict(keys_unsorted=np.zeros(R, np.uint64), values_unsorted=np.zeros(R, np.uint32), keys_sorted=np.zeros(R, np.uint64),
             point_list=np.zeros(R, np.uint32), ranges=np.zeros((T, 2), np.uint32))
    L.ex4d_oracle_binning(C.c_int(P), C.c_int(W), C.c_int(H), C.c_int64(R), p(g["radii"]), p(g["means2D"]), p(g["depths"]), p(g["point_offsets"]),
                          p(b["keys_unsorted"]), p(b["values_unsorted"]), p(b["keys_sorted"]), p(b["point_list"]), p(b["ranges"]))
    return dict(P=P, W=W, H=H, num_rendered=R, **g, **b)


@functools.lru_cache(maxsize=2)
def oracle_of(name):
    return oracle_binning(*scene(name))


# ------------------------------------------------------------------------------------------------ frames: option sets and capacities
# tile_sort_rows x depth_sort_msd, and ranking by ballots once per tile-sort chain (rows = 1: the row-segment sort; rows = 0: whichever
# pair sort the image takes); the sorted tile ids are materialised except where the ballots rank
OPTION_SETS = (
    ("rows, LSD", dict(tile_sort_rows=1, depth_sort_msd=0, binning_tile_ids=1)),
    ("rows, MSD", dict(tile_sort_rows=1, depth_sort_msd=2, binning_tile_ids=1)),
    ("pairs, LSD", dict(tile_sort_rows=0, depth_sort_msd=0, binning_tile_ids=1)),
    ("pairs, MSD", dict(tile_sort_rows=0, depth_sort_msd=2, binning_tile_ids=1)),
    ("rows, MSD, ballots", dict(tile_sort_rows=1, depth_sort_msd=2, rank_lds_atomics=0)),
    ("pairs, LSD, ballots", dict(tile_sort_rows=0, depth_sort_msd=0, rank_lds_atomics=0)),
)


def capacities(P, R):
    """None (synchronous), R, R + 1 and the capacities on either side of the row-segment sort's stage choice (cap > 20 P)"""
    caps = [None]
    if R > 0:
        caps += [R, R + 1, max(R, 20 * P + 1)] + ([20 * P] if R <= 20 * P else [])
    return [c for i, c in enumerate(caps) if c not in caps[:i]]


def frames(P, W, H, R):
    """[(label, options over BASE_OPTIONS, capacity)]: every option set x capacity, one frame per distinct kernel chain"""
    out, seen = [], set()
    for label, opts in OPTION_SETS:
        for cap in capacities(P, R):
            full_opts = dict(BASE_OPTIONS, **opts)
            key = (path_signature(P, W, H, MIN_DEPTH, MAX_DEPTH, full_opts, cap is not None), full_opts["rank_lds_atomics"], cap)
            if key not in seen:
                seen.add(key)
                out.append((label + (", synchronous" if cap is None else f", capacity {cap}"), opts, cap))
    return out


# ------------------------------------------------------------------------------------------------ census
def _bucket_cells(prefix, totals):
    """states of pass B's block cutting (ts_block_from_table's table, filled by workgroup 0 of rows_seg_scatter_kernel, and
    ts_locate_block) over the bucket totals"""
    t = np.asarray(totals, np.int64)
    cells = set()
    full = np.flatnonzero(t > 0)
    if full.size == 0:
        return cells
    if full[0] > 0:
        cells.add(prefix + "empty_front")
    if full[-1] < t.size - 1:
        cells.add(prefix + "empty_end")
    if (np.diff(full) >= 3).any():                       # two or more buckets without instances between two with
        cells.add(prefix + "empty_run_middle")
    if (t == RS_CHUNK).any():
        cells.add(prefix + "count4096")
    if (t == RS_CHUNK + 1).any():
        cells.add(prefix + "count4097")
    if (t > 2 * RS_CHUNK).any():
        cells.add(prefix + "blocks_ge3")
    return cells


def _bits_for(n):
    """ex4d_rowsort.hip: bits_for"""
    b = 1
    while (1 << b) < n:
        b += 1
    return b


def hint_shift(nwords):
    """rows_seg_scatter_kernel: the block's words fit ROWA_HINTS buckets of 2^sh words"""
    sh = 3
    while ((nwords - 1) >> sh) >= ROWA_HINTS:
        sh += 1
    return sh


def census(P, W, H, order, rects, options, capacity=None):
    """The cells a frame reaches: P Gaussians, a W x H image, `order` = the depth order (ids), rects [P,4] = (x0, y0, w, h) by id,
    options = every option of BASE_OPTIONS, capacity = that of an asynchronous forward or None.  Returns a set of names out of
    CELLS + the names of UNREACHED."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    T = gx * gy
    tb = tile_bits(T)
    packed, depth, _, tile, fused_scan, _, _ = path_signature(P, W, H, MIN_DEPTH, MAX_DEPTH, options, capacity is not None)
    r = np.asarray(rects, np.int64)[np.asarray(order, np.int64)]
    x0, y0, w, hh = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    cnt = w * hh
    live = cnt > 0
    R, S = int(cnt.sum()), int(hh[live].sum())
    cells = set()
    if R == 0:
        return {"frame.no_instances"}
    n = R                                                   # what the grids are sized for, and what the kernels sort
    if capacity is not None:
        cells.add({R: "cap.R", R + 1: "cap.R_plus_1", R - 1: "cap.R_minus_1"}.get(capacity, "cap.other"))
        n = min(R, capacity)
    if tile == "rows":
        if not packed:
            cells.add("rows.rect8")
        if P > (1 << 24):
            cells.add("rows.P_above_2^24")
        nbA = (P + ROWA_GAUSS - 1) // ROWA_GAUSS
        NRP = 64 if gy <= 64 else (128 if gy <= 128 else 256)
        big = (capacity > 20 * P) if capacity is not None else (2 * S > 7 * P)
        CAP = 2048 if big else 1024
        cells.add(f"rowsA.{NRP}.{CAP}")
        pad = nbA * ROWA_GAUSS - P
        seg = np.pad(np.where(live, hh, 0), (0, pad)).reshape(nbA, ROWA_GAUSS).sum(1)
        words = np.pad(cnt, (0, pad)).reshape(nbA, ROWA_GAUSS).sum(1)
        for total, nw in zip(seg.tolist(), words.tolist()):
            if total == 0:
                cells.add(f"rowsA.block.{CAP}.empty")
            elif total > CAP:
                cells.add(f"rowsA.block.{CAP}.sequential")
                if total == CAP + 1:
                    cells.add(f"rowsA.block.{CAP}.sequential_by1")
            else:
                cells.add(f"rowsA.block.{CAP}.staged" + ("_full" if total == CAP else ""))
                sh = hint_shift(nw)
                cells.add("rowsA.sh3" if sh == 3 else "rowsA.sh_gt3")
                if sh == 9:
                    cells.add("rowsA.sh9")
        if gy in (64, 65, 128, 129, 255) and (y0 + hh)[live].max() == gy:
            cells.add(f"rows.gy{gy}")
        if gx == 255 and ((w == 255) & live).any():
            cells.add("rows.gx255_full_width")
        if P % 256 in (0, 1, 255):
            cells.add(f"rows.P_mod256_{P % 256}")
        if nbA % 4 != 0:
            cells.add("rows.nbA_mod4_ne0")
        if P < 64:
            cells.add("rows.P_lt64")
        bx = _bits_for(gx)
        cells.add("passB.rows.bits." + ("7" if bx == 7 else "8" if bx == 8 else "generic"))
        diff = np.zeros(gy + 1, np.int64)
        np.add.at(diff, y0[live], w[live])
        np.add.at(diff, (y0 + hh)[live], -w[live])
        cells |= _bucket_cells("passB.rows.bucket.", np.cumsum(diff)[:gy])
        return cells
    # ---- the pair sorts: tile scan (its own kernel, or fused into the depth sort's bucket kernel), duplication, sort
    for p_edge in (SCAN_CHUNK, SCAN_CHUNK + 1, 2 * SCAN_CHUNK + 1):
        if P == p_edge:
            cells.add(f"dup.P{p_edge}")
    if (cnt >= 129).any():
        cells.add("dup.ge129_instances")
    waves = np.pad(cnt, (0, (-P) % 64)).reshape(-1, 64)
    if (waves.sum(1) == 0).any():
        cells.add("dup.wave_without_instance")
    if ((w == 1) & live).any():
        cells.add("dup.w1")
    cells.add("dup.offsets.bucket" if fused_scan else "dup.offsets.plain")
    cells.add("dup.division.plain" if T > 65535 else "dup.division.mulhi")
    if tile == "msd pair":
        low = (tb + 1) // 2
        high = tb - low
        cells.add("pairA.high." + (str(high) if high in (6, 7, 8) else "generic"))
        cells.add("passB.pair.bits." + (str(low) if low in (7, 8) else "generic"))
        if n % RS_CHUNK in (0, 1):
            cells.add(f"pairA.R_mod4096_{n % RS_CHUNK}")
        if n < RS_CHUNK:
            cells.add("pairA.R_lt4096")
        d2 = np.zeros((gy + 1, gx + 1), np.int64)
        for ys, sy in ((y0, 1), (y0 + hh, -1)):
            for xs, sx in ((x0, 1), (x0 + w, -1)):
                np.add.at(d2, (ys[live], xs[live]), sy * sx)
        per_tile = d2.cumsum(0).cumsum(1)[:gy, :gx].reshape(-1)
        totals = np.bincount(np.arange(T) >> low, weights=per_tile, minlength=1 << high).astype(np.int64)
        cells |= _bucket_cells("passB.pair.bucket.", totals)
        if high == 8 and totals[255] > 0:
            cells.add("passB.pair.nbuckets256_last_nonempty")
    else:
        if 9 <= tb <= 16:
            cells.add("radix.tile_bits_9_16")
        if n > (2 << 20):
            cells.add("radix.items16")
        cells.add("radix.two_pass_17bits" if tb == 17 else ("radix.one_pass.nbits8" if tb == 8 else "radix.one_pass.generic") if tb <= 8 else "radix.other")
    return cells


_BUCKET = ("empty_front", "empty_run_middle", "empty_end", "count4096", "count4097", "blocks_ge3")
CELLS = tuple(
    [f"rowsA.{nrp}.{cap}" for nrp in (64, 128, 256) for cap in (1024, 2048)]
    + [f"rowsA.block.{cap}.{k}" for cap in (1024, 2048) for k in ("empty", "staged", "staged_full", "sequential", "sequential_by1")]
    + ["rowsA.sh3", "rowsA.sh_gt3", "rowsA.sh9"]
    + [f"rows.gy{g}" for g in (64, 65, 128, 129, 255)] + ["rows.gx255_full_width"]
    + ["rows.P_mod256_0", "rows.P_mod256_1", "rows.P_mod256_255", "rows.nbA_mod4_ne0", "rows.P_lt64"]
    + [f"passB.rows.bits.{b}" for b in ("generic", "7", "8")] + [f"passB.rows.bucket.{k}" for k in _BUCKET]
    + [f"passB.pair.bits.{b}" for b in ("generic", "7", "8")] + [f"passB.pair.bucket.{k}" for k in _BUCKET] + ["passB.pair.nbuckets256_last_nonempty"]
    + [f"pairA.high.{b}" for b in ("generic", "6", "7", "8")] + ["pairA.R_mod4096_0", "pairA.R_mod4096_1", "pairA.R_lt4096"]
    + ["radix.one_pass.nbits8", "radix.one_pass.generic", "radix.two_pass_17bits"]
    + ["dup.P2048", "dup.P2049", "dup.P4097", "dup.ge129_instances", "dup.wave_without_instance", "dup.w1", "dup.offsets.plain", "dup.offsets.bucket",
       "dup.division.mulhi", "dup.division.plain"]
    + ["cap.R", "cap.R_plus_1", "cap.other"])
# cap.R_minus_1 is the one-instance-short test's (tests/test_gpu_binning_edges.py), outside the frames of the census
UNREACHED = (
    ("radix.tile_bits_9_16", "the radix pair sort at 9..16 tile bits: the MSD pair sort declines only when P > 2^(32 - low_bits) >= 2^24 Gaussians"),
    ("radix.items16", "the radix sort's 4096-item chunks (rs_items_for): more than 2^21 instances"),
    ("radix.other", "tile bits outside 1..8 and 17 behind the radix pair sort: 18 and more bits need more than 131072 tiles (33 Mpx)"),
    ("rows.rect8", "rect_at's 8-byte form: the row-segment sort applies to at most 255 x 255 tiles, where forward_impl always hands it the packed "
                   "rects (of the MSD depth sort, or gathered by the LSD sort's last pass)"),
    ("rows.P_above_2^24", "more than 2^24 Gaussians"),
    ("frame.no_instances", "a frame without instances launches no tile sort; tests/test_gpu_buffer_contract.py has it (\"nothing visible\")"),
)


def promised(name):
    """{frame label: cells} of a case, from the CPU oracle's depth order and rects: what the CPU test shows to cover CELLS and the GPU
    test finds again in the frame's own arrays"""
    o = oracle_of(name)
    hb = host_binning(o["radii"], o["means2D"], o["depths"], o["W"], o["H"])
    return {label: census(o["P"], o["W"], o["H"], hb["order"], hb["rects"], dict(BASE_OPTIONS, **opts), cap)
            for label, opts, cap in frames(o["P"], o["W"], o["H"], hb["R"])}


# ------------------------------------------------------------------------------------------------ the write-out's search, restated
def writeout_search(widths, CAP):
    """rows_seg_scatter_kernel's write-out on a block whose staged segments have these widths (1..255 words each, at most CAP of them):
    winc, sh, the hint table as the kernel's loop fills it, the halving steps for every word q of the block.
    Returns (segment found per word, largest index of winc the search reads, sh, hint)."""
    wv = np.asarray(widths, np.int64)
    total = wv.size
    assert 0 < total <= CAP and wv.min() >= 1 and wv.max() <= 255
    winc = np.full(CAP + 256, 0xFFFFFFFF, np.int64)
    run = np.cumsum(wv) - wv
    winc[:total] = run
    nwords = int(wv.sum())
    sh = hint_shift(nwords)
    first, last = (run + (1 << sh) - 1) >> sh, (run + wv - 1) >> sh          # hint[bkt] = p for bkt in [first, last]
    k = np.maximum(last - first + 1, 0)
    bkt = np.repeat(first, k) + (np.arange(int(k.sum())) - np.repeat(np.cumsum(k) - k, k))
    hint = np.full(ROWA_HINTS, -1, np.int64)
    assert bkt.size == np.unique(bkt).size and bkt.max() < ROWA_HINTS, "a hint entry with two writers, or one outside the table"
    hint[bkt] = np.repeat(np.arange(total), k)
    q = np.arange(nwords, dtype=np.int64)
    p = hint[q >> sh]
    assert (p >= 0).all(), "a word whose hint entry nobody wrote"
    top, step = 0, 1 << (sh - 1)
    while step > 0:
        top = max(top, int((p + step).max()))
        p = p + step * (winc[np.minimum(p + step, CAP + 255)] <= q)
        step >>= 1
    return p, top, sh, hint
