"""Designed frames, a host restatement and a host census of the depth sorts, shared by tests/test_cpu_depth_sort_cases.py (every
frame realises its plan on the CPU oracle; the frames reach every cell of the census the host rules make reachable) and
tests/test_gpu_depth_sort_edges.py (every kernel chain against the restatement, the census against the frame).

The depth sort is either the LSD radix sort (ex4dgs_amd/csrc/ex4d_binning.hip: ex4d_radix_sort_pairs, driven from forward_impl in
ex4d_api.hip) or the MSD-first sort (rs_histogram_kernel and rs_scatter_kernel mode 3 with the DigitRange rule,
depth_local_sort_kernel<256 | 512>).  Which
of their paths a frame takes depends on the two depth planes (the key is bits(p_view.z) - bits(min_depth); its width follows from the
planes alone) and on the keys the frame occupies (the MSD sort cuts its top digit from [kmin, kmax]; what is left, `rem` bits, is
sorted inside a bucket).  A frame here is a pair of planes and a list of keys in designed order: key k in [1, invisible - 1] is the
float32 depth whose bit pattern is bits(min_depth) + k, -1 a Gaussian hidden in front of the near plane.  The camera is that of
tests/binning_cases.py (identity view, focal length of 16 image sides), so p_view.z is the third coordinate of means3D exactly.

The restatement: the depth order is a stable ascending sort of the visible depths' bit patterns as unsigned 32-bit words, ties in
ascending id, the invisible Gaussians behind in id order (binning_cases.host_depth_order); everything behind it is
binning_cases.host_binning.

The census names the conditions the host code and the kernels branch on -- restated from those conditions, as names, so that a cell
nobody reaches can be printed."""
import functools
from collections import namedtuple

import numpy as np

from tests import binning_cases as bc
from tests.test_cpu_buffer_contract import depth_sort_msd_applies, depth_sort_msd_bits, float_bits, key_bits, path_signature
from tests.test_gpu_buffer_contract import BASE_OPTIONS

DLS_ITEMS = 16                                # ex4d_binning.hip: items per thread of the bucket kernel -> capacity = threads x 16
IDX_BITS = {256: 12, 512: 13}                 # DlsLds<THREADS>::IDX_BITS: the arrival index under the key bits of the LDS word
RS_SMALL_ITEMS = 8                            # items per thread of the partition and of the LSD sort up to 2 M Gaussians
PARTITION_BLOCK = RS_SMALL_ITEMS * 256        # 2048 ids per workgroup of the partition / of an LSD pass
RANGE_PAIR, RANGE_TRIP = 256, 8 * 256         # one (max key, max ~key) pair per 256 Gaussians, 2048 pairs per trip of dls_reduce_ranges
MSD_BITS_COUNT, THREADS_COUNT = 1300000, 1200000      # 9-bit digit up to 1.3 M Gaussians; 512 threads beyond 1.2 M under the 10-bit digit
LSD_MAX_DIGIT = 9                             # rs_max_bits_for(n <= 2 M)


def f32(bits):
    """the float32 with this bit pattern, as a python float"""
    return float(np.array(int(bits) & 0xFFFFFFFF, np.uint32).view(np.float32))


def planes_of_bits(min_depth, span):
    """(min_depth, max_depth) with bits(max_depth) - bits(min_depth) = span: the invisible key is span + 1"""
    return (float(min_depth), f32(float_bits(min_depth) + span))


def key_frame(min_depth, max_depth):
    """ex4d_api.hip, "depth-sort keys": (key base, invisible key, key bits)"""
    kb = key_bits(min_depth, max_depth)
    if min_depth >= 0.0 and max_depth > min_depth and max_depth < 3.0e38:
        return float_bits(min_depth), float_bits(max_depth) - float_bits(min_depth) + 1, kb
    return 0, 0xFFFFFFFF, kb


PLANES27 = planes_of_bits(2.0 ** -8, (1 << 27) - 2)         # [2^-8, 2^8): invisible key 2^27 - 1, 27 key bits
PLANES28 = planes_of_bits(2.0 ** -12, (1 << 28) - 2)        # [2^-12, 2^20): 28 key bits, the widest the MSD sort takes
PLANES26 = (bc.MIN_DEPTH, bc.MAX_DEPTH)

# keys: int64 in designed order, -1 = hidden; ids: the id of the i-th designed Gaussian (None: a seeded permutation);
# uncertain: designed indices whose visibility the CPU oracle decides (depths below zero under a negative near plane);
# options: "all" / "basic" (the chains only) / "async" (all, and asynchronous frames); specs: the rects of the designed Gaussians
# (None: spec_of's cycle of dot, 2 x 2 square and whole image)
Frame = namedtuple("Frame", "name W H min_depth max_depth keys ids hidden_z uncertain options why specs")


def _frame(name, planes, keys, why, W=64, H=48, ids=None, hidden_z=None, uncertain=(), options="all", specs=None):
    lo, hi = planes
    keys = np.asarray(keys, np.int64)
    base, inv, _ = key_frame(lo, hi)
    vis = keys >= 0
    assert ((keys[vis] >= 1) & (keys[vis] <= inv - 1)).all(), name
    if hidden_z is None:
        hidden_z = lo / 2.0 if lo > 0.0 else lo - 1.0
    return Frame(name, W, H, lo, hi, keys, ids, float(hidden_z), tuple(uncertain), options, why, specs)


def _runs(rng, values, n, mean_run):
    """n keys out of `values` in runs of equal keys (lengths around mean_run), neighbouring runs with different values"""
    out, last = [], None
    while len(out) < n:
        v = int(values[int(rng.integers(0, len(values)))])
        if v == last and len(values) > 1:
            continue
        out += [v] * min(int(rng.integers(1, 2 * mean_run)), n - len(out))
        last = v
    return out


def _log_uniform(rng, lo, hi, n):
    return np.clip(np.exp(rng.uniform(np.log(lo), np.log(hi + 1.0), n)).astype(np.int64), lo, hi)


def _span(name, planes, top, seed, why):
    """keys 1 and `top` and a few thousand spread log-uniformly between, a fifth of them tied in threes"""
    rng = np.random.default_rng(seed)
    k = _log_uniform(rng, 1, top, 3000)
    k = np.concatenate([[1, top], k[200:1600], np.repeat(k[:200], 3), [-1] * 37, k[1600:]])          # (runs of three stay runs: ids permute)
    return _frame(name, planes, k, why)


def _ladder(r):
    """27-bit planes, occupied range 511 << (r - 1) keys (510 for r = 0; r = 20: 1023 << 17, the widest range whose top 10-bit digit
    still leaves 18 bits): under the 9-bit digit rem = min(r, 19).  Seven clusters of keys whose bits under the 9-bit digit take every
    pattern that matters (all clear, all set, only the top one set, all but the top one), random ones and ties."""
    rng = np.random.default_rng(100 + r)
    width = 510 if r == 0 else ((1023 << 17) if r == 20 else (511 << (r - 1)))
    kmin = 1 if r == 20 else min((1 << 26) + 12345, (1 << 27) - 2 - width - 4321)
    rem = min(r, 19)
    keys = [kmin, kmin + width]
    for c in range(7):                                          # (the last one small: in LDS under a local capacity of 64)
        first = (int(rng.integers(0, (width >> rem) + 1)) << rem) if c else 0            # a bucket of the 9-bit digit
        lows = np.unique(np.concatenate([[0, (1 << rem) - 1, (1 << rem) >> 1, max(((1 << rem) >> 1) - 1, 0)], rng.integers(0, 1 << rem, 50)]))
        lows = lows[first + lows <= width]
        keys += [kmin + first + int(x) for x in lows] + [kmin + first + v for v in _runs(rng, lows, 120 if c < 6 else 0, 3)]
    keys += [-1] * 21
    return _frame(f"rem_ladder_{r}", PLANES27, np.roll(np.array(keys, np.int64), 333),
                  f"occupied range {width} keys: rem = {rem} under the 9-bit digit")


def _narrow(ulps):
    rng = np.random.default_rng(ulps)
    keys = np.concatenate([[1, ulps], rng.integers(1, ulps + 1, 1500), [-1] * 11])
    return _frame(f"narrow_planes_{ulps}", planes_of_bits(4.0, ulps), rng.permutation(keys), f"max_depth = min_depth + {ulps} ulps")


def _key_width(kb):
    """planes (256 - (2^kb - 2) ulps, 256]: kb key bits; the keys sit in the last 2^22 of the range (depths in (192, 256])"""
    rng = np.random.default_rng(500 + kb)
    hi = 256.0
    lo = f32(float_bits(hi) - ((1 << kb) - 2))
    top = (1 << kb) - 2
    keys = np.concatenate([[1 if kb <= 22 else top - (1 << 22), top], rng.integers(max(1, top - (1 << 22)), top + 1, 300), [-1] * 5])
    return _frame(f"key_width_{kb}", (lo, hi), rng.permutation(keys), f"{kb} key bits", options="basic")


def _wide_zero():
    rng = np.random.default_rng(31)
    z = np.exp(rng.uniform(np.log(0.5), np.log(250.0), 400)).astype(np.float32)
    keys = np.concatenate([z.view(np.uint32).astype(np.int64)[rng.integers(0, 400, 1200)], [-1] * 9])
    return _frame("wide_planes_31", (0.0, 300.0), rng.permutation(keys), "min_depth = 0: 31 key bits, LSD passes 8+8+8+7, the MSD option falls back")


def _wide_negative():
    """min_depth = -1, max_depth = 3.4e38: the key is the whole bit pattern, the invisible key 0xFFFFFFFF.  Eight rows at depths in
    [-0.9, -0.1] (two of them tied): if the CPU oracle renders them they sort behind every positive depth, in descending z"""
    rng = np.random.default_rng(32)
    z = np.exp(rng.uniform(np.log(0.5), np.log(250.0), 400)).astype(np.float32)
    pos = z.view(np.uint32).astype(np.int64)[rng.integers(0, 400, 1200)]
    neg = np.array([-0.9, -0.1, -0.5, -0.25, -0.5, -0.75, -0.3, -0.6], np.float32).view(np.uint32).astype(np.int64)
    keys = np.concatenate([pos, [-1] * 9])
    keys = rng.permutation(keys)
    at = np.sort(rng.choice(keys.size, 8, replace=False))
    keys = np.insert(keys, at, neg)
    uncertain = np.flatnonzero(keys >= (1 << 31))
    assert uncertain.size == 8
    return _frame("wide_planes_32", (-1.0, 3.4e38), keys, "32 key bits, LSD passes 8+8+8+8; depths below zero", uncertain=uncertain.tolist())


def _buckets(name, sizes, seed, why, options="all"):
    """27-bit planes, occupied range 511 << 3 keys: rem = 4 under the 9-bit digit, 256 buckets of 16 keys.  sizes = {digit: count}; the
    keys of a bucket come in runs of equal keys in designed order (a few hundred runs in the large ones)"""
    rng = np.random.default_rng(seed)
    kmin, width = (1 << 26) + 777, 511 << 3
    assert 0 in sizes and 255 in sizes, "the first and the last bucket hold the range's ends"
    keys = []
    for digit, n in sorted(sizes.items()):
        lows = np.arange(16) if digit < 255 else np.arange(width - (255 << 4) + 1)
        ks = _runs(rng, lows, n, max(1, n // 300))
        if digit == 0:
            ks[0] = 0
        if digit == 255:
            ks[0] = int(lows[-1])
        keys += [kmin + (digit << 4) + v for v in ks]
    keys = np.array(keys + [-1] * 13, np.int64)
    # (a run stays a run: the designed order is a rotation, the ids are a permutation)
    return _frame(name, PLANES27, np.roll(keys, 1000), why, options=options)


def _second_trip(name, swap):
    """P = 524288 + 300, 40 visible: the range's ends in the rows only the second trip of the reduction reads, or in the first
    workgroup and the last partial one"""
    P = 2048 * 256 + 300
    rng = np.random.default_rng(77)
    keys = np.full(P, -1, np.int64)
    mid = rng.integers(5000, 9000, 38)
    mid[:6] = mid[6:12]                                                   # ties
    keys[6 + rng.choice(250, 38, replace=False)] = mid                    # rows 6 .. 255
    lo_row, hi_row = (5, P - 1) if swap else (P - 1, 2048 * 256 + 1)
    keys[lo_row], keys[hi_row] = 100, 3_000_000
    assert int((keys >= 0).sum()) == 40
    return _frame(name, PLANES26, keys, "the key range reduced over two trips of 2048 pairs", ids=np.arange(P), options="async")


@functools.lru_cache(maxsize=None)
def frames():
    f = [
        _span("span27_full", PLANES27, (1 << 27) - 2, 1, "the whole 27-bit range: rem = 19 under the 9-bit digit (512 threads: the 32-bit LDS word), 18 under 10 bits"),
        _span("span27_half", PLANES27, (1 << 26) - 1, 2, "half the 27-bit range: rem = 18 under the 9-bit digit, 17 under 10 bits"),
        _span("span28_full", PLANES28, (1 << 28) - 2, 3, "the whole 28-bit range: only the 10-bit digit applies, rem = 19"),
        _span("span28_half", PLANES28, (1 << 27) - 1, 4, "half the 28-bit range: rem = 18 under the 10-bit digit"),
    ]
    f += [_ladder(r) for r in range(21)]
    f += [_narrow(u) for u in (100, 510, 511, 131071)]
    f += [_key_width(kb) for kb in range(2, 31)]
    f += [_wide_zero(), _wide_negative()]
    f += [
        _buckets("bucket_edges_a", {0: 1, 3: 4096, 17: 4097, 40: 8192, 90: 256, 130: 512, 131: 64, 200: 65, 255: 63}, 41,
                 "buckets of exactly 4096 / 8192 and of 4097; of 1, 63, 64, 65, 256, 512", options="async"),
        _buckets("bucket_edges_b", {0: 2, 9: 8193, 255: 130}, 42, "a bucket of 8193: one beyond the LDS of 512 threads, two scan chunks", options="async"),
        _buckets("bucket_edges_c", {0: 2, 77: 16385, 255: 130}, 43, "a bucket of 16385: three scan chunks under 512 threads, five under 256", options="async"),
    ]
    f[0] = f[0]._replace(options="async")
    f += [_second_trip("second_trip_ends_behind", False), _second_trip("second_trip_ends_apart", True)]
    f += [
        _frame("none_visible", PLANES26, [-1] * 2049, "no visible Gaussian: kmax == 0"),
        _frame("one_visible_p1", PLANES26, [1234567], "P = 1"),
        _frame("one_visible_last_row", PLANES26, [-1] * 2047 + [(1 << 25) + 3], "P = 2048, the visible one in the last row", ids=np.arange(2048)),
        # (no rect over the whole image here: 8681 of the 8704 tiles are without instances, in front of, between and behind the others)
        _frame("big_grid", PLANES26, [3000, 2000, 2000], "128 x 68 tiles: the zero fill of 8704 tile ranges rides in the depth sort's kernels", W=2048, H=1088,
               ids=np.array([2, 0, 1]), specs=(bc.dot(5, 3), bc.square(16 * 64, 30, 4), bc.square(16 * 100, 60, 2))),
    ]
    assert len({x.name for x in f}) == len(f)
    return tuple(f)


def frame(name):
    return next(x for x in frames() if x.name == name)


FRAME_NAMES = tuple(x.name for x in frames())
# frames whose every variant starts from state buffers of 0xFF bytes (a stale state already holds this frame's tile ranges, zeros for
# the tiles without instances included: a zero fill that did not happen would not show)
FRESH_STATE = ("big_grid",)


def auto_edge(threads, extra):
    """A frame whose largest bucket under the 9-bit digit is the capacity of a `threads`-wide bucket workgroup, + extra"""
    cap = threads * DLS_ITEMS
    return _buckets(f"auto_edge_{threads}_{extra}", {0: 5, 50: cap + extra, 120: cap - 1, 255: 7}, threads + extra, "the auto mode's edge")


# ------------------------------------------------------------------------------------------------ the designed scene
def spec_of(i, W, H):
    """the rect of the i-th designed Gaussian: a 1 x 1 dot, a 2 x 2 square, the whole image, in turn"""
    gx, gy = W // 16, H // 16
    j = i // 3
    if i % 3 == 0:
        return bc.dot(j % gx, (j // gx) % gy)
    if i % 3 == 1:
        return bc.square(16 * (1 + j % (gx - 1)), (j // (gx - 1)) % (gy - 1), 2)
    return bc.full(W, H)


def ids_of(fr):
    """the id of the i-th designed Gaussian: the frame's own list, or a seeded permutation"""
    if fr.ids is not None:
        return np.asarray(fr.ids, np.int64)
    seed = 8000 + FRAME_NAMES.index(fr.name) if fr.name in FRAME_NAMES else 7
    return np.random.default_rng(seed).permutation(fr.keys.size)


def designed(fr):
    """dict of the plan: z (float32, designed order), ids, specs; by id: keys_by_id (-1 hidden), z_by_id, uncertain_by_id"""
    P = fr.keys.size
    base, inv, kb = key_frame(fr.min_depth, fr.max_depth)
    vis = fr.keys >= 0
    zbits = np.where(vis, (base + fr.keys) & 0xFFFFFFFF, 0).astype(np.uint32)
    z = np.where(vis, zbits.view(np.float32), np.float32(fr.hidden_z)).astype(np.float32)
    ids = ids_of(fr)
    specs = [spec_of(i, fr.W, fr.H) if vis[i] else bc.HIDDEN for i in range(P)] if P < 100000 else None
    if fr.specs is not None:
        specs = list(fr.specs)
    if specs is None:                                      # (mostly hidden: only the visible rows need a spec)
        specs = [bc.HIDDEN] * P
        for i in np.flatnonzero(vis):
            specs[i] = spec_of(int(i), fr.W, fr.H)
    keys_by_id = np.full(P, -1, np.int64)
    keys_by_id[ids] = fr.keys
    z_by_id = np.zeros(P, np.float32)
    z_by_id[ids] = z
    unc = np.zeros(P, bool)
    unc[ids[np.array(fr.uncertain, np.int64)]] = True
    return dict(P=P, z=z, ids=ids, specs=specs, keys_by_id=keys_by_id, z_by_id=z_by_id, uncertain_by_id=unc, base=base, invisible=inv, key_bits=kb)


def scene_of(fr):
    """(inputs, settings) of a frame: binning_cases.build_scene on the designed depths and ids"""
    d = designed(fr)
    seed = 1900 + (FRAME_NAMES.index(fr.name) if fr.name in FRAME_NAMES else 99)
    return bc.build_scene(f"depth sort frame {fr.name}", fr.W, fr.H, d["specs"], d["z"], d["ids"], fr.min_depth, fr.max_depth, seed)


@functools.lru_cache(maxsize=2)
def scene(name):
    return scene_of(frame(name))


@functools.lru_cache(maxsize=2)
def oracle_of(name):
    return bc.oracle_binning(*scene(name))


def designed_rects(fr, d):
    """[P,4] by id: the tile rects the specs mean (x0, y0, w, h); zeros for hidden rows"""
    gx, gy = fr.W // 16, fr.H // 16
    out = np.zeros((d["P"], 4), np.int64)
    for i in np.flatnonzero(fr.keys >= 0):
        px, py, r, _ = d["specs"][i]
        if r == 2:                                         # binning_cases.dot
            rect = (int(px) // 16, int(py) // 16, 1, 1)
        elif r == max(fr.W, fr.H) + 32:                    # binning_cases.full
            rect = (0, 0, gx, gy)
        else:                                              # binning_cases.square with an even k, centred on a tile corner
            k = (r + 6) // 8
            assert k % 2 == 0 and int(px) % 16 == 0
            rect = (int(px) // 16 - k // 2, (int(py) - 8 * k) // 16, k, k)
        out[d["ids"][i]] = rect
    return out


def keys_of(fr, radii, depths):
    """the depth keys of a frame's own arrays, by id: bits(depth) - key base for radii > 0, -1 for the others"""
    base = key_frame(fr.min_depth, fr.max_depth)[0]
    bits = np.ascontiguousarray(bc._np(depths), np.float32).view(np.uint32).astype(np.int64)
    return np.where(bc._np(radii) > 0, (bits - base) & 0xFFFFFFFF, -1)


# ------------------------------------------------------------------------------------------------ census
def lsd_passes(kb):
    """ex4d_radix_sort_pairs up to 2 M items: ceil(kb / 9) passes of balanced widths"""
    npass = (kb + LSD_MAX_DIGIT - 1) // LSD_MAX_DIGIT
    widths, shift = [], 0
    for p in range(npass):
        widths.append((kb - shift + (npass - p) - 1) // (npass - p))
        shift += widths[-1]
    return widths


def scatter_of(nbits):
    return {9: "9", 8: "8"}.get(nbits, "g")


def msd_shift(width, digit_bits):
    """dls_reduce_ranges: the smallest shift with (kmax - kmin) >> shift <= BINS - 2"""
    s = 0
    while (width >> s) > (1 << digit_bits) - 2:
        s += 1
    return s


def bucket_pass_widths(rem):
    """dls_pass_bits: (rem + 8) / 9 passes of balanced widths"""
    npass = (rem + 8) // 9
    widths, lo = [], 0
    for p in range(npass):
        widths.append((rem - lo + (npass - p) - 1) // (npass - p))
        lo += widths[-1]
    return widths


def lds_sort_class(rem):
    return {16: "ct8+8", 17: "ct9+8"}.get(rem, "rt" + "+".join(str(w) for w in bucket_pass_widths(rem)))


def msd_choice(P, kb, options):
    """(digit bits, threads, capacity) of the MSD sort: forward_impl's msd_bits, depth_sort_msd_launch's local_threads / local_cap"""
    bits = depth_sort_msd_bits(P, kb)
    forced = options["depth_sort_msd_bits"]
    if forced == 10 or (forced == 9 and depth_sort_msd_bits(1, kb) == 9):
        bits = forced
    threads = options["depth_sort_local_threads"]
    if threads not in (256, 512):
        threads = 512 if (bits < 10 or P > THREADS_COUNT) else 256
    kcap = threads * DLS_ITEMS
    cap = options["depth_sort_local_cap"]
    if cap == 0 or cap > kcap:
        cap = kcap
    return bits, threads, cap


def census(fr, keys_by_id, options, asynchronous=False):
    """The cells a frame reaches under these options (every option of BASE_OPTIONS): keys_by_id = the depth keys by id, -1 for an
    invisible Gaussian"""
    keys_by_id = np.asarray(keys_by_id, np.int64)
    P = keys_by_id.size
    assert P <= (2 << 20), "beyond 2 M Gaussians the sorts run other instantiations: outside this census"
    base, inv, kb = key_frame(fr.min_depth, fr.max_depth)
    _, depth, _, tile_sort, fused_scan, lsd_gather, _ = path_signature(P, fr.W, fr.H, fr.min_depth, fr.max_depth, options, asynchronous)
    vis_ids = np.flatnonzero(keys_by_id >= 0)
    k = keys_by_id[vis_ids]
    cells = set()
    # ---- keys
    if k.size:
        if (k == 1).any():
            cells.add("keys.first")
        if (k == inv - 1).any():
            cells.add("keys.last")
        o = np.argsort(k, kind="stable")
        ks, ids_s = k[o], vis_ids[o]
        same = ks[1:] == ks[:-1]
        if (same & (ids_s[1:] // PARTITION_BLOCK != ids_s[:-1] // PARTITION_BLOCK)).any():
            cells.add("keys.tie_run_across_partition_blocks")
        if (same & (ids_s[1:] // 64 == ids_s[:-1] // 64)).any():
            cells.add("keys.tie_run_inside_a_wave")
    if depth == "lsd":
        widths = lsd_passes(kb)
        cells.add(f"lsd.passes.{len(widths)}")
        cells.add("lsd.scatter." + "+".join(scatter_of(w) for w in widths))
        cells.add(f"lsd.start_in_b.{len(widths) & 1}")
        cells.add(f"lsd.gather.{int(lsd_gather)}")
        if options["depth_sort_msd"] != 0:
            cells.add("lsd.msd_declined")
        return cells
    # ---- the MSD sort
    bits, threads, cap = msd_choice(P, kb, options)
    cells |= {f"msd.digit.{bits}", f"msd.threads.{threads}"}
    tile_rows = tile_sort == "rows"
    cells.add("msd.scan." + ("fused" if fused_scan else ("none" if tile_rows else "kernel")))
    if k.size == 0:
        cells.add("msd.no_visible")
        return cells
    kmin, kmax = int(k.min()), int(k.max())
    for what, extreme in (("min", kmin), ("max", kmax)):
        if (vis_ids[k == extreme] >= RANGE_PAIR * RANGE_TRIP).all():
            cells.add(f"msd.range.{what}_in_the_second_trip_only")
    rem = msd_shift(kmax - kmin, bits)
    assert rem + IDX_BITS[threads] <= 32, "the LDS word overflows"
    cells.add(f"msd.rem.{bits}.{rem}")
    if rem + IDX_BITS[threads] == 32:
        cells.add("msd.lds_word_32_bits")
    digit = (k - kmin) >> rem
    n_of = np.bincount(digit, minlength=(1 << bits) - 1)
    assert n_of.size == (1 << bits) - 1
    if (n_of == 0).any():
        cells.add("bucket.empty")
    if k.size < P:
        cells.add("bucket.invisible_digit")
    waves = threads // 64
    T = f"{threads}"
    for n in np.unique(n_of[n_of > 0]).tolist():
        if n == 1:
            cells.add("bucket.n1")
        elif rem == 0:
            cells.add("bucket.rem0_scan_only")
        elif n <= cap:
            cells.add(f"bucket.lds.{lds_sort_class(rem)}")
            cells.add(f"bucket.lds.rem.{rem}")
            if n < 64:
                cells.add(f"bucket.lds.{T}.n_lt_64")
            if n == 64 * waves:
                cells.add(f"bucket.lds.{T}.n_eq_64_waves")
            if n > 64 and n % 64:
                cells.add(f"bucket.lds.{T}.partial_last_wave")
            if n == threads * DLS_ITEMS:
                cells.add(f"bucket.lds.{T}.n_eq_cap")
        else:
            cells.add(f"bucket.mem.passes.{len(bucket_pass_widths(rem))}")
            if n == threads * DLS_ITEMS + 1:
                cells.add(f"bucket.mem.{T}.n_eq_cap_plus_1")
        if n > threads * DLS_ITEMS and fused_scan:
            cells.add(f"bucket.scan.{T}.chunks_ge_2")
    cells.add("msd.watch." + ("raised" if (n_of > cap).any() else "clear"))
    # ties inside one 64-wide step of a wave of the bucket kernel (arrival order = id order inside a bucket)
    o = np.lexsort((vis_ids, digit))
    d_s, k_s = digit[o], k[o]
    arrival = np.arange(k.size) - np.searchsorted(d_s, d_s, "left")
    n_s = n_of[d_s]
    in_lds = (n_s > 1) & (n_s <= cap) & (rem > 0)
    step = arrival // 64
    o2 = np.lexsort((step, k_s, d_s))
    a, b = o2[1:], o2[:-1]
    if (in_lds[a] & (d_s[a] == d_s[b]) & (k_s[a] == k_s[b]) & (step[a] == step[b])).any():
        cells.add("bucket.lds.tie_inside_a_wave_step")
    return cells


def reachable_cells():
    """Every cell reachable below 2 M Gaussians, and what the host rules exclude: (reachable, excluded).
    Computed from the host rules (key_bits' range 2..32, depth_sort_msd_applies, depth_sort_msd_bits, the LDS word's capacity): the LSD
    cells (pass counts, scatter instantiations per pass, the starting buffer), msd.rem.<digit>.<rem>, msd.lds_word_32_bits and, from
    the rems, bucket.lds.<passes>, bucket.lds.rem.<rem> and bucket.mem.passes.<n>; the excluded set likewise.
    Enumerated: the categorical cells that every value of an option or of a bucket's size reaches whatever the planes are (digit
    width, workgroup size, the three forms of the tile scan, the bucket kernel's early ends and the size edges per workgroup size, the
    watch word, the key cells).  Coverage is per cell, not joint: bucket.lds.rem.<rem> is not tied to a digit width or a workgroup
    size (the option sets run every ladder frame under both)."""
    cells = {"keys.first", "keys.last", "keys.tie_run_across_partition_blocks", "keys.tie_run_inside_a_wave", "lsd.msd_declined"}
    excluded = set()
    for kb in range(2, 33):                       # (max_depth > min_depth: the invisible key is at least 2)
        widths = lsd_passes(kb)
        cells |= {f"lsd.passes.{len(widths)}", "lsd.scatter." + "+".join(scatter_of(w) for w in widths), f"lsd.start_in_b.{len(widths) & 1}"}
    cells |= {"lsd.gather.0", "lsd.gather.1"}
    rems = set()
    for kb in range(2, 33):
        width = (1 << kb) - 3 if kb < 32 else 0xFFFFFFFD          # keys 1 .. invisible - 1 <= 2^kb - 2
        for bits in (9, 10):
            allowed = depth_sort_msd_applies(1, kb) and (bits == 10 or depth_sort_msd_bits(1, kb) == 9)
            for rem in range(0, msd_shift(width, bits) + 1):
                (cells if allowed else excluded).add(f"msd.rem.{bits}.{rem}")
                if allowed:
                    rems.add(rem)
                    assert rem + max(IDX_BITS.values()) <= 32, (kb, bits, rem)
            if not allowed:
                excluded.add(f"msd.digit.{bits}.at.{kb}")
    excluded -= cells
    cells |= {"msd.digit.9", "msd.digit.10", "msd.threads.256", "msd.threads.512", "msd.scan.fused", "msd.scan.kernel", "msd.scan.none",
              "msd.no_visible", "msd.range.min_in_the_second_trip_only", "msd.range.max_in_the_second_trip_only", "msd.watch.raised", "msd.watch.clear",
              "bucket.empty", "bucket.invisible_digit", "bucket.n1", "bucket.rem0_scan_only", "bucket.lds.tie_inside_a_wave_step"}
    if max(rems) + IDX_BITS[512] == 32:
        cells.add("msd.lds_word_32_bits")
    for rem in rems - {0}:
        cells |= {f"bucket.lds.{lds_sort_class(rem)}", f"bucket.lds.rem.{rem}", f"bucket.mem.passes.{len(bucket_pass_widths(rem))}"}
    for T in (256, 512):
        cells |= {f"bucket.lds.{T}.n_lt_64", f"bucket.lds.{T}.n_eq_64_waves", f"bucket.lds.{T}.partial_last_wave", f"bucket.lds.{T}.n_eq_cap",
                  f"bucket.mem.{T}.n_eq_cap_plus_1", f"bucket.scan.{T}.chunks_ge_2"}
    return cells, excluded


# ------------------------------------------------------------------------------------------------ option sets
_MSD = dict(depth_sort_msd=2, tile_sort_rows=0, binning_tile_ids=1)
CHAINS = (
    ("lsd, rows", dict(depth_sort_msd=0, tile_sort_rows=1, binning_tile_ids=1)),
    ("lsd, pairs", dict(depth_sort_msd=0, tile_sort_rows=0, binning_tile_ids=1)),
    ("msd, rows", dict(depth_sort_msd=2, tile_sort_rows=1, binning_tile_ids=1)),
    ("msd, pairs", _MSD),
    ("msd + scan kernel, pairs", dict(_MSD, depth_sort_msd=1)),
)
PATHS = tuple(
    [("msd + scan kernel, rows", dict(_MSD, depth_sort_msd=1, tile_sort_rows=1))]
    + [(f"msd, pairs, {b} bits, {t} threads, cap {c}", dict(_MSD, depth_sort_msd_bits=b, depth_sort_local_threads=t, depth_sort_local_cap=c))
       for b in (9, 10) for t in (256, 512) for c in (0, 1, 64)]
    + [("msd, rows, 10 bits, 512 threads", dict(_MSD, tile_sort_rows=1, depth_sort_msd_bits=10, depth_sort_local_threads=512)),
       ("msd + scan kernel, pairs, cap 1", dict(_MSD, depth_sort_msd=1, depth_sort_local_cap=1))])
BALLOTS = (
    ("lsd, pairs, ballots", dict(depth_sort_msd=0, tile_sort_rows=0, rank_lds_atomics=0)),
    ("msd, pairs, ballots", dict(depth_sort_msd=2, tile_sort_rows=0, rank_lds_atomics=0)),
    ("msd, pairs, cap 1, ballots", dict(depth_sort_msd=2, tile_sort_rows=0, depth_sort_local_cap=1, rank_lds_atomics=0)),
)
ASYNC = (("lsd, rows", CHAINS[0][1]), ("msd, rows", CHAINS[2][1]), ("msd, pairs", _MSD), ("msd, pairs, cap 64", dict(_MSD, depth_sort_local_cap=64)))


def option_sets(fr, keys_by_id):
    """[(label, options over BASE_OPTIONS, asynchronous, cells)]: the LSD variant first; of the candidates only those that select
    another chain or reach other cells on this frame"""
    cand = [(l, o, False) for l, o in CHAINS]
    if fr.options != "basic":
        cand += [(l, o, False) for l, o in PATHS + BALLOTS]
    if fr.options == "async":
        cand += [(l + ", asynchronous", o, True) for l, o in ASYNC]
    out, seen = [], set()
    P = int(np.asarray(keys_by_id).size)
    for label, opts, asyn in cand:
        full = dict(BASE_OPTIONS, **opts)
        cells = census(fr, keys_by_id, full, asyn)
        key = (path_signature(P, fr.W, fr.H, fr.min_depth, fr.max_depth, full, asyn), frozenset(cells), full["rank_lds_atomics"])
        if key not in seen:
            seen.add(key)
            out.append((label, opts, asyn, cells))
    return out


@functools.lru_cache(maxsize=None)
def promised(name):
    """{label: cells} of a frame, from the CPU oracle's radii and depths"""
    fr = frame(name)
    o = oracle_of(name)
    return {label: cells for label, _, _, cells in option_sets(fr, keys_of(fr, o["radii"], o["depths"]))}
