"""The sample depth sort (option "depth_sort_sample") restated in numpy, and the frames designed for it; shared by
tests/test_cpu_sample_sort_cases.py and tests/test_gpu_sample_sort.py.

The rule (ex4dgs_amd/csrc/ex4d_binning.hip, "depth sort by sampling"), on the keys by id -- bits(depth) - bits(min_depth) for a visible
Gaussian, the invisible key (one above every visible key) otherwise:
  sample     the keys at ids 0, s, 2 s, ... with s = ceil(P / 8192), sorted;
  splitters  B - 2 quantiles sorted[(j + 1) ns / (B - 1)] (ns = sample size, B = 512 buckets up to 1.3 M Gaussians, 1024 beyond),
             then the invisible key twice;
  table      a value that occurs once in that list closes the bucket (previous value, v]; a value that occurs more than once closes
             (previous value, v) and gets the bucket [v, v]; the upper bounds are kept in the doubled space 2 key + 1, padded with ~0;
  bucket     of a key: the number of table entries below 2 key + 1; the partition is stable;
  per bucket of n keys that admits the keys [klo, khi]: n == 0 empty; n == 1 or klo == khi skipped; n > capacity through memory;
             else in LDS on packed words where bits(khi - klo) + index bits <= 32, on (key, index) pairs where not.
The bucket kernel's capacity is derived: threads x 16 items (DlsLds<THREADS>::CAP), its index bits log2 of that."""
import functools

import numpy as np

from tests import binning_cases as bc
from tests import depth_sort_cases as dc

S = 8192                                      # SS_SAMPLE
BINS_COUNT = 1300000                          # ex4d_depth_sort_sample_bins: 512 buckets up to here, 1024 beyond
STATS = ("empty", "skipped", "packed", "pairs", "memory", "memory_gaussians", "largest", "distinct_splitters")
PLANES_WIDE = (0.01, 300.0)                   # cfg5's planes: 27 key bits


def capacity(threads):
    return threads * dc.DLS_ITEMS


def bins_of(P):
    return 512 if P <= BINS_COUNT else 1024


def stride_of(P):
    return -(-P // S)


def splitter_list(keys, inv):
    """the B splitters of a frame: sampled quantiles and the invisible key twice (ascending)"""
    keys = np.asarray(keys, np.int64)
    P, B = keys.size, bins_of(keys.size)
    sample = np.sort(keys[::stride_of(P)])
    ns = sample.size
    assert 1 <= ns <= S
    j = np.arange(B - 2, dtype=np.int64)
    return np.concatenate([sample[((j + 1) * ns) // (B - 1)], [inv, inv]]).astype(np.int64)


def bucket_table(spl):
    """upper bounds in the doubled space, padded to the list's length with 2^32 - 1; and the number of distinct splitters"""
    vals, counts = np.unique(spl, return_counts=True)
    ub = []
    for v, c in zip(vals.tolist(), counts.tolist()):
        ub += [2 * v, 2 * v + 1] if c >= 2 else [2 * v + 1]
    assert len(ub) <= spl.size
    return np.array(ub + [0xFFFFFFFF] * (spl.size - len(ub)), np.int64), int(vals.size)


def bucket_of(ub, keys):
    return np.searchsorted(ub, 2 * np.asarray(keys, np.int64) + 1, side="left")


def choice(options):
    """(threads, capacity) of the bucket kernel under these options (depth_sort_sample_launch)"""
    threads = options.get("depth_sort_local_threads", 0)
    if threads not in (256, 512):
        threads = 512
    cap = options.get("depth_sort_local_cap", 0)
    if cap == 0 or cap > capacity(threads):
        cap = capacity(threads)
    return threads, cap


def restate(keys, inv, options=None):
    """(order, census, paths): the depth order as the kernels arrive at it, the eight counters of ex4d_debug_sample_sort for one
    frame, and {bucket: path} of the non-empty buckets.  keys: by id, `inv` for an invisible Gaussian"""
    keys = np.asarray(keys, np.int64)
    threads, cap = choice(options or {})
    idx_bits = dc.IDX_BITS[threads]
    spl = splitter_list(keys, inv)
    ub, distinct = bucket_table(spl)
    b = bucket_of(ub, keys)
    assert b.max() < ub.size and ub[b.max()] != 0xFFFFFFFF
    order = np.argsort(b, kind="stable")                           # the stable partition: ascending id inside a bucket
    n_of = np.bincount(b, minlength=ub.size)
    starts = np.concatenate([[0], np.cumsum(n_of)])
    census = dict.fromkeys(STATS, 0)
    census["distinct_splitters"] = distinct
    census["empty"] = int((n_of == 0).sum())
    paths = {}
    for i in np.flatnonzero(n_of).tolist():
        n, s = int(n_of[i]), int(starts[i])
        klo = ((int(ub[i - 1]) if i else 0) + 1) >> 1
        khi = (int(ub[i]) - 1) >> 1
        ids = order[s:s + n]
        k = keys[ids]
        assert klo <= k.min() and k.max() <= khi
        span = khi - klo
        rem = span.bit_length()
        if span:
            census["largest"] = max(census["largest"], n)
        if n < 2 or span == 0:
            paths[i] = "skipped"
            assert (k[1:] >= k[:-1]).all()
        elif n > cap:
            paths[i] = "memory"
            census["memory_gaussians"] += n
            order[s:s + n] = ids[np.argsort(k - klo, kind="stable")]
        elif rem + idx_bits <= 32:
            paths[i] = "packed"                                     # one word per Gaussian: (key - klo) << index bits | arrival index
            words = ((k - klo) << idx_bits) | np.arange(n)
            assert words.max() < (1 << 32)
            order[s:s + n] = ids[np.sort(words) & ((1 << idx_bits) - 1)]
        else:
            paths[i] = "pairs"
            order[s:s + n] = ids[np.argsort(k - klo, kind="stable")]
        census[paths[i]] += 1
    return order, census, paths


def keys_with_inv(keys_by_id, inv):
    k = np.asarray(keys_by_id, np.int64)
    return np.where(k < 0, inv, k)


# ------------------------------------------------------------------------------------------------ the designed frames
def _spread(rng, n, top, ties=0.1):
    k = dc._log_uniform(rng, 1, top, n)
    t = int(n * ties)
    if t:
        k[rng.integers(0, n, t)] = k[rng.integers(0, n, t)]
    return k


def _mix(rng, vis, hidden):
    return rng.permutation(np.concatenate([np.asarray(vis, np.int64), np.full(hidden, -1, np.int64)]))


TOP26 = dc.key_frame(*dc.PLANES26)[1] - 1
TOP27 = dc.key_frame(*PLANES_WIDE)[1] - 1


def _sized(P):
    rng = np.random.default_rng(P)
    hidden = P // 20 if P > 2 else 0
    return dc._frame(f"p_{P}", dc.PLANES26, _mix(rng, _spread(rng, P - hidden, TOP26), hidden), f"P = {P}")


def _walls(name, walls, P, why, near=False):
    """`walls` = [(key, count)]: count Gaussians at one key (near: count distinct keys 3 apart), the rest spread over the range"""
    rng = np.random.default_rng(len(name) + P)
    vis = [np.arange(n) * 3 + k if near else np.full(n, k) for k, n in walls]
    rest = P - sum(n for _, n in walls) - 200
    return dc._frame(name, dc.PLANES26, _mix(rng, np.concatenate(vis + [_spread(rng, rest, TOP26)]), 200), why)


def _by_id(name, planes, keys, why):
    return dc._frame(name, planes, keys, why, ids=np.arange(len(keys)))


def _periodic():
    """P = 3 S: the sample reads ids 0, 3, 6, ... and sees ONE value A there; the other ids hold 8192 keys below A and 8192 above: four
    buckets -- below A and above A of exactly the capacity of 512 threads, A itself, the invisible key's (empty)"""
    rng = np.random.default_rng(12)
    P, A = 3 * S, 1 << 24
    keys = np.full(P, A, np.int64)
    other = np.flatnonzero(np.arange(P) % 3)
    keys[other] = rng.permutation(np.concatenate([rng.integers(1, A, S), rng.integers(A + 1, TOP26, S)]))
    return _by_id("periodic_with_the_stride", dc.PLANES26, keys, "the sample sees one value; two ordinary buckets of exactly 8192")


def _skipped(name, visible, why):
    """P = 3 S, visible Gaussians only at ids the sample skips: every splitter is the invisible key, every visible key in ONE bucket"""
    rng = np.random.default_rng(visible)
    P = 3 * S
    keys = np.full(P, -1, np.int64)
    other = np.flatnonzero(np.arange(P) % 3)
    keys[rng.choice(other, visible, replace=False)] = _spread(rng, visible, TOP26)
    return _by_id(name, dc.PLANES26, keys, why)


def _cap_edge():
    """P = 3 S.  The sampled ids hold A and B (half each): buckets below A, [A], (A, B), [B], (B, invisible), [invisible].  The other ids
    hold 64 distinct keys between A and B, 65 above B, 3 below A: under depth_sort_local_cap = 64 an ordinary bucket of exactly the
    capacity and one of one more"""
    rng = np.random.default_rng(64)
    P, A, B = 3 * S, 1 << 20, 1 << 23
    keys = np.full(P, -1, np.int64)
    sampled = np.arange(0, P, 3)
    keys[sampled] = np.where(np.arange(S) % 2 == 0, A, B)
    other = rng.permutation(np.flatnonzero(np.arange(P) % 3))
    keys[other[:64]] = rng.choice(np.arange(A + 1, B), 64, replace=False)
    keys[other[64:129]] = rng.choice(np.arange(B + 1, TOP26), 65, replace=False)
    keys[other[129:132]] = [5, 1, 5]
    return _by_id("cap_edge_64_65", dc.PLANES26, keys, "ordinary buckets of 64 and 65 under a capacity of 64")


def _sparse_tail():
    """(0.01, 300]: 27 key bits.  19000 Gaussians inside 2^16 keys near the far end, 1000 spread over everything in front: the front
    buckets hold ~40 Gaussians over more than 2^20 keys -- their span does not fit beside the arrival index"""
    rng = np.random.default_rng(27)
    dense = TOP27 - rng.integers(0, 1 << 16, 19000)
    tail = rng.integers(1, TOP27 - (1 << 17), 1000)
    return dc._frame("sparse_tail", PLANES_WIDE, _mix(rng, np.concatenate([dense, tail]), 100), "bucket spans beyond the packed word")


@functools.lru_cache(maxsize=None)
def frames():
    rng = np.random.default_rng(99)
    f = [_sized(P) for P in (1, 2, 63, 64, 65, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1)]
    f += [
        dc._frame("ss_none_visible", dc.PLANES26, [-1] * 3000, "no visible Gaussian: every splitter is the invisible key"),
        dc._frame("ss_one_visible", dc.PLANES26, [-1] * 1500 + [777777] + [-1] * 1499, "one visible Gaussian"),
        dc._frame("mostly_invisible", dc.PLANES26, _mix(rng, _spread(rng, 1000, TOP26), 19000), "95 % invisible"),
        dc._frame("none_invisible", dc.PLANES26, _spread(rng, 20000, TOP26), "no invisible Gaussian: the invisible key's bucket is empty"),
        dc._frame("all_equal", dc.PLANES26, _mix(rng, np.full(19990, 4242424), 10), "all visible keys equal"),
        dc._frame("two_values", dc.PLANES26, _mix(rng, rng.choice([1000, TOP26], 19990), 10), "keys of two values"),
        _walls("wall_exact", [(1 << 23, 14000)], 30000, "14000 of 30000 at one key"),
        _walls("wall_near", [(1 << 23, 14000)], 30000, "14000 distinct keys 3 apart among 30000", near=True),
        _walls("two_walls", [(1 << 22, 9000), ((1 << 24) + 5, 9000)], 30000, "two walls of 9000"),
        _sparse_tail(),
        _by_id("ascending_with_id", dc.PLANES26, 1000 + 7 * np.arange(20000), "keys ascending with id: the sample is sorted already"),
        _by_id("descending_with_id", dc.PLANES26, 1000 + 7 * np.arange(20000)[::-1], "keys descending with id"),
        _periodic(),
        _skipped("skipped_ids_6000", 6000, "the sample sees no visible key: one bucket of 6000"),
        _skipped("skipped_ids_16384", 2 * S, "the sample sees no visible key: one bucket of 16384, beyond the capacity (adversarial stride)"),
        _cap_edge(),
    ]
    assert len({x.name for x in f}) == len(f) and not {x.name for x in f} & set(dc.FRAME_NAMES)
    return tuple(f)


FRAME_NAMES = tuple(x.name for x in frames())
# (frame, options over the defaults) designed for the through-memory path: no other (frame, options) of the tests may reach it
MEMORY_DESIGNED = (("skipped_ids_16384", {}),
                   ("cap_edge_64_65", dict(depth_sort_local_cap=64, depth_sort_local_threads=256)),
                   ("cap_edge_64_65", dict(depth_sort_local_cap=64, depth_sort_local_threads=512)))


def frame(name):
    return next(x for x in frames() if x.name == name)


def option_sets(name):
    """the bucket-kernel options a frame runs under: the defaults, and the frame's designed ones"""
    return [{}] + [o for n, o in MEMORY_DESIGNED if n == name and o]


def designed_keys(fr):
    """(keys by id with the invisible key filled in, invisible key)"""
    inv = dc.key_frame(fr.min_depth, fr.max_depth)[1]
    keys_by_id = np.full(fr.keys.size, -1, np.int64)
    keys_by_id[dc.ids_of(fr)] = fr.keys
    return keys_with_inv(keys_by_id, inv), inv
