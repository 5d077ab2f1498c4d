"""The cases of tests/test_gpu_binning_edges.py, without a GPU: the host restatement of the binning (tests/binning_cases.py:
host_binning) equals the CPU oracle's on every case and every tile, the cases reach every cell of the census under the option sets and
capacities the GPU test runs, and the two pieces of arithmetic the kernels state in comments only -- the duplication's division by
multiply-high and the hinted search of the row-segment sort's write-out -- hold over their whole domains."""
import numpy as np
import pytest

from tests import binning_cases as bc
from tests import helpers as h


@pytest.mark.parametrize("name", bc.CASE_NAMES)
def test_host_binning_equals_the_oracle(name):
    """point list, ranges, sorted tile ids, tiles_touched and num_rendered of the restatement, fed with the oracle's radii, means2D and
    depths, equal the oracle's own: every instance, every tile."""
    o = bc.oracle_of(name)
    c = bc.case(name)
    hb = bc.host_binning(o["radii"], o["means2D"], o["depths"], o["W"], o["H"])
    vis = np.array([s[3] for s in c.specs], bool)
    assert int((o["radii"] > 0).sum()) == int(vis.sum()), "a designed Gaussian was culled (or a hidden one was not)"
    assert hb["R"] == o["num_rendered"] and o["num_rendered"] > 0
    assert np.array_equal(hb["tiles_touched"], o["tiles_touched"].astype(np.int64))
    assert np.array_equal(hb["point_list"], o["point_list"].astype(np.int64))
    assert np.array_equal(hb["tile_ids"], (o["keys_sorted"] >> np.uint64(32)).astype(np.int64))
    assert hb["ranges"].shape == o["ranges"].shape and np.array_equal(hb["ranges"], o["ranges"].astype(np.int64))
    # the depth order is the order of the oracle's keys inside every tile: the first tile of a full-image rect lists every Gaussian
    keys = o["keys_sorted"]
    assert bool((np.diff(keys.astype(np.int64) >> 32) >= 0).all())
    same_tile = (keys[1:] >> np.uint64(32)) == (keys[:-1] >> np.uint64(32))
    assert bool(((keys[1:] & np.uint64(0xFFFFFFFF)) >= (keys[:-1] & np.uint64(0xFFFFFFFF)))[same_tile].all())


def test_the_binning_stages_alone_equal_the_oracle_forward():
    """binning_cases.oracle_binning calls the two stages oracle.forward calls, without the compositing: same radii, same lists"""
    ins, st = bc.scene("gaps")
    a, b = bc.oracle_of("gaps"), h.oracle_forward(ins, st)
    assert a["num_rendered"] == b["num_rendered"]
    for k in ("radii", "means2D", "depths", "tiles_touched", "point_list", "keys_sorted", "ranges"):
        assert np.array_equal(a[k], b[k]), k


def test_truncated_restatement():
    """host_binning with a capacity keeps the first instances of the stream the tile sort reads: Gaussian-major for the pair sorts,
    tile-row-major for the row-segment sort"""
    # two Gaussians on a 32 x 32 image, both over all four tiles; the nearer one is id 1
    radii, m, d = np.array([40, 40]), np.array([[16.0, 16.0], [16.0, 16.0]], np.float32), np.array([2.0, 1.0], np.float32)
    whole = bc.host_binning(radii, m, d, 32, 32)
    assert whole["point_list"].tolist() == [1, 0] * 4 and whole["ranges"].tolist() == [[0, 2], [2, 4], [4, 6], [6, 8]] and whole["S"] == 4
    pair = bc.host_binning(radii, m, d, 32, 32, capacity=5, form="pair")           # id 1's four instances and id 0's first (tile 0)
    assert pair["point_list"].tolist() == [1, 0, 1, 1, 1] and pair["ranges"].tolist() == [[0, 2], [2, 3], [3, 4], [4, 5]] and pair["kept"] == 5
    rows = bc.host_binning(radii, m, d, 32, 32, capacity=5, form="rows")           # tile row 0 whole, then id 1's tile 2
    assert rows["point_list"].tolist() == [1, 0, 1, 0, 1] and rows["ranges"].tolist() == [[0, 2], [2, 4], [4, 5], [0, 0]]


def test_every_cell_is_reached():
    """The union of the census over the cases, under every option set and capacity the GPU test runs, is CELLS; no case reaches a
    cell of UNREACHED.  Prints the coverage per case; a missing cell is named."""
    assert len(set(bc.CELLS)) == len(bc.CELLS) and not set(bc.CELLS) & {n for n, _ in bc.UNREACHED}
    reached, first = {}, {}
    for name in bc.CASE_NAMES:
        per_frame = bc.promised(name)
        mine = set().union(*per_frame.values())
        new = sorted(mine - set(reached))
        for c in mine:
            reached.setdefault(c, []).append(name)
        o = bc.oracle_of(name)
        print(f"{name}: P={o['P']} {o['W']}x{o['H']} R={o['num_rendered']} frames={len(per_frame)} cells={len(mine)} first here: {', '.join(new) or '-'}")
    unknown = set(reached) - set(bc.CELLS)
    assert not unknown, f"cells outside CELLS (UNREACHED, or unnamed): {sorted(unknown)}"
    missing = [c for c in bc.CELLS if c not in reached]
    assert not missing, f"cells no case reaches: {missing}"
    alone = {c: v[0] for c, v in reached.items() if len(v) == 1}
    print("cells that rest on one case:", {n: sorted(c for c, v in alone.items() if v == n) for n in sorted(set(alone.values()))})


def test_deleting_a_case_is_noticed():
    """the census has teeth: without the case they rest on, these cells are missing"""
    per_case = {name: set().union(*bc.promised(name).values()) for name in ("sh9", "cap1024", "cap2048", "bits16", "bits17", "gy255")}
    rest = set()
    for name in bc.CASE_NAMES:
        if name not in per_case:
            rest |= set().union(*bc.promised(name).values())
    for name, cells in (("sh9", {"rowsA.sh9", "rows.gx255_full_width", "passB.rows.bits.8"}), ("cap1024", {"rowsA.block.1024.staged_full", "rowsA.block.1024.sequential_by1"}),
                        ("cap2048", {"rowsA.block.2048.sequential", "rowsA.block.2048.sequential_by1"}), ("bits16", {"pairA.high.8", "passB.pair.nbuckets256_last_nonempty"}),
                        ("bits17", {"radix.two_pass_17bits"}), ("gy255", {"rows.gy255"})):
        others = rest.union(*(v for k, v in per_case.items() if k != name))
        assert cells <= per_case[name] and not cells & others, (name, cells & others)


# ------------------------------------------------------------------------------------------------ division by multiply-high
def test_multiply_high_division_of_the_duplication():
    """duplicate_kernel: floor(local / w) == umulhi(local, 0xFFFFFFFF / w + 1) for local, w < 2^16 -- at every multiple of every w and
    its two neighbours, and exhaustively for the widths a packed rect can have times the locals a 255 x 255 rect can have."""
    ws = np.arange(1, 65536, dtype=np.uint64)
    n = (np.uint64(65536) // ws + np.uint64(2)).astype(np.int64)                   # k = 0 .. 65536 // w + 1
    w = np.repeat(ws, n)
    k = (np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)).astype(np.uint64)
    magic = np.uint64(0xFFFFFFFF) // w + np.uint64(1)
    checked = 0
    for off in (-1, 0, 1):
        local = (k * w).astype(np.int64) + off
        ok = (local >= 0) & (local < 65536)
        l, ww, mg = local[ok].astype(np.uint64), w[ok], magic[ok]
        assert bool(mg[ww > 1].max() < (1 << 32))
        assert np.array_equal((l * mg) >> np.uint64(32), l // ww), off       # (l < 2^16, magic <= 2^32: the product fits 64 bits)
        checked += int(ok.sum())
    assert checked > 2_000_000
    l = np.arange(65536, dtype=np.uint64)
    for w1 in range(2, 256):
        assert np.array_equal((l * np.uint64(0xFFFFFFFF // w1 + 1)) >> np.uint64(32), l // np.uint64(w1)), w1
    # w == 1: the 32-bit magic wraps to 0 (umulhi would give 0 for every local); the kernel's `r.w == 1` branch takes row = local
    assert (0xFFFFFFFF // 1 + 1) & 0xFFFFFFFF == 0


# ------------------------------------------------------------------------------------------------ the write-out's hinted search
def _check_search(widths, CAP):
    wv = np.asarray(widths, np.int64)
    p, top, sh, hint = bc.writeout_search(wv, CAP)
    starts = np.cumsum(wv) - wv
    want = np.searchsorted(starts, np.arange(int(wv.sum())), "right") - 1      # the last p with winc[p] <= q
    assert np.array_equal(p, want), (CAP, wv.size, sh)
    assert top <= CAP + 255, (CAP, wv.size, sh, top)
    return sh, top


@pytest.mark.parametrize("CAP", [1024, 2048])
def test_write_out_search_finds_the_segment_and_stays_inside_winc(CAP):
    """rows_seg_scatter_kernel: word q of a block belongs to the last staged segment p with winc[p] <= q; the search starts at
    hint[q >> sh] and halves from 2^(sh - 1).  Random and worst-case width arrays up to CAP segments of 255 words: the segment is found
    and no read of winc goes past CAP + 255 (the array has CAP + 256 words)."""
    rng = np.random.default_rng(CAP)
    seen = set()
    worst = [np.full(CAP, 255), np.full(CAP, 1), np.r_[np.full(CAP - 1, 255), 1], np.r_[np.full(CAP - 1, 1), 255], np.r_[1, np.full(CAP - 1, 255)],
             np.r_[np.full(CAP // 2, 1), np.full(CAP // 2, 255)], np.r_[np.full(CAP // 2, 255), np.full(CAP // 2, 1)], np.tile([255, 1], CAP // 2),
             np.array([1]), np.array([255]), np.full(33, 255), np.full(8192 // 255 + 1, 255)]
    for wv in worst:
        seen.add(_check_search(wv, CAP)[0])
    for trial in range(60):
        total = int(rng.integers(1, CAP + 1)) if trial % 3 else CAP
        hi = int(rng.choice([2, 4, 9, 17, 64, 256]))
        seen.add(_check_search(rng.integers(1, hi, size=total), CAP)[0])
    # every shift up to the largest this CAP can need, and the top of the array at the largest
    sh_max = bc.hint_shift(CAP * 255)
    assert sh_max == (9 if CAP == 2048 else 8) and seen == set(range(3, sh_max + 1)), seen
    # the top of the array: a last segment that holds a bucket boundary is its own hint (p = CAP - 1), and the first step reads
    # winc[CAP - 1 + 2^(sh - 1)] -- at CAP = 2048 and sh = 9 the last word, winc[CAP + 255]
    tops = [_check_search(np.r_[np.full(j, 1), np.full(CAP - j, 255)], CAP) for j in range(4)]
    assert max(top for sh, top in tops if sh == sh_max) == CAP - 1 + (1 << (sh_max - 1))
    assert (CAP - 1 + (1 << (sh_max - 1)) == CAP + 255) == (CAP == 2048)
