"""What tests/test_gpu_buffer_contract.py relies on, checked without a GPU: the guarded-buffer harness reports what it has to report,
the table of path variants reaches every kernel chain ex4d_api.hip's forward_impl can select, and the layout arithmetic of the three
state buffers (exported host functions; they run without a device) keeps every array -- the two aliased scratch arrays of the tile
sort included -- inside the buffer."""
import ctypes as C
import itertools
import struct

import pytest
import torch

from tests import raw_abi
from tests import test_gpu_buffer_contract as table


# ------------------------------------------------------------------------------------------------ the harness itself
def test_a_byte_written_into_a_guard_is_reported():
    for fill in ("zero", "ones", "finite"):
        bufs = raw_abi.Buffers("cpu")
        g = bufs.prepare("x", 1000, fill)
        assert bufs.guards_intact() == {"x": True}
        assert bool((g.payload == raw_abi.FILL_BYTES[fill]).all()) and g.payload.numel() == 1000
        g.payload[:] = 7                                   # the payload is the call's to write
        assert bufs.guards_intact() == {"x": True}
        g.base[raw_abi.GUARD - 1] ^= 1                      # the byte in front of the payload
        assert bufs.guards_intact() == {"x": [("front", raw_abi.GUARD - 1, 1)]}
        g.base[raw_abi.GUARD - 1] ^= 1
        g.base[raw_abi.GUARD + 1000] ^= 0x80                # the first byte behind it (inside the payload's alignment padding)
        g.base[raw_abi.GUARD + 1000 + raw_abi.GUARD - 1] ^= 1
        assert bufs.guards_intact() == {"x": [("back", 0, 2)]}
        with pytest.raises(AssertionError, match="outside the payload"):
            bufs.assert_guards_intact()
    assert raw_abi.GUARD >= 4096 and raw_abi.GUARD % 256 == 0


def test_a_leftover_fill_element_is_reported():
    assert raw_abi.fill_word("ones") == -1 and raw_abi.fill_word("finite") == 0x3C3C3C3C and raw_abi.fill_word("zero") is None
    as_float = torch.tensor([raw_abi.fill_word("finite")], dtype=torch.int32).view(torch.float32)
    assert 0.0 < float(as_float) < 0.02                     # `finite`: a small plausible float, not NaN
    assert bool(torch.isnan(torch.tensor([-1], dtype=torch.int32).view(torch.float32)).all())
    for fill in ("ones", "finite"):
        g = raw_abi.Buffers("cpu").prepare("x", 4 * 250, fill)
        v = g.view(torch.float32, 50, 5)
        assert raw_abi.leftover_fill(v, fill) == 250
        v[:] = 1.5
        assert raw_abi.leftover_fill(v, fill) == 0
        v.view(torch.int32)[17, 3] = raw_abi.fill_word(fill)
        assert raw_abi.leftover_fill(v, fill) == 1
        assert raw_abi.leftover_fill(v.view(torch.int32), fill) == 1
    assert raw_abi.leftover_fill(torch.zeros(8), "zero") == 0 and raw_abi.leftover_fill(torch.zeros(8), "stale") == 0
    # a value the call computes may have the bits of the `finite` pattern: it is written over zeros as well, a leftover is not
    w = raw_abi.fill_word("finite")
    got = torch.tensor([1, w, w, 5], dtype=torch.int32)
    assert raw_abi.leftover_fill(got, "finite") == 2
    assert raw_abi.leftover_fill(got, "finite", written=torch.tensor([1, w, 0, 5], dtype=torch.int32)) == 1          # bit-reproducible outputs
    x = got.view(torch.float32)
    near = x.clone()
    near[1] *= 1.00001
    near[2] = 0.0
    assert raw_abi.leftover_fill(x, "finite", written=near) == 1                                                       # outputs reproducible to rounding


def test_a_stale_sequence_reuses_storage():
    bufs = raw_abi.Buffers("cpu")
    g = bufs.prepare("x", 4096, "ones")
    ptr = g.payload.data_ptr()
    assert ptr == g.ptr
    g.payload[:] = torch.arange(4096, dtype=torch.int64).to(torch.uint8)
    kept = g.payload.clone()
    g2 = bufs.prepare("x", 1000, "stale")                  # a smaller frame: same storage, nothing touched
    assert g2 is g and g.payload.data_ptr() == ptr and g.payload.numel() == 1000 and torch.equal(g.payload, kept[:1000])
    assert torch.equal(g.base[raw_abi.GUARD: raw_abi.GUARD + 4096], kept) and bufs.guards_intact() == {"x": True, }
    g.base[raw_abi.GUARD + 1000] ^= 1                       # the previous frame's bytes behind the payload are this frame's guard
    assert bufs.guards_intact(["x"]) == {"x": [("back", 0, 1)]}
    g.base[raw_abi.GUARD + 1000] ^= 1
    bufs.prepare("x", 4096, "stale")
    assert g.payload.data_ptr() == ptr and torch.equal(g.payload, kept)
    bufs.prepare("x", 10000, "stale")                      # too small: grown, the old content in front (torch's resize_)
    assert g.payload.data_ptr() != ptr and g.capacity >= 10000 and torch.equal(g.payload[:4096], kept)
    assert bool((g.payload[4096:] == raw_abi.FRESH_BYTE).all())
    bufs.prepare("x", 4096, "zero")                        # any other fill clears payload and guards
    assert int(g.payload.sum()) == 0 and g.requests == [4096, 1000, 4096, 10000, 4096]


# ------------------------------------------------------------------------------------------------ the table reaches every path
# forward_impl's predicates (ex4dgs_amd/csrc/ex4d_api.hip), restated.  None of them is exported; each cites its line.
DLS_MSD_BITS, DLS_IDX_BITS = 10, 13           # ex4d_internal.h: EX4D_DLS_MSD_BITS; ex4d_binning.hip: DLS_IDX_BITS


def float_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def key_bits(min_depth, max_depth):
    """ex4d_api.hip, "depth-sort keys": the visible depths' bit patterns relative to bits(min_depth)"""
    if min_depth >= 0.0 and max_depth > min_depth and max_depth < 3.0e38:
        invisible = float_bits(max_depth) - float_bits(min_depth) + 1
        bits = 1
        while bits < 32 and (invisible >> bits) != 0:
            bits += 1
        return bits
    return 32


def tile_bits(T):
    """ex4d_api.hip: tile_bits"""
    b = 1
    while (1 << b) < T:
        b += 1
    return b


def depth_sort_msd_applies(P, kb):
    """ex4d_binning.hip: ex4d_depth_sort_msd_applies"""
    return P <= (1 << 26) and kb - (DLS_MSD_BITS - 1) + DLS_IDX_BITS <= 32


def depth_sort_msd_bits(P, kb):
    """ex4d_binning.hip: ex4d_depth_sort_msd_bits"""
    narrow = DLS_MSD_BITS - 1
    return narrow if (P <= 1300000 and kb - (narrow - 1) + DLS_IDX_BITS <= 32) else DLS_MSD_BITS


def tile_sort_msd_applies(P, tb):
    """ex4d_binning.hip: ex4d_tile_sort_msd_applies"""
    return 9 <= tb <= 16 and P <= (1 << (32 - (tb + 1) // 2))


def path_signature(P, W, H, min_depth, max_depth, opts, asynchronous):
    """Which kernel chain forward_impl selects (outside a graph capture, the auto mode not on hold):
    (packed_rects, depth sort, its digit width, tile sort, fused_scan, lsd_gather, asynchronous)"""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    kb = key_bits(min_depth, max_depth)
    packed_rects = gx <= 255 and gy <= 255                                                        # "packed_rects"
    msd_mode = opts["depth_sort_msd"]
    if not (packed_rects and depth_sort_msd_applies(P, kb)):
        msd_mode = 0
    elif msd_mode == 3:
        msd_mode = 2                                                                              # depth_sort_auto_msd
    msd_bits = depth_sort_msd_bits(P, kb)
    forced = opts["depth_sort_msd_bits"]
    if forced == DLS_MSD_BITS or (forced == DLS_MSD_BITS - 1 and depth_sort_msd_bits(1, kb) == forced):
        msd_bits = forced
    rows_sort = opts["tile_sort_rows"] != 0 and gx <= 255 and gy <= 255 and P <= (1 << 24)        # ex4d_rowsort.hip: ex4d_tile_sort_rows_applies
    fused_scan = msd_mode == 2 and not rows_sort
    lsd_gather = msd_mode == 0 and rows_sort and packed_rects
    tile = "rows" if rows_sort else ("msd pair" if tile_sort_msd_applies(P, tile_bits(gx * gy)) else "radix pair")
    depth = {0: "lsd", 1: "msd + scan kernel", 2: "msd"}[msd_mode]
    return (packed_rects, depth, msd_bits if msd_mode else None, tile, fused_scan, lsd_gather, bool(asynchronous))


def variant_signature(v):
    P, W, H, lo, hi = table.scene_shape(v.scene)
    return path_signature(P, W, H, lo, hi, dict(table.BASE_OPTIONS, **v.options), v.extras.get("asynchronous"))


def test_the_options_the_table_sets_exist_with_these_defaults():
    from ex4dgs_amd import _C
    for k, val in table.BASE_OPTIONS.items():
        assert _C.get_option(k) == val, k                    # (no test has run in this process that leaves an option changed)


def test_restated_predicates_on_known_frames():
    assert key_bits(4.0, 300.0) == 26 and key_bits(0.01, 300.0) == 27 and key_bits(0.001, 300.0) == 28 and key_bits(0.0, 300.0) == 31
    assert key_bits(-1.0, 300.0) == 32 and key_bits(4.0, 3.4e38) == 32
    assert tile_bits(85 * 64) == 13 and tile_bits(48) == 6 and tile_bits(257 * 257) == 17 and tile_bits(257 * 2) == 10 and tile_bits(128 * 68) == 14
    d = dict(table.BASE_OPTIONS)
    assert path_signature(1_000_000, 1352, 1014, 4.0, 300.0, d, False) == (True, "msd", 9, "rows", False, False, False)      # what bench.py times
    assert path_signature(2_000_000, 1352, 1014, 4.0, 300.0, d, False)[2] == 10
    assert path_signature(1000, 1352, 1014, 0.001, 300.0, dict(d, depth_sort_msd_bits=9), False)[2] == 10       # a forced 9 that does not fit
    assert path_signature(1000, 1352, 1014, 0.0, 300.0, d, False)[1] == "lsd"                                   # 31 key bits: no MSD sort
    assert path_signature(1500, 4112, 4112, 4.0, 300.0, d, True) == (False, "lsd", None, "radix pair", False, False, True)


def test_the_table_reaches_every_kernel_chain():
    """Every chain forward_impl can select -- over image classes (<= 256 tiles / 9..16 tile bits / a side above 255 tiles with and
    without more than 16 tile bits), key widths (26, 27, 28, 31 bits), every value of the three options that pick a chain, both
    kinds of forward -- has an entry in the table.  A new path (another value of an option, another predicate) without a table
    entry fails here."""
    images = [(1352, 1014), (2048, 1088), (128, 96), (131, 67), (4112, 32), (4112, 4112)]
    depths = [(4.0, 300.0), (0.01, 300.0), (0.001, 300.0), (0.0, 300.0)]
    possible = set()
    for (W, H), (lo, hi), msd, bits, rows, asyn in itertools.product(images, depths, (0, 1, 2, 3), (0, 9, 10), (0, 1), (False, True)):
        possible.add(path_signature(2049, W, H, lo, hi, dict(table.BASE_OPTIONS, depth_sort_msd=msd, depth_sort_msd_bits=bits, tile_sort_rows=rows), asyn))
    reached = {variant_signature(v) for v in table.VARIANTS}
    assert len(possible) == 34                               # 2 x (2 + 2 + 1 depth chains) x 3 tile chains behind packed rects + 2 x 2 behind 8-byte rects
    missing = possible - reached
    assert not missing, f"kernel chains without a table entry: {sorted(missing, key=str)}"
    assert reached <= possible, f"the table claims chains the host code cannot select: {sorted(reached - possible, key=str)}"
    # the switches that do not pick a chain but a kernel variant inside it
    opt = lambda v: dict(table.BASE_OPTIONS, **v.options)
    for k in ("geom_debug_arrays", "binning_tile_ids"):
        assert {opt(v)[k] for v in table.VARIANTS} == {0, 1}, k
    ballots = {variant_signature(v)[1:4:2] for v in table.VARIANTS if opt(v)["rank_lds_atomics"] == 0}
    assert {("msd", "rows"), ("lsd", "msd pair"), ("msd", "radix pair")} <= ballots          # every scatter kernel that ranks
    through_memory = {variant_signature(v)[1:5] for v in table.VARIANTS if opt(v)["depth_sort_local_cap"] or v.scene is table.WALL}
    assert {("msd", 9, "rows", False), ("msd", 9, "msd pair", True), ("msd + scan kernel", 9, "msd pair", False)} <= through_memory
    x = [v.extras for v in table.VARIANTS]
    assert {e.get("dir", "rand") for e in x} == {"rand", "zero", "null"}
    assert {bool(e.get("assume_no_flow")) for e in x if e.get("asynchronous")} == {False, True}
    for k in ("colors_precomp", "cov3D_precomp", "sh4", "subpixel", "prepare_backward"):
        assert any(e.get(k) for e in x) and any(not e.get(k) for e in x), k
    statics = {(e["n_static"], table.scene_shape(v.scene)[0]) for v, e in zip(table.VARIANTS, x) if e.get("n_static") is not None}
    assert any(n == 0 for n, P in statics) and any(n == P for n, P in statics) and any(0 < n < P and n % 64 for n, P in statics)
    for v in table.VARIANTS:
        if v.extras.get("assume_no_flow"):
            assert v.extras.get("dir") == "zero" and v.extras.get("asynchronous")
    assert {v.name for v in table.BWD_VARIANTS} >= {"cfg1 defaults", "cfg3 test options", "nothing visible", "cfg1 split SH, empty static part"}


# ------------------------------------------------------------------------------------------------ layout arithmetic
def _layouts(P, R, W, H):
    from ex4dgs_amd import _C
    lib = _C.load()
    g, b, i = _C.GeomLayout(), _C.BinningLayout(), _C.ImgLayout()
    lib.ex4d_geom_layout(P, C.byref(g))
    lib.ex4d_binning_layout(R, W, H, C.byref(b))
    lib.ex4d_img_layout(W, H, C.byref(i))
    as_dict = lambda s: {n: int(getattr(s, n)) for n, _ in s._fields_}
    return lib, as_dict(g), as_dict(b), as_dict(i)


SIZES = [(1, 0, 16, 16), (1, 1, 131, 67), (256, 16, 256, 256), (257, 17, 128, 96), (12000, 90_000, 1352, 1014), (1500, 400_000, 4112, 4112),
         (1_000_000, 7_500_000, 1352, 1014), (2_000_000, 31_500_000, 2048, 1088)]


@pytest.mark.parametrize("P,R,W,H", SIZES)
def test_totals_and_offsets_of_the_state_buffers(P, R, W, H):
    lib, g, b, i = _layouts(P, R, W, H)
    assert g["total"] == lib.ex4d_geom_bytes(P) and b["total"] == lib.ex4d_binning_bytes(R, W, H) and i["total"] == lib.ex4d_img_bytes(W, H)
    assert lib.ex4d_backward_scratch_bytes(P) == (64 * P + 255) // 256 * 256
    T = ((W + 15) // 16) * ((H + 15) // 16)
    n = max(R, 1)
    # every reported array: 256-byte aligned, in carving order, its elements in front of the next one
    sizes = dict(records=64 * P, cov3D=24 * P, clamped=P, tiles_touched=4 * P, rects=8 * P, depth_order=4 * P, sorted_offsets=4 * P,
                 point_list=4 * n, tile_ids=4 * n, qlist=16 * n, qcount=16 * T, final_T=4 * W * H, n_contrib=4 * W * H, ranges=8 * T)
    for lay, order in ((g, ("records", "cov3D", "clamped", "tiles_touched", "rects", "depth_order", "sorted_offsets")),
                       (b, ("point_list", "tile_ids", "qlist", "qcount")), (i, ("final_T", "n_contrib", "ranges"))):
        assert lay[order[0]] == 0 and lay["total"] % 256 == 0
        offs = [lay[k] for k in order] + [lay["total"]]
        for k, a, nxt in zip(order, offs, offs[1:]):
            assert a % 256 == 0 and a + sizes[k] <= nxt, (k, a, sizes[k], nxt)
    assert b["qcount"] + 16 * T <= b["total"] and i["ranges"] + 8 * T <= i["total"]


def test_sizes_are_monotone_in_P_and_R():
    from ex4dgs_amd import _C
    lib = _C.load()
    Ps = [1, 2, 63, 64, 65, 255, 256, 257, 2048, 2049, 4096, 4097, 12000, 100_000, 1_000_000, 1_300_001, 2_100_000]
    Rs = [0, 1, 16, 17, 4095, 4096, 4097, 65536, 1_000_000, 7_500_000, 31_500_000]
    for f, xs in ((lib.ex4d_geom_bytes, Ps), (lib.ex4d_backward_scratch_bytes, Ps)):
        v = [f(x) for x in xs]
        assert all(a <= b for a, b in zip(v, v[1:])) and v[0] > 0, (f, v)
    for W, H in ((16, 16), (131, 67), (1352, 1014), (4112, 4112)):
        v = [lib.ex4d_binning_bytes(R, W, H) for R in Rs]
        assert all(a <= b for a, b in zip(v, v[1:])) and v[0] > 0
    assert lib.ex4d_img_bytes(16, 16) <= lib.ex4d_img_bytes(131, 67) <= lib.ex4d_img_bytes(1352, 1014) <= lib.ex4d_img_bytes(4112, 4112)


@pytest.mark.parametrize("R", [0, 1, 16, 17, 31, 32, 63, 64, 65, 4097, 7_500_000])
@pytest.mark.parametrize("W,H", [(16, 16), (131, 67), (1352, 1014)])
def test_aliased_tile_sort_scratch_ends_inside_the_buffer(R, W, H):
    """carve_binning (ex4d_api.hip): vals_tmp = qlist, keys_tmp = qlist + align256(4 n) bytes, n = max(R, 1) words each.  They end
    inside the compacted-list region from n = 17 on; up to 16 instances keys_tmp is the first n words of the qcount region (both
    are scratch until the compositing forward, which writes every qcount word itself) -- inside the buffer either way."""
    _, _, b, _ = _layouts(1, R, W, H)
    n = max(R, 1)
    align = lambda x: (x + 255) // 256 * 256
    vals_end = b["qlist"] + 4 * n
    keys_tmp = b["qlist"] + align(4 * n)
    keys_end = keys_tmp + 4 * n
    assert vals_end <= keys_tmp and vals_end <= b["qcount"]
    assert keys_end <= b["total"]
    assert (keys_end <= b["qcount"]) == (n >= 17)
    if n <= 16:
        T = ((W + 15) // 16) * ((H + 15) // 16)
        assert keys_tmp == b["qcount"] and keys_end <= b["qcount"] + align(16 * T)
