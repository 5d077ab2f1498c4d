"""Resizing decoded frames as PIL does, without a GPU (include/ex4d_loss.h "RESIZING", ex4dgs_amd/frames.py): the numpy restatement
against Pillow's recorded and live bytes, the library's host-built coefficient tables against the restatement word for word, the
refusals, reference_size, and the tiling constants the GPU cases are built around."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from ex4dgs_amd import _abi, frames
from tests import resize_cases as rc
from tests import resize_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "resize.npz"))
BIG = 16384


@pytest.fixture(scope="module")
def lib():
    from ex4dgs_amd import build
    build.build()
    return _abi.load()


# ------------------------------------------------------------------------------------------------ the restatement is PIL
@pytest.mark.parametrize("case", rc.NAMED, ids=rc.case_id)
def test_restatement_equals_the_recorded_pillow_bytes(case):
    for content, make in rc.CONTENT.items():
        src = GOLDEN[f"{rc.case_id(case)}/{content}/in"]
        assert np.array_equal(src, make(case[0], case[1])), "the fixture's input is the generator's"
        for f in rc.FILTERS:
            want = GOLDEN[f"{rc.case_id(case)}/{content}/{f}"]
            got = rr.resize(src, case[2:], f)
            assert got.shape == want.shape and np.array_equal(got, want), (case, content, f, int((got != want).sum()))


def test_recorded_frames_are_the_restatement():
    for a, b in zip(GOLDEN["frames/in"], GOLDEN["frames/out"]):
        assert np.array_equal(rr.resize(a, b.shape[:2]), b)


@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
def test_restatement_equals_live_pillow(case):
    Image = pytest.importorskip("PIL.Image")
    for content, make in rc.CONTENT.items():
        src = make(case[0], case[1])
        for f in rc.FILTERS:
            want = np.asarray(Image.fromarray(src).resize((case[3], case[2]), resample=rr.FILTERS[f]))
            assert np.array_equal(rr.resize(src, case[2:], f), want), (case, content, f)


def test_bicubic_on_the_saturating_pattern_reaches_both_clamps():
    for case in rc.NAMED:
        src = rc.saturating(case[0], case[1])
        if case[1] != case[3]:
            acc = rr.accumulate(np.ascontiguousarray(src.transpose(1, 0, 2)), case[3], "bicubic") >> rr.BITS
            if acc.min() < 0 and acc.max() > 255:
                return
    raise AssertionError("no case reaches both clamps")


# ------------------------------------------------------------------------------------------------ the host-built tables
def _library_table(lib, n_in, n_out, filt):
    words = np.full(lib.ex4d_resize_u8_table_words(n_in, n_out, filt) + 2, -7, dtype=np.int32)     # two guard words
    _abi.call("ex4d_resize_u8_table", n_in, n_out, filt, words.ctypes.data)
    assert words[-1] == -7 and words[-2] == -7, "the builder wrote past its word count"
    return words[:-2]


@pytest.mark.parametrize("resample", rc.FILTERS)
def test_tables_equal_the_restatement_word_for_word(lib, resample):
    filt = rr.FILTERS[resample]
    pairs = [(a, b) for a in range(1, 49) for b in range(1, 49)] + [(2704, 1352), (2028, 1014), (2704, 338), (1352, 2704)]
    for n_in, n_out in pairs:
        want = rr.table_words(n_in, n_out, resample)
        assert lib.ex4d_resize_u8_table_words(n_in, n_out, filt) == want.size, (n_in, n_out)
        got = _library_table(lib, n_in, n_out, filt)
        assert np.array_equal(got, want), (resample, n_in, n_out, np.flatnonzero(got != want)[:5])


def test_table_layout_and_sums(lib):
    """ksize first, then out entries of xmin, n, ksize coefficients: taps inside the input, unused coefficients zero, the
    coefficients of an element sum to 2^22 within one unit per tap."""
    for resample, (n_in, n_out) in [("bilinear", (2704, 1352)), ("bicubic", (23, 7)), ("box", (8, 16)), ("bilinear", (100, 1))]:
        w = _library_table(lib, n_in, n_out, rr.FILTERS[resample])
        ksize = int(w[0])
        body = w[1:].reshape(n_out, ksize + 2)
        assert (body[:, 0] >= 0).all() and (body[:, 1] >= 1).all() and (body[:, 0] + body[:, 1] <= n_in).all() and (body[:, 1] <= ksize).all()
        for row in body:
            assert (row[2 + row[1]:] == 0).all() and abs(int(row[2:].sum()) - (1 << 22)) <= row[1]
    assert int(_library_table(lib, 100, 1, 2)[0]) == 201


# ------------------------------------------------------------------------------------------------ refusals (pure host code)
def test_library_refusals(lib):
    words = np.zeros(64, dtype=np.int32)
    for n_in, n_out, filt, text in [(0, 4, 2, "16384"), (4, 0, 2, "16384"), (-1, 4, 2, "16384"), (BIG + 1, 4, 2, "16384"), (4, BIG + 1, 2, "16384"),
                                    (4, 2, 1, "unknown filter"), (4, 2, 0, "unknown filter"), (4, 2, 5, "unknown filter")]:
        assert lib.ex4d_resize_u8_table_words(n_in, n_out, filt) == 0
        with pytest.raises(RuntimeError, match=text):
            _abi.call("ex4d_resize_u8_table", n_in, n_out, filt, words.ctypes.data)
        assert text in lib.ex4d_loss_last_error().decode()
    assert lib.ex4d_resize_u8_table_words(BIG, 1, 2) == 1 + (2 * BIG + 1 + 2) and lib.ex4d_resize_u8_table_words(1, BIG, 3) == 1 + BIG * 7
    assert lib.ex4d_resize_u8_scratch_bytes(2028, 2704, 1014, 1352) == 2028 * 1352 * 3
    assert lib.ex4d_resize_u8_scratch_bytes(BIG, BIG, 1, BIG - 1) == BIG * (BIG - 1) * 3         # above 2^31: a size_t
    assert lib.ex4d_resize_u8_scratch_bytes(9, 9, 9, 4) == 0 and lib.ex4d_resize_u8_scratch_bytes(9, 9, 4, 9) == 0
    assert lib.ex4d_resize_u8_scratch_bytes(0, 9, 4, 4) == 0 and lib.ex4d_resize_u8_scratch_bytes(9, 9, 4, BIG + 1) == 0
    # refused before any device call: the pointers are never used
    one = ctypes.c_void_p(1)
    for args, text in [((4, 4, 2, 2, 4), "premultiplied"), ((4, 4, 2, 2, 1), "pixel_stride"), ((0, 4, 2, 2, 3), "16384"),
                       ((4, 4, 2, BIG + 1, 3), "16384"), ((4, -3, 2, 2, 3), "16384")]:
        with pytest.raises(RuntimeError, match=text):
            _abi.call("ex4d_resize_u8", *args, one, one, one, one, one, None)
    with pytest.raises(RuntimeError, match="null"):
        _abi.call("ex4d_resize_u8", 4, 4, 2, 2, 3, one, one, one, one, None, None)
    with pytest.raises(RuntimeError, match="null"):
        _abi.call("ex4d_resize_u8", 4, 4, 4, 2, 3, one, one, None, None, None, None)
    assert lib.ex4d_abi_version() == 5


def test_python_refusals():
    for bad in [((0, 4), (2, 2)), ((4, 4), (2, BIG + 1)), ((4, BIG + 1), (2, 2))]:
        with pytest.raises(RuntimeError, match="16384"):
            frames.resize_plan(*bad)
    with pytest.raises(RuntimeError, match="lanczos"):
        frames.resize_plan((4, 4), (2, 2), resample="lanczos")
    with pytest.raises(RuntimeError, match="premultiplied"):
        frames.resize_u8(torch.zeros(4, 4, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frames.resize_u8(torch.zeros(4, 4, 3, dtype=torch.uint8), out=torch.zeros(2, 2, 3, dtype=torch.uint8))
    for make in (lambda: frames.FrameStore(2, 4, 4, pixel_stride=4, source_size=(8, 8)),
                 lambda: frames.FrameStream(4, 4, pixel_stride=4, source_size=(8, 8))):
        with pytest.raises(RuntimeError, match="pixel_stride 3.*premultiplied"):
            make()


# ------------------------------------------------------------------------------------------------ the size the reference resizes to
def test_reference_size_of_each_branch():
    rs = frames.reference_size
    assert rs(2704, 2028, 2) == (1352, 1014) and rs(2704, 2028, 1) == (2704, 2028) and rs(2704, 2028, 8) == (338, 254)   # 253.5 rounds to even
    assert rs(1001, 751, 2) == (500, 376)                    # Python's round: 500.5 -> 500, 375.5 -> 376
    assert rs(2704, 2028, 4, resolution_scale=2.0) == (338, 254)
    assert rs(2704, 2028, -1) == (1600, 1200)                # wider than 1600: global_down = 1.69
    assert rs(1352, 1014, -1) == (1352, 1014)
    assert rs(1352, 1014, -1, resolution_scale=2.0) == (676, 507)
    assert rs(2704, 2028, 800) == (800, 600) and rs(1001, 751, 333) == (333, 249)      # an explicit width: 751 / (1001 / 333) = 249.8
    assert rs(2704, 2028, 2, ss=True) == (1352, 1014) and rs(2705, 2029, 1, ss=True) == (1352, 1014)
    assert rs(2704, 2028, -1, ss=True) == (1352, 1014)


# ------------------------------------------------------------------------------------------------ tiling constants and their cases
def test_tiling_constants_mirror_the_header_and_have_their_edge_cases():
    text = open(os.path.join(ROOT, "include", "ex4d_loss.h")).read()
    header = {n: int(v) for n, v in re.findall(r"^#define[ \t]+(EX4D_RESIZE_\w+)[ \t]+(\d+)[ \t]*$", text, flags=re.M)}
    assert header == {n: v for n, (v, _) in rc.TILING.items()} and len(header) == 4
    axis = {"W_out": lambda c: c[3], "H_in": lambda c: c[0] if c[1] != c[3] else None, "H_out": lambda c: c[2] if c[0] != c[2] else None,
            "3 W_out": lambda c: c[3] if c[0] != c[2] else None}
    for name, (T, ax) in rc.TILING.items():
        sizes = {axis[ax](c) for c in rc.CASES}
        assert {T - 1, T, T + 1} <= sizes, (name, T)
    bytes_per_row = {3 * c[3] for c in rc.CASES if c[0] != c[2]}
    T = rc.TILING["EX4D_RESIZE_V_BYTES"][0]
    assert {T - 4, T - 1, T + 2} <= bytes_per_row             # the rows of whole pixels nearest to one tile of bytes
    assert (header["EX4D_RESIZE_H_PIXELS"] * header["EX4D_RESIZE_H_ROWS"], header["EX4D_RESIZE_V_BYTES"] // 4 * header["EX4D_RESIZE_V_ROWS"]) == (256, 256)
    assert frames.MAX_SIZE == BIG and frames.RESAMPLE == rr.FILTERS
    assert (len(rc.CASES), len(set(rc.CASES))) == (len(rc.NAMED) + len(rc.TILING_CASES),) * 2


# ------------------------------------------------------------------------------------------------ the built objects
def test_no_object_holds_a_packed_shift_clamp(lib):
    """v_ashr_pk_*: the compiler uses its destination's upper 16 bits as zero and the MI355X leaves them as they were (the vertical
    pass once stored bytes 2 and 3 of every dword OR-ed with an accumulator's upper half).  The build refuses such an object; this
    holds the objects as built to it, the resize kernels' first of all."""
    from ex4dgs_amd import build, isa_check
    objs = [os.path.join(build.CSRC, s.replace(".hip", ".o")) for s in build.SOURCES]
    assert "ex4d_frames.hip" in build.SOURCES and "-ffp-contract=off" in build.SOURCES["ex4d_frames.hip"]
    for o in objs:
        assert os.path.exists(o) and isa_check.packed_shift_clamps(o) == [], o
