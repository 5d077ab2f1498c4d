"""scikit-image's SSIM of a rendered view without a GPU (include/ex4d_loss.h: ex4d_frame_skssim / _u8; ex4dgs_amd/evaluate.py): the
entry points are declared, exported and sized; every refusal arrives with its message before any HIP call; the two formulations of the
reference agree; a float32 evaluation of the formula reaches the bar on every test input with fourfold room; the report aggregation
with sk_rows is render.py's arithmetic, and without them it is what it was."""
import ctypes
import os

import numpy as np
import pytest
import torch

from ex4dgs_amd import _abi
from tests import skssim_cases as sc
from tests import skssim_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ex4d_frame_skssim_scratch_floats", "ex4d_frame_skssim", "ex4d_frame_skssim_u8")
CASES = [("pair", H, W, clamp) for H, W in sc.SHAPES for clamp in (False, True)] + [("low", *sc.LOW_VARIANCE_SHAPE, False)] + \
        [(kind, *sc.ODD[0], False) for kind in ("u8", "u8_1.7")]


def test_the_table_declares_the_entry_points_and_the_library_exports_them():
    from ex4dgs_amd import build, evaluate, loss
    exports = _abi.exports("ex4d_loss.h")
    assert exports[-3:] == NEW and set(exports) == set(loss.EXPORTS)
    status = {name for _, protos in _abi.PROTOTYPES.values() for name, _, _, is_status in protos if is_status}
    assert set(NEW[1:]) <= status and NEW[0] not in status
    handle = ctypes.CDLL(build.build())
    for name in NEW:
        assert hasattr(handle, name), name
    header = open(os.path.join(ROOT, "include", "ex4d_loss.h")).read()
    assert f"#define EX4D_SKSSIM_WINDOW {evaluate.SK_WINDOW}\n" in header and evaluate.SK_WINDOW == sc.WIN == sr.WIN == 7
    assert [header.index(name + "(") for name in NEW] == sorted(header.index(name + "(") for name in NEW)
    assert header.index("ex4d_frame_metrics_u8(") < header.index(NEW[0] + "(")
    assert (evaluate.SK_ROW, evaluate.SKSSIM, evaluate.SKSSIM2, evaluate.SK_NONFINITE) == (4, 0, 1, 2)
    assert sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h")) == sorted(_abi.PROTOTYPES)


def test_scratch_size_is_three_partials_per_workgroup_of_the_padded_grid():
    lib = _abi.load()
    for H, W in sc.SHAPES + ((1014, 1352),):
        assert lib.ex4d_frame_skssim_scratch_floats(H, W) >= 3 * sc.blocks(H, W), (H, W)
    assert sc.blocks(1014, 1352) == 464 and sc.blocks(7, 7) == 8


def test_the_calls_refuse_before_any_hip_call():
    """Fake non-NULL pointers are never dereferenced: the call returns on its argument check."""
    lib = _abi.load()
    p = 4096
    good = [8, 8, p, p, 0, p, p, None]
    good_u8 = [8, 8, p, p, 3, None, 0, p, p, None]

    def refused(name, args, match):
        with pytest.raises(RuntimeError) as e:
            _abi.call(name, *args)
        assert str(e.value) == lib.ex4d_loss_last_error().decode() != "" and match in str(e.value), str(e.value)

    for hole in (2, 3, 5, 6):                                          # img, gt, row, scratch
        refused("ex4d_frame_skssim", good[:hole] + [None] + good[hole + 1:], "bad argument")
    for hole in (2, 3, 7, 8):
        refused("ex4d_frame_skssim_u8", good_u8[:hole] + [None] + good_u8[hole + 1:], "bad argument")
    for H, W in ((6, 8), (8, 6), (0, 8), (8, -1), (6, 6)):
        refused("ex4d_frame_skssim", [H, W] + good[2:], "win_size exceeds image extent")
        refused("ex4d_frame_skssim_u8", [H, W] + good_u8[2:], "win_size exceeds image extent")
    for stride in (5, 0, 1, 2, -3):
        refused("ex4d_frame_skssim_u8", good_u8[:4] + [stride] + good_u8[5:], "pixel_stride")
    for flags in (2, 3, 4, 8, -1):                                     # 2 is EX4D_METRICS_QUANT_TRUNC: no bytes are written here
        refused("ex4d_frame_skssim", good[:4] + [flags] + good[5:], "flags")
        refused("ex4d_frame_skssim_u8", good_u8[:6] + [flags] + good_u8[7:], "flags")
    assert lib.ex4d_frame_skssim(*good[:5], None, *good[6:]) == 1      # EX4D_ERR_ARG
    assert lib.ex4d_frame_skssim_scratch_floats(6, 100) == 0 == lib.ex4d_frame_skssim_scratch_floats(100, 6)


def test_the_python_layer_refuses_the_cpu():
    from ex4dgs_amd import evaluate
    x = torch.zeros(3, 8, 8)
    with pytest.raises(RuntimeError, match="frame_skssim has no CPU fallback"):
        evaluate.frame_skssim(x, x)
    with pytest.raises(RuntimeError, match="ROCm"):
        evaluate.Evaluator(2, 8, 8, device="cpu", skssim=True)


def test_the_shape_list_covers_what_it_promises():
    shapes = set(sc.SHAPES)
    assert (7, 7) in shapes and any(H == 7 and W > 7 for H, W in shapes) and any(W == 7 and H > 7 for H, W in shapes)
    assert {W - 6 for _, W in sc.STRIP_EDGE} == {sc.SW, sc.SW + 1} and {H - 6 for H, _ in sc.SEGMENT_EDGE} == {sc.SEG, sc.SEG + 1}
    assert sorted((sc.last_rows_out(H) + 6) % sc.RPI for H, _ in sc.REMAINDER) == [0, 1, 2, 3]
    assert all(0 < W - 6 - sc.SW < sc.HALO for _, W in sc.REMAINDER)
    assert sorted(sc.work_items(H, W) for H, W in sc.WORK_ITEM_SHAPES) == [1, 7, 8, 9, 17, 17] and (53, 139) in shapes
    assert sc.TRANSPOSED in shapes and sc.TRANSPOSED[::-1] in shapes
    with pytest.raises(ValueError, match="win_size exceeds image extent"):
        sr.skssim(np.zeros((3, 6, 9), np.float32), np.zeros((3, 6, 9), np.float32), 1)


@pytest.mark.parametrize("kind, H, W, clamp", CASES)
def test_the_references_agree_and_float32_has_fourfold_room(kind, H, W, clamp):
    """scipy's uniform filter against window means without scipy, in float64; and the formula in float32 against float64: the
    evidence that the bar is about the kernel, not about the number format, on exactly the inputs the GPU test uses."""
    from tests import metrics_ref as mr
    image, gt = sr.pair(kind, H, W)
    ref = sr.case(kind, H, W, clamp)
    scored = mr.clamp01(image) if clamp else image
    other = sr.skssim_windows(scored, gt, 1), sr.skssim_windows(scored, gt, 2)
    f32 = sr.both(image, gt, clamp, dtype=np.float32)
    print((kind, H, W, clamp), ref, [abs(a - b) for a, b in zip(ref, other)], [abs(a - b) for a, b in zip(ref, f32)])
    assert all(abs(a - b) <= 1e-13 for a, b in zip(ref, other))
    assert all(abs(a - b) <= sc.TOL / 4 for a, b in zip(ref, f32))
    assert all(0.0 < v < 1.0 for v in ref) and ref[0] < ref[1]


def test_the_transposed_pair_has_the_same_reference():
    H, W = sc.TRANSPOSED
    image, gt = sr.pair("pair", H, W)
    t = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1))
    assert all(abs(a - b) <= 1e-13 for a, b in zip(sr.both(image, gt), sr.both(t(image), t(gt))))


def test_equal_images_score_one_in_the_reference():
    image, _ = sr.pair("pair", 20, 30)
    assert sr.both(image, image) == (1.0, 1.0)


def test_report_aggregation_with_sk_rows_is_render_pys_arithmetic():
    from ex4dgs_amd import evaluate
    rows = np.zeros((3, 8))
    rows[:, evaluate.L1] = [0.1, 0.25, 1.0 / 3.0]
    rows[:, evaluate.PSNR] = [30.123456789, 28.7, 41.000001]
    rows[:, evaluate.SSIM] = [0.9, 0.87654321, 0.5]
    sk = np.zeros((3, 4))
    sk[:, evaluate.SKSSIM] = [0.912345678, 0.8, 2.0 / 3.0]
    sk[:, evaluate.SKSSIM2] = [0.95, 0.887654321, 0.7]
    sk[:, evaluate.SK_NONFINITE] = 5.0                                 # not reported
    names = ["cam00_0001.png", "cam00_0002.png", "cam01_0001.png"]
    before = evaluate.aggregate(rows, names)
    assert list(before[0]) == ["SSIM", "PSNR", "L1"] == list(before[1])
    assert evaluate.aggregate(rows, names, None) == before
    mean, per_view = evaluate.aggregate(rows, names, sk)
    assert list(mean) == ["SSIM", "PSNR", "L1", "SKSSIM", "SKSSIM2"] == list(per_view)
    assert ({k: mean[k] for k in before[0]}, {k: per_view[k] for k in before[1]}) == before
    for key, col in (("SKSSIM", evaluate.SKSSIM), ("SKSSIM2", evaluate.SKSSIM2)):
        collected = [float(v) for v in sk[:, col]]                     # render.py:78-79 appends Python floats (numpy float64 scalars)
        assert mean[key] == torch.tensor(collected).mean().item()      # :100-101: a float32 tensor, its float32 mean
        assert per_view[key] == {name: v for v, name in zip(torch.tensor(collected).tolist(), names)}       # :113-114
        assert list(per_view[key]) == names and mean[key] != float(np.mean(collected))
    with pytest.raises(RuntimeError, match="sk_rows"):
        evaluate.aggregate(rows, names, sk[:2])
