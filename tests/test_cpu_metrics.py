"""Scoring rendered views without a GPU (include/ex4d_loss.h: ex4d_frame_metrics / _u8; ex4dgs_amd/evaluate.py): the bars of
tests/metrics_ref.py are reachable -- by the reference's own float32 functions on the golden inputs (tests/golden/metrics.npz,
captured by tests/golden/make_golden_metrics.py) and by a float32 evaluation over the whole shape list --, the report aggregation is
render.py's arithmetic, and the calls refuse bad arguments before any HIP call."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from ex4dgs_amd import _abi
from tests import metrics_ref as mr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW = ("ex4d_frame_metrics_scratch_floats", "ex4d_frame_metrics", "ex4d_frame_metrics_u8")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "metrics.npz")), np.load(os.path.join(GOLDEN, "frames.npz"))


def test_the_table_declares_the_entry_points_and_the_library_exports_them():
    from ex4dgs_amd import build, evaluate, loss
    assert set(NEW) <= set(_abi.exports("ex4d_loss.h")) == set(loss.EXPORTS)
    status = {name for _, protos in _abi.PROTOTYPES.values() for name, _, _, is_status in protos if is_status}
    assert set(NEW[1:]) <= status and NEW[0] not in status
    handle = ctypes.CDLL(build.build())
    for name in NEW:
        assert hasattr(handle, name), name
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "ex4d_loss.h")).read()
    assert f"#define EX4D_METRICS_CLAMP {evaluate.METRICS_CLAMP}\n" in header
    assert f"#define EX4D_METRICS_QUANT_TRUNC {evaluate.METRICS_QUANT_TRUNC}\n" in header
    assert evaluate.metrics_flags() == 0 and evaluate.metrics_flags(True, "trunc") == 3
    with pytest.raises(RuntimeError, match="quant"):
        evaluate.metrics_flags(False, "floor")


def test_scratch_size_is_four_partials_per_workgroup_of_the_padded_grid():
    from tests import loss_cases
    lib = _abi.load()
    for H, W in mr.SHAPES + ((1014, 1352),):
        blocks = 8 * ((loss_cases.work_items(H, W) + 7) // 8)
        assert lib.ex4d_frame_metrics_scratch_floats(H, W) >= 4 * blocks, (H, W)


def test_the_references_own_float32_values_lie_within_the_bars(golden):
    """The reference's psnr / ssim / l1_loss in float32 against metrics_ref in float64, on the golden image: unclamped as render.py
    scores, clamped as train.py does; and train.py:101's bytes are metrics_ref.quant_trunc's."""
    from ex4dgs_amd.frames import gt_lut
    g, frames = golden
    render, u8 = g["render"], frames["rgb_u8"]
    assert render.dtype == np.float32 and render.shape == (3, 53, 139) and render.min() < 0 and render.max() > 1
    assert g["im_scales"].tolist() == [1.0, 1.7]
    for k, im_scale in enumerate(g["im_scales"].tolist()):
        gt = mr.looked_up(u8, gt_lut(im_scale))
        for tag, clamp in (("", False), ("_clamped", True)):
            ref = mr.metrics(render, gt, clamp)
            row = [float(g[f"l1{tag}_{k}"]), ref["mse"], float(g[f"psnr{tag}_{k}"]), float(g[f"ssim{tag}_{k}"]), 0, 0.0, 0.0, 0.0]
            mr.within_bars(row, ref, (im_scale, tag))
    assert np.array_equal(g["bytes_trunc"], mr.quant_trunc(render))
    assert np.array_equal(mr.quant_trunc(mr.clamp01(render)), mr.quant_trunc(render))
    assert not np.array_equal(mr.quant_round(render), mr.quant_trunc(render))


@pytest.mark.parametrize("H, W", mr.SHAPES)
def test_a_float32_evaluation_stays_within_the_bars(H, W):
    image, gt = mr.make_pair(H, W)
    assert image.min() < 0 or H * W < 4
    for clamp in (False, True):
        ref = mr.case(H, W, "float", clamp)
        f32 = mr.metrics(image, gt, clamp, dtype=torch.float32)
        mr.within_bars([f32["l1"], f32["mse"], f32["psnr"], f32["ssim"], f32["nonfinite"], 0.0, 0.0, 0.0], ref, (H, W, clamp))


def test_the_shape_list_covers_what_it_promises():
    from tests import loss_cases
    assert {(20, 1030), (769, 10), (100, 190)} <= set(mr.SHAPES)
    assert sorted((mr._last_rows_out(H) + 10) % 4 for H, _ in mr.REMAINDER) == [0, 1, 2, 3]
    assert all(H > loss_cases.SEG and W > loss_cases.SW for H, W in mr.REMAINDER)
    u8 = mr.make_bytes(7, 5, 4)
    assert u8.shape == (7, 5, 4) and np.array_equal(u8[..., :3], mr.make_bytes(7, 5))


def test_quantisation_references_at_the_thresholds():
    x = torch.tensor([0.6 / 255, 254.6 / 255, 1.0, 1.5, -0.0, -1.0, float("inf"), float("-inf")], dtype=torch.float32).reshape(1, 1, -1).repeat(3, 1, 1).numpy()
    r, t = mr.quant_round(x)[0, :, 0], mr.quant_trunc(x)[0, :, 0]
    assert r.tolist() == [1, 255, 255, 255, 0, 0, 255, 0] and t.tolist() == [0, 254, 255, 255, 0, 0, 255, 0]


def test_report_aggregation_is_render_pys_arithmetic(tmp_path):
    from ex4dgs_amd import evaluate
    rows = np.zeros((3, 8))
    rows[:, evaluate.L1] = [0.1, 0.25, 1.0 / 3.0]
    rows[:, evaluate.PSNR] = [30.123456789, 28.7, 41.000001]
    rows[:, evaluate.SSIM] = [0.9, 0.87654321, 0.5]
    rows[:, evaluate.MSE] = 7.0                                        # not reported
    names = ["cam00_0001.png", "cam00_0002.png", "cam01_0001.png"]
    mean, per_view = evaluate.aggregate(rows, names)
    assert list(mean) == ["SSIM", "PSNR", "L1"] == list(per_view)
    for key, col in (("SSIM", evaluate.SSIM), ("PSNR", evaluate.PSNR), ("L1", evaluate.L1)):
        collected = [torch.tensor(v, dtype=torch.float32) for v in rows[:, col]]           # what the reference's lists hold
        assert mean[key] == torch.tensor(collected).mean().item()                          # render.py:98-105
        assert per_view[key] == {name: v for v, name in zip(torch.tensor(collected).tolist(), names)}      # :111-118
        assert list(per_view[key]) == names
    evaluate.write_report(str(tmp_path), mean, per_view)
    assert json.load(open(tmp_path / "mean_metrics.json")) == mean and json.load(open(tmp_path / "all_metrics.json")) == per_view
    assert open(tmp_path / "mean_metrics.json").read() == json.dumps(mean, indent=True)
    with pytest.raises(RuntimeError, match="names"):
        evaluate.aggregate(rows, names[:2])
    inf = evaluate.aggregate(np.array([[0, 0, np.inf, 1, 0, 0, 0, 0.0]]), ["a"])[0]
    assert inf["PSNR"] == float("inf") and inf["SSIM"] == 1.0


def test_the_calls_refuse_before_any_hip_call():
    """The pattern of tests/test_cpu_frames.py: fake non-NULL pointers are never dereferenced, the call returns on its argument check."""
    lib = _abi.load()
    window = (ctypes.c_float * 11)(*[1.0 / 11] * 11)
    p = 4096
    good = [8, 8, p, p, ctypes.addressof(window), 0, None, p, p, None]
    good_u8 = [8, 8, p, p, 3, None, ctypes.addressof(window), 0, None, p, p, None]

    def refused(name, args, match):
        with pytest.raises(RuntimeError) as e:
            _abi.call(name, *args)
        assert str(e.value) == lib.ex4d_loss_last_error().decode() != "" and match in str(e.value)

    for hole in (2, 3, 4, 7, 8):                                       # img, gt, window, row, scratch (out_u8 may be NULL)
        refused("ex4d_frame_metrics", good[:hole] + [None] + good[hole + 1:], "bad argument")
    for hole in (2, 3, 6, 9, 10):
        refused("ex4d_frame_metrics_u8", good_u8[:hole] + [None] + good_u8[hole + 1:], "bad argument")
    for stride in (5, 0, 1, 2, -3):
        refused("ex4d_frame_metrics_u8", good_u8[:4] + [stride] + good_u8[5:], "pixel_stride")
    for flags in (4, 8, -1):
        refused("ex4d_frame_metrics", good[:5] + [flags] + good[6:], "flags")
        refused("ex4d_frame_metrics_u8", good_u8[:7] + [flags] + good_u8[8:], "flags")
    refused("ex4d_frame_metrics", [0] + good[1:], "bad argument")
    refused("ex4d_frame_metrics_u8", [8, -1] + good_u8[2:], "bad argument")
    assert lib.ex4d_frame_metrics(*good[:7], None, *good[8:]) == 1     # EX4D_ERR_ARG


def test_the_python_layer_refuses_the_cpu():
    from ex4dgs_amd import evaluate
    x = torch.zeros(3, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluate.frame_metrics(x, x)
    with pytest.raises(RuntimeError, match="ROCm"):
        evaluate.Evaluator(2, 4, 4, device="cpu")
