"""uint8 ground truth without a GPU: the three entry points are exported and bound, frames.gt_lut is bit for bit what the reference's
loader makes of a decoded frame (tests/golden/frames.npz, captured by tests/golden/make_golden_frames.py from the reference's own
PILtoTorch and im_reader), and the _u8 loss calls refuse bad arguments before any HIP call."""
import ctypes
import os

import numpy as np
import pytest
import torch

from ex4dgs_amd import _abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frames.npz")
NEW_LOSS = ("ex4d_l1_ssim_forward_u8", "ex4d_l1_ssim_backward_u8")
NEW_TRAINER = ("ex4d_trainer_step_u8",)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_the_built_library_exports_the_u8_entry_points():
    from ex4dgs_amd import build
    handle = ctypes.CDLL(build.build())
    for name in NEW_LOSS + NEW_TRAINER:
        assert hasattr(handle, name), name
    assert _abi.load().ex4d_abi_version() == 5


def test_the_table_declares_them_under_their_headers():
    from ex4dgs_amd import loss, native_trainer
    assert set(NEW_LOSS) <= set(_abi.exports("ex4d_loss.h")) == set(loss.EXPORTS)
    assert set(NEW_TRAINER) <= set(_abi.exports("ex4d_trainer.h")) == set(native_trainer.EXPORTS)
    status = {name for _, protos in _abi.PROTOTYPES.values() for name, _, _, is_status in protos if is_status}
    assert set(NEW_LOSS + NEW_TRAINER) <= status


@pytest.mark.parametrize("tag, stride", [("rgb", 3), ("rgba", 4)])
def test_gt_lut_is_the_references_image_bit_for_bit(golden, tag, stride):
    from ex4dgs_amd.frames import gt_lut
    u8 = torch.from_numpy(golden[tag + "_u8"])
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (53, 139, stride)
    assert all(len(torch.unique(u8[..., c])) == 256 for c in range(3))
    scales = golden["im_scales"].tolist()
    assert scales == [1.0, 0.5, 1.7]
    for k, im_scale in enumerate(scales):
        want = torch.from_numpy(golden[f"{tag}_f32_{k}"])
        got = gt_lut(im_scale)[u8.long()].permute(2, 0, 1)[:3]
        assert got.dtype == want.dtype == torch.float32 and torch.equal(got, want), (tag, im_scale)


def test_the_default_table_is_u_over_255():
    from ex4dgs_amd.frames import gt_lut
    lut = gt_lut()
    assert lut.dtype == torch.float32 and tuple(lut.shape) == (256,) and lut.device.type == "cpu" and lut.is_contiguous()
    assert np.array_equal(lut.numpy(), np.arange(256, dtype=np.float32) / np.float32(255.0))
    assert float(lut[0]) == 0.0 and float(lut[255]) == 1.0
    assert float(gt_lut(0.5).max()) == 1.0 and float(gt_lut(1.7)[255]) == float(torch.tensor(1.0) / 1.7)


def test_the_u8_loss_calls_refuse_before_any_hip_call():
    """The pattern of test_cpu_abi.py's ex4d_reg_forward refusal: fake non-NULL pointers are never dereferenced, because the call
    returns on its argument check."""
    lib = _abi.load()
    window = (ctypes.c_float * 11)(*[1.0 / 11] * 11)
    p = 4096                                                  # a non-NULL "device pointer" the refusal never touches
    good_fwd = [8, 8, p, p, 3, None, 0.2, ctypes.addressof(window), p, p, p, p, p, None]
    good_bwd = [8, 8, p, p, 3, None, 0.2, ctypes.addressof(window), p, p, p, None]

    def refused(name, args, match):
        with pytest.raises(RuntimeError) as e:
            _abi.call(name, *args)
        assert str(e.value) == lib.ex4d_loss_last_error().decode() != "" and match in str(e.value)

    for name, good in (("ex4d_l1_ssim_forward_u8", good_fwd), ("ex4d_l1_ssim_backward_u8", good_bwd)):
        for stride in (5, 0, 1, 2, -3):
            refused(name, good[:4] + [stride] + good[5:], "pixel_stride")
        for hole in (2, 3, 7):                                # img, gt, window
            refused(name, good[:hole] + [None] + good[hole + 1:], "bad argument")
        refused(name, [0] + good[1:], "bad argument")
    for hole in (8, 11, 12):                                  # loss, dmaps, scratch (the error maps may be NULL)
        refused("ex4d_l1_ssim_forward_u8", good_fwd[:hole] + [None] + good_fwd[hole + 1:], "bad argument")
    for hole in (8, 9, 10):                                   # dmaps, grad_loss, grad_img
        refused("ex4d_l1_ssim_backward_u8", good_bwd[:hole] + [None] + good_bwd[hole + 1:], "bad argument")
    assert lib.ex4d_l1_ssim_forward_u8(*good_fwd[:4], 5, *good_fwd[5:]) == 1      # EX4D_ERR_ARG


def test_frames_refuse_the_cpu():
    from ex4dgs_amd import frames
    with pytest.raises(RuntimeError, match="ROCm"):
        frames.FrameStore(2, 4, 4, device="cpu")
    with pytest.raises(RuntimeError, match="ROCm"):
        frames.FrameStream(4, 4, device="cpu")
