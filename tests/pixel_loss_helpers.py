"""What the GPU tests of the per-pixel losses (test_gpu_flow.py, test_gpu_depth_loss.py) share: the device, outputs prefilled with 0xFF
bytes, bit views for comparing two calls, and the relative error against a reference that may be exactly 0."""
import torch

DEV = torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def poisoned(*shape, dtype=torch.float32):
    words = torch.full(shape, -1, dtype=torch.int32 if dtype == torch.float32 else torch.int64, device=DEV)          # 0xFF bytes
    return words.view(dtype)


def close(got, ref):
    """|got - ref| / |ref|; a reference of exactly 0 has to be met exactly."""
    if ref == 0.0:
        assert got == 0.0, got
        return 0.0
    return abs(got - ref) / abs(ref)
