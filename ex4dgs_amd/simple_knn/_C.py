"""`simple_knn._C` of the reference, bound to the C ABI of include/ex4d_knn.h (libex4d_hip.so) with ctypes.

distCUDA2(points[P,3] float32 on a ROCm device) -> [P] float32: mean squared distance to the 3 nearest other points
(submodules/simple-knn/spatial.cu:15-27, simple_knn.cu:129-221).  No CPU fallback.
"""
import torch

from .. import _abi

EXPORTS = _abi.exports("ex4d_knn.h")


def distCUDA2(points):
    lib = _abi.load()
    if not points.is_cuda:
        raise RuntimeError(f"points are on {points.device}: distCUDA2 only runs on a ROCm GPU (no CPU fallback)")
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError("points must be [P,3]")
    pts = points.contiguous().float()
    P = pts.shape[0]
    means = torch.full((P,), 0.0, dtype=torch.float32, device=pts.device)          # spatial.cu:21
    if P == 0:
        return means
    scratch = torch.empty(lib.ex4d_dist2_scratch_bytes(P), dtype=torch.uint8, device=pts.device)
    with _abi.stream(pts.device) as stream:
        _abi.call("ex4d_dist2", P, pts.data_ptr(), means.data_ptr(), scratch.data_ptr(), stream)
    return means
