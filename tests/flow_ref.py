"""Shared by tests/test_cpu_flow.py, tests/test_gpu_flow.py and tools/make_golden_flow_decode.py: the case table of the fused flow
loss (include/ex4d_loss.h, "FLOW"; ex4dgs_amd/csrc/ex4d_flow.hip) and a float64 restatement of its loss, its row and its gradient on the
float32-decoded ground truth.

The shapes restate the kernel's tiling: a lane owns PPL = 4 consecutive pixels of the flat index y W + x, a workgroup has 256 lanes
(WG = 1024 pixels), and the one wave that adds the workgroups' partial sums takes FOLD = 64 of them per step.  A float plane goes as
16-byte vectors where its lane starts are 16-byte aligned: the v plane of a frame whose H W is no multiple of 4 is not.

The reference's lines (utils/general_utils.py:39-53) restated, float32 numpy as there:
    decode_flow:        flow = encoded[..., :2].astype(float32);  flow -= 2**15;  flow /= 2**8;  mask = (encoded[..., 2] > 2**15).astype(float32)
    read_opticalflow:   flow = flow * flow_scale                  (a Python float: numpy multiplies by float32(flow_scale))
"""
import functools

import numpy as np

from ex4dgs_amd import flow as xflow

PPL, THREADS, FOLD = xflow.PIXELS_PER_LANE, xflow.THREADS, xflow.FOLD
WG = PPL * THREADS
KINDS = ("l1", "charbonnier")
EPS = 1e-3
GRAD_LOSS = 1.7                        # the upstream gradient of the backward cases
# 1e-6 relative (the issue's bar, the one `evaluate` uses): a rho carries about six float32 roundings (3.6e-7), the sum of a workgroup
# is float, the sum over workgroups double
TOL = 1e-6
SCALES = (1.0, 0.5, 0.3)               # 0.3 is no power of two: the decode's product rounds


def blocks(H, W):
    return (H * W + WG - 1) // WG


# (name, H, W): the random frames
SHAPES = (
    ("one_pixel", 1, 1),
    ("row_wg_minus_1", 1, WG - 1),                 # the last lane of the workgroup holds PPL - 1 pixels
    ("row_wg", 1, WG),                             # exactly one workgroup
    ("row_wg_plus_1", 1, WG + 1),                  # a second workgroup of one pixel
    ("one_column", 37, 1),
    ("odd_rows", 7, 203),                          # W odd, H W = 1421 odd: rows and the v plane start misaligned; two workgroups
    ("odd_small", 5, 23),                          # H W = 115: one partial wave, a 3-pixel last lane
    ("many_blocks", 257, 257),                     # 65 workgroups: more than one fold step
)
assert blocks(257, 257) > FOLD and blocks(1, WG) == 1 and blocks(1, WG + 1) == 2
assert all(H <= 300 and W <= 300 or H == 1 for _, H, W in SHAPES)
assert any(W % 2 == 1 and W % PPL and H > 1 and (H * W) % PPL for _, H, W in SHAPES)
DESIGNED = tuple(f"designed_scale_{s}" for s in SCALES)
ALL_INVALID = "all_invalid"
RANDOM = tuple(n for n, _, _ in SHAPES)
CASES = RANDOM + DESIGNED + (ALL_INVALID,)

# the designed pixels: (u code, v code, validity word); every combination of the three designed codes, valid, then invalid ones
DESIGNED_CODES = tuple((u, v, 32769) for u in (0, 32768, 65535) for v in (0, 32768, 65535)) + \
    ((0, 65535, 32768), (32768, 32768, 32768), (65535, 0, 0), (12345, 54321, 65535), (40000, 30000, 32769), (33000, 33000, 32769))
DESIGNED_SHAPE = (3, 5)
assert len(DESIGNED_CODES) == DESIGNED_SHAPE[0] * DESIGNED_SHAPE[1]
DESIGNED_R0 = (4, 13)                  # flat pixels whose rendered flow equals the decoded ground truth: r = 0 exactly
DESIGNED_ACC0 = 14                     # flat pixel whose acc is 0 (valid, r != 0)


def decode(codes, scale):
    """The reference's decode, float32 numpy: (flow [H,W,2], mask [H,W] float32)."""
    flow = codes[..., :2].astype(np.float32)
    flow -= 2 ** 15
    flow /= 2 ** 8
    flow = flow * scale
    assert flow.dtype == np.float32
    return flow, (codes[..., 2] > 2 ** 15).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """{flow float32 [3,H,W], codes uint16 [H,W,3], acc float32 [H,W], scale}; never modified by its users."""
    if name in DESIGNED:
        scale = SCALES[DESIGNED.index(name)]
        H, W = DESIGNED_SHAPE
        rng = np.random.default_rng(5)
        codes = np.array(DESIGNED_CODES, np.uint16).reshape(H, W, 3)
        g, _ = decode(codes, scale)
        flow = np.concatenate([g.transpose(2, 0, 1) + rng.standard_normal((2, H, W)).astype(np.float32), rng.standard_normal((1, H, W)).astype(np.float32)])
        for p in DESIGNED_R0:
            flow[:2, p // W, p % W] = g[p // W, p % W]
        acc = (0.25 + 0.75 * rng.random((H, W))).astype(np.float32)
        acc[DESIGNED_ACC0 // W, DESIGNED_ACC0 % W] = 0.0
    else:
        H, W = (9, 31) if name == ALL_INVALID else next((h, w) for n, h, w in SHAPES if n == name)
        i = CASES.index(name)
        scale = SCALES[i % len(SCALES)]
        rng = np.random.default_rng(100 + i)
        codes = np.empty((H, W, 3), np.uint16)
        codes[..., :2] = rng.integers(32768 - 2560, 32768 + 2560, (H, W, 2))            # +- 10 pixels
        valid = rng.random((H, W)) < 0.7
        codes[..., 2] = np.where(valid, rng.integers(32769, 65536, (H, W)), rng.integers(0, 32769, (H, W)))
        if name == ALL_INVALID:
            codes[..., 2] = rng.integers(0, 32769, (H, W))
        g, _ = decode(codes, scale)
        flow = np.concatenate([g.transpose(2, 0, 1) + rng.standard_normal((2, H, W)).astype(np.float32), rng.standard_normal((1, H, W)).astype(np.float32)])
        every = np.arange(H * W).reshape(H, W) % 17 == 3                                  # r = 0 exactly, in both components
        flow[0][every], flow[1][every] = g[..., 0][every], g[..., 1][every]
        acc = rng.random((H, W)).astype(np.float32)
        acc[np.arange(H * W).reshape(H, W) % 29 == 5] = 0.0
    out = dict(flow=np.ascontiguousarray(flow, np.float32), codes=codes, acc=acc, scale=scale, H=H, W=W)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def with_stride(codes, S, fill=65535):
    """[H,W,S] codes: S = 4 appends a fourth word nobody may read into the result."""
    if S == 3:
        return codes
    return np.concatenate([codes, np.full(codes.shape[:2] + (1,), fill, np.uint16)], axis=2)


def encoded(codes, S=3, dtype="int16", device="cpu", word_offset=0):
    """The codes as the torch tensor the module takes: [H,W,S], int16 or uint16 (the same bits), a fresh copy; word_offset > 0 places it
    that many 2-byte words into a larger buffer (an odd offset: a base that is not 4-byte aligned)."""
    import torch
    words = with_stride(codes, S)
    buf = torch.zeros(word_offset + words.size + 3, dtype=torch.int16)
    buf[word_offset:word_offset + words.size] = torch.from_numpy(words.reshape(-1).view(np.int16).copy())
    buf = buf.to(device)
    out = buf[word_offset:word_offset + words.size].view(words.shape)
    return out.view(torch.uint16) if dtype == "uint16" else out


@functools.lru_cache(maxsize=None)
def reference(name, kind, use_acc, eps=EPS, grad_loss=GRAD_LOSS):
    """float64: (loss, row [4], grad_flow [3,H,W]) of the written formula on the float32-decoded ground truth."""
    c = case(name)
    return restate(c["flow"], c["codes"], c["scale"], kind, eps, c["acc"] if use_acc else None, grad_loss)


def restate(flow, codes, scale, kind, eps, acc, grad_loss):
    g, mask = decode(codes, scale)
    m = mask > 0
    f = flow.astype(np.float64)
    ru, rv = f[0] - g[..., 0].astype(np.float64), f[1] - g[..., 1].astype(np.float64)
    w = np.ones_like(ru) if acc is None else acc.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        if kind == "l1":
            rho, du, dv = np.abs(ru) + np.abs(rv), np.sign(ru), np.sign(rv)
        else:
            rho = np.sqrt(ru * ru + rv * rv + float(eps) ** 2)
            du, dv = ru / rho, rv / rho
        count = float(m.sum())
        denom = max(count, 1.0)
        loss = float(np.where(m, w * rho, 0.0).sum() / denom)
        epe = float(np.where(m, np.sqrt(ru * ru + rv * rv), 0.0).sum() / count) if count else 0.0
        bad = float((m & ~(np.isfinite(f[0]) & np.isfinite(f[1]))).sum())
        k = grad_loss * w / denom
        grad = np.stack([np.where(m, k * du, 0.0), np.where(m, k * dv, 0.0), np.zeros_like(ru)])
    return loss, np.array([loss, count, epe, bad]), grad


def exact_zero_mask(name):
    """[3,H,W] bool: where the gradient must be an exact zero -- plane 2, invalid pixels, r = 0 components (either kind)."""
    c = case(name)
    g, mask = decode(c["codes"], c["scale"])
    z = np.zeros((3, c["H"], c["W"]), bool)
    z[2] = True
    z[:2] |= (mask == 0)[None]
    both = (c["flow"][0] == g[..., 0]) & (c["flow"][1] == g[..., 1])
    z[:2] |= both[None]
    return z
