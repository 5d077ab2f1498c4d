"""Shared by tests/test_cpu_depth_loss.py and tests/test_gpu_depth_loss.py: the case table of the fused inverse-depth loss
(include/ex4d_loss.h, "DEPTH"; ex4dgs_amd/csrc/ex4d_depth.hip) and a float64 restatement, pure numpy, of its fit, its loss, its row and
its gradient.

The shapes restate the kernel's tiling: a lane owns PPL = 4 consecutive pixels of the flat index y W + x, a workgroup has 256 lanes
(WG = 1024 pixels), and the one wave that adds the workgroups' partial sums takes FOLD = 64 of them per step.

What the restatement takes over from the header as float32 BITS, because the header defines them as single float32 operations (numpy's
float32 arithmetic is IEEE, one rounding per operation, no contraction):
    g  = float32(v) * float32(code_scale)             the decode
    x  = float32(1) / depth                           the rendered inverse depth
    gh = float32(s) * g, rounded, + float32(o)        the alignment: a multiply, then an add
Everything else is float64: the five moments and the solve (s and o rounded to float32 once, as the header says), the residual
r = x - gh, rho, the sums, the gradient.  The kernel's float32 residual is one rounding of that r (2^-24 |r|; exact where x and gh are
within a factor of two), so neither its sign nor the Charbonnier slope near r = 0 is decided by cancellation; a rho carries at most
about four float32 roundings (2.4e-7), the gradient about eight (4.8e-7): inside TOL.

Conditions on the inputs, asserted at import (so on the CPU) for every case x align x acc on/off:
    every non-degenerate FIT has det >= 0.05 n Sgg;   mean |r| >= 0.1 mean |x| over the mask;   every |r| >= 1e-4 |x| except the
    designed zeros;   where at most four pixels count, every non-designed |r| >= 0.5 |x|.
"""
import functools

import numpy as np

from ex4dgs_amd import depth as xdepth

PPL, THREADS, FOLD = xdepth.PIXELS_PER_LANE, xdepth.THREADS, xdepth.FOLD
WG = PPL * THREADS
KINDS = ("l1", "charbonnier")
ALIGNS = ("given", "fit")
GT_TYPES = ("u16", "f32")
EPS = 1e-3
GRAD_LOSS = 1.7                        # the upstream gradient of the backward cases
TOL = 1e-6                             # the project's bar (flow_ref.TOL, evaluate): relative; for the gradient relative to max|ref|
CODE_SCALES = (1.0, 2.0 ** -16, 3e-5)  # 3e-5 is no power of two: the decode's product rounds
DET_FLOOR = 1e-10                      # the header's relative threshold of the degenerate fit
f32 = np.float32


def blocks(H, W):
    return (H * W + WG - 1) // WG


MANY = next(n for n in range(3, 4000, 2) if blocks(n, n) > FOLD)       # 257 with the flow loss's constants
# (name, H, W): the random frames
SHAPES = (
    ("one_pixel", 1, 1),
    ("row_wg_minus_1", 1, WG - 1),                 # the last lane of the workgroup holds PPL - 1 pixels
    ("row_wg", 1, WG),                             # exactly one workgroup
    ("row_wg_plus_1", 1, WG + 1),                  # a second workgroup of one pixel
    ("one_column", 37, 1),
    ("odd_rows", 7, 203),                          # W odd, H W = 1421 odd; two workgroups
    ("odd_small", 5, 23),                          # H W = 115: one partial wave, a 3-pixel last lane
    ("many_blocks", MANY, MANY),                   # more workgroups than one fold step of the finishing wave
)
assert blocks(MANY, MANY) > FOLD and blocks(1, WG) == 1 and blocks(1, WG + 1) == 2
ALL_INVALID, ONE_VALID, CONSTANT_GT, DESIGNED = "all_invalid", "one_valid", "constant_gt", "designed"
RANDOM = tuple(n for n, _, _ in SHAPES)
CASES = RANDOM + (ALL_INVALID, ONE_VALID, CONSTANT_GT, DESIGNED)
SPECIAL_SHAPES = {ALL_INVALID: (9, 31), ONE_VALID: (9, 31), CONSTANT_GT: (13, 89), DESIGNED: (3, 5)}
ONE_VALID_PIXEL = 100
LONE = (40000, 20.0, 0.7)              # code, depth, acc of the pixel of one_pixel and one_valid

# the designed frame, GIVEN with s = 1, o = 0 and code_scale 2^-8: (code, depth, acc); flat pixels 0 and 4 have r = 0 exactly
DESIGNED_SCALE = 2.0 ** -8
DESIGNED_PIXELS = ((256, 1.0, 1.0), (0, 2.0, 0.5), (65535, 4.0, 0.9), (512, 1.0, 0.0), (128, 2.0, 0.3),
                   (1000, 0.5, 0.25), (333, 8.0, 1.0), (77, 3.0, 0.6), (2000, 0.75, 0.1), (640, 0.5, 0.8),
                   (0, 0.5, 0.0), (150, 1.25, 0.45), (901, 6.0, 1.0), (65535, 50.0, 0.2), (1, 16.0, 0.7))
DESIGNED_R0 = (0, 4)
assert len(DESIGNED_PIXELS) == 15


def decode(raw, code_scale):
    """(g float32, valid bool) of raw values (uint16 codes or float32 values): the header's decode, float32 numpy."""
    v = raw.astype(f32)
    g = v * f32(code_scale)
    assert g.dtype == f32
    with np.errstate(invalid="ignore"):
        return g, np.isfinite(v) & (v > 0)


def inverse(depth):
    """x = 1.0f / depth, IEEE float32 division."""
    with np.errstate(divide="ignore", invalid="ignore"):
        x = f32(1.0) / depth
    assert x.dtype == f32
    return x


def mask_of(valid, acc):
    with np.errstate(invalid="ignore"):
        return valid if acc is None else valid & (acc > 0)


def fit64(g, x, m):
    """The header's closed form in float64 over the mask: dict(n, Sg, Sx, Sgg, Sgx, det, degenerate, s, o); s and o NOT yet rounded."""
    gm, xm = g[m].astype(np.float64), x[m].astype(np.float64)
    n = float(gm.size)
    Sg, Sx, Sgg, Sgx = float(gm.sum()), float(xm.sum()), float((gm * gm).sum()), float((gm * xm).sum())
    det = n * Sgg - Sg * Sg
    degenerate = not (n >= 2 and det > DET_FLOOR * n * Sgg)
    if degenerate:
        s, o = 0.0, Sx / max(n, 1.0)
    else:
        s = (n * Sgx - Sg * Sx) / det
        o = (Sx - s * Sg) / n
    return dict(n=n, Sg=Sg, Sx=Sx, Sgg=Sgg, Sgx=Sgx, det=det, degenerate=degenerate, s=s, o=o)


def aligned(g, s, o):
    """gh = s g + o as the header defines it: a float32 multiply, then a float32 add."""
    with np.errstate(invalid="ignore", over="ignore"):
        gh = f32(s) * g
        gh = gh + f32(o)
    assert gh.dtype == f32
    return gh


def restate(depth, raw, code_scale, align, given, kind, eps, acc, grad_loss):
    """float64: (loss, row [6], grad_depth [H,W], r [H,W], m [H,W]) of the header's definition; `given` = (scale, offset)."""
    g, valid = decode(raw, code_scale)
    m = mask_of(valid, acc)
    x32 = inverse(depth)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if align == "fit":
            f = fit64(g, x32, m)
            s, o = f32(f["s"]), f32(f["o"])
        else:
            s, o = f32(given[0]), f32(given[1])
        x = x32.astype(np.float64)
        r = x - aligned(g, s, o).astype(np.float64)
        w = np.ones_like(r) if acc is None else acc.astype(np.float64)
        if kind == "l1":
            rho, d = np.abs(r), np.sign(r)
        else:
            rho = np.sqrt(r * r + float(eps) ** 2)
            d = r / rho
        n = float(m.sum())
        denom = max(n, 1.0)
        loss = float((w * rho)[m].sum() / denom)
        rmse = float(np.sqrt((r * r)[m].sum() / n)) if n else 0.0
        bad = float((m & ~(np.isfinite(depth) & (depth > 0))).sum())
        grad = np.where(m, grad_loss * w / denom * d * -(x * x), 0.0)
    return loss, np.array([loss, n, float(s), float(o), rmse, bad]), grad, r, m


def _random_frame(rng, H, W, code_scale, constant=False):
    """Codes in 1..65535 with about 15 % zeros; x = 1 / depth correlated with the codes plus noise as large as a fifth of it, depth inside
    [0.5, 50]; acc in [0, 1] with exact zeros."""
    codes = rng.integers(1, 65536, (H, W)).astype(np.uint16)
    if constant:
        codes[:] = 12345
    u = codes.astype(np.float64) / 65535.0
    x = np.clip(0.3 + 1.2 * (rng.random((H, W)) if constant else u) + 0.8 * (rng.random((H, W)) - 0.5), 0.02, 2.0)
    depth = np.clip((1.0 / x).astype(f32), f32(0.5), f32(50.0))
    codes[rng.random((H, W)) < 0.15] = 0
    acc = rng.random((H, W)).astype(f32)
    acc[np.arange(H * W).reshape(H, W) % 29 == 5] = 0.0
    return depth, codes, acc


def _given_for(code_scale):
    """A plausible, deliberately imperfect alignment for the random frames: 0.9 of the planted slope, an offset 0.05 off."""
    return float(f32(0.9 * 1.2 / (65535.0 * code_scale))), float(f32(0.35))


@functools.lru_cache(maxsize=None)
def case(name):
    """{depth float32 [H,W], codes uint16 [H,W], acc float32 [H,W], code_scale, given (s, o)}; never modified by its users."""
    i = CASES.index(name)
    H, W = SPECIAL_SHAPES.get(name) or next((h, w) for n, h, w in SHAPES if n == name)
    rng = np.random.default_rng(300 + i)
    code_scale = CODE_SCALES[i % len(CODE_SCALES)]
    given = _given_for(code_scale)
    if name == DESIGNED:
        code_scale, given = DESIGNED_SCALE, (1.0, 0.0)
        t = np.array(DESIGNED_PIXELS, np.float64).reshape(H, W, 3)
        codes, depth, acc = t[..., 0].astype(np.uint16), t[..., 1].astype(f32), t[..., 2].astype(f32)
    else:
        depth, codes, acc = _random_frame(rng, H, W, code_scale, constant=name == CONSTANT_GT)
        if name == ALL_INVALID:
            codes[:] = 0
        if name in (ONE_VALID, "one_pixel"):
            p = ONE_VALID_PIXEL if name == ONE_VALID else 0
            codes[:] = 0
            codes.flat[p], depth.flat[p], acc.flat[p] = LONE
        # a residual that cancellation would decide is no test of the kernel: such a pixel loses its measurement (a handful per frame)
        for _ in range(8):
            hit = np.zeros((H, W), bool)
            for align in ALIGNS:
                for a in (None, acc):
                    _, _, _, r, m = restate(depth, codes, code_scale, align, given, "l1", EPS, a, GRAD_LOSS)
                    if m.sum() > 1:
                        hit |= m & (np.abs(r) < 2e-4 * inverse(depth))
            if not hit.any():
                break
            codes[hit] = 0
    out = dict(depth=np.ascontiguousarray(depth, f32), codes=codes, acc=acc, code_scale=code_scale, given=given, H=H, W=W)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def raw_of(c, gt):
    """The ground truth of a case as the kernels take it: uint16 codes, or the same values as float32."""
    return c["codes"] if gt == "u16" else c["codes"].astype(f32)


@functools.lru_cache(maxsize=None)
def reference(name, kind, align, use_acc, eps=EPS, grad_loss=GRAD_LOSS):
    """float64: (loss, row [6], grad_depth [H,W]) of the restatement on a case; both ground-truth types hold the same values."""
    c = case(name)
    loss, row, grad, _, _ = restate(c["depth"], c["codes"], c["code_scale"], align, c["given"], kind, eps, c["acc"] if use_acc else None, grad_loss)
    grad.setflags(write=False)
    row.setflags(write=False)
    return loss, row, grad


def designed_zeros(name, align, use_acc):
    """[H,W] bool: pixels in the mask whose residual is zero by construction -- the two of the designed frame under GIVEN, and the one
    pixel a FIT has when it has one (o = x)."""
    c = case(name)
    z = np.zeros((c["H"], c["W"]), bool)
    m = mask_of(decode(c["codes"], c["code_scale"])[1], c["acc"] if use_acc else None)
    if name == DESIGNED and align == "given":
        z.flat[list(DESIGNED_R0)] = True
    if align == "fit" and m.sum() == 1:
        z |= m
    return z & m


def exact_zero_mask(name, align, use_acc):
    """[H,W] bool: where the gradient must be an exact zero -- outside the mask, and at the designed zeros (either kind)."""
    c = case(name)
    m = mask_of(decode(c["codes"], c["code_scale"])[1], c["acc"] if use_acc else None)
    return ~m | designed_zeros(name, align, use_acc)


def conditions(name, align, use_acc):
    """What the module docstring promises of a case, as numbers: dict(n, degenerate, det_ratio, mean_ratio, min_ratio, zeros)."""
    c = case(name)
    acc = c["acc"] if use_acc else None
    _, _, _, r, m = restate(c["depth"], c["codes"], c["code_scale"], align, c["given"], "l1", EPS, acc, GRAD_LOSS)
    x = inverse(c["depth"]).astype(np.float64)
    f = fit64(decode(c["codes"], c["code_scale"])[0], inverse(c["depth"]), m)
    z = designed_zeros(name, align, use_acc)
    rest = m & ~z
    n = int(m.sum())
    return dict(n=n, degenerate=f["degenerate"], det_ratio=f["det"] / (f["n"] * f["Sgg"]) if n else 0.0,
                mean_ratio=float(np.abs(r[m]).mean() / np.abs(x[m]).mean()) if n else None,
                min_ratio=float((np.abs(r[rest]) / np.abs(x[rest])).min()) if rest.any() else None,
                zeros=int(z.sum()), zero_residuals=int((r[m] == 0).sum()))


def check_conditions():
    for name in CASES:
        for align in ALIGNS:
            for use_acc in (False, True):
                k = conditions(name, align, use_acc)
                what = (name, align, use_acc, k)
                assert k["zero_residuals"] == k["zeros"], what
                if align == "fit" and not k["degenerate"]:
                    assert k["det_ratio"] >= 0.05, what
                if align == "fit":
                    assert k["degenerate"] == (name in (ALL_INVALID, ONE_VALID, CONSTANT_GT, "one_pixel")), what
                if k["n"] > 1:
                    assert k["mean_ratio"] >= 0.1, what
                if k["min_ratio"] is not None:
                    assert k["min_ratio"] >= (0.5 if k["n"] <= 4 else 1e-4), what


check_conditions()


def torch_gt(c, gt, device="cpu", dtype="uint16", word_offset=0):
    """The ground truth as the torch tensor the module takes, a fresh copy: [H,W] uint16 / int16 codes (the same bits) or float32 values;
    word_offset > 0 places uint16 codes that many 2-byte words into a larger buffer (an odd offset: a base that is not 4-byte aligned)."""
    import torch
    if gt == "f32":
        return torch.from_numpy(raw_of(c, gt).copy()).to(device)
    words = c["codes"]
    buf = torch.zeros(word_offset + words.size + 3, dtype=torch.int16)
    buf[word_offset:word_offset + words.size] = torch.from_numpy(words.reshape(-1).view(np.int16).copy())
    buf = buf.to(device)
    out = buf[word_offset:word_offset + words.size].view(words.shape)
    return out.view(torch.uint16) if dtype == "uint16" else out
