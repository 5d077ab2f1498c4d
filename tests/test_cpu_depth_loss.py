"""The fused inverse-depth loss without a GPU (include/ex4d_loss.h "DEPTH", ex4dgs_amd/depth.py): the decode bit for bit; the closed-form
fit of tests/depth_ref.py against numpy's float64 least squares; its degenerate branches; the restatement's gradient against torch's
float64 autograd of the written formula with the fit detached; the refusals of the C entry points and of the module with their
messages; the census and the input conditions of the case table."""
import math
import os
import re

import numpy as np
import pytest
import torch

from ex4dgs_amd import _abi, build, depth as xdepth
from tests import depth_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the decode
@pytest.mark.parametrize("code_scale", dr.CODE_SCALES + (dr.DESIGNED_SCALE,))
def test_decode_invdepth_is_one_float32_product_for_both_ground_truth_types(code_scale):
    codes = np.concatenate([np.arange(0, 65536, 7, dtype=np.uint16), np.array([0, 1, 255, 256, 32767, 32768, 65534, 65535], np.uint16)])
    want = codes.astype(np.float32) * np.float32(code_scale)
    assert want.dtype == np.float32
    as_i16 = torch.from_numpy(codes.view(np.int16).copy())
    for gt in (as_i16, as_i16.view(torch.uint16), torch.from_numpy(codes.astype(np.float32))):
        g, valid = xdepth.decode_invdepth(gt, code_scale)
        assert g.dtype == torch.float32 and valid.dtype == torch.bool and g.shape == gt.shape
        assert np.array_equal(g.numpy().view(np.int32), want.view(np.int32))
        assert np.array_equal(valid.numpy(), codes > 0)
    mine, valid = dr.decode(codes, code_scale)
    assert np.array_equal(mine.view(np.int32), want.view(np.int32)) and np.array_equal(valid, codes > 0)


def test_a_float_ground_truth_is_a_measurement_only_where_it_is_finite_and_positive():
    v = torch.tensor([0.0, -0.0, -1.0, 1e-30, 3.5, float("inf"), -float("inf"), float("nan")])
    g, valid = xdepth.decode_invdepth(v, 2.0)
    assert valid.tolist() == [False, False, False, True, True, False, False, False] and g[4] == 7.0
    assert dr.decode(v.numpy(), 2.0)[1].tolist() == valid.tolist()
    with pytest.raises(RuntimeError, match="uint16 or torch.int16"):
        xdepth.decode_invdepth(torch.zeros(2, 2, dtype=torch.int32))


# ------------------------------------------------------------------ the fit
def _fit_inputs(name, use_acc):
    c = dr.case(name)
    g, valid = dr.decode(c["codes"], c["code_scale"])
    return c, g, dr.inverse(c["depth"]), dr.mask_of(valid, c["acc"] if use_acc else None)


@pytest.mark.parametrize("use_acc", (False, True))
@pytest.mark.parametrize("name", dr.CASES)
def test_the_closed_form_fit_is_numpys_least_squares(name, use_acc):
    c, g, x, m = _fit_inputs(name, use_acc)
    f = dr.fit64(g, x, m)
    assert f["n"] == float(m.sum())
    if f["degenerate"]:
        assert name in (dr.ALL_INVALID, dr.ONE_VALID, dr.CONSTANT_GT, "one_pixel")
        assert f["s"] == 0.0 and f["o"] == (float(x[m].astype(np.float64).sum()) / max(f["n"], 1.0))
        return
    gm, xm = g[m].astype(np.float64), x[m].astype(np.float64)
    top = gm.max()                                           # columns of like size: numpy's SVD is then as exact as the closed form
    (a, o), *_ = np.linalg.lstsq(np.stack([gm / top, np.ones_like(gm)], axis=1), xm, rcond=None)
    err = max(abs(f["s"] * top - a), abs(f["o"] - o)) / np.abs(xm).max()
    print(f"{name} acc={use_acc}: s {f['s']:.9g} o {f['o']:.9g}, |closed form - lstsq| / max|x| = {err:.3g}")
    assert err <= 1e-12, err


def test_the_degenerate_branches():
    g, x = np.array([3.0, 3.0, 3.0, 5.0], np.float32), np.array([1.0, 2.0, 6.0, 100.0], np.float32)
    none, one, same, line = (np.array(v, bool) for v in ([0, 0, 0, 0], [0, 0, 1, 0], [1, 1, 1, 0], [1, 1, 1, 1]))
    f = dr.fit64(g, x, none)
    assert f["degenerate"] and (f["n"], f["s"], f["o"]) == (0.0, 0.0, 0.0)
    f = dr.fit64(g, x, one)
    assert f["degenerate"] and (f["n"], f["s"], f["o"]) == (1.0, 0.0, 6.0)
    f = dr.fit64(g, x, same)                                 # a constant ground truth: the mean of x, whatever det's last bits are
    assert f["degenerate"] and (f["s"], f["o"]) == (0.0, 3.0) and abs(f["det"]) <= dr.DET_FLOOR * f["n"] * f["Sgg"]
    f = dr.fit64(g, x, line)
    assert not f["degenerate"] and f["det"] > 0.05 * f["n"] * f["Sgg"] * 0.5
    # codes so close that float64 sums leave a det of rounding noise: the relative threshold, not the sign of det, decides
    g = (np.float32(12345.0) * np.ones(1000, np.float32))
    g[::2] = np.nextafter(np.float32(12345.0), np.float32(2e4))
    f = dr.fit64(g, np.linspace(0.1, 1.0, 1000).astype(np.float32), np.ones(1000, bool))
    assert f["degenerate"] and f["s"] == 0.0 and abs(f["o"] - 0.55) < 1e-6
    for name, use_acc in ((dr.CONSTANT_GT, True), (dr.ONE_VALID, False), (dr.ALL_INVALID, True)):
        loss, row, grad = dr.reference(name, "l1", "fit", use_acc)
        c, g, x, m = _fit_inputs(name, use_acc)
        assert row[2] == 0.0 and row[3] == float(np.float32(x[m].astype(np.float64).sum() / max(float(m.sum()), 1.0)))
    assert dr.reference(dr.ONE_VALID, "l1", "fit", True)[0] == 0.0 and not dr.reference(dr.ONE_VALID, "charbonnier", "fit", True)[2].any()
    loss, row, grad = dr.reference(dr.ALL_INVALID, "charbonnier", "fit", False)
    assert loss == 0.0 and not row.any() and not grad.any()


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("use_acc", (False, True))
@pytest.mark.parametrize("align", dr.ALIGNS)
@pytest.mark.parametrize("kind", dr.KINDS)
@pytest.mark.parametrize("name", dr.CASES)
def test_the_restatement_is_torch_float64_autograd_with_the_fit_detached(name, kind, align, use_acc):
    c = dr.case(name)
    loss, row, grad = dr.reference(name, kind, align, use_acc)
    g, valid = dr.decode(c["codes"], c["code_scale"])
    m = torch.tensor(dr.mask_of(valid, c["acc"] if use_acc else None))
    s, o = row[2], row[3]
    assert s == float(np.float32(s)) and o == float(np.float32(o)), "s and o are float32 values"
    if align == "given":
        assert (s, o) == tuple(float(np.float32(v)) for v in c["given"])
    gh = torch.tensor(dr.aligned(g, s, o), dtype=torch.float64)
    depth = torch.tensor(c["depth"], dtype=torch.float64, requires_grad=True)
    x32 = torch.tensor(dr.inverse(c["depth"]), dtype=torch.float64)
    x = 1.0 / depth
    r = (x - x.detach() + x32) - gh                               # the value of the float32 division, the slope of 1 / depth
    rho = r.abs() if kind == "l1" else (r * r + dr.EPS ** 2).sqrt()
    w = torch.tensor(c["acc"], dtype=torch.float64) if use_acc else torch.ones_like(rho)
    ref = torch.where(m, w * rho, torch.zeros_like(rho)).sum() / max(float(m.sum()), 1.0)
    (ref * dr.GRAD_LOSS).backward()
    assert abs(loss - float(ref.detach())) <= 1e-13 * max(1.0, abs(float(ref.detach()))) and row[0] == loss
    assert row[1] == float(m.sum()) and row[5] == 0.0
    # autograd's slope is -1 / depth^2 with depth exact, the restatement's -x^2 with x the float32 quotient: 2^-23 apart at most
    want = depth.grad.numpy()
    assert np.abs(grad - want).max() <= 2.0 ** -22 * max(np.abs(want).max(), 1e-300)
    zero = dr.exact_zero_mask(name, align, use_acc)
    assert not grad[zero].any() and not want[zero].any() and np.array_equal(grad != 0, ~zero)
    if row[1] == 0:
        assert loss == 0.0 and not grad.any() and row[4] == 0.0
    elif not zero[m.numpy()].all():
        assert loss > 0 and row[4] > 0 and np.abs(grad).max() > 0


def test_the_case_table_census_and_its_input_conditions():
    dr.check_conditions()
    shapes = {(H, W) for _, H, W in dr.SHAPES}
    assert {(1, 1), (1, dr.WG - 1), (1, dr.WG), (1, dr.WG + 1), (37, 1), (7, 203), (5, 23)} <= shapes
    assert max(dr.blocks(H, W) for H, W in shapes) > dr.FOLD
    assert {dr.case(n)["code_scale"] for n in dr.RANDOM} == set(dr.CODE_SCALES) and not math.log2(3e-5).is_integer()
    for name in dr.RANDOM[1:] + (dr.CONSTANT_GT,):
        c = dr.case(name)
        assert c["depth"].min() >= 0.5 and c["depth"].max() <= 50.0 and c["codes"].dtype == np.uint16 and c["depth"].dtype == np.float32
        assert (c["codes"] == 0).mean() >= 0.10 or c["codes"].size < 64, name
        assert (c["acc"] == 0).any() or c["acc"].size < 30
        assert c["acc"].min() >= 0.0 and c["acc"].max() <= 1.0
    assert len(set(dr.case(dr.CONSTANT_GT)["codes"].ravel()) - {0}) == 1
    assert not dr.case(dr.ALL_INVALID)["codes"].any() and (dr.case(dr.ONE_VALID)["codes"] > 0).sum() == 1
    d = dr.case(dr.DESIGNED)
    assert (d["H"], d["W"]) == (3, 5) and d["given"] == (1.0, 0.0) and d["code_scale"] == 2.0 ** -8
    flat = d["codes"].ravel()
    assert (flat == 0).any() and (flat == 65535).any() and flat[0] == 256 and d["depth"].ravel()[0] == 1.0
    assert (d["acc"] == 0).any() and (d["acc"] == 1).any()
    assert (d["acc"].ravel()[flat > 0] == 0).any(), "a pixel with a measurement and acc = 0"
    _, _, _, r, m = dr.restate(d["depth"], d["codes"], d["code_scale"], "given", d["given"], "l1", dr.EPS, d["acc"], 1.0)
    assert [p for p in range(15) if m.ravel()[p] and r.ravel()[p] == 0.0] == list(dr.DESIGNED_R0)


# ------------------------------------------------------------------ the C entry points: constants, scratch, refusals
def _defines():
    text = open(os.path.join(ROOT, "include", "ex4d_loss.h")).read()
    return {n: int(v) for n, v in re.findall(r"^#define[ \t]+(EX4D_DEPTH_\w+)[ \t]+(\d+)[ \t]*$", text, flags=re.M)}


def test_the_modules_constants_are_the_headers_and_the_source_is_built_without_contraction():
    d = _defines()
    assert (d["EX4D_DEPTH_PIXELS_PER_LANE"], d["EX4D_DEPTH_THREADS"], d["EX4D_DEPTH_FOLD"]) == (xdepth.PIXELS_PER_LANE, xdepth.THREADS, xdepth.FOLD)
    assert xdepth.KINDS == {"l1": d["EX4D_DEPTH_L1"], "charbonnier": d["EX4D_DEPTH_CHARBONNIER"]}
    assert xdepth.ALIGNS == {"given": d["EX4D_DEPTH_ALIGN_GIVEN"], "fit": d["EX4D_DEPTH_ALIGN_FIT"]}
    assert (xdepth.GT_U16, xdepth.GT_F32) == (d["EX4D_DEPTH_GT_U16"], d["EX4D_DEPTH_GT_F32"])
    assert "-ffp-contract=off" in build.SOURCES["ex4d_depth.hip"]
    q = _abi.load().ex4d_depth_loss_scratch_bytes
    assert q(0, 5) == 0 and q(5, 0) == 0 and q(-1, -1) == 0
    for H, W in [(H, W) for _, H, W in dr.SHAPES] + [(1352, 1014)]:
        assert q(H, W) >= 8 + 9 * 8 * dr.blocks(H, W) and q(H, W) % 8 == 0


FAKE = 0x1000                    # never dereferenced: every call below is refused before any launch
FWD = dict(H=4, W=5, depth=FAKE, gt=FAKE, gt_type=0, code_scale=1.0, acc=None, align=1, scale=1.0, offset=0.0, kind=1, eps=1e-3,
           loss=FAKE, row=FAKE, scratch=FAKE)
BWD = dict(H=4, W=5, depth=FAKE, gt=FAKE, gt_type=0, code_scale=1.0, acc=None, align=1, kind=1, eps=1e-3, row=FAKE, grad_loss=FAKE,
           grad_depth=FAKE)
NAN, INF = float("nan"), float("inf")
REFUSALS = [
    (dict(H=0), "H and W must be positive"), (dict(W=0), "H and W must be positive"), (dict(H=-3), "H and W must be positive"),
    (dict(gt_type=2), "gt_type 2"), (dict(gt_type=-1), "gt_type -1"),
    (dict(align=2), "align 2"), (dict(align=-1), "align -1"),
    (dict(kind=2), "kind 2"), (dict(kind=-1), "kind -1"),
    (dict(eps=0.0), "eps"), (dict(eps=-1e-3), "eps"), (dict(eps=NAN), "eps"), (dict(eps=INF), "eps"),
    (dict(code_scale=0.0), "code_scale"), (dict(code_scale=-1.0), "code_scale"), (dict(code_scale=NAN), "code_scale"), (dict(code_scale=INF), "code_scale"),
    (dict(depth=None), "depth is NULL"), (dict(gt=None), "gt is NULL"),
]
FWD_ONLY = [(dict(loss=None), "loss is NULL"), (dict(row=None), "row is NULL"), (dict(scratch=None), "scratch is NULL"),
            (dict(scratch=FAKE + 4), "8-byte aligned"),
            (dict(align=0, scale=NAN), "scale"), (dict(align=0, scale=INF), "scale"), (dict(align=0, offset=NAN), "offset"), (dict(align=0, offset=-INF), "offset")]
BWD_ONLY = [(dict(row=None), "row is NULL"), (dict(grad_loss=None), "grad_loss is NULL"), (dict(grad_depth=None), "grad_depth is NULL")]


@pytest.mark.parametrize("entry,base,cases", [("ex4d_depth_loss_forward", FWD, REFUSALS + FWD_ONLY), ("ex4d_depth_loss_backward", BWD, REFUSALS + BWD_ONLY)])
def test_refusals_carry_their_message(entry, base, cases):
    lib = _abi.load()
    for change, text in cases:
        args = list(dict(base, **change).values()) + [None]
        with pytest.raises(RuntimeError) as e:
            _abi.call(entry, *args)
        assert str(e.value) == lib.ex4d_loss_last_error().decode() and text in str(e.value) and str(e.value).startswith("depth loss: "), (change, str(e.value))
        assert getattr(lib, entry)(*args) != 0


# ------------------------------------------------------------------ the module without a device
def test_the_module_without_a_device():
    c = dr.case("odd_small")
    depth, gt = torch.tensor(c["depth"]), dr.torch_gt(c, "u16")
    row, one = torch.zeros(6, dtype=torch.float64), torch.ones(1)
    for call in (lambda: xdepth.depth_loss(depth, gt), lambda: xdepth.depth_loss_raw(depth, gt), lambda: xdepth.depth_metrics(depth, gt),
                 lambda: xdepth.depth_loss(depth[None], dr.torch_gt(c, "f32"), align="given", scale=2.0, offset=0.1),
                 lambda: xdepth.depth_loss_backward_raw(depth, gt, row, one)):
        with pytest.raises(RuntimeError, match="only run on a ROCm GPU"):
            call()
    with pytest.raises(ValueError, match="unknown kind"):
        xdepth.depth_loss(depth, gt, kind="huber")
    with pytest.raises(ValueError, match="unknown align"):
        xdepth.depth_loss(depth, gt, align="median")
    with pytest.raises(ValueError, match="unknown align"):
        xdepth.depth_loss_backward_raw(depth, gt, row, one, align="median")
    with pytest.raises(RuntimeError, match="uint16 or torch.int16"):
        xdepth.gt_type(torch.zeros(2, 2, dtype=torch.float64))
    assert {"ex4d_depth_loss_scratch_bytes", "ex4d_depth_loss_forward", "ex4d_depth_loss_backward"} <= set(_abi.exports("ex4d_loss.h"))
    import __graft_entry__ as entry
    import inspect
    assert "ex4dgs_amd.depth" in inspect.getsource(entry.build)
