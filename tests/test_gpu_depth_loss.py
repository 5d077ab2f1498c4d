"""The fused inverse-depth loss on the GPU (include/ex4d_loss.h "DEPTH", ex4dgs_amd/csrc/ex4d_depth.hip, ex4dgs_amd/depth.py) against the
float64 restatement of tests/depth_ref.py on its case table, and through the layers above it: autograd, a captured graph, render() and
FrameTrainer.step.

Achieved on MI355X (printed by every run and written to the parity report; the bar is 1e-6): forward 6.5e-8 relative at worst over the
table (loss, row[0], s, o, RMSE; counts exact), backward 1.9e-7 of max|ref|; a planted alignment (s 1.7, o -0.25) comes back as
1.70000005, -0.25 with a loss of 4e-8 mean|x|.
"""
import math

import numpy as np
import pytest
import torch

from tests import depth_ref as dr
from tests import helpers as h
from tests.pixel_loss_helpers import DEV, bits as _bits, close as _close, poisoned as _poisoned

pytestmark = pytest.mark.gpu
TABLE = [(n, k, al, a, gt) for n in dr.CASES for k in dr.KINDS for al in dr.ALIGNS for a in (False, True) for gt in dr.GT_TYPES]
IDS = [f"{n}-{k}-{al}-{'acc' if a else 'noacc'}-{gt}" for n, k, al, a, gt in TABLE]
WORST = {"forward": 0.0, "backward": 0.0}


def _xdepth():
    from ex4dgs_amd import depth as xdepth
    return xdepth


def _inputs(name, gt, use_acc, dtype="uint16", word_offset=0):
    c = dr.case(name)
    depth = torch.tensor(c["depth"]).to(DEV)
    acc = torch.tensor(c["acc"]).to(DEV) if use_acc else None
    return c, depth, dr.torch_gt(c, gt, DEV, dtype, word_offset), acc


def _poisoned_scratch(c):
    return torch.full((_xdepth().new_scratch(c["H"], c["W"], DEV).numel(),), 255, dtype=torch.uint8, device=DEV)


def _forward(c, depth, gt, acc, kind, align, loss=None, row=None, scratch=None):
    """(loss [1], row [6]) into outputs and scratch prefilled with 0xFF bytes."""
    return _xdepth().depth_loss_raw(depth, gt, c["code_scale"], align, c["given"][0], c["given"][1], kind, dr.EPS, acc,
                                    loss=_poisoned(1) if loss is None else loss, row=_poisoned(6, dtype=torch.float64) if row is None else row,
                                    scratch=_poisoned_scratch(c) if scratch is None else scratch)


def _backward(c, depth, gt, acc, kind, align, row, out=None, grad_loss=dr.GRAD_LOSS):
    g = torch.full((1,), grad_loss, device=DEV)
    return _xdepth().depth_loss_backward_raw(depth, gt, row, g, c["code_scale"], align, kind, dr.EPS, acc,
                                             out=_poisoned(c["H"], c["W"]) if out is None else out)


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- the kernels on the case table
@pytest.mark.parametrize("name,kind,align,use_acc,gt", TABLE, ids=IDS)
def test_forward_and_backward_match_the_float64_restatement(hip_lib, name, kind, align, use_acc, gt):
    c, depth, g, acc = _inputs(name, gt, use_acc)
    loss, row = _forward(c, depth, g, acc, kind, align)
    grad = _backward(c, depth, g, acc, kind, align, row).cpu().numpy()
    ref_loss, ref_row, ref = dr.reference(name, kind, align, use_acc)
    loss, row = float(loss.cpu()[0]), row.cpu().numpy()
    assert row[1] == ref_row[1] and row[5] == ref_row[5] == 0.0, (row, ref_row)
    if align == "given":
        assert row[2] == ref_row[2] and row[3] == ref_row[3]
    errs = (_close(loss, ref_loss),) + tuple(_close(row[i], ref_row[i]) for i in (0, 2, 3, 4))
    print(f"{name} {kind} {align} acc={use_acc} {gt}: loss {loss:.9g} (ref {ref_loss:.9g}) s {row[2]:.9g} o {row[3]:.9g}; relative errors "
          f"loss {errs[0]:.3g} row[0] {errs[1]:.3g} s {errs[2]:.3g} o {errs[3]:.3g} rmse {errs[4]:.3g}")
    assert loss == float(np.float32(row[0])), "loss is the row's first entry, rounded once"
    assert max(errs) <= dr.TOL, errs
    WORST["forward"] = max(WORST["forward"], max(errs))
    if name == dr.ALL_INVALID:
        assert loss == 0.0 and not row[[0, 1, 4, 5]].any() and (align == "given" or not row.any())
    assert not np.isnan(grad).any()
    assert not grad[dr.exact_zero_mask(name, align, use_acc)].any(), "exact zeros: outside the mask, r = 0"
    scale = float(np.abs(ref).max())
    if scale == 0.0:
        assert not grad.any()
        return
    err = float(np.abs(grad - ref).max()) / scale
    print(f"{name} {kind} {align} acc={use_acc} {gt}: |grad - ref| / max|ref| = {err:.3g}")
    assert err <= dr.TOL, err
    assert np.array_equal(grad != 0, ref != 0), "a gradient is zero exactly where the restatement's is"
    WORST["backward"] = max(WORST["backward"], err)


@pytest.mark.parametrize("align", dr.ALIGNS)
def test_all_invalid_is_a_zero_loss_a_zero_row_and_a_zero_gradient(hip_lib, align):
    for gt in dr.GT_TYPES:
        c, depth, g, acc = _inputs(dr.ALL_INVALID, gt, True)
        loss, row = _forward(c, depth, g, acc, "charbonnier", align)
        want = [0.0] * 6 if align == "fit" else [0.0, 0.0, c["given"][0], c["given"][1], 0.0, 0.0]
        assert float(loss) == 0.0 and row.cpu().tolist() == want
        assert not _backward(c, depth, g, acc, "charbonnier", align, row).any()


# ---------------------------------------------------------------------------------------------- NaN and inf
def test_nothing_behind_a_pixel_outside_the_mask_reaches_anything_and_a_bad_depth_inside_it_is_counted(hip_lib):
    c, depth, g, acc = _inputs("odd_small", "f32", True)
    codes, a = c["codes"], c["acc"]
    no_code = np.argwhere(codes == 0)
    no_acc = np.argwhere((codes > 0) & (a == 0))
    inside = np.argwhere((codes > 0) & (a > 0))
    assert len(no_code) >= 3 and len(no_acc) >= 2 and len(inside) >= 6
    (y0, x0), (y1, x1), (y4, x4) = no_code[:3]
    depth[y0, x0] = float("nan"); acc[y0, x0] = float("inf")                        # no measurement: a NaN depth, an infinite weight
    depth[y1, x1] = 0.0; g[y1, x1] = float("nan")                                   # a NaN measurement is none
    g[y4, x4] = float("inf"); depth[y4, x4] = -1.0                                  # nor is an infinite one
    (y2, x2), (y3, x3) = no_acc[:2]
    depth[y2, x2] = float("inf")                                                    # acc = 0: not composited
    depth[y3, x3] = float("nan"); acc[y3, x3] = float("nan")                        # a NaN weight is not > 0
    for kind in dr.KINDS:
        for align in dr.ALIGNS:
            loss, row = _forward(c, depth, g, acc, kind, align)
            ref_loss, ref_row, ref_grad, _, _ = dr.restate(depth.cpu().numpy(), g.cpu().numpy(), c["code_scale"], align, c["given"], kind, dr.EPS,
                                                           acc.cpu().numpy(), dr.GRAD_LOSS)
            row_h = row.cpu().numpy()
            assert math.isfinite(float(loss)) and np.isfinite(row_h).all() and row_h[1] == ref_row[1] == len(inside) and row_h[5] == 0.0
            assert max(_close(float(loss), ref_loss), *(_close(row_h[i], ref_row[i]) for i in (0, 2, 3, 4))) <= dr.TOL
            grad = _backward(c, depth, g, acc, kind, align, row)
            assert torch.isfinite(grad).all() and np.abs(grad.cpu().numpy() - ref_grad).max() <= dr.TOL * np.abs(ref_grad).max()
            for y, x in ((y0, x0), (y1, x1), (y2, x2), (y3, x3), (y4, x4)):
                assert float(grad[y, x]) == 0.0
    for k, bad in enumerate((float("nan"), 0.0, -2.0, float("inf"))):
        depth[inside[k][0], inside[k][1]] = bad
    for kind in dr.KINDS:
        for align in dr.ALIGNS:
            loss, row = _forward(c, depth, g, acc, kind, align)
            row_h = row.cpu().numpy()
            assert math.isnan(float(loss)) and math.isnan(row_h[0]) and row_h[1] == len(inside) and row_h[5] == 4.0, (kind, align, row_h)


# ---------------------------------------------------------------------------------------------- poisoned outputs
@pytest.mark.parametrize("name", ("one_pixel", "row_wg_plus_1", "odd_rows", dr.ALL_INVALID))
def test_poisoned_outputs_and_scratch_are_fully_overwritten(hip_lib, name):
    xdepth = _xdepth()
    for kind in dr.KINDS:
        for align in dr.ALIGNS:
            for gt in dr.GT_TYPES:
                c, depth, g, acc = _inputs(name, gt, True)
                loss_p, row_p = _forward(c, depth, g, acc, kind, align)
                loss_z, row_z = _forward(c, depth, g, acc, kind, align, loss=torch.zeros(1, device=DEV), row=torch.zeros(6, dtype=torch.float64, device=DEV),
                                         scratch=torch.zeros_like(xdepth.new_scratch(c["H"], c["W"], DEV)))
                assert _same((loss_p, row_p), (loss_z, row_z)) and torch.isfinite(loss_p).all() and torch.isfinite(row_p).all()
                grad_p = _backward(c, depth, g, acc, kind, align, row_p)
                grad_z = _backward(c, depth, g, acc, kind, align, row_p, out=torch.zeros(c["H"], c["W"], device=DEV))
                assert torch.equal(_bits(grad_p), _bits(grad_z)) and torch.isfinite(grad_p).all()


# ---------------------------------------------------------------------------------------------- misaligned inputs, guard words
@pytest.mark.parametrize("name", (dr.DESIGNED, "row_wg_plus_1", "odd_rows", "many_blocks"))
def test_misaligned_inputs_give_the_aligned_bits_and_leave_the_guards_alone(hip_lib, name):
    for kind, align, gt, use_acc in (("l1", "fit", "u16", True), ("charbonnier", "given", "u16", False), ("charbonnier", "fit", "f32", True)):
        c, depth, g, acc = _inputs(name, gt, use_acc)
        loss0, row0 = _forward(c, depth, g, acc, kind, align)
        grad0 = _backward(c, depth, g, acc, kind, align, row0)
        n = depth.numel()
        for word_offset, float_offset in ((1, 1), (3, 2), (2, 3), (1, 0)):
            _, _, g_m, _ = _inputs(name, gt, use_acc, word_offset=word_offset)
            if gt == "u16":
                assert g_m.data_ptr() % 8 == (2 * word_offset) % 8, "an odd word offset: a base that is not 4-byte aligned"
            fbuf = torch.full((n + 8,), 12345.0, device=DEV)
            fbuf[float_offset:float_offset + n] = depth.reshape(-1)
            depth_m = fbuf[float_offset:float_offset + n].view(depth.shape)
            keep = fbuf.clone()
            gbuf, lbuf, rbuf = _poisoned(n + 8), _poisoned(3), _poisoned(8, dtype=torch.float64)
            grad_m = gbuf[float_offset:float_offset + n].view(depth.shape)
            assert depth_m.data_ptr() % 16 == (4 * float_offset) % 16 and grad_m.is_contiguous()
            acc_m = None
            if use_acc:
                abuf = torch.full((n + 8,), float("nan"), device=DEV)
                abuf[float_offset:float_offset + n] = acc.reshape(-1)
                acc_m = abuf[float_offset:float_offset + n].view(acc.shape)
            loss1, row1 = _forward(c, depth_m, g_m, acc_m, kind, align, loss=lbuf[1:2], row=rbuf[1:7])
            _backward(c, depth_m, g_m, acc_m, kind, align, row1, out=grad_m)
            assert _same((loss1, row1, grad_m), (loss0, row0, grad0))
            guards = torch.cat([_bits(gbuf)[:float_offset], _bits(gbuf)[float_offset + n:], _bits(lbuf)[[0, 2]]])
            assert (guards == -1).all() and (_bits(rbuf)[[0, 7]] == -1).all(), "the words around grad_depth, loss and row stay untouched"
            assert torch.equal(_bits(fbuf), _bits(keep))


# ---------------------------------------------------------------------------------------------- determinism, ground-truth types
@pytest.mark.parametrize("name", ("odd_rows", "many_blocks", dr.CONSTANT_GT))
def test_two_calls_and_every_ground_truth_type_give_equal_bits(hip_lib, name):
    for kind in dr.KINDS:
        for align in dr.ALIGNS:
            results = []
            for gt, dtype in (("u16", "uint16"), ("f32", None), ("u16", "int16"), ("u16", "uint16")):
                c, depth, g, acc = _inputs(name, gt, True, dtype=dtype)
                assert g.dtype == (torch.float32 if gt == "f32" else getattr(torch, dtype))
                loss, row = _forward(c, depth, g, acc, kind, align)
                results.append((loss, row, _backward(c, depth, g, acc, kind, align, row)))
            assert all(_same(results[0], other) for other in results[1:])


# ---------------------------------------------------------------------------------------------- the fit
@pytest.mark.parametrize("name", ("odd_small", "many_blocks"))
def test_fit_recovers_a_planted_alignment(hip_lib, name):
    c = dr.case(name)
    s_true, o_true = 1.7, -0.25                                           # a negative offset keeps every planted value positive
    x = dr.inverse(c["depth"]).astype(np.float64)
    planted = ((x - o_true) / s_true).astype(np.float32)
    assert planted.min() > 0
    planted[c["codes"] == 0] = 0.0                                        # the frame's own holes
    depth, g = torch.tensor(c["depth"]).to(DEV), torch.tensor(planted).to(DEV)
    for kind in ("l1",):
        loss, row = _xdepth().depth_loss_raw(depth, g, 1.0, "fit", kind=kind)
        loss, row = float(loss), row.cpu().numpy()
        mean_x = float(x[c["codes"] > 0].mean())
        print(f"{name}: planted s {s_true} o {o_true}: fitted {row[2]:.9g} {row[3]:.9g}, loss {loss:.3g} = {loss / mean_x:.3g} mean|x|, rmse {row[4]:.3g}")
        assert row[1] == float((c["codes"] > 0).sum()) and row[5] == 0.0
        assert abs(row[2] - s_true) <= dr.TOL * abs(s_true) and abs(row[3] - o_true) <= dr.TOL * abs(o_true)
        assert loss < 1e-6 * mean_x


def test_the_gradient_is_the_detached_one_not_autograd_through_a_least_squares_fit(hip_lib):
    name, kind = "odd_small", "l1"
    c, depth, g, acc = _inputs(name, "u16", False)
    d = depth.clone().requires_grad_(True)
    (_xdepth().depth_loss(d, g, c["code_scale"], "fit", kind=kind) * dr.GRAD_LOSS).backward()
    got = d.grad.cpu().numpy()
    _, _, ref = dr.reference(name, kind, "fit", False)
    # the same loss with the fit inside the graph, float64
    gg, valid = dr.decode(c["codes"], c["code_scale"])
    m = torch.tensor(valid)
    dd = torch.tensor(c["depth"], dtype=torch.float64, requires_grad=True)
    x, gt64 = 1.0 / dd, torch.tensor(gg, dtype=torch.float64)
    sol = torch.linalg.lstsq(torch.stack([gt64[m], torch.ones_like(gt64[m])], 1), x[m][:, None]).solution
    r = x - (sol[0] * gt64 + sol[1])
    (torch.where(m, r.abs(), torch.zeros_like(r)).sum() / m.sum() * dr.GRAD_LOSS).backward()
    through = dd.grad.numpy()
    top = np.abs(ref).max()
    assert np.abs(got - ref).max() <= dr.TOL * top
    assert np.abs(through - ref).max() >= 1e-3 * top, "the two gradients are far enough apart for this test to tell them apart"


# ---------------------------------------------------------------------------------------------- autograd, graph capture
@pytest.mark.parametrize("align,kind,gt", (("fit", "l1", "u16"), ("given", "charbonnier", "f32")))
def test_autograd_is_the_raw_backward_bit_for_bit(hip_lib, align, kind, gt):
    xdepth = _xdepth()
    c, depth, g, acc = _inputs("odd_rows", gt, True)
    s, o = c["given"]
    for shape, factor in (((c["H"], c["W"]), 1.0), ((1, c["H"], c["W"]), -2.5)):
        d = depth.reshape(shape).clone().requires_grad_(True)
        a = acc.reshape(shape)
        loss = xdepth.depth_loss(d, g, c["code_scale"], align, s, o, kind, dr.EPS, a)
        assert loss.dim() == 0 and loss.requires_grad
        (loss * factor).backward()
        loss_raw, row = xdepth.depth_loss_raw(depth, g, c["code_scale"], align, s, o, kind, dr.EPS, acc)
        raw = xdepth.depth_loss_backward_raw(depth, g, row, torch.full((1,), factor, device=DEV), c["code_scale"], align, kind, dr.EPS, acc)
        assert d.grad.shape == d.shape and torch.equal(_bits(d.grad.reshape(raw.shape)), _bits(raw)) and torch.equal(_bits(loss.detach().reshape(1)), _bits(loss_raw))
    m = xdepth.depth_metrics(depth, g, c["code_scale"], align, s, o)
    _, want = xdepth.depth_loss_raw(depth, g, c["code_scale"], align, s, o, "l1", 0.0, None)
    table = torch.zeros(3, 6, dtype=torch.float64, device=DEV)
    xdepth.depth_metrics(depth, g, c["code_scale"], align, s, o, row=table[1])
    assert torch.equal(_bits(m), _bits(want)) and torch.equal(_bits(table[1]), _bits(want)) and not table[0].any() and not table[2].any()


def test_the_module_refuses_what_the_kernels_cannot_take(hip_lib):
    xdepth = _xdepth()
    c, depth, g, acc = _inputs("odd_small", "u16", True)
    row, one = torch.zeros(6, dtype=torch.float64, device=DEV), torch.ones(1, device=DEV)
    for call, text in ((lambda: xdepth.depth_loss_raw(depth.double(), g), "out_depth must be"), (lambda: xdepth.depth_loss_raw(depth[None, None], g), "out_depth must be"),
                       (lambda: xdepth.depth_loss_raw(depth.t(), g), "out_depth must be"), (lambda: xdepth.depth_loss_raw(depth, g[:-1]), "gt must be"),
                       (lambda: xdepth.depth_loss_raw(depth, g.cpu()), "gt must be"), (lambda: xdepth.depth_loss_raw(depth, g.view(torch.int16).to(torch.int32)), "gt must be"),
                       (lambda: xdepth.depth_loss_raw(depth, g, acc=acc[:-1]), "acc must be"), (lambda: xdepth.depth_loss_raw(depth, g, row=row[:4]), "row must be"),
                       (lambda: xdepth.depth_loss_raw(depth, g, scratch=torch.zeros(8, dtype=torch.uint8, device=DEV)), "scratch must be"),
                       (lambda: xdepth.depth_loss_backward_raw(depth, g, row.float(), one), "row must be"),
                       (lambda: xdepth.depth_loss_backward_raw(depth, g, row, one.cpu()), "grad_loss must be"),
                       (lambda: xdepth.depth_loss_backward_raw(depth, g, row, one, out=torch.zeros(3, device=DEV)), "out must be"),
                       (lambda: xdepth.depth_loss_raw(depth, g, kind="charbonnier", eps=0.0), "eps"),
                       (lambda: xdepth.depth_loss_raw(depth, g, code_scale=0.0), "code_scale"),
                       (lambda: xdepth.depth_loss_raw(depth, g, align="given", scale=float("nan")), "scale")):
        with pytest.raises(RuntimeError, match=text):
            call()


def test_a_captured_forward_and_backward_replay_on_inputs_changed_in_place(hip_lib):
    xdepth = _xdepth()
    c, depth, g, acc = _inputs("odd_rows", "u16", True, dtype="int16")
    kind, align = "charbonnier", "fit"
    loss, row = torch.zeros(1, device=DEV), torch.zeros(6, dtype=torch.float64, device=DEV)
    scratch, grad, gl = xdepth.new_scratch(c["H"], c["W"], DEV), torch.zeros_like(depth), torch.full((1,), dr.GRAD_LOSS, device=DEV)

    def both():
        xdepth.depth_loss_raw(depth, g, c["code_scale"], align, kind=kind, eps=dr.EPS, acc=acc, loss=loss, row=row, scratch=scratch)
        xdepth.depth_loss_backward_raw(depth, g, row, gl, c["code_scale"], align, kind, dr.EPS, acc, out=grad)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    first = (loss.clone(), row.clone(), grad.clone())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    depth.mul_(1.37)
    g.copy_(torch.roll(g, 5, dims=1))
    gl.fill_(-0.5)
    graph.replay()
    torch.cuda.synchronize()
    replayed = (loss.clone(), row.clone(), grad.clone())
    loss.zero_(); row.zero_(); grad.zero_()
    both()
    torch.cuda.synchronize()
    for a, b, old in zip(replayed, (loss, row, grad), first):
        assert torch.equal(_bits(a), _bits(b)) and not torch.equal(_bits(a), _bits(old))


# ---------------------------------------------------------------------------------------------- end to end: render(), FrameTrainer.step
T_RENDER = 137.5


def _scene():
    from ex4dgs_amd.scene import SceneConfig, make_scene
    cfg = SceneConfig("depth: 3000 static+dynamic, 96x64", 3000, 96, 64, 60.0, dyn_frac=0.3, z_lo=4.5, z_hi=30.0, sigma_px_med=3.0, seed=29)
    model, cam, bg = make_scene(cfg, device=DEV, fused=True)
    return model, cam.to(DEV), bg.to(DEV)


def _invdepth_codes(depth, seed):
    """uint16 [H,W] codes on the device: the frame's own inverse depth, scaled into the code range and disturbed by 30 %, with holes."""
    gen = torch.Generator().manual_seed(seed)
    d = depth.detach().reshape(depth.shape[-2:]).cpu()
    inv = 1.0 / d
    codes = (inv / inv.max() * 40000.0 * (1.0 + 0.3 * torch.randn(d.shape, generator=gen))).round().clamp(1, 65535)
    codes[torch.rand(d.shape, generator=gen) < 0.15] = 0
    return torch.from_numpy(codes.numpy().astype(np.uint16).view(np.int16)).to(DEV).view(torch.uint16)


def test_a_depth_loss_on_a_rendered_frame_reaches_the_gaussians(hip_lib):
    from ex4dgs_amd.render import render
    xdepth = _xdepth()
    model, cam, bg = _scene()
    for n in model.PARAM_NAMES:
        setattr(model, n, getattr(model, n).detach().clone().requires_grad_(True))
    with torch.no_grad():
        seen = render(cam, model, None, bg, timestamp=T_RENDER)
    gt = _invdepth_codes(seen["depth"], 3)
    out = render(cam, model, None, bg, timestamp=T_RENDER)
    assert out["depth"].shape == (1, cam.image_height, cam.image_width) and (out["acc"] > 0).any()
    loss = xdepth.depth_loss(out["depth"], gt, acc=out["acc"])
    loss.backward()
    loss = loss.detach()
    row = xdepth.depth_metrics(out["depth"], gt).cpu().numpy()
    print(f"rendered frame: loss {float(loss):.6g}, fit s {row[2]:.6g} o {row[3]:.6g}, n {row[1]:.0f}")
    assert math.isfinite(float(loss)) and float(loss) > 0 and row[1] > 0 and row[5] == 0 and np.isfinite(row).all()
    for n in ("_xyz", "_opacity"):
        grad = getattr(model, n).grad
        assert grad is not None and torch.isfinite(grad).all() and grad.abs().max() > 0, n


def test_frame_trainer_takes_the_depth_gradient_beside_a_colour_gradient(hip_lib):
    from ex4dgs_amd.trainer import FrameTrainer
    xdepth = _xdepth()
    scenes = [_scene() for _ in range(3)]
    cam, bg = scenes[0][1], scenes[0][2]
    H, W = cam.image_height, cam.image_width
    from ex4dgs_amd.render import render
    with torch.no_grad():
        gt = _invdepth_codes(render(cam, scenes[0][0], None, bg, timestamp=T_RENDER)["depth"], 3)
    g_color = 1e-3 * torch.randn(3, H, W, generator=torch.Generator().manual_seed(5)).to(DEV)
    weight = torch.full((1,), 100.0, device=DEV)

    def with_depth(out):
        d, acc = out["depth"].detach(), out["acc"].detach()
        _, row = xdepth.depth_loss_raw(d, gt, acc=acc)
        return [out["render"], out["depth"]], [g_color, xdepth.depth_loss_backward_raw(d, gt, row, weight, acc=acc)]

    ups = (with_depth, lambda out: ([out["render"], out["depth"]], [g_color, torch.zeros_like(out["depth"])]), lambda out: ([out["render"]], [g_color]))
    start = {n: getattr(scenes[0][0], n).detach().clone() for n in scenes[0][0].PARAM_NAMES}
    for (model, _, _), up in zip(scenes, ups):
        tr = FrameTrainer(model, optimizer=True, lrs={n: 1e-3 for n in model.PARAM_NAMES})
        out = tr.step(cam, bg, T_RENDER, up)
        tr.flush()
        torch.cuda.synchronize()
        assert out["depth"].shape == (1, H, W)
        assert all(torch.isfinite(getattr(model, n)).all() for n in model.PARAM_NAMES)
    a, b, plain = (m._xyz.detach() for m, _, _ in scenes)
    moved = float((plain - start["_xyz"]).abs().max())
    noise, signal = float((b - plain).abs().max()), float((a - b).abs().max())
    print(f"_xyz after one step: moved {moved:.3g}; zero depth gradient against no depth output {noise:.3g}; depth gradient against zero {signal:.3g}")
    # the compositing backward sums with float atomics ("noise floor"): two rasterizations of one frame differ in the last bits
    assert moved > 0 and noise <= 1e-4 * moved, "a zero depth gradient is no depth term"
    assert signal > 100 * max(noise, 1e-12), "the depth gradient moves the Gaussians"


def test_zz_report_the_achieved_errors(hip_lib):
    """Last in the file: the largest errors of the table test of this run, for the README row."""
    print(f"depth loss: worst relative error forward {WORST['forward']:.3g}, backward {WORST['backward']:.3g} (bar {dr.TOL:g})")
    h.REPORT.append(dict(kind="depth_loss", worst_forward=WORST["forward"], worst_backward=WORST["backward"], bar=dr.TOL))
    assert WORST["forward"] <= dr.TOL and WORST["backward"] <= dr.TOL
