"""The fused flow loss on the GPU (include/ex4d_loss.h "FLOW", ex4dgs_amd/csrc/ex4d_flow.hip, ex4dgs_amd/flow.py) against the float64
restatement of tests/flow_ref.py on its case table, and through the layers above it: autograd, a captured graph, render(flow_to=) and
FrameTrainer.step(flow_to=).

Achieved on MI355X (printed by every run and written to the parity report; the bar is 1e-6): forward 1.3e-7 relative at worst over the
table, backward 2.4e-7 of max|ref|.
"""
import math

import numpy as np
import pytest
import torch

from tests import flow_ref as fr
from tests import helpers as h
from tests.pixel_loss_helpers import DEV, bits as _bits, close as _close, poisoned as _poisoned

pytestmark = pytest.mark.gpu
TABLE = [(n, k, a, s) for n in fr.CASES for k in fr.KINDS for a in (False, True) for s in (3, 4)]
IDS = [f"{n}-{k}-{'acc' if a else 'noacc'}-s{s}" for n, k, a, s in TABLE]
WORST = {"forward": 0.0, "backward": 0.0}


def _inputs(name, S, use_acc, dtype="int16", word_offset=0):
    from ex4dgs_amd import flow as xflow
    c = fr.case(name)
    flow = torch.tensor(c["flow"]).to(DEV)
    enc = fr.encoded(c["codes"], S, dtype, DEV, word_offset)
    acc = torch.tensor(c["acc"]).to(DEV) if use_acc else None
    return xflow, c, flow, enc, acc


def _forward(xflow, c, flow, enc, acc, kind):
    """(loss [1], row [4]) into outputs and scratch prefilled with 0xFF bytes."""
    loss, row = _poisoned(1), _poisoned(4, dtype=torch.float64)
    scratch = _poisoned(xflow.new_scratch(c["H"], c["W"], DEV).numel())
    return xflow.flow_loss_raw(flow, enc, c["scale"], kind, fr.EPS, acc, loss=loss, row=row, scratch=scratch)


def _backward(xflow, c, flow, enc, acc, kind, row, out=None):
    g = torch.full((1,), fr.GRAD_LOSS, device=DEV)
    return xflow.flow_loss_backward_raw(flow, enc, row, g, c["scale"], kind, fr.EPS, acc, out=_poisoned(3, c["H"], c["W"]) if out is None else out)


# ---------------------------------------------------------------------------------------------- 1, 2: the kernels on the case table
@pytest.mark.parametrize("name,kind,use_acc,S", TABLE, ids=IDS)
def test_forward_matches_the_float64_restatement(hip_lib, name, kind, use_acc, S):
    xflow, c, flow, enc, acc = _inputs(name, S, use_acc)
    loss, row = _forward(xflow, c, flow, enc, acc, kind)
    ref_loss, ref_row, _ = fr.reference(name, kind, use_acc)
    loss, row = float(loss.cpu()[0]), row.cpu().numpy()
    assert row[1] == ref_row[1] and row[3] == ref_row[3] == 0.0, (row, ref_row)
    errs = (_close(loss, ref_loss), _close(row[0], ref_row[0]), _close(row[2], ref_row[2]))
    print(f"{name} {kind} acc={use_acc} S={S}: loss {loss:.9g} (ref {ref_loss:.9g}), relative errors loss {errs[0]:.3g} row[0] {errs[1]:.3g} row[2] {errs[2]:.3g}")
    assert loss == float(np.float32(row[0])), "loss is the row's first entry, rounded once"
    # the float loss carries one more rounding (2^-24) than the double row entry: inside the bar
    assert max(errs) <= fr.TOL, errs
    WORST["forward"] = max(WORST["forward"], max(errs))
    if name == fr.ALL_INVALID:
        assert loss == 0.0 and not row.any()


@pytest.mark.parametrize("name,kind,use_acc,S", TABLE, ids=IDS)
def test_backward_matches_the_float64_restatement(hip_lib, name, kind, use_acc, S):
    xflow, c, flow, enc, acc = _inputs(name, S, use_acc)
    _, row = _forward(xflow, c, flow, enc, acc, kind)
    grad = _backward(xflow, c, flow, enc, acc, kind, row).cpu().numpy()
    _, _, ref = fr.reference(name, kind, use_acc)
    assert not np.isnan(grad).any()
    zero = fr.exact_zero_mask(name)
    assert not grad[zero].any(), "exact zeros: plane 2, invalid pixels, r = 0"
    assert not grad[2].any()
    scale = float(np.abs(ref).max())
    if name == fr.ALL_INVALID:
        assert scale == 0.0 and not grad.any()
        return
    err = float(np.abs(grad - ref).max()) / scale
    print(f"{name} {kind} acc={use_acc} S={S}: |grad - ref| / max|ref| = {err:.3g}")
    assert err <= fr.TOL, err
    assert np.array_equal(grad != 0, ref != 0), "a gradient is zero exactly where the restatement's is"
    WORST["backward"] = max(WORST["backward"], err)


def test_a_nan_in_a_valid_pixel_reaches_the_loss_and_one_behind_an_invalid_pixel_reaches_nothing(hip_lib):
    xflow, c, flow, enc, acc = _inputs("odd_small", 3, True)
    valid = torch.tensor(c["codes"][..., 2] > 32768).to(DEV)
    inv = (~valid).nonzero()[0]
    flow[0, inv[0], inv[1]] = float("nan")
    acc[inv[0], inv[1]] = float("inf")
    for kind in fr.KINDS:
        loss, row = _forward(xflow, c, flow, enc, acc, kind)
        ref_loss, ref_row, ref_grad = fr.restate(flow.cpu().numpy(), c["codes"], c["scale"], kind, fr.EPS, acc.cpu().numpy(), fr.GRAD_LOSS)
        assert math.isfinite(float(loss)) and abs(float(loss) - ref_loss) <= fr.TOL * ref_loss and row.cpu().tolist()[1:] == [ref_row[1], pytest.approx(ref_row[2], rel=fr.TOL), 0.0]
        grad = _backward(xflow, c, flow, enc, acc, kind, row)
        assert torch.isfinite(grad).all() and not grad[:, inv[0], inv[1]].any()
    ok = valid.nonzero()[1]
    flow[1, ok[0], ok[1]] = float("inf")
    ok2 = valid.nonzero()[2]
    flow[0, ok2[0], ok2[1]] = float("nan")
    for kind in fr.KINDS:
        loss, row = _forward(xflow, c, flow, enc, acc, kind)
        row = row.cpu().numpy()
        assert math.isnan(float(loss)) and math.isnan(row[0]) and row[1] == float(valid.sum()) and row[3] == 2.0


# ---------------------------------------------------------------------------------------------- 3: poisoned outputs
@pytest.mark.parametrize("name", ("one_pixel", "row_wg_plus_1", "odd_rows", fr.ALL_INVALID))
def test_poisoned_outputs_are_fully_overwritten(hip_lib, name):
    for kind in fr.KINDS:
        for S in (3, 4):
            xflow, c, flow, enc, acc = _inputs(name, S, True)
            loss_p, row_p = _forward(xflow, c, flow, enc, acc, kind)
            loss_z, row_z = xflow.flow_loss_raw(flow, enc, c["scale"], kind, fr.EPS, acc, loss=torch.zeros(1, device=DEV),
                                                row=torch.zeros(4, dtype=torch.float64, device=DEV),
                                                scratch=torch.zeros(xflow.new_scratch(c["H"], c["W"], DEV).numel(), device=DEV))
            assert torch.equal(_bits(loss_p), _bits(loss_z)) and torch.equal(_bits(row_p), _bits(row_z))
            assert torch.isfinite(loss_p).all() and torch.isfinite(row_p).all()
            grad_p = _backward(xflow, c, flow, enc, acc, kind, row_p)
            grad_z = _backward(xflow, c, flow, enc, acc, kind, row_p, out=torch.zeros(3, c["H"], c["W"], device=DEV))
            assert torch.equal(_bits(grad_p), _bits(grad_z)) and torch.isfinite(grad_p).all()


# ---------------------------------------------------------------------------------------------- 4: misaligned inputs
@pytest.mark.parametrize("name", ("designed_scale_0.3", "row_wg_plus_1", "odd_rows", "many_blocks"))
def test_misaligned_inputs_give_the_aligned_bits_and_leave_the_guards_alone(hip_lib, name):
    for kind, S, use_acc in (("l1", 3, True), ("charbonnier", 4, False), ("charbonnier", 3, True)):
        xflow, c, flow, enc, acc = _inputs(name, S, use_acc)
        loss0, row0 = _forward(xflow, c, flow, enc, acc, kind)
        grad0 = _backward(xflow, c, flow, enc, acc, kind, row0)
        n = flow.numel()
        for word_offset, float_offset in ((1, 1), (3, 2), (2, 3), (1, 0)):
            _, _, _, enc_m, _ = _inputs(name, S, use_acc, word_offset=word_offset)
            assert enc_m.data_ptr() % 4 == (2 * word_offset) % 4
            fbuf = torch.full((n + 8,), 12345.0, device=DEV)
            fbuf[float_offset:float_offset + n] = flow.reshape(-1)
            flow_m = fbuf[float_offset:float_offset + n].view(flow.shape)
            keep = fbuf.clone()
            gbuf = _poisoned(n + 8)
            grad_m = gbuf[float_offset:float_offset + n].view(flow.shape)
            assert flow_m.data_ptr() % 16 == (4 * float_offset) % 16 and grad_m.is_contiguous()
            loss1, row1 = _forward(xflow, c, flow_m, enc_m, acc, kind)
            _backward(xflow, c, flow_m, enc_m, acc, kind, row1, out=grad_m)
            assert torch.equal(_bits(loss1), _bits(loss0)) and torch.equal(_bits(row1), _bits(row0))
            assert torch.equal(_bits(grad_m), _bits(grad0))
            guards = torch.cat([_bits(gbuf)[:float_offset], _bits(gbuf)[float_offset + n:]])
            assert (guards == -1).all(), "the words around grad_flow stay untouched"
            assert torch.equal(_bits(fbuf), _bits(keep))


# ---------------------------------------------------------------------------------------------- 5: determinism
@pytest.mark.parametrize("name", ("odd_rows", "many_blocks"))
def test_two_calls_and_both_code_dtypes_give_equal_bits(hip_lib, name):
    for kind in fr.KINDS:
        results = []
        for dtype in ("int16", "uint16", "int16"):
            xflow, c, flow, enc, acc = _inputs(name, 3, True, dtype=dtype)
            assert enc.dtype == getattr(torch, dtype)
            loss, row = _forward(xflow, c, flow, enc, acc, kind)
            results.append((loss, row, _backward(xflow, c, flow, enc, acc, kind, row)))
        for other in results[1:]:
            for a, b in zip(results[0], other):
                assert torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------- 6: graph capture
def test_a_captured_forward_and_backward_replay_on_inputs_changed_in_place(hip_lib):
    xflow, c, flow, enc, acc = _inputs("odd_rows", 3, True)
    kind = "charbonnier"
    loss, row = torch.zeros(1, device=DEV), torch.zeros(4, dtype=torch.float64, device=DEV)
    scratch, grad, g = xflow.new_scratch(c["H"], c["W"], DEV), torch.zeros_like(flow), torch.full((1,), fr.GRAD_LOSS, device=DEV)

    def both():
        xflow.flow_loss_raw(flow, enc, c["scale"], kind, fr.EPS, acc, loss=loss, row=row, scratch=scratch)
        xflow.flow_loss_backward_raw(flow, enc, row, g, c["scale"], kind, fr.EPS, acc, out=grad)

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
    flow.add_(0.37)
    enc.copy_(torch.roll(enc, 5, dims=1))
    g.fill_(-0.5)
    graph.replay()
    torch.cuda.synchronize()
    replayed = (loss.clone(), row.clone(), grad.clone())
    loss.zero_(); row.zero_(); grad.zero_()
    both()
    torch.cuda.synchronize()
    for a, b, old in zip(replayed, (loss, row, grad), first):
        assert torch.equal(_bits(a), _bits(b)) and not torch.equal(_bits(a), _bits(old))


# ---------------------------------------------------------------------------------------------- 7: end to end through render()
T_RENDER, T_FLOW = 137.5, 150.0


def _scene():
    from ex4dgs_amd.scene import SceneConfig, make_scene
    cfg = SceneConfig("flow: 3000 static+dynamic, 96x64", 3000, 96, 64, 60.0, dyn_frac=0.3, z_lo=4.5, z_hi=30.0, sigma_px_med=3.0, seed=29)
    model, cam, bg = make_scene(cfg, device=DEV, fused=True)
    return model, cam.to(DEV), bg.to(DEV)


def _encode(target, seed):
    """uint16 codes [H,W,3] (as int16 bits, on the device) of a float [2,H,W] flow: rounded to 1/256 pixel, about 70 % valid."""
    gen = torch.Generator().manual_seed(seed)
    H, W = target.shape[1:]
    words = torch.empty(H, W, 3, dtype=torch.int32)
    words[..., :2] = (target.cpu().permute(1, 2, 0) * 256).round().to(torch.int32).clamp(-32768, 32767) + 32768
    valid = torch.rand(H, W, generator=gen) < 0.7
    words[..., 2] = torch.where(valid, torch.randint(32769, 65536, (H, W), generator=gen), torch.randint(0, 32769, (H, W), generator=gen)).to(torch.int32)
    assert valid.sum() * 2 >= valid.numel()
    return fr.encoded(words.numpy().astype(np.uint16), 3, "int16", DEV)


def _torch_flow_loss(out_flow, enc, scale, kind, eps, acc):
    """The torch composition a user writes today: decode, mask, norm, masked mean."""
    from ex4dgs_amd.flow import decode_flow
    g, m = decode_flow(enc, scale)
    r = out_flow[:2] - g.permute(2, 0, 1)
    rho = r.abs().sum(0) if kind == "l1" else (r.pow(2).sum(0) + eps ** 2).sqrt()
    w = acc.detach().reshape(rho.shape) if acc is not None else torch.ones_like(rho)
    return torch.where(m > 0, w * rho, torch.zeros_like(rho)).sum() / m.sum().clamp(min=1)


@pytest.mark.parametrize("kind,use_acc", (("charbonnier", True), ("l1", False)))
def test_a_flow_loss_on_a_rendered_frame_trains_the_motion_like_the_torch_composition(hip_lib, kind, use_acc):
    from ex4dgs_amd.flow import flow_loss
    from ex4dgs_amd.render import render
    model, cam, bg = _scene()
    names = ("_xyz", "_xyz_disp", "_xyz_motion")
    for n in model.PARAM_NAMES:
        setattr(model, n, getattr(model, n).detach().clone().requires_grad_(True))
    with torch.no_grad():
        seen = render(cam, model, None, bg, timestamp=T_RENDER, flow_to=T_FLOW)["opticalflow"]
    enc = _encode(seen[:2] + 0.5 * torch.randn(2, *seen.shape[1:], generator=torch.Generator().manual_seed(4)).to(DEV), 8)
    scale = 0.75
    grads = []
    for fn in (flow_loss, _torch_flow_loss):
        model.zero_grad()
        out = render(cam, model, None, bg, timestamp=T_RENDER, flow_to=T_FLOW)
        loss = fn(out["opticalflow"], enc, scale, kind, 1e-3, out["acc"] if use_acc else None)
        loss.backward()
        grads.append((float(loss.detach()), {n: getattr(model, n).grad.clone() for n in names}))
    (loss_a, ga), (loss_b, gb) = grads
    assert loss_a > 0 and abs(loss_a - loss_b) <= 1e-5 * loss_b, (loss_a, loss_b)
    assert ga["_xyz_motion"].abs().max() > 0 and ga["_xyz"].abs().max() > 0 and ga["_xyz_disp"].abs().max() > 0
    for n in names:
        ref = gb[n]
        bar = 1e-5 * max(1.0, float(ref.abs().max()))
        err = float((ga[n] - ref).abs().max())
        print(f"{kind} acc={use_acc} {n}: |fused - composition| = {err:.3g}, bar {bar:.3g}, |ref|inf {float(ref.abs().max()):.3g}")
        h.REPORT.append(dict(kind="flow_loss_end_to_end", loss=kind, acc=use_acc, tensor=n, err=err, bar=bar))
        assert err <= bar, (n, err, bar)


# ---------------------------------------------------------------------------------------------- 8: FrameTrainer.step(flow_to=)
BETAS, RADAM_EPS = (0.9, 0.999), 1e-8
STEPS = ((137.5, 150.0), (41.0, 29.5))                     # (t, flow_to): forwards and backwards in time, different keyframe windows


def _record(tr, monkeypatch):
    """What the rasterizer's backward handed a FrameTrainer's frame: the gradients of the four boundary tensors (the attribute
    backward's input), of dir3D (the displacement backward's input) and of the four feature tensors.  The compositing backward adds
    its terms with float atomics in an order that changes from run to run ("noise floor"), so a second rasterization would
    not give these bits: the hand-composed step starts from the frame's own."""
    from ex4dgs_amd import attributes as attr, motion
    rec = {}
    attr_bwd, motion_bwd, submit = attr.backward_raw, motion.displacement_backward_raw, tr._submit

    def attr_wrapper(scal, params, grads_in, *a, **kw):
        rec["gin"] = tuple(None if g is None else g.clone() for g in grads_in)
        return attr_bwd(scal, params, grads_in, *a, **kw)

    def motion_wrapper(s0, s1, xyz, xyz_disp, xyz_motion, g_out, *a, **kw):
        rec["gdir"] = g_out.clone()
        return motion_bwd(s0, s1, xyz, xyz_disp, xyz_motion, g_out, *a, **kw)

    def submit_wrapper(grads, windows=None):
        rec["features"] = {tr.names[i]: grads[i].clone() for i in tr.feature_idx}
        return submit(grads, windows)

    monkeypatch.setattr(attr, "backward_raw", attr_wrapper)
    monkeypatch.setattr(motion, "displacement_backward_raw", motion_wrapper)
    monkeypatch.setattr(tr, "_submit", submit_wrapper)
    return rec, (attr_bwd, motion_bwd)


def _hand_step(model, rec, raw, cam, t, flow_to, near=0.2):
    """The dense gradients of one flow_to frame from the raw calls on the frame's rasterizer gradients: the attribute window, then
    motion window 0, then motion window 1 added into a zero dense gradient; the two static terms summed."""
    from ex4dgs_amd import attributes as attr, motion
    attr_bwd, motion_bwd = raw
    names = list(attr.PARAM_ORDER)
    params = [getattr(model, n) for n in names]
    Ns, Nd, K = model.num_static, model.num_dynamic, model._xyz_motion.shape[1]
    scal = lambda tt: attr.time_scalars(tt, Ns, Nd, K, model.duration, model.interval, model.time_shift, model.var_pad, model.interp_type)
    s0, s1 = scal(t), scal(flow_to)
    moving = [params[names.index(n)] for n in motion.PARAM_NAMES]
    fidx = [names.index(n) for n in attr.FEATURE_NAMES]
    gout, hint = attr_bwd(s0, params, rec["gin"], with_shs=False, sliced=True, interp_type=model.interp_type)
    g_xyz, g_disp, w0, w1, mh = motion_bwd(s0, s1, *moving, rec["gdir"], space="screen", camera=cam, near=near, interp_type=model.interp_type)
    assert w0.abs().max() > 0 and w1.abs().max() > 0 and g_xyz.abs().max() > 0
    dense = {}
    for i, n in enumerate(names):
        if i in fidx:
            dense[n] = rec["features"][n]
        elif n == "_xyz_motion":
            d = torch.zeros_like(params[i])
            d[:, hint[0]:hint[0] + hint[1]] += gout[i]
            d[:, mh[0]:mh[0] + mh[1]] += w0
            d[:, mh[2]:mh[2] + mh[3]] += w1
            dense[n] = d
        elif n == "_rotation_motion":
            d = torch.zeros_like(params[i])
            d[:, hint[2]:hint[2] + hint[3]] += gout[i]
            dense[n] = d
        elif n == "_xyz":
            dense[n] = gout[i] + g_xyz
        elif n == "_xyz_disp":
            dense[n] = gout[i] + g_disp
        else:
            dense[n] = gout[i]
    return dense


def _radam(model, dense, M, V, lrs, step):
    from ex4dgs_amd.optim import radam_step_raw
    from ex4dgs_amd.trainer import NAN_TO_NUM
    keep = {n: g.contiguous() for n, g in dense.items()}
    items = [(getattr(model, n).data_ptr(), g.data_ptr(), M[n].data_ptr(), V[n].data_ptr(), g.numel(), lrs[n], step, int(n in NAN_TO_NUM))
             for n, g in keep.items()]
    radam_step_raw(items, BETAS, RADAM_EPS, DEV)
    torch.cuda.synchronize()


def _upstream(enc, gt):
    from ex4dgs_amd.flow import flow_loss
    from ex4dgs_amd.loss import l1_ssim_loss
    return lambda out: ([flow_loss(out["opticalflow"], enc, 1.0, "charbonnier", 1e-3, out["acc"]), l1_ssim_loss(out["render"], gt, 0.2)[0]], [None, None])


def _targets(cam):
    gen = torch.Generator().manual_seed(11)
    H, W = cam.image_height, cam.image_width
    gt = torch.rand(3, H, W, generator=gen).to(DEV)
    enc = _encode(2.0 * torch.randn(2, H, W, generator=gen), 12)
    return enc, gt


@pytest.mark.parametrize("mode", ("sliced", "dense", "async"))
def test_frame_trainer_with_flow_to_takes_the_hand_composed_step_bit_for_bit(hip_lib, monkeypatch, mode):
    from ex4dgs_amd.trainer import FrameTrainer
    (ma, cam, bg), (mb, _, _) = _scene(), _scene()
    assert ma.num_static > 0 and ma.num_dynamic > 0
    enc, gt = _targets(cam)
    up = _upstream(enc, gt)
    lrs = {n: 1e-3 for n in ma.PARAM_NAMES}
    kw = {"sliced": {}, "dense": {"sliced": False}, "async": {"async_forward": True}}[mode]
    tr = FrameTrainer(ma, optimizer=True, lrs=lrs, **kw)
    assert tr.sliced == (mode != "dense")
    rec, raw = _record(tr, monkeypatch)
    p0 = {n: getattr(mb, n).clone() for n in mb.PARAM_NAMES}
    M = {n: torch.zeros_like(getattr(mb, n)) for n in mb.PARAM_NAMES}
    V = {n: torch.zeros_like(getattr(mb, n)) for n in mb.PARAM_NAMES}
    for step, (t, t_to) in enumerate(STEPS, 1):
        out = tr.step(cam, bg, t, up, flow_to=t_to)
        assert out["opticalflow"].abs().max() > 0 and out["viewspace_l1points"].abs().max() > 0
        tr.flush()
        torch.cuda.synchronize()
        dense = _hand_step(mb, rec, raw, cam, t, t_to)
        _radam(mb, dense, M, V, lrs, step)
        for i, n in enumerate(tr.names):
            assert torch.equal(_bits(getattr(ma, n)), _bits(getattr(mb, n))), (mode, step, n)
            assert torch.equal(_bits(tr.m[i]), _bits(M[n])) and torch.equal(_bits(tr.v[i]), _bits(V[n])), (mode, step, n)
    for n in ("_xyz", "_xyz_disp", "_xyz_motion"):
        assert not torch.equal(getattr(ma, n), p0[n]), n
    # a plain step on the same trainer still runs: a zero dir3D, a zero flow image, finite parameters that moved
    before = {n: getattr(ma, n).clone() for n in ma.PARAM_NAMES}
    from ex4dgs_amd.loss import l1_ssim_loss
    out = tr.step(cam, bg, 7.0, lambda o: ([l1_ssim_loss(o["render"], gt, 0.2)[0]], [None]))
    tr.flush()
    torch.cuda.synchronize()
    assert not out["opticalflow"].any() and not out["viewspace_l1points"].any() and tr._flow is None
    assert all(torch.isfinite(getattr(ma, n)).all() for n in ma.PARAM_NAMES) and not torch.equal(ma._xyz, before["_xyz"])


def test_frame_trainer_without_optimizer_hands_out_the_hand_composed_dense_gradient_and_refuses_what_is_not_built(hip_lib, monkeypatch):
    from ex4dgs_amd.trainer import FrameTrainer
    (ma, cam, bg), (mb, _, _) = _scene(), _scene()
    enc, gt = _targets(cam)
    up = _upstream(enc, gt)
    tr = FrameTrainer(ma, optimizer=False)
    assert not tr.sliced
    rec, raw = _record(tr, monkeypatch)
    t, t_to = STEPS[0]
    tr.step(cam, bg, t, up, flow_to=t_to)
    tr.flush()
    torch.cuda.synchronize()
    grads = tr.grads()
    dense = _hand_step(mb, rec, raw, cam, t, t_to)
    for n in tr.names:
        assert torch.equal(grads[n], dense[n]), n
    plain = FrameTrainer(mb, optimizer=False)
    plain.step(cam, bg, t, up)
    plain.flush()
    torch.cuda.synchronize()
    assert not torch.equal(plain.grads()["_xyz_motion"], grads["_xyz_motion"]), "the flow loss reaches the keyframes only through flow_to"
    for kw, text in ((dict(exchange="allreduce"), "allreduce"), (dict(exchange="sharded"), "sharded"), (dict(views_per_step=2), "views_per_step=2")):
        refused = FrameTrainer(mb, **kw)
        with pytest.raises(NotImplementedError, match=text):
            refused.step(cam, bg, t, up, flow_to=t_to)
    torch.cuda.synchronize()


def test_zz_report_the_achieved_errors(hip_lib):
    """Last in the file: the largest errors of the two table tests of this run, for the README row."""
    print(f"flow loss: worst relative error forward {WORST['forward']:.3g}, backward {WORST['backward']:.3g} (bar {fr.TOL:g})")
    h.REPORT.append(dict(kind="flow_loss", worst_forward=WORST["forward"], worst_backward=WORST["backward"], bar=fr.TOL))
    assert WORST["forward"] <= fr.TOL and WORST["backward"] <= fr.TOL
