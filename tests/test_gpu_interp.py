"""The 'linear' and 'pchip' position interpolators on the GPU (ex4dgs_amd/csrc/ex4d_attributes.hip: the interpolator is a template
parameter of the per-Gaussian forward kernel and of the dense / sliced backward kernel) against the reference's own CGaussianModel
(tests/golden/model_getters_interp.npz; layout, families, census and bars in tests/interp_ref.py; tests/test_cpu_interp.py holds this
repository's CPU restatements to half of every bar used here):

  forward    the dynamic rows of means3D bit for bit the float32 reference (IEEE add, multiply, divide only); everything else FWD_BAR
  gradients  dense and sliced, GRAD_BAR * max(1, |reference|inf) per family; NaN (pchip rows with y[k+1] == y[k-1]) in the same places
  sliced == dense bit for bit once scattered; the hint is {k, 2, k, 2} for linear and {k-1, 4, k, 2} for pchip
  row counts across the 256-thread block edge inside the dynamic rows, Ns = 0, Nd = 1, K at its minimum, outputs prefilled with 0xFF
  a keyframe index one outside the interpolator's range and an unknown interpolator are refused and nothing is written
  autograd surface, a FrameTrainer step on sliced windows against the dense RAdam step, the 2-slice window in ex4d_radam_step_sliced,
  NativeTrainer (ex4d_trainer_set_interp) against FrameTrainer, growth and scoring on a linear model.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import interp_ref as ir

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = [(cfg, t) for cfg in ir.CONFIGS for t in ir.CONFIGS[cfg]["timestamps"]]


@pytest.fixture(scope="module")
def z():
    return ir.load()


def _features(Ns, Nd, seed=5):
    g = torch.Generator().manual_seed(seed)
    return {"_features_dc": torch.randn(Ns, 1, 3, generator=g), "_features_rest": torch.randn(Ns, 15, 3, generator=g),
            "_features_dc_motion": torch.randn(Nd, 1, 3, generator=g), "_features_rest_motion": torch.randn(Nd, 15, 3, generator=g)}


def _device_params(z, cfg, rows=None, static_rows=None, keyframes=None):
    """The 15 parameter tensors on the GPU in PARAM_ORDER (fixture rows, seeded features; keyframes: a slice of the keyframe axis) and
    the weights."""
    from ex4dgs_amd.attributes import PARAM_ORDER
    P, W = ir.params(z, cfg), ir.weights(z, cfg)
    Ns_all = P["_xyz"].shape[0]
    rows = np.arange(P["_xyz_motion"].shape[0]) if rows is None else np.asarray(rows, np.int64)
    static_rows = np.arange(Ns_all) if static_rows is None else np.asarray(static_rows, np.int64)
    sub = {n: torch.tensor(P[n][static_rows if n in ir.STATIC else rows]) for n in ir.NAMES}
    if keyframes is not None:
        for n in ("_xyz_motion", "_rotation_motion"):
            sub[n] = sub[n][:, keyframes].contiguous()
    sub.update(_features(static_rows.size, rows.size))
    all_rows = np.concatenate([static_rows, Ns_all + rows])
    wts = [torch.tensor(W[k][all_rows]).to(DEV) for k in ir.OUTPUTS]
    return [sub[n].to(DEV).contiguous() for n in PARAM_ORDER], wts, sub


def _scalars(cfg, t, Ns, Nd):
    from ex4dgs_amd.attributes import time_scalars
    c = ir.CONFIGS[cfg]
    s = time_scalars(t, Ns, Nd, c["K"], c["duration"], c["interval"], c["time_shift"], ir.VAR_PAD, c["interp"])
    assert s.k == ir.time_index(cfg, t)[0]
    return s


def _named(tensors):
    from ex4dgs_amd.attributes import PARAM_ORDER
    return {n: (None if g is None else g.cpu().numpy()) for n, g in zip(PARAM_ORDER, tensors)}


def _outs(outs):
    return {k: o.detach().cpu().numpy() for k, o in zip(ir.OUTPUTS, outs)}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _hint(cfg, k):
    first, count = ir.shapes(cfg)
    return (k + first, count, k, 2)


def _assert_ok(failures, what):
    assert not failures, f"{what}: {len(failures)} rows outside their bar: " + ir.format_failures(failures)


def _report(worst, what):
    top = sorted(worst.items(), key=lambda kv: -kv[1][2])[:3]
    print(what, "worst error / bar:", "; ".join(f"{f}/{n} {e:.3g}/{b:.3g}" for (f, n), (e, b, _) in top))


def _ff(shape):
    """A float32 tensor whose every byte is 0xFF."""
    return torch.full(shape, -1, dtype=torch.int32, device=DEV).view(torch.float32)


def _untouched(t):
    return bool((t.view(torch.int32) == -1).all())


# ------------------------------------------------------------------ 1. the fixture, every family and timestamp
@pytest.mark.parametrize("cfg,t", CASES)
def test_forward_dense_and_sliced_backward_match_the_reference(hip_lib, z, cfg, t):
    from ex4dgs_amd.attributes import backward_raw, forward_raw
    interp = ir.CONFIGS[cfg]["interp"]
    params, wts, sub = _device_params(z, cfg)
    Ns, Nd = sub["_xyz"].shape[0], sub["_xyz_motion"].shape[0]
    scal = _scalars(cfg, t, Ns, Nd)
    outs = forward_raw(scal, params, with_shs=False, interp_type=interp)
    got = _outs(outs)
    ref = z[f"{cfg}/{ir.tkey(t)}/xyz"]
    assert np.array_equal(_bits(got["xyz"][Ns:]), _bits(ref[Ns:])), "dynamic positions are not the reference's bits"
    dense = backward_raw(scal, params, wts + [None], with_shs=False, interp_type=interp)
    sliced, hint = backward_raw(scal, params, wts + [None], with_shs=False, sliced=True, interp_type=interp)
    assert hint == _hint(cfg, scal.k)
    assert tuple(sliced[7].shape) == (Nd, ir.shapes(cfg)[1], 3) and tuple(sliced[8].shape) == (Nd, 2, 4)
    dense_windows = ir.slice_grads(_named(dense), cfg, t)          # asserts exact zeros outside the window
    worst, failures = ir.check(z, cfg, t, got, dense_windows)
    _report(worst, ("dense", cfg, t))
    _assert_ok(failures, ("dense", cfg, t))
    _assert_ok(ir.check(z, cfg, t, got, _named(sliced))[1], ("sliced", cfg, t))
    sliced_named = _named(sliced)
    for n in ir.NAMES:
        assert np.array_equal(_bits(dense_windows[n]), _bits(sliced_named[n])), n
    if interp == "pchip":
        nan = np.isnan(sliced_named["_xyz_motion"]).any(axis=(1, 2))
        assert np.array_equal(nan, z[f"{cfg}/{ir.tkey(t)}/census/nan_gradient"]) and nan.sum() >= 8


@pytest.mark.parametrize("cfg,t", [("lin_b", 4.5), ("lin_a", 302), ("pchip_b", 4.5), ("pchip_b", 58)])
@pytest.mark.parametrize("with_shs", [True, False])
def test_autograd_surface_equals_the_raw_calls(hip_lib, z, cfg, t, with_shs):
    from ex4dgs_amd.attributes import PARAM_ORDER, backward_raw, evaluate_attributes, forward_raw
    c = ir.CONFIGS[cfg]
    params, wts, sub = _device_params(z, cfg)
    Ns, Nd = sub["_xyz"].shape[0], sub["_xyz_motion"].shape[0]
    named = {n: p.clone().requires_grad_(True) for n, p in zip(PARAM_ORDER, params)}
    outs = evaluate_attributes(named, t, duration=c["duration"], interval=c["interval"], time_shift=c["time_shift"], var_pad=ir.VAR_PAD,
                               with_shs=with_shs, interp_type=c["interp"])
    g_shs = torch.randn(outs[4].shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    (sum((o * w).sum() for o, w in zip(outs[:4], wts)) + (outs[4] * g_shs).sum()).backward()
    scal = _scalars(cfg, t, Ns, Nd)
    raw_out = forward_raw(scal, params, with_shs=with_shs, interp_type=c["interp"])
    raw = backward_raw(scal, params, wts + [g_shs if with_shs else None], with_shs=with_shs, interp_type=c["interp"])
    for a, b in zip(outs, raw_out):
        assert np.array_equal(_bits(a.detach().cpu().numpy()), _bits(b.cpu().numpy()))
    for n, r in zip(PARAM_ORDER, raw):
        if r is None:
            assert named[n].grad is None
        else:
            assert np.array_equal(_bits(named[n].grad.cpu().numpy()), _bits(r.cpu().numpy())), n
    _assert_ok(ir.check(z, cfg, t, _outs(outs), ir.slice_grads(_named([named[n].grad for n in PARAM_ORDER]), cfg, t))[1], ("autograd", cfg, t))


# ------------------------------------------------------------------ 2. block edges, minimal K, prefilled buffers
SIZES = [(1, 256), (200, 57), (255, 256), (1, 512), (256, 257), (0, 257), (0, 1), (300, 1), (0, 513)]      # Ns + Nd = 257, 511, 513, ...


@pytest.mark.parametrize("cfg,t", [("lin_b", 0), ("pchip_b", 4.5)])
@pytest.mark.parametrize("Ns,Nd", SIZES)
@pytest.mark.parametrize("min_k", [False, True])
def test_block_edges_minimal_keyframes_and_prefilled_buffers(hip_lib, z, cfg, t, Ns, Nd, min_k):
    """Rows taken from the fixture cyclically, so the expected values are the reference's.  min_k: the keyframe tensors cut down to the
    window the timestamp reads -- K = 2 (linear) or 4 (pchip), k = 0 or 1 -- which must give the same bits as the whole track.  Every
    output and gradient buffer starts as 0xFF bytes and sits between guards."""
    from ex4dgs_amd import attributes as A
    c = ir.CONFIGS[cfg]
    interp, code = c["interp"], ir.INTERP_CODE[c["interp"]]
    first, count = ir.shapes(cfg)
    rows = np.arange(Nd) % z[f"{cfg}/family"].shape[0]
    static_rows = np.arange(Ns) % z[f"{cfg}/param/_xyz"].shape[0]
    k_full = ir.time_index(cfg, t)[0]
    window = slice(k_full + first, k_full + first + count) if min_k else None
    params, wts, sub = _device_params(z, cfg, rows, static_rows, keyframes=window)
    scal = _scalars(cfg, t, Ns, Nd)
    if min_k:
        scal.K, scal.k = count, -first
        assert params[7].shape[1] == count == (2 if interp == "linear" else 4)
    N = Ns + Nd
    lib = A._lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    guard = 64
    bufs = []
    for s in ((N, 3), (N, 4), (N, 1), (N, 3)):
        n = int(np.prod(s))
        base = _ff((guard + (n + 3) // 4 * 4 + guard,))
        bufs.append((base, base[guard:guard + n].view(s), n))
    rc = lib.ex4d_attributes_forward_ex(C.byref(scal), code, *[A._ptr(p) for p in params], *[A._ptr(b[1]) for b in bufs], None, stream)
    assert rc == 0, lib.ex4d_attributes_last_error().decode()
    torch.cuda.synchronize()
    for base, view, n in bufs:
        assert _untouched(base[:guard]) and _untouched(base[guard + n:]) and not bool(torch.isnan(view).any())
    got = {k_: b[1].cpu().numpy() for k_, b in zip(ir.OUTPUTS, bufs)}
    ref = z[f"{cfg}/{ir.tkey(t)}/xyz"]
    assert np.array_equal(_bits(got["xyz"][Ns:]), _bits(ref[ref.shape[0] - z[f'{cfg}/family'].shape[0] + rows]))
    results = []
    for sliced in (False, True):
        gb = []
        for n_, p in zip(A.PARAM_ORDER, params):
            shape = (p.shape[0],) + A.sliced_shapes(interp)[n_] if sliced and n_ in A.SLICED_SHAPES else tuple(p.shape)
            n = int(np.prod(shape))
            base = _ff((guard + (n + 3) // 4 * 4 + guard,))
            gb.append((base, base[guard:guard + n].view(shape), n))
        out = A.backward_raw(scal, params, wts + [None], with_shs=False, out=[None if n_ in A.FEATURE_NAMES else b[1] for n_, b in zip(A.PARAM_ORDER, gb)],
                             sliced=sliced, interp_type=interp)
        if sliced:
            out, hint = out
            assert hint == ((scal.k + first), count, scal.k, 2)
        torch.cuda.synchronize()
        named = _named(out)
        for n_, (base, view, n) in zip(A.PARAM_ORDER, gb):
            assert _untouched(base[:guard]) and _untouched(base[guard + n:]), n_
            if n_ in A.FEATURE_NAMES:
                assert _untouched(view)
            else:
                assert not (_bits(named[n_]) == -1).any(), f"{n_}: entries never written"
        if not sliced:                                           # dense: exact zeros outside the window
            k = scal.k
            for n_, (f_, c_) in (("_xyz_motion", (first, count)), ("_rotation_motion", (0, 2))):
                g = named[n_]
                rest = np.delete(g, np.arange(k + f_, k + f_ + c_), axis=1)
                assert not rest.any() and not np.isnan(rest).any()
                named[n_] = g[:, k + f_:k + f_ + c_]
        results.append(named)
        _assert_ok(ir.check(z, cfg, t, got, named, rows=rows, static_rows=static_rows)[1], (cfg, t, Ns, Nd, min_k, sliced))
    for n_ in ir.NAMES:
        assert np.array_equal(_bits(results[0][n_]), _bits(results[1][n_])), n_


# ------------------------------------------------------------------ 3. refusals
@pytest.mark.parametrize("cfg", ["lin_b", "pchip_b"])
@pytest.mark.parametrize("edge", ["below", "above", "unknown"])
def test_keyframe_index_outside_the_range_and_unknown_interpolator_are_refused(hip_lib, z, cfg, edge):
    from ex4dgs_amd import attributes as A
    c = ir.CONFIGS[cfg]
    interp, code, K = c["interp"], ir.INTERP_CODE[c["interp"]], c["K"]
    lo, hi = (0, K - 2) if interp == "linear" else (1, K - 3)
    params, wts, sub = _device_params(z, cfg)
    Ns, Nd = sub["_xyz"].shape[0], sub["_xyz_motion"].shape[0]
    scal = _scalars(cfg, c["timestamps"][1], Ns, Nd)
    if edge == "unknown":
        code, match = 3, "unknown interpolator"
    else:
        scal.k, match = (lo - 1 if edge == "below" else hi + 1), "keyframe index"
    lib = A._lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    N = Ns + Nd
    outs = [_ff(s) for s in ((N, 3), (N, 4), (N, 1), (N, 3), (N, 16, 3))]
    rc = lib.ex4d_attributes_forward_ex(C.byref(scal), code, *[A._ptr(p) for p in params], *[A._ptr(o) for o in outs], stream)
    assert rc == 1 and match.encode() in lib.ex4d_attributes_last_error()
    for sliced in (False, True):
        bufs = [_ff((p.shape[0],) + A.sliced_shapes(interp)[n] if sliced and n in A.SLICED_SHAPES else tuple(p.shape)) for n, p in zip(A.PARAM_ORDER, params)]
        byname = dict(zip(A.PARAM_ORDER, params))
        tensors = [A._ptr(byname["_xyz_motion"])] + [A._ptr(byname[n]) for n in A._BWD_INPUTS] + [A._ptr(w) for w in wts] + [None] + [A._ptr(b) for b in bufs]
        if sliced:
            rc = lib.ex4d_attributes_backward_sliced_ex(C.byref(scal), code, *tensors, (C.c_int32 * 4)(), stream)
        else:
            rc = lib.ex4d_attributes_backward_ex(C.byref(scal), code, *tensors, stream)
        assert rc == 1 and match.encode() in lib.ex4d_attributes_last_error()
        torch.cuda.synchronize()
        assert all(_untouched(b) for b in bufs)
    torch.cuda.synchronize()
    assert all(_untouched(o) for o in outs)
    if edge != "unknown":
        with pytest.raises(RuntimeError, match="keyframe index"):
            A.forward_raw(scal, params, interp_type=interp)
        scal.k = lo if edge == "below" else hi                    # the neighbours inside the range are accepted
        A.forward_raw(scal, params, interp_type=interp)
        A.backward_raw(scal, params, wts + [None], with_shs=False, interp_type=interp)
    else:
        with pytest.raises(ValueError):
            A.forward_raw(scal, params, interp_type="nearest")
    # the pchip backward without the keyframe positions is refused too
    if interp == "pchip" and edge == "unknown":
        scal = _scalars(cfg, c["timestamps"][1], Ns, Nd)
        bufs = [_ff(tuple(p.shape)) for p in params]
        byname = dict(zip(A.PARAM_ORDER, params))
        tensors = [None] + [A._ptr(byname[n]) for n in A._BWD_INPUTS] + [A._ptr(w) for w in wts] + [None] + [A._ptr(b) for b in bufs]
        assert lib.ex4d_attributes_backward_ex(C.byref(scal), 2, *tensors, stream) == 1 and b"xyz_motion" in lib.ex4d_attributes_last_error()
        torch.cuda.synchronize()
        assert all(_untouched(b) for b in bufs)


# ------------------------------------------------------------------ 4. trainers and the optimizer
def _scene(interp, fused=True):
    from ex4dgs_amd.scene import SceneConfig, make_scene
    cfg = SceneConfig("interp: 2000 static+dynamic, 64x48", 2000, 64, 48, 60.0, dyn_frac=0.3, z_lo=4.5, z_hi=30.0, sigma_px_med=3.0, seed=17)
    model, cam, bg = make_scene(cfg, device=DEV, fused=fused, interp_type=interp)
    return model, cam.to(DEV), bg.to(DEV)


@pytest.mark.parametrize("interp", ["linear", "pchip"])
def test_frame_trainer_step_on_sliced_windows_equals_the_dense_gradient_step(hip_lib, interp):
    """One FrameTrainer step with sliced keyframe gradients against the dense-gradient RAdam step, bit for bit.  The rasterizer's
    backward sums with float atomics, so two renders of one frame do not give the same gradient bits; the dense step therefore takes
    the SAME frame's gradients: the windows the trainer holds after its frame are scattered into zeros and ex4d_radam_step runs on
    copies of the parameters and (zero) moments.  What is compared is everything after the rasterizer: the window bookkeeping of the
    trainer, its slice gather, and ex4d_radam_step_sliced on a 2- or 4-slice position window."""
    from ex4dgs_amd.optim import radam_step_raw
    from ex4dgs_amd.trainer import FrameTrainer, NAN_TO_NUM
    model, cam, bg = _scene(interp)
    assert model.interp_type == interp and model.time_shift == (2 if interp == "linear" else 12)
    w = torch.rand(3, cam.image_height, cam.image_width, generator=torch.Generator().manual_seed(5)).to(DEV)
    lrs = {n: 1e-3 for n in model.PARAM_NAMES}
    tr = FrameTrainer(model, optimizer=True, lrs=lrs)
    count = 2 if interp == "linear" else 4
    assert tr.sliced and tr.pgrad[tr.names.index("_xyz_motion")].shape[1:] == (count, 3)
    t = 137.5
    tr.step(cam, bg, t, lambda out: ([out["render"]], [w]))
    tr._drain()
    torch.cuda.synchronize()
    k = int((t + model.time_shift) // model.interval)
    assert tr._hint == ((k, 2, k, 2) if interp == "linear" else (k - 1, 4, k, 2))
    before = [p.detach().clone() for p in tr.params]
    dense = []
    for i, (n, p, g) in enumerate(zip(tr.names, tr.params, tr._grads)):
        if i in tr.kf_idx:
            first = tr._hint[0] if n == "_xyz_motion" else tr._hint[2]
            full = torch.zeros_like(p)
            full[:, first:first + g.shape[1]] = g
            assert float(g.abs().sum()) > 0
            dense.append(full)
        else:
            dense.append(g.detach().clone())
    m = [torch.zeros_like(p) for p in before]
    v = [torch.zeros_like(p) for p in before]
    radam_step_raw([(p.data_ptr(), g.data_ptr(), mm.data_ptr(), vv.data_ptr(), p.numel(), 1e-3, 1, int(n in NAN_TO_NUM))
                    for n, p, g, mm, vv in zip(tr.names, before, dense, m, v)], (0.9, 0.999), 1e-8, DEV)
    tr.flush()
    torch.cuda.synchronize()
    assert tr.steps == 1
    moved = 0.0
    for n, p, q, mm, vv, tm, tv in zip(tr.names, tr.params, before, m, v, tr.m, tr.v):
        assert torch.equal(p.detach().view(torch.int32), q.view(torch.int32)), n
        assert torch.equal(tm.view(torch.int32), mm.view(torch.int32)) and torch.equal(tv.view(torch.int32), vv.view(torch.int32)), n
        moved += float(tm.abs().sum())
    assert moved > 0 and all(torch.isfinite(p).all() for p in tr.params)


def test_sliced_radam_with_a_two_slice_window_equals_the_dense_step(hip_lib):
    from ex4dgs_amd.optim import radam_step_raw, radam_step_sliced_raw
    g = torch.Generator().manual_seed(12)
    for rows, K in ((1003, 34), (5, 2), (257, 15)):
        p0 = torch.randn(rows, K, 3, generator=g).to(DEV)
        A, B = p0.clone(), p0.clone()
        mA, vA, mB, vB = [torch.zeros_like(p0) for _ in range(4)]
        for step in range(1, 8):
            first = (0, K - 2, (step * 5) % (K - 1))[step % 3]
            blk = torch.randn(rows, 2, 3, generator=g).to(DEV)
            dense = torch.zeros_like(p0)
            dense[:, first:first + 2] = blk
            radam_step_raw([(A.data_ptr(), dense.data_ptr(), mA.data_ptr(), vA.data_ptr(), A.numel(), 1e-2, step)], (0.9, 0.999), 1e-8, DEV)
            radam_step_sliced_raw([(B.data_ptr(), mB.data_ptr(), vB.data_ptr(), rows, K, 3, 1e-2, step, [(first, 2, blk.data_ptr())])], (0.9, 0.999), 1e-8, DEV)
            torch.cuda.synchronize()
            assert torch.equal(A, B) and torch.equal(mA, mB) and torch.equal(vA, vB), (rows, K, step)


@pytest.mark.parametrize("interp", ["linear", "pchip"])
def test_native_trainer_with_set_interp_tracks_the_frame_trainer(hip_lib, interp):
    """ex4d_trainer_set_interp: the gradients of one frame and the parameters after two steps against trainer.FrameTrainer on a copy of
    the model, at the bars tests/test_gpu_round2.py::test_compiled_host_path_matches_the_python_trainer uses for cube (gradients 1e-5
    of the tensor's largest entry; parameters 1e-3 of the distance moved + two ulp of the largest parameter)."""
    from ex4dgs_amd.loss import l1_ssim_loss
    from ex4dgs_amd.native_trainer import NativeTrainer
    from ex4dgs_amd.trainer import FrameTrainer
    ma, cam, bg = _scene(interp)
    mb, _, _ = _scene(interp)
    gt = torch.rand(3, cam.image_height, cam.image_width, generator=torch.Generator().manual_seed(11)).to(DEV)
    count = 2 if interp == "linear" else 4
    lrs = {n: 1e-6 for n in ma.PARAM_NAMES}
    na = NativeTrainer(ma, cam, optimizer=False, lrs=lrs)
    assert na.interp_type == interp
    fb = FrameTrainer(mb, optimizer=False)
    up = lambda out: ([l1_ssim_loss(out["render"], gt, 0.2)[0]], [None])
    na.step(cam, bg, 137, gt)
    out = fb.step(cam, bg, 137, up)
    fb.flush(); torch.cuda.synchronize()
    assert float((na.output("render") - out["render"].detach()).abs().max()) <= 1e-6 and torch.equal(na.output("radii"), out["radii"])
    ref = fb.grads()
    k = int((137 + ma.time_shift) // ma.interval)
    for n in ("_xyz_motion", "_rotation_motion", "_xyz", "_opacity_motion"):
        g, hint = na.grad(n)
        assert hint == ((k, 2, k, 2) if interp == "linear" else (k - 1, 4, k, 2))
        r = ref[n]
        if n == "_xyz_motion":
            assert g.shape == (ma.num_dynamic, count, 3)
            r = r[:, hint[0]:hint[0] + count]
        elif n == "_rotation_motion":
            r = r[:, hint[2]:hint[2] + 2]
        assert float(r.abs().sum()) > 0 and float((r - g).abs().max()) <= 1e-5 * max(1.0, float(ref[n].abs().max())), n
    with pytest.raises(RuntimeError, match="interpolator is fixed"):
        na.set_interp("cube")                                   # a step has run
    assert na.interp_type == interp
    na.close()
    # two optimizer steps
    lrs = {n: 1e-4 for n in ma.PARAM_NAMES}
    p0 = {n: getattr(ma, n).clone() for n in ma.PARAM_NAMES}
    na = NativeTrainer(ma, cam, optimizer=True, lrs=lrs)
    fb = FrameTrainer(mb, optimizer=True, lrs=lrs)
    for t in (0, 137):
        na.step(cam, bg, t, gt); fb.step(cam, bg, t, up)
    fb.flush(); torch.cuda.synchronize()
    total = 0.0
    for n in ma.PARAM_NAMES:
        a, b = getattr(ma, n), getattr(mb, n)
        moved = float((a - p0[n]).abs().max())
        total += moved
        ulp = 2.0 ** -23 * float(a.abs().max())
        assert torch.isfinite(a).all() and float((a - b).abs().max()) <= 1e-3 * moved + 2 * ulp, (n, float((a - b).abs().max()), moved)
    assert total > 0
    # the interpolator survives a rebind: the model loses its last dynamic row, the new handle is told again
    na.begin_density_control()
    with torch.no_grad():
        for n in ma.PARAM_NAMES:
            if n in ir.DYNAMIC or n.endswith("_motion"):
                setattr(ma, n, getattr(ma, n)[:-1].clone().contiguous())
    na.rebind_parameters()
    assert na.interp_type == interp and na.steps() == 2
    na.step(cam, bg, 41, gt)
    g, hint = na.grad("_xyz_motion")
    k = int((41 + ma.time_shift) // ma.interval)
    assert g.shape == (ma.num_dynamic, count, 3) and hint == ((k, 2, k, 2) if interp == "linear" else (k - 1, 4, k, 2))
    with pytest.raises(RuntimeError, match="interpolator is fixed"):
        na.set_interp(interp)
    na.close()
    with pytest.raises(ValueError):
        NativeTrainer(mb, cam).set_interp("cubic_diff")


# ------------------------------------------------------------------ 5. growth and scoring on a linear model
def test_growth_and_scoring_on_a_linear_model(hip_lib):
    """extract_dynamic_points and expand_duration read the model's own time shift (2 under 'linear', not 12): against the restatement
    tests/growth_ref.py run with that shift; the grown tracks through the linear kernel against the float64 restatement at FWD_BAR at
    every keyframe time and between; evaluate.frame_metrics on the grown model's render."""
    from ex4dgs_amd import densify, evaluate, growth
    from ex4dgs_amd.render import render
    from ex4dgs_amd.scene import DynamicGaussians
    from tests import growth_ref as R
    from tests.test_gpu_growth import GENERATED, _assert_against_restatement, _model_from, _random_state
    st = _random_state(600, 0, 34, 21)
    st["params"]["_xyz_disp"][::7] *= 30.0                       # |disp| ~ 0.3: selected; every keyframe stays below 8 in magnitude
    model, stats, opt = _model_from(st, 300)
    model = DynamicGaussians({n: getattr(model, n) for n in model.PARAM_NAMES}, duration=300, interval=10, time_pad=2, interp_type="linear")
    assert model.time_shift == 2 and growth.first_keyframe_count(model, 300) == 34
    vis = torch.ones(600, dtype=torch.bool, device=DEV)
    cam_loc = torch.tensor([0.3, -0.2, 0.5])
    out = growth.extract_dynamic_points(model, stats, opt, cam_loc, 0.0, vis, 5.0, percentile=0.9)
    ref = {k: ({a: b.clone() for a, b in v.items()}) for k, v in st.items()}
    rm = {"interval": 10, "time_shift": 2, "time_pad": 2, "duration": 300}
    info = R.extract(ref, rm, cam_loc, vis, 5.0, percentile=0.9)
    assert out["dynamic"]["clone"] == int(info["mask"].sum()) > 20 and model._xyz_motion.shape[1:] == (34, 3)
    _assert_against_restatement(model, stats, opt, ref, GENERATED["extract"])
    for k in GENERATED["extract"]:                               # generated values agree to their bar: the expansion starts from the model's
        ref["params"][k] = getattr(model, k).detach().clone()
    assert R.expand_duration(ref, rm, 330) and growth.expand_duration(model, opt, 330)
    K2 = DynamicGaussians.keyframe_count(331, 10, 2, interp_type="linear")
    assert model.duration == 331 and model._xyz_motion.shape[1] == K2 == 37
    _assert_against_restatement(model, stats, opt, ref, GENERATED["expand"])
    # the grown tracks through the linear kernel
    from ex4dgs_amd.attributes import evaluate_attributes
    y64 = model._xyz_motion.detach().cpu().numpy().astype(np.float64)
    named = {n: getattr(model, n).detach() for n in model.PARAM_NAMES}
    times = [j * 10 - 2 for j in range(K2 - 1)] + [3.5, 171.25, 330.0]
    for t in times:
        tp = t + 2
        k, d = int(tp // 10), (tp % 10) / 10
        got = evaluate_attributes(named, t, duration=model.duration, interval=10, time_shift=2, var_pad=3, with_shs=False, interp_type="linear")[0]
        want = ir.position_forward(y64, k, (1 - d, 0.0, d, 0.0), "linear")
        # |y| < 8: two products rounded to at most half an ulp (2.4e-7) each and their sum likewise, under the absolute bar
        assert float(np.abs(want).max()) < 8 and float(np.abs(got[model.num_static:].cpu().numpy() - want).max()) <= ir.FWD_BAR, t
    # scoring a render of a linear model
    model2, cam, bg = _scene("linear")
    assert model2.num_dynamic == 600 and model2.fused
    with torch.no_grad():
        image = render(cam, model2, None, bg, timestamp=41.0, far=300.0)["render"]
    gt = torch.rand(3, cam.image_height, cam.image_width, generator=torch.Generator().manual_seed(2)).to(DEV)
    row = evaluate.frame_metrics(image.contiguous(), gt).cpu()
    assert torch.isfinite(row[:3]).all() and float(row[0]) > 0
