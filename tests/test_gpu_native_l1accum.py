"""The compiled trainer driving the reference's default schedule (include/ex4d_trainer.h: ex4d_trainer_step_ex): the l1_accum error
hook against the Python composition, the densification statistics against the library's own kernel fed the trainer's own tensors,
an overflowing asynchronous frame counted once, the skipped optimizer step, the round trip through density control and growth, the
NaN census kernel on raw tensors and the census wired into the trainer.

Scene: 1500 Gaussians (a quarter dynamic, K = 35) on a 200 x 152 image -- neither side a multiple of the 16-pixel tile or of the
loss's 64-column strip; 1125 static and 375 dynamic rows are several 256-thread blocks with a partial last one."""
import ctypes

import pytest
import torch

from ex4dgs_amd import _abi

pytestmark = pytest.mark.gpu

DEV = "cuda"
LR = 1e-4
W3 = (1e-4, 1e-4, 1e-3)


def _scene(seed=17):
    from ex4dgs_amd.scene import SceneConfig, make_scene
    cfg = SceneConfig("l1_accum: 1500 static + dynamic, 200x152", 1500, 200, 152, 110.0, dyn_frac=0.25, seed=seed)
    model, cam, bg = make_scene(cfg, device=DEV, fused=True)
    assert (model.num_static, model.num_dynamic, model._xyz_motion.shape[1]) == (1125, 375, 35)
    return model, cam.to(DEV), bg.to(DEV)


def _gt(cam, seed=11):
    return torch.rand(3, cam.image_height, cam.image_width, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _lrs(model, lr=LR):
    return {n: lr for n in model.PARAM_NAMES}


def _hook_upstream(gt, keep=None):
    """train.py:144-153: the fused loss with the hook tensor installed as the gradient of the flow image."""
    from ex4dgs_amd.loss import l1_ssim_loss

    def up(out):
        loss, _, _, hook = l1_ssim_loss(out["render"], gt, 0.2, acc=out["acc"])
        if keep is not None:
            keep.append((loss.detach(), hook))
        return [loss, out["opticalflow"]], [None, hook]
    return up


def _within_the_trainers_bar(a, b, p0, what):
    """The bar of test_compiled_host_path_matches_the_python_trainer: 1e-3 of the movement + 2 ulp of the parameter."""
    moved = float((a - p0).abs().max())
    ulp = 2.0 ** -23 * float(a.abs().max())
    err = float((a - b).abs().max())
    assert torch.isfinite(a).all() and err <= 1e-3 * moved + 2 * ulp, (what, err, moved)
    return moved


# ------------------------------------------------------------------------------------------------ 1. the hook
def test_error_hook_matches_the_python_composition(hip_lib):
    from ex4dgs_amd.native_trainer import NativeTrainer
    from ex4dgs_amd.trainer import FrameTrainer
    (ma, cam, bg), (mb, _, _) = _scene(), _scene()
    gt = _gt(cam)
    na = NativeTrainer(ma, cam, optimizer=False, lrs=_lrs(ma))
    fb = FrameTrainer(mb, optimizer=False)
    kept = []
    na.step(cam, bg, 137, gt, l1_accum=True)
    out = fb.step(cam, bg, 137, _hook_upstream(gt, kept))
    fb.flush(); torch.cuda.synchronize()
    loss, hook = kept[0]
    assert abs(float(na.output("loss")) - float(loss)) <= 1e-6
    assert float((na.output("render") - out["render"].detach()).abs().max()) <= 1e-6 and torch.equal(na.output("radii"), out["radii"])
    assert na.num_rendered > 0
    ref = fb.grads()
    dense = {"_xyz_motion": 4, "_rotation_motion": 2}
    for n in ma.PARAM_NAMES:
        g, hint = na.grad(n)
        r = ref[n]
        if n in dense:
            first = hint[0] if n == "_xyz_motion" else hint[2]
            assert float(r.abs().sum()) > 0 and float((r[:, first:first + dense[n]] - g).abs().max()) <= 1e-5 * max(1.0, float(r.abs().max())), n
        else:
            assert g.shape == r.shape and float((g - r).abs().max()) <= 1e-5 * max(1.0, float(r.abs().max())), n
    eref = out["viewspace_l1points"].grad
    egrad = na.output("error_grad")
    assert egrad.shape == eref.shape == (1500, 3)
    assert float((egrad - eref).abs().max()) <= 1e-5 * max(1.0, float(eref.abs().max()))
    vref = out["viewspace_points"].grad
    assert float((na.output("viewspace_grad") - vref).abs().max()) <= 1e-5 * max(1.0, float(vref.abs().max()))
    nhook = na.output("hook")
    assert float((nhook - hook).abs().max()) <= 1e-6
    assert torch.equal(nhook[0], na.output("acc")[0])                 # output 5 keeps meaning the accumulation image
    radii = na.output("radii")
    visible = radii > 0
    assert int(visible.sum()) > 100 and int((~visible).sum()) > 0
    assert float(egrad[~visible].abs().max()) == 0.0                  # exactly zero where nothing was rendered
    # e0 = sum of alpha T over the pixels a Gaussian contributes to: positive for every row that reached a pixel
    touched = egrad[visible][:, 0] > 0
    assert int(touched.sum()) > int(visible.sum()) // 2 and float(egrad[visible].abs().sum()) > 0
    # without the option the same call is the plain step: the flow image has no gradient
    na.step(cam, bg, 137, gt)
    assert abs(float(na.output("loss")) - float(loss)) <= 1e-6
    na.close()


# ------------------------------------------------------------------------------------------------ 2. statistics
@pytest.mark.parametrize("l1_accum, densify_stats", [(True, True), (True, False), (False, True)])
def test_statistics_are_the_librarys_own_on_the_trainers_tensors(hip_lib, l1_accum, densify_stats):
    from ex4dgs_amd import densify
    from ex4dgs_amd.native_trainer import NativeTrainer
    model, cam, bg = _scene()
    gt = _gt(cam)
    nt = NativeTrainer(model, cam, optimizer=True, lrs=_lrs(model))
    stats, twin = densify.DensityStats(model), densify.DensityStats(model)
    fresh = densify.DensityStats(model)
    for t in (0, 137, 41, 299):
        nt.step(cam, bg, t, gt, l1_accum=l1_accum, stats=stats, densify_stats=densify_stats)
        twin.update(nt.output("radii"), nt.output("viewspace_grad"), nt.output("error_grad") if l1_accum else None, t,
                    densify_stats=densify_stats, l1_accum=l1_accum)
        torch.cuda.synchronize()
        assert torch.equal(stats.static, twin.static) and torch.equal(stats.dynamic, twin.dynamic), t       # same kernel, same inputs
    changed = [bool((stats.static[r] != fresh.static[r]).any() or (stats.dynamic[r] != fresh.dynamic[r]).any()) for r in range(9)]
    if l1_accum and densify_stats:
        assert all(changed), changed
    elif l1_accum:                         # mark_prune_stats alone: min_radii2D
        assert changed == [r == 6 for r in range(9)], changed
    else:                                  # gradient statistics only: the error rows stay at their initial values
        assert changed == [r in (0, 1, 5) for r in range(9)], changed
    with pytest.raises(RuntimeError, match="l1_accum"):
        o = _abi.Ex4dTrainerStepOptions()
        o.stats_flags, o.stats_s, o.stats_d = densify.L1_STATS, stats.static.data_ptr(), stats.dynamic.data_ptr()
        with _abi.stream(nt.device) as stream:
            _abi.call("ex4d_trainer_step_ex", nt.handle, 0.0, cam.world_view_transform.data_ptr(), cam.full_proj_transform.data_ptr(),
                      cam.camera_center.data_ptr(), bg.data_ptr(), gt.data_ptr(), stream, None, ctypes.byref(o))
    nt.close()


# ------------------------------------------------------------------------------------------------ 3. a re-run frame counts once
def test_an_overflowing_asynchronous_frame_is_counted_once(hip_lib):
    from ex4dgs_amd import densify
    from ex4dgs_amd.native_trainer import NativeTrainer
    from ex4dgs_amd.scene import make_scene
    # the scene of test_compiled_host_path_asynchronous_mode_is_exact_and_replays_overflowing_frames: the 200 x 152 one never leaves
    # the capacity's fixed headroom of 4096 instances
    model, cam, bg = make_scene("cfg3", P=8000, device=DEV, fused=True)
    cam, bg = cam.to(DEV), bg.to(DEV)
    gt = _gt(cam)
    nt = NativeTrainer(model, cam, optimizer=True, lrs=_lrs(model))
    nt.set_async(True)
    stats = densify.DensityStats(model)
    with torch.no_grad():                                     # exp(-3): footprints 20x smaller -> the seed frame has few tile instances
        model._scaling -= 3.0; model._scaling_motion -= 3.0
    nt.step(cam, bg, 0, gt, l1_accum=True, stats=stats)       # (the synchronous seed frame)
    small = nt.num_rendered
    with torch.no_grad():
        model._scaling += 3.0; model._scaling_motion += 3.0
    for t in (5, 137, 250):
        before = torch.cat([stats.static[1], stats.dynamic[1]]).clone()
        replays = nt.replays()
        nt.step(cam, bg, t, gt, l1_accum=True, stats=stats)
        torch.cuda.synchronize()
        rose = torch.cat([stats.static[1], stats.dynamic[1]]) - before
        assert torch.equal(rose, (nt.output("radii") > 0).float()), (t, nt.replays() - replays)
    assert nt.num_rendered > 1.5 * small and nt.replays() >= 1, (small, nt.num_rendered, nt.replays())
    nt.close()


# ------------------------------------------------------------------------------------------------ 4. the skipped optimizer step
def test_a_step_without_the_optimizer_leaves_parameters_moments_and_step_count_alone(hip_lib):
    """The ordinary steps after the skipped one are compared with a trainer that never ran it at the trainers' existing bar (1e-3 of
    the movement + 2 ulp), not bit for bit: the gradients come out of the rasterizer's float atomics, whose order differs from run to
    run, so two equal trainers do not agree bit for bit either.  What the skipped step itself must not touch is compared exactly."""
    from ex4dgs_amd import densify
    from ex4dgs_amd.native_trainer import NativeTrainer
    (ma, cam, bg), (mb, _, _) = _scene(), _scene()
    gt = _gt(cam)
    p0 = {n: getattr(ma, n).clone() for n in ma.PARAM_NAMES}
    na = NativeTrainer(ma, cam, optimizer=True, lrs=_lrs(ma))
    nb = NativeTrainer(mb, cam, optimizer=True, lrs=_lrs(mb))
    stats = densify.DensityStats(ma)
    times = (0, 137, 41, 299, 7, 138)
    for t in times:
        na.step(cam, bg, t, gt, l1_accum=True, stats=stats)
        nb.step(cam, bg, t, gt)
    torch.cuda.synchronize()
    params = {n: getattr(ma, n).clone() for n in ma.PARAM_NAMES}
    moments = na.moments()
    denom = stats.static[1].clone()
    assert na.steps() == len(times)
    na.step(cam, bg, 40, gt, l1_accum=True, stats=stats, apply_optimizer=False)
    torch.cuda.synchronize()
    assert na.steps() == len(times)
    after = na.moments()
    for n in ma.PARAM_NAMES:
        assert torch.equal(getattr(ma, n), params[n]), n
        assert torch.equal(after[n][0], moments[n][0]) and torch.equal(after[n][1], moments[n][1]), n
    g, _ = na.grad("_xyz")
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0                           # gradients readable
    assert torch.equal(stats.static[1] - denom, (na.output("radii")[:ma.num_static] > 0).float()) and float((stats.static[1] - denom).sum()) > 0
    loss, nan_s, nan_d = na.report()
    assert loss == float(na.output("loss")) > 0 and (nan_s, nan_d) == (0, 0)
    for t in (139, 200):
        na.step(cam, bg, t, gt, l1_accum=True, stats=stats)
        nb.step(cam, bg, t, gt)
    torch.cuda.synchronize()
    assert na.steps() == nb.steps() == len(times) + 2
    for n in ma.PARAM_NAMES:
        assert _within_the_trainers_bar(getattr(ma, n), getattr(mb, n), p0[n], n) > 0, n
    na.close(); nb.close()


# ------------------------------------------------------------------------------------------------ 5. density control and growth
def _clone_model(model):
    from ex4dgs_amd.scene import DynamicGaussians
    twin = DynamicGaussians({n: getattr(model, n).detach().clone() for n in model.PARAM_NAMES}, duration=model.duration, fused=True)
    twin.active_sh_degree = model.active_sh_degree
    return twin


def test_density_control_and_growth_round_trip(hip_lib):
    from ex4dgs_amd import densify, growth
    from ex4dgs_amd.native_trainer import NativeTrainer
    from ex4dgs_amd.trainer import FrameTrainer
    model, cam, bg = _scene()
    gt = _gt(cam)
    nt = NativeTrainer(model, cam, optimizer=True, lrs=_lrs(model))
    lrs = dict(_lrs(model), _xyz=3e-4, _opacity_motion=5e-5)
    nt.set_lrs(lrs)
    nt.set_sh_degree(2)
    nt.set_regularizers(W3)
    stats = densify.DensityStats(model)
    for t in (0, 137, 41, 299, 7):
        nt.step(cam, bg, t, gt, l1_accum=True, stats=stats)
    nt.step(cam, bg, 138, gt, l1_accum=True, stats=stats, apply_optimizer=False)     # the iteration train.py densifies in
    rows0 = (model.num_static, model.num_dynamic)
    handed = {}
    rebind = nt.rebind_parameters
    nt.rebind_parameters = lambda moments=None: (handed.update(moments), rebind(moments))[1]
    res = densify.densify_and_prune(model, stats, nt, 1e-6, 1e-6, 0.01, 0.01, 5.0, generator=torch.Generator(device=DEV).manual_seed(0))
    del nt.rebind_parameters
    rows1 = (model.num_static, model.num_dynamic)
    assert rows1 != rows0 and rows1 == (res["static"]["rows"], res["dynamic"]["rows"]) == (nt.cfg.Ns, nt.cfg.Nd)
    assert res["static"]["clone"] + res["static"]["split"] > 0 and stats.static.shape == (9, rows1[0]) and stats.dynamic.shape == (9, rows1[1])
    assert all(p is getattr(model, n) for p, n in zip(nt.params, nt.names))
    assert nt.steps() == 5
    moments = nt.moments()
    for n in model.PARAM_NAMES:
        assert moments[n][0].shape == getattr(model, n).shape
        assert torch.equal(moments[n][0], handed[n][0]) and torch.equal(moments[n][1], handed[n][1]), n
    assert float(moments["_xyz"][1].abs().max()) > 0                                   # the surviving rows kept their state
    # the same state in a FrameTrainer, three more steps on both
    twin = _clone_model(model)
    ft = FrameTrainer(twin, optimizer=True, lrs=lrs, regularizers=W3)
    ft.rebind_parameters({n: (m.clone(), v.clone()) for n, (m, v) in moments.items()})
    ft.steps = nt.steps()
    p0 = {n: getattr(model, n).clone() for n in model.PARAM_NAMES}
    upg = _hook_upstream(gt)
    for t in (40, 139, 200):
        nt.step(cam, bg, t, gt, l1_accum=True, stats=stats)
        ft.step(cam, bg, t, upg)
    ft.flush(); torch.cuda.synchronize()
    assert nt.steps() == ft.steps == 8
    moved = {n: _within_the_trainers_bar(getattr(model, n), getattr(twin, n), p0[n], n) for n in model.PARAM_NAMES}
    # the learning rates set before the rebind are in force: the twin was built with them, and RAdam's step is ~lr whatever the
    # gradient's scale, so a lost 3e-4 on _xyz would be two thirds of its movement, not 1e-3 of it ...
    assert moved["_xyz"] > 0 and moved["_opacity_motion"] > 0
    # ... and the SH degree (degree 2: the seven degree-3 coefficients get no gradient) and the regularisers (their float[4] is filled)
    g_rest, _ = nt.grad("_features_rest")
    assert nt.cfg.sh_degree == 2 and float(g_rest[:, 8:].abs().max()) == 0.0 and float(g_rest[:, :8].abs().max()) > 0
    reg = nt.output("reg")
    assert float(reg[3]) != 0.0 and float((reg - ft.last["reg"]).abs().max()) <= 1e-4 * float(reg.abs().max())

    def one_finite_step(t):
        nt.step(cam, bg, t, gt, l1_accum=True, stats=stats, nan_census=True)
        loss, nan_s, nan_d = nt.report()
        assert 0 < loss < 10 and (nan_s, nan_d) == (0, 0)
        assert all(torch.isfinite(p).all() for p in nt.params) and all(p is getattr(model, n) for p, n in zip(nt.params, nt.names))
        assert (nt.cfg.Ns, nt.cfg.Nd, stats.static.shape[1], stats.dynamic.shape[1]) == (model.num_static, model.num_dynamic) * 2

    steps = nt.steps()
    total = model.num_static + model.num_dynamic
    out = densify.prune_invisible(model, stats, nt)
    assert out["static"]["rows"] + out["dynamic"]["rows"] == model.num_static + model.num_dynamic <= total
    one_finite_step(10)
    ns, nd = model.num_static, model.num_dynamic
    vis = (nt.output("radii")[:ns] > 0).contiguous()
    out = growth.extract_dynamic_points(model, stats, nt, cam.camera_center, 0.0, vis, 5.0, percentile=0.5)
    assert out["dynamic"]["clone"] > 0 and (model.num_static, model.num_dynamic) == (ns - out["dynamic"]["clone"], nd + out["dynamic"]["clone"])
    one_finite_step(20)
    assert growth.expand_duration(model, nt, 320) and model._xyz_motion.shape[1] == nt.cfg.K == 37 and nt.cfg.duration == model.duration == 321
    one_finite_step(315)
    growth.adjust_temp_opa(model, nt)
    one_finite_step(30)
    assert nt.steps() == steps + 4
    nt.close()


# ------------------------------------------------------------------------------------------------ 6. the census kernel
N_A = (0, 1, 3, 4, 5, 63 * 3, 64 * 3, 65 * 3, 257 * 3, 4099 * 3)
N_B = (0, 15, 17 * 15, 1031 * 15)


def _census(a, b, flags):
    flags.fill_(-1)                                            # 0xFF in every byte: the call has to write both words
    with _abi.stream(flags.device) as stream:
        _abi.call("ex4d_nan_any", _abi.ptr(a), a.numel(), _abi.ptr(b), b.numel(), flags.data_ptr(), stream)
    return flags.tolist()


def _edge_positions(x):
    """Indices of x worth a NaN: first, last, the element on each side of the first and of the last 16-byte boundary inside it, and
    every element of the scalar tail (after the last boundary)."""
    n = x.numel()
    bounds = [i for i in range(n) if (x.data_ptr() + 4 * i) % 16 == 0 and i > 0]
    pos = {0, n - 1}
    for i in bounds[:1] + bounds[-1:]:
        pos |= {i - 1, i}
    if bounds:
        pos |= set(range(bounds[-1], n))
    return sorted(p for p in pos if 0 <= p < n)


@pytest.mark.parametrize("offset", [0, 1])
def test_nan_census_kernel_against_torch(hip_lib, offset):
    g = torch.Generator().manual_seed(5)
    base_a = torch.randn(max(N_A) + 8, generator=g).to(DEV)
    base_b = torch.randn(max(N_B) + 8, generator=g).to(DEV)
    assert base_a.data_ptr() % 16 == 0 and base_b.data_ptr() % 16 == 0
    flags = torch.empty(2, dtype=torch.int32, device=DEV)
    nan = float("nan")
    for n_a in N_A:
        a = base_a[offset:offset + n_a]
        for n_b in N_B:
            b = base_b[offset:offset + n_b]
            assert _census(a, b, flags) == [0, 0] == [int(torch.isnan(a).any()), int(torch.isnan(b).any())], (n_a, n_b)
    # one NaN at every edge position of one array, the other array clean, for every size of the array
    for which, sizes, base, other in ((0, N_A, base_a, base_b[offset:offset + 17 * 15]), (1, N_B, base_b, base_a[offset:offset + 65 * 3])):
        for n in sizes:
            x = base[offset:offset + n]
            for i in _edge_positions(x):
                keep = float(x[i])
                x[i] = nan
                got = _census(x, other, flags) if which == 0 else _census(other, x, flags)
                want = [int(torch.isnan(x).any()), 0] if which == 0 else [0, int(torch.isnan(x).any())]
                x[i] = keep
                assert got == want and want[which] == 1, (which, n, i, got)
            # a NaN right outside the array (the float before it / after it) is not the array's
            if offset == 1 and n > 0:
                lo, hi = float(base[0]), float(base[offset + n])
                base[0] = nan; base[offset + n] = nan
                got = _census(x, other, flags) if which == 0 else _census(other, x, flags)
                base[0] = lo; base[offset + n] = hi
                assert got == [0, 0], (which, n, got)
    # both at once; a NULL pointer for an empty array
    a, b = base_a[offset:offset + 257 * 3], base_b[offset:offset + 1031 * 15]
    a[100] = nan; b[-1] = nan
    assert _census(a, b, flags) == [1, 1]
    assert _census(a, base_b[:0], flags) == [1, 0] and _census(base_a[:0], b, flags) == [0, 1] and _census(base_a[:0], base_b[:0], flags) == [0, 0]


def test_nan_census_special_values_and_graph_replay(hip_lib):
    flags = torch.empty(2, dtype=torch.int32, device=DEV)
    words = lambda *w: torch.tensor([x - 2 ** 32 if x >= 2 ** 31 else x for x in w], dtype=torch.int32, device=DEV).view(torch.float32)
    # +-Inf, -0, the smallest and largest denormal (both signs), FLT_MAX (both signs): none is a NaN
    finite = words(0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x007FFFFF, 0x80000001, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000000)
    assert not torch.isnan(finite).any()
    pad = torch.ones(64 * 3, device=DEV)
    for k in range(finite.numel()):
        x = pad.clone(); x[7] = finite[k]; x[-1] = finite[k]
        assert _census(x, finite, flags) == [0, 0], k
    # quiet NaN with the sign bit, signalling NaN with the smallest payload, a non-default payload, all mantissa bits, both signs
    for w in (0xFFC00000, 0x7F800001, 0xFF800001, 0x7FC12345, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FC00000):
        x = pad.clone(); x[6:7] = words(w)
        assert bool(torch.isnan(x).any()) and _census(x, pad, flags) == [1, 0] and _census(pad, x, flags) == [0, 1], hex(w)
    # one capture, replayed with the NaN moved between replays
    a, b = torch.randn(4099 * 3, device=DEV), torch.randn(1031 * 15, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _census(a, b, flags)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with _abi.stream(flags.device) as stream:
            _abi.call("ex4d_nan_any", a.data_ptr(), a.numel(), b.data_ptr(), b.numel(), flags.data_ptr(), stream)
    for place in ((a, 12000), None, (b, 3), (a, 1), None):
        if place is not None:
            place[0][place[1]] = float("nan")
        flags.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert flags.tolist() == [int(torch.isnan(a).any()), int(torch.isnan(b).any())] == [int(place is not None and place[0] is a),
                                                                                              int(place is not None and place[0] is b)], place
        if place is not None:
            place[0][place[1]] = 0.0


# ------------------------------------------------------------------------------------------------ 7. the census in the trainer
def test_census_reports_a_nan_the_optimizer_wrote_and_the_prune_removes_that_row(hip_lib):
    from ex4dgs_amd import densify
    from ex4dgs_amd.native_trainer import NativeTrainer
    model, cam, bg = _scene()
    gt = _gt(cam)
    nt = NativeTrainer(model, cam, optimizer=True, lrs=_lrs(model))
    stats = densify.DensityStats(model)
    nt.step(cam, bg, 0, gt, l1_accum=True, stats=stats, nan_census=True)
    assert nt.report()[1:] == (0, 0)
    row = 700
    m = nt.moments()["_xyz"][0]
    m[row, 1] = float("nan")
    nt.write_moment("_xyz", 0, m)                              # ex4d_trainer_write: the parameters rendered below are still clean
    nt.step(cam, bg, 137, gt, l1_accum=True, stats=stats, nan_census=True)
    loss, nan_s, nan_d = nt.report()
    assert 0 < loss < 10 and (nan_s, nan_d) == (1, 0)
    xyz = model._xyz.detach().clone()
    bad = torch.isnan(xyz).any(dim=1)
    assert bad.nonzero().flatten().tolist() == [row]
    ns, nd = model.num_static, model.num_dynamic
    out = densify.prune_nan_points(model, stats, nt)
    assert (model.num_static, model.num_dynamic) == (ns - 1, nd) == (out["static"]["rows"], out["dynamic"]["rows"])
    assert torch.equal(model._xyz, torch.cat([xyz[:row], xyz[row + 1:]]))            # exactly that row, the others as they were
    assert all(torch.isfinite(mv).all() for pair in nt.moments().values() for mv in pair) and nt.steps() == 2
    nt.step(cam, bg, 41, gt, l1_accum=True, stats=stats, nan_census=True)
    loss, nan_s, nan_d = nt.report()
    assert 0 < loss < 10 and (nan_s, nan_d) == (0, 0)
    nt.close()
