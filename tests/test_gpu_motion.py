"""ex4dgs_amd.motion on the GPU (ex4dgs_amd/csrc/ex4d_motion.hip); states, camera, timestamp pairs, the float64 restatement and the
fixture of the reference's own getters: tests/motion_ref.py (tests/test_cpu_motion.py pins the restatement to the fixture and checks the
scenes' row classes on the CPU oracle).

  forward, world   bit for bit attributes.forward_raw(t1).means3D - forward_raw(t0).means3D; t0 == t1 gives exact zeros
  forward, screen  bit for bit the means2D / depths the rasterizer keeps in its geometry records at t0 and t1 (rows with radii > 0 in both
                   frames: at least half of all rows); rows at or behind `near` at either timestamp exact zeros; the remaining rows against
                   the float64 projection of the same float32 means within twice the error the rasterizer's own records have against it
  both             output buffers prefilled with 0xFF bytes; a captured graph replayed after the keyframes changed in place
  backward, world  bit for bit two sliced attribute backwards (t0 fed -g, t1 fed g): windows, hints, g_xyz_disp; g_xyz exact zeros
  backward         1e-5 * max(1, |reference|inf) per tensor against the float64 restatement and against the reference's autograd (fixture),
                   NaN where the reference has NaN (pchip, constant tracks); dense gradient from the two windows; the hint; exact zeros
                   for g_xyz in world space and for rows under the depth rule; the two windows in ex4d_radam_step_sliced
  render           flow_to=None unchanged; with flow_to "opticalflow" is the direct rasterizer call on the screen displacement; gradients
                   are the composition of the rasterizer's backward and the motion backward; under async_frames
"""
import math

import numpy as np
import pytest
import torch

from tests import motion_ref as mr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# The largest error of the rasterizer's OWN geometry records (means2D, depths) against the float64 projection of the float32 means they
# were computed from, relative to max(1, |value|), over every scene and timestamp of this file (measured before this test was written, on
# the CPU oracle, whose records the GPU's equal bit for bit; the screen test prints the GPU's figure on every run):
PROJ_ERR_UV, PROJ_ERR_Z = 9.67e-6, 1.49e-7
# rows without a record are held to twice that: the margin covers the one extra subtraction


def _params(P):
    from ex4dgs_amd.attributes import PARAM_ORDER
    return [torch.tensor(P[n]).to(DEV).contiguous() for n in PARAM_ORDER]


def _scal(interp, t, Ns, Nd, K):
    from ex4dgs_amd.attributes import time_scalars
    s = time_scalars(t, Ns, Nd, K, mr.DURATION, mr.INTERVAL, mr.time_shift(interp), mr.VAR_PAD, interp)
    assert s.k == mr.time_index(interp, t)[0]
    return s


def _xyz3(params):
    return params[0], params[1], params[7]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _poisoned(N):
    return torch.full((N, 3), -1, dtype=torch.int32, device=DEV).view(torch.float32)          # 0xFF bytes


def _cases(interp):
    for K in (mr.K_MANY, mr.k_min(interp)):
        for name, pair in mr.pairs(interp, K).items():
            yield K, name, pair


def _raster(cam, means3D, dir3D, opac, scales, rots, shs, **kw):
    from ex4dgs_amd import _C
    e = torch.Tensor([])
    bg = torch.zeros(3, device=DEV)
    sub = torch.zeros(cam.image_height, cam.image_width, 2, device=DEV)
    out = _C.rasterize_gaussians(bg, means3D, dir3D, e, opac, scales, rots, 1.0, e, cam.world_view_transform, cam.full_proj_transform,
                                 math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), 0.1, sub, cam.image_height, cam.image_width, shs, 3,
                                 cam.camera_center, False, mr.NEAR, 100.0, False, **kw)
    return dict(zip(("num_rendered", "color", "radii", "geom", "binning", "img", "depth", "acc", "flow", "idx"), out))


# ---------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("Ns,Nd", mr.SHAPES)
@pytest.mark.parametrize("interp", mr.INTERPS)
def test_world_displacement_is_the_difference_of_two_attribute_forwards_bit_for_bit(hip_lib, interp, Ns, Nd):
    from ex4dgs_amd.attributes import forward_raw
    from ex4dgs_amd.motion import displacement_raw
    for K, name, (t0, t1) in _cases(interp):
        params = _params(mr.state(Ns, Nd, K))
        s0, s1 = _scal(interp, t0, Ns, Nd, K), _scal(interp, t1, Ns, Nd, K)
        ref = forward_raw(s1, params, False, interp)[0] - forward_raw(s0, params, False, interp)[0]
        got = displacement_raw(s0, s1, *_xyz3(params), interp_type=interp)
        again = displacement_raw(s0, s1, *_xyz3(params), interp_type=interp, out=_poisoned(Ns + Nd))
        assert got.shape == (Ns + Nd, 3) and torch.equal(_bits(got), _bits(ref)), (K, name)
        assert torch.equal(_bits(again), _bits(ref)), (K, name, "poisoned buffer")
        if t0 == t1:
            assert not _bits(got).any(), "t0 == t1: exact (positive) zeros"
        else:
            assert got.abs().max() > 0


@pytest.mark.parametrize("Ns,Nd", mr.SHAPES)
@pytest.mark.parametrize("interp", mr.INTERPS)
def test_screen_displacement_carries_the_bits_of_the_rasterizers_geometry_records(hip_lib, interp, Ns, Nd):
    from ex4dgs_amd import _C
    from ex4dgs_amd.attributes import forward_raw
    from ex4dgs_amd.motion import displacement_raw
    cam = mr.camera().to(DEV)
    cam64 = mr.camera()
    N = Ns + Nd
    worst_uv = worst_z = rest_uv = rest_z = 0.0
    for K, name, (t0, t1) in _cases(interp):
        params = _params(mr.state(Ns, Nd, K))
        s0, s1 = _scal(interp, t0, Ns, Nd, K), _scal(interp, t1, Ns, Nd, K)
        frames = []
        for s in (s0, s1):
            means3D, rots, opac, scales, shs = forward_raw(s, params, True, interp)
            f = _raster(cam, means3D, torch.zeros_like(means3D), opac, scales, rots, shs)
            g = _C.geom_views(f["geom"], N)
            q64 = mr.project(means3D.cpu().double(), cam64)
            frames.append(dict(radii=f["radii"], uvz=torch.cat([g["means2D"], g["depths"][:, None]], 1).clone(), q64=q64))
            vis = (f["radii"] > 0).cpu()
            err = ((frames[-1]["uvz"].cpu().double() - q64).abs() / q64.abs().clamp_min(1.0))[vis]
            if err.numel():
                worst_uv, worst_z = max(worst_uv, float(err[:, :2].max())), max(worst_z, float(err[:, 2].max()))
        got = displacement_raw(s0, s1, *_xyz3(params), space="screen", camera=cam, near=mr.NEAR, interp_type=interp)
        again = displacement_raw(s0, s1, *_xyz3(params), space="screen", camera=cam, near=mr.NEAR, interp_type=interp, out=_poisoned(N))
        assert torch.equal(_bits(got), _bits(again)), (K, name, "poisoned buffer")
        both = (frames[0]["radii"] > 0) & (frames[1]["radii"] > 0)
        ref = frames[1]["uvz"] - frames[0]["uvz"]
        assert torch.equal(_bits(got[both]), _bits(ref[both])), (K, name, int((_bits(got[both]) != _bits(ref[both])).sum()))
        # the depth rule, decided on the float64 depth of the float32 means (no row of these scenes lies within rounding of `near`)
        z0, z1 = frames[0]["q64"][:, 2], frames[1]["q64"][:, 2]
        assert ((z0 - mr.NEAR).abs().min() > 1e-5) and ((z1 - mr.NEAR).abs().min() > 1e-5)
        behind = ((z0 <= mr.NEAR) | (z1 <= mr.NEAR)).to(DEV)
        assert not _bits(got[behind]).any(), (K, name, "rows behind min_depth are exact zeros")
        assert not (both & behind).any()
        rest = (~both & ~behind).cpu()
        if rest.any():
            d64 = (frames[1]["q64"] - frames[0]["q64"])[rest]
            scale = torch.maximum(frames[0]["q64"].abs(), frames[1]["q64"].abs()).clamp_min(1.0)[rest]
            err = (got.cpu().double()[rest] - d64).abs() / scale
            rest_uv, rest_z = max(rest_uv, float(err[:, :2].max())), max(rest_z, float(err[:, 2].max()))
        if K == mr.K_MANY:
            classes = mr.row_classes(frames[0]["radii"].cpu(), frames[1]["radii"].cpu(), z0.numpy(), z1.numpy())
            assert 2 * int(both.sum()) >= N, (K, name, "at least half of all rows are compared with the geometry records")
            if name in mr.CLASS_PAIRS and Nd >= 255:
                assert all(v.any() for v in classes.values()), (name, {k: int(v.sum()) for k, v in classes.items()})
        if t0 == t1:
            assert not _bits(got).any()
    print(f"{interp} Ns {Ns} Nd {Nd}: geometry records vs float64: uv {worst_uv:.3g} z {worst_z:.3g} (recorded {PROJ_ERR_UV:g}, {PROJ_ERR_Z:g}); "
          f"rows without a record vs float64: uv {rest_uv:.3g} z {rest_z:.3g}")
    assert rest_uv <= 2 * PROJ_ERR_UV and rest_z <= 2 * PROJ_ERR_Z


def test_a_captured_forward_replays_on_keyframes_changed_in_place(hip_lib):
    from ex4dgs_amd.motion import displacement_raw
    cam = mr.camera().to(DEV)
    Ns, Nd, K, interp = 257, 256, mr.K_MANY, "pchip"
    params = _params(mr.state(Ns, Nd, K))
    t0, t1 = mr.pairs(interp, K)["far"]
    s0, s1 = _scal(interp, t0, Ns, Nd, K), _scal(interp, t1, Ns, Nd, K)
    outs = {space: _poisoned(Ns + Nd) for space in ("world", "screen")}
    call = lambda space, out=None: displacement_raw(s0, s1, *_xyz3(params), space=space, camera=cam, near=mr.NEAR, interp_type=interp, out=out)
    before = {space: call(space).clone() for space in outs}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # one stream, two launches one after the other: no parallel branches
        for space, out in outs.items():
            call(space, out)
    other = _params(mr.state(Ns, Nd, K, seed=3))
    for i in (0, 1, 7):
        params[i].copy_(other[i])
    graph.replay()
    torch.cuda.synchronize()
    for space, out in outs.items():
        fresh = call(space)
        assert torch.equal(_bits(out), _bits(fresh)) and not torch.equal(_bits(out), _bits(before[space])), space


# ---------------------------------------------------------------------------------------------- backward
def _backward(interp, space, P, params, t0, t1, W, cam):
    from ex4dgs_amd.motion import dense_from_windows, displacement_backward_raw
    Ns, Nd, K = P["_xyz"].shape[0], P["_xyz_motion"].shape[0], P["_xyz_motion"].shape[1]
    s0, s1 = _scal(interp, t0, Ns, Nd, K), _scal(interp, t1, Ns, Nd, K)
    g_xyz, g_disp, w0, w1, hint = displacement_backward_raw(s0, s1, *_xyz3(params), torch.tensor(W).to(DEV), space=space, camera=cam,
                                                            near=mr.NEAR, interp_type=interp)
    assert hint == mr.window(interp, t0) + mr.window(interp, t1)
    assert w0.shape == w1.shape == (Nd, hint[1], 3) and g_xyz.shape == g_disp.shape == (Ns, 3)
    dense = dense_from_windows(w0, w1, hint, K)
    return dict(_xyz=g_xyz, _xyz_disp=g_disp, _xyz_motion=dense), (w0, w1, hint)


@pytest.mark.parametrize("space", ["world", "screen"])
@pytest.mark.parametrize("interp", mr.INTERPS)
def test_backward_matches_the_float64_restatement(hip_lib, interp, space):
    """Every shape, every pair (coinciding, overlapping and disjoint windows among them).  Rows with a constant track give NaN under pchip,
    as the restatement's autograd does."""
    cam = mr.camera().to(DEV)
    cam64 = mr.camera()
    worst = {}
    for Ns, Nd in mr.SHAPES:
        for K, name, (t0, t1) in _cases(interp):
            P = mr.state(Ns, Nd, K)
            params = _params(P)
            W = mr.functional(Ns + Nd)
            got, _ = _backward(interp, space, P, params, t0, t1, W, cam)
            ref = mr.gradients(P, W, t0, t1, interp, space, cam64)
            for n in mr.NAMES:
                e = mr.check_grad(f"{interp}/{space}/{Ns}+{Nd}/K{K}/{name}/{n}", got[n].cpu().numpy(), ref[n])
                worst[n] = max(worst.get(n, 0.0), e)
            if space == "world":
                assert not _bits(got["_xyz"]).any(), "g_xyz in world space is exact zeros"
            else:
                x0, x1 = (mr.positions(*[torch.tensor(P[n]).double() for n in mr.NAMES], t, interp) for t in (t0, t1))
                behind = mr.screen_displacement(x0, x1, cam64)[1]
                assert not got["_xyz"].cpu()[behind[:Ns]].any() and not got["_xyz_disp"].cpu()[behind[:Ns]].any()
                assert not _bits(got["_xyz_motion"].cpu()[behind[Ns:]]).any(), "rows under the depth rule have zero gradients"
            if Nd and interp != "pchip" and t0 != t1:          # (t0 == t1: the two windows cancel exactly)
                assert got["_xyz_motion"].abs().max() > 0
    print(f"{interp}/{space}: worst error / max(1, |reference|inf):", {n: f"{e:.3g}" for n, e in worst.items()})


@pytest.mark.parametrize("interp,K,Ns,Nd", mr.fixture_cases())
def test_backward_matches_the_references_autograd_and_its_nan_pattern(hip_lib, interp, K, Ns, Nd):
    z = mr.load()
    cam = mr.camera().to(DEV)
    P = {n: z[f"{mr.key(interp, K)}/param/{n}"] for n in mr.NAMES}
    full = mr.state(Ns, Nd, K)
    assert all(np.array_equal(full[n], P[n]) for n in mr.NAMES)
    params, W = _params(full), z[f"{mr.key(interp, K)}/weight"]
    nans = 0
    for name, (t0, t1) in mr.pairs(interp, K).items():
        for space in ("world", "screen"):
            base = f"{mr.key(interp, K, name)}/{space}"
            got, _ = _backward(interp, space, P, params, t0, t1, W, cam)
            for n in mr.NAMES:
                mr.check_grad(f"{base}/{n}", got[n].cpu().numpy(), z[f"{base}/grad/{n}"])
            assert np.array_equal(np.isnan(got["_xyz_motion"].cpu().numpy()), z[f"{base}/nan32"])
            nans += int(z[f"{base}/nan32"].sum())
    assert (nans > 0) == (interp == "pchip")


@pytest.mark.parametrize("Ns,Nd", mr.SHAPES)
@pytest.mark.parametrize("interp", mr.INTERPS)
def test_world_backward_is_two_sliced_attribute_backwards_bit_for_bit(hip_lib, interp, Ns, Nd):
    """The adjoint's twin of the forward's pin: in world space the window of t1 carries the bits of the `_xyz_motion` slices the attribute
    backward gives at t1 for g_means3D = g, the window of t0 those at t0 for -g (NaN patterns included: pchip, constant tracks); the static
    rows get g_xyz = exact zeros and g_xyz_disp = the float32 sum of the two attribute results; the window hints are the attribute call's."""
    from ex4dgs_amd.attributes import backward_raw
    from ex4dgs_amd.motion import displacement_backward_raw
    g = torch.randn(Ns + Nd, 3, generator=torch.Generator().manual_seed(11)).to(DEV)
    for K, name, (t0, t1) in _cases(interp):
        params = _params(mr.state(Ns, Nd, K))
        s0, s1 = _scal(interp, t0, Ns, Nd, K), _scal(interp, t1, Ns, Nd, K)
        g_xyz, g_disp, w0, w1, hint = displacement_backward_raw(s0, s1, *_xyz3(params), g, interp_type=interp)
        (a0, hint0), (a1, hint1) = (backward_raw(s, params, [gm, None, None, None, None], with_shs=False, sliced=True, interp_type=interp)
                                    for s, gm in ((s0, -g), (s1, g)))
        assert hint == hint0[:2] + hint1[:2], (K, name)
        assert w0.shape == a0[7].shape and torch.equal(_bits(w0), _bits(a0[7])), (K, name, "window of t0")
        assert w1.shape == a1[7].shape and torch.equal(_bits(w1), _bits(a1[7])), (K, name, "window of t1")
        assert g_xyz.shape == (Ns, 3) and not _bits(g_xyz).any(), (K, name, "g_xyz: exact (positive) zeros")
        assert torch.equal(_bits(g_disp), _bits(a0[1] + a1[1])), (K, name, "g_xyz_disp")
        if Nd and interp != "pchip":
            assert torch.isfinite(w1).all() and w1.abs().max() > 0


@pytest.mark.parametrize("interp,pair", [("cube", "adjacent"), ("cube", "far"), ("cube", "same"), ("linear", "adjacent"), ("linear", "reverse")])
def test_the_two_windows_feed_the_sliced_radam_step_like_the_dense_gradient(hip_lib, interp, pair):
    from ex4dgs_amd.optim import radam_step_raw, radam_step_sliced_raw
    cam = mr.camera().to(DEV)
    Ns, Nd, K = 1, 255, mr.K_MANY
    P = mr.state(Ns, Nd, K)
    params = _params(P)
    t0, t1 = mr.pairs(interp, K)[pair]
    got, (w0, w1, hint) = _backward(interp, "screen", P, params, t0, t1, mr.functional(Ns + Nd), cam)
    dense = got["_xyz_motion"].contiguous()
    assert torch.isfinite(dense).all() and dense.abs().max() > 0
    A, B = params[7].clone(), params[7].clone()
    mA, vA, mB, vB = [torch.zeros_like(A) for _ in range(4)]
    for step in (1, 2, 3):
        radam_step_raw([(A.data_ptr(), dense.data_ptr(), mA.data_ptr(), vA.data_ptr(), A.numel(), 1e-2, step)], (0.9, 0.999), 1e-8, DEV)
        radam_step_sliced_raw([(B.data_ptr(), mB.data_ptr(), vB.data_ptr(), Nd, K, 3, 1e-2, step,
                                [(hint[0], hint[1], w0.data_ptr()), (hint[2], hint[3], w1.data_ptr())])], (0.9, 0.999), 1e-8, DEV)
    torch.cuda.synchronize()
    assert torch.equal(_bits(A), _bits(B)) and torch.equal(_bits(mA), _bits(mB)) and torch.equal(_bits(vA), _bits(vB))
    assert not torch.equal(A, params[7])


def test_autograd_surface_and_the_models_getter(hip_lib):
    from ex4dgs_amd.motion import displacement
    from ex4dgs_amd.scene import DynamicGaussians
    cam = mr.camera().to(DEV)
    cam64 = mr.camera()
    Ns, Nd, K, interp = 256, 257, mr.K_MANY, "cube"
    P = mr.state(Ns, Nd, K)
    t0, t1 = mr.pairs(interp, K)["adjacent"]
    W = mr.functional(Ns + Nd)
    model = DynamicGaussians({n: torch.tensor(v).to(DEV).requires_grad_(True) for n, v in P.items()}, duration=mr.DURATION, interval=mr.INTERVAL,
                             time_pad=mr.TIME_PAD, var_pad=mr.VAR_PAD, interp_type=interp)
    for space in ("world", "screen"):
        model.zero_grad()
        out = model.get_displacement(t0, t1, space=space, camera=cam, near=mr.NEAR)
        direct = displacement({n: getattr(model, n) for n in mr.NAMES}, t0, t1, space=space, camera=cam, near=mr.NEAR, **mr.model_kwargs(interp))
        assert torch.equal(_bits(out.detach()), _bits(direct.detach()))
        ref64 = mr.displacement(P, t0, t1, interp, space, cam64)[0]
        assert (out.detach().cpu().double() - ref64).abs().max() <= 1e-4 * max(1.0, float(ref64.abs().max()))
        assert torch.equal(model.get_displacement(t0, t1, mode=1, space=space, camera=cam).detach(), out.detach()[:Ns])
        assert torch.equal(model.get_displacement(t0, t1, mode=2, space=space, camera=cam).detach(), out.detach()[Ns:])
        (out * torch.tensor(W).to(DEV)).sum().backward()
        ref = mr.gradients(P, W, t0, t1, interp, space, cam64)
        for n in mr.NAMES:
            assert getattr(model, n).grad.shape == getattr(model, n).shape
            mr.check_grad(f"{space}/{n}", getattr(model, n).grad.cpu().numpy(), ref[n])
    with torch.no_grad():
        assert not model.get_displacement(t0, t1).requires_grad


# ---------------------------------------------------------------------------------------------- render
T_RENDER, T_FLOW = 137.5, 150.0


def _scene():
    from ex4dgs_amd.scene import SceneConfig, make_scene
    cfg = SceneConfig("motion: 2000 static+dynamic, 64x48", 2000, 64, 48, 60.0, dyn_frac=0.3, z_lo=4.5, z_hi=30.0, sigma_px_med=3.0, seed=23)
    model, cam, bg = make_scene(cfg, device=DEV, fused=True)
    return model, cam.to(DEV), bg.to(DEV)


def _direct(model, cam, bg, t, dir3D):
    """The rasterizer called directly on the attribute forward's outputs at t (no autograd)."""
    from ex4dgs_amd import _C
    from ex4dgs_amd.attributes import forward_raw, time_scalars
    params = [p.detach() for p in model.parameters()]
    s = time_scalars(t, model.num_static, model.num_dynamic, model._xyz_motion.shape[1], model.duration, model.interval, model.time_shift,
                     model.var_pad, model.interp_type)
    means3D, rots, opac, scales, _ = forward_raw(s, params, False, model.interp_type)
    shs = model.get_features()                 # the four feature tensors where they are (SplitSH), as render() hands them over
    assert isinstance(shs, _C.SplitSH)
    e = torch.Tensor([])
    sub = torch.zeros(cam.image_height, cam.image_width, 2, device=DEV)
    out = _C.rasterize_gaussians(bg, means3D, torch.zeros_like(means3D) if dir3D is None else dir3D, e, opac, scales, rots, 1.0, e,
                                 cam.world_view_transform, cam.full_proj_transform, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5),
                                 model.kernel_size, sub, cam.image_height, cam.image_width, shs, model.active_sh_degree, cam.camera_center,
                                 False, 0.2, 100.0, False)
    return dict(zip(("num_rendered", "render", "radii", "geom", "binning", "img", "depth", "acc", "opticalflow", "idx"), out))


SAME = ("render", "depth", "acc", "radii")


def test_render_without_flow_to_is_unchanged_and_with_it_composites_the_screen_displacement(hip_lib):
    from ex4dgs_amd.render import render
    model, cam, bg = _scene()
    with torch.no_grad():
        plain = render(cam, model, None, bg, timestamp=T_RENDER)
        zero = _direct(model, cam, bg, T_RENDER, None)
        for k in SAME + ("opticalflow",):
            assert torch.equal(plain[k], zero[k]), k
        assert not plain["opticalflow"].any() and not plain["viewspace_l1points"].any()
        disp = model.get_displacement(T_RENDER, T_FLOW, space="screen", camera=cam, near=0.2)
        flow = render(cam, model, None, bg, timestamp=T_RENDER, flow_to=T_FLOW)
        again = render(cam, model, None, bg, timestamp=T_RENDER, flow_to=T_FLOW)
        direct = _direct(model, cam, bg, T_RENDER, disp)
    assert torch.equal(_bits(flow["viewspace_l1points"]), _bits(disp))
    assert torch.equal(_bits(flow["opticalflow"]), _bits(direct["opticalflow"])) and torch.equal(_bits(flow["opticalflow"]), _bits(again["opticalflow"]))
    for k in SAME:
        assert torch.equal(flow[k], plain[k]), k
    assert flow["opticalflow"].abs().max() > 1e-3
    assert not flow["opticalflow"][:, plain["acc"][0] == 0].any(), "zero where nothing was hit"


def test_a_loss_on_the_optical_flow_reaches_the_keyframes_as_the_composition_of_the_two_backwards(hip_lib):
    from ex4dgs_amd.attributes import backward_raw, time_scalars
    from ex4dgs_amd.motion import dense_from_windows, displacement_backward_raw
    from ex4dgs_amd.render import render
    model, cam, bg = _scene()
    for n in model.PARAM_NAMES:
        setattr(model, n, getattr(model, n).detach().clone().requires_grad_(True))
    w = torch.randn(3, cam.image_height, cam.image_width, generator=torch.Generator().manual_seed(3)).to(DEV)
    # the four boundary tensors of this frame (the fused model caches them: render() consumes these very tensors)
    boundary = [model.get_xyz_at_t(T_RENDER), model.get_rotation_at_t(T_RENDER), model.get_opacity_at_t(T_RENDER), model.get_scaling()]
    for b in boundary:
        b.retain_grad()
    out = render(cam, model, None, bg, timestamp=T_RENDER, flow_to=T_FLOW)
    assert out["viewspace_l1points"].requires_grad
    (out["opticalflow"] * w).sum().backward()
    g_dir = out["viewspace_l1points"].grad
    assert g_dir is not None and g_dir.abs().max() > 0
    Ns, Nd, K = model.num_static, model.num_dynamic, model._xyz_motion.shape[1]
    scal = lambda t: time_scalars(t, Ns, Nd, K, model.duration, model.interval, model.time_shift, model.var_pad, model.interp_type)
    params = [p.detach() for p in model.parameters()]
    g_attr = backward_raw(scal(T_RENDER), params, [b.grad for b in boundary] + [None], with_shs=False, interp_type=model.interp_type)
    g_xyz, g_disp, w0, w1, hint = displacement_backward_raw(scal(T_RENDER), scal(T_FLOW), params[0], params[1], params[7], g_dir, space="screen",
                                                            camera=cam, near=0.2, interp_type=model.interp_type)
    expect = {"_xyz": g_attr[0] + g_xyz, "_xyz_disp": g_attr[1] + g_disp, "_xyz_motion": g_attr[7] + dense_from_windows(w0, w1, hint, K)}
    for n, ref in expect.items():
        got = getattr(model, n).grad
        scale = float(ref.abs().max())
        assert scale > 0 and got.abs().max() > 0, n
        err = float((got - ref).abs().max())
        print(f"{n}: |gradient - composition| {err:.3g} of {scale:.3g}; bit-equal: {torch.equal(_bits(got), _bits(ref))}")
        assert err <= 1e-6 * scale, (n, err, scale)
    # the displacement's own share is not nothing: without it the keyframes of the flow_to window would see no gradient at all
    only_flow = dense_from_windows(w0, w1, hint, K)
    assert only_flow.abs().max() > 0 and model._xyz_motion.grad[:, hint[2] + hint[3] - 1].abs().max() > 0


def test_a_flow_to_frame_under_async_frames_never_runs_on_the_flow_free_kernel(hip_lib):
    from ex4dgs_amd.diff_gaussian_rasterization_df import async_frames
    from ex4dgs_amd.render import render
    model, cam, bg = _scene()
    with torch.no_grad():
        sync_flow = render(cam, model, None, bg, timestamp=T_RENDER, flow_to=T_FLOW)
        sync_plain = render(cam, model, None, bg, timestamp=T_RENDER)
        async_frames.enable()
        try:
            for _ in range(4):                           # plain frames: the policy learns that there is no flow
                plain = render(cam, model, None, bg, timestamp=T_RENDER)
            async_frames.poll()
            assert async_frames.capacity > 0 and async_frames.no_flow, "the plain frames run asynchronously on the flow-free kernel"
            flow = render(cam, model, None, bg, timestamp=T_RENDER, flow_to=T_FLOW)
            async_frames.drain()                         # strict: an invalid frame raises here
            assert async_frames.invalid_frames == 0 and not async_frames.no_flow
            after = render(cam, model, None, bg, timestamp=T_RENDER)
            async_frames.drain()
        finally:
            async_frames.strict = False
            async_frames.disable()
            async_frames.strict = True
    for k in SAME + ("opticalflow",):
        assert torch.equal(flow[k], sync_flow[k]), k
        assert torch.equal(plain[k], sync_plain[k]) and torch.equal(after[k], sync_plain[k]), k
