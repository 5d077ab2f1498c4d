"""ex4dgs_amd.motion without a GPU: the float64 restatement of tests/motion_ref.py against the reference's own getters and autograd
(tests/golden/motion.npz), the refusals of ex4d_motion_forward / ex4d_motion_backward with their messages, the time scalars and the
window hint of two timestamps, the module without a device, and the census of the scenes the GPU tests use (the CPU oracle's radii:
at least half of all rows visible in both frames, every class of row present where the timestamps lie intervals apart)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import motion_ref as mr


@pytest.fixture(scope="module")
def z():
    return mr.load()


def _state(z, interp, K):
    return {n: z[f"{mr.key(interp, K)}/param/{n}"] for n in mr.NAMES}


# ---------------------------------------------------------------------------------------------- the restatement against the fixture
@pytest.mark.parametrize("interp,K,Ns,Nd", mr.fixture_cases())
def test_restatement_reproduces_the_reference_positions_and_gradients(z, interp, K, Ns, Nd):
    cam = mr.camera()
    P, W = _state(z, interp, K), z[f"{mr.key(interp, K)}/weight"]
    assert P["_xyz"].shape == (Ns, 3) and P["_xyz_motion"].shape == (Nd, K, 3) and W.shape == (Ns + Nd, 3)
    nans = 0
    for name, (t0, t1) in mr.pairs(interp, K).items():
        base = mr.key(interp, K, name)
        for t, x in ((t0, "x0"), (t1, "x1")):
            for dtype, tag, bar in ((torch.float64, "f64/", 1e-13), (torch.float32, "", 1e-6)):
                got = mr.positions(*[torch.tensor(P[n]).to(dtype) for n in mr.NAMES], t, interp).numpy()
                ref = z[f"{base}/{tag}{x}"]
                assert got.dtype == ref.dtype and np.abs(got - ref).max() <= bar * max(1, np.abs(ref).max()), (base, x, tag)
        for space in ("world", "screen"):
            grads = mr.gradients(P, W, t0, t1, interp, space, cam)
            for n in mr.NAMES:
                mr.check_grad(f"{base}/{space}/{n}", grads[n], z[f"{base}/{space}/grad/{n}"], bar=1e-12)
            nan32 = z[f"{base}/{space}/nan32"]
            assert np.array_equal(np.isnan(grads["_xyz_motion"]), nan32), "float32 and float64 runs of the reference disagree on NaN"
            nans += int(nan32.sum())
            if space == "world":
                assert not grads["_xyz"].any()
            # outside the two windows the dense gradient is zero
            keep = np.ones(K, bool)
            for t in (t0, t1):
                first, count = mr.window(interp, t)
                keep[first:first + count] = False
            assert not np.nan_to_num(grads["_xyz_motion"][:, keep], nan=1.0).any()
    assert (nans > 0) == (interp == "pchip"), "the constant tracks give NaN under pchip and only there"


def test_fixture_is_small_and_holds_data_only():
    import os
    assert os.path.getsize(mr.GOLDEN) < 400 * 1024
    with np.load(mr.GOLDEN, allow_pickle=False) as f:
        assert all(f[k].dtype.kind in "fb" for k in f.files)


# ---------------------------------------------------------------------------------------------- time scalars and the window hint
@pytest.mark.parametrize("interp", mr.INTERPS)
def test_time_scalars_of_two_timestamps_and_the_window_hint(interp):
    from ex4dgs_amd import _abi
    from ex4dgs_amd.attributes import Ex4dAttrParams, interp_code, time_scalars
    lib = _abi.load()
    for K in (mr.K_MANY, mr.k_min(interp)):
        for t0, t1 in mr.pairs(interp, K).values():
            scal = []
            for t in (t0, t1):
                a = Ex4dAttrParams()
                _abi.call("ex4d_attr_time_scalars", interp_code(interp), float(mr.DURATION), float(mr.INTERVAL), float(mr.time_shift(interp)),
                          float(mr.VAR_PAD), 0, 0, K, float(t), C.byref(a))
                b = time_scalars(t, 0, 0, K, mr.DURATION, mr.INTERVAL, mr.time_shift(interp), mr.VAR_PAD, interp)
                assert bytes(a) == bytes(b)
                k, d = mr.time_index(interp, t)
                assert a.k == k and a.delta == np.float32(d)
                assert (1 if interp != "linear" else 0) <= k <= (K - 3 if interp != "linear" else K - 2)
                scal.append(a)
            # no rows: the call validates, writes the host hint and launches nothing
            hint = (C.c_int32 * 4)(-1, -1, -1, -1)
            rc = lib.ex4d_motion_backward(C.byref(scal[0]), C.byref(scal[1]), interp_code(interp), 0, *[None] * 5, 0, 0, 0.0, *[None] * 5, hint, None)
            assert rc == 0 and tuple(hint) == mr.window(interp, t0) + mr.window(interp, t1)
    assert mr.time_index(interp, 7)[1] == 0.0 and mr.time_index(interp, 2)[1] == 0.0 and mr.time_index(interp, -3) == (1 if interp != "linear" else 0, 0.0)


# ---------------------------------------------------------------------------------------------- refusals
def _scal(interp, t, Ns=4, Nd=4, K=mr.K_MANY):
    from ex4dgs_amd.attributes import time_scalars
    return time_scalars(t, Ns, Nd, K, mr.DURATION, mr.INTERVAL, mr.time_shift(interp), mr.VAR_PAD, interp)


def _both(a0, a1, interp, space, vm=None, pm=None, W=0, H=0):
    """Call the forward and the backward entry with fake (never dereferenced) tensor pointers: every refusal comes before a launch."""
    from ex4dgs_amd import _abi
    lib = _abi.load()
    fake = 256
    texts = []
    for name, tail in (("ex4d_motion_forward", (fake, None)), ("ex4d_motion_backward", (fake,) * 5 + ((C.c_int32 * 4)(), None))):
        with pytest.raises(RuntimeError) as e:
            _abi.call(name, C.byref(a0), C.byref(a1), interp, space, fake, fake, fake, vm, pm, W, H, 0.2, *tail)
        assert str(e.value) == lib.ex4d_motion_last_error().decode() != ""
        texts.append(str(e.value))
    assert texts[0] == texts[1]
    return texts[0]


def test_refusals_come_before_any_launch_with_their_message():
    a0, a1 = _scal("cube", 0.5), _scal("cube", 1.5)
    assert "unknown interpolator 3" in _both(a0, a1, 3, 0)
    assert "unknown interpolator -1" in _both(a0, a1, -1, 0)
    assert "unknown space 2" in _both(a0, a1, 0, 2)
    assert "unknown space -1" in _both(a0, a1, 0, -1)
    for field in ("Ns", "Nd", "K"):
        b = _scal("cube", 1.5)
        setattr(b, field, getattr(b, field) + 1)
        assert "disagree" in _both(a0, b, 0, 0) and field in _both(a0, b, 0, 0)
    # a keyframe index outside the interpolator's range, at either timestamp: cube / pchip 1 .. K-3, linear 0 .. K-2
    for interp, code, lo, hi in (("cube", 0, 1, mr.K_MANY - 3), ("pchip", 2, 1, mr.K_MANY - 3), ("linear", 1, 0, mr.K_MANY - 2)):
        for bad in (lo - 1, hi + 1):
            for which in (0, 1):
                pair = [_scal(interp, 0.5), _scal(interp, 1.5)]
                pair[which].k = bad
                text = _both(pair[0], pair[1], code, 0)
                assert f"keyframe index {bad} of t{which}" in text
        ok = [_scal(interp, 0.5), _scal(interp, 1.5)]
        ok[0].k, ok[1].k = lo, hi
        assert "screen space needs viewmatrix" in _both(ok[0], ok[1], code, 1, None, None, 96, 64)      # the range itself passes
    assert "screen space needs viewmatrix" in _both(a0, a1, 0, 1, None, 256, 96, 64)
    assert "screen space needs viewmatrix" in _both(a0, a1, 0, 1, 256, None, 96, 64)
    assert "screen space needs viewmatrix" in _both(a0, a1, 0, 1, 256, 256, 0, 64)


def test_the_status_functions_report_through_their_own_error_text():
    from ex4dgs_amd import _abi, attributes
    assert {"ex4d_motion_last_error", "ex4d_motion_forward", "ex4d_motion_backward"} <= set(attributes.EXPORTS)
    assert _abi._LAST_ERROR["ex4d_motion_forward"] == _abi._LAST_ERROR["ex4d_motion_backward"] == "ex4d_motion_last_error"
    assert _abi._LAST_ERROR["ex4d_attributes_forward_ex"] == "ex4d_attributes_last_error"


# ---------------------------------------------------------------------------------------------- the module without a device
def test_module_imports_without_a_gpu_and_refuses_cpu_tensors():
    from ex4dgs_amd import motion
    from ex4dgs_amd.scene import DynamicGaussians
    P = {n: torch.tensor(v) for n, v in mr.state(3, 4, mr.K_MANY).items()}
    for call in (lambda: motion.displacement(P, 0.5, 1.5, **mr.model_kwargs("cube")),
                 lambda: motion.displacement(P, 0.5, 1.5, space="screen", camera=mr.camera(), **mr.model_kwargs("cube")),
                 lambda: mr.cpu_model(P, "cube").get_displacement(0.5, 1.5)):
        with pytest.raises(RuntimeError, match="only run on a ROCm GPU"):
            call()
    with pytest.raises(ValueError, match="unknown space"):
        motion.displacement(P, 0.5, 1.5, space="view", **mr.model_kwargs("cube"))
    with pytest.raises(ValueError, match="needs a camera"):
        motion.displacement_raw(_scal("cube", 0.5, 3, 4), _scal("cube", 1.5, 3, 4), P["_xyz"], P["_xyz_disp"], P["_xyz_motion"], space="screen")
    with pytest.raises(ValueError, match="unknown interp_type"):
        motion.displacement(P, 0.5, 1.5, interp_type="spline")
    assert isinstance(DynamicGaussians.get_displacement.__doc__, str)
    d = motion.dense_from_windows(torch.ones(2, 4, 3), 2 * torch.ones(2, 4, 3), (1, 4, 2, 4), 8)
    assert d[0, :, 0].tolist() == [0, 1, 3, 3, 3, 2, 0, 0]


def test_render_takes_flow_to_and_the_policy_hook_exists():
    import inspect
    from ex4dgs_amd import render
    from ex4dgs_amd.diff_gaussian_rasterization_df import expect_flow, _flow_expected
    assert inspect.signature(render.render).parameters["flow_to"].default is None
    with expect_flow():
        assert _flow_expected
    assert not _flow_expected


# ---------------------------------------------------------------------------------------------- the scenes of the GPU screen test
@pytest.mark.parametrize("interp,shapes", [(interp, mr.SHAPES) for interp in mr.INTERPS])
def test_oracle_radii_give_the_gpu_screen_test_its_rows(interp, shapes):
    """The conditions of tests/test_gpu_motion.py::test_screen_displacement..., on the CPU oracle's frames: at least half of all rows have a
    geometry record (radii > 0) in both frames; where the timestamps lie intervals apart and the scene has its dynamic classes (Nd >= 255)
    every class of row is present."""
    cam = mr.camera()
    for Ns, Nd in shapes:
        P = mr.state(Ns, Nd, mr.K_MANY)
        for name, (t0, t1) in mr.pairs(interp, mr.K_MANY).items():
            (f0, z0), (f1, z1) = mr.oracle_frame(P, t0, interp, cam), mr.oracle_frame(P, t1, interp, cam)
            classes = mr.row_classes(f0["radii"], f1["radii"], z0, z1)
            assert 2 * int(classes["visible_both"].sum()) >= Ns + Nd, (Ns, Nd, name)
            if name in mr.CLASS_PAIRS and Nd >= 255:
                assert all(v.any() for v in classes.values()), (Ns, Nd, name, {k: int(v.sum()) for k, v in classes.items()})
