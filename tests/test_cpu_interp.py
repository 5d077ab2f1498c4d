"""The 'linear' and 'pchip' position interpolators without a GPU: tests/golden/model_getters_interp.npz (the reference's CGaussianModel,
tests/interp_ref.py for the layout) against the numpy restatement and against the torch getters of scene.DynamicGaussians at HALF the
bars the GPU tests use, the census of the pchip branches, ex4d_attr_time_scalars against the Python-number arithmetic for all three
interpolators, time_shift / keyframe_count, and the refusals."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import interp_ref as ir

CASES = [(cfg, t) for cfg in ir.CONFIGS for t in ir.CONFIGS[cfg]["timestamps"]]


@pytest.fixture(scope="module")
def z():
    return ir.load()


def test_fixture_layout_and_census(z):
    assert tuple(z["families"]) == ir.FAMILIES
    for cfg, c in ir.CONFIGS.items():
        shift = c["time_pad"] if c["interp"] == "linear" else c["time_pad"] + c["interval"]
        assert c["time_shift"] == shift and c["K"] == math.ceil((c["duration"] + shift + 2 * c["time_pad"] + 1) / c["interval"]) + 3
        assert z[f"{cfg}/param/_xyz_motion"].shape[1:] == (c["K"], 3)
        ks = [ir.time_index(cfg, t)[0] for t in c["timestamps"]]
        deltas = [ir.time_index(cfg, t)[1] for t in c["timestamps"]]
        first = 0 if c["interp"] == "linear" else 1
        # the last index the reference's own assertion t <= duration + time_shift admits
        last = int((c["duration"] + 2 * shift) // c["interval"])
        assert min(ks) == first and max(ks) == last and last <= c["K"] - (2 if c["interp"] == "linear" else 3)
        assert 0.0 in deltas and any(float(t) != int(t) for t in c["timestamps"])
        for t in c["timestamps"]:
            assert -shift <= t <= c["duration"] + shift
    assert ir.time_index("pchip_b", 58)[0] == ir.CONFIGS["pchip_b"]["K"] - 3
    cfg = "pchip_b"
    P = ir.params(z, cfg)
    assert not ir.subnormal_products(P, cfg).any()
    fam = ir.FAMILIES
    rows = {name: z[f"{cfg}/family"] == i for i, name in enumerate(fam)}
    for t in ir.CONFIGS[cfg]["timestamps"]:
        comp, row = ir.census(P, cfg, t)
        for name in ir.CENSUS:
            assert np.array_equal(comp[name], z[f"{cfg}/{ir.tkey(t)}/census/{name}"])
            assert (comp[name].sum(0) >= ir.MIN_ROWS_PER_BRANCH).all(), (t, name, comp[name].sum(0))
        assert row["three_branches"].sum() >= ir.MIN_ROWS_PER_BRANCH and row["three_branches"][rows["mixed"]].all()
        # NaN keyframe gradients exactly on the rows with a vanishing s, in the reference's float32 AND float64 runs
        for sub in ("", "f64/"):
            g = z[f"{cfg}/{ir.tkey(t)}/{sub}grad/_xyz_motion"]
            assert np.array_equal(np.isnan(g).any(axis=(1, 2)), row["nan_gradient"])
            assert not np.isinf(g).any()
        g = z[f"{cfg}/{ir.tkey(t)}/grad/_xyz_motion"]
        both, one = comp["s_zero_both"], comp["s_zero_one"]
        nan_keys = np.isnan(g).sum(1)                                   # [Nd,3]: keyframes with NaN per component
        assert (nan_keys[both] == 4).all() and (nan_keys[one] == 3).all() and (nan_keys[~both & ~one] == 0).all()
        assert (rows["constant"] | rows["pingpong"] == both.all(1)).all() and (rows["pingpong_one"] == one.all(1)).all()
        # a == 0 / b == 0 with s != 0: finite
        assert np.isfinite(g[rows["flat"]]).all()
    # the ratio family spans the decades
    y = P["_xyz_motion"][rows["ratio"]]
    step = np.abs(np.diff(y, axis=1))
    with np.errstate(divide="ignore"):
        ratio = step[:, 1:] / step[:, :-1]
    assert ratio[np.isfinite(ratio)].max() >= 1e5 and ratio[ratio > 0].min() <= 1e-5
    # linear never yields NaN
    for cfg in ("lin_a", "lin_b"):
        for t in ir.CONFIGS[cfg]["timestamps"]:
            assert np.isfinite(z[f"{cfg}/{ir.tkey(t)}/grad/_xyz_motion"]).all()


@pytest.mark.parametrize("cfg,t", CASES)
def test_restatement_and_torch_getters_match_the_reference(z, cfg, t):
    P, W = ir.params(z, cfg), ir.weights(z, cfg)
    c = ir.CONFIGS[cfg]
    Ns = P["_xyz"].shape[0]
    for run in (ir.run_restatement, ir.run_getters):
        outs, grads = run(P, W, cfg, t)
        failures = ir.check(z, cfg, t, outs, grads, scale=0.5)[1]
        assert not failures, (run.__name__, ir.format_failures(failures))
    # the float32 restatement of the positions is the reference's arithmetic: same bits
    k = ir.time_index(cfg, t)[0]
    got = ir.position_forward(P["_xyz_motion"], k, ir.weights_of(cfg, t), c["interp"])
    assert np.array_equal(got.view(np.int32), z[f"{cfg}/{ir.tkey(t)}/xyz"][Ns:].view(np.int32))
    # its float64 twin against the reference run in float64
    P64 = ir.params(z, cfg, np.float64)
    got64 = ir.position_forward(P64["_xyz_motion"], k, ir.weights_of(cfg, t, np.float64), c["interp"])
    assert np.abs(got64 - z[f"{cfg}/{ir.tkey(t)}/f64/xyz"][Ns:]).max() <= 1e-13
    g64 = ir.position_backward(P64["_xyz_motion"], k, ir.weights_of(cfg, t, np.float64), ir.weights(z, cfg, np.float64)["xyz"][Ns:], c["interp"])
    r64 = z[f"{cfg}/{ir.tkey(t)}/f64/grad/_xyz_motion"]
    assert np.array_equal(np.isnan(g64), np.isnan(r64))
    assert np.nanmax(np.abs(g64 - r64)) <= 1e-12 * max(1.0, np.nanmax(np.abs(r64)))


def _python_scalars(interp, t, duration, interval, time_shift, var_pad):
    tp = t + time_shift
    d = (tp % interval) / interval
    if interp == "linear":
        h = (1 - d, 0.0, d, 0.0)
    else:
        h = (2 * d ** 3 - 3 * d ** 2 + 1, d ** 3 - 2 * d ** 2 + d, -2 * d ** 3 + 3 * d ** 2, d ** 3 - d ** 2)
    return int(tp // interval), [np.float32(x) for x in (t, max(duration, 1), d, *h, tp / interval, var_pad / interval)]


@pytest.mark.parametrize("interp", ["cube", "linear", "pchip"])
def test_time_scalars_entry_point_equals_the_python_arithmetic(interp):
    from ex4dgs_amd import _abi, attributes as A
    from ex4dgs_amd._abi import Ex4dAttrParams, Ex4dTrainerConfig
    lib = _abi.load()
    rng = np.random.default_rng(7)
    cases = [(300, 10, 2, t) for t in (-2, 0, 3, 8, 137, 137.5, 299, 302, 0.1, 9.999999, 29.999999999)]
    cases += [(50, 5, 3, t) for t in (-3, 0, 4.5, 27, 53, 58)]
    cases += [(int(rng.integers(1, 400)), float(rng.choice([1, 3, 5, 7.5, 10])), int(rng.integers(0, 4)), float(rng.uniform(-3, 300))) for _ in range(200)]
    fields = ("t", "duration", "delta", "h00", "h10", "h01", "h11", "tau", "var_min")
    for duration, interval, pad, t in cases:
        shift = pad if interp == "linear" else pad + interval
        out = Ex4dAttrParams()
        _abi.call("ex4d_attr_time_scalars", A.interp_code(interp), duration, interval, shift, 3, 5, 7, 40, t, C.byref(out))
        k, want = _python_scalars(interp, t, duration, interval, shift, 3)
        assert (out.Ns, out.Nd, out.K, out.k) == (5, 7, 40, k), (duration, interval, pad, t)
        got = [np.float32(getattr(out, f)) for f in fields]
        assert [g.tobytes() for g in got] == [w.tobytes() for w in want], (duration, interval, pad, t, got, want)
        py = A.time_scalars(t, 5, 7, 40, duration, interval, shift, 3, interp)
        assert bytes(py) == bytes(out)
        if interp == "cube":                          # the trainer's entry point is this call for the cube interpolator
            cfg = Ex4dTrainerConfig()
            cfg.Ns, cfg.Nd, cfg.K = 5, 7, 40
            cfg.duration, cfg.interval, cfg.time_shift, cfg.var_pad = duration, interval, shift, 3
            tr = Ex4dAttrParams()
            lib.ex4d_trainer_time_scalars(C.byref(cfg), t, C.byref(tr))
            assert bytes(tr) == bytes(out)
    with pytest.raises(RuntimeError, match="unknown interpolator"):
        _abi.call("ex4d_attr_time_scalars", 3, 300, 10, 12, 3, 1, 1, 35, 0.0, C.byref(Ex4dAttrParams()))
    assert A.INTERP_TYPES == ir.INTERP_CODE


def test_time_shift_keyframe_count_and_refusals():
    from ex4dgs_amd import attributes as A
    from ex4dgs_amd.scene import DynamicGaussians, make_scene
    for cfg, c in ir.CONFIGS.items():
        assert DynamicGaussians.keyframe_count(c["duration"], c["interval"], c["time_pad"], interp_type=c["interp"]) == c["K"]
    assert DynamicGaussians.keyframe_count() == 35 == DynamicGaussians.keyframe_count(interp_type="pchip")
    assert DynamicGaussians.keyframe_count(interp_type="linear") == 34
    for interp, shift, K in (("cube", 12, 35), ("linear", 2, 34), ("pchip", 12, 35)):
        model, _, _ = make_scene("cfg3", P=50, interp_type=interp)
        assert (model.interp_type, model.time_shift, model._xyz_motion.shape[1]) == (interp, shift, K)
        assert A.sliced_shapes(interp) == {"_xyz_motion": (2 if interp == "linear" else 4, 3), "_rotation_motion": (2, 4)}
    assert A.SLICED_SHAPES == A.sliced_shapes("cube")
    params = {n: getattr(model, n) for n in model.PARAM_NAMES}
    with pytest.raises(ValueError, match="cubic_diff.*reference"):
        DynamicGaussians(params, interp_type="cubic_diff")
    with pytest.raises(ValueError, match="unknown interp_type"):
        DynamicGaussians(params, interp_type="spline")
    with pytest.raises(ValueError, match="lerp.*reference.*quat_interpolation"):
        DynamicGaussians(params, rot_interp_type="lerp")
    with pytest.raises(ValueError):
        A.time_scalars(0, 1, 1, 35, 300, 10, 12, 3, "cubic_diff")
    with pytest.raises(ValueError):
        A.sliced_shapes("nearest")
    # the CPU getters refuse nothing they can evaluate: a linear model reads keyframes k, k+1 only (K = 2 suffices)
    two = {n: (v[:, :2].contiguous() if n in ("_xyz_motion", "_rotation_motion") else v) for n, v in params.items()}
    m = DynamicGaussians(two, duration=1, interval=10, time_pad=0, interp_type="linear")
    y = two["_xyz_motion"]
    assert torch.equal(m.get_xyz_at_t(2.5, mode=2), y[:, 0] * (1 - 0.25) + y[:, 1] * 0.25)
