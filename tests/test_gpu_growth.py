"""Growth of the dynamic set on the GPU (ex4dgs_amd.growth, the ex4d_growth_* entry points of include/ex4d_densify.h): the reference's
outputs (tests/golden/growth.npz) through torch.optim.RAdam, FusedRAdam and a FrameTrainer; the radix select against torch.quantile
on the device, bit for bit; classification and compaction beyond one workgroup against maps known by construction; expansion
against the restatement (tests/growth_ref.py); and the grown model through the fused attribute kernels and a FrameTrainer step."""
import types

import numpy as np
import pytest
import torch

from tests import densify_ref as D
from tests import growth_ref as R
from tests.test_cpu_growth import (EXPAND_CASES, EXTRACT_CASES, GENERATED, GOLD, assert_old_rows_untouched, assert_state, cfg_of,
                                   extract_kwargs, model_of, state_from)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
OPT_KINDS = ("radam", "fused", "trainer")
EMPTY = {"_xyz_motion": (0, 35, 3), "_rotation_motion": (0, 35, 4), "_opacity_motion": (0, 1), "_opacity_duration_center": (0, 2, 1),
         "_opacity_duration_var": (0, 2, 1), "_scaling_motion": (0, 3), "_features_dc_motion": (0, 1, 3), "_features_rest_motion": (0, 15, 3)}


def _shaped(k, t):
    # the all-static fixture holds 1-D empty tensors; the model takes them with 35 keyframes, which the first extraction must not read
    return t.reshape(EMPTY[k]) if t.numel() == 0 and k in EMPTY else t


def hip_setup(case, opt_kind):
    from ex4dgs_amd import densify
    from ex4dgs_amd.optim import FusedRAdam
    from ex4dgs_amd.scene import DynamicGaussians
    from ex4dgs_amd.trainer import FrameTrainer
    st = state_from(case, "pre", DEV)
    params = {k: torch.nn.Parameter(_shaped(k, v).contiguous()) for k, v in st["params"].items()}
    model = DynamicGaussians(params, duration=model_of(case)["duration"], interval=10, time_pad=2)
    stats = densify.DensityStats(model)
    for names, blk in ((D.S_STATS, stats.static), (D.D_STATS, stats.dynamic)):
        for i, k in enumerate(names):
            blk[i].copy_(st["stats"][k].view(-1))
    if opt_kind == "trainer":
        opt = FrameTrainer(model, optimizer=True)
        for i, k in enumerate(opt.names):
            opt.m[i], opt.v[i] = _shaped(k, st["m"][k]).clone(), _shaped(k, st["v"][k]).clone()
        opt.steps = 1
        return model, stats, opt
    cls = FusedRAdam if opt_kind == "fused" else torch.optim.RAdam
    opt = cls([{"params": [getattr(model, k)], "lr": 1e-3} for k in model.PARAM_NAMES], lr=1e-3)
    for k in model.PARAM_NAMES:
        opt.state[getattr(model, k)] = {"step": torch.tensor(float(GOLD[f"{case}/pre/step/{k}"])), "exp_avg": _shaped(k, st["m"][k]).clone(),
                                        "exp_avg_sq": _shaped(k, st["v"][k]).clone()}
    return model, stats, opt


def hip_state(model, stats, opt, empty_as_fixture=False):
    from ex4dgs_amd.trainer import FrameTrainer
    flat = lambda t: t.reshape(0) if empty_as_fixture and t.numel() == 0 else t
    out = {"params": {k: flat(getattr(model, k).detach()) for k in D.STATIC + D.DYNAMIC}, "m": {}, "v": {}, "stats": {}}
    for i, k in enumerate(model.PARAM_NAMES):
        if isinstance(opt, FrameTrainer):
            out["m"][k], out["v"][k] = flat(opt.m[i]), flat(opt.v[i])
        else:
            s = opt.state[getattr(model, k)]
            out["m"][k], out["v"][k] = flat(s["exp_avg"]), flat(s["exp_avg_sq"])
    for k in D.S_STATS + D.D_STATS:
        out["stats"][k] = getattr(stats, k)
    return out


def assert_steps_kept(model, opt, case):
    from ex4dgs_amd.trainer import FrameTrainer
    if isinstance(opt, FrameTrainer):
        assert opt.steps == 1 and all(a is b for a, b in zip(opt.params, [getattr(model, n) for n in opt.names]))
        return
    groups = [g["params"][0] for g in opt.param_groups]
    for k in model.PARAM_NAMES:                                  # state re-keyed to the new parameter objects, step kept
        p = getattr(model, k)
        assert any(p is q for q in groups), k
        assert float(opt.state[p]["step"]) == float(GOLD[f"{case}/post/step/{k}"]), k


# ------------------------------------------------------------------------------------------------- the reference's outputs
@pytest.mark.parametrize("opt_kind", OPT_KINDS)
def test_extraction_matches_reference(opt_kind):
    from ex4dgs_amd import growth
    for case in EXTRACT_CASES:
        model, stats, opt = hip_setup(case, opt_kind)
        vis, cam = torch.from_numpy(GOLD[f"{case}/vis"].copy()).to(DEV), torch.from_numpy(GOLD[f"{case}/cam"].copy())
        c = cfg_of(case)
        out = growth.extract_dynamic_points(model, stats, opt, cam, 0.0, vis, **extract_kwargs(case))
        assert out["visible"] == int(vis.sum()) and out["dynamic"]["clone"] == c["selected"], (case, out)
        assert out["static"]["rows"] == model.num_static == GOLD[f"{case}/post/param/_xyz"].shape[0]
        assert out["dynamic"]["rows"] == model.num_dynamic and model._xyz_motion.shape[1] == c["keyframe_num"]
        assert abs(out["threshold"] - c["theta64"]) <= 1e-5 * c["theta64"], (case, out["threshold"], c["theta64"])
        state = hip_state(model, stats, opt)
        assert_state(state, case, GENERATED["extract"])
        assert_old_rows_untouched(state, case)
        assert_steps_kept(model, opt, case)


@pytest.mark.parametrize("opt_kind", OPT_KINDS)
def test_expand_duration_and_adjust_temp_opa_match_reference(opt_kind):
    from ex4dgs_amd import growth
    for case in EXPAND_CASES:
        c = cfg_of(case)
        model, stats, opt = hip_setup(case, opt_kind)
        before = [getattr(model, k) for k in model.PARAM_NAMES]
        assert growth.expand_duration(model, opt, c["argument"]) is c["returned"], case
        assert model.duration == c["duration_after"], case
        assert_state(hip_state(model, stats, opt, empty_as_fixture=True), case, GENERATED["expand"] if c["returned"] else ())
        assert_steps_kept(model, opt, case)
        if c["returned"]:
            K = GOLD[f"{case}/pre/param/_xyz_motion"].shape[1]
            for k in ("_xyz_motion", "_rotation_motion"):
                np.testing.assert_array_equal(getattr(model, k).detach().cpu().numpy()[:, :K], GOLD[f"{case}/pre/param/{k}"], err_msg=k)
        else:                                                    # an early-out replaces nothing
            assert all(a is b for a, b in zip(before, [getattr(model, k) for k in model.PARAM_NAMES]))
    model, stats, opt = hip_setup("adjust", opt_kind)
    growth.adjust_temp_opa(model, opt)
    assert_state(hip_state(model, stats, opt), "adjust")
    assert_steps_kept(model, opt, "adjust")
    model, stats, opt = hip_setup("early_static", opt_kind)      # no dynamic rows: nothing happens
    before = model._opacity_duration_var
    growth.adjust_temp_opa(model, opt)
    assert model._opacity_duration_var is before


# ------------------------------------------------------------------------------------------------- the radix select
SELECT_COUNTS = (1, 2, 3, 51, 256, 257, 65537, 1_000_003)


def _patterns(n, g):
    base = (torch.rand(n, generator=g) ** 3 * 0.2).to(DEV)
    yield "random", base
    yield "equal", torch.full((n,), 0.37, device=DEV)
    yield "two values", torch.where(torch.rand(n, generator=g).to(DEV) < 0.97, torch.tensor(0.2, device=DEV), torch.tensor(0.7, device=DEV))
    yield "zeros", base * (torch.rand(n, generator=g).to(DEV) < 0.6)
    nan = base.clone()
    nan[n // 2] = float("nan")
    yield "one NaN", nan


@pytest.mark.parametrize("n", SELECT_COUNTS)
def test_threshold_equals_torch_quantile_bit_for_bit(n):
    """theta of the select against torch.quantile on the device over the same score vector: q (n - 1) in float32 (980 002 at
    n = 1 000 003), both order statistics found exactly, torch's lerp."""
    from ex4dgs_amd import growth
    g = torch.Generator().manual_seed(n)
    for name, s in _patterns(n, g):
        for q in (0.98, 0.8):
            u = s / (s.max() + 0.000001)
            want = torch.quantile(u, q)
            res = growth.quantile_threshold(s.contiguous(), q)
            got = res[growth.SELECT_THETA]
            words = res.view(torch.int32)
            assert int(words[growth.SELECT_COUNT]) == n, (name, n)
            if name == "one NaN":
                assert bool(torch.isnan(want)) and bool(torch.isnan(got)), (name, n, q)
                continue
            assert torch.equal(res[growth.SELECT_MAX], s.max()), (name, n)
            assert got.view(torch.int32).item() == want.view(torch.int32).item(), (name, n, q, float(got), float(want))


def test_threshold_skips_absent_entries_and_handles_none():
    from ex4dgs_amd import growth
    g = torch.Generator().manual_seed(9)
    s = (torch.rand(70001, generator=g) * 3).to(DEV)
    absent = torch.rand(70001, generator=g).to(DEV) < 0.3
    masked = torch.where(absent, torch.tensor(-1.0, device=DEV), s)
    present = s[~absent]
    res = growth.quantile_threshold(masked, 0.98)
    want = torch.quantile(present / (present.max() + 0.000001), 0.98)
    assert int(res.view(torch.int32)[growth.SELECT_COUNT]) == present.numel()
    assert res[0].view(torch.int32).item() == want.view(torch.int32).item()
    res = growth.quantile_threshold(torch.full((300,), -1.0, device=DEV), 0.98)
    assert bool(torch.isnan(res[0])) and float(res[1]) == 0.0 and int(res.view(torch.int32)[2]) == 0


# ------------------------------------------------------------------------------------------------- classification and compaction
CLASSIFY_ROWS = (1, 255, 256, 257, 513 * 256)


def _layouts(n):
    """Which rows move, by construction: needles at the block edges, whole blocks, every third row."""
    edges = sorted({a for a in (0, 255, 256, 511, 512, n - 1) if 0 <= a < n})
    needles = np.zeros(n, bool)
    needles[edges] = True
    blocks = np.zeros(n, bool)
    blocks[256:512] = True
    if n <= 256:
        blocks[:] = True
    if n > 1024:
        blocks[-256:] = True                                     # the last, partial-free block and a run across a boundary
        blocks[1000:1300] = True
    return {"needles": needles, "blocks": blocks, "third": np.arange(n) % 3 == 1, "none": np.zeros(n, bool)}


@pytest.mark.parametrize("n", CLASSIFY_ROWS)
def test_classification_and_map_beyond_one_workgroup(n):
    """The selected rows are fixed by |disp| against motion_thres * extent (the quantile term is off: percentile 1), the
    invisible and the never-seen among them stay: destination map, selection list and counts are known by construction."""
    from ex4dgs_amd import growth
    rng = np.random.default_rng(n)
    for name, big in _layouts(n).items():
        vis = rng.random(n) < 0.9
        seen = rng.random(n) < 0.9
        still = (rng.random(n) < 0.05) & ~big
        want = big & vis & seen
        norm = np.where(big, 2.0, np.where(still, 0.0, 0.5)).astype(np.float32)
        disp = np.zeros((n, 3), np.float32)
        disp[np.arange(n), rng.integers(0, 3, n)] = norm
        xyz = rng.standard_normal((n, 3)).astype(np.float32)
        stats = torch.zeros(9, n, device=DEV)
        stats[8] = torch.from_numpy(np.where(seen, rng.uniform(0, 300, n) * (rng.random(n) < 0.8), -1.0).astype(np.float32)).to(DEV)
        model = types.SimpleNamespace(_xyz=torch.from_numpy(xyz).to(DEV), _xyz_disp=torch.from_numpy(disp).to(DEV), num_static=n)
        mp, counts, selected, counts_out, result = growth._classify(model, types.SimpleNamespace(static=stats), torch.tensor([0.5, 0.2, 9.0], device=DEV),
                                                                    torch.from_numpy(vis).to(DEV).view(torch.uint8), 1.0, 1.0, 0.1)
        nsel = int(want.sum())
        keep = ~want
        exp_map = np.full((n, 8), -1, np.int32)
        exp_map[keep, 0] = np.arange(n - nsel, dtype=np.int32)
        np.testing.assert_array_equal(mp.cpu().numpy(), exp_map, err_msg=f"{name} {n}")
        np.testing.assert_array_equal(counts.cpu().numpy(), np.array([n - nsel, 0, 0, 0, 0, 0, 0, n - nsel], np.int32), err_msg=name)
        np.testing.assert_array_equal(counts_out.cpu().numpy(), np.array([nsel, n - nsel], np.int32), err_msg=name)
        np.testing.assert_array_equal(selected.cpu().numpy()[:nsel], np.nonzero(want)[0].astype(np.int32), err_msg=name)
        assert int(result.view(torch.int32)[growth.SELECT_COUNT]) == int(vis.sum())


def _random_state(ns, nd, K, seed):
    g = torch.Generator().manual_seed(seed)
    Rn = lambda *s: torch.randn(*s, generator=g).to(DEV)
    P = dict(_xyz=Rn(ns, 3), _xyz_disp=0.01 * Rn(ns, 3), _rotation=Rn(ns, 4), _opacity=Rn(ns, 1), _scaling=Rn(ns, 3) - 4, _features_dc=Rn(ns, 1, 3),
             _features_rest=0.2 * Rn(ns, 15, 3), _xyz_motion=torch.cumsum(0.2 * Rn(nd, K, 3), 1), _rotation_motion=Rn(nd, K, 4), _opacity_motion=Rn(nd, 1),
             _opacity_duration_center=torch.sort(2 + torch.rand(nd, 2, 1, generator=g).to(DEV) * (K - 5), dim=1)[0], _opacity_duration_var=Rn(nd, 2, 1),
             _scaling_motion=Rn(nd, 3) - 4, _features_dc_motion=Rn(nd, 1, 3), _features_rest_motion=0.2 * Rn(nd, 15, 3))
    stats = D.init_stats(ns, nd, device=DEV)
    for names, n in ((D.S_STATS, ns), (D.D_STATS, nd)):
        for k in names:
            stats[k] = torch.rand(stats[k].shape, generator=g).to(DEV) * 7
        ts = torch.rand(n, 1, generator=g).to(DEV) * 300
        stats[names[8]] = torch.where(torch.rand(n, 1, generator=g).to(DEV) < 0.1, torch.full_like(ts, -1.0), ts)
    return {"params": P, "m": {k: v * 0.37 + 3 for k, v in P.items()}, "v": {k: v * v + 0.1 for k, v in P.items()}, "stats": stats}


def _model_from(state, duration, opt_kind="fused"):
    from ex4dgs_amd import densify
    from ex4dgs_amd.optim import FusedRAdam
    from ex4dgs_amd.scene import DynamicGaussians
    model = DynamicGaussians({k: torch.nn.Parameter(v.clone()) for k, v in state["params"].items()}, duration=duration, interval=10, time_pad=2)
    stats = densify.DensityStats(model)
    for names, blk in ((D.S_STATS, stats.static), (D.D_STATS, stats.dynamic)):
        for i, k in enumerate(names):
            blk[i].copy_(state["stats"][k].view(-1))
    opt = None
    if opt_kind == "fused":
        opt = FusedRAdam([{"params": [getattr(model, k)], "lr": 1e-3} for k in model.PARAM_NAMES], lr=1e-3)
        for k in model.PARAM_NAMES:
            opt.state[getattr(model, k)] = {"step": torch.tensor(3.0), "exp_avg": state["m"][k].clone(), "exp_avg_sq": state["v"][k].clone()}
    return model, stats, opt


def _assert_against_restatement(model, stats, opt, ref, generated):
    for k, x in ref["params"].items():
        y = getattr(model, k).detach()
        assert y.shape == x.shape, (k, y.shape, x.shape)
        if k in generated:
            torch.testing.assert_close(y, x, rtol=1e-6, atol=1e-6, msg=lambda m: f"{k}: {m}")
        else:
            assert torch.equal(y, x), k
        if opt is not None:
            s = opt.state[getattr(model, k)]
            assert torch.equal(s["exp_avg"], ref["m"][k]) and torch.equal(s["exp_avg_sq"], ref["v"][k]) and float(s["step"]) == 3.0, k
    for k, x in ref["stats"].items():
        assert torch.equal(getattr(stats, k), x), k


def test_extraction_beyond_one_workgroup_against_restatement():
    """513 * 256 static rows, 257 dynamic ones, through the quantile: 97 % of the rows barely move, 2 % are copies of one row -- the
    0.98 quantile of the visible rows falls among them, so the threshold IS their score and none of them is above it -- and 1 % move
    several times as far again: selected, unless invisible or never seen.  Decided with margin in float32 and in the restatement."""
    from ex4dgs_amd import growth
    ns, nd, K = 513 * 256, 257, 35
    st = _random_state(ns, nd, K, 5)
    g = torch.Generator().manual_seed(6)
    P = st["params"]
    cls = torch.rand(ns, generator=g).to(DEV)
    P["_xyz"][:, 2] += 20.0                                       # |xyz - cam|^2 within [300, 500]: the groups' scores cannot meet
    twin = (cls >= 0.97) & (cls < 0.99)
    far = cls >= 0.99
    P["_xyz"][twin], P["_xyz_disp"][twin] = P["_xyz"][7].clone(), torch.tensor([0.4, 0.0, 0.3], device=DEV)      # |disp| 0.5: ten times the others' largest
    P["_xyz_disp"][far] = P["_xyz_disp"][far] * 100 + 5.0                                                          # |disp| > 3
    vis = torch.rand(ns, generator=g).to(DEV) < 0.9
    cam = torch.tensor([0.3, -0.2, 0.5])
    model, stats, opt = _model_from(st, 300)
    out = growth.extract_dynamic_points(model, stats, opt, cam, 17.0, vis, 5.0)
    ref = {k: ({a: b.clone() for a, b in v.items()}) for k, v in st.items()}
    info = R.extract(ref, {"interval": 10, "time_shift": 12, "time_pad": 2, "duration": 300}, cam, vis, 5.0)
    want = far & vis & (st["stats"]["xyz_error_min_timestamp"].view(-1) >= 0)
    assert torch.equal(info["mask"], want) and 800 < int(want.sum()) == out["dynamic"]["clone"]
    assert out["visible"] == int(vis.sum()) and out["static"]["rows"] == ns - int(want.sum()) and out["dynamic"]["rows"] == nd + int(want.sum())
    assert abs(out["threshold"] - info["threshold"]) <= 1e-6 * info["threshold"]       # (bit for bit: the select's own tests)
    _assert_against_restatement(model, stats, opt, ref, GENERATED["extract"])


def test_extraction_edges_no_visible_row_nothing_selected_all_static():
    from ex4dgs_amd import growth
    st = _random_state(300, 5, 35, 8)
    model, stats, opt = _model_from(st, 300)
    before = {k: getattr(model, k) for k in model.PARAM_NAMES}
    blocks = (stats.static, stats.dynamic)
    out = growth.extract_dynamic_points(model, stats, opt, [0.0, 0.0, 5.0], None, torch.zeros(300, dtype=torch.bool, device=DEV), 5.0)
    assert out["visible"] == 0 and out["dynamic"]["clone"] == 0 and out["static"]["rows"] == 300 and np.isnan(out["threshold"])
    assert all(getattr(model, k) is v for k, v in before.items()) and stats.static is blocks[0] and stats.dynamic is blocks[1]
    # visible rows, none selected (nothing moves further than min_motion_thres * extent): values kept, dynamic accumulators reset
    vis = torch.ones(300, dtype=torch.bool, device=DEV)
    out = growth.extract_dynamic_points(model, stats, opt, [0.0, 0.0, 5.0], None, vis, 5.0, min_motion_thres=10.0)
    assert out["visible"] == 300 and out["dynamic"]["clone"] == 0 and out["dynamic"]["rows"] == 5
    ref = {k: ({a: b.clone() for a, b in v.items()}) for k, v in st.items()}
    for k, init in zip(D.D_STATS[:7], D.INIT):
        ref["stats"][k] = torch.full_like(ref["stats"][k], init)
    _assert_against_restatement(model, stats, opt, ref, ())
    # an all-static model with nothing selected stays as it is
    st0 = _random_state(300, 0, 35, 9)
    model, stats, opt = _model_from(st0, 300)
    empty = model._xyz_motion
    out = growth.extract_dynamic_points(model, stats, opt, [0.0, 0.0, 5.0], None, vis, 5.0, min_motion_thres=10.0)
    assert out["visible"] == 300 and model._xyz_motion is empty and model.num_static == 300
    with pytest.raises(RuntimeError):
        growth.extract_dynamic_points(model, stats, opt, [0.0, 0.0, 5.0], None, vis[:299], 5.0)


# ------------------------------------------------------------------------------------------------- expansion
@pytest.mark.parametrize("nd", [1, 257])
@pytest.mark.parametrize("grow", [1, 7])
def test_expand_duration_against_restatement(nd, grow):
    """K = 35 -> 36 and 42 keyframes: the first K copied exactly, the new ones within the bar of generated values of the
    restatement; centres and vars exact (comparisons, minima and constants only); moments zeroed for the four tensors alone."""
    from ex4dgs_amd import growth
    argument = {1: 305, 7: 365}[grow]
    st = _random_state(64, nd, 35, 10 + nd + grow)
    st["params"]["_opacity_duration_center"] = torch.sort(27 + torch.rand(nd, 2, 1, generator=torch.Generator().manual_seed(nd)).to(DEV) * 12, dim=1)[0]
    model, stats, opt = _model_from(st, 300)
    ref = {k: ({a: b.clone() for a, b in v.items()}) for k, v in st.items()}
    rm = {"interval": 10, "time_shift": 12, "time_pad": 2, "duration": 300}
    assert R.expand_duration(ref, rm, argument) and growth.expand_duration(model, opt, argument)
    assert model.duration == rm["duration"] == argument + 1 and model._xyz_motion.shape == (nd, 35 + grow, 3) and model._rotation_motion.shape == (nd, 35 + grow, 4)
    _assert_against_restatement(model, stats, opt, ref, GENERATED["expand"])
    for k in ("_xyz_motion", "_rotation_motion"):
        assert torch.equal(getattr(model, k)[:, :35], st["params"][k]), k
        assert not opt.state[getattr(model, k)]["exp_avg"].any()
    assert opt.state[model._scaling_motion]["exp_avg"].any()


# ------------------------------------------------------------------------------------------------- the grown model in use
def _fused_equals_unfused(model, t):
    """The fused attribute kernels against the torch getters of DynamicGaussians at timestamp t: the bar of
    test_fused_attributes_vs_oracle_at_scale_and_render_equivalence, 2e-6 of the tensor's magnitude."""
    with torch.no_grad():
        model.fused = True
        model._drop_fused_cache()
        fused = [x.clone() for x in model.evaluate_at_t(t)[:4]]
        model.fused = False
        plain = [model.get_xyz_at_t(t), model.get_rotation_at_t(t), model.get_opacity_at_t(t), model.get_scaling()]
        model.fused = True
    for a, b, k in zip(fused, plain, ("xyz", "rotation", "opacity", "scaling")):
        assert a.shape == b.shape and torch.isfinite(b).all(), k
        assert float((a - b).abs().max()) <= 2e-6 * max(1.0, float(b.abs().max())), (k, t, float((a - b).abs().max()))


def test_grown_model_through_attribute_kernels_and_frame_trainer():
    """An all-static scene of duration 5: the first extraction gives K = 6 keyframes, an expansion 9.  After each, the fused
    evaluation equals the unfused getters at a timestamp in the first and in the last keyframe segment, and a FrameTrainer step with
    the regularisers on runs."""
    from ex4dgs_amd import densify, growth
    from ex4dgs_amd.scene import make_scene, upstream_grads
    from ex4dgs_amd.trainer import FrameTrainer
    model, cam, bg = make_scene("cfg1", P=2048, device=DEV, duration=5, fused=True)
    cam, bg = cam.to(DEV), bg.to(DEV)
    for k, shape in EMPTY.items():
        setattr(model, k, torch.zeros(shape, device=DEV))
    for p in model.PARAM_NAMES:
        setattr(model, p, torch.nn.Parameter(getattr(model, p)))
    stats = densify.DensityStats(model)
    stats.static[8].fill_(2.0)
    H, W = cam.image_height, cam.image_width

    def upstream(out):
        gc, gd, gf, ga = upstream_grads(out["acc"], H, W, device=DEV)
        return [out["render"], out["depth"], out["opticalflow"], out["acc"]], [gc, gd, gf, ga]
    out = growth.extract_dynamic_points(model, stats, None, cam.camera_center, 1.5, torch.ones(2048, dtype=torch.bool, device=DEV), 5.0, percentile=0.5)
    assert out["dynamic"]["rows"] == model.num_dynamic > 500 and model._xyz_motion.shape[1:] == (6, 3) and model.num_static + model.num_dynamic == 2048
    for t in (1.0, 20.0):                                        # keyframe segments 1 and K - 3 = 3
        _fused_equals_unfused(model, t)
    tr = FrameTrainer(model, optimizer=True, regularizers=(1e-3, 1e-3, 1e-3))
    tr.step(cam, bg, 1.0, upstream)
    tr.flush()
    assert tr.steps == 1 and all(torch.isfinite(p).all() for p in tr.params)
    assert growth.expand_duration(model, tr, 40) and model.duration == 41 and model._xyz_motion.shape[1:] == (9, 3)
    assert all(a is b for a, b in zip(tr.params, [getattr(model, n) for n in tr.names])) and not tr.m[tr.names.index("_xyz_motion")].any()
    growth.adjust_temp_opa(model, tr)
    for t in (1.0, 53.0):                                        # segments 1 and K' - 3 = 6
        _fused_equals_unfused(model, t)
    tr.step(cam, bg, 30.0, upstream)
    tr.flush()
    assert tr.steps == 2 and all(torch.isfinite(p).all() for p in tr.params)
