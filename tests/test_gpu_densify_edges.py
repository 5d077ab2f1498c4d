"""Adaptive density control beyond one workgroup (ex4dgs_amd/csrc/ex4d_densify.hip, ex4dgs_amd/densify.py) on the constructed
models of tests/densify_cases.py: every row class uniform over whole 256-row blocks (each packed per-block counter at 256), needles
at block edges, class changes at the boundaries of plan_scan_kernel's per-thread block ranges, 1 to 513 blocks.

The checker always runs on the CPU: counts and destination maps against expectations written down by construction, everything
that is copied / zeroed / reset bit for bit against the float32 restatement (tests/densify_ref.py; tests/test_cpu_densify_cases.py
pins it to those expectations), the five transformed tensors against the FLOAT64 restatement within the bar of
test_densify_at_one_million_against_restatement, gradient_accum within 2 n + 1 float32 ulps of the float64 value after n updates.
tests/test_cpu_densify_cases.py shows the float32 restatement itself within half of these bars on the same inputs.

What the case list found: max3() of plan_classify_kernel dropped a NaN scale unless it sat in the third column, where torch.max
propagates it from any column (class nan_scale: such a row was cloned / split instead of being left alone)."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from tests import densify_cases as dc
from tests import densify_ref as R
from tests import helpers as h
from tests.test_gpu_densify import hip_state, run_densify

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ERR_ARG = 1
PAYLOAD = 0x7FC0BEEF                     # a quiet NaN no computation produces: marks destination elements nobody wrote
MODES = {"invisible": 1, "small": 2, "nan": 3}

_WORST = dict(kind="densify_edges", tag="worst error / bar over tests/densify_cases.py (transformed tensors: float64 restatement, "
              "1e-6 |ref| + 1e-6 max(1, |ref|_inf); gradient_accum: 2 n + 1 ulp)", cases=0, gradient_accum=[0.0, 0.0, 0.0],
              **{k: 0.0 for k in dc.TRANSFORMED})
h.REPORT.append(_WORST)


# ------------------------------------------------------------------------------------------------------------------ helpers
def step_of(k):
    return float(3 + R.STATIC.index(k) if k in R.STATIC else 20 + R.DYNAMIC.index(k))


def hip_setup(state, opt_kind="fused"):
    """Model, statistics and optimizer on the device from a state dict of tests/densify_ref.py (as hip_setup of
    tests/test_gpu_densify.py builds them from the fixture).  opt_kind: "fused", "radam", "trainer" (a FrameTrainer whose moments are
    overwritten with the state's) or None."""
    from ex4dgs_amd import densify
    from ex4dgs_amd.optim import FusedRAdam
    from ex4dgs_amd.scene import DynamicGaussians
    params = {k: torch.nn.Parameter(v.to(DEV).contiguous()) for k, v in state["params"].items()}
    model = DynamicGaussians(params, duration=300, interval=10, time_pad=2)
    assert (model.interval, model.time_shift, model.duration) == (dc.MODEL["interval"], dc.MODEL["time_shift"], dc.MODEL["duration"])
    stats = densify.DensityStats(model)
    for names, blk in ((R.S_STATS, stats.static), (R.D_STATS, stats.dynamic)):
        for i, k in enumerate(names):
            blk[i].copy_(state["stats"][k].view(-1))
    if opt_kind is None:
        return model, stats, None
    if opt_kind == "trainer":
        from ex4dgs_amd.trainer import FrameTrainer
        opt = FrameTrainer(model, optimizer=True)
        for i, k in enumerate(opt.names):
            opt.m[i].copy_(state["m"][k])
            opt.v[i].copy_(state["v"][k])
        return model, stats, opt
    cls = FusedRAdam if opt_kind == "fused" else torch.optim.RAdam
    opt = cls([{"params": [getattr(model, k)], "lr": 1e-3} for k in model.PARAM_NAMES], lr=1e-3)
    for k in model.PARAM_NAMES:
        opt.state[getattr(model, k)] = {"step": torch.tensor(step_of(k)), "exp_avg": state["m"][k].to(DEV).clone(),
                                        "exp_avg_sq": state["v"][k].to(DEV).clone()}
    return model, stats, opt


def to_cpu(state):
    conv = lambda d: {k: v.detach().cpu().numpy() for k, v in d.items()}
    return {k: conv(state[k]) for k in ("params", "m", "v", "stats")}


def bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def assert_state(got, r32, r64, what, exact_transformed=False):
    """`got` (numpy, from the device) against the restatement: bit-exact (NaN-aware) against float32 for everything but the five
    transformed tensors, those within the bar against float64.  Returns {tensor: error / bar}."""
    ratios = {}
    for k, x in got["params"].items():
        ref = r32["params"][k].numpy()
        assert x.shape == ref.shape, (what, k, x.shape, ref.shape)
        if k in dc.TRANSFORMED and not exact_transformed:
            ratios[k] = dc.transformed_error_over_bar(x, r64["params"][k].numpy())
            print(f"{what}: {k} error / bar {ratios[k]:.4f}")
            assert ratios[k] <= 1.0, (what, k, ratios[k])
        else:
            dc.assert_same(x, ref, f"{what}: {k}")
    for mk in ("m", "v"):
        assert set(got[mk]) == set(r32[mk]), (what, mk)
        for k, x in got[mk].items():
            dc.assert_same(x, r32[mk][k].numpy(), f"{what}: {mk} {k}")
    for k, x in got["stats"].items():
        dc.assert_same(x, r32["stats"][k].numpy(), f"{what}: {k}")
    for k, v in ratios.items():
        _WORST[k] = max(_WORST[k], v)
    return ratios


def assert_rekeyed(model, opt, what):
    """The optimizer's groups and state hold the model's NEW parameter objects, `step` as before the call."""
    new = [getattr(model, k) for k in model.PARAM_NAMES]
    assert len(opt.param_groups) == len(new) and all(g["params"][0] is p for g, p in zip(opt.param_groups, new)), what
    assert len(opt.state) == len(new) and all(p in opt.state for p in new), what
    for k, p in zip(model.PARAM_NAMES, new):
        st = opt.state[p]
        assert float(st["step"]) == step_of(k), (what, k)
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape, (what, k)


@functools.lru_cache(maxsize=2)
def case_data(name):
    """(state, draws, counts, maps, float32 restatement, float64 restatement) of a densify case, all on the CPU."""
    c = dc.case_by_name(name)
    sc, dy = dc.layout(c.config, c.static), dc.layout(c.config, c.dynamic)
    pre = dc.make_state(sc, dy, c.seed, config=c.config)
    counts = dc.expected_counts(sc, c.config), dc.expected_counts(dy, c.config)
    maps = dc.expected_map(sc, c.config), dc.expected_map(dy, c.config)
    draws = dc.make_draws(counts[0], counts[1], c.seed)
    return pre, draws, counts, maps, dc.run_restatement(pre, c.config, draws), dc.run_restatement(pre, c.config, draws, torch.float64)


def thresholds(config):
    """The threshold fields of Ex4dDensifyPlanGroup as densify_and_prune fills them (both groups: the configurations use the same
    numbers for static and dynamic rows)."""
    cfg = dc.CONFIGS[config]
    return dict(dense_scale=dc.f32(cfg["percent_dense"] * cfg["extent"]), big_scale=dc.f32(0.1 * cfg["extent"]), grad_thr=dc.f32(cfg["max_grad"]),
                use_screen=int(bool(cfg["max_screen_size"])), screen_size=dc.f32(cfg["max_screen_size"] or 0), min_opacity=dc.f32(cfg["min_opacity"]),
                l1_thres=dc.f32(cfg["s_l1_thres"]), max_ssim=dc.f32(cfg["s_max_ssim"]))


def assert_plan(mp, counts, flags, what):
    want_c, want_m = dc.counts_of_flags(flags), dc.map_of_flags(flags)
    got_c, got_m = counts.cpu().numpy(), mp.cpu().numpy()[: len(flags)]
    assert got_c.tolist() == want_c.tolist(), (what, "counts", dict(zip(dc.COUNTERS + ("ROWS",), zip(got_c.tolist(), want_c.tolist()))))
    bad = np.nonzero((got_m != want_m).any(axis=1))[0]
    assert bad.size == 0, (what, f"map differs in {bad.size} rows, first at row {bad[0]} (block {bad[0] // dc.BLOCK}, lane {bad[0] % dc.BLOCK})",
                           got_m[bad[0]].tolist(), want_m[bad[0]].tolist())


def all_layout_specs(config):
    out = list(dc.layout_specs(config))
    for c in dc.cases():
        if c.config == config:
            out += [s for s in (c.static, c.dynamic) if s is not None and s not in out]
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. the plan alone
@pytest.mark.parametrize("config", ["A", "B"])
def test_plan_counts_and_map_are_exact_on_every_layout(hip_lib, config):
    from ex4dgs_amd import densify
    thr = thresholds(config)
    for k, spec in enumerate(all_layout_specs(config)):
        classes = dc.layout(config, spec)
        block, scaling, logit = dc.make_plan_inputs(config, classes, 500 + k)
        dev = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (block, scaling, logit)]
        plan = densify._plan(densify.PLAN_DENSIFY, dev[0], len(classes), DEV, dev[1], dev[2], thr=thr)
        assert_plan(plan[0], plan[1], dc.class_flags(config, classes), (config, spec))


def test_prune_plans_are_exact_on_every_layout(hip_lib):
    from ex4dgs_amd import densify
    for k, spec in enumerate(dc.prune_layout_specs()):
        classes = dc.layout("P", spec)
        flags = dc.class_flags("P", classes)
        for kind in dc.PRUNE_KINDS:
            for dynamic in (False, True):
                if dynamic and len(classes) > 65537:
                    continue
                st = dc.make_prune_state(kind, [] if dynamic else classes, classes if dynamic else [], 700 + k, moments=False)
                names, xyz = (R.D_STATS, "_xyz_motion") if dynamic else (R.S_STATS, "_xyz")
                block = torch.stack([st["stats"][n].view(-1) for n in names]).to(DEV).contiguous()
                x = st["params"][xyz].to(DEV).contiguous()
                plan = densify._plan(MODES[kind], block, len(classes), DEV, xyz=x)
                assert x[0].numel() == (105 if dynamic else 3)
                assert_plan(plan[0], plan[1], flags, (kind, "dynamic" if dynamic else "static", spec))


# --------------------------------------------------------------------------------------------------------------- 2. the whole call
@pytest.mark.parametrize("name", [c.name for c in dc.cases()])
def test_densify_and_prune_on_constructed_case(hip_lib, name):
    c = dc.case_by_name(name)
    pre, draws, counts, maps, r32, r64 = case_data(name)
    results = []
    for opt_kind in ("fused", "radam"):
        model, stats, opt = hip_setup(pre, opt_kind)
        out = run_densify(model, stats, opt, dc.CONFIGS[c.config], noise=draws)
        for gi, key in enumerate(("static", "dynamic")):
            assert [out[key][n] for n in ("keep", "clone", "keep_clone", "split", "split_clone", "keep_child", "keep_child_clone", "rows")] == \
                counts[gi].tolist(), (name, opt_kind, key, out[key])
        got = to_cpu(hip_state(model, stats, opt))
        assert_state(got, r32, r64, f"{name} [{opt_kind}]")
        assert_rekeyed(model, opt, (name, opt_kind))
        results.append(got)
    # no atomics in these kernels: the two runs (same inputs, same draws) agree in every bit
    for grp in ("params", "m", "v", "stats"):
        for k in results[0][grp]:
            assert same_bits(results[0][grp][k], results[1][grp][k]), (name, grp, k)
    _WORST["cases"] += 1


@pytest.mark.parametrize("name", [c.name for c in dc.prune_cases()])
def test_prunes_on_constructed_case(hip_lib, name):
    from ex4dgs_amd import densify
    c = dc.case_by_name(name)
    sc, dy = dc.layout("P", c.static), dc.layout("P", c.dynamic)
    want = dc.expected_counts(sc, "P"), dc.expected_counts(dy, "P")
    for kind, fn in (("invisible", densify.prune_invisible), ("small", densify.prune_small), ("nan", densify.prune_nan_points)):
        pre = dc.make_prune_state(kind, sc, dy, c.seed)
        ref = dc.clone_state(pre)
        R.prune(ref, kind)
        for opt_kind in ("fused", "radam"):
            model, stats, opt = hip_setup(pre, opt_kind)
            out = fn(model, stats, opt)
            assert (out["static"]["keep"], out["static"]["rows"]) == (want[0][0], want[0][7]), (name, kind)
            assert (out["dynamic"]["keep"], out["dynamic"]["rows"]) == (want[1][0], want[1][7]), (name, kind)
            assert_state(to_cpu(hip_state(model, stats, opt)), ref, None, f"{name} {kind} [{opt_kind}]", exact_transformed=True)
            assert_rekeyed(model, opt, (name, kind, opt_kind))


# -------------------------------------------------------------------------------------------------- 3. the FrameTrainer adapter
@pytest.mark.parametrize("config", ["A", "B"])
def test_frame_trainer_moments_follow_their_rows(hip_lib, config):
    name = dc.MIXED[config]
    pre, draws, counts, maps, r32, r64 = case_data(name)
    model, stats, opt = hip_setup(pre, "fused")
    run_densify(model, stats, opt, dc.CONFIGS[config], noise=draws)
    want = to_cpu(hip_state(model, stats, opt))
    assert_state(want, r32, r64, f"{name} [fused]")
    model, stats, tr = hip_setup(pre, "trainer")
    tr.steps = 5
    before = list(tr.params)
    run_densify(model, stats, tr, dc.CONFIGS[config], noise=draws)
    assert tr.steps == 5 and tr._grads is None
    for i, k in enumerate(tr.names):
        assert tr.params[i] is getattr(model, k) and tr.params[i] is not before[i], k
        assert tr.params[i].shape[0] == counts[0 if k in R.STATIC else 1][dc.ROWS], k
        for what, x, ref in (("param", tr.params[i], want["params"][k]), ("m", tr.m[i], want["m"][k]), ("v", tr.v[i], want["v"][k])):
            assert same_bits(x.detach().cpu().numpy(), ref), (name, what, k)
        if tr.pgrad[i] is not None:                                    # gradient buffers rebuilt for the new row counts
            assert tr.pgrad[i].shape[0] == tr.params[i].shape[0] and tr.pgrad[i].device == tr.params[i].device, k
    for k in R.S_STATS + R.D_STATS:
        assert same_bits(getattr(stats, k).cpu().numpy(), want["stats"][k]), k


# --------------------------------------------------------------------------------- 4. every destination element written, nothing else
def _guarded(rows, tail_shape, extra_rows=1):
    """A destination of `rows` rows with `extra_rows` guard rows behind it, every element the recognisable NaN."""
    width = int(np.prod(tail_shape)) if tail_shape else 1
    base = torch.full(((rows + extra_rows) * width,), PAYLOAD, dtype=torch.int32, device=DEV)
    return base, base.view(torch.float32)[: rows * width].view((rows,) + tuple(tail_shape))


@pytest.mark.parametrize("config", ["A", "B"])
def test_prefilled_destinations_are_fully_written_and_nothing_else(hip_lib, config):
    from ex4dgs_amd import densify as D
    name = dc.MIXED[config]
    pre, draws, want_counts, maps, r32, r64 = case_data(name)
    model, stats, opt = hip_setup(pre, "fused")
    run_densify(model, stats, opt, dc.CONFIGS[config], noise=draws)
    want = to_cpu(hip_state(model, stats, opt))
    assert_state(want, r32, r64, f"{name} [fused]")

    model, stats, opt = hip_setup(pre, "fused")
    thr = thresholds(config)
    ns, nd = model.num_static, model.num_dynamic
    plans = [D._plan(D.PLAN_DENSIFY, stats.static, ns, DEV, model._scaling.detach(), model._opacity.detach(), thr=thr),
             D._plan(D.PLAN_DENSIFY, stats.dynamic, nd, DEV, model._scaling_motion.detach(), model._opacity_motion.detach(), thr=thr)]
    counts = torch.stack([plans[0][1], plans[1][1]]).cpu().tolist()
    assert counts == [want_counts[0].tolist(), want_counts[1].tolist()]                # the gather below runs on verified counts only
    on_dev = D._draws(counts, True, DEV, None, draws)
    groups = D._groups(plans, counts, [{"split_z": on_dev["static_split_z"]},
                                       {k: on_dev[k] for k in ("split_z", "split_c1", "split_c0", "clone_c1", "clone_c0")}], model)
    rules = {"_xyz": (D.RULE_CHILD_XYZ, model._rotation.detach(), model._scaling.detach(), 1.0),
             "_scaling": (D.RULE_CHILD_SCALING, None, None, 0.0),
             "_xyz_motion": (D.RULE_CHILD_XYZ, model._rotation_motion.detach(), model._scaling_motion.detach(), 2.0),
             "_scaling_motion": (D.RULE_CHILD_SCALING, None, None, 0.0),
             "_opacity_duration_center": (D.RULE_CENTER, None, None, 0.0),
             "_opacity_duration_var": (D.RULE_CONST_NEW, None, None, 2.0)}
    descs, outs = [], []                                                             # outs: (what, key, base, view)
    for gi, names in enumerate((R.STATIC, R.DYNAMIC)):
        rows_src, rows_dst = (ns, nd)[gi], counts[gi][7]
        for k in names:
            src = getattr(model, k).detach()
            base, dst = _guarded(rows_dst, src.shape[1:])
            rule, aux0, aux1, value = rules.get(k, (D.RULE_COPY, None, None, 0.0))
            descs.append(D._desc(src, dst, rows_src, rows_dst, rule, gi, 1, aux0, aux1, value))
            outs.append(("params", k, base, dst))
            for mk, key in (("m", "exp_avg"), ("v", "exp_avg_sq")):
                mom = opt.state[getattr(model, k)][key]
                base, dst = _guarded(rows_dst, src.shape[1:])
                descs.append(D._desc(mom, dst, rows_src, rows_dst, D.RULE_ZERO_NEW, gi))
                outs.append((mk, k, base, dst))
        blk = (stats.static, stats.dynamic)[gi]
        base, dst = _guarded(9 * rows_dst, (), extra_rows=16)
        descs.append(D._desc(blk, dst, rows_src, rows_dst, D.RULE_STATS, gi, planes=9))
        outs.append(("block", gi, base, dst.view(9, rows_dst)))
    assert len(descs) == 47 > D.MAX_TENSORS                                          # two ex4d_densify_apply batches
    D._apply(descs, groups, DEV)
    torch.cuda.synchronize()
    for what, k, base, dst in outs:
        inside = dst.contiguous().view(torch.int32)
        assert int((inside == PAYLOAD).sum()) == 0, f"{what} {k}: destination elements never written"
        guard = base[dst.numel():]
        assert guard.numel() > 0 and bool((guard == PAYLOAD).all()), f"{what} {k}: written behind the last destination row"
        x = dst.cpu().numpy()
        if what == "block":
            names = (R.S_STATS, R.D_STATS)[k]
            for i, n in enumerate(names):
                assert same_bits(x[i], want["stats"][n].reshape(-1)), n
        else:
            assert same_bits(x, want[what][k]), (what, k)
    del on_dev, plans


# ---------------------------------------------------------------------------------------------------------------- 5. the statistics
STAT_SHAPES = ((1, 0), (255, 257), (256, 256), (257, 1), (65537, 300))
FLAG_COMBOS = [dict(densify_stats=a, prune_stats=b, l1_accum=c, egrad=True) for a in (True, False) for b in (True, False) for c in (True, False)] + \
              [dict(densify_stats=True, prune_stats=True, l1_accum=True, egrad=False)]


def _block_of(st, names):
    return torch.stack([st[k].view(-1) for k in names]) if st[names[0]].shape[0] else torch.zeros(9, 0)


@pytest.mark.parametrize("ns,nd", STAT_SHAPES)
def test_update_flag_combinations_and_untouched_rows(hip_lib, ns, nd):
    from ex4dgs_amd import densify
    frames = dc.make_frames(ns, nd, ns + 3 * nd)
    for start in ("prefilled", "fresh"):
        for combo in FLAG_COMBOS if start == "prefilled" else FLAG_COMBOS[:1] + FLAG_COMBOS[-1:]:
            st32 = dc.make_stats_prefill(ns, nd, ns + nd) if start == "prefilled" else R.init_stats(ns, nd)
            st64 = {k: v.double() for k, v in st32.items()}
            first = {k: v.clone() for k, v in st32.items()}
            stats = densify.DensityStats(types.SimpleNamespace(num_static=ns, num_dynamic=nd), device=DEV)
            stats.static.copy_(_block_of(st32, R.S_STATS))
            stats.dynamic.copy_(_block_of(st32, R.D_STATS))
            kw = {k: combo[k] for k in ("densify_stats", "prune_stats", "l1_accum")}
            for j, (radii, vg, eg, ts) in enumerate(frames):
                eg_ = eg if combo["egrad"] else None
                stats.update(radii.to(DEV), vg.to(DEV), eg_.to(DEV) if eg_ is not None else None, ts, **kw)
                R.update(st32, radii, vg, eg_, ts, **kw)
                R.update(st64, radii, vg.double(), eg_.double() if eg_ is not None else None, ts, **kw)
                for k in R.S_STATS + R.D_STATS:
                    x = getattr(stats, k).cpu().numpy()
                    if "gradient_accum" in k:
                        e = dc.grad_accum_error_over_bar(x, st64[k].numpy(), j + 1)
                        print(f"({ns}, {nd}) {start} {combo} frame {j}: {k} error / bar {e:.4f}")
                        assert e <= 1.0, (ns, nd, start, combo, j, k, e)
                        _WORST["gradient_accum"][j] = max(_WORST["gradient_accum"][j], e)
                    else:
                        dc.assert_same(x, st32[k].numpy(), f"({ns}, {nd}) {start} {combo} frame {j}: {k}")
            # a flag that is off leaves its rows of the [9, N] block exactly as they were
            grad_on = combo["densify_stats"]
            l1_on = grad_on and combo["l1_accum"] and combo["egrad"]
            prune_on = combo["prune_stats"] and combo["l1_accum"] and combo["egrad"]
            untouched = ([] if grad_on else [0, 1, 5]) + ([] if l1_on else [2, 3, 4, 7, 8]) + ([] if prune_on else [6])
            for names in (R.S_STATS, R.D_STATS):
                for i in untouched:
                    assert same_bits(getattr(stats, names[i]).cpu().numpy(), first[names[i]].numpy()), (ns, nd, combo, names[i])


# ------------------------------------------------------------------------------------------------------------------- 6. refusals
def _refused(lib, rc, outputs, what):
    assert rc == ERR_ARG, (what, rc)
    assert lib.ex4d_densify_last_error().decode() != "", what
    torch.cuda.synchronize()
    for name, t, fill in outputs:
        assert bool((t.view(torch.int32) == fill).all()), (what, f"{name} was written")


def test_plan_refuses_bad_arguments_without_writing(hip_lib):
    from ex4dgs_amd import _C, densify as D
    lib = _C.load()
    n, fill = 8, -7
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    f = lambda *s: torch.zeros(*s, device=DEV)
    stats, scaling, opacity, xyz = f(9, n), f(n, 3), f(n), f(n, 3)
    mp = torch.full((n, 8), fill, dtype=torch.int32, device=DEV)
    counts = torch.full((8,), fill, dtype=torch.int32, device=DEV)
    scratch = torch.zeros(max(int(lib.ex4d_densify_scratch_bytes(n)), 1), dtype=torch.uint8, device=DEV)
    outputs = [("map", mp, fill), ("counts", counts, fill)]

    def group(**over):
        g = D.Ex4dDensifyPlanGroup()
        g.n, g.stats, g.scaling, g.opacity, g.xyz, g.xyz_width = n, stats.data_ptr(), scaling.data_ptr(), opacity.data_ptr(), xyz.data_ptr(), 3
        g.map, g.counts, g.scratch = mp.data_ptr(), counts.data_ptr(), scratch.data_ptr()
        for k, v in over.items():
            setattr(g, k, v)
        return g
    for what, mode, g in (("unknown mode 4", 4, group()), ("unknown mode -1", -1, group()), ("n < 0", D.PLAN_DENSIFY, group(n=-1)),
                          ("n = 2^31 - 1", D.PLAN_DENSIFY, group(n=2 ** 31 - 1)), ("no scaling", D.PLAN_DENSIFY, group(scaling=None)),
                          ("no opacity", D.PLAN_DENSIFY, group(opacity=None)), ("xyz_width 0", D.PLAN_PRUNE_NAN, group(xyz_width=0)),
                          ("no xyz", D.PLAN_PRUNE_NAN, group(xyz=None))):
        _refused(lib, lib.ex4d_densify_plan(mode, C.byref(g), stream), outputs, what)
    _refused(lib, lib.ex4d_densify_plan(D.PLAN_DENSIFY, None, stream), outputs, "null group")


def test_apply_refuses_bad_descriptors_without_writing(hip_lib):
    from ex4dgs_amd import _C, densify as D
    lib = _C.load()
    n = 8
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    mp = torch.full((n, 8), -1, dtype=torch.int32, device=DEV)
    mp[:, 0] = torch.arange(n, dtype=torch.int32, device=DEV)                       # a valid map: every row kept in place
    z = torch.zeros(64, device=DEV)
    g = D.Ex4dDensifyApplyGroup()
    g.map, g.child_stride, g.n_split = mp.data_ptr(), 0, 0
    for k in ("split_z", "split_c1", "split_c0", "clone_c1", "clone_c0"):
        setattr(g, k, z.data_ptr())
    g.min_len, g.center_lo, g.center_hi, g.split_div = 0.2, 1.3, 31.1, 1.6
    garr = (D.Ex4dDensifyApplyGroup * 2)(g, g)
    src = torch.ones(n * 9 * 4, device=DEV)
    base, dst = _guarded(n * 9 * 4, ())
    aux = torch.ones(n * 4 * 4, device=DEV)
    outputs = [("dst", base, PAYLOAD)]

    def desc(width=3, planes=1, rule=D.RULE_COPY, group=0):
        return D.Ex4dDensifyTensor(src.data_ptr(), dst.data_ptr(), n, n, width, planes, rule, group, aux.data_ptr(), aux.data_ptr(), 0.0, 0)
    cases = (("count 25", [desc()] * 25), ("CHILD_XYZ with width 4", [desc(width=4, rule=D.RULE_CHILD_XYZ)]),
             ("planes 9 with ZERO_NEW", [desc(width=1, planes=9, rule=D.RULE_ZERO_NEW)]),
             ("planes 9 with CONST_NEW", [desc(width=1, planes=9, rule=D.RULE_CONST_NEW)]),
             ("planes 9 with width 3", [desc(width=3, planes=9)]), ("STATS with planes 1", [desc(width=1, rule=D.RULE_STATS)]),
             ("CENTER with width 3", [desc(width=3, rule=D.RULE_CENTER)]), ("group 2", [desc(group=2)]), ("group -1", [desc(group=-1)]),
             ("unknown rule 7", [desc(rule=7)]), ("a good descriptor, then a bad one", [desc(), desc(group=2)]))
    for what, ds in cases:
        arr = (D.Ex4dDensifyTensor * len(ds))(*ds)
        _refused(lib, lib.ex4d_densify_apply(arr, len(ds), garr, stream), outputs, what)
    _refused(lib, lib.ex4d_densify_apply(None, 1, garr, stream), outputs, "null descriptors")
