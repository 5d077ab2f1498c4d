"""Adaptive density control on the GPU (ex4dgs_amd.densify, include/ex4d_densify.h): the HIP statistics, densify_and_prune and the
three prunes against the reference's outputs (tests/golden/densify.npz) and, at config-3 scale, against the torch restatement
(tests/densify_ref.py) with identical draws; the optimizer adapters; edge cases; graph capture of the per-iteration update."""
import json

import numpy as np
import pytest
import torch

from tests import densify_ref as R
from tests.test_cpu_densify import GOLD, MODEL, assert_state, draws_of, state_from

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def hip_setup(case, tag="pre", opt_kind="radam"):
    from ex4dgs_amd import densify
    from ex4dgs_amd.optim import FusedRAdam
    from ex4dgs_amd.scene import DynamicGaussians
    st = state_from(case, tag, DEV)
    params = {k: torch.nn.Parameter(v.contiguous()) for k, v in st["params"].items()}
    model = DynamicGaussians(params, duration=300, interval=10, time_pad=2)
    stats = densify.DensityStats(model)
    for names, blk in ((R.S_STATS, stats.static), (R.D_STATS, stats.dynamic)):
        for i, k in enumerate(names):
            blk[i].copy_(st["stats"][k].view(-1))
    cls = FusedRAdam if opt_kind == "fused" else torch.optim.RAdam
    opt = cls([{"params": [getattr(model, k)], "lr": 1e-3} for k in model.PARAM_NAMES], lr=1e-3)
    for k in model.PARAM_NAMES:
        if k in st["m"]:
            p = getattr(model, k)
            opt.state[p] = {"step": torch.tensor(float(GOLD[f"{case}/{tag}/step/{k}"])), "exp_avg": st["m"][k].clone(), "exp_avg_sq": st["v"][k].clone()}
    return model, stats, opt


def hip_state(model, stats, opt):
    out = {"params": {k: getattr(model, k).detach() for k in R.STATIC + R.DYNAMIC}, "m": {}, "v": {}, "stats": {}}
    for k in out["params"]:
        s = opt.state.get(getattr(model, k)) if opt is not None else None
        if s:
            out["m"][k], out["v"][k] = s["exp_avg"], s["exp_avg_sq"]
    for k in R.S_STATS + R.D_STATS:
        out["stats"][k] = getattr(stats, k)
    return out


def run_densify(model, stats, opt, cfg, noise=None, generator=None):
    from ex4dgs_amd import densify
    return densify.densify_and_prune(model, stats, opt, cfg["max_grad"], cfg["max_dgrad"], cfg["min_opacity"], cfg["min_motion_opacity"], cfg["extent"],
                                     cfg["max_screen_size"], cfg["max_dynamic_screen_size"], s_max_ssim=cfg["s_max_ssim"], s_l1_thres=cfg["s_l1_thres"],
                                     d_max_ssim=cfg["d_max_ssim"], d_l1_thres=cfg["d_l1_thres"], percent_dense=cfg["percent_dense"], noise=noise,
                                     generator=generator)


def test_update_matches_reference_statistics():
    from ex4dgs_amd import densify
    from ex4dgs_amd.scene import DynamicGaussians
    for case in ("default", "screen", "staticonly"):
        st = state_from(case, "pre", DEV)
        model = DynamicGaussians(st["params"], duration=300, interval=10, time_pad=2)
        stats = densify.DensityStats(model)
        for j in range(2):
            a = lambda k: torch.from_numpy(GOLD[f"{case}/A{j}/{k}"].copy()).to(DEV).contiguous()
            stats.update(a("radii"), a("vgrad"), a("egrad"), float(GOLD[f"{case}/A{j}/timestamp"]))
            for k in R.S_STATS + R.D_STATS:
                x, g = getattr(stats, k).cpu().numpy(), GOLD[f"{case}/A{j}/stats/{k}"]
                if "gradient_accum" in k:                      # |grad[:, :2]|: sqrt of a sum of two squares, within 2 ulp
                    np.testing.assert_array_max_ulp(x, g, maxulp=2)
                else:
                    np.testing.assert_array_equal(x, g, err_msg=k)


@pytest.mark.parametrize("opt_kind", ["radam", "fused"])
def test_densify_and_prunes_match_reference(opt_kind):
    from ex4dgs_amd import densify
    for case in ("default", "screen", "staticonly"):
        cfg = json.loads(str(GOLD[f"{case}/cfg"]))
        model, stats, opt = hip_setup(case, opt_kind=opt_kind)
        out = run_densify(model, stats, opt, cfg, noise=draws_of(case, DEV))
        assert out["static"]["rows"] == GOLD[f"{case}/post/param/_xyz"].shape[0]
        assert_state(hip_state(model, stats, opt), case)
        for k in model.PARAM_NAMES:                        # step kept, state re-keyed to the new parameter objects
            if f"{case}/post/step/{k}" in GOLD.files:
                assert float(opt.state[getattr(model, k)]["step"]) == float(GOLD[f"{case}/post/step/{k}"])
        if case == "screen":
            assert out["static"]["split_clone"] > 0 or out["dynamic"]["split_clone"] > 0
    for case, fn in (("invisible", densify.prune_invisible), ("small", densify.prune_small), ("nan", densify.prune_nan_points)):
        model, stats, opt = hip_setup(case, opt_kind=opt_kind)
        fn(model, stats, opt)
        assert_state(hip_state(model, stats, opt), case, exact_transformed=True)


def _random_stats(model, stats, g):
    ns, nd = model.num_static, model.num_dynamic
    for blk, n in ((stats.static, ns), (stats.dynamic, nd)):
        den = torch.randint(0, 6, (n,), generator=g).float()
        blk[1].copy_(den)
        blk[0].copy_(den * torch.rand(n, generator=g) * 4e-4)
        blk[5].copy_(torch.randint(0, 40, (n,), generator=g).float())
        blk[6].copy_(torch.randint(0, 12, (n,), generator=g).float())
        blk[8].copy_(torch.randint(-1, 2, (n,), generator=g).float())


def test_densify_at_one_million_against_restatement():
    from ex4dgs_amd import densify
    from ex4dgs_amd.scene import make_scene
    model, _, _ = make_scene("cfg3", device=DEV)
    stats = densify.DensityStats(model)
    _random_stats(model, stats, torch.Generator().manual_seed(5))
    ref = {"params": {k: getattr(model, k).clone() for k in R.STATIC + R.DYNAMIC}, "m": None, "v": None,
           "stats": {k: getattr(stats, k).clone() for k in R.S_STATS + R.D_STATS}}
    cfg = dict(max_grad=0.0002, max_dgrad=0.0002, min_opacity=0.01, min_motion_opacity=0.01, extent=5.0, max_screen_size=20,
               max_dynamic_screen_size=20, s_max_ssim=0.5, s_l1_thres=0.1, d_max_ssim=0.5, d_l1_thres=0.1, percent_dense=0.01)
    out = run_densify(model, stats, None, cfg, generator=torch.Generator(device=DEV).manual_seed(3))
    R.densify_and_prune(ref, MODEL, cfg["max_grad"], cfg["max_dgrad"], cfg["min_opacity"], cfg["min_motion_opacity"], cfg["extent"], 20, 20,
                        out["draws"], percent_dense=0.01)
    assert out["static"]["clone"] > 1000 and out["static"]["split"] > 1000
    for k, x in ref["params"].items():
        y = getattr(model, k).detach()
        assert y.shape == x.shape, (k, y.shape, x.shape)
        if k in ("_xyz", "_scaling", "_xyz_motion", "_scaling_motion", "_opacity_duration_center"):
            # 1e-6 relative to the tensor's magnitude: a child position is x + R (sigma z), whose two terms may cancel
            torch.testing.assert_close(y, x, rtol=1e-6, atol=1e-6 * max(1.0, x.abs().max().item()))
        else:
            assert torch.equal(y, x), k
    for k, x in ref["stats"].items():
        assert torch.equal(getattr(stats, k), x), k


def test_fused_radam_step_after_densify_equals_torch_radam():
    from ex4dgs_amd import densify
    cfg = json.loads(str(GOLD["default/cfg"]))
    runs = []
    for kind in ("fused", "radam"):
        model, stats, opt = hip_setup("default", opt_kind=kind)
        run_densify(model, stats, opt, cfg, noise=draws_of("default", DEV))
        g = torch.Generator(device=DEV).manual_seed(1)
        for k in model.PARAM_NAMES:
            p = getattr(model, k)
            p.grad = torch.randn(p.shape, device=DEV, generator=g)
        opt.step()
        runs.append([getattr(model, k).detach().clone() for k in model.PARAM_NAMES])
    for a, b in zip(*runs):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


def test_frame_trainer_densify_between_steps():
    from ex4dgs_amd import densify
    from ex4dgs_amd.scene import make_scene, upstream_grads
    from ex4dgs_amd.trainer import FrameTrainer
    model, cam, bg = make_scene("cfg2", P=20000, device=DEV)
    P0 = model.num_static + model.num_dynamic
    tr = FrameTrainer(model, optimizer=True)
    stats = densify.DensityStats(model)
    H, W = cam.image_height, cam.image_width

    def upstream(out):
        gc, gd, gf, ga = upstream_grads(out["acc"], H, W, device=DEV)
        return [out["render"], out["depth"], out["opticalflow"], out["acc"]], [gc, gd, gf, ga]
    for i in range(5):
        out = tr.step(cam, bg, i, upstream)
        stats.update(out["radii"].int().contiguous(), out["viewspace_points"].grad, out["viewspace_l1points"].grad, i)
    steps_before = tr.steps
    before = [p.clone() for p in tr.params]
    res = densify.densify_and_prune(model, stats, tr, 1e-6, 1e-6, 0.01, 0.01, 5.0, generator=torch.Generator(device=DEV).manual_seed(0))
    assert tr.steps == steps_before and tr._grads is None          # the pending update was dropped, not applied
    P1 = model.num_static + model.num_dynamic
    assert P1 != P0 and P1 == res["static"]["rows"] + res["dynamic"]["rows"]
    keep = [getattr(model, n) for n in tr.names]
    assert all(a is b for a, b in zip(keep, tr.params))
    stats2 = stats
    for i in range(5):
        out = tr.step(cam, bg, 10 + i, upstream)
        stats2.update(out["radii"].int().contiguous(), out["viewspace_points"].grad, out["viewspace_l1points"].grad, 10 + i)
    tr.flush()
    assert tr.steps == steps_before + 5 and all(torch.isfinite(p).all() for p in tr.params)
    del before
    with pytest.raises(NotImplementedError):
        FrameTrainer(model, optimizer=True, views_per_step=2, sliced=False).begin_density_control()


def test_edge_cases_nothing_selected_everything_pruned_static_only():
    from ex4dgs_amd import densify
    cfg = json.loads(str(GOLD["default/cfg"]))
    # nothing selected: thresholds out of reach, nothing pruned -> the same rows, statistics reset, moments kept
    model, stats, opt = hip_setup("default")
    before = {k: getattr(model, k).detach().clone() for k in model.PARAM_NAMES}
    out = run_densify(model, stats, opt, dict(cfg, max_grad=1e9, max_dgrad=1e9, min_opacity=0.0, min_motion_opacity=0.0, extent=1e9))
    assert out["static"]["rows"] == before["_xyz"].shape[0] and out["dynamic"]["rows"] == before["_xyz_motion"].shape[0]
    for k, v in before.items():
        assert torch.equal(getattr(model, k).detach(), v), k
    assert (stats.denom == 0).all() and (stats.min_radii2D == 1000).all()
    # everything pruned in the dynamic group
    model, stats, opt = hip_setup("default")
    out = run_densify(model, stats, opt, dict(cfg, min_motion_opacity=2.0))
    assert out["dynamic"]["rows"] == 0 and model._xyz_motion.shape[0] == 0 and stats.dynamic.shape == (9, 0)
    assert opt.state[model._xyz_motion]["exp_avg"].shape[0] == 0
    # Nd == 0: the dynamic half untouched
    model, stats, opt = hip_setup("staticonly")
    dyn = model._xyz_motion
    run_densify(model, stats, opt, cfg, noise=draws_of("staticonly", DEV))
    assert model._xyz_motion is dyn


def test_update_captured_in_a_graph():
    from ex4dgs_amd import densify
    from ex4dgs_amd.scene import DynamicGaussians
    st = state_from("default", "pre", DEV)
    model = DynamicGaussians(st["params"], duration=300, interval=10, time_pad=2)
    a = lambda k: torch.from_numpy(GOLD[f"default/A0/{k}"].copy()).to(DEV).contiguous()
    radii, vg, eg = a("radii"), a("vgrad"), a("egrad")
    eager, graphed = densify.DensityStats(model), densify.DensityStats(model)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        graphed.update(radii, vg, eg, 7.0)                    # warm-up outside the capture (library load)
    torch.cuda.current_stream().wait_stream(s)
    graphed.static.copy_(eager.static); graphed.dynamic.copy_(eager.dynamic)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.update(radii, vg, eg, 7.0)
    for _ in range(3):
        g.replay()
        eager.update(radii, vg, eg, 7.0)
    torch.cuda.synchronize()
    assert torch.equal(graphed.static, eager.static) and torch.equal(graphed.dynamic, eager.dynamic)
