"""Adaptive density control without a GPU: the torch restatement (tests/densify_ref.py) against the reference's own outputs
(tests/golden/densify.npz, tests/golden/make_golden_densify.py), and the host-side prune schedule (the C ABI's exports and
structure sizes: tests/test_cpu_abi.py)."""
import json
import os

import numpy as np
import torch

from tests import densify_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "densify.npz"))
MODEL = {"interval": 10, "time_shift": 12, "duration": 300}
TRANSFORMED = ("_xyz", "_scaling", "_xyz_motion", "_scaling_motion", "_opacity_duration_center")


def state_from(case, tag, device="cpu"):
    t = lambda k: torch.from_numpy(GOLD[k].copy()).to(device)
    params = {k: t(f"{case}/{tag}/param/{k}") for k in R.STATIC + R.DYNAMIC}
    m = {k: t(f"{case}/{tag}/m/{k}") for k in params if f"{case}/{tag}/m/{k}" in GOLD.files}
    v = {k: t(f"{case}/{tag}/v/{k}") for k in params if f"{case}/{tag}/v/{k}" in GOLD.files}
    stats = {k: t(f"{case}/{tag}/stats/{k}") for k in R.S_STATS + R.D_STATS}
    return {"params": params, "m": m, "v": v, "stats": stats}


def draws_of(case, device="cpu"):
    return {k.split("/")[-1]: torch.from_numpy(GOLD[k].copy()).to(device) for k in GOLD.files if k.startswith(f"{case}/draw/")}


def assert_state(state, case, tag="post", exact_transformed=False):
    for k, x in state["params"].items():
        g = GOLD[f"{case}/{tag}/param/{k}"]
        assert x.shape == g.shape, (k, x.shape, g.shape)
        if k in TRANSFORMED and not exact_transformed:
            np.testing.assert_allclose(x.cpu().numpy(), g, rtol=1e-6, atol=1e-6, err_msg=k)
        else:
            np.testing.assert_array_equal(x.cpu().numpy(), g, err_msg=k)
    for mk in ("m", "v"):
        for k, x in state[mk].items():
            if x.numel() or f"{case}/{tag}/{mk}/{k}" in GOLD.files:
                np.testing.assert_array_equal(x.cpu().numpy(), GOLD[f"{case}/{tag}/{mk}/{k}"], err_msg=f"{mk} {k}")
    for k, x in state["stats"].items():
        np.testing.assert_array_equal(x.cpu().numpy(), GOLD[f"{case}/{tag}/stats/{k}"], err_msg=k)


def test_restatement_statistics_match_reference():
    for case in ("default", "screen", "staticonly", "invisible"):
        p = GOLD[f"{case}/pre/param/_xyz"].shape[0], GOLD[f"{case}/pre/param/_xyz_motion"].shape[0]
        st = R.init_stats(*p)
        for j in range(2):
            a = lambda k: torch.from_numpy(GOLD[f"{case}/A{j}/{k}"].copy())
            R.update(st, a("radii"), a("vgrad"), a("egrad"), float(GOLD[f"{case}/A{j}/timestamp"]))
            for k, x in st.items():
                g = GOLD[f"{case}/A{j}/stats/{k}"]
                if "gradient_accum" in k:
                    np.testing.assert_allclose(x.numpy(), g, rtol=2.5e-7, atol=0, err_msg=k)
                else:
                    np.testing.assert_array_equal(x.numpy(), g, err_msg=k)


def test_restatement_densify_and_prunes_match_reference():
    for case in ("default", "screen", "staticonly"):
        cfg = json.loads(str(GOLD[f"{case}/cfg"]))
        st = state_from(case, "pre")
        R.densify_and_prune(st, MODEL, cfg["max_grad"], cfg["max_dgrad"], cfg["min_opacity"], cfg["min_motion_opacity"], cfg["extent"],
                            cfg["max_screen_size"], cfg["max_dynamic_screen_size"], draws_of(case), s_max_ssim=cfg["s_max_ssim"],
                            s_l1_thres=cfg["s_l1_thres"], d_max_ssim=cfg["d_max_ssim"], d_l1_thres=cfg["d_l1_thres"], percent_dense=cfg["percent_dense"])
        assert_state(st, case)
    for case in ("invisible", "small", "nan"):
        st = state_from(case, "pre")
        R.prune(st, case)
        assert_state(st, case, exact_transformed=True)


def test_fixture_covers_the_cases():
    # a clone split through the max_screen_size terms, children, a static-only model, a NaN row, both sides of e0 = 0.01 and 0
    assert GOLD["screen/pre/param/_xyz"].shape[0] + 2 * GOLD["screen/draw/static_split_z"].shape[0] // 2 >= GOLD["screen/post/param/_xyz"].shape[0]
    assert GOLD["staticonly/pre/param/_xyz_motion"].shape[0] == 0
    assert np.isnan(GOLD["nan/pre/param/_xyz"]).any() and not np.isnan(GOLD["nan/post/param/_xyz"]).any()
    e0 = GOLD["default/A0/egrad"][:, 0]
    assert (e0 == 0).any() and ((e0 > 0) & (e0 <= 0.01)).any() and (e0 > 0.01).any()


def test_densify_thresholds_follow_train_py():
    from ex4dgs_amd.densify import densify_thresholds

    class Opt:
        densification_interval, error_base_prune_steps, ssim_prune_every, l1_prune_every = 100, 1000, 3, 5
        s_max_ssim, s_l1_thres, d_max_ssim, d_l1_thres = 0.6, 0.07, 0.4, 0.09
    o = Opt()
    for it in range(100, 4000, 100):
        late = it > o.error_base_prune_steps
        want = (o.s_max_ssim if late and it % (o.densification_interval * o.ssim_prune_every) == 0 else 0,
                o.s_l1_thres if late and it % (o.densification_interval * o.l1_prune_every) == 0 else 100,
                o.d_max_ssim if late and it % (o.densification_interval * o.ssim_prune_every) == 0 else 0,
                o.d_l1_thres if late and it % (o.densification_interval * o.l1_prune_every) == 0 else 100)
        assert densify_thresholds(it, o) == want
        assert densify_thresholds(it, dict(vars(Opt))) == want
    assert densify_thresholds(1500, o) == (0.6, 0.07, 0.4, 0.09)
