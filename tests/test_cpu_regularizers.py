"""CPU checks of the motion regularisers (include/ex4d_regularizers.h, ex4dgs_amd/regularizers.py): the numpy restatement
tests/reg_ref.py (hand-derived adjoint, float32 with keyframe 0's sum in ascending k) against what the reference's own lines gave
(tests/golden/regularizers.npz, captured by tests/golden/make_golden_regularizers.py), the iteration gates (the ABI: tests/test_cpu_abi.py)."""
import os
import re
import types

import numpy as np

from oracle import optim_oracle
from tests import reg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("_xyz_disp", "_xyz_motion", "_rotation_motion")
HALF_ULP = 2.0 ** -24


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "regularizers.npz"))


def test_fixture_holds_the_edge_rows_and_stays_small():
    z = golden()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "regularizers.npz")) <= 512 * 1024
    d, m, r = (z["probe" + n] for n in NAMES)
    assert (d.shape, m.shape, r.shape) == ((256, 3), (40, 35, 3), (40, 35, 4))
    assert (np.abs(d).sum(1) == 0).any()                                           # a zero _xyz_disp row
    assert ((m == m[:, :1]).all(axis=(1, 2))).any()                                # a row whose keyframes all equal keyframe 0
    n = np.sqrt((r.astype(np.float64) ** 2).sum(-1))
    assert (n == 0).any() and ((n > 0) & (n < 1e-6)).any()                         # a zero rotation keyframe, one below the clamp
    assert (z["probe_weights"] > 0).all()


def test_values_match_the_reference_lines():
    z = golden()
    d, m, r = (z["probe" + n] for n in NAMES)
    v = reg_ref.values(d, m, r, np.float64)
    for got, name in zip(v, ("static_reg", "motion_reg", "rot_reg")):
        want = float(z["probe_mean_" + name])
        assert abs(got - want) <= 1e-12 * abs(want), (name, got, want)
    assert abs(reg_ref.loss(d, m, r, z["probe_weights"]) - float(z["probe_loss_f64"])) <= 1e-12 * abs(float(z["probe_loss_f64"]))
    # float32 restatement: the project's loss bar (1e-6 of the term) against the float64 value
    v32 = reg_ref.values(d, m, r, np.float32)
    for got, want in zip(v32, v):
        assert abs(float(got) - want) <= 1e-6 * abs(want)


def test_hand_derived_adjoint_matches_autograd_of_the_reference_lines():
    z = golden()
    d, m, r = (z["probe" + n] for n in NAMES)
    w = z["probe_weights"]
    g64 = reg_ref.grads(d, m, r, w, np.float64)
    g32 = reg_ref.grads(d, m, r, w, np.float32)
    scales = reg_ref.grad_scales(d, m, r, w)
    for i, n in enumerate(NAMES):
        ref64 = z[f"probe_grad{n}_f64"]
        assert np.abs(g64[i] - ref64).max() <= 1e-12 * np.abs(ref64).max(), n        # the adjoint itself
        A, terms = scales[i]
        bar = (16 + terms) * HALF_ULP * A
        assert g32[i].dtype == np.float32 and np.isfinite(g32[i]).all()
        assert (np.abs(g32[i].astype(np.float64) - ref64) <= bar).all(), n             # the float32 arithmetic of the kernels, per entry
        assert (g32[i][A == 0] == 0).all() and (ref64[A == 0] == 0).all(), n           # exact zeros where no term acts
        # the reference's own float32 autograd sits inside the same bar (so the bar is not a property of this restatement)
        assert (np.abs(z[f"probe_grad{n}_f32"].astype(np.float64) - ref64) <= bar).all(), n
    # quirks: gradient 0 at a zero norm, and the clamped norm still divides next to a zero rotation keyframe
    assert (g32[0][np.abs(d).sum(1) == 0] == 0).all()
    rows, ks = np.nonzero(np.sqrt((r.astype(np.float64) ** 2).sum(-1)) == 0)
    assert np.abs(g32[2][rows, ks]).max() > 1e3 * np.abs(np.median(g32[2]))


class _Opt(types.SimpleNamespace):
    pass


def test_gates_follow_train_py():
    from ex4dgs_amd.regularizers import regularizer_weights
    z = golden()
    d, m, r = (z["gate" + n] for n in NAMES)
    terms = reg_ref.values(d, m, r, np.float64)
    seen = set()
    for row, want in zip(z["gate_cases"], z["gate_loss"]):
        opt = _Opt(static_reg=row[0], motion_reg=row[1], rot_reg=row[2], progressive_growing_steps=int(row[3]),
                   make_dynamic_interval=int(row[4]), extract_every=int(row[5]))
        it, nd = int(row[6]), int(row[7])
        w = regularizer_weights(opt, it, nd)
        assert w == regularizer_weights(dict(vars(opt)), it, nd)
        got = sum(wi * ti for wi, ti in zip(w, terms))
        assert abs(got - want) <= 1e-12 * max(abs(want), 1e-12), (row, w, got, want)
        seen.add(tuple(x > 0 for x in w))
    # the cases separate the gates: everything off, static alone, each weight off, everything on
    assert {(False, False, False), (True, False, False), (True, True, True), (False, True, True), (True, False, True), (True, True, False)} <= seen


def test_trajectory_of_the_float32_restatement_follows_torch_radam():
    """hand-derived adjoint + oracle.optim_oracle.radam_step on the stored windows against the reference block + torch.optim.RAdam:
    the bar the GPU test holds the fused step to, per tensor and step."""
    z = golden()
    p = {n: z["traj_init" + n].copy() for n in NAMES}
    mom = {n: (np.zeros_like(p[n]), np.zeros_like(p[n])) for n in NAMES}
    w, lrs = z["traj_weights"], dict(zip(NAMES, z["traj_lrs"]))
    worst = 0.0
    for s in range(z["traj_first"].shape[0]):
        fx, fr = (int(x) for x in z["traj_first"][s])
        g = list(reg_ref.grads(p["_xyz_disp"], p["_xyz_motion"], p["_rotation_motion"], w, np.float32))
        g[1] = reg_ref.scatter_windows(p["_xyz_motion"].shape, [(fx, z["traj_window_xyz"][s])]) + g[1]
        g[2] = reg_ref.scatter_windows(p["_rotation_motion"].shape, [(fr, z["traj_window_rot"][s])]) + g[2]
        for n, gi in zip(NAMES, g):
            optim_oracle.radam_step(p[n], gi.astype(np.float32), mom[n][0], mom[n][1], s + 1, lrs[n])
        for n in NAMES:
            want = z["traj" + n][s]
            moved = np.abs(want - z["traj_init" + n]).max()
            bar = 1e-3 * moved + 2 * 2.0 ** -23 * np.abs(want).max()
            err = np.abs(p[n] - want).max()
            worst = max(worst, err / bar)
            assert err <= bar, (n, s, err, bar)
    # the trajectory moved every tensor (the steps past RAdam's rho_t > 5 switch are ~lr whatever the gradient's scale)
    for n in NAMES:
        assert np.abs(p[n] - z["traj_init" + n]).max() > 0, n
    print(f"worst error / bar over the trajectory: {worst:.3f}")


def test_package_does_not_import_tests_or_oracle():
    pkg = os.path.join(ROOT, "ex4dgs_amd")
    for base, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(base, f)).read()
                assert not re.search(r"^\s*(from|import)\s+(tests|oracle)\b", src, flags=re.M), os.path.join(base, f)
