"""GPU tests of the motion regularisers (train.py:155-168 of the reference): the stand-alone op (ex4dgs_amd/regularizers.py), the
regularised sliced RAdam step (ex4d_radam_step_sliced_reg) and both trainers, against tests/golden/regularizers.npz (what the
reference's own lines + torch.optim.RAdam gave) and tests/reg_ref.py in float64."""
import os

import numpy as np
import pytest
import torch

from tests import helpers as h
from tests import reg_ref

pytestmark = pytest.mark.gpu

ROOT = h.ROOT
NAMES = ("_xyz_disp", "_xyz_motion", "_rotation_motion")
HALF_ULP = 2.0 ** -24
BETAS, EPS = (0.9, 0.999), 1e-8


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "regularizers.npz"))


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def seeded_model(seed, Ns, Nd, K, edges=True):
    """_xyz_disp, _xyz_motion (a random walk per Gaussian), _rotation_motion (near-unit quaternions), with the edge rows."""
    g = torch.Generator().manual_seed(seed)
    disp = 0.02 * torch.randn(Ns, 3, generator=g)
    motion = torch.randn(Nd, 1, 3, generator=g) + torch.cumsum(0.05 * torch.randn(Nd, K, 3, generator=g), 1)
    rot = torch.nn.functional.normalize(torch.randn(Nd, 1, 4, generator=g) + torch.cumsum(0.1 * torch.randn(Nd, K, 4, generator=g), 1), dim=-1)
    rot = rot * (1 + 0.05 * torch.randn(Nd, K, 1, generator=g))
    if edges and Ns > 3:
        disp[3] = 0
    if edges and Nd > 7 and K > 9:
        motion[5] = motion[5, :1]
        motion[6, 7] = motion[6, 0]
        rot[2, 9] = 0
        rot[4, 0] = 0
        rot[7, K - 1] = rot[7, K - 1] / rot[7, K - 1].norm() * 1e-8
    return disp.contiguous(), motion.contiguous(), rot.contiguous()


def torch_twin(d, m, r, w):
    """The three terms in plain torch (what a user composes today), from the formulas of include/ex4d_regularizers.h."""
    loss = torch.zeros((), dtype=d.dtype, device=d.device)
    if w[0] > 0:
        loss = loss + w[0] * torch.log(d.norm(dim=-1) + 0.001).mean()
    if w[1] > 0 and m.shape[0] > 0:
        loss = loss + w[1] * (m[:, :1] - m[:, 1:]).norm(dim=-1).mean()
    if w[2] > 0 and r.shape[0] > 0:
        a, b = r[:, 1:], r[:, :-1]
        loss = loss + w[2] * (1 - (a * b).sum(dim=-1) / a.norm(dim=-1).clamp_min(1e-6) / b.norm(dim=-1).clamp_min(1e-6)).mean()
    return loss


def check_values(out4, d, m, r, w, want3=None, tag=""):
    got = out4.double().cpu().numpy()
    want = [float(x) for x in (want3 if want3 is not None else reg_ref.values(d, m, r, np.float64))]
    scale = reg_ref.mean_abs_terms(d, m, r)
    rep = {}
    for i, n in enumerate(("static", "motion", "rot")):
        err, bar = abs(got[i] - want[i]), 1e-6 * scale[i]
        rep[n] = dict(value=want[i], err=float(err), bar=float(bar))
        print(f"{tag} {n}: value {want[i]:.9g} err {err:.3e} bar {bar:.3e}")
        assert err <= bar, (n, got[i], want[i], err, bar)
    total = sum(float(wi) * x for wi, x in zip(w, want))
    bar = 1e-6 * sum(abs(float(wi)) * s for wi, s in zip(w, scale))
    assert abs(got[3] - total) <= bar, (got[3], total, bar)
    h.REPORT.append(dict(kind="regularizer_values", tag=tag, **rep))


def check_dense_grads(grads, d, m, r, w, ref64=None, tag=""):
    ref64 = ref64 if ref64 is not None else reg_ref.grads(d, m, r, w, np.float64)
    scales = reg_ref.grad_scales(d, m, r, w)
    rep = {}
    for i, n in enumerate(NAMES):
        got = grads[i].double().cpu().numpy()
        A, terms = scales[i]
        bar = (16 + terms) * HALF_ULP * A
        err = np.abs(got - ref64[i])
        live = A > 0
        worst = float((err[live] / bar[live]).max()) if live.any() else 0.0
        rep[n] = dict(worst_err_over_bar=worst, max_abs_err=float(err.max()), max_abs_grad=float(np.abs(ref64[i]).max()))
        print(f"{tag} {n}: worst error / bar {worst:.3f}, max |err| {err.max():.3e}, max |grad| {np.abs(ref64[i]).max():.3e}")
        assert np.isfinite(got).all(), n
        assert (got[~live] == 0).all() and (ref64[i][~live] == 0).all(), n          # exact zeros where no term acts
        assert (err <= bar).all(), (n, worst)
    h.REPORT.append(dict(kind="regularizer_gradients", tag=tag, **rep))


# ------------------------------------------------------------------------------------------------ values and dense gradients
def test_values_match_the_reference_lines(hip_lib):
    from ex4dgs_amd import regularizers as reg
    z = golden()
    d, m, r = (z["probe" + n] for n in NAMES)
    w = z["probe_weights"]
    out = reg.forward_raw(cuda(d), cuda(m), cuda(r), w)
    torch.cuda.synchronize()
    check_values(out, d, m, r, w, want3=[z["probe_mean_" + n] for n in ("static_reg", "motion_reg", "rot_reg")], tag="probe")
    total = float(out[3])
    assert abs(total - float(z["probe_loss_f64"])) <= 1e-6 * sum(wi * s for wi, s in zip(w, reg_ref.mean_abs_terms(d, m, r)))
    # the same bits on every call (fixed partial-sum layout, no atomics)
    again = reg.forward_raw(cuda(d), cuda(m), cuda(r), w)
    assert torch.equal(out, again)
    # a mean over nothing is 0: no static Gaussians, no dynamic ones, one keyframe
    e = reg.forward_raw(torch.zeros(0, 3).cuda(), torch.zeros(0, 35, 3).cuda(), torch.zeros(0, 35, 4).cuda(), w)
    assert float(e.abs().max()) == 0.0
    one = reg.forward_raw(cuda(d), cuda(m[:, :1]), cuda(r[:, :1]), w)
    assert float(one[1]) == 0.0 and float(one[2]) == 0.0 and float(one[0]) == float(out[0])
    # a larger seeded model against the float64 restatement
    d2, m2, r2 = (t.numpy() for t in seeded_model(21, 4000, 2000, 35))
    check_values(reg.forward_raw(cuda(d2), cuda(m2), cuda(r2), w), d2, m2, r2, w, tag="seed21")


def test_dense_gradients_match_autograd_of_the_reference_lines(hip_lib):
    from ex4dgs_amd import regularizers as reg
    z = golden()
    d, m, r = (z["probe" + n] for n in NAMES)
    w = z["probe_weights"]
    ref64 = [z[f"probe_grad{n}_f64"] for n in NAMES]
    P = [cuda(x) for x in (d, m, r)]
    G = [torch.full_like(p, float("nan")) for p in P]                                  # accumulate = 0 writes every element
    reg.backward_raw(*P, w, G)
    torch.cuda.synchronize()
    check_dense_grads(G, d, m, r, w, ref64=ref64, tag="probe raw")
    # autograd surface: the weighted sum and its gradients
    Q = [p.clone().requires_grad_(True) for p in P]
    loss = reg.motion_regularizers(*Q, *w)
    (2.0 * loss).backward()                                                            # upstream scalar 2: an exact scaling in float32
    assert abs(float(loss.detach()) - float(z["probe_loss_f64"])) <= 1e-6 * sum(wi * s for wi, s in zip(w, reg_ref.mean_abs_terms(d, m, r)))
    for q, g in zip(Q, G):
        assert torch.equal(q.grad, 2.0 * g)
    # accumulate = 1 adds to what is there; a NULL gradient skips its tensor; weight 0 leaves the gradient alone
    base = [torch.randn_like(p) * 1e-6 for p in P]
    acc = [b.clone() for b in base]
    reg.backward_raw(*P, w, acc, accumulate=True)
    for a, b, g in zip(acc, base, G):
        assert torch.equal(a, b + g)
    acc = [b.clone() for b in base]
    reg.backward_raw(*P, (w[0], 0.0, w[2]), [acc[0], acc[1], None], accumulate=True)
    assert torch.equal(acc[0], base[0] + G[0]) and torch.equal(acc[1], base[1]) and torch.equal(acc[2], base[2])
    zero = [torch.full_like(p, float("nan")) for p in P]
    reg.backward_raw(*P, (0.0, 0.0, 0.0), zero)
    assert all(float(t.abs().max()) == 0.0 for t in zero)
    # larger seeded models, edge rows included, against the float64 restatement (pinned to the fixture by the CPU tests)
    for seed in (21, 22):
        d2, m2, r2 = seeded_model(seed, 4000, 2000, 35)
        P2 = [d2.cuda(), m2.cuda(), r2.cuda()]
        G2 = [torch.empty_like(p) for p in P2]
        reg.backward_raw(*P2, w, G2)
        check_dense_grads(G2, d2.numpy(), m2.numpy(), r2.numpy(), w, tag=f"seed{seed}")


# ------------------------------------------------------------------------------------------------ fused step = dense step
def _keyframe_tensor(g, rows, K, Cc):
    if Cc == 3:
        p = torch.randn(rows, 1, 3, generator=g) + torch.cumsum(0.05 * torch.randn(rows, K, 3, generator=g), 1)
        if rows > 2:
            p[2] = p[2, :1]                                   # every keyframe equals keyframe 0
    else:
        p = torch.nn.functional.normalize(torch.randn(rows, 1, 4, generator=g) + torch.cumsum(0.1 * torch.randn(rows, K, 4, generator=g), 1), dim=-1)
        if rows > 2 and K > 1:
            p[2, 1] = 0                                       # a zero keyframe
            p[1, K - 1] = p[1, K - 1] * 1e-8                  # one below the clamp
    return p.contiguous().cuda()


def _fused_vs_dense(g, total_rows, row0, rows, K, Cc, kind, n_windows, steps, first_dev, weight=1e-3, lr=1e-2):
    """`steps` optimizer steps on rows [row0, row0 + rows) of a [total_rows, K, C] tensor, both ways; returns nothing, asserts bits."""
    from ex4dgs_amd import optim
    from ex4dgs_amd import regularizers as reg
    dev = torch.device("cuda", 0)
    p0 = _keyframe_tensor(g, total_rows, K, Cc)
    A, B = p0.clone(), p0.clone()
    mA, vA, mB, vB = [torch.zeros_like(p0) for _ in range(4)]
    cnt = min(4 if Cc == 3 else 2, K)
    off = row0 * K * Cc
    rng = lambda t: t.view(-1)[off:off + rows * K * Cc]
    for step in range(1, steps + 1):
        wins, dense = [], torch.zeros_like(p0)
        for _ in range(n_windows):
            first = int(torch.randint(0, K - cnt + 1, (1,), generator=g))
            blk = (1e-4 * torch.randn(rows, cnt, Cc, generator=g)).cuda()
            wins.append((first, cnt, blk))
            dense[row0:row0 + rows, first:first + cnt] += blk                         # windows added in index order
        # dense path: windows scattered into zeros + the regulariser's dense gradient (over the FULL tensor: the mean's constant) + ex4d_radam_step
        w3 = (0.0, weight if kind == optim.REG_MOTION else 0.0, weight if kind == optim.REG_ROT else 0.0)
        if kind == optim.REG_MOTION:
            reg.backward_raw(None, A, None, w3, (None, dense, None), accumulate=True)
        elif kind == optim.REG_ROT:
            reg.backward_raw(None, None, A, w3, (None, None, dense), accumulate=True)
        if rows:
            optim.radam_step_raw([(rng(A).data_ptr(), rng(dense).data_ptr(), rng(mA).data_ptr(), rng(vA).data_ptr(), rows * K * Cc, lr, step)], BETAS, EPS, dev)
        fdev = torch.tensor([f for f, _, _ in wins], dtype=torch.int32).cuda() if first_dev else None
        item = (rng(B).data_ptr() if rows else B.data_ptr(), rng(mB).data_ptr() if rows else mB.data_ptr(), rng(vB).data_ptr() if rows else vB.data_ptr(),
                rows, K, Cc, lr, step, [((None if first_dev else f), c, b.data_ptr()) for f, c, b in wins], fdev.data_ptr() if first_dev else None,
                kind, weight, total_rows)
        optim.radam_step_sliced_reg_raw([item], BETAS, EPS, dev)
        torch.cuda.synchronize()
        assert torch.equal(A, B) and torch.equal(mA, mB) and torch.equal(vA, vB), (total_rows, row0, rows, K, Cc, kind, n_windows, step)
        assert torch.isfinite(A).all()
    if rows and K > 1 and kind:
        assert not torch.equal(A, p0)
    # rows outside the range were not touched
    if row0:
        assert torch.equal(B[:row0], p0[:row0]) and float(mB[:row0].abs().max()) == 0.0


@pytest.mark.parametrize("K", [1, 2, 35])
@pytest.mark.parametrize("kind", [1, 2])
def test_fused_regularised_step_equals_the_dense_step_bit_for_bit(hip_lib, K, kind):
    """ex4d_radam_step_sliced_reg against (windows scattered into zeros + ex4d_reg_backward(accumulate=1) + ex4d_radam_step): p, m, v
    bit-identical.  A consistency check between two paths; the anchor is the trajectory test below."""
    from ex4dgs_amd import optim
    Cc = 3 if kind == optim.REG_MOTION else 4
    R = optim.sliced_reg_rows(K, Cc)
    assert R >= 4 and R % 4 == 0
    g = torch.Generator().manual_seed(100 * K + kind)
    for rows in (1, 3, R - 1, R, R + 1, 5 * R + 2):
        for n_windows in (1, 3):
            _fused_vs_dense(g, rows, 0, rows, K, Cc, kind, n_windows, steps=2, first_dev=(n_windows == 3))
    _fused_vs_dense(g, 5 * R + 2, 0, 5 * R + 2, K, Cc, kind, 3, steps=8, first_dev=False)          # crosses rho_t > 5
    # an offset row range of a larger tensor (the base pointer is not 16-byte aligned for odd K C): the mean's constant is the full count
    _fused_vs_dense(g, 5 * R + 9, 3, 5 * R + 2, K, Cc, kind, 1, steps=2, first_dev=False)
    _fused_vs_dense(g, 5 * R + 9, 4, R + 1, K, Cc, kind, 3, steps=2, first_dev=True)
    _fused_vs_dense(g, 7, 0, 0, K, Cc, kind, 1, steps=1, first_dev=False)                           # rows = 0: nothing happens


def test_fused_step_without_a_regulariser_gives_the_bits_of_the_sliced_step(hip_lib):
    from ex4dgs_amd import optim
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(7)
    for rows, K, Cc in ((1003, 35, 3), (777, 35, 4), (5, 7, 3), (33, 1, 4)):
        p0 = torch.randn(rows, K, Cc, generator=g).cuda()
        A, B, Cw = p0.clone(), p0.clone(), p0.clone()
        mA, vA, mB, vB, mC, vC = [torch.zeros_like(p0) for _ in range(6)]
        cnt = min(4 if Cc == 3 else 2, K)
        for step in range(1, 9):
            wins = []
            for _ in range(1 + step % 3):
                first = int(torch.randint(0, K - cnt + 1, (1,), generator=g))
                wins.append((first, cnt, torch.randn(rows, cnt, Cc, generator=g).cuda()))
            ws = [(f, c, b.data_ptr()) for f, c, b in wins]
            optim.radam_step_sliced_raw([(A.data_ptr(), mA.data_ptr(), vA.data_ptr(), rows, K, Cc, 1e-2, step, ws)], BETAS, EPS, dev)
            optim.radam_step_sliced_reg_raw([(B.data_ptr(), mB.data_ptr(), vB.data_ptr(), rows, K, Cc, 1e-2, step, ws, None, optim.REG_NONE, 0.0, rows)],
                                            BETAS, EPS, dev)
            # a live kind with weight 0 is a plain step too
            kind = optim.REG_MOTION if Cc == 3 else optim.REG_ROT
            optim.radam_step_sliced_reg_raw([(Cw.data_ptr(), mC.data_ptr(), vC.data_ptr(), rows, K, Cc, 1e-2, step, ws, None, kind, 0.0, rows)],
                                            BETAS, EPS, dev)
            torch.cuda.synchronize()
            assert torch.equal(A, B) and torch.equal(mA, mB) and torch.equal(vA, vB), (rows, K, Cc, step)
            assert torch.equal(A, Cw) and torch.equal(mA, mC) and torch.equal(vA, vC), (rows, K, Cc, step)
    # argument errors: a kind that does not fit C, a K whose rows do not fit the staging LDS (the callers then take the dense path)
    with pytest.raises(RuntimeError, match="reg_kind"):
        optim.radam_step_sliced_reg_raw([(A.data_ptr(), mA.data_ptr(), vA.data_ptr(), 33, 1, 4, 1e-2, 1, [], None, optim.REG_MOTION, 1.0, 33)], BETAS, EPS, dev)
    assert optim.sliced_reg_rows(2000, 3) == 0
    big = torch.zeros(4, 2000, 3).cuda()
    with pytest.raises(RuntimeError, match="do not fit"):
        optim.radam_step_sliced_reg_raw([(big.data_ptr(), big.data_ptr(), big.data_ptr(), 4, 2000, 3, 1e-2, 1, [], None, optim.REG_MOTION, 1.0, 4)], BETAS, EPS, dev)
    h.assert_sliced_steps_refuse_bad_descriptors(dev)


# ------------------------------------------------------------------------------------------------ the anchor: reference lines + torch.optim.RAdam
def _trajectory_bar(z, n, s, got):
    want = z["traj" + n][s]
    moved = np.abs(want - z["traj_init" + n]).max()
    bar = 1e-3 * moved + 2 * 2.0 ** -23 * np.abs(want).max()
    err = np.abs(got.cpu().numpy() - want).max()
    return float(err), float(bar)


def test_trajectory_follows_the_reference_lines_and_torch_radam(hip_lib):
    """8 steps (crossing rho_t > 5) of loss = reference block + sum(window * slice) under torch.optim.RAdam, recorded in the fixture:
    (i) raw fused step + ex4d_reg_backward / ex4d_radam_step for _xyz_disp, (ii) motion_regularizers -> autograd -> FusedRAdam."""
    from ex4dgs_amd import optim
    from ex4dgs_amd import regularizers as reg
    z = golden()
    dev = torch.device("cuda", 0)
    w, lrs = [float(x) for x in z["traj_weights"]], dict(zip(NAMES, (float(x) for x in z["traj_lrs"])))
    steps = z["traj_first"].shape[0]
    assert steps == 8
    # (i)
    P = {n: cuda(z["traj_init" + n]) for n in NAMES}
    M = {n: torch.zeros_like(P[n]) for n in NAMES}
    V = {n: torch.zeros_like(P[n]) for n in NAMES}
    Nd, K = P["_xyz_motion"].shape[:2]
    worst = 0.0
    for s in range(steps):
        fx, fr = (int(x) for x in z["traj_first"][s])
        wx, wr = cuda(z["traj_window_xyz"][s]), cuda(z["traj_window_rot"][s])
        gd = torch.zeros_like(P["_xyz_disp"])
        reg.backward_raw(P["_xyz_disp"], None, None, w, (gd, None, None), accumulate=True)
        optim.radam_step_raw([(P["_xyz_disp"].data_ptr(), gd.data_ptr(), M["_xyz_disp"].data_ptr(), V["_xyz_disp"].data_ptr(), gd.numel(),
                               lrs["_xyz_disp"], s + 1)], BETAS, EPS, dev)
        items = []
        for n, Cc, first, blk, kind, wt in (("_xyz_motion", 3, fx, wx, optim.REG_MOTION, w[1]), ("_rotation_motion", 4, fr, wr, optim.REG_ROT, w[2])):
            items.append((P[n].data_ptr(), M[n].data_ptr(), V[n].data_ptr(), Nd, K, Cc, lrs[n], s + 1, [(first, blk.shape[1], blk.data_ptr())], None,
                          kind, wt, Nd))
        optim.radam_step_sliced_reg_raw(items, BETAS, EPS, dev)
        torch.cuda.synchronize()
        for n in NAMES:
            err, bar = _trajectory_bar(z, n, s, P[n])
            print(f"raw step {s + 1} {n}: err {err:.3e} bar {bar:.3e}")
            worst = max(worst, err / bar)
            assert err <= bar, ("raw", n, s, err, bar)
    h.REPORT.append(dict(kind="regularizer_trajectory", tag="raw fused step", worst_err_over_bar=worst))
    # (ii)
    Q = {n: cuda(z["traj_init" + n]).requires_grad_(True) for n in NAMES}
    opt = optim.FusedRAdam([{"params": [Q[n]], "lr": lrs[n]} for n in NAMES], lr=0.001)
    worst = 0.0
    for s in range(steps):
        fx, fr = (int(x) for x in z["traj_first"][s])
        wx, wr = cuda(z["traj_window_xyz"][s]), cuda(z["traj_window_rot"][s])
        opt.zero_grad(set_to_none=True)
        loss = reg.motion_regularizers(Q["_xyz_disp"], Q["_xyz_motion"], Q["_rotation_motion"], *w)
        loss = loss + (Q["_xyz_motion"][:, fx:fx + 4] * wx).sum() + (Q["_rotation_motion"][:, fr:fr + 2] * wr).sum()
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        for n in NAMES:
            err, bar = _trajectory_bar(z, n, s, Q[n].detach())
            print(f"autograd step {s + 1} {n}: err {err:.3e} bar {bar:.3e}")
            worst = max(worst, err / bar)
            assert err <= bar, ("autograd", n, s, err, bar)
    h.REPORT.append(dict(kind="regularizer_trajectory", tag="autograd + FusedRAdam", worst_err_over_bar=worst))


# ------------------------------------------------------------------------------------------------ trainers on a rendered scene
TIMES = (0, 137, 41, 299, 7, 138, 40, 139)
W3 = (1e-4, 1e-4, 1e-3)


def _scene():
    from ex4dgs_amd.scene import make_scene
    model, cam, bg = make_scene("cfg3", P=8000, device="cuda", fused=True)
    return model, cam.to("cuda"), bg.cuda()


def _agree(ma, mb, p0, what):
    for n in ma.PARAM_NAMES:
        a, b = getattr(ma, n), getattr(mb, n)
        moved = float((a - p0[n]).abs().max())
        assert moved > 0 and torch.isfinite(a).all(), (what, n)
        ulp = 2.0 ** -23 * float(a.abs().max())
        err = float((a - b).abs().max())
        assert err <= 1e-3 * moved + 2 * ulp, (what, n, err, moved)


def test_trainers_with_regularizers_agree_with_each_other_and_with_the_torch_composition(hip_lib):
    """FrameTrainer(regularizers=w) sliced and dense, NativeTrainer.set_regularizers(w), and what a user composes today (the
    FrameTrainer's gradients + autograd of the three torch terms + torch.optim.RAdam), on copies of one model over several timestamps:
    the bars of the compiled trainer's own test (tests/test_gpu_round2.py).  The regularisers are live: the parameters differ from a run
    without them."""
    from ex4dgs_amd.loss import l1_ssim_loss
    from ex4dgs_amd.native_trainer import NativeTrainer
    from ex4dgs_amd.trainer import FrameTrainer, NAN_TO_NUM
    models = [_scene() for _ in range(5)]
    (ms, cam, bg), (md, _, _), (mn, _, _), (mt, _, _), (moff, _, _) = models
    assert ms.num_dynamic > 0 and ms.num_static > 0
    gt = torch.rand(3, cam.image_height, cam.image_width, generator=torch.Generator().manual_seed(11)).cuda()
    lrs = {n: 1e-4 for n in ms.PARAM_NAMES}
    p0 = {n: getattr(ms, n).clone() for n in ms.PARAM_NAMES}
    upg = lambda out: ([l1_ssim_loss(out["render"], gt, 0.2)[0]], [None])
    ts = FrameTrainer(ms, optimizer=True, lrs=lrs, regularizers=W3)
    td = FrameTrainer(md, optimizer=True, lrs=lrs, regularizers=lambda: W3, sliced=False)
    toff = FrameTrainer(moff, optimizer=True, lrs=lrs)
    tn = NativeTrainer(mn, cam, optimizer=True, lrs=lrs)
    tn.set_regularizers(W3)
    assert ts.sliced and not td.sliced
    # the composition of today: gradients of the render + L1/SSIM part from a FrameTrainer without optimizer, the three terms by autograd
    tg = FrameTrainer(mt, optimizer=False)
    names = list(mt.PARAM_NAMES)
    topt = torch.optim.RAdam([{"params": [getattr(mt, n)], "lr": lrs[n]} for n in names], lr=0.001)
    for t in TIMES:
        ts.step(cam, bg, t, upg); td.step(cam, bg, t, upg); toff.step(cam, bg, t, upg); tn.step(cam, bg, t, gt)
        tg.step(cam, bg, t, upg); tg.flush()
        grads = tg.grads()
        leaves = [getattr(mt, n).detach().clone().requires_grad_(True) for n in NAMES]
        rg = torch.autograd.grad(torch_twin(*leaves, W3), leaves)
        for n in names:
            g = grads[n].clone()
            if n in NAMES:
                g += rg[NAMES.index(n)]
            if n in NAN_TO_NUM:
                g = torch.nan_to_num(g)
            getattr(mt, n).grad = g
        topt.step()
        # the reported terms: float[4] on the device, at the parameters the frame was rendered with
        torch.cuda.synchronize()
    reg4 = ts.last["reg"]
    assert reg4.is_cuda and reg4.shape == (4,) and torch.isfinite(reg4).all() and float(reg4[3]) != 0.0
    ts.flush(); td.flush(); toff.flush(); torch.cuda.synchronize()
    # NativeTrainer's output 6 is evaluated at the same (pre-update) parameters of the last frame as FrameTrainer's last["reg"]
    rn = tn.output("reg")
    assert float((rn - reg4).abs().max()) <= 1e-4 * float(reg4.abs().max())      # (the two trainers' parameters agree to 1e-3 of their movement)
    assert float(tn.output("loss")) > 0                              # what = 0 stays the L1/SSIM loss
    _agree(ms, md, p0, "sliced vs dense")
    _agree(ms, mn, p0, "FrameTrainer vs NativeTrainer")
    _agree(ms, mt, p0, "FrameTrainer vs torch composition")
    _agree(mn, mt, p0, "NativeTrainer vs torch composition")
    # the feature is live.  _xyz_disp: further from the run without regularisers than two equal computations may be; the keyframe tensors
    # (values of order 10-100, updates of a few ulp): keyframes no window touched never move without the regularisers (zero gradient,
    # zero momentum) and do move with them
    a, b = ms._xyz_disp, moff._xyz_disp
    moved = float((a - p0["_xyz_disp"]).abs().max())
    assert float((a - b).abs().max()) > 1e-3 * moved + 2 * 2.0 ** -23 * float(a.abs().max())
    for n in NAMES[1:]:
        still = getattr(moff, n) == p0[n]
        frac_still, frac_moved = float(still.float().mean()), float((getattr(ms, n)[still] != p0[n][still]).float().mean())
        print(f"{n}: {frac_still:.3f} of the entries untouched without regularisers, {frac_moved:.3f} of those moved with them")
        assert frac_still > 0 and frac_moved > 0, (n, frac_still, frac_moved)      # (without the terms such an entry cannot move at all)
    tn.close()
    with pytest.raises(NotImplementedError):
        FrameTrainer(moff, exchange="allreduce", optimizer=True, regularizers=W3)


def test_trainers_with_regularizers_off_reproduce_todays_parameters_bit_for_bit(hip_lib):
    """regularizers=None / weights 0 take today's call sequence: the parameters of 4 steps are those of a trainer built without the
    keyword, bit for bit -- FrameTrainer and NativeTrainer."""
    from ex4dgs_amd.loss import l1_ssim_loss
    from ex4dgs_amd.native_trainer import NativeTrainer
    from ex4dgs_amd.trainer import FrameTrainer
    runs = [_scene() for _ in range(5)]
    cam, bg = runs[0][1], runs[0][2]
    gt = torch.rand(3, cam.image_height, cam.image_width, generator=torch.Generator().manual_seed(11)).cuda()
    lrs = {n: 1e-4 for n in runs[0][0].PARAM_NAMES}
    upg = lambda out: ([l1_ssim_loss(out["render"], gt, 0.2)[0]], [None])
    f_today = FrameTrainer(runs[0][0], optimizer=True, lrs=lrs)
    f_none = FrameTrainer(runs[1][0], optimizer=True, lrs=lrs, regularizers=None)
    f_zero = FrameTrainer(runs[2][0], optimizer=True, lrs=lrs, regularizers=(0.0, 0.0, 0.0))
    n_today = NativeTrainer(runs[3][0], cam, optimizer=True, lrs=lrs)
    n_zero = NativeTrainer(runs[4][0], cam, optimizer=True, lrs=lrs)
    n_zero.set_regularizers(0.0, 0.0, 0.0)
    for t in TIMES[:4]:
        for f in (f_today, f_none, f_zero):
            f.step(cam, bg, t, upg)
        n_today.step(cam, bg, t, gt); n_zero.step(cam, bg, t, gt)
    for f in (f_today, f_none, f_zero):
        f.flush()
    torch.cuda.synchronize()
    for n in runs[0][0].PARAM_NAMES:
        assert torch.equal(getattr(runs[0][0], n), getattr(runs[1][0], n)), ("FrameTrainer None", n)
        assert torch.equal(getattr(runs[0][0], n), getattr(runs[2][0], n)), ("FrameTrainer zero weights", n)
        assert torch.equal(getattr(runs[3][0], n), getattr(runs[4][0], n)), ("NativeTrainer zero weights", n)
    n_today.close(); n_zero.close()


# ------------------------------------------------------------------------------------------------ graph capture, scale
def test_forward_and_fused_step_replay_from_a_graph(hip_lib):
    from ex4dgs_amd import optim
    from ex4dgs_amd import regularizers as reg
    dev = torch.device("cuda", 0)
    d, m, r = (t.cuda() for t in seeded_model(31, 500, 300, 35))
    w = (1e-4, 1e-4, 1e-3)
    wx, wr = (1e-4 * torch.randn(300, 4, 3)).cuda(), (1e-4 * torch.randn(300, 2, 4)).cuda()

    class State:
        def __init__(self):
            self.m, self.r = m.clone(), r.clone()
            self.mom = [torch.zeros_like(t) for t in (m, m, r, r)]
            self.out, self.scratch = torch.zeros(4, device=dev), reg.new_scratch(dev)

        def run(self, step):
            reg.forward_raw(d, self.m, self.r, w, out=self.out, scratch=self.scratch)
            optim.radam_step_sliced_reg_raw([
                (self.m.data_ptr(), self.mom[0].data_ptr(), self.mom[1].data_ptr(), 300, 35, 3, 1e-3, step, [(5, 4, wx.data_ptr())], None, optim.REG_MOTION, w[1], 300),
                (self.r.data_ptr(), self.mom[2].data_ptr(), self.mom[3].data_ptr(), 300, 35, 4, 1e-3, step, [(9, 2, wr.data_ptr())], None, optim.REG_ROT, w[2], 300)],
                BETAS, EPS, dev)
    eager, graphed = State(), State()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        graphed.run(7)                                       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graphed.m.copy_(m); graphed.r.copy_(r)
    for t in graphed.mom:
        t.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.run(7)                                       # the step count is a host constant of the capture
    graphed.m.copy_(m); graphed.r.copy_(r)
    for t in graphed.mom:
        t.zero_()
    for _ in range(3):
        g.replay()
        eager.run(7)
    torch.cuda.synchronize()
    assert torch.equal(graphed.out, eager.out) and torch.equal(graphed.m, eager.m) and torch.equal(graphed.r, eager.r)
    assert all(torch.equal(a, b) for a, b in zip(graphed.mom, eager.mom)) and not torch.equal(eager.m, m)


def test_config3_scale_fused_equals_dense_and_values_hold(hip_lib):
    """Ns = 800 k, Nd = 200 k, K = 35 once: the fused step against the dense one bit for bit, the loss terms against float64."""
    from ex4dgs_amd import optim
    from ex4dgs_amd import regularizers as reg
    dev = torch.device("cuda", 0)
    Ns, Nd, K = 800_000, 200_000, 35
    d, m, r = seeded_model(41, Ns, Nd, K)
    w = (1e-4, 1e-4, 1e-3)
    dc, mc, rc = d.cuda(), m.cuda(), r.cuda()
    check_values(reg.forward_raw(dc, mc, rc, w), d.numpy(), m.numpy(), r.numpy(), w, tag="config 3")
    g = torch.Generator().manual_seed(5)
    for p0, Cc, cnt, kind, wt in ((mc, 3, 4, optim.REG_MOTION, w[1]), (rc, 4, 2, optim.REG_ROT, w[2])):
        A, B = p0.clone(), p0.clone()
        mA, vA, mB, vB = [torch.zeros_like(p0) for _ in range(4)]
        for step in (1, 2):
            first = int(torch.randint(0, K - cnt + 1, (1,), generator=g))
            blk = (1e-4 * torch.randn(Nd, cnt, Cc, generator=g)).cuda()
            dense = torch.zeros_like(p0)
            dense[:, first:first + cnt] += blk
            w3 = (0.0, wt if kind == optim.REG_MOTION else 0.0, wt if kind == optim.REG_ROT else 0.0)
            reg.backward_raw(None, A if Cc == 3 else None, A if Cc == 4 else None, w3, (None, dense if Cc == 3 else None, dense if Cc == 4 else None),
                             accumulate=True)
            optim.radam_step_raw([(A.data_ptr(), dense.data_ptr(), mA.data_ptr(), vA.data_ptr(), A.numel(), 1e-3, step)], BETAS, EPS, dev)
            optim.radam_step_sliced_reg_raw([(B.data_ptr(), mB.data_ptr(), vB.data_ptr(), Nd, K, Cc, 1e-3, step, [(first, cnt, blk.data_ptr())], None, kind, wt, Nd)],
                                            BETAS, EPS, dev)
            torch.cuda.synchronize()
            assert torch.equal(A, B) and torch.equal(mA, mB) and torch.equal(vA, vB), (Cc, step)
        del A, B, mA, vA, mB, vB, dense
