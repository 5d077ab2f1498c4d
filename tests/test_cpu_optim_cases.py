"""What keeps the bit-for-bit bars of tests/test_gpu_optim_edges.py honest, without a GPU: the scalar coefficients of every case
are not rounding accidents of the host's pow / sqrt, the numpy restatement (oracle/optim_oracle.py) follows torch.optim.RAdam in
float64 at every case step, the cases of tests/optim_cases.py hit the edges they name, and ex4d_radam_step refuses bad descriptors
before it launches anything."""
import ctypes
import decimal
import fractions

import numpy as np
import torch

from oracle import optim_oracle as oo
from tests import optim_cases as oc

f32 = np.float32
FLT_MAX = np.finfo(f32).max


# ------------------------------------------------------------------------------------------------------------------ coefficients
MIDPOINT_MARGIN = 1e-12           # relative; the host's double pow / sqrt / products are good to ~1e-15


def _is_the_float32_of(x32, exact):
    """x32 is what a single correct rounding of the real number `exact` (a Fraction) gives, and stays so under a relative error of
    MIDPOINT_MARGIN (thousands of double ulps): `exact` lies between the midpoints to x32's float32 neighbours, further than that
    margin from either."""
    x = fractions.Fraction(float(x32))
    lo = (x + fractions.Fraction(float(np.nextafter(x32, f32(-np.inf))))) / 2
    hi = (x + fractions.Fraction(float(np.nextafter(x32, f32(np.inf))))) / 2
    slack = abs(exact) * fractions.Fraction(MIDPOINT_MARGIN)
    return lo + slack < exact < hi - slack


def _exact_coefficients(step, lr, beta1, beta2, eps):
    """The coefficients of fill_coefficients as real numbers of the DOUBLE arguments, to 80 digits."""
    D = decimal.Decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 80
        b1, b2 = D(beta1), D(beta2)                      # exact values of the doubles
        rho_inf = 2 / (1 - b2) - 1
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        rho_t = rho_inf - 2 * step * b2 ** step / bc2
        rect = ((rho_t - 4) * (rho_t - 2) * rho_inf / ((rho_inf - 4) * (rho_inf - 2) * rho_t)).sqrt() if rho_t > 5 else D(0)
        vals = dict(w1=1 - b1, beta2=b2, w2=1 - b2, bc1=bc1, lr=D(lr), sqrt_bc2=bc2.sqrt(), rect=rect, eps=D(eps))
        return {k: fractions.Fraction(v) for k, v in vals.items()}, rho_t > 5, float(abs(rho_t - 5))


def test_no_coefficient_of_any_case_is_a_rounding_accident():
    """Each float32 coefficient of every (step, betas, lr) the cases run equals the float32 of its exact value (80 digits), which is
    further than 1e-12 (relative) from the next rounding midpoint, and no rho_t sits within 1e-3 of the switch: errors of the host's
    double pow / sqrt, thousands of ulps even, cannot decide a GPU test."""
    pts = oc.coefficient_points()
    assert {s for s, _, _ in pts} >= {1, 5, 6, 7, 8, 12, 100, 29999, 30000, 30001, 120000} and {b for _, b, _ in pts} == {oc.BETAS, oc.BETAS_B}
    for step, betas, lr in pts:
        c = oo.radam_coefficients(step, lr, betas[0], betas[1], oc.EPS)
        exact, rectified, margin = _exact_coefficients(step, lr, betas[0], betas[1], oc.EPS)
        assert c.rectified == rectified and margin > 1e-3, (step, betas)
        for k, x in exact.items():
            got = getattr(c, k)
            assert got.dtype == f32
            if k == "rect" and not rectified:
                assert got == 0
            else:
                assert _is_the_float32_of(got, x), (step, betas, lr, k)


# ------------------------------------------------------------------------------------------------------------------ torch in float64
def _torch_step64(p, g, m, v, step, lr, betas):
    q = torch.nn.Parameter(torch.tensor(p, dtype=torch.float64))
    opt = torch.optim.RAdam([q], lr=lr, betas=betas, eps=oc.EPS)
    q.grad = torch.tensor(g, dtype=torch.float64)
    opt.step()                                             # creates the state; overwritten below
    st = opt.state[q]
    with torch.no_grad():
        q.copy_(torch.tensor(p, dtype=torch.float64))
        st["step"].fill_(step - 1)
        st["exp_avg"].copy_(torch.tensor(m, dtype=torch.float64))
        st["exp_avg_sq"].copy_(torch.tensor(v, dtype=torch.float64))
    opt.step()
    return q.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


# measured on these inputs: rel exp_avg 1.10e-07, rel exp_avg_sq 1.24e-07, |dp| 0.498 ulp(max |p|) (2.4e-07 at max |p| = 5.0).
# The bars are 4 x that (numpy builds may sum differently); values far above mean the restatement is wrong, not the bar tight.
MEASURED_M, MEASURED_V, MEASURED_P_ULP = 1.10e-7, 1.24e-7, 0.498
BAR_M, BAR_V, BAR_P_ULP = 4 * MEASURED_M, 4 * MEASURED_V, 4 * MEASURED_P_ULP


def test_restatement_follows_torch_float64_at_every_case_step():
    """One step from identical float32 state at every (step, betas, lr) of the cases against torch.optim.RAdam on the CPU in float64
    (state preset): largest relative error of exp_avg and exp_avg_sq, largest |dp| in ulp(max |p|).  Bars: 4 x the measured values."""
    r = np.random.default_rng(77)
    n = 2000
    p = (r.standard_normal(n) * 1.5).astype(f32)
    g = (r.standard_normal(n) * 1e-2).astype(f32)
    m = (np.sign(g) * np.abs(r.standard_normal(n)) * 1e-2).astype(f32)      # the sign of g: the relative error of exp_avg is not a cancellation's
    v = (r.random(n) * 1e-4 + 1e-6).astype(f32)
    ulp = float(np.spacing(np.abs(p).max()))
    worst = [0.0, 0.0, 0.0]
    for step, betas, lr in oc.coefficient_points():
        t = dict(p=p, g=g, m=m, v=v, step=step, lr=lr, betas=betas)
        p32, m32, v32 = oc.expected_dense(t)
        p64, m64, v64 = _torch_step64(p, g, m, v, step, lr, betas)
        e = (float(np.abs((m32 - m64) / m64).max()), float(np.abs((v32 - v64) / v64).max()), float(np.abs(p32 - p64).max()) / ulp)
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert not np.array_equal(p32, p)
    print(f"restatement against torch float64: rel m {worst[0]:.3e}, rel v {worst[1]:.3e}, |dp| {worst[2]:.3f} ulp(max|p|) = {worst[2] * ulp:.3e}")
    assert worst[0] <= BAR_M and worst[1] <= BAR_V and worst[2] <= BAR_P_ULP, worst


# ------------------------------------------------------------------------------------------------------------------ the cases hit their edges
def test_value_edge_plants_give_what_they_are_named_for():
    at = oc.edge_index
    with np.errstate(all="ignore"):
        res = {run: oc.expected_dense(oc.edge_run(*run)) for run in oc.EDGE_RUNS}
    t = oc.edge_tensor()
    tiny = np.finfo(f32).tiny
    for (step, flag), (p, m, v) in res.items():
        c = oo.radam_coefficients(step, oc.EDGE_LR, *oc.BETAS, oc.EPS)
        assert c.rectified == (step == 6)
        # zero state, zero gradient: nothing moves, the zeros keep their signs' meaning (0 / (0 + eps) is 0, not NaN)
        for name in ("zero", "neg_zero"):
            assert p[at(name)] == t["p"][at(name)] and m[at(name)] == 0 and v[at(name)] == 0
        # a subnormal gradient: exp_avg is a subnormal that a flushing kernel would lose, exp_avg_sq underflows to 0
        for i in (at("g_subnormal"), at("g_subnormal", tail=True)):
            assert 0 < m[i] < tiny and v[i] == 0
        assert 0 < v[at("v_subnormal")] < tiny and 0.9 < np.sqrt(v[at("v_at_eps")]) / c.eps < 1.1
        # (w2 g) g: finite at 1e20 (1e37), inf at 1e21 -- there adaptive = 0 and the update is 0 times a finite exp_avg
        for s in ("", "-"):
            assert np.isfinite(v[at(f"g_{s}1e20")]) and v[at(f"g_{s}1e20")] > 9e36
            i = at(f"g_{s}1e21")
            assert v[i] == np.inf and np.isfinite(m[i]) and m[i] != 0
            if c.rectified:
                assert c.sqrt_bc2 / (np.sqrt(v[i]) + c.eps) == 0 and p[i] == t["p"][i]           # adaptive == 0, upd == 0
            else:
                assert p[i] != t["p"][i]
        i, j, k = at("g_inf"), at("g_-inf"), at("g_nan")
        if flag:
            # sanitised: +-inf -> +-FLT_MAX, exp_avg = exp_avg + 0.1 (FLT_MAX - exp_avg) -- 0.1 FLT_MAX to the bit here; NaN -> 0
            assert m[i] == f32(t["m"][i] + f32(0.1) * (FLT_MAX - t["m"][i])) and m[j] == f32(t["m"][j] + f32(0.1) * (-FLT_MAX - t["m"][j]))
            assert m[i] == f32(0.1) * FLT_MAX and m[j] == -(f32(0.1) * FLT_MAX)
            assert v[i] == np.inf and v[j] == np.inf and np.isfinite(m[k]) and np.isfinite(v[k]) and np.isfinite(p[k])
            assert not np.isnan(p).any() and not np.isnan(m).any() and not np.isnan(v).any()
        else:
            assert m[i] == np.inf and m[j] == -np.inf and np.isnan(m[k]) and np.isnan(v[k]) and np.isnan(p[k])
            if c.rectified:
                assert np.isnan(p[i]) and np.isnan(p[j])                                          # inf * (sqrt_bc2 / inf)
            else:
                assert p[i] == -np.inf and p[j] == np.inf
            nan = np.isnan(p) | np.isnan(m) | np.isnan(v)
            assert set(np.flatnonzero(nan)) <= set(t["planted"])
        # |p| = 1e30 does not notice the update, 1e-30 is replaced by it; exp_avg against the gradient's sign shrinks
        assert p[at("p_1e30")] == f32(1e30) and p[at("p_-1e30")] == f32(-1e30) and abs(p[at("p_1e-30")]) > 1e-9
        assert -0.5 < m[at("m_against_g")] < 0 and 0 < m[at("g_against_m")] < 0.5


def test_slot_list_alternates_and_differs_between_neighbours():
    ts = oc.slot_tensors(oc.MAX_TENSORS + 1)
    assert len(ts) == 33 and {t["p"].size for t in ts} == set(oc.SLOT_NUMELS) and sum(t["p"].size for t in ts) < 200_000
    rect = [oo.radam_coefficients(t["step"], t["lr"], *oc.BETAS, oc.EPS).rectified for t in ts]
    assert all(a != b for a, b in zip(rect, rect[1:]))
    assert {t["step"] for t in ts} == set(oc.UNRECTIFIED_STEPS) | set(oc.RECTIFIED_STEPS) == {1, 5, 6, 7, 12, 100, 29999, 30000, 120000}
    assert all(a["lr"] != b["lr"] and a["step"] != b["step"] for a, b in zip(ts, ts[1:]))
    assert any({a["lr"], b["lr"]} == {1e-4, 5e-2} for a, b in zip(ts, ts[1:]))
    flags = [t["nan_to_num"] for t in ts]
    assert all(not (a and b) for a, b in zip(flags, flags[1:])) and {(f, r) for f, r in zip(flags, rect)} == {(0, False), (0, True), (1, False), (1, True)}
    for t in ts:
        g = t["g"]
        assert np.isnan(g).sum() == 1 and (g.size == 1 or ((g == np.inf).sum() == 1 and (g == -np.inf).sum() == 1))
        p, m, v = oc.expected_dense(t)
        nan = np.isnan(p) | np.isnan(m) | np.isnan(v)
        assert (nan & ~oc.planted_mask(t)).sum() == 0 and nan.any() == (not t["nan_to_num"])
    assert oc.ZERO_POSITIONS == (0, 5, 6, 31)


def test_trajectories_cross_the_switch_of_both_beta_pairs():
    for betas in (oc.BETAS, oc.BETAS_B):
        sw = oc.switch_step(betas)
        steps = oc.trajectory_steps(betas)
        assert betas[0] > 0.5 and {sw - 1, sw} <= set(steps) and set(range(1, 9)) <= set(steps)
        assert not oo.radam_coefficients(sw - 1, 1e-3, *betas, oc.EPS).rectified and oo.radam_coefficients(sw, 1e-3, *betas, oc.EPS).rectified
        runs = oc.trajectory(betas)
        assert [s for s, _, _ in runs["late"][3]] == [29999, 30000, 30001] and runs["late"][1].any() and not runs["early"][1].any()
        assert runs["early"][0].size == oc.CHUNK + 1


def test_window_sets_show_every_class_and_the_staging_limits_are_exact():
    ts = oc.sliced_tensors()
    assert [t["shape"] for t in ts][:5] == [(1003, 35, 3), (0, 35, 4), (777, 35, 4), (5, 7, 3), (33, 1, 4)]
    assert sum(1 for t in ts if t["shape"][0]) == 6                                       # 4 + 2 launches
    assert len({(t["step"], t["lr"]) for t in ts}) == len(ts)
    seen = set().union(*(oc.window_classes(t) for t in ts if t["shape"][0]))
    assert seen == {"eight", "identical", "count==K", "count==1", "first==0", "first==K-count", "overlapping"}
    assert oc.window_classes(ts[3]) >= {"overlapping"} and len(ts[3]["windows"]) == 3
    assert any(f + b.shape[1] == t["shape"][1] and b.shape[1] > 1 for t in ts for f, b in t["windows"])   # a window touching K on its last slice
    rng = oc.sliced_tensors(True)[3]
    assert (rng["row0"] * rng["shape"][1] * rng["shape"][2]) % 4 != 0 and rng["shape"][0] * 21 > 3 * oc.CHUNK
    # the out-of-range positions are what the host refuses, and clipping leaves the windows the header describes
    for t in oc.outside_tensors():
        K = t["shape"][1]
        count = t["windows"][0][1].shape[1]
        assert [f for f, _ in t["windows"]] == [-count, -1, K - count + 1, K - 1, K]
        dense = oo.dense_from_windows(*t["shape"], t["windows"])
        assert dense[:, 0].any() and dense[:, K - 1].any()
        first, blk = t["windows"][1]                                                     # first = -1: keyframe 0 takes the block's slice 1
        alone = oo.dense_from_windows(*t["shape"], [(first, blk)])
        assert np.array_equal(alone[:, 0], blk[:, 1]) and (count < 3 or np.array_equal(alone[:, 1], blk[:, 2])) and not alone[:, count - 1:].any()
    # staging limits
    assert {k: oc.reg_rows(*k) for k in oc.REG_ROWS_TABLE} == oc.REG_ROWS_TABLE
    assert oc.reg_lds_bytes(341, 3) == 32736 and oc.reg_lds_bytes(256, 4) == 32768 == oc.REG_LDS_BYTES
    mixed = oc.reg_mixed_case()
    assert {t["shape"][1] for t in mixed} == {1, 2, 35, 341} and {t["kind"] for t in mixed} == {0, 1, 2}
    assert len({oc.reg_rows(t["shape"][1], t["shape"][2]) for t in mixed}) >= 3
    assert max(range(4), key=lambda i: oc.reg_lds_bytes(*mixed[i]["shape"][1:])) != 3


def test_dense_from_windows_adds_in_index_order_in_float32():
    a = np.full((1, 1, 3), 1e8, f32); b = np.full((1, 1, 3), 1.0, f32); c = np.full((1, 1, 3), -1e8, f32)
    assert oo.dense_from_windows(1, 2, 3, [(0, a), (0, b), (0, c)])[0, 0, 0] == 0.0      # (1e8 + 1) - 1e8 in float32
    assert oo.dense_from_windows(1, 2, 3, [(0, a), (0, c), (0, b)])[0, 0, 0] == 1.0
    assert oo.dense_from_windows(1, 2, 3, [(1, a)]).dtype == f32 and not oo.dense_from_windows(1, 2, 3, [(2, a), (-1, a)]).any()


# ------------------------------------------------------------------------------------------------------------------ refusals before any launch
def test_dense_step_refuses_bad_descriptors_before_any_launch():
    """ex4d_radam_step validates on the host and returns before its launch in each of these calls (a launch without a GPU would give
    EX4D_ERR_HIP, not EX4D_ERR_ARG / EX4D_OK).  The pointers are addresses of host dummies that nothing dereferences."""
    from ex4dgs_amd import _abi
    lib = _abi.load()
    OK, ERR_ARG = 0, 1
    dummy = (ctypes.c_float * 4)()
    a = ctypes.addressof(dummy)
    T = _abi.Ex4dRadamTensor
    good = lambda **kw: T(**{**dict(param=a, grad=a, exp_avg=a, exp_avg_sq=a, numel=4, lr=1e-3, step=1, nan_to_num=0, reserved=0), **kw})
    empty = T(None, None, None, None, 0, 1e-3, 1, 0, 0)

    def call(descs, count=None):
        arr = (T * max(1, len(descs)))(*descs)
        rc = lib.ex4d_radam_step(arr if descs or count is None else None, len(descs) if count is None else count, 0.9, 0.999, 1e-8, None)
        return rc, lib.ex4d_optim_last_error().decode()

    assert call([good()] * 33) == (ERR_ARG, "count 33 outside [0, 32]")
    assert call([good()], count=-1) == (ERR_ARG, "count -1 outside [0, 32]")
    assert call([], count=1) == (ERR_ARG, "count 1 outside [0, 32]")                      # null tensors with count > 0
    for bad in (good(step=0), good(numel=-1), good(param=None), good(grad=None), good(exp_avg=None), good(exp_avg_sq=None)):
        assert call([empty, bad]) == (ERR_ARG, "tensor 1: null pointer, negative size or step < 1")
    assert call([good(numel=1 << 44)]) == (ERR_ARG, "too many elements for one launch")
    # nothing to do is not an error, and clears the text of the refusal before it
    assert call([empty]) == (OK, "") and call([empty] * 32) == (OK, "") and call([], count=0) == (OK, "")
    assert lib.ex4d_radam_step(None, 0, 0.9, 0.999, 1e-8, None) == OK
