"""The keyframe states that training creates (tests/golden/model_getters_states.npz, captured from the reference's CGaussianModel in
float32 and float64 by tests/golden/make_golden_attr_states.py): before the HIP kernels are compared with that fixture
(tests/test_gpu_attr_states.py), this repository's two CPU restatements -- oracle/model_oracle.py and the torch getters of
ex4dgs_amd.scene.DynamicGaussians -- must agree with it on every family and timestamp, NaN positions included, within HALF of every bar the
GPU test uses (tests/attr_states.py), and the fixture must hold the inputs it claims: every branch taken, no row near a threshold."""
import numpy as np
import pytest

from tests import attr_states as st

CASES = [(cfg, t) for cfg in st.CONFIGS for t in st.CONFIGS[cfg]["timestamps"]]


@pytest.fixture(scope="module")
def z():
    return st.load()


def test_clamp_constants_are_the_same_floats_in_c_and_torch():
    f = np.float32
    assert f(1) - f(1e-4) == f(1 - 1e-4) and f(-1) + f(1e-4) == f(-1 + 1e-4)       # `1.0f - 1e-4f` of the kernel == clamp(..., 1-1e-4) of torch


def test_fixture_layout_and_families(z):
    assert tuple(z["families"]) == st.FAMILIES
    for cfg, c in st.CONFIGS.items():
        fam = z[f"{cfg}/family"]
        assert z[f"{cfg}/param/_rotation_motion"].shape == (fam.size, c["K"], 4)
        assert set(np.unique(fam)) == set(range(len(st.FAMILIES)))
        # ordinary rows lie between the special ones: no family is one contiguous block
        assert all(np.ptp(rows) >= rows.size for rows in st.family_rows(z, cfg).values())
        for t in c["timestamps"]:                  # keyframe gradients are stored as the 4 / 2 keyframes around k, everything else is zero
            k = st.time_index(cfg, t)[0]
            assert z[f"{cfg}/{st.tkey(t)}/grad_slices/_xyz_motion"].tolist() == [k - 1, k, k + 1, k + 2]
            assert z[f"{cfg}/{st.tkey(t)}/grad_slices/_rotation_motion"].tolist() == [k, k + 1]
            assert z[f"{cfg}/{st.tkey(t)}/grad/_xyz_motion"].shape == (fam.size, 4, 3) and z[f"{cfg}/{st.tkey(t)}/f64/grad/_rotation_motion"].dtype == np.float64
    rows = st.family_rows(z, "a")
    assert all(24 <= rows[f].size <= 48 for f in st.FAMILIES if f not in ("opposite_exact", "window_underflow"))
    assert rows["opposite_exact"].size >= 16 and rows["window_underflow"].size >= 12
    q = z["a/param/_rotation_motion"]
    assert (q[rows["identical"]] == q[rows["identical"]][:, :1]).all()
    norms = np.linalg.norm(q[rows["identical"]][:, 0], axis=-1)
    assert norms.min() < 0.4 and norms.max() > 2.5
    assert (q[rows["opposite_exact"]][:, 1:] == -q[rows["opposite_exact"]][:, :-1]).all()
    v = z["a/param/_opacity_duration_var"]
    assert (v[rows["window_clone_split"]] == 2).all() and v[rows["window_conversion"]].max() >= 300 and v[rows["window_underflow"]].max() < -87.4


def test_time_scalars_of_both_configurations():
    from ex4dgs_amd.attributes import time_scalars
    expect = {("a", 0): (1, 0.2), ("a", 3): (1, 0.5), ("a", 8): (2, 0.0), ("a", 137): (14, 0.9), ("a", 299): (31, 0.1), ("a", 308): (32, 0.0),
              ("b", 0): (1, 0.6), ("b", 4.5): (2, 0.5), ("b", 27): (7, 0.0), ("b", 57): (13, 0.0)}
    for (cfg, t), (k, delta) in expect.items():
        c = st.CONFIGS[cfg]
        shift = c["time_pad"] + c["interval"]
        s = time_scalars(t, 3, 5, c["K"], c["duration"], c["interval"], shift, st.VAR_PAD)
        assert (s.Ns, s.Nd, s.K, s.k) == (3, 5, c["K"], k) and s.k == st.time_index(cfg, t)[0]
        assert s.delta == np.float32(delta) and s.tau == np.float32((t + shift) / c["interval"]) and s.var_min == np.float32(st.VAR_PAD / c["interval"])
        assert s.t == np.float32(t) and s.duration == c["duration"]
        d = delta
        basis = (2 * d ** 3 - 3 * d ** 2 + 1, d ** 3 - 2 * d ** 2 + d, -2 * d ** 3 + 3 * d ** 2, d ** 3 - d ** 2)
        assert (s.h00, s.h10, s.h01, s.h11) == tuple(np.float32(b) for b in basis)
    for cfg, c in st.CONFIGS.items():              # the last timestamp is the last usable keyframe index, the first ones the first
        assert st.time_index(cfg, c["timestamps"][-1])[0] == c["K"] - 3 and st.time_index(cfg, c["timestamps"][0])[0] == 1
        assert c["timestamps"][-1] >= c["duration"] + 5


def test_every_branch_is_taken_and_no_row_sits_on_a_threshold(z):
    for cfg, c in st.CONFIGS.items():
        P = st.params(z, cfg)
        assert not st.margin_violations(P, cfg).any()
        most = dict.fromkeys(st.CENSUS, 0)
        for t in c["timestamps"]:
            now = st.census(P, cfg, t)
            k, delta, _ = st.time_index(cfg, t)
            raw, ps_raw, _ = st.slerp_state(P["_rotation_motion"][:, k], P["_rotation_motion"][:, k + 1], delta)
            assert np.abs(np.abs(raw) - st.HI).min() >= st.THRESHOLD_MARGIN and ps_raw.min() >= 1 - 1e-12
            for b in st.CENSUS:
                assert np.array_equal(now[b], z[f"{cfg}/{st.tkey(t)}/census/{b}"]), (cfg, t, b)     # the stored census is the census of the stored rows
                most[b] = max(most[b], int(now[b].sum()))
        print(cfg, "most rows per branch at one timestamp:", most)
        assert all(most[b] == 0 for b in st.UNREACHABLE)
        if cfg == "a":
            assert all(most[b] >= st.MIN_ROWS_PER_BRANCH for b in st.CENSUS if b not in st.UNREACHABLE), most
    # delta = 0, 0.5 and two more; tau before both centres, between them, after both and on one
    assert {st.time_index("a", t)[1] for t in st.CONFIGS["a"]["timestamps"]} >= {0.0, 0.5, 0.2, 0.9}


@pytest.mark.parametrize("runner", ["run_oracle", "run_getters"])
@pytest.mark.parametrize("cfg,t", CASES)
def test_cpu_restatements_sit_within_half_of_every_bar(z, runner, cfg, t):
    outs, grads = getattr(st, runner)(st.params(z, cfg), st.weights(z, cfg), cfg, t)
    worst, failures = st.check(z, cfg, t, outs, grads, scale=0.5)
    assert not failures, st.format_failures(failures)
    nan = {n: int(np.isnan(z[f"{cfg}/{st.tkey(t)}/grad/{n}"]).sum()) for n in st.NAMES}
    assert all(v == 0 for n, v in nan.items() if n != "_opacity_duration_var")            # the reference's NaN: 0 * inf of an overflowing width only
    over = z[f"{cfg}/{st.tkey(t)}/census/overflow"]
    assert nan["_opacity_duration_var"] == int(over.sum())
    assert np.array_equal(np.isnan(z[f"{cfg}/{st.tkey(t)}/grad/_opacity_duration_var"]).any(axis=(1, 2)), over)
    print(runner, cfg, t, "worst error / bar:", max(v[2] for v in worst.values()))


def test_opposite_rows_are_where_the_reference_itself_is_noisy(z):
    """The per-row bars of the opposite families come from here: max |float32 reference - float64 reference| per family."""
    noise = {}
    for cfg, t in CASES:
        key = f"{cfg}/{st.tkey(t)}"
        Ns = z[f"{cfg}/param/_xyz"].shape[0]
        for f, rows in st.family_rows(z, cfg).items():
            a = np.abs(z[f"{key}/rot"][Ns + rows] - z[f"{key}/f64/rot"][Ns + rows]).max()
            g32, g64 = z[f"{key}/grad/_rotation_motion"][rows], z[f"{key}/f64/grad/_rotation_motion"][rows]
            b = np.abs(g32 - g64).max() / max(1.0, np.abs(g32).max())
            noise[f] = tuple(max(x, y) for x, y in zip(noise.get(f, (0, 0)), (a, b)))
    print("float32 against float64 reference, (rotation output, relative keyframe gradient):", noise)
    for f, (a, b) in noise.items():
        if f not in st.OPPOSITE:
            assert a <= st.FWD_BAR / 2 and b <= st.GRAD_BAR / 2, (f, a, b)
