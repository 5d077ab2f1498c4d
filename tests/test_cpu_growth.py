"""Growth of the dynamic set without a GPU: the torch restatement (tests/growth_ref.py) against the reference's own outputs
(tests/golden/growth.npz, tests/golden/make_golden_growth.py), ErrorTimestamps against the reference's recorded sequence, the
arithmetic the radix select relies on (select, then normalise; the float32 rank of torch.quantile), and the new part of the C ABI."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import densify_ref as D
from tests import growth_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "growth.npz"))
EXTRACT_CASES = ("extract", "first", "motion", "minmotion", "unseen")
EXPAND_CASES = ("early_short", "early_static", "early_fits", "expand", "expand_small")
# what a call computes rather than copies: held to rtol = atol = 1e-6 (the bar of tests/test_cpu_densify.py for transformed values);
# everything else is exact
GENERATED = {"extract": ("_xyz_motion", "_opacity_duration_center", "_opacity_duration_var"),
             "expand": ("_xyz_motion", "_rotation_motion"), "adjust": ()}
EXTRACT_KEYS = ("extent", "percentile", "motion_thres", "min_motion_thres")


def cfg_of(case):
    return json.loads(str(GOLD[f"{case}/cfg"]))


def model_of(case):
    c = cfg_of(case) if f"{case}/cfg" in GOLD.files else {}
    if case in EXTRACT_CASES:
        duration = c["duration"]
    else:
        duration = c.get("duration_before", 300)
    return {"interval": 10, "time_shift": 12, "time_pad": 2, "duration": duration}


def state_from(case, tag, device="cpu"):
    t = lambda k: torch.from_numpy(GOLD[k].copy()).to(device)
    names = D.STATIC + D.DYNAMIC
    params = {k: t(f"{case}/{tag}/param/{k}") for k in names}
    m = {k: t(f"{case}/{tag}/m/{k}") for k in names if f"{case}/{tag}/m/{k}" in GOLD.files}
    v = {k: t(f"{case}/{tag}/v/{k}") for k in names if f"{case}/{tag}/v/{k}" in GOLD.files}
    stats = {k: t(f"{case}/{tag}/stats/{k}") for k in D.S_STATS + D.D_STATS}
    return {"params": params, "m": m, "v": v, "stats": stats}


def assert_state(state, case, generated=(), tag="post"):
    """Parameters, moments and statistics of `state` against the reference's: exact, the `generated` parameters within 1e-6."""
    for k, x in state["params"].items():
        g = GOLD[f"{case}/{tag}/param/{k}"]
        assert tuple(x.shape) == g.shape, (k, x.shape, g.shape)
        if k in generated:
            np.testing.assert_allclose(x.detach().cpu().numpy(), g, rtol=1e-6, atol=1e-6, err_msg=k)
        else:
            np.testing.assert_array_equal(x.detach().cpu().numpy(), g, err_msg=k)
    for mk in ("m", "v"):
        for k, x in state[mk].items():
            np.testing.assert_array_equal(x.cpu().numpy(), GOLD[f"{case}/{tag}/{mk}/{k}"], err_msg=f"{mk} {k}")
    for k, x in state["stats"].items():
        np.testing.assert_array_equal(x.cpu().numpy(), GOLD[f"{case}/{tag}/stats/{k}"], err_msg=k)


def assert_old_rows_untouched(state, case):
    """The dynamic rows an extraction finds keep their bits (parameters and moments)."""
    for k in D.DYNAMIC:
        old = GOLD[f"{case}/pre/param/{k}"]
        if old.shape[0]:
            np.testing.assert_array_equal(state["params"][k].detach().cpu().numpy()[:old.shape[0]], old, err_msg=k)


def extract_kwargs(case):
    c = cfg_of(case)
    return {k: c[k] for k in EXTRACT_KEYS if k in c}


# ------------------------------------------------------------------------------------------ the restatement against the reference
@pytest.mark.parametrize("case", EXTRACT_CASES)
def test_restatement_extraction_matches_reference(case):
    st, model = state_from(case, "pre"), model_of(case)
    vis, cam = torch.from_numpy(GOLD[f"{case}/vis"].copy()), torch.from_numpy(GOLD[f"{case}/cam"].copy())
    out = R.extract(st, model, cam, vis, **extract_kwargs(case))
    c = cfg_of(case)
    assert int(out["mask"].sum()) == c["selected"] and out["visible"] == int(vis.sum())
    assert st["params"]["_xyz_motion"].shape[1] == c["keyframe_num"]
    assert abs(out["threshold"] - c["theta64"]) <= 1e-5 * c["theta64"]
    assert_state(st, case, GENERATED["extract"])
    assert_old_rows_untouched(st, case)


def test_fixture_covers_the_cases():
    assert GOLD["first/pre/param/_xyz_motion"].shape[0] == 0 and cfg_of("first")["keyframe_num"] == 6 and cfg_of("first")["duration"] == 5
    assert GOLD["extract/pre/param/_xyz_motion"].shape[0] > 0 and cfg_of("extract")["keyframe_num"] == 35
    for case in EXTRACT_CASES:
        # the selection was decided with margin: no visible score within 1e-5 (relative) of the threshold
        assert cfg_of(case)["margin"] > 1e-5 and cfg_of(case)["selected"] > 0
        st = state_from(case, "pre")
        vis, cam = torch.from_numpy(GOLD[f"{case}/vis"].copy()), torch.from_numpy(GOLD[f"{case}/cam"].copy())
        u, n = R.scores(st["params"], cam, vis)
        above = u > R.quantile(u, cfg_of(case).get("percentile", 0.98))
        seen = st["stats"]["xyz_error_min_timestamp"].view(-1)[vis] >= 0
        kw = extract_kwargs(case)
        if case == "motion":
            assert (~above & (n > kw["motion_thres"] * kw["extent"])).any()
        if case == "minmotion":
            assert (above & ~(n > kw["min_motion_thres"] * kw["extent"])).any()
        if case == "unseen":
            assert (above & ~seen).any() and (above & seen).any()
    k35, k5 = GOLD["expand/pre/param/_xyz_motion"].shape[1], GOLD["expand_small/pre/param/_xyz_motion"].shape[1]
    assert (k35, GOLD["expand/post/param/_xyz_motion"].shape[1]) == (35, 38) and (k5, GOLD["expand_small/post/param/_xyz_motion"].shape[1]) == (5, 7)
    c, v = GOLD["adjust/pre/param/_opacity_duration_center"], GOLD["adjust/pre/param/_opacity_duration_var"]
    assert (c < 1.4).any() and (c > 31.0).any() and (v < 0.5).any() and ((v > 0.5) & (v < 1)).any() and (v > 1).any()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "growth.npz")) < 1 << 20


@pytest.mark.parametrize("case", EXPAND_CASES)
def test_restatement_expand_duration_matches_reference(case):
    c = cfg_of(case)
    st, model = state_from(case, "pre"), model_of(case)
    assert R.expand_duration(st, model, c["argument"]) is c["returned"]
    assert model["duration"] == c["duration_after"]
    assert_state(st, case, GENERATED["expand"] if c["returned"] else ())
    if c["returned"]:
        K = GOLD[f"{case}/pre/param/_xyz_motion"].shape[1]
        for k in ("_xyz_motion", "_rotation_motion"):              # the first K keyframes are copies
            np.testing.assert_array_equal(st["params"][k].numpy()[:, :K], GOLD[f"{case}/pre/param/{k}"])


def test_restatement_adjust_temp_opa_matches_reference():
    st, model = state_from("adjust", "pre"), model_of("adjust")
    R.adjust_temp_opa(st, model)
    assert_state(st, "adjust")
    assert (st["m"]["_opacity_duration_var"] == 0).all() and (st["m"]["_xyz_motion"] != 0).any()


def test_extrapolation_step_is_the_references():
    """lin_interp_last subtracts ONE keyframe (x[K - avg - 1]) from each of the last avg: on a track that moves one unit per
    keyframe the step is the mean of 1 .. avg, not 1.  The golden pins it; this says what it is."""
    x = torch.arange(10, dtype=torch.float32).view(1, 10, 1).repeat(2, 1, 3)
    y = R._extrapolate(x, 2, 4)
    assert torch.equal(y[:, 10:, 0], torch.tensor([[9 + 2.5, 9 + 5.0]] * 2))


# ------------------------------------------------------------------------------------------ the error-timestamp bookkeeping
def test_error_timestamps_follow_the_recorded_sequence():
    from ex4dgs_amd.growth import ErrorTimestamps
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "growth.json")))
    et = ErrorTimestamps(rec["interval"])
    pops = 0
    for op in rec["timestamps"]:
        if op[0] == "mark":
            et.mark(op[1], op[2])
        else:
            assert et.pop() == op[1], (pops, op)
            pops += 1
    assert pops > 30 and et.pop() is None
    # insertion order decides: an interval seen once, met BEFORE the often-seen one, passes the tenth-of-the-most-frequent test
    a, b = ErrorTimestamps(10), ErrorTimestamps(10)
    a.mark(9.0, 5.0)
    for _ in range(20):
        a.mark(1.0, 15.0)
    for _ in range(20):
        b.mark(1.0, 15.0)
    b.mark(9.0, 5.0)
    assert a.pop() == 5.0 and b.pop() == 15.0
    assert sorted(a.errors) == [1.0] and sorted(b.errors) == [0.0]


# ------------------------------------------------------------------------------------------ what the radix select relies on
def _score_vectors():
    g = torch.Generator().manual_seed(3)
    out = []
    for n in (1, 2, 3, 51, 256, 257, 4099, 65537):
        s = torch.rand(n, generator=g) ** 4 * 10 ** float(torch.randint(-3, 4, (1,), generator=g))
        out += [s, torch.full((n,), 0.37), torch.where(torch.rand(n, generator=g) < 0.5, torch.tensor(0.2), torch.tensor(0.7)),
                s * (torch.rand(n, generator=g) < 0.6)]
    return out


def test_select_then_normalise_gives_the_same_bits():
    """The kernels select the two order statistics on the raw scores and divide afterwards; torch normalises, then takes the
    quantile.  Division by a positive constant is monotone (it may merge values, never reorder them), so the results are the same
    bits -- for every vector here, ties, zeros and the interpolated and the exact ranks included."""
    for s in _score_vectors():
        for q in (0.98, 0.5, 0.0, 1.0, 0.8):
            u = s / (s.max() + 0.000001)
            want = torch.quantile(u, q)
            assert torch.equal(R.quantile(u, q), want), (s.numel(), q)
            assert torch.equal(R.quantile_select_then_normalise(s, q), want), (s.numel(), q)
    bits = torch.rand(1000, generator=torch.Generator().manual_seed(1)).mul(100)
    assert torch.equal(torch.argsort(bits, stable=True), torch.argsort(bits.view(torch.int32), stable=True)), "non-negative floats order as integers"
    nan = torch.tensor([0.1, float("nan"), 0.3])
    assert torch.isnan(torch.quantile(nan / (nan.max() + 0.000001), 0.98)) and torch.isnan(R.quantile_select_then_normalise(nan, 0.98))


def test_quantile_rank_is_float32():
    n = 1_000_003
    lo, hi, w = R.quantile_rank(0.98, n)
    assert (lo, hi, float(w)) == (980002, 980002, 0.0) and int(0.98 * (n - 1)) == 980001
    x = torch.rand(n, generator=torch.Generator().manual_seed(2))
    want = torch.quantile(x, 0.98)
    srt = torch.sort(x)[0]
    assert torch.equal(R.quantile(x, 0.98), want) and want == srt[980002] and srt[980001] != srt[980002]
    assert R.quantile_rank(0.98, 51)[:2] == (49, 49) and R.quantile_rank(0.8, 38)[:2] == (29, 30)


# ------------------------------------------------------------------------------------------ the C boundary
def test_growth_abi_exports_and_struct_sizes():
    from ex4dgs_amd import _abi, densify, growth
    names = ("ex4d_growth_scores", "ex4d_growth_select_scratch_bytes", "ex4d_growth_select", "ex4d_growth_classify", "ex4d_growth_append",
             "ex4d_growth_extrapolate", "ex4d_growth_expand_opacity", "ex4d_growth_adjust_opacity")
    assert densify.EXPORTS[-len(names):] == names and densify.EXPORTS.index("ex4d_densify_last_error") == len(densify.EXPORTS) - len(names) - 1
    assert ctypes.sizeof(_abi.Ex4dGrowthClassify) == 88 and ctypes.sizeof(_abi.Ex4dGrowthTensor) == 48 and ctypes.sizeof(_abi.Ex4dGrowthAppend) == 64
    assert growth.MAX_TENSORS == 28 and growth.GROW_STATS == 6
    lib = _abi.load()
    assert lib.ex4d_abi_version() == 5
    assert lib.ex4d_growth_select_scratch_bytes() >= (4 * 256 + 9) * 4 and lib.ex4d_growth_select_scratch_bytes() % 256 == 0
    # refused before any HIP call, with the header's own error text
    for name, args in (("ex4d_growth_select", (None, 5, 0.5, None, None, None)), ("ex4d_growth_extrapolate", (None, None, 0, 5, 5, 3, 3, None)),
                       ("ex4d_growth_classify", (None, None)), ("ex4d_growth_append", (None, 29, None, None))):
        with pytest.raises(RuntimeError) as e:
            _abi.call(name, *args)
        assert str(e.value) == lib.ex4d_densify_last_error().decode() != ""
    assert growth.first_keyframe_count(type("M", (), {"time_shift": 12, "interval": 10})(), 5) == 6
