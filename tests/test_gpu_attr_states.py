"""The fused attribute kernels (ex4dgs_amd/csrc/ex4d_attributes.hip: forward, dense backward, sliced backward) on the keyframe states that
training creates, against the reference's own CGaussianModel (tests/golden/model_getters_states.npz; families, bars, census and margins
in tests/attr_states.py; tests/test_cpu_attr_states.py holds this repository's CPU restatements to half of every bar used here):
identical / nearly parallel / opposite keyframe quaternions (both clamp branches of the slerp, its pass-through gates, the zero-vector
fallback), opacity windows as the static->dynamic conversion and clone / split make them (clamped and equal centres, tau on a centre,
log-widths whose exp overflows or underflows: the reference's NaN must come out as NaN in the same place), k = 1 and k = K-3 in two
keyframe configurations, row counts around the 256-thread blocks, fully written gradient buffers, the feature copy beyond one trip of its
grid-stride loop, and states made by this repository's own densify_and_prune.  No row of the fixture is excluded anywhere.

Every comparison records its worst error and bar per family and tensor in the parity report (helpers.REPORT).

Measured on an MI355X when these tests were written (worst error / bar over all cases): opposite_exact rotation output 2.6e-6 / 7.1e-6 and
keyframe gradient 5.2e-3 / 3.3e-2, opposite_perturbed 8.2e-6 / 4.8e-5 and 7.3e-3 / 4.5e-2 (per-row bars: project bar + 4 x the row's
float32-float64 spread of the reference); every other family at most 0.18 of the project bars (1e-6 forward, 1e-5 relative gradients).

Mutants of ex4d_attributes.hip these tests were run against (scratch builds, values only), and whether the earlier attribute tests
(goldens, 200k oracle test, training loop, sliced == dense, split SH) noticed:
  clamp pass-through gate of the dot product removed      caught (12 perturbed-opposite rows below -(1-1e-4), delta not in {0, 0.5}); earlier: no.
      Only the lower half of that gate is observable: above +(1-1e-4) d out / d omega is second order in the angle, removing the gate
      moves the near-parallel gradients by at most 0.26 of their bar, and by exactly 0 on identical keyframes.
  gate of the weight-sum clamp removed (always / never add) not caught, and cannot be: the clamp never binds (tests/attr_states.py), and
      the term it gates is g_r . r = 0 because the blend is renormalised afterwards -- both variants differ from the kernel by rounding only
  zero-vector fallback removed                            caught (NaN output on the exact -q rows at delta = 0.5); earlier: no
  `after` with && instead of ||                           caught (inside the window the other width is selected: the NaN of an overflowing one moves); earlier: no
  tie of the two centres sent to the second index         caught; earlier: no
  width gradient written to the other index               caught; earlier: yes
  `inside` with <= instead of <                           caught (tau exactly on a centre); earlier: no
  dense keyframe offset in the sliced buffer (wrapped)    caught; earlier: yes (sliced == dense)
  feature kernel's stride one block too long              caught (400k rows); earlier: no
`acos >= 1e-4` and `sin >= 1e-4` cannot be false after the clamp of the dot product: no input reaches them."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import attr_states as st
from tests import helpers as h

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = -7.25e33            # where NaN is a legal result (the gradient of an overflowing log-width), buffers are prefilled with this
GUARD = 64                     # floats on either side of a gradient buffer that a call must leave alone (a multiple of 4: float4 stores)

_WORST = dict(kind="attribute_states", tag="fused attribute kernels against the reference's float32 getters on trained keyframe states "
              "(worst error, its bar, error / bar per family and tensor over the cases run)", cases=0, worst={})


def _record(worst, what):
    if _WORST["cases"] == 0:
        h.REPORT.append(_WORST)
    _WORST["cases"] += 1
    for (family, tensor), (err, bar, ratio) in worst.items():
        key = f"{family}/{tensor}"
        if key not in _WORST["worst"] or ratio > _WORST["worst"][key]["ratio"]:
            _WORST["worst"][key] = dict(error=err, bar=bar, ratio=ratio, at=str(what))


@pytest.fixture(scope="module")
def z():
    return st.load()


def _features(Ns, Nd, seed=5):
    g = torch.Generator().manual_seed(seed)
    return {"_features_dc": torch.randn(Ns, 1, 3, generator=g), "_features_rest": torch.randn(Ns, 15, 3, generator=g),
            "_features_dc_motion": torch.randn(Nd, 1, 3, generator=g), "_features_rest_motion": torch.randn(Nd, 15, 3, generator=g)}


def _device_params(z, cfg, rows=None, static_rows=None):
    """The 15 parameter tensors on the GPU in PARAM_ORDER (fixture rows `static_rows` / `rows`, seeded features) and the weights."""
    from ex4dgs_amd.attributes import PARAM_ORDER
    P, W = st.params(z, cfg), st.weights(z, cfg)
    Ns_all = P["_xyz"].shape[0]
    rows = np.arange(P["_xyz_motion"].shape[0]) if rows is None else np.asarray(rows, np.int64)
    static_rows = np.arange(Ns_all) if static_rows is None else np.asarray(static_rows, np.int64)
    sub = {n: torch.tensor(P[n][static_rows if n in st.STATIC else rows]) for n in st.NAMES}
    sub.update(_features(static_rows.size, rows.size))
    all_rows = np.concatenate([static_rows, Ns_all + rows])
    wts = [torch.tensor(W[k][all_rows]).to(DEV) for k in st.OUTPUTS]
    return [sub[n].to(DEV).contiguous() for n in PARAM_ORDER], wts, sub


def _scalars(cfg, t, Ns, Nd):
    from ex4dgs_amd.attributes import time_scalars
    c = st.CONFIGS[cfg]
    s = time_scalars(t, Ns, Nd, c["K"], c["duration"], c["interval"], c["time_pad"] + c["interval"], st.VAR_PAD)
    assert s.k == st.time_index(cfg, t)[0]
    return s


def _named(tensors):
    from ex4dgs_amd.attributes import PARAM_ORDER
    return {n: (None if g is None else g.cpu().numpy()) for n, g in zip(PARAM_ORDER, tensors)}


def _outs(outs):
    return {k: o.detach().cpu().numpy() for k, o in zip(st.OUTPUTS, outs)}


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _check_features(outs, gout, sub, g_shs, with_shs):
    """The feature block is a copy both ways: bit for bit torch.cat forward, bit for bit the split of dL/dshs backward."""
    from ex4dgs_amd.attributes import FEATURE_NAMES, PARAM_ORDER
    if not with_shs:
        assert outs[4].numel() == 0 and all(gout[PARAM_ORDER.index(n)] is None for n in FEATURE_NAMES)
        return
    Ns = sub["_xyz"].shape[0]
    cat = torch.cat([torch.cat([sub["_features_dc"], sub["_features_rest"]], 1), torch.cat([sub["_features_dc_motion"], sub["_features_rest_motion"]], 1)], 0)
    assert _same_bits(outs[4].cpu(), cat)
    g = g_shs.cpu()
    for n, ref in zip(FEATURE_NAMES, (g[:Ns, :1], g[:Ns, 1:], g[Ns:, :1], g[Ns:, 1:])):
        assert _same_bits(gout[PARAM_ORDER.index(n)].cpu(), ref), n


def _assert_ok(failures, what):
    assert not failures, f"{what}: {len(failures)} rows outside their bar: " + st.format_failures(failures)


# ------------------------------------------------------------------ 1. the fixture, every family and timestamp, three ways
CASES = [(cfg, t) for cfg in st.CONFIGS for t in st.CONFIGS[cfg]["timestamps"]]


@pytest.mark.parametrize("cfg,t", CASES)
def test_forward_dense_and_sliced_backward_match_the_reference(hip_lib, z, cfg, t):
    """forward_raw / backward_raw dense and sliced on the whole fixture.  The first and the last timestamp of either configuration are
    k = 1 and k = K-3, the two ends of the keyframe range the kernels accept."""
    from ex4dgs_amd.attributes import backward_raw, forward_raw
    params, wts, sub = _device_params(z, cfg)
    Ns, Nd = sub["_xyz"].shape[0], sub["_xyz_motion"].shape[0]
    scal = _scalars(cfg, t, Ns, Nd)
    outs = forward_raw(scal, params, with_shs=True)
    g_shs = torch.randn(Ns + Nd, 16, 3, generator=torch.Generator().manual_seed(9)).to(DEV)
    dense = backward_raw(scal, params, wts + [g_shs], with_shs=True)
    sliced, hint = backward_raw(scal, params, wts + [g_shs], with_shs=True, sliced=True)
    assert hint == (scal.k - 1, 4, scal.k, 2)
    _check_features(outs, dense, sub, g_shs, True)
    _check_features(outs, sliced, sub, g_shs, True)
    worst, failures = st.check(z, cfg, t, _outs(outs), st.slice_grads(_named(dense), cfg, t))
    _record(worst, ("dense", cfg, t))
    _assert_ok(failures, ("dense", cfg, t))
    worst, failures = st.check(z, cfg, t, _outs(outs), _named(sliced))
    _assert_ok(failures, ("sliced", cfg, t))
    # the two backward entry points run the same arithmetic: same bits, NaN in the same places
    dense_slices, sliced_named = st.slice_grads(_named(dense), cfg, t), _named(sliced)
    for n in st.NAMES:
        assert np.array_equal(dense_slices[n].view(np.int32), sliced_named[n].view(np.int32)), n
    nan = np.isnan(_named(dense)["_opacity_duration_var"]).any(axis=(1, 2))
    assert np.array_equal(nan, z[f"{cfg}/{st.tkey(t)}/census/overflow"])


@pytest.mark.parametrize("cfg,t", [("a", 3), ("a", 137), ("b", 57)])
@pytest.mark.parametrize("with_shs", [True, False])
def test_autograd_surface_matches_the_reference(hip_lib, z, cfg, t, with_shs):
    from ex4dgs_amd.attributes import PARAM_ORDER, evaluate_attributes
    c = st.CONFIGS[cfg]
    params, wts, sub = _device_params(z, cfg)
    named = {n: p.requires_grad_(True) for n, p in zip(PARAM_ORDER, params)}
    outs = evaluate_attributes(named, t, duration=c["duration"], interval=c["interval"], time_shift=c["time_pad"] + c["interval"], var_pad=st.VAR_PAD,
                               with_shs=with_shs)
    g_shs = torch.randn(outs[4].shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    (sum((o * w).sum() for o, w in zip(outs[:4], wts)) + (outs[4] * g_shs).sum()).backward()
    grads = [named[n].grad for n in PARAM_ORDER]
    _check_features(outs, grads, sub, g_shs, with_shs)
    worst, failures = st.check(z, cfg, t, _outs(outs), st.slice_grads(_named(grads), cfg, t))
    _record(worst, ("autograd", cfg, t, with_shs))
    _assert_ok(failures, ("autograd", cfg, t, with_shs))


# ------------------------------------------------------------------ 2. every gradient buffer fully written, nothing else touched
def _guarded(shape, fill):
    """A contiguous tensor of `shape` filled with `fill`, inside a larger buffer whose GUARD floats on either side hold SENTINEL."""
    n = int(np.prod(shape))
    n4 = (n + 3) // 4 * 4
    base = torch.full((GUARD + n4 + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    view = base[GUARD:GUARD + n].view(shape)
    view.fill_(fill)
    return base, view, n


def _guards_intact(base, n):
    return bool((base[:GUARD] == SENTINEL).all()) and bool((base[GUARD + n:] == SENTINEL).all())


@pytest.mark.parametrize("cfg,t", [("a", 0), ("a", 3), ("a", 137), ("a", 308), ("b", 0), ("b", 57)])
@pytest.mark.parametrize("sliced", [False, True])
def test_prefilled_gradient_buffers_are_fully_written_and_nothing_else(hip_lib, z, cfg, t, sliced):
    from ex4dgs_amd import attributes as A
    from ex4dgs_amd.attributes import PARAM_ORDER, SLICED_SHAPES, backward_raw
    # all dynamic rows but the last: with K = 35 an odd row count leaves the dense keyframe gradients a tail of 3 words behind their last
    # 16 bytes, which the clearing kernel writes separately, right in front of the guard
    rows = np.arange(z[f"{cfg}/family"].shape[0] - 1)
    params, wts, sub = _device_params(z, cfg, rows=rows)
    Ns, Nd = sub["_xyz"].shape[0], sub["_xyz_motion"].shape[0]
    scal = _scalars(cfg, t, Ns, Nd)
    g_shs = torch.randn(Ns + Nd, 16, 3, generator=torch.Generator().manual_seed(9)).to(DEV)
    if not sliced:
        # the forward entry point itself on NaN-prefilled, guarded outputs: every output entry written (no output of these rows is NaN)
        lib = A._lib()
        outs = [_guarded(s, float("nan")) for s in ((Ns + Nd, 3), (Ns + Nd, 4), (Ns + Nd, 1), (Ns + Nd, 3), (Ns + Nd, 16, 3))]
        rc = lib.ex4d_attributes_forward(C.byref(scal), *[A._ptr(p) for p in params], *[A._ptr(o[1]) for o in outs],
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, lib.ex4d_attributes_last_error().decode()
        torch.cuda.synchronize()
        for (base, view, count), ref in zip(outs, A.forward_raw(scal, params, with_shs=True)):
            assert _guards_intact(base, count) and not bool(torch.isnan(view).any()) and _same_bits(view, ref)
    results = []
    for fill in (float("nan"), SENTINEL):
        bufs = []
        for n, p in zip(PARAM_ORDER, params):
            shape = (p.shape[0],) + SLICED_SHAPES[n] if sliced and n in SLICED_SHAPES else tuple(p.shape)
            bufs.append(_guarded(shape, fill))
        got = backward_raw(scal, params, wts + [g_shs], with_shs=True, out=[b[1] for b in bufs], sliced=sliced)
        if sliced:
            got, hint = got
            assert hint == (scal.k - 1, 4, scal.k, 2)
        torch.cuda.synchronize()
        for n, (base, view, count), g in zip(PARAM_ORDER, bufs, got):
            assert g.data_ptr() == view.data_ptr() and _guards_intact(base, count), n
        results.append(_named(got))
    nan_run, sentinel_run = results
    for n in PARAM_ORDER:
        assert not (sentinel_run[n] == np.float32(SENTINEL)).any(), f"{n}: entries never written"
        assert np.array_equal(nan_run[n], sentinel_run[n], equal_nan=True), n           # the prefill never shows in a result
        if n != "_opacity_duration_var":
            assert not np.isnan(nan_run[n]).any(), f"{n}: entries never written"
    grads = sentinel_run if sliced else st.slice_grads(sentinel_run, cfg, t)           # dense: zero outside the 4 / 2 keyframes
    keep = np.concatenate([np.arange(Ns), Ns + rows])
    _assert_ok(st.check(z, cfg, t, {k: z[f"{cfg}/{st.tkey(t)}/{k}"][keep] for k in st.OUTPUTS}, grads, rows=rows)[1], ("prefilled", cfg, t, sliced))


# ------------------------------------------------------------------ 3. row counts around the 256-thread blocks
EDGES = (0, 1, 255, 256, 257, 511, 513)
SIZES = [(n, 0) for n in EDGES] + [(0, n) for n in EDGES[1:]] + [(257, 255), (1, 513), (511, 1)]


@pytest.mark.parametrize("Ns,Nd", SIZES)
@pytest.mark.parametrize("with_shs", [True, False])
def test_row_counts_around_the_block_size(hip_lib, z, Ns, Nd, with_shs):
    """Rows taken from the fixture by index (cyclically), so the expected values are the reference's; t = 3: delta = 0.5, the fallback rows."""
    from ex4dgs_amd.attributes import backward_raw, forward_raw
    cfg, t = "a", 3
    rows = np.arange(Nd) % z["a/family"].shape[0]
    static_rows = np.arange(Ns) % z["a/param/_xyz"].shape[0]
    params, wts, sub = _device_params(z, cfg, rows, static_rows)
    scal = _scalars(cfg, t, Ns, Nd)
    outs = forward_raw(scal, params, with_shs=with_shs)
    assert [tuple(o.shape) for o in outs[:4]] == [(Ns + Nd, 3), (Ns + Nd, 4), (Ns + Nd, 1), (Ns + Nd, 3)]
    g_shs = torch.randn(Ns + Nd, 16, 3, generator=torch.Generator().manual_seed(9)).to(DEV)
    dense = backward_raw(scal, params, wts + [g_shs], with_shs=with_shs)
    sliced, hint = backward_raw(scal, params, wts + [g_shs], with_shs=with_shs, sliced=True)
    for gout, grads in ((dense, st.slice_grads(_named(dense), cfg, t)), (sliced, _named(sliced))):
        _check_features(outs, gout, sub, g_shs, with_shs)
        worst, failures = st.check(z, cfg, t, _outs(outs), grads, rows=rows, static_rows=static_rows)
        _assert_ok(failures, (Ns, Nd, with_shs))
    _record(worst, ("sizes", Ns, Nd, with_shs))


# ------------------------------------------------------------------ 4. the feature copy beyond one trip of its grid-stride loop
@pytest.mark.parametrize("Ns,Nd", [(300_001, 100_003), (400_004, 0), (0, 400_004)])
def test_feature_gather_and_scatter_above_one_grid_trip(hip_lib, Ns, Nd):
    """features_kernel caps its grid at 16384 blocks of 256 threads, one float4 each: rows above 16384 * 256 / 12 = 349 525 are reached
    only by the second trip of its loop.  Bit for bit against torch.cat, and the split of dL/dshs bit for bit the other way."""
    from ex4dgs_amd.attributes import PARAM_ORDER, backward_raw, forward_raw, time_scalars
    assert (Ns + Nd) * 12 > 16384 * 256
    g = torch.Generator().manual_seed(Ns + 7)
    K = 4
    sub = dict(_xyz=torch.randn(Ns, 3, generator=g), _xyz_disp=torch.randn(Ns, 3, generator=g), _rotation=torch.randn(Ns, 4, generator=g),
               _opacity=torch.randn(Ns, 1, generator=g), _scaling=torch.randn(Ns, 3, generator=g) - 2,
               _xyz_motion=torch.randn(Nd, K, 3, generator=g), _rotation_motion=torch.randn(Nd, K, 4, generator=g), _opacity_motion=torch.randn(Nd, 1, generator=g),
               _opacity_duration_center=torch.rand(Nd, 2, 1, generator=g) * 3, _opacity_duration_var=torch.randn(Nd, 2, 1, generator=g),
               _scaling_motion=torch.randn(Nd, 3, generator=g) - 2)
    sub.update(_features(Ns, Nd, seed=Nd + 1))
    params = [sub[n].to(DEV).contiguous() for n in PARAM_ORDER]
    scal = time_scalars(3, Ns, Nd, K, 300, 10, 12, 3)
    assert scal.k == 1
    outs = forward_raw(scal, params, with_shs=True)
    g_shs = torch.randn(Ns + Nd, 16, 3, generator=g).to(DEV)
    for sliced in (False, True):
        gout = backward_raw(scal, params, [None, None, None, None, g_shs], with_shs=True, sliced=sliced)
        _check_features(outs, gout[0] if sliced else gout, sub, g_shs, True)
    # the per-Gaussian outputs of the last rows: the static rotation is a copy, the dynamic scale exp()
    if Ns:
        assert _same_bits(outs[1][:Ns].cpu(), sub["_rotation"])
    if Nd:
        assert float((outs[3][Ns:].cpu() - torch.exp(sub["_scaling_motion"])).abs().max()) <= 1e-6


# ------------------------------------------------------------------ 5. keyframe indices outside [1, K-3] are refused
@pytest.mark.parametrize("cfg", ["a", "b"])
@pytest.mark.parametrize("edge", ["below", "above"])
def test_keyframe_index_outside_the_range_is_refused_and_nothing_is_written(hip_lib, z, cfg, edge):
    from ex4dgs_amd import attributes as A
    params, wts, sub = _device_params(z, cfg)
    Ns, Nd = sub["_xyz"].shape[0], sub["_xyz_motion"].shape[0]
    K = st.CONFIGS[cfg]["K"]
    scal = _scalars(cfg, st.CONFIGS[cfg]["timestamps"][0], Ns, Nd)
    scal.k = 0 if edge == "below" else K - 2                  # k-1 = -1 / k+2 = K: one keyframe outside the tensor
    with pytest.raises(RuntimeError, match="keyframe index"):
        A.forward_raw(scal, params)
    # the forward entry point itself, with prefilled outputs
    lib = A._lib()
    N = Ns + Nd
    outs = [torch.full(s, SENTINEL, device=DEV) for s in ((N, 3), (N, 4), (N, 1), (N, 3), (N, 16, 3))]
    rc = lib.ex4d_attributes_forward(C.byref(scal), *[A._ptr(p) for p in params], *[A._ptr(o) for o in outs],
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc != 0 and b"keyframe index" in lib.ex4d_attributes_last_error()
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs)
    for sliced in (False, True):
        bufs = [torch.full((p.shape[0],) + A.SLICED_SHAPES[n] if sliced and n in A.SLICED_SHAPES else tuple(p.shape), SENTINEL, device=DEV)
                for n, p in zip(A.PARAM_ORDER, params)]
        with pytest.raises(RuntimeError, match="keyframe index"):
            A.backward_raw(scal, params, wts + [None], out=bufs, sliced=sliced)
        torch.cuda.synchronize()
        assert all(bool((b == SENTINEL).all()) for b in bufs)
    # the neighbours inside the range are accepted
    scal.k = 1 if edge == "below" else K - 3
    A.forward_raw(scal, params)


# ------------------------------------------------------------------ 6. states made by this repository's own density control
def test_states_made_by_densify_and_prune_match_the_oracle(hip_lib):
    """make_scene cfg3 at 200k rows, a third of the dynamic rows with all keyframe quaternions identical (as a Gaussian that has just turned
    dynamic), one densify_and_prune with fixed draws: the clone and split children get log-widths of exactly 2 and jittered, clamped
    centres.  HIP forward and backward on the new model against oracle/model_oracle.py at the bars of the 200k test of
    tests/test_gpu_parity.py (2e-6 relative forward, 2e-5 of the row's largest gradient backward)."""
    from oracle import model_oracle as mo
    from ex4dgs_amd.attributes import evaluate_attributes
    from ex4dgs_amd.scene import make_scene
    from ex4dgs_amd import densify
    from tests.test_gpu_densify import _random_stats, run_densify
    model, _, _ = make_scene("cfg3", P=200_000, device=DEV)
    with torch.no_grad():
        model._rotation_motion[::3] = model._rotation_motion[::3, :1] * 1.7
    nd_before = model.num_dynamic
    stats = densify.DensityStats(model)
    _random_stats(model, stats, torch.Generator().manual_seed(5))
    cfg = dict(max_grad=0.0002, max_dgrad=0.0002, min_opacity=0.01, min_motion_opacity=0.01, extent=5.0, max_screen_size=20,
               max_dynamic_screen_size=20, s_max_ssim=0.5, s_l1_thres=0.1, d_max_ssim=0.5, d_l1_thres=0.1, percent_dense=0.01)
    out = run_densify(model, stats, None, cfg, generator=torch.Generator(device=DEV).manual_seed(3))
    assert out["dynamic"]["clone"] > 100 and out["dynamic"]["split"] > 100 and out["static"]["clone"] > 100 and out["static"]["split"] > 100
    P = {n: getattr(model, n).detach().cpu().numpy() for n in model.PARAM_NAMES}
    c, v, q = P["_opacity_duration_center"][:, :, 0], P["_opacity_duration_var"][:, :, 0], P["_rotation_motion"]
    lo, hi = np.float32(13 / 10), np.float32(311 / 10)
    children = (v == 2).all(1)
    assert children.sum() > 200 and model.num_dynamic != nd_before
    assert ((c[children] == lo).any(1).sum() >= 8) and ((c[children] == hi).any(1).sum() >= 8)          # centres on either clamp bound
    assert (q == q[:, :1]).all(axis=(1, 2)).sum() > 1000                                                # identical keyframes survived
    worst = {}
    for t in (3, 137, 299):
        params = {n: getattr(model, n).detach().clone().requires_grad_(True) for n in model.PARAM_NAMES}
        outs = evaluate_attributes(params, t)
        ref = mo.forward(P, t)
        for o, k in zip(outs, ("means3D", "rotations", "opacities", "scales", "shs")):
            a, b = o.detach().cpu().numpy(), ref[k]
            err = np.abs(a - b).max() / max(1.0, np.abs(b).max())
            worst[k] = max(worst.get(k, 0.0), float(err))
            assert err <= 2e-6, (t, k, err)
        g = torch.Generator().manual_seed(3)
        wts = [torch.randn(o.shape, generator=g).to(DEV) for o in outs]
        sum((o * w).sum() for o, w in zip(outs, wts)).backward()
        gref = mo.backward(P, t, dict(zip(("means3D", "rotations", "opacities", "scales", "shs"), [w.cpu().numpy() for w in wts])))
        for n in model.PARAM_NAMES:
            a, b = params[n].grad.cpu().numpy(), gref[n]
            scale = np.maximum(np.abs(b).reshape(b.shape[0], -1).max(1), 1.0).reshape((-1,) + (1,) * (b.ndim - 1))
            err = float((np.abs(a - b) / scale).max())
            worst[n] = max(worst.get(n, 0.0), err)
            assert err <= 2e-5, (t, n, err)
    h.REPORT.append(dict(kind="attribute_states_densified", tag="fused attributes on a model after densify_and_prune (200k rows before), against model_oracle",
                         rows=int(model.num_static + model.num_dynamic), children=int(children.sum()), worst=worst))
