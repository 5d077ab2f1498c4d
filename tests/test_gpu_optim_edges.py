"""The fused RAdam steps (ex4dgs_amd/csrc/ex4d_optim.hip) against the numpy restatement oracle/optim_oracle.py BIT FOR BIT, on the
constructed cases of tests/optim_cases.py: the slot table of a dense launch (32 and 33 tensors, empty descriptors between live ones,
neighbours that differ in step, learning rate, rectification and nan_to_num), step counts up to 120 000, unaligned full chunks between
guard words, zeros / subnormals / overflow / inf / NaN, sliced and regularised launches of four tensors with every window class,
window positions outside [0, K) in device memory, and the regularised step at the two shapes that fill its staging LDS.

The file is built without contraction and every + - * / sqrt of the kernels is correctly rounded with denormals kept, so the bar is
equality of the uint32 views of p, exp_avg and exp_avg_sq; where the restatement is NaN the kernel must be NaN (sign and payload free:
x86 and the GPU make different default NaNs), and NaN may appear only at planted unsanitised gradient elements.  No element is left
out.  tests/test_cpu_optim_cases.py pins the restatement to torch in float64 and shows that no coefficient is a rounding accident."""
import numpy as np
import pytest
import torch

from oracle import optim_oracle as oo
from tests import helpers as h
from tests import optim_cases as oc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------ helpers
def dev(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


assert_bits = h.assert_same_bits


def assert_state(tag, got, want, may_be_nan=None):
    for name, g, w in zip(("p", "exp_avg", "exp_avg_sq"), got, want):
        assert_bits(g, w, may_be_nan, f"{tag} {name}")


def dense_item(t, bufs):
    p, g, m, v = bufs
    return (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), t["lr"], t["step"], t["nan_to_num"])


def run_dense(ts, betas=oc.BETAS, descriptors=None):
    """One call of the dense step over tensor dicts ts; returns the device buffers.  descriptors(items) -> the ctypes descriptors to
    launch instead of going through radam_step_raw."""
    from ex4dgs_amd import optim
    bufs = [tuple(dev(t[k]) for k in "pgmv") for t in ts]
    items = [dense_item(t, b) for t, b in zip(ts, bufs)]
    if descriptors is None:
        optim.radam_step_raw(items, betas, oc.EPS, DEV)
    else:
        optim._launch(descriptors(items), optim.Ex4dRadamTensor, "ex4d_radam_step", optim.MAX_TENSORS, betas, oc.EPS, DEV)
    torch.cuda.synchronize()
    return bufs


def check_dense(tag, ts, bufs):
    for i, (t, (p, g, m, v)) in enumerate(zip(ts, bufs)):
        assert_state(f"{tag} tensor {i} (numel {t['p'].size}, step {t['step']}, lr {t['lr']}, nan_to_num {t['nan_to_num']})", (p, m, v),
                     oc.expected_dense(t), oc.planted_mask(t))
        assert_bits(g, t["g"].copy(), np.isnan(t["g"]), f"{tag} tensor {i} gradient (read-only)")


# ------------------------------------------------------------------------------------------------------------------ dense: slot table
def test_constants_restate_the_library(hip_lib):
    from ex4dgs_amd import optim
    assert (optim.MAX_TENSORS, optim.MAX_SLICED, optim.MAX_WINDOWS) == (oc.MAX_TENSORS, oc.MAX_SLICED, oc.MAX_WINDOWS)
    assert (optim.REG_NONE, optim.REG_MOTION, optim.REG_ROT) == (oc.REG_NONE, oc.REG_MOTION, oc.REG_ROT)
    for (K, C), R in oc.REG_ROWS_TABLE.items():
        assert optim.sliced_reg_rows(K, C) == R == oc.reg_rows(K, C), (K, C)


@pytest.mark.parametrize("count", [oc.MAX_TENSORS, oc.MAX_TENSORS + 1])
def test_dense_slot_table(hip_lib, count):
    """32 tensors = one full launch, 33 = two launches: every slot takes its own step, learning rate, rectification and nan_to_num."""
    ts = oc.slot_tensors(count)
    check_dense(f"{count} tensors", ts, run_dense(ts))


def test_dense_slot_table_with_empty_descriptors(hip_lib):
    """numel == 0 descriptors with null pointers at positions 0, 5, 6 and last of a 32-descriptor call through the C ABI (radam_step_raw
    drops such items): the library compacts the slots, the live tensors take the step of their own descriptor."""
    from ex4dgs_amd import optim
    ts = oc.slot_tensors(oc.MAX_TENSORS - len(oc.ZERO_POSITIONS))

    def descriptors(items):
        live = iter(items)
        out = []
        for i in range(oc.MAX_TENSORS):
            if i in oc.ZERO_POSITIONS:
                out.append(optim.Ex4dRadamTensor(None, None, None, None, 0, 1e-3, 1, 1, 0))
            else:
                it = next(live)
                out.append(optim.Ex4dRadamTensor(*[int(x) for x in it[:5]], float(it[5]), int(it[6]), int(it[7]), 0))
        assert next(live, None) is None and len(out) == oc.MAX_TENSORS
        return out
    check_dense("empty descriptors", ts, run_dense(ts, descriptors=descriptors))


# ------------------------------------------------------------------------------------------------------------------ dense: trajectory
@pytest.mark.parametrize("betas", [oc.BETAS, oc.BETAS_B], ids=["b2=0.999", "b2=0.99"])
def test_step_trajectory(hip_lib, betas):
    """Steps 1..8 from zero state (both sides of the rho_t > 5 switch), then 29999, 30000, 30001 on seeded state: state carried forward
    on the device and in the restatement, compared after every step."""
    from ex4dgs_amd import optim
    for name, (p0, m0, v0, seq) in oc.trajectory(betas).items():
        p, m, v = dev(p0), dev(m0), dev(v0)
        rp, rm, rv = p0.copy(), m0.copy(), v0.copy()
        for step, lr, g in seq:
            gd = dev(g)
            optim.radam_step_raw([(p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, step)], betas, oc.EPS, DEV)
            torch.cuda.synchronize()
            oo.radam_step(rp, g, rm, rv, step, lr, betas[0], betas[1], oc.EPS)
            assert_state(f"{name} step {step} betas {betas}", (p, m, v), (rp, rm, rv))
        assert not np.array_equal(rp, p0)


# ------------------------------------------------------------------------------------------------------------------ dense: alignment and guards
@pytest.mark.parametrize("offsets", oc.ALIGN_OFFSETS, ids=lambda o: "".join(map(str, o)))
def test_alignment_and_guards(hip_lib, offsets):
    """p, g, m, v as views at float offsets into allocations filled with a guard pattern: a full chunk on the element-by-element path
    (numel 4096 from an unaligned pointer), 8192 + 5 and 3 elements in one launch.  The padding around p, m, v and the whole gradient
    allocation keep their bits."""
    from ex4dgs_amd import optim
    ts = oc.alignment_tensors()
    guard = np.array([oc.GUARD], np.uint32).view(np.int32)[0]
    allocs, items = [], []
    for t in ts:
        n = t["p"].size
        views = []
        for k, off in zip("pgmv", offsets):
            whole = torch.full((oc.ALIGN_FRONT + off + n + oc.ALIGN_BACK,), int(guard), dtype=torch.int32, device=DEV).view(torch.float32)
            assert whole.data_ptr() % 16 == 0
            view = whole[oc.ALIGN_FRONT + off:oc.ALIGN_FRONT + off + n]
            view.copy_(dev(t[k]))
            assert view.data_ptr() % 16 == 4 * off
            views.append((whole, view))
        allocs.append(views)
        items.append(tuple(v.data_ptr() for _, v in views) + (n, t["lr"], t["step"], 0))
    before_g = [views[1][0].clone() for views in allocs]
    optim.radam_step_raw(items, oc.BETAS, oc.EPS, DEV)
    torch.cuda.synchronize()
    for i, (t, views) in enumerate(zip(ts, allocs)):
        n = t["p"].size
        tag = f"offsets {offsets} numel {n}"
        assert_state(tag, [views[j][1] for j in (0, 2, 3)], oc.expected_dense(t))
        for j, off in ((0, offsets[0]), (2, offsets[2]), (3, offsets[3])):
            words = views[j][0].view(torch.int32).cpu().numpy().view(np.uint32)
            lo = oc.ALIGN_FRONT + off
            assert (words[:lo] == oc.GUARD).all() and (words[lo + n:] == oc.GUARD).all(), (tag, "pmv"[j - 1 if j else 0], "padding written")
        assert torch.equal(views[1][0].view(torch.int32), before_g[i].view(torch.int32)), (tag, "gradient allocation written")


# ------------------------------------------------------------------------------------------------------------------ dense: value edges
@pytest.mark.parametrize("step,flag", oc.EDGE_RUNS)
def test_value_edges(hip_lib, step, flag):
    """Zero state with zero gradient, subnormal g and v, sqrt(v) at eps, (w2 g) g finite at 1e37 and overflowing, +-inf and NaN with and
    without nan_to_num, |p| = 1e30 and 1e-30, exp_avg against the gradient's sign: an unrectified and a rectified step."""
    t = oc.edge_run(step, flag)
    (bufs,) = run_dense([t])
    check_dense(f"value edges step {step} nan_to_num {flag}", [t], [bufs])


# ------------------------------------------------------------------------------------------------------------------ FusedRAdam.step
def test_fused_radam_optimizer_over_forty_parameters(hip_lib):
    """FusedRAdam.step() over 40 small parameters (two launches) twice; parameters without a gradient keep their step count and bits."""
    from ex4dgs_amd.optim import FusedRAdam
    specs = oc.optimizer_params()
    params = [torch.nn.Parameter(dev(q["p"])) for q in specs]
    opt = FusedRAdam([{"params": [p], "lr": q["lr"]} for p, q in zip(params, specs)], lr=0.001)
    P = [q["p"].copy() for q in specs]
    M = [np.zeros_like(a) for a in P]; V = [np.zeros_like(a) for a in P]
    steps = [0] * len(specs)
    for s in range(2):
        for i, (p, q) in enumerate(zip(params, specs)):
            g = q["grads"][s]
            p.grad = None if g is None else dev(g)
            if g is not None:
                steps[i] += 1
                oo.radam_step(P[i], g, M[i], V[i], steps[i], q["lr"], *oc.BETAS, oc.EPS)
        opt.step()
        torch.cuda.synchronize()
        for i, p in enumerate(params):
            st = opt.state.get(p, {})
            assert float(st["step"]) == steps[i] if steps[i] else not st, i
            assert_bits(p, P[i], None, f"optimizer pass {s} parameter {i} (step {steps[i]})")
            if steps[i]:
                assert_bits(st["exp_avg"], M[i], None, f"optimizer pass {s} exp_avg {i}")
                assert_bits(st["exp_avg_sq"], V[i], None, f"optimizer pass {s} exp_avg_sq {i}")
    assert sorted(set(steps)) == [1, 2] and sum(q["grads"][0] is None for q in specs) > 2


# ------------------------------------------------------------------------------------------------------------------ sliced
def _range_view(full, t):
    rows, K, C = t["shape"]
    lo = t["row0"] * K * C
    return full.view(-1)[lo:lo + rows * K * C]


def run_sliced(ts, entry, first_dev=False):
    """One wrapper call (launches of <= 4 tensors) over sliced tensor dicts; entry: "sliced" or "reg" (REG_NONE unless a dict has a kind).
    first_dev: the window positions only in device memory.  Returns the device (p, m, v) of the FULL tensors."""
    from ex4dgs_amd import optim
    keep, items, bufs = [], [], []
    for t in ts:
        rows, K, C = t["shape"]
        full = tuple(dev(t[k]) for k in "pmv")
        bufs.append(full)
        blocks = {}
        wins = []
        for f, b in t["windows"]:
            blk = blocks.setdefault(id(b), dev(b) if rows else torch.zeros(1, device=DEV))
            wins.append(((None if first_dev else f), b.shape[1], blk.data_ptr()))
        fd = torch.tensor([f for f, _ in t["windows"]], dtype=torch.int32, device=DEV) if first_dev and t["windows"] else None
        keep += [blocks, fd]
        item = tuple(_range_view(x, t).data_ptr() if rows else x.data_ptr() for x in full) + (rows, K, C, t["lr"], t["step"], wins)
        if t["row0"] * K * C % 4:                                  # an offset row range: the pointers launched on are not 16-byte aligned
            assert all(ptr % 16 != 0 for ptr in item[:3]), (t["shape"], t["row0"])
        if entry == "reg":
            item += (fd.data_ptr() if fd is not None else None, t.get("kind", oc.REG_NONE), t.get("weight", 0.0), t.get("reg_rows", max(rows, 1)))
        elif fd is not None:
            item += (fd.data_ptr(),)
        items.append(item)
    (optim.radam_step_sliced_reg_raw if entry == "reg" else optim.radam_step_sliced_raw)(items, oc.BETAS, oc.EPS, DEV)
    torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("entry", ["sliced", "reg"])
@pytest.mark.parametrize("with_range", [False, True], ids=["whole", "row_range"])
def test_sliced_launches_of_four_tensors(hip_lib, entry, with_range):
    """Seven items (one without rows: 4 + 2 tensors per launch), each with its own step and learning rate: 8 windows with two identical,
    count == K, count == 1, first == 0, first == K - count, three overlapping, none.  Against the restatement on dense_from_windows; the
    same through ex4d_radam_step_sliced_reg with REG_NONE.  row_range: one tensor is rows [3, 643) of a [650, 7, 3] tensor (a base pointer
    that is not 16-byte aligned); the rows outside keep their bits."""
    ts = oc.sliced_tensors(with_range)
    assert any(t["row0"] * t["shape"][1] * t["shape"][2] % 4 for t in ts) == with_range        # run_sliced asserts the launched pointers
    for i, (t, got) in enumerate(zip(ts, run_sliced(ts, entry))):
        assert_state(f"{entry} tensor {i} {t['shape']} step {t['step']}", got, oc.expected_sliced(t))


@pytest.mark.parametrize("entry", ["sliced", "reg"])
def test_first_dev_positions_outside_the_keyframes(hip_lib, entry):
    """Window positions -count, -1, K - count + 1, K - 1 and K in device memory (the host would refuse them): the part of a window inside
    [0, K) counts, keyframe k takes slice k - first of the block -- the step on dense_from_windows, as include/ex4d_optim.h says."""
    ts = oc.outside_tensors()
    for i, (t, got) in enumerate(zip(ts, run_sliced(ts, entry, first_dev=True))):
        assert_state(f"{entry} first_dev tensor {i} {t['shape']}", got, oc.expected_sliced(t))


# ------------------------------------------------------------------------------------------------------------------ regularised step
def _dense_with_regulariser(t):
    """The dense gradient of the existing composition: windows scattered into zeros (restatement), then the library's
    regularizers.backward_raw(accumulate=True) over the full tensor (pinned to float64 by tests/test_gpu_regularizers.py), read back."""
    from ex4dgs_amd import regularizers as reg
    rows, K, C = t["shape"]
    dense = dev(oo.dense_from_windows(rows, K, C, t["windows"]))
    p = dev(t["p"])
    if t["kind"] == oc.REG_MOTION:
        reg.backward_raw(None, p, None, (0.0, t["weight"], 0.0), (None, dense, None), accumulate=True)
    elif t["kind"] == oc.REG_ROT:
        reg.backward_raw(None, None, p, (0.0, 0.0, t["weight"]), (None, None, dense), accumulate=True)
    torch.cuda.synchronize()
    return dense.cpu().numpy()


def _check_reg(tag, ts):
    grads = [_dense_with_regulariser(t) for t in ts]
    for i, (t, g, got) in enumerate(zip(ts, grads, run_sliced(ts, "reg"))):
        rows, K, C = t["shape"]
        if t["kind"] and K > 1:
            assert not np.array_equal(g, oo.dense_from_windows(rows, K, C, t["windows"])), (tag, i, "the regulariser added nothing")
        assert_state(f"{tag} tensor {i} {t['shape']} kind {t['kind']} windows {len(t['windows'])} step {t['step']}", got, oc.expected_sliced(t, grad=g))


@pytest.mark.parametrize("K,C,kind", oc.REG_LIMITS, ids=["motion_K341", "rot_K256"])
def test_regularised_step_at_the_staging_limit(hip_lib, K, C, kind):
    """K = 341 (motion, 32 736 bytes) and K = 256 (rotation, all 32 768 bytes of the staging LDS) with four rows per workgroup: rows
    1, 4, 5, 9 and 1 and 3 windows; one keyframe more is refused."""
    from ex4dgs_amd import optim
    for t in oc.reg_limit_cases():
        if t["shape"][1:] == (K, C):
            _check_reg("staging limit", [t])
    z = torch.zeros(4 * (K + 1) * C, device=DEV)
    with pytest.raises(RuntimeError, match="do not fit"):
        optim.radam_step_sliced_reg_raw([(z.data_ptr(), z.data_ptr(), z.data_ptr(), 4, K + 1, C, 1e-2, 1, [], None, kind, 1.0, 4)], oc.BETAS, oc.EPS, DEV)


def test_regularised_launch_of_four_tensors_with_their_own_rows_per_workgroup(hip_lib):
    """K in {341, 1, 35, 2}, both kinds and REG_NONE in one launch: each slot has its own rows per workgroup and its own offset of the
    gradient half of the LDS, the launch the LDS size of its largest member."""
    _check_reg("mixed launch", list(oc.reg_mixed_case()))
