"""The fused flow loss without a GPU (include/ex4d_loss.h "FLOW", ex4dgs_amd/flow.py): the float64 restatement of tests/flow_ref.py
against torch's float64 autograd of the written formula; the decode against what the reference's decode_flow returned
(tests/golden/flow_decode.npz, captured by tools/make_golden_flow_decode.py from the imported reference with a stub for cv2);
the refusals of the C entry points with their messages; the module on a machine without a device; the census of the case table."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from ex4dgs_amd import _abi, build, flow as xflow
from tests import flow_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "flow_decode.npz")


# ------------------------------------------------------------------ the restatement
def _torch_formula(flow, g, mask, acc, kind, eps):
    r = flow[:2] - g.permute(2, 0, 1)
    rho = r.abs().sum(0) if kind == "l1" else (r.pow(2).sum(0) + eps ** 2).sqrt()
    w = torch.ones_like(rho) if acc is None else acc
    m = mask > 0
    return torch.where(m, w * rho, torch.zeros_like(rho)).sum() / max(float(m.sum()), 1.0)


@pytest.mark.parametrize("use_acc", (False, True))
@pytest.mark.parametrize("kind", fr.KINDS)
@pytest.mark.parametrize("name", fr.CASES)
def test_the_restatement_is_torch_float64_autograd_of_the_written_formula(name, kind, use_acc):
    c = fr.case(name)
    loss, row, grad = fr.reference(name, kind, use_acc)
    g32, mask = fr.decode(c["codes"], c["scale"])
    flow = torch.tensor(c["flow"], dtype=torch.float64, requires_grad=True)
    acc = torch.tensor(c["acc"], dtype=torch.float64) if use_acc else None
    ref = _torch_formula(flow, torch.tensor(g32, dtype=torch.float64), torch.tensor(mask), acc, kind, fr.EPS)
    (ref * fr.GRAD_LOSS).backward()
    assert abs(loss - float(ref.detach())) <= 1e-13 * max(1.0, abs(float(ref.detach()))) and row[0] == loss
    assert row[1] == float((c["codes"][..., 2] > 32768).sum()) and row[3] == 0.0
    assert np.abs(grad - flow.grad.numpy()).max() <= 1e-13 * max(1.0, np.abs(grad).max())
    assert not grad[fr.exact_zero_mask(name)].any() and not flow.grad.numpy()[fr.exact_zero_mask(name)].any()
    if name == fr.ALL_INVALID:
        assert loss == 0.0 and not row.any() and not grad.any()
    else:
        assert loss > 0 and row[2] > 0 and np.abs(grad[:2]).max() > 0


def test_the_case_table_census():
    """From the codes, on the host: every random frame has at least half of its pixels valid (about 70 % are drawn valid); the one
    all-invalid frame is the designed one; the designed frames hold the designed codes, validity words on both sides of the threshold,
    pixels with r = 0 exactly and a pixel with acc = 0; the three flow scales are used."""
    for name in fr.RANDOM:
        c = fr.case(name)
        valid = c["codes"][..., 2] > 32768
        assert valid.sum() * 2 >= valid.size, (name, int(valid.sum()), valid.size)
        assert c["flow"].shape == (3, c["H"], c["W"]) and c["codes"].shape == (c["H"], c["W"], 3) and c["codes"].dtype == np.uint16
    assert not (fr.case(fr.ALL_INVALID)["codes"][..., 2] > 32768).any()
    assert {fr.case(n)["scale"] for n in fr.DESIGNED} == {1.0, 0.5, 0.3} and {fr.case(n)["scale"] for n in fr.RANDOM} == {1.0, 0.5, 0.3}
    assert not any(math.log2(s).is_integer() for s in (0.3,))
    for name in fr.DESIGNED:
        c = fr.case(name)
        flat = c["codes"].reshape(-1, 3)
        for code in (0, 32768, 65535):
            assert (flat[:, 0] == code).any() and (flat[:, 1] == code).any()
        assert (flat[:, 2] == 32768).any() and (flat[:, 2] == 32769).any()
        g, mask = fr.decode(c["codes"], c["scale"])
        for p in fr.DESIGNED_R0:
            y, x = divmod(p, c["W"])
            assert mask[y, x] == 1 and c["flow"][0, y, x] == g[y, x, 0] and c["flow"][1, y, x] == g[y, x, 1]
        y, x = divmod(fr.DESIGNED_ACC0, c["W"])
        assert mask[y, x] == 1 and c["acc"][y, x] == 0 and c["flow"][0, y, x] != g[y, x, 0]
    shapes = {(H, W) for _, H, W in fr.SHAPES}
    assert {(1, 1), (1, fr.WG - 1), (1, fr.WG), (1, fr.WG + 1)} <= shapes and any(W == 1 and H > 1 for H, W in shapes)
    assert max(fr.blocks(H, W) for H, W in shapes) > fr.FOLD


# ------------------------------------------------------------------ the decode
def test_decode_flow_gives_the_references_bits():
    with np.load(GOLDEN) as z:
        codes, flow, mask = z["codes"], z["flow"], z["mask"]
    assert codes.dtype == np.uint16 and flow.dtype == np.float32 and mask.dtype == np.float32
    assert {tuple(int(v) for v in c) for c in fr.DESIGNED_CODES} <= {tuple(int(v) for v in c) for c in codes.reshape(-1, 3)}
    assert {32767, 32768, 32769} <= set(int(v) for v in codes[..., 2].ravel())
    mine, mine_mask = fr.decode(codes, 1.0)
    assert np.array_equal(mine.view(np.int32), flow.view(np.int32)) and np.array_equal(mine_mask, mask)
    for enc in (torch.from_numpy(codes.view(np.int16)), torch.from_numpy(codes.view(np.int16)).view(torch.uint16)):
        f, m = xflow.decode_flow(enc)
        assert f.dtype == torch.float32 and m.dtype == torch.float32 and tuple(f.shape) == flow.shape and tuple(m.shape) == mask.shape
        assert np.array_equal(f.numpy().view(np.int32), flow.view(np.int32)) and np.array_equal(m.numpy(), mask)
        for scale in fr.SCALES:
            scaled = flow * scale                              # read_opticalflow: a float32 array times a Python float
            assert scaled.dtype == np.float32
            f, _ = xflow.decode_flow(enc, scale)
            assert np.array_equal(f.numpy().view(np.int32), scaled.view(np.int32)), scale
            assert np.array_equal(fr.decode(codes, scale)[0].view(np.int32), scaled.view(np.int32))
    # a fourth word changes nothing
    four = torch.from_numpy(fr.with_stride(codes, 4).view(np.int16))
    assert torch.equal(xflow.decode_flow(four)[0], xflow.decode_flow(torch.from_numpy(codes.view(np.int16)))[0])


# ------------------------------------------------------------------ the C entry points: constants, scratch, refusals
def _defines():
    text = open(os.path.join(ROOT, "include", "ex4d_loss.h")).read()
    return {n: int(v) for n, v in re.findall(r"^#define[ \t]+(EX4D_FLOW_\w+)[ \t]+(\d+)[ \t]*$", text, flags=re.M)}


def test_the_modules_constants_are_the_headers_and_the_source_is_built_without_contraction():
    d = _defines()
    assert (d["EX4D_FLOW_PIXELS_PER_LANE"], d["EX4D_FLOW_THREADS"], d["EX4D_FLOW_FOLD"]) == (xflow.PIXELS_PER_LANE, xflow.THREADS, xflow.FOLD)
    assert xflow.KINDS == {"l1": d["EX4D_FLOW_L1"], "charbonnier": d["EX4D_FLOW_CHARBONNIER"]}
    assert "-ffp-contract=off" in build.SOURCES["ex4d_flow.hip"]
    lib = _abi.load()
    q = lib.ex4d_flow_loss_scratch_floats
    assert q(0, 5) == 0 and q(5, 0) == 0 and q(-1, -1) == 0
    for _, H, W in fr.SHAPES:
        assert q(H, W) >= 4 * fr.blocks(H, W)
    assert q(1352, 1014) >= 4 * fr.blocks(1352, 1014)


FAKE = 0x1000                    # never dereferenced: every call below is refused before any launch
FWD = dict(H=4, W=5, flow=FAKE, gt=FAKE, S=3, scale=1.0, acc=None, kind=1, eps=1e-3, loss=FAKE, row=FAKE, scratch=FAKE)
BWD = dict(H=4, W=5, flow=FAKE, gt=FAKE, S=3, scale=1.0, acc=None, kind=1, eps=1e-3, row=FAKE, grad_loss=FAKE, grad_flow=FAKE)
REFUSALS = [
    (dict(H=0), "H and W must be positive"), (dict(W=0), "H and W must be positive"), (dict(H=-3), "H and W must be positive"),
    (dict(S=2), "pixel_stride 2"), (dict(S=5), "pixel_stride 5"), (dict(S=6), "pixel_stride 6"),
    (dict(kind=2), "kind 2"), (dict(kind=-1), "kind -1"),
    (dict(eps=0.0), "eps"), (dict(eps=-1e-3), "eps"), (dict(eps=float("nan")), "eps"), (dict(eps=float("inf")), "eps"),
    (dict(flow=None), "flow is NULL"), (dict(gt=None), "gt is NULL"),
]
FWD_ONLY = [(dict(loss=None), "loss is NULL"), (dict(row=None), "row is NULL"), (dict(scratch=None), "scratch is NULL")]
BWD_ONLY = [(dict(row=None), "row is NULL"), (dict(grad_loss=None), "grad_loss is NULL"), (dict(grad_flow=None), "grad_flow is NULL")]


@pytest.mark.parametrize("entry,base,cases", [("ex4d_flow_loss_forward", FWD, REFUSALS + FWD_ONLY), ("ex4d_flow_loss_backward", BWD, REFUSALS + BWD_ONLY)])
def test_refusals_carry_their_message(entry, base, cases):
    lib = _abi.load()
    for change, text in cases:
        args = list(dict(base, **change).values()) + [None]
        with pytest.raises(RuntimeError) as e:
            _abi.call(entry, *args)
        assert str(e.value) == lib.ex4d_loss_last_error().decode() and text in str(e.value), (change, str(e.value))
        assert getattr(lib, entry)(*args) != 0


# ------------------------------------------------------------------ the module without a device
def test_the_module_without_a_device():
    c = fr.case("odd_small")
    flow, enc = torch.tensor(c["flow"]), fr.encoded(c["codes"])
    for call in (lambda: xflow.flow_loss(flow, enc), lambda: xflow.flow_loss_raw(flow, enc), lambda: xflow.flow_metrics(flow, enc),
                 lambda: xflow.flow_loss_backward_raw(flow, enc, torch.zeros(4, dtype=torch.float64), torch.ones(1))):
        with pytest.raises(RuntimeError, match="only run on a ROCm GPU"):
            call()
    with pytest.raises(ValueError, match="unknown kind"):
        xflow.flow_loss(flow, enc, kind="huber")
    with pytest.raises(RuntimeError, match="uint16 or torch.int16"):
        xflow.decode_flow(torch.zeros(2, 2, 3, dtype=torch.int32))
    assert {"ex4d_flow_loss_scratch_floats", "ex4d_flow_loss_forward", "ex4d_flow_loss_backward"} <= set(_abi.exports("ex4d_loss.h"))


def test_frame_trainer_step_takes_flow_to_and_defaults_to_none():
    from ex4dgs_amd.trainer import FrameTrainer
    assert inspect.signature(FrameTrainer.step).parameters["flow_to"].default is None
