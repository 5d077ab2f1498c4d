"""The fused L1 + SSIM loss (ex4dgs_amd/csrc/ex4d_loss.hip) at every edge of its rolling-window tiling (run with `-m gpu`).

1. Oracle sweep (tests/loss_cases.py): strip widths around 64 / 74 / 128 / 138, segment heights around 48 / 96 with last segments
   of 1 .. 11 rows and every phase of the four-rows-per-iteration walk, channel counts around the groups of three, work-item counts
   with and without padded workgroups -- against the float64 oracle at the bars of non-flat input, nothing left unwritten.
2. Placement invariance, bit for bit: the zero padding is zeros fed through the same taps in the same order, so an image pair
   embedded in an all-zero canvas gives, inside its rectangle, exactly the error maps (and derivative maps, and -- with the
   upstream gradient scaled by the pixel-count ratio, a power of two -- the image gradient) of the plain call, whatever strip
   column, ring slot, segment, halo role or workgroup each pixel lands in.  No tolerance, so it also holds the flat,
   ill-conditioned images (where the oracle bar is 5e-4) to the last bit at every seam.
3. The hook views of `acc=`, the metric functions, strided inputs, argument checks, null error maps, run-to-run identity.

Value-only mutants of the kernels this module fails on and the loss tests of tests/test_gpu_parity.py pass: a later channel group
that overwrites the SSIM map instead of accumulating in every segment but the first (sweep C >= 4 at 49x65 / 97x129, forward placement
C = 4); a per-XCD share of work items that is wrong when their count is a multiple of 8 (sweep 3x49x256: unwritten elements); the
backward's halo columns 2e-5 too bright (backward placement, sweep)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import helpers as h
from tests import loss_cases as lc

pytestmark = pytest.mark.gpu

EX4D_OK, EX4D_ERR_ARG = 0, 1
NAN = float("nan")


# ------------------------------------------------------------------ the C ABI of include/ex4d_loss.h, every buffer the caller's
def _filled(shape, value):
    return torch.full(shape, value, dtype=torch.float32, device="cuda")


def raw_forward(x, y, lam, l1=True, ss=True):
    """ex4d_l1_ssim_forward on contiguous [C,H,W] CUDA tensors; every output buffer is NaN before the call."""
    from ex4dgs_amd import loss as L
    lib = L._lib()
    Cn, H, W = x.shape
    assert x.is_contiguous() and y.is_contiguous() and x.shape == y.shape
    out = dict(loss=_filled((1,), NAN), l1_errors=_filled((H, W), NAN) if l1 else None, ssim_errors=_filled((H, W), NAN) if ss else None,
               dmaps=_filled((3, Cn, H, W), NAN))
    scratch = _filled((lib.ex4d_l1_ssim_scratch_floats(H, W),), NAN)
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = lib.ex4d_l1_ssim_forward(Cn, H, W, x.data_ptr(), y.data_ptr(), float(lam), L._WINDOW.ctypes.data, out["loss"].data_ptr(),
                                  ptr(out["l1_errors"]), ptr(out["ssim_errors"]), out["dmaps"].data_ptr(), scratch.data_ptr(),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == EX4D_OK, lib.ex4d_loss_last_error().decode()
    torch.cuda.synchronize()
    return out


def raw_backward(x, y, lam, dmaps, grad_loss):
    """ex4d_l1_ssim_backward with `dmaps` as given; the gradient buffer is NaN before the call."""
    from ex4dgs_amd import loss as L
    lib = L._lib()
    Cn, H, W = x.shape
    assert x.is_contiguous() and y.is_contiguous() and dmaps.is_contiguous() and dmaps.shape == (3, Cn, H, W)
    grad = _filled((Cn, H, W), NAN)
    gl = _filled((1,), float(grad_loss))
    rc = lib.ex4d_l1_ssim_backward(Cn, H, W, x.data_ptr(), y.data_ptr(), float(lam), L._WINDOW.ctypes.data, dmaps.data_ptr(),
                                   gl.data_ptr(), grad.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == EX4D_OK, lib.ex4d_loss_last_error().decode()
    torch.cuda.synchronize()
    return grad


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


# ------------------------------------------------------------------ 1. oracle sweep over the tiling edges
_WORST = dict(kind="loss_edges", tag="fused L1+SSIM, tiling-edge sweep against the float64 oracle (worst over the cases run)", cases=0,
              loss=0.0, l1_errors=0.0, ssim_errors=0.0, grad_over_gmax=0.0, grad_over_bar=0.0, at={})


def _record(e, what):
    if _WORST["cases"] == 0:
        h.REPORT.append(_WORST)
    _WORST["cases"] += 1
    rel = e["grad"] / e["gmax"] if e["gmax"] > 1e-3 else 0.0
    for k, v in (("loss", e["loss"]), ("l1_errors", e["l1_errors"]), ("ssim_errors", e["ssim_errors"]), ("grad_over_gmax", rel),
                 ("grad_over_bar", e["grad"] / e["grad_bar"])):
        if v > _WORST[k]:
            _WORST[k], _WORST["at"][k] = float(v), str(what)


@pytest.mark.parametrize("shape", lc.sweep_shapes(), ids=lambda s: "x".join(map(str, s)))
def test_edge_sweep_vs_oracle(hip_lib, shape):
    from oracle import loss_oracle
    from ex4dgs_amd.loss import l1_ssim_loss
    image, gt = lc.make_pair(shape)
    y = torch.tensor(gt, device="cuda")
    for lam in lc.LAMBDAS:
        x = torch.tensor(image, device="cuda", requires_grad=True)
        loss, l1e, sse = l1_ssim_loss(x, y, lam)
        assert not l1e.requires_grad and not sse.requires_grad and loss.shape == () and l1e.shape == sse.shape == shape[1:]
        (loss * 1.0).backward()
        got = dict(loss=loss.item(), l1_errors=l1e.cpu().numpy(), ssim_errors=sse.cpu().numpy(), grad=x.grad.cpu().numpy())
        # nothing left unwritten: the same call into buffers that hold NaN, which then hold exactly what the autograd surface returned
        raw = raw_forward(x.detach(), y, lam)
        grad = raw_backward(x.detach(), y, lam, raw["dmaps"], 1.0)
        for k, t in list(raw.items()) + [("grad", grad)]:
            assert bool(torch.isfinite(t).all()), (shape, lam, k, "elements left unwritten:", int((~torch.isfinite(t)).sum()))
        assert same_bits(raw["loss"].reshape(()), loss.detach()) and same_bits(raw["l1_errors"], l1e) and same_bits(raw["ssim_errors"], sse)
        assert same_bits(grad, x.grad)
        for k in ("l1_errors", "ssim_errors", "grad"):
            assert np.isfinite(got[k]).all(), (shape, lam, k)
        e = lc.errors(got, loss_oracle.l1_ssim(image, gt, lam))
        print(f"loss edges {shape} lam={lam}: loss {e['loss']:.2e} l1 {e['l1_errors']:.2e} ssim {e['ssim_errors']:.2e} "
              f"grad {e['grad']:.2e} (bar {e['grad_bar']:.2e})")
        _record(e, (shape, lam))
        lc.assert_within_bars(e, what=(shape, lam))


# ------------------------------------------------------------------ 2. placement invariance, bit for bit
PH, PW = 60, 80                                     # the embedded pair; canvas 2 PH x 2 PW = 120 x 160: three strips, three segments
OFF_Y = (0, 1, 3, 5, 37, 38, 43, 47, 48, 49)       # rows: window clipped / not clipped above, every ring phase, both sides of a segment seam
OFF_X = (0, 1, 5, 53, 54, 58, 59, 63, 64, 65)      # columns: right edge at 133 .. 145 and left edge at 0 .. 65 cross the halo and strip seams
OFFSETS = [(dy, dx) for dy in OFF_Y for dx in OFF_X]


def _render_crop():
    """A PH x PW crop of an actual render that is part flat background (image == background colour: sigma = 0, the ill-conditioned
    SSIM case) and part content, and a ground truth for it that keeps the background flat."""
    from ex4dgs_amd.scene import make_scene
    from ex4dgs_amd.render import render
    model, cam, bg = make_scene("cfg2", P=2000, device="cuda")       # sparse enough to leave ~45 % of the frame untouched
    with torch.no_grad():
        out = render(cam, model, None, bg, timestamp=0, near=4.0, far=300.0)
    image, acc = out["render"].detach(), out["acc"].detach()[0]
    empty = (acc == 0).float()[None, None]
    frac = torch.nn.functional.avg_pool2d(empty, (PH, PW), stride=(12, 16))[0, 0]          # background share of every candidate crop
    i = int(torch.argmin((frac - 0.5).abs()))
    y0, x0 = 12 * (i // frac.shape[1]), 16 * (i % frac.shape[1])
    share = float(frac.flatten()[i])
    assert 0.15 <= share <= 0.85, f"no crop of the render is part background, part content (best share {share})"
    print(f"render crop at ({y0}, {x0}): background share {share:.2f}")
    crop = image[:, y0:y0 + PH, x0:x0 + PW].contiguous()
    g = torch.Generator(device="cpu").manual_seed(5)
    gt = (crop * 0.9 + 0.05 * torch.rand(crop.shape, generator=g).to(crop.device) * (acc[y0:y0 + PH, x0:x0 + PW] > 0)).clamp(0, 1)
    return crop.cpu().numpy(), gt.cpu().numpy()


def _placement_pair(name, Cn):
    if name == "noise":
        image, gt = lc.make_pair((3, PH, PW))
    elif name == "smooth":                          # the golden's 48 x 40 smooth pair, mirrored outwards to PH x PW (stays smooth)
        g = np.load(os.path.join(h.ROOT, "tests", "golden", "loss_l1_ssim.npz"))
        pad = ((0, 0), ((PH - 48) // 2,) * 2, ((PW - 40) // 2,) * 2)
        image, gt = np.pad(g["smooth/image"], pad, mode="symmetric"), np.pad(g["smooth/gt"], pad, mode="symmetric")
    else:
        image, gt = _render_crop()
    assert image.shape == gt.shape == (3, PH, PW)
    if Cn == 4:                                     # a second channel group: channel 1 turned by 180 degrees
        image, gt = (np.concatenate([a, a[1:2, ::-1, ::-1]]) for a in (image, gt))
    return (torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda") for a in (image, gt))


def _embed(t, H, W, dy, dx):
    out = torch.zeros(t.shape[:-2] + (H, W), dtype=torch.float32, device="cuda")
    out[..., dy:dy + PH, dx:dx + PW] = t
    return out


def _mismatch(a, b):
    return int((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).sum())


@pytest.mark.parametrize("Cn", [3, 4])
@pytest.mark.parametrize("name", ["noise", "smooth", "render"])
def test_forward_is_placement_invariant_bit_for_bit(hip_lib, name, Cn):
    x, y = _placement_pair(name, Cn)
    plain = raw_forward(x, y, 0.2)
    H, W = 2 * PH, 2 * PW
    bad = []
    for dy, dx in OFFSETS:
        big = raw_forward(_embed(x, H, W, dy, dx), _embed(y, H, W, dy, dx), 0.2)
        inside = (Ellipsis, slice(dy, dy + PH), slice(dx, dx + PW))
        n = {k: _mismatch(big[k][inside], plain[k]) for k in ("l1_errors", "ssim_errors", "dmaps")}
        outside = big["l1_errors"].clone()
        outside[inside] = 0
        n["l1_errors outside the rectangle"] = int((outside != 0).sum())
        n["not finite"] = sum(int((~torch.isfinite(big[k])).sum()) for k in ("loss", "l1_errors", "ssim_errors", "dmaps"))
        if any(n.values()):
            bad.append(((dy, dx), n))
    assert not bad, f"{name} C={Cn}: elements that differ from the plain {PH}x{PW} call, per offset (dy, dx): {bad}"


@pytest.mark.parametrize("Cn", [3, 4])
@pytest.mark.parametrize("name", ["noise", "smooth", "render"])
def test_backward_is_placement_invariant_bit_for_bit(hip_lib, name, Cn):
    """Canvas of exactly 2h x 2w and grad_loss = 4: inv_count is exactly a quarter of the plain call's, every product scales by a
    power of two, so the gradient inside the rectangle is the plain call's with grad_loss = 1 to the bit."""
    x, y = _placement_pair(name, Cn)
    lam = 0.2
    dmaps = raw_forward(x, y, lam)["dmaps"]
    plain = raw_backward(x, y, lam, dmaps, 1.0)
    assert float(plain.abs().max()) > 0
    H, W = 2 * PH, 2 * PW
    bad = []
    for dy, dx in OFFSETS:
        big = raw_backward(_embed(x, H, W, dy, dx), _embed(y, H, W, dy, dx), lam, _embed(dmaps, H, W, dy, dx), 4.0)
        n = _mismatch(big[:, dy:dy + PH, dx:dx + PW], plain) + int((~torch.isfinite(big)).sum())
        if n:
            bad.append(((dy, dx), n))
    assert not bad, f"{name} C={Cn}: gradient elements that differ from the plain {PH}x{PW} call, per offset (dy, dx): {bad}"


# ------------------------------------------------------------------ 3. small things that belong with it
EDGE = (4, 106, 70)                                 # two channel groups, three segments (the last of 10 rows), a second strip of 6 columns


def test_acc_hook_views_hold_the_maps_of_the_plain_call(hip_lib):
    from ex4dgs_amd.loss import l1_ssim_loss
    image, gt = lc.make_pair(EDGE)
    x, y = torch.tensor(image, device="cuda", requires_grad=True), torch.tensor(gt, device="cuda")
    acc = torch.rand(1, *EDGE[1:], device="cuda", requires_grad=True)
    loss0, l1e0, sse0 = l1_ssim_loss(x, y, 0.2)
    loss0.backward()
    g0, x.grad = x.grad.clone(), None
    junk = [torch.full((3,) + EDGE[1:], NAN, device="cuda") for _ in range(4)]    # what the allocator hands out next holds NaN
    del junk
    loss, l1e, sse, hook = l1_ssim_loss(x, y, 0.2, acc=acc)
    loss.backward()
    assert hook.shape == (3,) + EDGE[1:] and not hook.requires_grad
    assert same_bits(hook[0], acc.detach()[0]) and same_bits(hook[1], l1e0) and same_bits(hook[2], sse0)
    assert l1e.data_ptr() == hook[1].data_ptr() and sse.data_ptr() == hook[2].data_ptr()       # views, not copies
    assert same_bits(l1e, l1e0) and same_bits(sse, sse0) and same_bits(loss.detach(), loss0.detach()) and same_bits(x.grad, g0)


def test_metric_functions_vs_oracle(hip_lib):
    """ssim / l1_loss / psnr under the reference's names.  Bars: the per-channel SSIM map at the bar of the channel-mean map (1e-5; the
    float32 reference is within 5e-6 of float64 per channel on this input); scalar means at the loss bar 1e-6; PSNR to 1e-4 dB (a float32
    mean of 3e4 squares is good to ~1e-5 relative at worst, and d(dB) = 10 / ln 10 * d(mse) / mse < 5e-5 dB)."""
    from oracle import loss_oracle
    from ex4dgs_amd.loss import ssim, l1_loss, psnr
    shape = (4, 53, 70)
    image, gt = lc.make_pair(shape)
    o = loss_oracle.l1_ssim(image, gt, 1.0)          # lambda = 1: loss = 1 - mean(ssim_map)
    x, y = torch.tensor(image, device="cuda", requires_grad=True), torch.tensor(gt, device="cuda")
    m = ssim(x, y, reduce=False)
    assert m.shape == shape and not m.requires_grad
    np.testing.assert_allclose(m.cpu().numpy(), o["ssim_map"], rtol=0, atol=lc.TOL_SSIM)
    m4 = ssim(x[None], y[None], reduce=False)
    assert m4.shape == (1,) + shape and same_bits(m4[0], m)
    s = ssim(x, y)
    assert abs(s.item() - o["ssim_map"].mean()) < lc.TOL_LOSS
    s.backward()
    gmax = np.abs(o["grad"]).max()
    np.testing.assert_allclose(x.grad.cpu().numpy(), -o["grad"], rtol=0, atol=lc.TOL_GRAD_REL * gmax + lc.TOL_GRAD_ABS)
    assert same_bits(ssim(x[None], y[None]).detach(), s.detach())
    d = image.astype(np.float64) - gt.astype(np.float64)
    assert abs(l1_loss(x, y).item() - np.abs(d).mean()) < lc.TOL_LOSS
    mask = torch.tensor(gt[0] > 0.5, device="cuda")
    assert abs(l1_loss(x, y, mask=mask[None].expand(shape)).item() - np.abs(d)[:, gt[0] > 0.5].mean()) < lc.TOL_LOSS
    p = psnr(x[None], y[None])
    assert p.shape == (1, 1) and abs(p.item() - 20 * np.log10(1.0 / np.sqrt((d ** 2).mean()))) < 1e-4


@pytest.mark.parametrize("view", ["transposed", "channel_step", "channel_range", "row_step"])
def test_strided_inputs_give_the_result_of_their_contiguous_copies(hip_lib, view):
    from ex4dgs_amd.loss import l1_ssim_loss
    Cn, H, W = 3, 53, 70
    take = {"transposed": ((Cn, W, H), lambda t: t.transpose(1, 2)), "channel_step": ((2 * Cn, H, W), lambda t: t[::2]),
            "channel_range": ((Cn + 2, H, W), lambda t: t[1:1 + Cn]), "row_step": ((Cn, 2 * H, W), lambda t: t[:, ::2])}[view]
    img_base, gt_base = lc.make_pair(take[0])
    xb, yb = torch.tensor(img_base, device="cuda", requires_grad=True), torch.tensor(gt_base, device="cuda")
    xv, yv = take[1](xb), take[1](yb)
    assert xv.shape == (Cn, H, W) and (view == "channel_range" or not xv.is_contiguous())
    loss, l1e, sse = l1_ssim_loss(xv, yv, 0.2)
    (2.0 * loss).backward()
    xc = xv.detach().contiguous().requires_grad_(True)
    loss_c, l1e_c, sse_c = l1_ssim_loss(xc, yv.contiguous(), 0.2)
    (2.0 * loss_c).backward()
    assert same_bits(loss.detach(), loss_c.detach()) and same_bits(l1e, l1e_c) and same_bits(sse, sse_c)
    assert same_bits(take[1](xb.grad), xc.grad)
    untouched = torch.ones_like(xb, dtype=torch.bool)
    take[1](untouched)[...] = False
    assert float(xb.grad[untouched].abs().sum()) == 0                  # nothing leaks into the elements the view skips


def test_c_abi_refuses_bad_arguments_with_a_message(hip_lib):
    from ex4dgs_amd import loss as L
    lib = L._lib()
    Cn, H, W = 3, 8, 8
    t = lambda *s: torch.zeros(*s, device="cuda")
    x, y, loss, l1e, sse, dm, grad, gl = t(Cn, H, W), t(Cn, H, W), t(1), t(H, W), t(H, W), t(3, Cn, H, W), t(Cn, H, W), t(1)
    scratch = t(lib.ex4d_l1_ssim_scratch_floats(H, W))
    win = L._WINDOW.ctypes.data
    fwd = [Cn, H, W, x.data_ptr(), y.data_ptr(), 0.2, win, loss.data_ptr(), l1e.data_ptr(), sse.data_ptr(), dm.data_ptr(), scratch.data_ptr(), None]
    bwd = [Cn, H, W, x.data_ptr(), y.data_ptr(), 0.2, win, dm.data_ptr(), gl.data_ptr(), grad.data_ptr(), None]

    def refused(fn, args, i, v):
        a = list(args)
        a[i] = v
        rc = fn(*a)
        msg = lib.ex4d_loss_last_error().decode()
        assert rc == EX4D_ERR_ARG and msg, (fn.__name__, i, v, rc, msg)

    assert lib.ex4d_l1_ssim_forward(*fwd) == EX4D_OK and lib.ex4d_loss_last_error().decode() == ""
    assert lib.ex4d_l1_ssim_backward(*bwd) == EX4D_OK and lib.ex4d_loss_last_error().decode() == ""
    for i in (0, 1, 2):
        for v in (0, -1):
            refused(lib.ex4d_l1_ssim_forward, fwd, i, v)
            refused(lib.ex4d_l1_ssim_backward, bwd, i, v)
    for i in (3, 4, 6, 7, 10, 11):                  # img, gt, window, loss, dmaps, scratch
        refused(lib.ex4d_l1_ssim_forward, fwd, i, None)
    for i in (3, 4, 6, 7, 8, 9):                    # img, gt, window, dmaps, grad_loss, grad_img
        refused(lib.ex4d_l1_ssim_backward, bwd, i, None)
    assert lib.ex4d_l1_ssim_forward(*fwd) == EX4D_OK and lib.ex4d_loss_last_error().decode() == ""     # a good call clears the message
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", [EDGE, (3, 49, 65)])
def test_null_error_maps_change_nothing_else(hip_lib, shape):
    image, gt = lc.make_pair(shape)
    x, y = torch.tensor(image, device="cuda"), torch.tensor(gt, device="cuda")
    full = raw_forward(x, y, 0.2)
    for l1, ss in ((False, True), (True, False), (False, False)):
        part = raw_forward(x, y, 0.2, l1=l1, ss=ss)
        assert same_bits(part["loss"], full["loss"]) and same_bits(part["dmaps"], full["dmaps"])
        assert part["l1_errors"] is None or same_bits(part["l1_errors"], full["l1_errors"])
        assert part["ssim_errors"] is None or same_bits(part["ssim_errors"], full["ssim_errors"])


@pytest.mark.parametrize("shape", [EDGE, (3, 100, 190), (5, 97, 129)])
def test_two_calls_are_bit_identical(hip_lib, shape):
    image, gt = lc.make_pair(shape)
    x, y = torch.tensor(image, device="cuda"), torch.tensor(gt, device="cuda")
    a, b = raw_forward(x, y, 0.2), raw_forward(x, y, 0.2)
    for k in a:
        assert same_bits(a[k], b[k]), k
    assert same_bits(raw_backward(x, y, 0.2, a["dmaps"], 1.5), raw_backward(x, y, 0.2, b["dmaps"], 1.5))
