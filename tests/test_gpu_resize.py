"""Resizing decoded frames on the GPU (include/ex4d_loss.h: ex4d_resize_u8; ex4dgs_amd/frames.py: resize_u8, FrameStore / FrameStream
with source_size).  The arithmetic is integer behind a host-built table, so the bar is equality of every byte with the numpy
restatement (tests/resize_ref.py), which tests/test_cpu_resize.py holds to Pillow's bytes, and with Pillow's recorded bytes
(tests/golden/resize.npz).  Pillow itself is not needed here."""
import os

import numpy as np
import pytest
import torch

from ex4dgs_amd import frames
from tests import resize_cases as rc
from tests import resize_ref as rr

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "resize.npz"))
# byte offsets of (src, dst, scratch) inside their buffers: each of 0, 1, 2, 3 once per buffer
PLACEMENTS = [(0, 0, 0), (1, 3, 2), (2, 1, 3), (3, 2, 1)]
FILLS = (0xA5, 0x00)
_REF = {}


def _reference(case, content, resample):
    """(source bytes, the restatement's resize) of a case: computed once, shared, never written."""
    key = (case, content, resample)
    if key not in _REF:
        src = rc.CONTENT[content](case[0], case[1])
        out = rr.resize(src, case[2:], resample)
        src.setflags(write=False)
        out.setflags(write=False)
        _REF[key] = (src, out)
    return _REF[key]


class _Guarded:
    """`nbytes` bytes at byte offset `offset` behind a guard band, with a guard band after them."""

    def __init__(self, nbytes, offset, fill):
        self.lo, self.n = GUARD + offset, nbytes
        self.buf = torch.full((GUARD + offset + nbytes + GUARD,), fill, dtype=torch.uint8, device=DEV)
        self.fill = fill
        assert self.buf.data_ptr() % 4 == 0

    def view(self, *shape):
        return self.buf[self.lo:self.lo + self.n].view(*shape)

    def guards_untouched(self):
        b = self.buf.cpu()
        return bool((b[:self.lo] == self.fill).all() and (b[self.lo + self.n:] == self.fill).all())


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _placed(src_np, offset):
    buf = torch.zeros(offset + src_np.size, dtype=torch.uint8, device=DEV)
    buf[offset:] = _dev(src_np).reshape(-1)
    return buf, buf[offset:].view(*src_np.shape)


def _run(case, resample, src_view, o_dst, o_scr, fill):
    """One resize into guarded, pre-filled dst and scratch; returns the bytes and checks the guard bands."""
    plan = frames.ResizePlan(case[:2], case[2:], resample, DEV)
    dst = _Guarded(case[2] * case[3] * 3, o_dst, fill)
    scr = _Guarded(plan.scratch.numel(), o_scr, fill)
    plan.scratch = scr.view(-1)
    out = frames.resize_u8(src_view, out=dst.view(case[2], case[3], 3), plan=plan)
    got = out.cpu().numpy()
    assert dst.guards_untouched() and scr.guards_untouched(), (case, resample, o_dst, o_scr, fill)
    return got


# ------------------------------------------------------------------------------------------------ 1. every byte, every case
@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
def test_resize_equals_the_restatement_byte_for_byte(hip_lib, case):
    for content in rc.CONTENT:
        for resample in rc.FILTERS:
            src, want = _reference(case, content, resample)
            if case in rc.NAMED:
                assert np.array_equal(want, GOLDEN[f"{rc.case_id(case)}/{content}/{resample}"]), "the restatement is Pillow's recorded bytes"
            for o_src, o_dst, o_scr in PLACEMENTS:
                keep, view = _placed(src, o_src)
                assert view.data_ptr() % 4 == o_src
                for fill in FILLS:
                    got = _run(case, resample, view, o_dst, o_scr, fill)
                    bad = int((got != want).sum())
                    assert bad == 0, (case, content, resample, (o_src, o_dst, o_scr), hex(fill), bad, np.argwhere(got != want)[:4].tolist())
                assert np.array_equal(view.cpu().numpy(), src), "the source is not written"


@pytest.mark.parametrize("case", [(14, 22, 7, 11), (253, 338, 126, 169)], ids=rc.case_id)
def test_bicubic_on_the_saturating_pattern_reaches_both_clamps(hip_lib, case):
    """The point of the 0 / 255 pattern, asserted from the restatement so that it cannot be lost silently: some un-clamped accumulator
    is below 0 and some is above 255, in the horizontal pass and in the vertical one; and the kernels' bytes are the clamped ones."""
    src = rc.saturating(case[0], case[1])
    out, mid = rr.resize(src, case[2:], "bicubic", parts=True)
    h = rr.accumulate(np.ascontiguousarray(src.transpose(1, 0, 2)), case[3], "bicubic") >> rr.BITS
    v = rr.accumulate(mid, case[2], "bicubic") >> rr.BITS
    assert h.min() < 0 and h.max() > 255 and v.min() < 0 and v.max() > 255, (h.min(), h.max(), v.min(), v.max())
    assert 0 in out and 255 in out
    got = frames.resize_u8(_dev(src), plan=frames.resize_plan(case[:2], case[2:], "bicubic", DEV))
    assert np.array_equal(got.cpu().numpy(), out)


def test_default_plan_is_bilinear_and_cached(hip_lib):
    case = (15, 23, 7, 11)
    src, want = _reference(case, "random", "bilinear")
    out = torch.empty(7, 11, 3, dtype=torch.uint8, device=DEV)
    assert frames.resize_u8(_dev(src), out=out) is out and np.array_equal(out.cpu().numpy(), want)
    plan = frames.resize_plan((15, 23), (7, 11), device=DEV)
    assert plan is frames.resize_plan((15, 23), (7, 11), "bilinear", DEV) and plan.resample == "bilinear"
    other = frames.resize_plan((15, 23), (7, 11), "box", DEV)
    assert other is not plan and other.scratch.data_ptr() != plan.scratch.data_ptr()
    assert plan.table_x is frames.ResizePlan((15, 23), (9, 11), device=DEV).table_x, "tables are shared per (in, out, filter)"
    assert np.array_equal(frames.resize_u8(_dev(src), plan=plan).cpu().numpy(), want)
    with pytest.raises(RuntimeError, match="the plan resizes"):
        frames.resize_u8(torch.zeros(14, 23, 3, dtype=torch.uint8, device=DEV), plan=plan)
    with pytest.raises(RuntimeError, match="the plan gives"):
        frames.resize_u8(_dev(src), out=torch.zeros(7, 12, 3, dtype=torch.uint8, device=DEV), plan=plan)
    with pytest.raises(RuntimeError, match="premultiplied"):
        frames.resize_u8(torch.zeros(15, 23, 4, dtype=torch.uint8, device=DEV), plan=plan)
    with pytest.raises(RuntimeError, match="premultiplied"):
        frames.resize_u8(_dev(src), out=torch.zeros(7, 11, 4, dtype=torch.uint8, device=DEV), plan=plan)


# ------------------------------------------------------------------------------------------------ 2. no state in the plan
@pytest.mark.parametrize("resample", rc.FILTERS)
def test_one_plan_two_frames_in_a_row(hip_lib, resample):
    case = (33, 65, 16, 32)
    plan = frames.ResizePlan(case[:2], case[2:], resample, DEV)
    a = rc.random_bytes(33, 65, seed=21)
    b = rc.saturating(33, 65)
    da, db = _dev(a), _dev(b)
    out_a = frames.resize_u8(da, plan=plan)
    out_b = frames.resize_u8(db, plan=plan)                  # enqueued behind the first: the scratch is rewritten before it is read
    out_a2 = frames.resize_u8(da, plan=plan)
    assert np.array_equal(out_a.cpu().numpy(), rr.resize(a, case[2:], resample))
    assert np.array_equal(out_b.cpu().numpy(), rr.resize(b, case[2:], resample))
    assert torch.equal(out_a, out_a2)


# ------------------------------------------------------------------------------------------------ 3. graph capture
def test_resize_is_captured_and_replayed_on_changed_bytes(hip_lib):
    """A linear chain (two kernels, one stream): captured once, replayed twice on other source bytes."""
    case = (40, 64, 13, 21)
    plan = frames.ResizePlan(case[:2], case[2:], "bilinear", DEV)
    inputs = [rc.random_bytes(40, 64, seed=31 + i) for i in range(3)]
    src = _dev(inputs[0])
    out = torch.zeros(13, 21, 3, dtype=torch.uint8, device=DEV)
    frames.resize_u8(src, out=out, plan=plan)                # warm: nothing is created during the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        frames.resize_u8(src, out=out, plan=plan)
    for a in inputs[1:]:
        src.copy_(_dev(a))
        out.fill_(0xA5)
        graph.replay()
        torch.cuda.synchronize()
        eager = frames.resize_u8(_dev(a), plan=frames.ResizePlan(case[:2], case[2:], "bilinear", DEV))
        assert torch.equal(out, eager) and np.array_equal(out.cpu().numpy(), rr.resize(a, case[2:]))


# ------------------------------------------------------------------------------------------------ 4. FrameStore / FrameStream
def test_frame_store_resizes_full_resolution_frames(hip_lib):
    full, small = GOLDEN["frames/in"], GOLDEN["frames/out"]
    n, (H, W) = len(full), small.shape[1:3]
    store = frames.FrameStore(n, H, W, device=DEV, source_size=full.shape[1:3])
    for i in range(n):
        store.put(i, full[i] if i % 2 else torch.from_numpy(full[i]))
    for i in range(n):
        view = store.get(i)
        assert view.data_ptr() == store.frames.data_ptr() + i * H * W * 3 and tuple(view.shape) == (H, W, 3)
        assert np.array_equal(view.cpu().numpy(), small[i]), i
    # an already-resized frame into the same store: today's path, the bytes as they are
    plain = frames.FrameStore(n, H, W, device=DEV)
    already = rc.random_bytes(H, W, seed=77)
    store.put(1, already)
    plain.put(1, already)
    assert torch.equal(store.get(1), plain.get(1)) and np.array_equal(store.get(1).cpu().numpy(), already)
    store.put(1, full[3])                                    # and a full-resolution one over it
    assert np.array_equal(store.get(1).cpu().numpy(), small[3])
    with pytest.raises(RuntimeError, match=r"\[7, 11, 3\] or \[15, 23, 3\]"):
        store.put(0, np.zeros((15, 22, 3), np.uint8))
    with pytest.raises(RuntimeError, match=r"uint8 \[7, 11, 3\]$"):
        plain.put(0, full[0])                                # without source_size nothing changes: the frame is refused
    assert plain._source is None and store._source.staged.shape == (frames.FrameStore.STAGING, 15, 23, 3)


def test_frame_store_ready_event_is_behind_the_resize(hip_lib):
    """The consumer is on another stream and is enqueued at once: it sees the resized bytes, for every frame, because the frame's
    event is recorded behind the resize."""
    case = (253, 338, 126, 169)
    srcs = [rc.random_bytes(253, 338, seed=90 + i) for i in range(4)]
    store = frames.FrameStore(4, 126, 169, device=DEV, source_size=(253, 338))
    side = torch.cuda.Stream()
    copies = []
    for i, a in enumerate(srcs):
        store.put(i, a)
        view = store.get(i, stream=side)
        with torch.cuda.stream(side):
            copies.append(view.clone())
    side.synchronize()
    for a, c in zip(srcs, copies):
        assert np.array_equal(c.cpu().numpy(), rr.resize(a, case[2:]))


def test_frame_stream_resizes_in_order(hip_lib):
    full, small = GOLDEN["frames/in"], GOLDEN["frames/out"]
    fs = frames.FrameStream(7, 11, depth=2, device=DEV, source_size=(15, 23))
    assert fs.bytes() == 2 * 7 * 11 * 3
    copies = []
    fs.push(full[0])
    for i in range(5):
        if i + 1 < 5:
            fs.push(full[i + 1])
        copies.append(fs.pop().clone())
    for i in range(5):
        assert np.array_equal(copies[i].cpu().numpy(), small[i]), i
    fs.push(small[2])                                        # an already-resized frame takes the plain path
    assert np.array_equal(fs.pop().cpu().numpy(), small[2])


# ------------------------------------------------------------------------------------------------ 5. end to end: the loss
def test_loss_on_a_frame_resized_on_the_gpu_equals_the_loss_on_the_restatements_bytes(hip_lib):
    from ex4dgs_amd.loss import l1_ssim_loss
    H, W = 53, 139
    full = rc.random_bytes(2 * H, 2 * W, seed=55)
    image = torch.rand(3, H, W, generator=torch.Generator().manual_seed(3)).to(DEV)
    lut = frames.gt_lut(1.15)
    store = frames.FrameStore(2, H, W, device=DEV, source_size=(2 * H, 2 * W))
    store.put(1, full)                                       # frame 1 starts at an odd byte
    plain = frames.FrameStore(2, H, W, device=DEV)
    plain.put(1, rr.resize(full, (H, W)))

    def run(gt):
        x = image.clone().requires_grad_(True)
        loss, l1e, sse = l1_ssim_loss(x, gt, lut=lut)
        loss.backward()
        return loss.detach(), l1e, sse, x.grad

    for a, b in zip(run(store.get(1)), run(plain.get(1))):
        assert torch.isfinite(b).all() and torch.equal(a, b)
