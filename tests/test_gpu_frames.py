"""uint8 ground truth on the GPU (include/ex4d_loss.h: ex4d_l1_ssim_forward_u8 / _backward_u8; include/ex4d_trainer.h:
ex4d_trainer_step_u8; ex4dgs_amd/frames.py).

The _u8 kernels are the float kernels with another ground-truth load: behind the load the arithmetic is the same code, and neither
kernel has an atomic.  So the bar between the loss on bytes and the loss on the looked-up float image is equality of bits."""
import pytest
import torch

from ex4dgs_amd import _abi

pytestmark = pytest.mark.gpu

DEV = "cuda"
LAMBDA = 0.2
UPSTREAM = 0.37
GUARD = 4096
FILL = 0xA5

SHAPES = [(1, 1),          # smallest legal image
          (7, 5),          # window larger than the image
          (48, 64),        # exactly one segment x one strip
          (49, 65),        # second segment and second strip of one row / column
          (53, 139),       # odd H*W: the golden image's shape
          (100, 200)]      # several full iterations of the ring


def _img(H, W, seed=3):
    return torch.rand(3, H, W, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _gt8(H, W, S, seed=5, alpha="ff"):
    """Seeded bytes with long constant runs (every third row is one value per channel), isolated extremes and a checkerboard of 0 and
    255 in the top-left corner; at S = 4 the fourth byte is 0xFF or noise."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    a[::3] = torch.randint(0, 256, (a[::3].shape[0], 1, 3), generator=g, dtype=torch.uint8)
    a[H // 2, W // 2] = torch.tensor([0, 255, 0], dtype=torch.uint8)
    a[H - 1, W - 1] = torch.tensor([255, 0, 255], dtype=torch.uint8)
    ch, cw = min(8, H), min(8, W)
    yy, xx = torch.meshgrid(torch.arange(ch), torch.arange(cw), indexing="ij")
    a[:ch, :cw] = (((yy + xx) % 2) * 255).to(torch.uint8)[..., None]
    if S == 4:
        fourth = torch.full((H, W, 1), 255, dtype=torch.uint8) if alpha == "ff" else torch.randint(0, 256, (H, W, 1), generator=g, dtype=torch.uint8)
        a = torch.cat([a, fourth], dim=2)
    return a.contiguous()


def _luts():
    from ex4dgs_amd.frames import gt_lut
    seeded = torch.randn(256, generator=torch.Generator().manual_seed(9))
    assert len(torch.unique(seeded)) == 256
    return {"default": None, "im_scale 1.7": gt_lut(1.7), "256 distinct": seeded}


def _as_float(gt8_cpu, lut):
    from ex4dgs_amd.frames import gt_lut
    table = gt_lut() if lut is None else lut
    return table[gt8_cpu.long()].permute(2, 0, 1)[:3].contiguous().to(DEV)


def _loss(img, gt, lut=None):
    """(loss, l1_errors, ssim_errors, image gradient) through l1_ssim_loss with the hook tensor, upstream gradient 0.37."""
    from ex4dgs_amd.loss import l1_ssim_loss
    x = img.clone().requires_grad_(True)
    acc = torch.ones(1, *img.shape[1:], device=DEV)
    loss, l1e, sse, hook = l1_ssim_loss(x, gt, LAMBDA, acc=acc, lut=lut)
    loss.backward(torch.tensor(UPSTREAM, device=DEV))
    assert l1e.data_ptr() == hook[1].data_ptr() and sse.data_ptr() == hook[2].data_ptr()
    return loss.detach(), l1e, sse, x.grad


def _same(got, want, what):
    for name, a, b in zip(("loss", "l1_errors", "ssim_errors", "grad"), got, want):
        assert torch.isfinite(b).all() and torch.equal(a, b), (what, name, float((a - b).abs().max()))


# ------------------------------------------------------------------------------------------------ 1. bytes = looked-up floats
@pytest.mark.parametrize("H, W", SHAPES)
def test_loss_on_bytes_equals_loss_on_the_looked_up_floats_bit_for_bit(hip_lib, H, W):
    img = _img(H, W)
    for S in (3, 4):
        gt8 = _gt8(H, W, S)
        block = torch.randint(0, 256, (3, H, W, S), generator=torch.Generator().manual_seed(6), dtype=torch.uint8)
        block[1] = gt8
        block = block.to(DEV)
        own = gt8.to(DEV)
        if (H * W * S) % 2:
            assert block[1].data_ptr() % 2 == 1                       # (53, 139, 3): an odd base address
        for tag, lut in _luts().items():
            want = _loss(img, _as_float(gt8, lut))
            _same(_loss(img, own, lut), want, (S, tag, "own allocation"))
            _same(_loss(img, block[1], lut), want, (S, tag, "frame 1 of 3"))
            if S == 4:                                                 # the fourth byte is never read
                noisy = _gt8(H, W, 4, alpha="noise")
                assert torch.equal(noisy[..., :3], gt8[..., :3]) and not torch.equal(noisy[..., 3], gt8[..., 3])
                _same(_loss(img, noisy.to(DEV), lut), want, (S, tag, "noise in the fourth byte"))


def test_the_float_path_keeps_its_refusals(hip_lib):
    from ex4dgs_amd.loss import l1_ssim_loss
    img = _img(7, 5)
    with pytest.raises(RuntimeError, match="float32 \\[C,H,W\\] tensors of the same shape"):
        l1_ssim_loss(img, img[:, :6])
    with pytest.raises(RuntimeError, match="lut= belongs to uint8"):
        l1_ssim_loss(img, img, lut=torch.zeros(256))
    with pytest.raises(RuntimeError, match="\\[H,W,3\\] or \\[H,W,4\\]"):
        l1_ssim_loss(img, torch.zeros(7, 5, 2, dtype=torch.uint8, device=DEV))


# ------------------------------------------------------------------------------------------------ 2. written before read, nothing beyond
def _guarded(nbytes):
    """(whole buffer, payload view) with GUARD bytes of FILL either side of the payload."""
    whole = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    return whole, whole[GUARD:GUARD + nbytes]


def _guards_kept(whole, nbytes):
    return bool((whole[:GUARD] == FILL).all()) and bool((whole[GUARD + nbytes:] == FILL).all())


@pytest.mark.parametrize("H, W", [(49, 65), (53, 139)])
def test_u8_calls_write_every_output_and_nothing_beyond(hip_lib, H, W):
    from ex4dgs_amd.frames import gt_lut
    from ex4dgs_amd.loss import _WINDOW
    lut = gt_lut(1.7)
    img = _img(H, W)
    gt8 = _gt8(H, W, 3)
    HW = H * W
    n_scratch = hip_lib.ex4d_l1_ssim_scratch_floats(H, W)
    sizes = {"gt": 3 * HW, "loss": 4, "l1e": 4 * HW, "sse": 4 * HW, "dmaps": 4 * 9 * HW, "scratch": 4 * n_scratch, "grad": 4 * 3 * HW, "gl": 4}
    buf = {k: _guarded(n) for k, n in sizes.items()}
    buf["gt"][1].copy_(gt8.reshape(-1))
    f = lambda k: buf[k][1].view(torch.float32)
    for k in ("loss", "l1e", "sse", "dmaps", "grad"):
        f(k).fill_(float("nan"))                                       # every element has to be written
    f("gl").fill_(UPSTREAM)
    p = lambda k: buf[k][1].data_ptr()
    with _abi.stream(img.device) as stream:
        _abi.call("ex4d_l1_ssim_forward_u8", H, W, img.data_ptr(), p("gt"), 3, lut.data_ptr(), LAMBDA, _WINDOW.ctypes.data,
                  p("loss"), p("l1e"), p("sse"), p("dmaps"), p("scratch"), stream)
        _abi.call("ex4d_l1_ssim_backward_u8", H, W, img.data_ptr(), p("gt"), 3, lut.data_ptr(), LAMBDA, _WINDOW.ctypes.data,
                  p("dmaps"), p("gl"), p("grad"), stream)
    torch.cuda.synchronize()
    for k in ("loss", "l1e", "sse", "dmaps", "grad"):
        assert torch.isfinite(f(k)).all(), k
    for k, n in sizes.items():
        assert _guards_kept(buf[k][0], n), k
    assert torch.equal(buf["gt"][1].cpu(), gt8.reshape(-1)) and float(f("gl")[0]) == pytest.approx(UPSTREAM)
    want = _loss(img, _as_float(gt8, lut))
    got = (f("loss")[0], f("l1e").view(H, W), f("sse").view(H, W), f("grad").view(3, H, W))
    _same(got, want, "raw calls")


# ------------------------------------------------------------------------------------------------ 3. graph
def test_u8_forward_and_backward_replay_from_one_graph(hip_lib):
    from ex4dgs_amd.frames import gt_lut
    from ex4dgs_amd.loss import _WINDOW
    H, W = 49, 65
    img = _img(H, W)
    frames = [_gt8(H, W, 3, seed=s) for s in (21, 22, 23)]
    gt8 = frames[0].to(DEV)
    f32 = dict(dtype=torch.float32, device=DEV)
    loss, l1e, sse, dmaps, grad = torch.empty(1, **f32), torch.empty(H, W, **f32), torch.empty(H, W, **f32), torch.empty(9, H, W, **f32), torch.empty(3, H, W, **f32)
    scratch = torch.empty(hip_lib.ex4d_l1_ssim_scratch_floats(H, W), **f32)
    gl = torch.full((1,), UPSTREAM, **f32)

    def both():
        lut = gt_lut(1.7)                      # read during the call: the graph holds the table by value, this tensor dies here
        with _abi.stream(img.device) as stream:
            _abi.call("ex4d_l1_ssim_forward_u8", H, W, img.data_ptr(), gt8.data_ptr(), 3, lut.data_ptr(), LAMBDA, _WINDOW.ctypes.data,
                      loss.data_ptr(), l1e.data_ptr(), sse.data_ptr(), dmaps.data_ptr(), scratch.data_ptr(), stream)
            _abi.call("ex4d_l1_ssim_backward_u8", H, W, img.data_ptr(), gt8.data_ptr(), 3, lut.data_ptr(), LAMBDA, _WINDOW.ctypes.data,
                      dmaps.data_ptr(), gl.data_ptr(), grad.data_ptr(), stream)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):              # one eager call first
        both()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _same((loss[0], l1e, sse, grad), _loss(img, _as_float(frames[0], gt_lut(1.7))), "eager")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    for frame in frames[1:]:
        gt8.copy_(frame.to(DEV))               # new content in place
        for t in (loss, l1e, sse, grad):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        _same((loss[0], l1e, sse, grad), _loss(img, _as_float(frame, gt_lut(1.7))), "replay")


# ------------------------------------------------------------------------------------------------ 4. the compiled trainer
def test_the_compiled_trainer_on_bytes_is_the_compiled_trainer_on_floats(hip_lib):
    from tests import test_gpu_native_l1accum as l1a            # the smallest model the compiled-trainer tests use, and their bars
    from ex4dgs_amd import densify
    from ex4dgs_amd.frames import gt_lut
    from ex4dgs_amd.native_trainer import NativeTrainer
    (ma, cam, bg), (mb, _, _) = l1a._scene(), l1a._scene()
    H, W = int(cam.image_height), int(cam.image_width)
    lut = gt_lut(1.7)
    gt8_cpu = _gt8(H, W, 3, seed=31)
    gt8, gtf = gt8_cpu.to(DEV), _as_float(gt8_cpu, lut)
    p0 = {n: getattr(ma, n).clone() for n in ma.PARAM_NAMES}
    na = NativeTrainer(ma, cam, optimizer=True, lrs=l1a._lrs(ma))
    nb = NativeTrainer(mb, cam, optimizer=True, lrs=l1a._lrs(mb))
    sa, sb = densify.DensityStats(ma), densify.DensityStats(mb)
    for i, t in enumerate((0, 137, 41)):
        na.step(cam, bg, t, gtf, l1_accum=True, stats=sa, nan_census=True)
        nb.step(cam, bg, t, gt8, l1_accum=True, stats=sb, nan_census=True, lut=lut)
        ra, rb = na.report(), nb.report()
        assert na.num_rendered == nb.num_rendered > 0 and ra[1:] == rb[1:] == (0, 0)
        if i == 0:                             # the forward is deterministic: same parameters, same bits
            assert ra[0] == rb[0] > 0
            assert torch.equal(na.output("render"), nb.output("render"))
            ha, hb = na.output("hook"), nb.output("hook")
            assert torch.equal(ha[1], hb[1]) and torch.equal(ha[2], hb[2]) and float(ha[1].abs().max()) > 0
        else:                                  # behind the compositing backward's float atomics: the trainers' own bars
            assert abs(ra[0] - rb[0]) <= 1e-6, (t, ra[0], rb[0])
    torch.cuda.synchronize()
    assert na.steps() == nb.steps() == 3
    moved = {n: l1a._within_the_trainers_bar(getattr(ma, n), getattr(mb, n), p0[n], n) for n in ma.PARAM_NAMES}
    assert len(moved) == 15 and moved["_xyz"] > 0 and moved["_xyz_motion"] > 0 and moved["_features_dc"] > 0
    na.close(); nb.close()


def test_the_compiled_trainer_on_rgba_bytes_and_with_the_asynchronous_forward(hip_lib):
    from tests import test_gpu_native_l1accum as l1a
    from ex4dgs_amd.frames import gt_lut
    from ex4dgs_amd.native_trainer import NativeTrainer
    model, cam, bg = l1a._scene()
    H, W = int(cam.image_height), int(cam.image_width)
    lut = gt_lut(0.5)
    rgba_cpu = _gt8(H, W, 4, seed=32, alpha="noise")
    rgba, rgb = rgba_cpu.to(DEV), rgba_cpu[..., :3].contiguous().to(DEV)
    gtf = _as_float(rgba_cpu, lut)
    nt = NativeTrainer(model, cam, optimizer=False, lrs=l1a._lrs(model))     # no optimizer: every step sees the same parameters

    def frame(gt, **kw):
        nt.step(cam, bg, 137, gt, l1_accum=True, **kw)
        return nt.report()[0], nt.output("render"), nt.output("hook"), nt.num_rendered

    def same(a, b):
        assert a[0] == b[0] > 0 and a[3] == b[3] > 0 and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])

    want = frame(gtf)
    same(frame(rgba, lut=lut), want)
    same(frame(rgb), frame(_as_float(rgba_cpu, None)))                       # lut=None through the trainer: u / 255
    nt.set_async(True)
    frame(gtf)                                 # (the synchronous frame that seeds the capacity)
    want = frame(gtf)
    same(frame(rgb, lut=lut), want)
    same(frame(rgba, lut=lut), want)
    with pytest.raises(RuntimeError, match="uint8 gt_image"):
        nt.step(cam, bg, 137, rgba[:, :-1])
    with pytest.raises(RuntimeError, match="lut= belongs to uint8"):
        nt.step(cam, bg, 137, gtf, lut=lut)
    with pytest.raises(RuntimeError, match="pixel_stride"):
        with _abi.stream(nt.device) as stream:
            _abi.call("ex4d_trainer_step_u8", nt.handle, 0.0, cam.world_view_transform.data_ptr(), cam.full_proj_transform.data_ptr(),
                      cam.camera_center.data_ptr(), bg.data_ptr(), rgba.data_ptr(), 5, None, stream, None, None)
    nt.close()


# ------------------------------------------------------------------------------------------------ 5. FrameStore / FrameStream
def test_frame_store_keeps_what_was_put(hip_lib):
    from ex4dgs_amd.frames import FrameStore
    H, W = 53, 139
    frames = [_gt8(H, W, 3, seed=40 + i) for i in range(5)]
    store = FrameStore(5, H, W, device=DEV)
    assert store.bytes() == 5 * H * W * 3 and len(store) == 5
    with pytest.raises(RuntimeError, match="never put"):
        store.get(0)
    for i, f in enumerate(frames):
        store.put(i, f.numpy() if i % 2 else f)                # numpy and torch sources
    for i, f in enumerate(frames):
        view = store.get(i)
        assert view.data_ptr() == store.frames.data_ptr() + i * H * W * 3 and tuple(view.shape) == (H, W, 3)
        assert torch.equal(view.cpu(), f), i
    newer = _gt8(H, W, 3, seed=50)
    store.put(2, newer)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        copy = store.get(2, stream=side).clone()
    side.synchronize()
    assert torch.equal(copy.cpu(), newer) and torch.equal(store.get(2).cpu(), newer) and torch.equal(store.get(1).cpu(), frames[1])
    with pytest.raises(RuntimeError, match="uint8"):
        store.put(0, newer[:, :-1])


def test_frame_stream_orders_uploads_and_consumers(hip_lib):
    """Push and pop 7 frames through 2 slots with a device copy of each view enqueued before the next push: a copy that ran before its
    upload, or a slot overwritten before its consumer ran, shows as a wrong copy."""
    from ex4dgs_amd.frames import FrameStream
    H, W = 53, 139
    frames = [_gt8(H, W, 3, seed=60 + i) for i in range(7)]
    fs = FrameStream(H, W, depth=2, device=DEV)
    assert fs.bytes() == 2 * H * W * 3
    with pytest.raises(RuntimeError, match="nothing pushed"):
        fs.pop()
    copies = []
    fs.push(frames[0])
    for i in range(7):
        if i + 1 < 7:
            fs.push(frames[i + 1])             # the next frame's upload is in flight while this one is consumed
        view = fs.pop()
        copies.append(view.clone())            # the consumer, on the current stream
    with pytest.raises(RuntimeError, match="nothing pushed"):
        fs.pop()
    torch.cuda.synchronize()
    for i, (c, f) in enumerate(zip(copies, frames)):
        assert torch.equal(c.cpu(), f), i
    fs.push(frames[0]); fs.push(frames[1])
    with pytest.raises(RuntimeError, match="pop one first"):
        fs.push(frames[2])
