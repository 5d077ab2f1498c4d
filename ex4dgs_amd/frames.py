"""Ground-truth frames as the image decoder leaves them: uint8 [H,W,3|4], from host memory to the loss kernels.

The reference decodes an image per iteration, divides by 255.0, permutes, divides by im_scale, clamps (scene/__init__.py:199-201,
utils/general_utils.py:23-29) and uploads 16.4 MB of pageable float32 at 1352x1014 (train.py:125).  Here the frame stays the 4.1 MB of
bytes it was decoded into; the float value of a byte is a 256-entry table the loss kernels read on load (include/ex4d_loss.h:
ex4d_l1_ssim_forward_u8), so the float image is never written or read.

    lut = gt_lut(im_scale)                                  # (u / 255.0 / im_scale).clamp(0, 1), bit for bit the reference's floats
    store = FrameStore(n_frames, H, W)                      # a whole scene resident: 19 x 300 x 1352 x 1014 x 3 B = 23 GB
    store.put(i, np.array(Image.open(path)))                # asynchronous, through pinned memory
    native.step(cam, bg, t, store.get(i), lut=lut)          # or loss.l1_ssim_loss(image, store.get(i), lut=lut)

    stream = FrameStream(H, W, depth=2)                     # a scene that does not fit: the upload of frame n + 1 overlaps step n
    stream.push(next_frame); gt = stream.pop()

Frames decoded at another resolution are resized on the device, bit for bit as the reference's PILtoTorch(image, resolution) does it
(PIL's 8-bit Image.resize, resample=2; include/ex4d_loss.h: ex4d_resize_u8):

    W, H = reference_size(2704, 2028, resolution=2)         # the size the reference computes: another size is not its frame
    store = FrameStore(n_frames, H, W, source_size=(2028, 2704))
    store.put(i, np.array(Image.open(path)))                # [2028,2704,3]: uploaded, then resized on the copy stream
    small = resize_u8(frame_u8_cuda, plan=resize_plan((2028, 2704), (H, W)))

Decoding stays with PIL on the host.  Plain events and two streams; no host threads.  No CPU fallback.
"""
import numpy as np
import torch

from . import _abi

RESAMPLE = {"bilinear": 2, "bicubic": 3, "box": 4}          # EX4D_FILTER_*: PIL's resample numbers
MAX_SIZE = 16384                                            # EX4D_FRAME_MAX_SIZE
RGBA_REFUSED = ("four-byte pixels are not resized: PIL resizes RGBA on premultiplied colour, which gives other colour bytes than its "
                "RGB resize; drop the fourth byte first")


def gt_lut(im_scale=1.0):
    """float32 [256] CPU table: the value the reference's image tensor holds for each byte -- built with the torch ops the reference
    applies to the image itself (PILtoTorch's `/ 255.0`, im_reader's `/ im_scale` and `.clamp(0, 1)`), so lut[u8] is that tensor."""
    return (torch.arange(256, dtype=torch.uint8) / 255.0 / im_scale).clamp(0, 1)


def _host_frame(host_u8, shape, source_shape=None):
    t = torch.from_numpy(host_u8) if isinstance(host_u8, np.ndarray) else host_u8
    ok = isinstance(t, torch.Tensor) and t.device.type == "cpu" and t.dtype == torch.uint8
    if not ok or (tuple(t.shape) != shape and (source_shape is None or tuple(t.shape) != source_shape)):
        either = f" or {list(source_shape)}" if source_shape is not None else ""
        raise RuntimeError(f"a frame is a numpy array or a CPU torch tensor, uint8 {list(shape)}{either}")
    return t


def _device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("frames live on a ROCm device (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def reference_size(orig_w, orig_h, resolution, resolution_scale=1.0, ss=False):
    """(W, H) the reference resizes an orig_w x orig_h image to (scene/cameras.py:165-182): round(orig / (resolution_scale *
    resolution)) for resolution 1, 2, 4, 8; for -1, width 1600 where the image is wider and its own size otherwise; any other value is
    the width asked for; both of these truncate.  ss=True: the (int(orig_w / 2), int(orig_h / 2)) of :255, whatever the resolution."""
    if ss:
        return int(orig_w / 2), int(orig_h / 2)
    if resolution in (1, 2, 4, 8):
        return round(orig_w / (resolution_scale * resolution)), round(orig_h / (resolution_scale * resolution))
    if resolution == -1:
        global_down = orig_w / 1600 if orig_w > 1600 else 1
    else:
        global_down = orig_w / resolution
    scale = float(global_down) * float(resolution_scale)
    return int(orig_w / scale), int(orig_h / scale)


_TABLES = {}         # (in, out, filter, device) -> device int32 table: read-only, shared by every plan
_PLANS = {}          # resize_plan's cache


def _filter(resample):
    if resample not in RESAMPLE:
        raise RuntimeError(f"resample {resample!r}: one of {sorted(RESAMPLE)} (Lanczos and Hamming depend on libm and are not offered)")
    return RESAMPLE[resample]


def _checked(in_hw, out_hw, resample):
    """((H_in, W_in), (H_out, W_out), filter number); refuses what the library refuses, before any device is touched."""
    in_hw, out_hw = (int(in_hw[0]), int(in_hw[1])), (int(out_hw[0]), int(out_hw[1]))
    filt = _filter(resample)
    if any(v < 1 or v > MAX_SIZE for v in in_hw + out_hw):
        raise RuntimeError(f"resize {in_hw} -> {out_hw}: sizes are 1 .. {MAX_SIZE} per axis")
    return in_hw, out_hw, filt


def _table(n_in, n_out, filt, device):
    """The device table of one axis (None where the pass is skipped), built by the library's host code and uploaded once."""
    if n_in == n_out:
        return None
    key = (n_in, n_out, filt, device)
    if key not in _TABLES:
        lib = _abi.load()
        words = np.empty(lib.ex4d_resize_u8_table_words(n_in, n_out, filt), dtype=np.int32)
        _abi.call("ex4d_resize_u8_table", n_in, n_out, filt, words.ctypes.data)
        _TABLES[key] = torch.from_numpy(words).to(device)
    return _TABLES[key]


class ResizePlan:
    """The two device tables (shared, read-only) and the scratch (this plan's own) of one [H_in,W_in,3] -> [H_out,W_out,3] resize.  The
    scratch serialises the plan's calls: use one plan on one stream at a time."""

    def __init__(self, in_hw, out_hw, resample="bilinear", device="cuda"):
        self.in_hw, self.out_hw, filt = _checked(in_hw, out_hw, resample)
        self.resample, self.device = resample, _device(device)
        self.table_x = _table(self.in_hw[1], self.out_hw[1], filt, self.device)
        self.table_y = _table(self.in_hw[0], self.out_hw[0], filt, self.device)
        self.scratch = torch.empty(_abi.load().ex4d_resize_u8_scratch_bytes(self.in_hw[0], self.in_hw[1], self.out_hw[0], self.out_hw[1]),
                                   dtype=torch.uint8, device=self.device)


def resize_plan(in_hw, out_hw, resample="bilinear", device="cuda"):
    """The cached ResizePlan of (in_hw, out_hw, resample, device)."""
    key = _checked(in_hw, out_hw, resample)[:2] + (resample, _device(device))
    if key not in _PLANS:
        _PLANS[key] = ResizePlan(in_hw, out_hw, resample, key[3])
    return _PLANS[key]


def _check_source(owner, source_size, pixel_stride):
    if source_size is not None and pixel_stride != 3:
        raise RuntimeError(f"{owner}: source_size needs pixel_stride 3: {RGBA_REFUSED}")


def _rgb_frame(t, what):
    if isinstance(t, torch.Tensor) and t.dim() == 3 and t.shape[2] == 4:
        raise RuntimeError(f"resize_u8: {what}: {RGBA_REFUSED}")
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != torch.uint8 or t.dim() != 3:
        raise RuntimeError(f"resize_u8: {what} is a device uint8 [H,W,3] tensor (no CPU fallback)")
    if t.shape[2] != 3 or not t.is_contiguous():
        raise RuntimeError(f"resize_u8: {what} is tightly packed [H,W,3]")


def resize_u8(src, out=None, plan=None):
    """src device uint8 [H_in,W_in,3] -> [H_out,W_out,3] (any byte alignment: views into a store are fine) on the current stream, bit for
    bit PIL's Image.resize of the plan's filter.  The output size comes from `plan` or from `out`; without a plan the cached bilinear
    plan of the two sizes is used.  Does not synchronise; can be captured into a graph."""
    _rgb_frame(src, "src")
    if out is not None:
        _rgb_frame(out, "out")
    if plan is None:
        if out is None:
            raise RuntimeError("resize_u8: the output size comes from `out` or from `plan`")
        plan = resize_plan(src.shape[:2], out.shape[:2], device=src.device)
    if tuple(src.shape[:2]) != plan.in_hw or src.device != plan.device:
        raise RuntimeError(f"resize_u8: src is {list(src.shape)} on {src.device}, the plan resizes {plan.in_hw} on {plan.device}")
    if out is None:
        out = torch.empty(plan.out_hw + (3,), dtype=torch.uint8, device=src.device)
    elif tuple(out.shape[:2]) != plan.out_hw or out.device != plan.device:
        raise RuntimeError(f"resize_u8: out is {list(out.shape)} on {out.device}, the plan gives {plan.out_hw} on {plan.device}")
    with _abi.stream(src.device) as stream:
        _abi.call("ex4d_resize_u8", plan.in_hw[0], plan.in_hw[1], plan.out_hw[0], plan.out_hw[1], 3, src.data_ptr(), out.data_ptr(),
                  _abi.ptr(plan.table_x), _abi.ptr(plan.table_y), _abi.ptr(plan.scratch), stream)
    return out


class _Source:
    """What a store or a stream holds for frames that arrive at another resolution: `slots` pinned and device staging frames of the
    source size and a plan of its own (its scratch is used on the owner's copy stream only)."""

    def __init__(self, source_size, shape, resample, slots, device):
        self.shape = (int(source_size[0]), int(source_size[1]), 3)
        self.plan = ResizePlan(self.shape[:2], shape[:2], resample, device)
        self.pinned = [torch.empty(self.shape, dtype=torch.uint8).pin_memory() for _ in range(slots)]
        self.staged = torch.empty((slots,) + self.shape, dtype=torch.uint8, device=device)

    def upload(self, slot, src, dst):
        """On the current (copy) stream: pinned -> device staging -> resized into dst."""
        self.pinned[slot].copy_(src)
        self.staged[slot].copy_(self.pinned[slot], non_blocking=True)
        resize_u8(self.staged[slot], out=dst, plan=self.plan)


class FrameStore:
    """n_frames ground-truth frames resident on the device as one uint8 [N,H,W,S] allocation (frame i starts at byte i*H*W*S: odd for
    odd H*W at S = 3 -- the loss kernels take any alignment).  A store larger than free memory raises from the allocation."""
    STAGING = 2                  # pinned staging slots: the host copy of put n + 1 overlaps the upload of put n

    def __init__(self, n_frames, H, W, pixel_stride=3, device="cuda", source_size=None, resample="bilinear"):
        """source_size=(H_in, W_in): put additionally takes [H_in,W_in,3] frames and resizes them on the device (resize_u8 with
        `resample`), behind their upload on the copy stream; the store then also holds STAGING pinned and STAGING device frames of that
        size.  Without it nothing is allocated or launched for resizing."""
        if pixel_stride not in (3, 4) or n_frames <= 0 or H <= 0 or W <= 0:
            raise RuntimeError("FrameStore: n_frames, H, W > 0 and pixel_stride 3 or 4")
        _check_source("FrameStore", source_size, pixel_stride)
        self.device = _device(device)
        self.shape = (int(H), int(W), int(pixel_stride))
        self._source = None if source_size is None else _Source(source_size, self.shape, resample, self.STAGING, self.device)
        self.frames = torch.empty((int(n_frames),) + self.shape, dtype=torch.uint8, device=self.device)
        self._staging = [torch.empty(self.shape, dtype=torch.uint8).pin_memory() for _ in range(self.STAGING)]
        self._staged = [None] * self.STAGING         # the event behind the last upload out of each staging slot
        self._copy = torch.cuda.Stream(self.device)
        self._ready = [None] * int(n_frames)         # per frame: the event behind its last upload
        self._waited = [set() for _ in range(int(n_frames))]
        self._puts = 0

    def __len__(self):
        return self.frames.shape[0]

    def bytes(self):
        return self.frames.numel()

    def put(self, i, host_u8):
        """Upload frame i (numpy or CPU torch uint8 [H,W,S]) asynchronously on the store's copy stream.  The upload is ordered behind
        the work enqueued so far on the current stream, so a consumer of the frame's previous content that was enqueued there is done
        with it first.  With source_size, a [H_in,W_in,3] frame is uploaded to a staging frame and resized into frame i on the same
        stream; the frame is ready when the resize is done."""
        full = self._source is not None and self._source.shape != self.shape
        src = _host_frame(host_u8, self.shape, self._source.shape if full else None)
        full = full and tuple(src.shape) == self._source.shape
        slot = self._puts % self.STAGING
        self._puts += 1
        if self._staged[slot] is not None:
            self._staged[slot].synchronize()         # the upload (and resize) that last used this slot's staging
        if not full:
            self._staging[slot].copy_(src)
        self._copy.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self._copy):
            if full:
                self._source.upload(slot, src, self.frames[i])
            else:
                self.frames[i].copy_(self._staging[slot], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._copy)
        self._staged[slot] = self._ready[i] = ev
        self._waited[i].clear()

    def get(self, i, stream=None):
        """The device view [H,W,S] of frame i; `stream` (default: the current one) waits for the frame's upload, once per upload."""
        stream = torch.cuda.current_stream(self.device) if stream is None else stream
        ev = self._ready[i]
        if ev is None:
            raise RuntimeError(f"frame {i} was never put")
        if stream.cuda_stream not in self._waited[i]:
            stream.wait_event(ev)
            self._waited[i].add(stream.cuda_stream)
        return self.frames[i]


class FrameStream:
    """For scenes that do not fit: `depth` pinned slots paired with `depth` device slots.  push() copies a frame into the next pinned
    slot and enqueues its upload on the copy stream; pop() makes the consuming stream wait for the oldest pushed frame and returns its
    device view, valid until the next pop: that pop records the slot's release event on the consuming stream, and a push into the slot
    waits on the host for that event only."""

    def __init__(self, H, W, pixel_stride=3, depth=2, device="cuda", source_size=None, resample="bilinear"):
        """source_size=(H_in, W_in): push additionally takes [H_in,W_in,3] frames, as FrameStore.put does (`depth` pinned and device
        staging frames of that size)."""
        if pixel_stride not in (3, 4) or depth < 1 or H <= 0 or W <= 0:
            raise RuntimeError("FrameStream: H, W > 0, pixel_stride 3 or 4, depth >= 1")
        _check_source("FrameStream", source_size, pixel_stride)
        self.device = _device(device)
        self.shape = (int(H), int(W), int(pixel_stride))
        self.depth = int(depth)
        self._source = None if source_size is None else _Source(source_size, self.shape, resample, self.depth, self.device)
        self._pinned = [torch.empty(self.shape, dtype=torch.uint8).pin_memory() for _ in range(self.depth)]
        self._slots = torch.empty((self.depth,) + self.shape, dtype=torch.uint8, device=self.device)
        self._copy = torch.cuda.Stream(self.device)
        self._ready = [None] * self.depth            # upload done
        self._release = [None] * self.depth          # consumer done (recorded by the pop after the one that handed the slot out)
        self._pushed = self._popped = 0
        self._held = None                            # (slot, stream) of the view the last pop returned

    def bytes(self):
        return self._slots.numel()

    def _let_go(self):
        if self._held is not None:
            slot, stream = self._held
            ev = torch.cuda.Event()
            ev.record(stream)
            self._release[slot] = ev
            self._held = None

    def push(self, host_u8):
        full = self._source is not None and self._source.shape != self.shape
        src = _host_frame(host_u8, self.shape, self._source.shape if full else None)
        full = full and tuple(src.shape) == self._source.shape
        if self._pushed - self._popped >= self.depth:
            raise RuntimeError(f"FrameStream: {self.depth} frames are pushed and not popped: pop one first")
        slot = self._pushed % self.depth
        if self._held is not None and self._held[0] == slot:
            self._let_go()                           # depth 1, or a push before the next pop: the held view ends here
        if self._release[slot] is not None:
            self._release[slot].synchronize()        # the slot's consumer ran behind its upload: both are done
            self._release[slot] = None
        if not full:
            self._pinned[slot].copy_(src)
        with torch.cuda.stream(self._copy):
            if full:
                self._source.upload(slot, src, self._slots[slot])     # the slot's staging is free: its last resize ran before the release
            else:
                self._slots[slot].copy_(self._pinned[slot], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._copy)
        self._ready[slot] = ev
        self._pushed += 1

    def pop(self, stream=None):
        if self._popped >= self._pushed:
            raise RuntimeError("FrameStream: nothing pushed")
        stream = torch.cuda.current_stream(self.device) if stream is None else stream
        self._let_go()
        slot = self._popped % self.depth
        self._popped += 1
        stream.wait_event(self._ready[slot])
        self._held = (slot, stream)
        return self._slots[slot]
