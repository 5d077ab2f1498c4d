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

Decoding and resizing stay with PIL on the host.  Plain events and two streams; no host threads.  No CPU fallback.
"""
import numpy as np
import torch


def gt_lut(im_scale=1.0):
    """float32 [256] CPU table: the value the reference's image tensor holds for each byte -- built with the torch ops the reference
    applies to the image itself (PILtoTorch's `/ 255.0`, im_reader's `/ im_scale` and `.clamp(0, 1)`), so lut[u8] is that tensor."""
    return (torch.arange(256, dtype=torch.uint8) / 255.0 / im_scale).clamp(0, 1)


def _host_frame(host_u8, shape):
    t = torch.from_numpy(host_u8) if isinstance(host_u8, np.ndarray) else host_u8
    if not isinstance(t, torch.Tensor) or t.device.type != "cpu" or t.dtype != torch.uint8 or tuple(t.shape) != shape:
        raise RuntimeError(f"a frame is a numpy array or a CPU torch tensor, uint8 {list(shape)}")
    return t


def _device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("frames live on a ROCm device (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


class FrameStore:
    """n_frames ground-truth frames resident on the device as one uint8 [N,H,W,S] allocation (frame i starts at byte i*H*W*S: odd for
    odd H*W at S = 3 -- the loss kernels take any alignment).  A store larger than free memory raises from the allocation."""
    STAGING = 2                  # pinned staging slots: the host copy of put n + 1 overlaps the upload of put n

    def __init__(self, n_frames, H, W, pixel_stride=3, device="cuda"):
        if pixel_stride not in (3, 4) or n_frames <= 0 or H <= 0 or W <= 0:
            raise RuntimeError("FrameStore: n_frames, H, W > 0 and pixel_stride 3 or 4")
        self.device = _device(device)
        self.shape = (int(H), int(W), int(pixel_stride))
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
        with it first."""
        src = _host_frame(host_u8, self.shape)
        slot = self._puts % self.STAGING
        self._puts += 1
        if self._staged[slot] is not None:
            self._staged[slot].synchronize()         # the upload that last used this pinned slot
        self._staging[slot].copy_(src)
        self._copy.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self._copy):
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

    def __init__(self, H, W, pixel_stride=3, depth=2, device="cuda"):
        if pixel_stride not in (3, 4) or depth < 1 or H <= 0 or W <= 0:
            raise RuntimeError("FrameStream: H, W > 0, pixel_stride 3 or 4, depth >= 1")
        self.device = _device(device)
        self.shape = (int(H), int(W), int(pixel_stride))
        self.depth = int(depth)
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
        src = _host_frame(host_u8, self.shape)
        if self._pushed - self._popped >= self.depth:
            raise RuntimeError(f"FrameStream: {self.depth} frames are pushed and not popped: pop one first")
        slot = self._pushed % self.depth
        if self._held is not None and self._held[0] == slot:
            self._let_go()                           # depth 1, or a push before the next pop: the held view ends here
        if self._release[slot] is not None:
            self._release[slot].synchronize()        # the slot's consumer ran behind its upload: both are done
            self._release[slot] = None
        self._pinned[slot].copy_(src)
        with torch.cuda.stream(self._copy):
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
