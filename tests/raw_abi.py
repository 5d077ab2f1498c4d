"""Test-only driver of the rasterizer's C ABI (include/ex4d_rasterizer.h) on buffers the TEST owns.

`ex4dgs_amd._C` hands the library fresh `torch.empty` tensors: what a kernel finds in a word it reads before anybody wrote it is
whatever the caching allocator returns in that process.  Here every buffer the library writes -- the six forward outputs, the nine
(or twelve) gradients, the backward scratch, the three opaque state buffers, the status words of an asynchronous forward -- is a
view inside a larger byte tensor

    [ guard | payload | guard ]          guards >= 4096 bytes and a multiple of 256 (the payload keeps torch's 256-byte alignment)

whose payload AND guards are prefilled before the call:

    zero     bytes 0x00
    ones     bytes 0xFF: NaN as a float, -1 / 2^32-1 as an integer
    finite   bytes 0x3C: 0.0115 as a float (plausible, not NaN: accumulating onto garbage cannot hide behind NaN propagation)
    stale    nothing is touched: the buffers keep what the previous frame in this `Buffers` left; a buffer grows only when it is
             too small, keeping its old content in front, as torch's resize_ does

The driver returns the dictionaries of tests/helpers.py (gpu_forward_raw / gpu_backward_raw), so compare_forward / compare_backward
and the typed views of `_C` apply unchanged, and `Buffers.guards_intact()` reports, per buffer, whether a byte outside its payload
changed during the call."""
import ctypes as C

import torch

GUARD = 4096
FILL_BYTES = {"zero": 0x00, "ones": 0xFF, "finite": 0x3C}
FRESH_BYTE = 0x5A                   # what a grown buffer holds behind its old content (resize_ leaves that part uninitialised)
FILLS = ("zero", "ones", "finite", "stale")
FORWARD_OUTPUTS = ("color", "radii", "depth", "acc", "flow", "idx")
STATE_BUFFERS = ("geom", "binning", "img")
GRAD_NAMES = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations", "dL_ddir")
SPLIT_GRAD_NAMES = ("dL_dsh_dc_static", "dL_dsh_rest_static", "dL_dsh_dc_dynamic", "dL_dsh_rest_dynamic")

assert GUARD >= 4096 and GUARD % 256 == 0


def fill_word(fill, dtype=torch.int32):
    """The 32-bit pattern an element never written by the call still holds (None: `zero` and `stale` leave no recognisable one)."""
    if fill not in ("ones", "finite"):
        return None
    b = FILL_BYTES[fill]
    w = b | (b << 8) | (b << 16) | (b << 24)
    return w - (1 << 32) if w >= (1 << 31) else w


class Guarded:
    """One caller-owned buffer: [guard | payload | guard] inside `base`.  The payload starts GUARD bytes into the allocation; the
    trailing guard starts right behind the payload's last byte (not behind its alignment padding)."""

    def __init__(self, name, device):
        self.name, self.device = name, torch.device(device)
        self.base = None
        self.capacity = 0            # payload bytes the allocation has room for
        self.nbytes = 0              # payload bytes of the current frame
        self.requests = []           # byte counts asked for (allocation callbacks record theirs here)
        self._snap = None

    def prepare(self, nbytes, fill):
        """Make room for `nbytes` payload bytes, apply `fill` to payload and guards, remember the guards; returns the payload pointer."""
        nbytes = int(nbytes)
        self.requests.append(nbytes)
        if self.base is None or nbytes > self.capacity:
            cap = (nbytes + 255) // 256 * 256
            new = torch.full((GUARD + cap + GUARD,), FRESH_BYTE, dtype=torch.uint8, device=self.device)
            if self.base is not None:
                new[: GUARD + self.capacity] = self.base[: GUARD + self.capacity]          # resize_: the old content stays in front
            self.base, self.capacity = new, cap
        self.nbytes = nbytes
        if fill != "stale":
            self.base[: GUARD + nbytes + GUARD].fill_(FILL_BYTES[fill])
        assert self.device.type == "cpu" or self.base.data_ptr() % 256 == 0, "device allocation not 256-byte aligned (ex4d_alloc_fn promises that)"
        self._snap = (self.base[:GUARD].clone(), self.base[GUARD + nbytes: GUARD + nbytes + GUARD].clone())
        return self.ptr

    @property
    def ptr(self):
        return self.base.data_ptr() + GUARD

    @property
    def payload(self):
        return self.base[GUARD: GUARD + self.nbytes]

    def view(self, dtype, *shape):
        return self.payload.view(dtype).view(*shape)

    def guard_damage(self):
        """[] if no byte of either guard changed since prepare(), else [(which, first byte offset, count)]."""
        out = []
        for which, snap, now in (("front", self._snap[0], self.base[:GUARD]),
                                 ("back", self._snap[1], self.base[GUARD + self.nbytes: GUARD + self.nbytes + GUARD])):
            bad = (snap != now).nonzero()
            if bad.numel():
                out.append((which, int(bad[0]), int(bad.numel())))
        return out


class Buffers:
    """The buffers of one caller, by name; reused frame after frame (fill `stale`) like FrameTrainer's arenas and a replayed graph."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.by_name = {}
        self.touched = []            # names prepared by the most recent call

    def get(self, name):
        if name not in self.by_name:
            self.by_name[name] = Guarded(name, self.device)
        return self.by_name[name]

    def prepare(self, name, nbytes, fill):
        g = self.get(name)
        g.prepare(nbytes, fill)
        self.touched.append(name)
        return g

    def guards_intact(self, names=None):
        """{buffer name: True / list of damaged spans} for the buffers of the most recent call (or `names`)."""
        return {n: (self.by_name[n].guard_damage() or True) for n in (self.touched if names is None else names)}

    def assert_guards_intact(self, names=None):
        bad = {n: d for n, d in self.guards_intact(names).items() if d is not True}
        assert not bad, f"bytes outside the payload changed: {bad}"


def leftover_fill(t, fill, written=None):
    """Number of 32-bit elements of `t` that still hold the prefill pattern, i.e. that the call did not write.
    written (optional, same shape): what the same call writes there when its buffers held something else (the zero-fill run).  The
    `finite` pattern is an ordinary float (0.011489...): among the millions of elements of an image a value the call computes can
    have exactly these bits.  Such an element is not a leftover -- the call writes the same bits over zeros -- while an element the
    call never writes holds the pattern here and zero there, and is counted.  With `written` given as FLOATS that are reproducible to
    rounding only (the backward's atomics), an element counts unless the zero-fill run has a value within `close` of it."""
    w = fill_word(fill)
    if w is None or t.numel() == 0:
        return 0
    held = t.contiguous().view(torch.int32) == w
    if written is not None:
        ref = written.contiguous()
        if ref.dtype == torch.int32:
            held &= ref.view_as(held) != w
        else:
            x = t.contiguous().view(torch.float32)
            held &= ~((ref.view_as(x) - x).abs() <= 1e-4 * ref.abs().clamp_min(1e-30))
    return int(held.sum())


# ------------------------------------------------------------------------------------------------ the C ABI
def _dev(t, device):
    """contiguous float32 tensor on the device (kept alive by the caller) or None"""
    if t is None or t.numel() == 0:
        return None
    return t.to(device=device, dtype=torch.float32).contiguous()


def _p(t):
    return None if t is None else t.data_ptr()


def _split_parts(shs, n_static, offset=0):
    """[P,16,3] -> (dc static, rest static, dc dynamic, rest dynamic), each its own contiguous tensor (an empty part keeps 0 rows).
    offset: each part starts this many elements into its own allocation (4 * offset bytes behind torch's 256-byte alignment)."""
    parts = [shs[:n_static, :1].contiguous(), shs[:n_static, 1:].contiguous(), shs[n_static:, :1].contiguous(), shs[n_static:, 1:].contiguous()]
    if offset:
        parts = [_offset_view(torch.empty(p.numel() + offset, dtype=p.dtype, device=p.device), p.shape, offset).copy_(p) for p in parts]
    return parts


def _offset_view(flat, shape, offset):
    """The tensor of `shape` that starts `offset` elements into the 1-d tensor `flat`."""
    n = 1
    for d in shape:
        n *= d
    return flat[offset: offset + n].view(*shape)


def _split_struct(parts, n_static):
    from ex4dgs_amd import _C
    ptr = [p.data_ptr() if p.numel() else None for p in parts]
    return _C.Ex4dSplitSH((C.c_void_p * 2)(ptr[0], ptr[2]), (C.c_void_p * 2)(ptr[1], ptr[3]), int(n_static))


def forward(ins, settings, bufs, fill="zero", state_fill=None, subpixel_offset=None, prepare_backward=False, instance_capacity=0,
            assume_no_flow=False, n_static=None, split_offset=0, device="cuda"):
    """ex4d_forward / ex4d_forward_split_sh (n_static given: the SH tensor is passed as its four parts) with every buffer in `bufs`.
    fill: outputs (and the status words of an asynchronous forward); state_fill: the three state buffers (default: the same).
    split_offset: the four SH parts start this many floats into their allocations (_split_parts).
    Returns helpers.gpu_forward_raw's dictionary + rc / requested bytes / the Buffers."""
    from ex4dgs_amd import _C
    from tests import helpers as h
    lib = _C.load()
    state_fill = fill if state_fill is None else state_fill
    dev = torch.device(device)
    s = h.gpu_settings(settings, dev, subpixel_offset)
    t = {k: _dev(ins.get(k), dev) for k in ("means3D", "dir3D", "shs", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp")}
    cam = {k: _dev(getattr(s, k), dev) for k in ("bg", "viewmatrix", "projmatrix", "campos")}
    sub = _dev(s.subpixel_offset, dev)
    P, H, W = int(t["means3D"].shape[0]), int(s.image_height), int(s.image_width)
    split = n_static is not None
    M = 16 if split else (int(t["shs"].shape[1]) if t["shs"] is not None else 0)
    prm = _C._params(P, int(s.sh_degree), M, W, H, s.tanfovx, s.tanfovy, s.kernel_size, s.scale_modifier, s.min_depth, s.max_depth, s.prefiltered, s.debug,
                     prepare_backward, instance_capacity, assume_no_flow)
    bufs.touched = []
    shapes = dict(color=(torch.float32, (3, H, W)), radii=(torch.int32, (P,)), depth=(torch.float32, (1, H, W)), acc=(torch.float32, (1, H, W)),
                  flow=(torch.float32, (3, H, W)), idx=(torch.int32, (1, H, W)))
    out = {}
    for name, (dt, shape) in shapes.items():
        n = 4
        for d in shape:
            n *= d
        out[name] = bufs.prepare(name, n, fill).view(dt, *shape)
    asked = {}

    def alloc(name):
        def fn(_user, nbytes):
            asked[name] = int(nbytes)
            return bufs.prepare(name, nbytes, state_fill).ptr
        return _C.ALLOC_FN(fn)
    cbs = [alloc(n) for n in STATE_BUFFERS]
    count = C.c_int32(0)
    count_ref = C.byref(count)
    status = None
    if instance_capacity > 0:
        status = bufs.prepare("status", 32, fill)            # Ex4dFrameStatus in (guarded) device memory
        count_ref = C.cast(status.ptr, C.POINTER(C.c_int32))
    keep = None
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        tail = (cbs[0], None, cbs[1], None, cbs[2], None, out["color"].data_ptr(), out["radii"].data_ptr(), out["depth"].data_ptr(),
                out["acc"].data_ptr(), out["flow"].data_ptr(), out["idx"].data_ptr(), stream, count_ref)
        if split:
            keep = _split_parts(t["shs"], n_static, split_offset)
            st = _split_struct(keep, n_static)
            rc = lib.ex4d_forward_split_sh(C.byref(prm), _p(cam["bg"]), _p(t["means3D"]), _p(t["dir3D"]), C.byref(st), _p(t["opacities"]),
                                           _p(t["scales"]), _p(t["rotations"]), _p(t["cov3D_precomp"]), _p(cam["viewmatrix"]), _p(cam["projmatrix"]),
                                           _p(cam["campos"]), _p(sub), *tail)
        else:
            rc = lib.ex4d_forward(C.byref(prm), _p(cam["bg"]), _p(t["means3D"]), _p(t["dir3D"]), _p(t["shs"]), _p(t["colors_precomp"]), _p(t["opacities"]),
                                  _p(t["scales"]), _p(t["rotations"]), _p(t["cov3D_precomp"]), _p(cam["viewmatrix"]), _p(cam["projmatrix"]),
                                  _p(cam["campos"]), _p(sub), *tail)
        torch.cuda.synchronize()
    res = dict(rc=int(rc), error=lib.ex4d_last_error().decode(), settings=s, bufs=bufs, asked=asked, params=prm, inputs=t, camera=cam, subpixel=sub,
               n_static=n_static, split_parts=keep, **out)
    if rc != 0:
        return res
    if status is not None:
        words = status.view(torch.int32, 8).cpu()
        res["status"] = [int(x) & 0xFFFFFFFF for x in words]
        res["num_rendered"] = res["status"][0]
        res["layout_R"] = int(instance_capacity)             # the binning buffer is laid out for the capacity
    else:
        res["num_rendered"] = int(count.value)
        res["layout_R"] = int(count.value)
    res.update(geomBuffer=bufs.get("geom").payload, binningBuffer=bufs.get("binning").payload, imgBuffer=bufs.get("img").payload)
    res.update(_C.geom_views(res["geomBuffer"], P))
    res.update(_C.binning_views(res["binningBuffer"], res["layout_R"], W, H))
    res.update(_C.img_views(res["imgBuffer"], W, H))
    res["expected_bytes"] = dict(geom=int(lib.ex4d_geom_bytes(P)), binning=int(lib.ex4d_binning_bytes(res["layout_R"], W, H)), img=int(lib.ex4d_img_bytes(W, H)))
    return res


def backward(fwd, grads, bufs=None, fill="zero", prepared=False, null_outputs=(), null_grads=(), split_grad_offset=0, device="cuda"):
    """ex4d_backward / ex4d_backward_split_sh on the state a forward of this driver left (same inputs, same Buffers unless `bufs` is
    given).  fill: the gradient outputs and the scratch.  null_outputs: of ("dL_dcolors", "dL_dcov3D") passed as NULL;
    null_grads: indices 0..3 of the upstream gradients (colour, depth, flow, acc) passed as NULL.
    split_grad_offset: the four gradient parts of the split layout start this many floats into their (guarded, prefilled) payloads;
    the floats in front of them come back under "split_grad_lead".
    Returns helpers.gpu_backward_raw's dictionary (split SH: dL_dsh is the four parts concatenated back to [P,16,3], the parts
    themselves under SPLIT_GRAD_NAMES) + rc."""
    from ex4dgs_amd import _C
    lib = _C.load()
    bufs = fwd["bufs"] if bufs is None else bufs
    dev = torch.device(device)
    s, t, cam, prm0 = fwd["settings"], fwd["inputs"], fwd["camera"], fwd["params"]
    P, M, W, H = prm0.P, prm0.M, prm0.W, prm0.H
    prm = _C._params(P, prm0.D, M, W, H, s.tanfovx, s.tanfovy, s.kernel_size, s.scale_modifier, s.min_depth, s.max_depth, False, s.debug, prepared)
    up = [None if i in null_grads else _dev(g, dev) for i, g in enumerate(grads)]
    split = fwd["n_static"] is not None
    n_static = fwd["n_static"]
    shapes = dict(dL_dmeans2D=(P, 3), dL_dcolors=(P, 3), dL_dopacity=(P, 1), dL_dmeans3D=(P, 3), dL_dcov3D=(P, 6), dL_dsh=(P, M, 3),
                  dL_dscales=(P, 3), dL_drotations=(P, 4), dL_ddir=(P, 3))
    if split:
        del shapes["dL_dsh"]
        shapes.update(dL_dsh_dc_static=(n_static, 1, 3), dL_dsh_rest_static=(n_static, 15, 3), dL_dsh_dc_dynamic=(P - n_static, 1, 3),
                      dL_dsh_rest_dynamic=(P - n_static, 15, 3))
    bufs.touched = []
    out = {}
    for name, shape in shapes.items():
        if name in null_outputs:
            continue
        n = 4
        for d in shape:
            n *= d
        lead = split_grad_offset if name in SPLIT_GRAD_NAMES else 0
        out[name] = _offset_view(bufs.prepare(name, n + 4 * lead, fill).payload.view(torch.float32), shape, lead)
    scratch = bufs.prepare("scratch", int(lib.ex4d_backward_scratch_bytes(P)), fill)
    optr = lambda n: out[n].data_ptr() if (n in out and out[n].numel()) else None
    state = [bufs.get(n).ptr for n in STATE_BUFFERS]
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        mid = (_p(t["scales"]), _p(t["rotations"]), _p(t["cov3D_precomp"]), _p(cam["viewmatrix"]), _p(cam["projmatrix"]), _p(cam["campos"]),
               _p(fwd["subpixel"]), fwd["depth"].data_ptr(), fwd["acc"].data_ptr(), state[0], state[1], state[2],
               _p(up[0]), _p(up[1]), _p(up[2]), _p(up[3]),
               optr("dL_dmeans2D"), optr("dL_dcolors"), optr("dL_dopacity"), optr("dL_dmeans3D"), optr("dL_dcov3D"))
        tail = (optr("dL_dscales"), optr("dL_drotations"), optr("dL_ddir"), scratch.ptr, stream)
        if split:
            st = _split_struct(fwd["split_parts"], n_static)
            gparts = [out[n] for n in SPLIT_GRAD_NAMES]
            gst = _split_struct(gparts, n_static)
            rc = lib.ex4d_backward_split_sh(C.byref(prm), C.c_int32(fwd["layout_R"]), _p(cam["bg"]), _p(t["means3D"]), fwd["radii"].data_ptr(),
                                            C.byref(st), *mid, C.byref(gst), *tail)
        else:
            rc = lib.ex4d_backward(C.byref(prm), C.c_int32(fwd["layout_R"]), _p(cam["bg"]), _p(t["means3D"]), fwd["radii"].data_ptr(),
                                   _p(t["shs"]), _p(t["colors_precomp"]), *mid, optr("dL_dsh"), *tail)
        torch.cuda.synchronize()
    res = dict(rc=int(rc), error=lib.ex4d_last_error().decode(), bufs=bufs, written=dict(out), **out)
    if rc != 0:
        return res
    if split:
        res["split_grad_lead"] = {n: bufs.get(n).payload.view(torch.float32)[:split_grad_offset] for n in SPLIT_GRAD_NAMES}
        res["dL_dsh"] = torch.cat([torch.cat([out["dL_dsh_dc_static"], out["dL_dsh_rest_static"]], 1),
                                   torch.cat([out["dL_dsh_dc_dynamic"], out["dL_dsh_rest_dynamic"]], 1)], 0)
    e = torch.empty(0, dtype=torch.float32, device=dev)
    for n in ("dL_dcolors", "dL_dcov3D"):
        res.setdefault(n, e)
    res["acc16"] = scratch.payload[: P * 64].view(torch.float32).view(P, 16)
    return res
