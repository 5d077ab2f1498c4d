"""Times the fused flow loss (ex4dgs_amd.flow) at 1352 x 1014 on one GPU against the torch composition of the same loss on the same
GPU: decode (ex4dgs_amd.flow.decode_flow), mask, norm, masked mean, and its autograd graph.

Per operation the variants take turns in windows of at least a second between device events (ROUNDS windows each); the median window
is reported with its min / max.  Operations, for both kinds, with and without acc:
  fwd_*      the forward's two launches into preallocated outputs  |  the composition's forward (no graph)
  bwd_*      the backward's launch into a preallocated gradient (no counterpart: the composition has no backward of its own)
  grad_*     forward + backward through flow.flow_loss  |  forward + backward through the composition
Bytes moved are what the algorithm needs, from the shapes, per pixel: forward 8 B of flow + 6 B of codes (+ 4 B of acc); backward the
same reads + 12 B of gradient.  Share of peak = bytes / time / 8 TB/s.

--l1-ssim-lib PATH: instead, times ex4d_l1_ssim_forward / _backward of the library at PATH (bound with ctypes here, so that a build
without the flow entry points loads too) -- run in alternating processes on two builds, it shows whether the training loss, which
shares the header, moved.  Prints one JSON line; --out writes it to a file as well."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

WINDOW_S, ROUNDS, H, W, PEAK, EPS, SCALE = 1.0, 3, 1014, 1352, 8e12, 1e-3, 0.5


def window(torch, fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches          # us per call


def measure(torch, ops, window_s):
    result = {}
    for op, variants in ops.items():
        row, launches = {}, {}
        for v, fn in variants.items():
            window(torch, fn, 5)                          # warm-up
            launches[v] = int(window_s * 1e6 / window(torch, fn, 50)) + 1
        ts = {v: [] for v in variants}
        for _ in range(ROUNDS):
            for v, fn in variants.items():                # the variants alternate
                ts[v].append(window(torch, fn, launches[v]))
        for v, t in ts.items():
            row[v] = {"median_us": round(sorted(t)[len(t) // 2], 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2),
                      "launches_per_window": launches[v]}
        if "composition" in row:
            row["composition_over_kernel"] = round(row["composition"]["median_us"] / row["kernel"]["median_us"], 2)
        result[op] = row
    return result


def l1_ssim(torch, path, window_s):
    """ex4d_l1_ssim_forward / _backward of the library at `path`, float ground truth, lambda 0.2."""
    from ex4dgs_amd.loss import gaussian_window
    lib = ctypes.CDLL(path)
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float
    lib.ex4d_l1_ssim_scratch_floats.restype, lib.ex4d_l1_ssim_scratch_floats.argtypes = ctypes.c_size_t, [i32, i32]
    lib.ex4d_l1_ssim_forward.argtypes = [i32, i32, i32, vp, vp, f32] + [vp] * 7
    lib.ex4d_l1_ssim_backward.argtypes = [i32, i32, i32, vp, vp, f32] + [vp] * 5
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(2)
    img, gt = torch.rand(3, H, W, generator=gen).to(dev), torch.rand(3, H, W, generator=gen).to(dev)
    f = dict(dtype=torch.float32, device=dev)
    loss, l1e, sse, dmaps = torch.empty(1, **f), torch.empty(H, W, **f), torch.empty(H, W, **f), torch.empty(3, 3, H, W, **f)
    scratch, g, grad = torch.empty(lib.ex4d_l1_ssim_scratch_floats(H, W), **f), torch.ones(1, **f), torch.empty(3, H, W, **f)
    taps = gaussian_window()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fwd():
        assert lib.ex4d_l1_ssim_forward(3, H, W, img.data_ptr(), gt.data_ptr(), 0.2, taps.ctypes.data, loss.data_ptr(), l1e.data_ptr(), sse.data_ptr(),
                                        dmaps.data_ptr(), scratch.data_ptr(), stream) == 0

    def bwd():
        assert lib.ex4d_l1_ssim_backward(3, H, W, img.data_ptr(), gt.data_ptr(), 0.2, taps.ctypes.data, dmaps.data_ptr(), g.data_ptr(), grad.data_ptr(),
                                         stream) == 0

    fwd()
    return measure(torch, {"l1_ssim_fwd": {"kernel": fwd}, "l1_ssim_bwd": {"kernel": bwd}}, window_s), float(loss.cpu()[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--window", type=float, default=WINDOW_S)
    ap.add_argument("--l1-ssim-lib")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    if a.l1_ssim_lib:
        result, loss = l1_ssim(torch, a.l1_ssim_lib, a.window)
        doc = {"library": a.l1_ssim_lib, "H": H, "W": W, "loss": loss, "window_s": a.window, "rounds": ROUNDS, "us_per_call": result}
    else:
        doc = flow(torch, a.window)
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(json.dumps(doc, indent=1) + "\n")


def flow(torch, window_s):
    from ex4dgs_amd import flow as xflow
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1)
    words = torch.empty(H, W, 3, dtype=torch.int32)
    words[..., :2] = torch.randint(32768 - 2560, 32768 + 2560, (H, W, 2), generator=gen)
    words[..., 2] = torch.where(torch.rand(H, W, generator=gen) < 0.7, torch.randint(32769, 65536, (H, W), generator=gen), torch.randint(0, 32769, (H, W), generator=gen))
    enc = (words - 65536 * (words >= 32768)).to(torch.int16).to(dev)          # the same bits as uint16
    out_flow = (torch.randn(3, H, W, generator=gen) * 3).to(dev)
    acc = torch.rand(1, H, W, generator=gen).to(dev)
    loss, row = torch.empty(1, device=dev), torch.empty(4, dtype=torch.float64, device=dev)
    scratch, grad, g = xflow.new_scratch(H, W, dev), torch.empty(3, H, W, device=dev), torch.ones(1, device=dev)
    leaf = out_flow.clone().requires_grad_(True)

    def composition(x, kind, w):
        gt, m = xflow.decode_flow(enc, SCALE)
        r = x[:2] - gt.permute(2, 0, 1)
        rho = r.abs().sum(0) if kind == "l1" else (r.pow(2).sum(0) + EPS ** 2).sqrt()
        if w is not None:
            rho = rho * w.detach()[0]
        return torch.where(m > 0, rho, torch.zeros_like(rho)).sum() / m.sum().clamp(min=1)

    def through(fn):
        leaf.grad = None
        fn().backward()

    ops, bytes_moved = {}, {}
    for kind in ("l1", "charbonnier"):
        for w in (None, acc):
            tag = f"{kind}_{'acc' if w is not None else 'noacc'}"
            mine = xflow.flow_loss_raw(out_flow, enc, SCALE, kind, EPS, w, loss=loss, row=row, scratch=scratch)[0].clone()
            theirs = composition(out_flow, kind, w)
            err = float((mine[0] - theirs).abs() / theirs.abs())
            assert err < 1e-5, (tag, err)                  # the two agree before they are timed
            ops[f"fwd_{tag}"] = {"kernel": (lambda kind=kind, w=w: xflow.flow_loss_raw(out_flow, enc, SCALE, kind, EPS, w, loss=loss, row=row, scratch=scratch)),
                                 "composition": (lambda kind=kind, w=w: composition(out_flow, kind, w))}
            ops[f"bwd_{tag}"] = {"kernel": (lambda kind=kind, w=w: xflow.flow_loss_backward_raw(out_flow, enc, row, g, SCALE, kind, EPS, w, out=grad))}
            ops[f"grad_{tag}"] = {"kernel": (lambda kind=kind, w=w: through(lambda: xflow.flow_loss(leaf, enc, SCALE, kind, EPS, w))),
                                  "composition": (lambda kind=kind, w=w: through(lambda: composition(leaf, kind, w)))}
            read = H * W * (8 + 6 + (4 if w is not None else 0))
            bytes_moved[f"fwd_{tag}"], bytes_moved[f"bwd_{tag}"] = read, read + H * W * 12
    result = measure(torch, ops, window_s)
    for op, n in bytes_moved.items():
        result[op]["bytes"] = n
        result[op]["share_of_8TBps_peak"] = round(n / (result[op]["kernel"]["median_us"] * 1e-6) / PEAK, 4)
    return {"config": "cfg3 frame", "device": torch.cuda.get_device_name(0), "H": H, "W": W, "flow_scale": SCALE, "eps": EPS,
            "window_s": window_s, "rounds": ROUNDS, "us_per_call": result}


if __name__ == "__main__":
    main()
