"""Times the fused inverse-depth loss (ex4dgs_amd.depth) at 1352 x 1014 on one GPU against the torch composition of the same loss on the
same GPU: decode (ex4dgs_amd.depth.decode_invdepth), mask, reciprocal, masked float64 moments, solve, residual, masked mean, and its
autograd graph with the fit detached.

Per operation the variants take turns in windows of at least a second between device events (ROUNDS windows each); the median window
is reported with its min / max.  Operations, L1, uint16 ground truth, with and without acc:
  fwd_given_*   the GIVEN forward's two launches into preallocated outputs        |  the composition's forward without the fit (no graph)
  fwd_fit_*     the FIT forward's four launches into preallocated outputs         |  the composition's forward with the fit (no graph)
  bwd_*         the backward's launch into a preallocated gradient (no counterpart: the composition has no backward of its own)
  grad_fit_*    forward + backward through depth.depth_loss                       |  forward + backward through the composition
fwd_fit - fwd_given is what the moments and solve launches add; the split between the four launches themselves needs a kernel trace.
Bytes moved are what the algorithm needs, from the shapes, per pixel and pass: 4 B of depth + 2 B of codes (+ 4 B of acc); the GIVEN
forward is one pass, the FIT forward two, the backward one pass + 4 B of gradient.  Share of peak = bytes / time / 8 TB/s.
Prints one JSON line; --out writes it to a file as well."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tools.dev.dev_flow_loss_time import PEAK, ROUNDS, WINDOW_S, H, W, measure        # noqa: E402  the windows of the flow loss's timing

CODE_SCALE, GIVEN = 2.0 ** -16, (1.1, 0.3)


def depth(torch, window_s):
    from ex4dgs_amd import depth as xdepth
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1)
    codes = torch.randint(1, 65536, (H, W), generator=gen)
    inv = (0.3 + 1.2 * codes / 65535.0 + 0.8 * (torch.rand(H, W, generator=gen) - 0.5)).clamp(0.02, 2.0)
    codes[torch.rand(H, W, generator=gen) < 0.15] = 0
    gt = (codes - 65536 * (codes >= 32768)).to(torch.int16).to(dev)           # the same bits as uint16
    out_depth = (1.0 / inv).to(torch.float32).reshape(1, H, W).to(dev)
    acc = torch.rand(1, H, W, generator=gen).to(dev)
    acc[0, ::7, ::5] = 0.0
    loss, row = torch.empty(1, device=dev), torch.empty(xdepth.ROW, dtype=torch.float64, device=dev)
    scratch, grad, g = xdepth.new_scratch(H, W, dev), torch.empty(1, H, W, device=dev), torch.ones(1, device=dev)
    leaf = out_depth.clone().requires_grad_(True)

    def composition(d, align, w):
        gv, m = xdepth.decode_invdepth(gt, CODE_SCALE)
        if w is not None:
            m = m & (w[0] > 0)
        x = 1.0 / d[0]
        n = m.sum().clamp(min=1)
        if align == "fit":
            g64, x64 = torch.where(m, gv, 0).double(), torch.where(m, x.detach(), 0).double()
            nd, Sg, Sx, Sgg, Sgx = n.double(), g64.sum(), x64.sum(), (g64 * g64).sum(), (g64 * x64).sum()
            det = nd * Sgg - Sg * Sg
            ok = (nd >= 2) & (det > 1e-10 * nd * Sgg)
            s = torch.where(ok, (nd * Sgx - Sg * Sx) / det, 0.0)
            o = ((Sx - s * Sg) / nd).float()
            s = s.float()
        else:
            s, o = GIVEN
        rho = (x - (s * gv + o)).abs()
        if w is not None:
            rho = rho * w.detach()[0]
        return torch.where(m, rho, torch.zeros_like(rho)).sum() / n

    def through(fn):
        leaf.grad = None
        fn().backward()

    ops, bytes_moved = {}, {}
    for w in (None, acc):
        tag = "acc" if w is not None else "noacc"
        for align in ("given", "fit"):
            mine = xdepth.depth_loss_raw(out_depth, gt, CODE_SCALE, align, *GIVEN, "l1", 0.0, w, loss=loss, row=row, scratch=scratch)[0].clone()
            theirs = composition(out_depth, align, w)
            err = float((mine[0] - theirs).abs() / theirs.abs())
            assert err < 1e-5, (tag, align, err)           # the two agree before they are timed
            ops[f"fwd_{align}_{tag}"] = {"kernel": (lambda align=align, w=w: xdepth.depth_loss_raw(out_depth, gt, CODE_SCALE, align, *GIVEN, "l1", 0.0, w, loss=loss, row=row, scratch=scratch)),
                                         "composition": (lambda align=align, w=w: composition(out_depth, align, w))}
        xdepth.depth_loss_raw(out_depth, gt, CODE_SCALE, "fit", *GIVEN, "l1", 0.0, w, loss=loss, row=row, scratch=scratch)       # the row the backward reads
        ops[f"bwd_{tag}"] = {"kernel": (lambda w=w: xdepth.depth_loss_backward_raw(out_depth, gt, row, g, CODE_SCALE, "fit", "l1", 0.0, w, out=grad))}
        ops[f"grad_fit_{tag}"] = {"kernel": (lambda w=w: through(lambda: xdepth.depth_loss(leaf, gt, CODE_SCALE, "fit", acc=w))),
                                  "composition": (lambda w=w: through(lambda: composition(leaf, "fit", w)))}
        one_pass = H * W * (4 + 2 + (4 if w is not None else 0))
        bytes_moved[f"fwd_given_{tag}"], bytes_moved[f"fwd_fit_{tag}"], bytes_moved[f"bwd_{tag}"] = one_pass, 2 * one_pass, one_pass + H * W * 4
    result = measure(torch, ops, window_s)
    for op, n in bytes_moved.items():
        result[op]["bytes"] = n
        result[op]["share_of_8TBps_peak"] = round(n / (result[op]["kernel"]["median_us"] * 1e-6) / PEAK, 4)
    for tag in ("noacc", "acc"):
        result[f"fwd_fit_{tag}"]["moments_and_solve_us"] = round(result[f"fwd_fit_{tag}"]["kernel"]["median_us"] - result[f"fwd_given_{tag}"]["kernel"]["median_us"], 2)
    return {"config": "cfg3 frame", "device": torch.cuda.get_device_name(0), "H": H, "W": W, "code_scale": CODE_SCALE, "given": GIVEN, "kind": "l1",
            "gt": "uint16", "window_s": window_s, "rounds": ROUNDS, "per_launch_split": "not measured (no kernel trace was taken)", "us_per_call": result}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_loss_time_cfg3.json"))
    ap.add_argument("--window", type=float, default=WINDOW_S)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    doc = depth(torch, a.window)
    print(json.dumps(doc))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fp:
        fp.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
