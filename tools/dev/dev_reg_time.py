"""Times the motion regularisers at config 3 (1.0 M Gaussians, Nd = 200 k dynamic, K = 35) on one GPU:
  * ex4d_radam_step_sliced on the two keyframe tensors (no regularisers: the baseline),
  * ex4d_radam_step_sliced_reg with motion_reg + rot_reg on the same tensors (bytes, fraction of the 8 TB/s HBM peak),
  * what a user pays without it: forward + autograd backward of the three terms in torch, and the dense keyframe step
    (zero fill + the terms' gradients added + ex4d_radam_step over dense keyframe gradients),
  * ex4d_reg_forward / ex4d_reg_backward alone, and a FrameTrainer iteration without / with regularisers (sliced and dense).
The two optimizer steps are timed alternately in rounds of 50 launches between device events (200 launches each after warm-up).
Prints one JSON line."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ex4dgs_amd import optim, regularizers as reg  # noqa: E402
from ex4dgs_amd.loss import l1_ssim_loss  # noqa: E402
from ex4dgs_amd.scene import make_scene  # noqa: E402
from ex4dgs_amd.trainer import FrameTrainer  # noqa: E402

PEAK = 8.0e12
W3 = (1e-4, 1e-4, 1e-3)
BETAS, EPS = (0.9, 0.999), 1e-8


def torch_terms(d, m, r, w):
    """The three terms in plain torch, from the formulas of include/ex4d_regularizers.h."""
    loss = w[0] * torch.log(d.norm(dim=-1) + 0.001).mean()
    loss = loss + w[1] * (m[:, :1] - m[:, 1:]).norm(dim=-1).mean()
    a, b = r[:, 1:], r[:, :-1]
    return loss + w[2] * (1 - (a * b).sum(dim=-1) / a.norm(dim=-1).clamp_min(1e-6) / b.norm(dim=-1).clamp_min(1e-6)).mean()


def events_us(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def alternate(fns, rounds=4, launches=50):
    """Median over `rounds` of each fn's time per launch, the fns taking turns (same thermal / clock state for all)."""
    for fn in fns:
        events_us(fn, 10)
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            ts[i].append(events_us(fn, launches))
    return [sorted(t)[len(t) // 2] for t in ts], [(min(t), max(t)) for t in ts]


def main():
    dev = torch.device("cuda:0")
    model, cam, bg = make_scene("cfg3", device=dev, fused=True)
    cam, bg = cam.to(dev), bg.to(dev)
    Ns, Nd, K = model.num_static, model.num_dynamic, model._xyz_motion.shape[1]
    d, m, r = model._xyz_disp, model._xyz_motion.clone(), model._rotation_motion.clone()
    mom = [torch.zeros_like(t) for t in (m, m, r, r)]
    wx, wr = 1e-4 * torch.randn(Nd, 4, 3, device=dev), 1e-4 * torch.randn(Nd, 2, 4, device=dev)
    step = [10]

    def items(with_reg):
        tail = lambda kind, w: (None, kind, w, Nd) if with_reg else ()
        return [(m.data_ptr(), mom[0].data_ptr(), mom[1].data_ptr(), Nd, K, 3, 1.6e-4, step[0], [(5, 4, wx.data_ptr())]) + tail(optim.REG_MOTION, W3[1]),
                (r.data_ptr(), mom[2].data_ptr(), mom[3].data_ptr(), Nd, K, 4, 1e-3, step[0], [(9, 2, wr.data_ptr())]) + tail(optim.REG_ROT, W3[2])]
    plain = lambda: optim.radam_step_sliced_raw(items(False), BETAS, EPS, dev)
    fused = lambda: optim.radam_step_sliced_reg_raw(items(True), BETAS, EPS, dev)
    (plain_us, fused_us), spread = alternate([plain, fused])
    elems = Nd * K * 7
    step_bytes = 24 * elems + 4 * (wx.numel() + wr.numel())

    # the stand-alone op
    out4, scratch = torch.empty(4, device=dev), reg.new_scratch(dev)
    gd, gm, gr = torch.zeros_like(d), torch.zeros_like(m), torch.zeros_like(r)
    fwd_us = events_us(lambda: reg.forward_raw(d, m, r, W3, out=out4, scratch=scratch), 200)
    bwd_us = events_us(lambda: reg.backward_raw(d, m, r, W3, (gd, gm, gr), accumulate=True), 200)
    bwd_disp_us = events_us(lambda: reg.backward_raw(d, None, None, W3, (gd, None, None), accumulate=True), 200)

    # what a user pays today: the torch composition (forward + autograd backward) ...
    leaves = [t.detach().clone().requires_grad_(True) for t in (d, m, r)]

    def torch_fb():
        return torch.autograd.grad(torch_terms(*leaves, W3), leaves)
    for _ in range(3):
        torch_fb()
    torch_us = events_us(torch_fb, 30)
    # ... and dense keyframe gradients through the optimizer: zero fill (what the dense attribute backward starts with), the terms'
    # gradients added, ex4d_radam_step over 28 B per element
    tg = torch_fb()

    def dense_step():
        gm.zero_(); gr.zero_()
        gm[:, 5:9] += wx; gr[:, 9:11] += wr
        gm.add_(tg[1]); gr.add_(tg[2])
        optim.radam_step_raw([(m.data_ptr(), gm.data_ptr(), mom[0].data_ptr(), mom[1].data_ptr(), m.numel(), 1.6e-4, step[0]),
                              (r.data_ptr(), gr.data_ptr(), mom[2].data_ptr(), mom[3].data_ptr(), r.numel(), 1e-3, step[0])], BETAS, EPS, dev)
    dense_step()
    dense_us = events_us(dense_step, 100)

    # a FrameTrainer iteration (render + L1/SSIM + backward + optimizer) without / with regularisers
    gt = torch.rand(3, cam.image_height, cam.image_width, device=dev)
    upg = lambda o: ([l1_ssim_loss(o["render"], gt, 0.2)[0]], [None])
    iters = {}
    for name, kw in (("off", {}), ("sliced", dict(regularizers=W3)), ("dense", dict(regularizers=W3, sliced=False))):
        mdl, _, _ = make_scene("cfg3", device=dev, fused=True)
        tr = FrameTrainer(mdl, optimizer=True, **kw)
        ts = [(17 * i) % 300 for i in range(40)]
        for t in ts[:8]:
            tr.step(cam, bg, t, upg)
        tr.flush(); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in ts[8:]:
            tr.step(cam, bg, t, upg)
        tr.flush()
        e1.record(); torch.cuda.synchronize()
        iters[name] = e0.elapsed_time(e1) / len(ts[8:])
        del tr, mdl
    print(json.dumps({
        "config": "cfg3", "static": Ns, "dynamic": Nd, "K": K, "device": torch.cuda.get_device_name(0), "weights": W3,
        "sliced_step_us": round(plain_us, 2), "sliced_step_min_max_us": [round(x, 2) for x in spread[0]],
        "sliced_reg_step_us": round(fused_us, 2), "sliced_reg_step_min_max_us": [round(x, 2) for x in spread[1]],
        "step_bytes": step_bytes, "sliced_step_hbm_fraction": round(step_bytes / (plain_us * 1e-6) / PEAK, 3),
        "sliced_reg_step_hbm_fraction": round(step_bytes / (fused_us * 1e-6) / PEAK, 3),
        "ratio_reg_over_plain": round(fused_us / plain_us, 3),
        "reg_forward_us": round(fwd_us, 2), "reg_backward_all_us": round(bwd_us, 2), "reg_backward_xyz_disp_us": round(bwd_disp_us, 2),
        "torch_composition_fwd_bwd_us": round(torch_us, 1), "dense_keyframe_step_us": round(dense_us, 1),
        "user_today_us": round(torch_us + dense_us, 1),
        "condition_fused_not_slower_than_plain_plus_torch": bool(fused_us <= plain_us + torch_us),
        "frame_trainer_iteration_ms": {k: round(v, 3) for k, v in iters.items()}}))


if __name__ == "__main__":
    main()
