"""Captures tests/golden/regularizers.npz from the reference checkout: what the reference's OWN regularisation lines compute.

    python tests/golden/make_golden_regularizers.py /path/to/reference

Nothing of the reference is copied: train.py is read at capture time, the block from `# Regularization` up to `loss.backward()` is
cut out, dedented, compiled and executed with `opt`, `iteration`, `gaussians` (a namespace of parameters), `loss` and `torch`
supplied.  Runs on the CPU.  Recorded:
  * probe model (Ns 256, Nd 40, K 35, all three terms live, edge rows): inputs, loss and autograd gradients in float32 and float64;
  * the loss either side of every gate of the three `if`s (iteration thresholds, weight 0, no dynamic Gaussians);
  * an 8-step trajectory: loss = the block + sum(window * slice) with stored random windows, torch.optim.RAdam with the reference's
    learning rates, parameters after every step.
"""
import os
import sys
import textwrap
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "regularizers.npz")
LRS = {"_xyz_disp": 0.0001, "_xyz_motion": 0.00016, "_rotation_motion": 0.001}      # c_gaussian_model.py:430-447, spatial_lr_scale 1


def reference_block(ref):
    src = open(os.path.join(ref, "train.py")).read()
    lines = src.splitlines()
    start = [i for i, l in enumerate(lines) if l.strip() == "# Regularization"]
    assert len(start) == 1, "anchor `# Regularization` not found exactly once in the reference's train.py"
    end = [i for i, l in enumerate(lines) if i > start[0] and l.strip() == "loss.backward()"]
    assert end, "anchor `loss.backward()` not found after the regularisation block"
    block = textwrap.dedent("\n".join(lines[start[0]:end[0]]))
    assert "static_reg" in block and "motion_reg" in block and "rot_reg" in block
    return compile(block, "reference_train_regularization", "exec")


def run_block(code, opt, iteration, params, dtype):
    g = types.SimpleNamespace(**params)
    env = {"opt": opt, "iteration": iteration, "gaussians": g, "loss": torch.zeros((), dtype=dtype), "torch": torch}
    exec(code, env)
    return env["loss"]


def make_opt(**kw):
    base = dict(static_reg=1e-4, motion_reg=1e-4, rot_reg=1e-3, progressive_growing_steps=300, make_dynamic_interval=100, extract_every=1)
    base.update(kw)
    return types.SimpleNamespace(**base)


def make_model(seed, Ns, Nd, K, edges):
    g = torch.Generator().manual_seed(seed)
    disp = 0.02 * torch.randn(Ns, 3, generator=g)
    motion = torch.randn(Nd, 1, 3, generator=g) + torch.cumsum(0.05 * torch.randn(Nd, K, 3, generator=g), 1)      # a random walk per Gaussian
    rot = torch.nn.functional.normalize(torch.randn(Nd, 1, 4, generator=g) + torch.cumsum(0.1 * torch.randn(Nd, K, 4, generator=g), 1), dim=-1)
    rot = rot * (1 + 0.05 * torch.randn(Nd, K, 1, generator=g))
    if edges:
        disp[3] = 0                                   # norm 0: gradient 0
        motion[5] = motion[5, :1]                     # every keyframe equals keyframe 0
        motion[6, 7] = motion[6, 0]                   # one keyframe equals keyframe 0
        rot[2, 9] = 0                                 # a zero keyframe between unit ones
        rot[4, 0] = 0                                 # ... at the start of the row
        rot[7, K - 1] = rot[7, K - 1] / rot[7, K - 1].norm() * 1e-8      # norm below the clamp
    return {"_xyz_disp": disp.contiguous(), "_xyz_motion": motion.contiguous(), "_rotation_motion": rot.contiguous()}


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("EX4D_REFERENCE", "")
    assert ref and os.path.exists(os.path.join(ref, "train.py")), "usage: make_golden_regularizers.py <reference checkout>"
    code = reference_block(ref)
    torch.set_num_threads(1)
    out = {}

    # ---- probe model
    opt = make_opt()
    base = make_model(1, 256, 40, 35, edges=True)
    out["probe_weights"] = np.array([opt.static_reg, opt.motion_reg, opt.rot_reg], np.float64)
    for n, v in base.items():
        out["probe" + n] = v.numpy()
    for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        params = {n: v.to(dtype).clone().requires_grad_(True) for n, v in base.items()}
        loss = run_block(code, opt, 1000, params, dtype)
        loss.backward()
        out["probe_loss_" + tag] = loss.detach().numpy()
        for n, v in params.items():
            out[f"probe_grad{n}_{tag}"] = v.grad.numpy()
    # the three terms one at a time, float64 (the unweighted means follow by division)
    for i, name in enumerate(("static_reg", "motion_reg", "rot_reg")):
        o = make_opt(**{k: (getattr(opt, k) if k == name else 0.0) for k in ("static_reg", "motion_reg", "rot_reg")})
        params = {n: v.double() for n, v in base.items()}
        out["probe_mean_" + name] = (run_block(code, o, 1000, params, torch.float64) / getattr(opt, name)).numpy()

    # ---- gates
    small = {n: v.double() for n, v in make_model(2, 16, 6, 5, edges=False).items()}
    empty = dict(small, _xyz_motion=torch.zeros(0, 5, 3, dtype=torch.float64), _rotation_motion=torch.zeros(0, 5, 4, dtype=torch.float64))
    for n, v in small.items():
        out["gate" + n] = v.numpy()
    cases = []
    for it in (399, 400, 401, 402):
        cases.append((dict(), it, 6))
    for it in (399, 400, 401, 699, 700, 701):
        cases.append((dict(extract_every=2), it, 6))
    for name in ("static_reg", "motion_reg", "rot_reg"):
        cases.append(({name: 0.0}, 1000, 6))
    cases.append((dict(), 1000, 0))
    rows, losses = [], []
    for kw, it, nd in cases:
        o = make_opt(**kw)
        losses.append(float(run_block(code, o, it, small if nd else empty, torch.float64)))
        rows.append([o.static_reg, o.motion_reg, o.rot_reg, o.progressive_growing_steps, o.make_dynamic_interval, o.extract_every, it, nd])
    out["gate_cases"] = np.array(rows, np.float64)
    out["gate_loss"] = np.array(losses, np.float64)

    # ---- trajectory
    steps, Ns, Nd, K = 8, 64, 24, 35
    params = {n: v.clone().requires_grad_(True) for n, v in make_model(3, Ns, Nd, K, edges=False).items()}
    for n, v in params.items():
        out["traj_init" + n] = v.detach().numpy().copy()
    optim = torch.optim.RAdam([{"params": [v], "lr": LRS[n], "name": n} for n, v in params.items()], lr=0.001)
    g = torch.Generator().manual_seed(4)
    firsts, wx, wr = [], [], []
    traj = {n: [] for n in params}
    for s in range(steps):
        fx, fr = int(torch.randint(0, K - 3, (1,), generator=g)), int(torch.randint(0, K - 1, (1,), generator=g))
        gx, gr = 1e-4 * torch.randn(Nd, 4, 3, generator=g), 1e-4 * torch.randn(Nd, 2, 4, generator=g)
        firsts.append([fx, fr]); wx.append(gx.numpy()); wr.append(gr.numpy())
        optim.zero_grad(set_to_none=True)
        loss = run_block(code, opt, 1000 + s, params, torch.float32)
        loss = loss + (params["_xyz_motion"][:, fx:fx + 4] * gx).sum() + (params["_rotation_motion"][:, fr:fr + 2] * gr).sum()
        loss.backward()
        optim.step()
        for n, v in params.items():
            traj[n].append(v.detach().numpy().copy())
    out["traj_first"] = np.array(firsts, np.int32)
    out["traj_window_xyz"] = np.stack(wx)
    out["traj_window_rot"] = np.stack(wr)
    out["traj_weights"] = out["probe_weights"]
    out["traj_lrs"] = np.array([LRS[n] for n in params], np.float64)
    for n, v in traj.items():
        out["traj" + n] = np.stack(v)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
