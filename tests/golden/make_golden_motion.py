"""Generates tests/golden/motion.npz by importing the REFERENCE's CGaussianModel on the CPU (like make_golden_interp.py: third-party
modules stubbed, Tensor.cuda the identity): for every state and timestamp pair of tests/motion_ref.py the positions get_xyz_at_t gives
at both timestamps, in float32 and with the same reference code run in float64, and the autograd gradients (float64) of a fixed random
linear functional of the world displacement x(t1) - x(t0) and of the screen displacement.  The reference has no projection in Python:
the screen displacement is tests/motion_ref.screen_displacement applied to the reference getters' outputs, so the keyframe adjoints
are the reference's own (the pchip NaN pattern included; it is also recorded from a float32 run).

Run:  python tests/golden/make_golden_motion.py      (needs the reference checkout; byte-stable from run to run)
"""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from make_golden import _stub_modules  # noqa: E402
from make_golden_attr_states import save  # noqa: E402
from tests import motion_ref as mr  # noqa: E402


def model(P, interp, dtype):
    from scene.c_gaussian_model import CGaussianModel
    pc = CGaussianModel(3, mr.DURATION, mr.INTERVAL, mr.TIME_PAD, interp_type=interp, rot_interp_type="slerp", var_pad=mr.VAR_PAD)
    assert pc.time_shift == mr.time_shift(interp)
    for n in mr.NAMES:
        setattr(pc, n, torch.tensor(P[n]).to(dtype).requires_grad_(True))
    pc._rotation_motion = torch.zeros(P["_xyz_motion"].shape[0], P["_xyz_motion"].shape[1], 4, dtype=dtype)
    return pc


def capture(P, W, interp, K, cam):
    out = {}
    for name, (t0, t1) in mr.pairs(interp, K).items():
        base = mr.key(interp, K, name)
        for dtype, tag in ((torch.float32, ""), (torch.float64, "f64/")):
            pc = model(P, interp, dtype)
            leaves = [getattr(pc, n) for n in mr.NAMES]
            x0, x1 = pc.get_xyz_at_t(t0), pc.get_xyz_at_t(t1)
            assert x0.dtype == dtype and x0.shape == W.shape
            out[f"{base}/{tag}x0"], out[f"{base}/{tag}x1"] = x0.detach().numpy(), x1.detach().numpy()
            w = torch.tensor(W).to(dtype)
            for space, disp in (("world", x1 - x0), ("screen", mr.screen_displacement(x0, x1, cam)[0])):
                grads = torch.autograd.grad((disp * w).sum(), leaves, retain_graph=True)
                for n, g in zip(mr.NAMES, grads):
                    if dtype == torch.float64:
                        out[f"{base}/{space}/grad/{n}"] = g.numpy()
                    elif n == "_xyz_motion":
                        out[f"{base}/{space}/nan32"] = np.isnan(g.numpy())
    return out


def main():
    _stub_modules()
    torch.set_default_dtype(torch.float32)
    cam = mr.camera()
    out = {}
    for interp, K, Ns, Nd in mr.fixture_cases():
        P = mr.state(Ns, Nd, K)
        W = mr.functional(Ns + Nd)
        for n in mr.NAMES:
            out[f"{mr.key(interp, K)}/param/{n}"] = P[n]
        out[f"{mr.key(interp, K)}/weight"] = W
        arrays = capture(P, W, interp, K, cam)
        out.update(arrays)
        nan = sum(int(v.sum()) for k, v in arrays.items() if k.endswith("nan32"))
        print(f"{mr.key(interp, K)}: Ns {Ns}, Nd {Nd}, {len(mr.pairs(interp, K))} pairs, {nan} NaN keyframe gradients (float32 run)")
    path = os.path.join(OUT, "motion.npz")
    save(path, out)
    print("motion.npz:", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
