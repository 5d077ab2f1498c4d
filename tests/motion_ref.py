"""Shared by tests/golden/make_golden_motion.py, tests/test_cpu_motion.py and tests/test_gpu_motion.py: the states, camera, timestamp
pairs and the layout of tests/golden/motion.npz, and a float64 torch restatement of what ex4dgs_amd.motion computes -- the three
position interpolators (operation order of utils/interpolations.py of the reference), the projection of the rasterizer's preprocess
(full projection, inv_w = 1 / (w + 1e-7f), ndc2Pix) and the depth rule (a row at or behind `near` at either timestamp is zero and gets
zero gradients).  Gradients are torch autograd of that restatement.

Time numbers: duration 50, interval 5, time_pad 3; time_shift = 3 for linear, 8 for cube and pchip.  K = 12, and the interpolator's
minimum (4; linear 2).  Valid keyframe indices: 1 .. K-3 (linear 0 .. K-2).

Timestamp pairs at K = 12 (k, delta of t0 -> of t1; hermite = cube, pchip):
  same        hermite (0.5, 1.5)   k 1 -> 1            linear (0.5, 1.5)   k 0 -> 0         windows coincide; the first valid index
  adjacent    hermite (1.5, 4.5)   k 1 -> 2            linear (1.5, 4.5)   k 0 -> 1         windows overlap in 3 slices (linear 1)
  far         hermite (0, 30.5)    k 1 -> 7            linear (0, 40.5)    k 0 -> 8         windows disjoint
  equal       (4.5, 4.5)                                                                    t0 == t1
  reverse     hermite (21, 13.25)  k 5 -> 4            linear (21, 13.25)  k 4 -> 3         t1 < t0
  ends        hermite (-3, 41.5)   k 1, delta 0 -> 9   linear (-3, 51.5)   k 0, delta 0 -> 10   first and last valid index
  knots       (7, 2)               delta == 0 exactly at both timestamps
and at the minimum K, whose only valid index admits t in [-3, 2): (-3, 1.5), (0.5, 0.5), (1.5, -1).
"""
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "motion.npz")
DURATION, INTERVAL, TIME_PAD, VAR_PAD, NEAR = 50, 5, 3, 3, 0.2
INTERPS = ("cube", "linear", "pchip")
K_MANY = 12
GRAD_BAR = 1e-5                       # the README parity row: 1e-5 * max(1, |reference|inf) per tensor
W_IMG, H_IMG = 96, 64
NAMES = ("_xyz", "_xyz_disp", "_xyz_motion")
EPS_W = float(np.float32(0.0000001))


def time_shift(interp):
    return TIME_PAD if interp == "linear" else TIME_PAD + INTERVAL


def k_min(interp):
    return 2 if interp == "linear" else 4


def pairs(interp, K):
    """{name: (t0, t1)}"""
    if K == k_min(interp):
        return {"min_a": (-3, 1.5), "min_equal": (0.5, 0.5), "min_reverse": (1.5, -1)}
    return {"same": (0.5, 1.5), "adjacent": (1.5, 4.5), "far": (0, 40.5 if interp == "linear" else 30.5), "equal": (4.5, 4.5), "reverse": (21, 13.25),
            "ends": (-3, 51.5 if interp == "linear" else 41.5), "knots": (7, 2)}


def time_index(interp, t):
    tp = t + time_shift(interp)
    return int(tp // INTERVAL), (tp % INTERVAL) / INTERVAL


def window(interp, t):
    """(first keyframe, count) of the position window of t."""
    k = time_index(interp, t)[0]
    return (k, 2) if interp == "linear" else (k - 1, 4)


def model_kwargs(interp):
    """Keyword arguments of ex4dgs_amd.motion.displacement / attributes.evaluate_attributes for these time numbers."""
    return dict(interp_type=interp, duration=DURATION, interval=INTERVAL, time_shift=time_shift(interp), var_pad=VAR_PAD)


# ---------------------------------------------------------------------------------------------- states and camera
def camera():
    """96 x 64, 60 degrees across, turned 0.15 rad about y and shifted: every matrix entry the projection reads is in play."""
    from ex4dgs_amd.scene import make_camera
    a = 0.15
    R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    fovx = math.radians(60)
    fovy = 2 * math.atan(math.tan(fovx / 2) * H_IMG / W_IMG)
    return make_camera(W_IMG, H_IMG, fovx, fovy, R=R, T=np.array([0.2, -0.1, 0.3]))


def state(Ns, Nd, K, seed=0):
    """The 15 parameter tensors (float32 numpy) of a scene in front of camera().  Static row i, dynamic row j, by class:
      i % 8 == 7   behind the camera at every t             i % 8 == 6   at z = 0.3 with a disp that carries it behind `near`
      j % 10 == 5  a constant track (pchip: s == 0, NaN gradients)
      j % 10 == 6  z ramps from behind the camera to far in front over the keyframes      j % 10 == 7  the reverse ramp
      j % 10 == 8  behind at every t                        j % 10 == 9  x ramps out of the frustum
    everything else: 3 <= z <= 8 inside the frustum, a random walk of 0.15 per keyframe."""
    rng = np.random.default_rng(1000 + 7 * seed + Ns * 13 + Nd * 131 + K)
    N, U = rng.standard_normal, rng.random

    def start(n):
        z = 3 + 5 * U(n)
        return np.stack([(U(n) - 0.5) * 0.9 * z, (U(n) - 0.5) * 0.4 * z, z], 1)

    xyz, disp = start(Ns), 0.5 * N((Ns, 3))
    i = np.arange(Ns)
    xyz[i % 8 == 7, 2] = -1.0 - U(int((i % 8 == 7).sum()))
    cross = i % 8 == 6
    xyz[cross, 2] = 0.3
    disp[cross, 2] = -1.0 - U(int(cross.sum()))
    y = start(Nd)[:, None, :] + np.cumsum(0.15 * N((Nd, K, 3)), 1)
    j = np.arange(Nd)
    ramp = np.linspace(0, 1, K)[None, :]
    y[j % 10 == 5] = y[j % 10 == 5][:, :1]
    y[j % 10 == 6, :, 2] = (-3 + 9 * ramp) + 0.01 * N((int((j % 10 == 6).sum()), K))
    y[j % 10 == 7, :, 2] = (6 - 9 * ramp) + 0.01 * N((int((j % 10 == 7).sum()), K))
    y[j % 10 == 8, :, 2] = -2.0 + 0.1 * N((int((j % 10 == 8).sum()), K))
    y[j % 10 == 9, :, 0] += 6 * y[j % 10 == 9, :, 2] * ramp
    P = dict(_xyz=xyz, _xyz_disp=disp, _rotation=N((Ns, 4)), _opacity=N((Ns, 1)), _scaling=0.3 * N((Ns, 3)) - 2.5,
             _features_dc=N((Ns, 1, 3)), _features_rest=0.1 * N((Ns, 15, 3)),
             _xyz_motion=y, _rotation_motion=N((Nd, K, 4)), _opacity_motion=N((Nd, 1)),
             _opacity_duration_center=np.sort(1 + U((Nd, 2, 1)) * (K - 2), 1), _opacity_duration_var=N((Nd, 2, 1)),
             _scaling_motion=0.3 * N((Nd, 3)) - 2.5, _features_dc_motion=N((Nd, 1, 3)), _features_rest_motion=0.1 * N((Nd, 15, 3)))
    return {n: np.ascontiguousarray(v, np.float32) for n, v in P.items()}


def functional(N, seed=0):
    """The fixed random linear functional: weights [N,3], float32."""
    return np.random.default_rng(77 + seed).standard_normal((N, 3)).astype(np.float32)


# ---------------------------------------------------------------------------------------------- the restatement
def _hermite(d):
    return 2 * d ** 3 - 3 * d ** 2 + 1, d ** 3 - 2 * d ** 2 + d, -2 * d ** 3 + 3 * d ** 2, d ** 3 - d ** 2


def _pchip_slope(before, at, after):
    return torch.where((after - at) * (at - before) > 0, (after - at) * (at - before) / (after - before) * 2, torch.zeros_like(at))


def positions(xyz, xyz_disp, xyz_motion, t, interp):
    """x(t) [Ns+Nd,3] in the tensors' precision, static rows first (c_gaussian_model.py:170-193 of the reference)."""
    static = xyz + xyz_disp * t / max(DURATION, 1)
    if xyz_motion.shape[0] == 0:
        return static
    k, d = time_index(interp, t)
    y = xyz_motion
    if interp == "linear":
        dyn = y[:, k] * (1 - d) + y[:, k + 1] * d
    else:
        h00, h10, h01, h11 = _hermite(d)
        y0, y1, y2, y3 = y[:, k - 1], y[:, k], y[:, k + 1], y[:, k + 2]
        if interp == "pchip":
            m_k, m_k1 = _pchip_slope(y0, y1, y2), _pchip_slope(y1, y2, y3)
        else:
            m_k, m_k1 = (y2 - y0) / 2, (y3 - y1) / 2
        dyn = h00 * y1 + h10 * m_k + h01 * y2 + h11 * m_k1
    return torch.cat([static, dyn], 0)


def project(x, cam):
    """(u, v, z) [N,3] of means x in x's precision: the rasterizer's pixel position and view depth."""
    pm = cam.full_proj_transform.to(x.dtype)
    vm = cam.world_view_transform.to(x.dtype)
    h = x @ pm[:3] + pm[3]
    inv_w = 1.0 / (h[:, 3] + EPS_W)
    u = ((h[:, 0] * inv_w + 1.0) * cam.image_width - 1.0) * 0.5
    v = ((h[:, 1] * inv_w + 1.0) * cam.image_height - 1.0) * 0.5
    z = (x @ vm[:3] + vm[3])[:, 2]
    return torch.stack([u, v, z], 1)


def screen_displacement(x0, x1, cam, near=NEAR):
    """project(x1) - project(x0) with the depth rule."""
    q0, q1 = project(x0, cam), project(x1, cam)
    behind = (q0[:, 2] <= near) | (q1[:, 2] <= near)
    return torch.where(behind[:, None], torch.zeros_like(q0), q1 - q0), behind


def displacement(P, t0, t1, interp, space="world", cam=None, near=NEAR, dtype=torch.float64, requires_grad=False):
    """(displacement [N,3], the three leaf tensors) of the state P (numpy or torch, any precision) in `dtype`."""
    leaves = [torch.as_tensor(P[n]).detach().to(dtype).clone().requires_grad_(requires_grad) for n in NAMES]
    x0, x1 = positions(*leaves, t0, interp), positions(*leaves, t1, interp)
    out = x1 - x0 if space == "world" else screen_displacement(x0, x1, cam, near)[0]
    return out, leaves


def gradients(P, weights, t0, t1, interp, space="world", cam=None, near=NEAR, dtype=torch.float64):
    """{name: d sum(weights * displacement) / d name} as numpy, by autograd of the restatement."""
    out, leaves = displacement(P, t0, t1, interp, space, cam, near, dtype, requires_grad=True)
    loss = (out * torch.as_tensor(weights).to(dtype)).sum()
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)          # (no dynamic rows: the keyframes take no part)
    return {n: (torch.zeros_like(x) if g is None else g).numpy() for n, x, g in zip(NAMES, leaves, grads)}


def row_classes(radii0, radii1, z0, z1, near=NEAR):
    """The classes of rows the screen test tells apart, as boolean masks: from the radii of the two frames and the view depths."""
    radii0, radii1, z0, z1 = (np.asarray(a) for a in (radii0, radii1, z0, z1))
    b0, b1 = z0 <= near, z1 <= near
    return dict(visible_both=(radii0 > 0) & (radii1 > 0), visible_one=(radii0 > 0) ^ (radii1 > 0),
                behind_t0=b0 & ~b1, behind_t1=~b0 & b1, behind_both=b0 & b1)


def check_grad(name, got, ref, bar=GRAD_BAR):
    """NaN in the same places; elsewhere |got - ref| <= bar * max(1, |ref|inf over the finite entries).  Returns the worst error."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), f"{name}: NaN in other places than the reference ({int(np.isnan(got).sum())} / {int(nan.sum())})"
    if nan.all():
        return 0.0
    scale = max(1.0, float(np.abs(ref[~nan]).max()))
    err = float(np.abs(got[~nan] - ref[~nan]).max()) if (~nan).any() else 0.0
    assert err <= bar * scale, f"{name}: error {err:.3g} > {bar:g} * {scale:.3g}"
    return err / scale


# (Ns, Nd) of the GPU tests: each of 0, 1, 255, 256, 257, 300 on both sides -- the 256-lane block edge and the static / dynamic seam
# inside a block; never both 0
SHAPES = ((0, 300), (300, 0), (1, 255), (255, 1), (256, 257), (257, 256), (300, 300))
CLASS_PAIRS = ("far", "ends")          # t0 < t1 intervals apart: every class of row can exist (t0 == t1 or one interval cannot hold them)


def cpu_model(P, interp):
    """ex4dgs_amd.scene.DynamicGaussians over P with the torch getters (CPU)."""
    from ex4dgs_amd.scene import DynamicGaussians
    return DynamicGaussians({n: torch.as_tensor(v) for n, v in P.items()}, duration=DURATION, interval=INTERVAL, time_pad=TIME_PAD,
                            var_pad=VAR_PAD, interp_type=interp)


def oracle_frame(P, t, interp, cam, near=NEAR):
    """(radii, view depths) of the CPU oracle's frame of state P at t."""
    from oracle import oracle
    m = cpu_model(P, interp)
    with torch.no_grad():
        x = m.get_xyz_at_t(t)
        fwd = oracle.forward(x, None, m.get_opacity_at_t(t), shs=m.get_features(), scales=m.get_scaling(), rotations=m.get_rotation_at_t(t),
                             bg=np.zeros(3, np.float32), viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform,
                             campos=cam.camera_center, image_height=cam.image_height, image_width=cam.image_width,
                             tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5), kernel_size=0.1, sh_degree=3,
                             min_depth=near, max_depth=100.0, want_fragile=False)
        z = project(x.double(), cam)[:, 2].numpy()
    return fwd, z


def load():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def fixture_cases():
    """(interp, K, Ns, Nd) of the states the fixture holds."""
    return [(interp, K, Ns, Nd) for interp in INTERPS for K, Ns, Nd in ((K_MANY, 8, 20), (k_min(interp), 3, 10))]


def key(interp, K, pair=None):
    return f"{interp}/K{K}" + ("" if pair is None else f"/{pair}")
