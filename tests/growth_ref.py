"""Device-agnostic torch restatement of the reference's growth of the dynamic set (scene/c_gaussian_model.py:1147-1358:
extract_dynamic_points_from_static, expand_duration, adjust_temp_opa): the checker of ex4dgs_amd.growth, pinned itself by
tests/golden/growth.npz.

State: the dict of tests/densify_ref.py ({"params", "m", "v", "stats"}, the reference's shapes).  Model: {"interval", "time_shift",
"time_pad", "duration"} -- extract / expand_duration update "duration" as the reference updates self.duration.  New tensors are
allocated in the inputs' dtype: a float64 state gives the float64 restatement.
"""
import math

import torch

from tests.densify_ref import D_STATS, DYNAMIC, INIT, S_STATS, STATIC


def quantile_rank(q, n):
    """(lo, hi, weight) of torch.quantile(x, q) with linear interpolation over n values: the rank is float32(q) * (n - 1) evaluated
    in float32 (n = 1 000 003, q = 0.98 gives 980 002 where float64 gives 980 001)."""
    rank = torch.tensor(q, dtype=torch.float32) * torch.tensor(float(n - 1), dtype=torch.float32)
    lo = torch.floor(rank)
    return int(lo), int(torch.ceil(rank)), rank - lo


def lerp(a, b, w):
    """torch.lerp: w < 0.5 ? a + w (b - a) : b - (b - a)(1 - w), the multiply-add fused (one rounding) -- the primitive itself, so
    that the restatement rounds as the library it restates does on the device it runs on."""
    return torch.lerp(a, b, w.to(a))


def quantile(x, q):
    """torch.quantile(x, q) of a 1-D tensor from a sort, in the restatement's words; a NaN makes it NaN."""
    if torch.isnan(x).any():
        return torch.full((), float("nan"), dtype=x.dtype, device=x.device)
    lo, hi, w = quantile_rank(q, x.numel())
    s = torch.sort(x)[0]
    return lerp(s[lo], s[hi], w.to(x.device))


def quantile_select_then_normalise(s, q):
    """The threshold as the kernels compute it: the two order statistics of the UN-normalised scores, normalised afterwards
    (x -> x / (max + 1e-6) is monotone, so it maps order statistics to order statistics)."""
    if torch.isnan(s).any():
        return torch.full((), float("nan"), dtype=s.dtype, device=s.device)
    lo, hi, w = quantile_rank(q, s.numel())
    srt = torch.sort(s)[0]
    den = srt[-1] + 0.000001
    return lerp(srt[lo] / den, srt[hi] / den, w.to(s.device))


def scores(P, cam, vis):
    """(u, |disp|) of the visible rows, u the normalised motion score (:1153-1156)."""
    n = P["_xyz_disp"][vis].norm(dim=-1)
    r = (P["_xyz"][vis] - cam.to(P["_xyz"])).norm(dim=-1) ** 2
    s = n / (r + 0.000001)
    return s / (s.max() + 0.000001), n


def first_keyframes(model, max_dur):
    """K of the first extraction (:1166); not keyframe_count's formula."""
    return math.ceil((max_dur + model["time_shift"] * 2 + 1) / model["interval"]) + 3


def resize_two_points(a, b, K):
    """torch's bilinear resize (align_corners=False) of the pair (a, b) [N, 3] to K samples [N, K, 3]: source coordinate
    max(0, (2 / K)(k + 0.5) - 0.5); a while it is 0, a blend below 1, b from 1 on."""
    k = torch.arange(K, dtype=torch.float32, device=a.device)
    at = (torch.tensor(2.0, dtype=torch.float32) / K * (k + 0.5) - 0.5).clamp_min(0).to(a.dtype).view(1, K, 1)
    blend = (1 - at) * a[:, None, :] + at * b[:, None, :]
    return torch.where(at < 1, blend, b[:, None, :].expand_as(blend))


def extract(state, model, cam, vis, extent, percentile=0.98, motion_thres=1000.0, min_motion_thres=1e-6, max_dur=None):
    """extract_dynamic_points_from_static on `state` (in place).  Returns {"mask": the selected static rows, "threshold", "visible"};
    no visible row: nothing happens (the reference raises there)."""
    P, st = state["params"], state["stats"]
    vis = vis.bool()
    max_dur = model["duration"] if max_dur is None else max(float(max_dur), model["interval"])
    nvis = int(vis.sum())
    if nvis == 0:
        return {"mask": torch.zeros_like(vis), "threshold": float("nan"), "visible": 0}
    u, n = scores(P, cam, vis)
    theta = quantile(u, percentile)
    sel = ((u > theta) | (n > motion_thres * extent)) & (n > min_motion_thres * extent)
    mask = vis.clone()
    mask[vis] = sel
    mask &= st["xyz_error_min_timestamp"].view(-1) >= 0
    nd = P["_xyz_motion"].shape[0]
    K = P["_xyz_motion"].shape[1] if nd > 0 else first_keyframes(model, max_dur)
    iv, sh, pad = model["interval"], model["time_shift"], model["time_pad"]
    x, d = P["_xyz"][mask], P["_xyz_disp"][mask]
    t = st["xyz_error_min_timestamp"][mask]
    op = P["_opacity"][mask]
    one = torch.ones_like(op)
    new = {"_xyz_motion": resize_two_points(x - d * iv / max_dur, x + d * (1 + iv / max_dur), K),
           "_rotation_motion": P["_rotation"][mask].unsqueeze(1).repeat(1, K, 1),
           "_opacity_motion": op, "_scaling_motion": P["_scaling"][mask],
           "_features_dc_motion": P["_features_dc"][mask], "_features_rest_motion": P["_features_rest"][mask],
           "_opacity_duration_center": torch.stack([one * (t / 2 + sh) / iv, one * ((max_dur + t.clamp_min(0)) / 2 + sh) / iv],
                                                   dim=1).clamp((sh + 1) / iv, (sh + max_dur - 1) / iv),
           "_opacity_duration_var": torch.stack([one * (t + pad), one * (max_dur - t + pad)], dim=1)}
    n_new = int(mask.sum())
    for k in DYNAMIC:
        old = P[k] if nd > 0 else P[k].new_zeros((0,) + tuple(new[k].shape[1:]))
        P[k] = torch.cat([old, new[k]])
        for mom in ("m", "v"):
            if state[mom] is not None and k in state[mom]:
                prev = state[mom][k] if nd > 0 else old
                state[mom][k] = torch.cat([prev, torch.zeros_like(new[k])])
    for k, init in zip(D_STATS, INIT):
        flat = k.endswith("radii2D")
        if k in D_STATS[:7]:                                                   # "reset grad anyway": old and new rows
            st[k] = torch.full((nd + n_new,) if flat else (nd + n_new, 1), init, dtype=st[k].dtype, device=st[k].device)
        else:
            st[k] = torch.cat([st[k], torch.full((n_new, 1), init, dtype=st[k].dtype, device=st[k].device)])
    keep = ~mask
    for k in STATIC:
        P[k] = P[k][keep]
        for mom in ("m", "v"):
            if state[mom] is not None and k in state[mom]:
                state[mom][k] = state[mom][k][keep]
    for k in S_STATS:
        st[k] = st[k][keep]
    return {"mask": mask, "threshold": float(theta), "visible": nvis}


def expanded_keyframes(model, duration):
    return math.ceil((duration + model["time_shift"] + model["time_pad"] * 2 + 1) / model["interval"]) + 3


def _extrapolate(x, n, avg):
    """lin_interp_last (:1264): the step is the mean of the last `avg` keyframes' offsets from the keyframe before them."""
    K = x.shape[1]
    step = (x[:, K - avg:] - x[:, K - avg - 1:K - avg]).mean(dim=1, keepdim=True)
    j = torch.arange(1, n + 1, device=x.device).view(1, -1, 1)
    return torch.cat([x, j * step + x[:, -1:]], dim=1)


def _replace(state, new):
    for k, v in new.items():
        state["params"][k] = v
        for mom in ("m", "v"):
            if state[mom] is not None and k in state[mom]:
                state[mom][k] = torch.zeros_like(v)


def expand_duration(state, model, duration):
    P = state["params"]
    duration = int(duration) + 1
    if duration <= model["duration"]:
        return False
    if P["_xyz_motion"].shape[0] == 0:
        model["duration"] = duration
        return False
    K = P["_xyz_motion"].shape[1]
    grow = expanded_keyframes(model, duration) - K
    if grow < 1:
        model["duration"] = duration
        return False
    iv, sh = model["interval"], model["time_shift"]
    avg = min(K - 2, 4)
    c, v = P["_opacity_duration_center"], P["_opacity_duration_var"]
    var = v.clone()
    var[:, 1] = torch.where((c + sh / iv > (duration + sh) / iv - 0.5).any(dim=1), torch.ones_like(v[:, 1]), v[:, 1])
    _replace(state, {"_xyz_motion": _extrapolate(P["_xyz_motion"], grow, avg), "_rotation_motion": _extrapolate(P["_rotation_motion"], grow, avg),
                     "_opacity_duration_center": c.clamp_max((sh + model["duration"] - 1) / iv), "_opacity_duration_var": var})
    model["duration"] = duration
    return True


def adjust_temp_opa(state, model, max_dur=None):
    P = state["params"]
    max_dur = model["duration"] if max_dur is None else float(max_dur)
    if P["_xyz_motion"].shape[0] == 0:
        return
    iv, sh = model["interval"], model["time_shift"]
    lo, hi = sh / iv + 0.2, (max_dur + sh) / iv - 0.2
    c, v = P["_opacity_duration_center"], P["_opacity_duration_var"]
    var = v.clone()
    var[:, 1] = torch.where((c > hi).any(dim=1), v[:, 1].clamp_min(1) * 2, v[:, 1])
    var[:, 0] = torch.where((c < lo).any(dim=1), v[:, 0].clamp_min(1) * 2, v[:, 0])
    var = torch.where(v < 0.5, torch.full_like(v, 0.5), var)                     # the OLD var decides, and overrides the doubling
    _replace(state, {"_opacity_duration_center": c.clamp(lo, hi), "_opacity_duration_var": var})
