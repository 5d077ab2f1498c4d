"""Scenes, hand-built tie frames and a host census of the compositing forward's walk, shared by tests/test_cpu_composite_fwd_cases.py
(the cases have the properties they are chosen for, on the CPU oracle) and tests/test_gpu_composite_fwd_paths.py (every path of the walk
against the oracle, and the census against the kernel's own compacted lists).

The census restates the control flow of composite_fwd_body (ex4dgs_amd/csrc/ex4d_composite.hip): one wave per 8x8 quadrant of a 16x16
tile streams the tile's list in chunks of 64 positions while a lane is live; a chunk's survivors of the quadrant cull are staged in
list order and walked j = 0, 1, ... in groups of 16, entry j on register set a (j even) or b (j odd).  The chunk runs the CLAMP variant
of the walk when one of its staged entries has w > 0.99.  Per entry the walk reaches one of five outcomes:
    skip       no live lane in range (power <= 0 and alpha >= 1/255)
    add        lanes add, nobody saturates
    rare_add   a lane saturates (T (1 - alpha) < 1e-4: Lrare), others still add
    rare_skip  a lane saturates, nobody adds, lanes stay live
    rare_dead  the last live lane saturates: the rest of the chunk is abandoned (Ldead)
The decisions are taken in float64 (dtype = np.float32: in float32, in the oracle's order of operations -- what exact ties need) on
the float32 inputs, so they are the oracle's and the kernel's on every pixel that is not fragile."""
import math

import numpy as np
import torch

from ex4dgs_amd.scene import SceneConfig, focal_camera
from tests import composite_cases as cc
from tests import helpers as h

TILE, QUAD, CHUNK, GROUP = 16, 8, 64, 16
OUTCOMES = ("skip", "add", "rare_add", "rare_skip", "rare_dead")
VARIANTS = ("noclamp", "clamp")
SETS = ("a", "b")
BRANCHES = ("inside", "vertical", "horizontal", "corner")
CLAMP_F32 = np.float32(0.99)                    # 0x3f7d70a4, the kernel's and the oracle's 0.99f
ALPHA_MIN_F32 = np.float32(1.0) / np.float32(255.0)
T_MIN_F32 = np.float32(0.0001)


def cell(variant, set_, outcome):
    """Name of one of the 20 cells; variant and set_ as indices or names."""
    v = VARIANTS[variant] if isinstance(variant, (int, np.integer)) else variant
    s = SETS[set_] if isinstance(set_, (int, np.integer)) else set_
    return f"{v}.{s}.{outcome}"


# the forward's outputs and per-pixel state that do not depend on dir3D (tests/test_cpu_composite_fwd_cases.py checks it on the oracle):
# what the flow kernel shares bit for bit with the flow-free walks
FLOW_INDEPENDENT = ("color", "depth", "acc", "idx", "final_T", "n_contrib")
CELLS = tuple(cell(v, s, o) for v in VARIANTS for s in SETS for o in OUTCOMES)

# ------------------------------------------------------------------ scenes
DEEP, WRAP, SPARSE = cc.DEEP, cc.WRAP, cc.SPARSE
# DEEP with 3000 Gaussians, a third of the opacities in (0.99, 1.0] and a sixth in (0.97, 0.99]: footprints of 5 px keep the filter's
# coefficient near 0.996, so most of the first share stays above 0.99 after it -- chunks of the CLAMP variant whose v_min decides
OPAQUE = DEEP._replace(name="composite deep, opaque", P=3000)
# WRAP with 1 px footprints: an entry reaches a few pixels of a quadrant, so one whose pixels all saturate while others stay live --
# "saturates, nobody adds, lanes stay live" -- occurs a dozen times; 3 % of the Gaussians are three times as large and opaque (w > 0.99
# after the filter), which puts those entries into chunks of the CLAMP variant
STACK = WRAP._replace(name="composite 1 px footprints, opaque pile", P=6000, sigma_px_med=1.0)
# SPARSE with 0.7 px footprints: tile lists of a few entries of which a quadrant often keeps none -- two dozen chunks that stage nothing
# while every lane is live (SPARSE itself has five) -- and tiles without a list
SPECKS = SPARSE._replace(name="composite specks", sigma_px_med=0.7)


def _opaque(ins, st):
    g = torch.Generator().manual_seed(4100)
    P = ins["opacities"].shape[0]
    u, v = torch.rand(P, generator=g), torch.rand(P, generator=g)
    op = ins["opacities"].clone().reshape(P)
    hi, mid = u < 1.0 / 3.0, (u >= 1.0 / 3.0) & (u < 0.5)
    op[hi] = (0.9901 + 0.02 * v[hi]).clamp(max=1.0)            # (0.99, 1.0], half of them 1.0 itself
    op[mid] = 0.99 - 0.0199 * v[mid]                           # (0.97, 0.99]
    ins["opacities"] = op.reshape(P, 1).contiguous()


def _stack(ins, st):
    g = torch.Generator().manual_seed(4200)
    P = ins["opacities"].shape[0]
    u, v = torch.rand(P, generator=g), torch.rand(P, generator=g)
    big = u < 0.03
    op = ins["opacities"].clone().reshape(P)
    op[big] = 1.0
    sc = ins["scales"].clone()
    sc[big] = sc[big] * 3.0
    ins["opacities"], ins["scales"] = op.reshape(P, 1).contiguous(), sc.contiguous()


SCENES = {"deep": (DEEP, None), "wrap": (WRAP, None), "sparse": (SPARSE, None), "opaque": (OPAQUE, _opaque), "stack": (STACK, _stack),
          "specks": (SPECKS, None)}


def scene_inputs(name, dir_scale=0.0):
    cfg, mutate = SCENES[name]
    ins, st = h.scene_inputs(cfg, dir_scale=dir_scale)
    if mutate:
        mutate(ins, st)
    return ins, st


# ------------------------------------------------------------------ the quadrant cull in numpy (float32, operation by operation)
def cull_constants(conic_opacity):
    """tau, k1, k2 per Gaussian as the per-Gaussian forward kernel forms them (ex4d_preprocess.hip)."""
    co = np.asarray(conic_opacity, np.float32)
    A, B, C, w = co[:, 0], co[:, 1], co[:, 2], co[:, 3]
    with np.errstate(all="ignore"):
        convex = (A > 0) & (C > 0) & (A * C - B * B > 0)
        tau = np.where(w < ALPHA_MIN_F32, np.float32(-np.inf),
                       np.where(~convex, np.float32(np.inf), np.log(np.float32(255.0) * w, dtype=np.float32) + np.float32(0.01))).astype(np.float32)
        return tau, (-B / C).astype(np.float32), (-B / A).astype(np.float32)


def quadrant_cull(mx, my, A, B, C, tau, k1, k2, bx0, bx1, by0, by1):
    """quadrant_cull of ex4d_composite.hip on float32 arrays -> (culled, branch): branch 0 mean inside the box, 1 faces a vertical edge,
    2 a horizontal edge, 3 a corner."""
    f = np.float32
    with np.errstate(all="ignore"):
        dxc = np.minimum(np.maximum(mx, bx0), bx1) - mx
        dyc = np.minimum(np.maximum(my, by0), by1) - my
        ver, hor = dxc != 0, dyc != 0
        qmin, mag = np.full(mx.shape, f(3.0e38), f), np.zeros(mx.shape, f)
        dy = np.minimum(np.maximum(k1 * dxc, by0 - my), by1 - my)
        t1, t2, t3 = f(0.5) * A * dxc * dxc, f(0.5) * C * dy * dy, B * dxc * dy
        q = t1 + t2 + t3
        up = ver & (q < qmin)
        qmin, mag = np.where(up, q, qmin), np.where(up, np.abs(t1) + np.abs(t2) + np.abs(t3), mag)
        dx = np.minimum(np.maximum(k2 * dyc, bx0 - mx), bx1 - mx)
        t1, t2, t3 = f(0.5) * A * dx * dx, f(0.5) * C * dyc * dyc, B * dx * dyc
        q = t1 + t2 + t3
        up = hor & (q < qmin)
        qmin, mag = np.where(up, q, qmin), np.where(up, np.abs(t1) + np.abs(t2) + np.abs(t3), mag)
        culled = np.where(~ver & ~hor, tau < f(-3.0e38), qmin > tau + f(1e-5) * mag)
    return culled, ver.astype(np.int64) + 2 * hor.astype(np.int64)


# ------------------------------------------------------------------ census
def _np(x):
    return None if x is None else (x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x))


def census(ranges, point_list, conic_opacity, means2D, W, H, offsets=None, qlist=None, qcount=None, dtype=np.float64):
    """Which paths the compositing forward walks on this frame.  qlist / qcount given: the staged entries are the kernel's own
    (BinState::qlist, qcount); otherwise those of the numpy cull.  Returns counts (plain ints: the dict goes into the parity report) and,
    under "per_quadrant", arrays per quadrant (flat index 4 * tile + quadrant): chunks (walked), last_live_chunk (-1: none), staged
    (entries), fragile-free replays of the per-pixel state `last` (n_contrib) and `dom` (idx) as [H,W] images, `lists` (the staged
    positions, per quadrant) and `dom_at` ([H,W,2]: chunk and j of the dominant entry)."""
    D = dtype
    ranges = _np(ranges).astype(np.int64).reshape(-1, 2)
    pl = _np(point_list).astype(np.int64).reshape(-1)
    co32 = np.ascontiguousarray(_np(conic_opacity), np.float32).reshape(-1, 4)
    m32 = np.ascontiguousarray(_np(means2D), np.float32).reshape(-1, 2)
    tau, k1, k2 = cull_constants(co32)
    co, m2 = co32.astype(D), m32.astype(D)
    off32 = np.zeros((H, W, 2), np.float32) if offsets is None else _np(offsets).reshape(H, W, 2).astype(np.float32)
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    Q = 4 * gx * gy
    assert ranges.shape[0] == gx * gy, (ranges.shape, gx, gy)
    if qlist is not None:
        ql = _np(qlist).astype(np.int64).reshape(-1) & 0xFFFFFFFF
        qc = _np(qcount).astype(np.int64).reshape(-1) & 0xFFFFFFFF
        assert qc.shape[0] == Q, (qc.shape, Q)
    clamp_D, amin_D, tmin_D, amust = D(CLAMP_F32), D(ALPHA_MIN_F32), D(T_MIN_F32), (1.0 + 1e-4) / 255.0

    cells = {k: 0 for k in CELLS}
    cnt_mod = {r: 0 for r in range(GROUP)}
    cull = {f"{b}.{o}": 0 for b in BRANCHES for o in ("kept", "culled")}
    n = dict(chunks=0, chunks_empty_live=0, chunks_multi_group=0, chunks_end_on_a=0, abandoned_a=0, abandoned_b=0, later_chunks=0,
             quadrants_unfinished=0, quadrants_finished=0, quadrants_empty_list=0, quadrants_outside=0, quadrants_partly_outside=0,
             clamped_pairs=0, clamped_entries=0, new_dominant_group_ge1=0, new_dominant_chunk_ge1=0, weight_ties=0,
             tau_pos_inf=0, tau_neg_inf=0, cull_differs=0, cull_missed=0, staged_entries=0, pairs_added=0)
    clamped_ids = set()
    chunks_q, last_live_q, staged_q = np.zeros(Q, np.int64), np.full(Q, -1, np.int64), np.zeros(Q, np.int64)
    lists = [np.zeros(0, np.int64) for _ in range(Q)]
    last_img, dom_img, dom_at = np.zeros((H, W), np.int64), np.full((H, W), -1, np.int64), np.full((H, W, 2), -1, np.int64)
    lane = np.arange(QUAD * QUAD)

    for i in range(Q):
        t, q = divmod(i, 4)
        px = (t % gx) * TILE + (q & 1) * QUAD + (lane & 7)
        py = (t // gx) * TILE + (q >> 1) * QUAD + (lane >> 3)
        inside = (px < W) & (py < H)
        if not inside.any():
            n["quadrants_outside"] += 1
            continue
        n["quadrants_partly_outside"] += int(not inside.all())
        r0, r1 = ranges[t]
        cnt_list = int(r1 - r0)
        if cnt_list == 0:
            n["quadrants_empty_list"] += 1
            continue
        # pixel positions: float32(px) + offset in float32 for inside lanes, the bare integer for the others (pixel_of_lane)
        pxi, pyi = np.minimum(px, W - 1), np.minimum(py, H - 1)
        fx32 = np.where(inside, (px.astype(np.float32) + off32[pyi, pxi, 0]).astype(np.float32), px.astype(np.float32))
        fy32 = np.where(inside, (py.astype(np.float32) + off32[pyi, pxi, 1]).astype(np.float32), py.astype(np.float32))
        bx0, bx1, by0, by1 = fx32.min(), fx32.max(), fy32.min(), fy32.max()
        fx, fy = fx32.astype(D), fy32.astype(D)
        mine = None
        if qlist is not None:
            s0 = 4 * r0 + q * cnt_list
            mine = ql[s0: s0 + qc[i]]
        live = inside.copy()
        T, maxw = np.ones(64, D), np.zeros(64, D)
        last, dom, dat = np.zeros(64, np.int64), np.full(64, -1, np.int64), np.full((64, 2), -1, np.int64)
        staged_all = []
        finished = True
        for c, base in enumerate(range(0, cnt_list, CHUNK)):
            if not live.any():
                finished = False
                break
            n["chunks"] += 1
            n["later_chunks"] += int(c >= 1)
            chunks_q[i] += 1
            last_live_q[i] = c
            pos = np.arange(base, min(base + CHUNK, cnt_list))
            ids = pl[r0 + pos]
            culled, branch = quadrant_cull(m32[ids, 0], m32[ids, 1], co32[ids, 0], co32[ids, 1], co32[ids, 2], tau[ids], k1[ids], k2[ids], bx0, bx1, by0, by1)
            for b in range(4):
                cull[BRANCHES[b] + ".kept"] += int((~culled & (branch == b)).sum())
                cull[BRANCHES[b] + ".culled"] += int((culled & (branch == b)).sum())
            n["tau_pos_inf"] += int(np.isposinf(tau[ids]).sum())
            n["tau_neg_inf"] += int(np.isneginf(tau[ids]).sum())
            keep = ~culled
            if mine is not None:
                kernel_keep = np.isin(pos, mine)
                n["cull_differs"] += int((kernel_keep != keep).sum())
                keep = kernel_keep
            # every (entry, pixel) pair of the chunk, in the oracle's order of operations (CR/forward.cu:368-379)
            dx, dy = m2[ids, 0][:, None] - fx[None], m2[ids, 1][:, None] - fy[None]
            A, B, C, w = (co[ids, k][:, None] for k in range(4))
            power = D(-0.5) * (A * dx * dx + C * dy * dy) - B * dx * dy
            with np.errstate(over="ignore", under="ignore"):
                wG = w * np.exp(np.minimum(power, D(0)))
            alpha_all = np.minimum(clamp_D, wG)
            reach = (power <= 0) & (alpha_all >= amin_D)
            must = ((power.astype(np.float64) <= 0) & (alpha_all.astype(np.float64) >= amust) & inside[None]).any(1)
            n["cull_missed"] += int((must & ~keep).sum())
            sel = np.flatnonzero(keep)
            cnt = len(sel)
            staged_all.append(pos[sel])
            staged_q[i] += cnt
            n["staged_entries"] += cnt
            if cnt == 0:
                n["chunks_empty_live"] += 1
                continue
            cnt_mod[cnt % GROUP] += 1
            n["chunks_multi_group"] += int(cnt > GROUP)
            variant = int((co32[ids[sel], 3] > CLAMP_F32).any())
            dead_at = -1
            for j, e in enumerate(sel):
                s = j & 1
                ok = live & reach[e]
                if not ok.any():
                    cells[cell(variant, s, "skip")] += 1
                    continue
                alpha = alpha_all[e]
                test_T = T * (D(1) - alpha)
                stop = ok & (test_T < tmin_D)
                if stop.any():
                    live &= ~stop
                    ok &= ~stop
                    if not ok.any():
                        if not live.any():
                            cells[cell(variant, s, "rare_dead")] += 1
                            dead_at = j
                            break
                        cells[cell(variant, s, "rare_skip")] += 1
                        continue
                    cells[cell(variant, s, "rare_add")] += 1
                else:
                    cells[cell(variant, s, "add")] += 1
                wgt = alpha * T
                hit = ok & (wG[e] > clamp_D)
                if hit.any():
                    n["clamped_pairs"] += int(hit.sum())
                    n["clamped_entries"] += 1
                    clamped_ids.add(int(ids[e]))
                n["pairs_added"] += int(ok.sum())
                better = ok & (wgt > maxw)
                n["weight_ties"] += int((ok & (wgt == maxw)).sum())
                n["new_dominant_group_ge1"] += int(better.sum()) if j >= GROUP else 0
                n["new_dominant_chunk_ge1"] += int(better.sum()) if c >= 1 else 0
                maxw = np.where(better, wgt, maxw)
                dom[better] = ids[e]
                dat[better] = (c, j)
                T = np.where(ok, test_T, T)
                last[ok] = pos[e] + 1
            if dead_at >= 0:
                if dead_at < cnt - 1:
                    n["abandoned_" + SETS[dead_at & 1]] += 1
            else:
                n["chunks_end_on_a"] += cnt & 1
        n["quadrants_finished" if finished else "quadrants_unfinished"] += 1
        lists[i] = np.concatenate(staged_all) if staged_all else np.zeros(0, np.int64)
        last_img[py[inside], px[inside]] = last[inside]
        dom_img[py[inside], px[inside]] = dom[inside]
        dom_at[py[inside], px[inside]] = dat[inside]
    out = {k: int(v) for k, v in n.items()}
    out["clamped_gaussians"] = len(clamped_ids)
    per = dict(chunks=chunks_q, last_live_chunk=last_live_q, staged=staged_q, last=last_img, dom=dom_img, dom_at=dom_at, lists=lists)
    return dict(cells=cells, cnt_mod16={int(k): int(v) for k, v in cnt_mod.items()}, cull=cull, from_kernel_lists=int(qlist is not None),
                dtype=np.dtype(D).name, per_quadrant=per, **out)


def census_of(o, offsets=None, g=None, dtype=np.float64):
    """The census of a forward: geometry from the oracle's forward `o`, lists from the GPU forward `g` when given."""
    return census(o["ranges"], o["point_list"], o["conic_opacity"], o["means2D"], o["W"], o["H"], offsets,
                  None if g is None else g["qlist"], None if g is None else g["qcount"], dtype)


def report(c, tag):
    """The census without its arrays, as an entry of helpers.REPORT."""
    return dict(kind="composite_fwd_census", tag=tag, **{k: v for k, v in c.items() if k != "per_quadrant"})


def fragile_quadrants(fragile, W, H, frag_eps):
    """Per quadrant: does it hold a fragile pixel (a decision of the oracle within frag_eps of its threshold)?"""
    return cc._quads(np.asarray(fragile).reshape(H, W) <= frag_eps, W, H, False).any(1)


# ------------------------------------------------------------------ coverage conditions
def cells_of(c, outcome):
    return {(v, s): c["cells"][cell(v, s, outcome)] for v in VARIANTS for s in SETS}


def assert_coverage(by_scene):
    """The conditions the scenes are chosen for, over {scene name: census}: what tests/test_gpu_composite_fwd_paths.py proves has run."""
    cs = list(by_scene.values())
    union = {k: sum(c["cells"][k] for c in cs) for k in CELLS}
    assert all(v >= 1 for v in union.values()), {k: v for k, v in union.items() if v < 1}
    for outcome in ("add", "skip", "rare_add", "rare_dead"):
        for v in VARIANTS:
            for s in SETS:
                best = max(c["cells"][cell(v, s, outcome)] for c in cs)
                assert best >= 8, (cell(v, s, outcome), best)
    mods = {r: sum(c["cnt_mod16"][r] for c in cs) for r in range(GROUP)}
    assert all(v >= 1 for v in mods.values()), mods
    for k in ("chunks_empty_live", "chunks_end_on_a", "abandoned_a", "abandoned_b", "later_chunks"):
        assert max(c[k] for c in cs) >= 8, (k, [c[k] for c in cs])
    for b in BRANCHES:
        for o in ("kept", "culled"):
            want = 1 if (b, o) == ("inside", "culled") else 8
            assert sum(c["cull"][f"{b}.{o}"] for c in cs) >= want, (b, o, [c["cull"][f"{b}.{o}"] for c in cs])
    if "opaque" in by_scene:
        assert by_scene["opaque"]["clamped_pairs"] >= 50, by_scene["opaque"]["clamped_pairs"]


# ------------------------------------------------------------------ hand-built tie frames
TIE_W = TIE_H = 41                  # odd: the optical axis meets the integer centre pixel (20, 20) = tile (1, 1), quadrant 0, lane 36
TIE_FOCAL = 40.0
TIE_FILLERS = (0, 14, 15, 63)       # tied entries at j = (0, 1), (14, 15): one group; (15, 16): two groups; list positions 63, 64: two chunks
TIE_CENTRE = (TIE_W // 2, TIE_H // 2)
TIE_FIRST, TIE_SECOND = 1, 0        # Gaussian ids: the nearer tied entry carries the LARGER id
TIE_CFG = SceneConfig("composite tie frame", 2, TIE_W, TIE_H, TIE_FOCAL, min_depth=0.01, max_depth=100.0)
_TIE_Z = (3.0, 4.0)
_TIE_SIGMA_PX = 3.0
_TIE = {}


def _tie_settings():
    cam = focal_camera(TIE_W, TIE_H, TIE_FOCAL, znear=0.01, zfar=100.0)
    return dict(bg=torch.tensor([0.25, 0.5, 0.125]), viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform,
                campos=cam.camera_center, image_height=TIE_H, image_width=TIE_W, tanfovx=math.tan(cam.FoVx * 0.5),
                tanfovy=math.tan(cam.FoVy * 0.5), kernel_size=0.1, sh_degree=3, min_depth=TIE_CFG.min_depth, max_depth=TIE_CFG.max_depth,
                scale_modifier=1.0, prefiltered=False)


def _tie_gaussians(z, sigma_px, px, py, opacity, seed, dir_scale):
    """Axis-aligned isotropic Gaussians at depth z whose means project to pixel (px, py)."""
    z, px, py = (torch.as_tensor(v, dtype=torch.float32).reshape(-1) for v in (z, px, py))
    P = z.shape[0]
    g = torch.Generator().manual_seed(seed)
    cx, cy = (TIE_W - 1) * 0.5, (TIE_H - 1) * 0.5
    means = torch.stack([(px - cx) * z / TIE_FOCAL, (py - cy) * z / TIE_FOCAL, z], -1)
    rot = torch.zeros(P, 4); rot[:, 0] = 1.0
    scales = (z * torch.as_tensor(sigma_px, dtype=torch.float32) / TIE_FOCAL).reshape(-1, 1).expand(P, 3)
    shs = torch.cat([torch.randn(P, 1, 3, generator=g), 0.15 * torch.randn(P, 15, 3, generator=g)], 1)
    return dict(means3D=means.contiguous(), rotations=rot, opacities=torch.as_tensor(opacity, dtype=torch.float32).reshape(P, 1).contiguous(),
                scales=scales.contiguous(), shs=shs.contiguous(), dir3D=(dir_scale * torch.randn(P, 3, generator=g)).contiguous())


def tie_opacities(candidates=2048):
    """Opacities (front, back) of two Gaussians on the optical axis whose blending weights at the centre pixel tie exactly in float32:
    w_back (1 - w_front) == w_front with G = 1 and T = 1 in front of the pair.  Found by searching float bit patterns of the
    opacity on the CPU oracle's own conic_opacity (the filter's coefficient sits between the opacity and w)."""
    if "pair" in _TIE:
        return _TIE["pair"]
    centre = lambda n: (np.full(n, TIE_CENTRE[0]), np.full(n, TIE_CENTRE[1]))
    # the filter's coefficients of the two Gaussians: w = opacity x coefficient
    o = h.oracle_forward(_tie_gaussians(np.array(_TIE_Z, np.float32), _TIE_SIGMA_PX, *centre(2), np.ones(2, np.float32), 1, 0.0), _tie_settings())
    c1, c2 = (float(x) for x in o["conic_opacity"][:, 3])
    bits = lambda x0: (np.array([x0], np.float32).view(np.uint32)[0] - np.uint32(candidates // 2) + np.arange(candidates, dtype=np.uint32)).view(np.float32)
    w_front = 0.26                                   # in [0.25, 0.5): one ulp of w_front is more than one step of w_back (1 - w_front)
    cand = np.concatenate([bits(w_front / c1), bits(w_front / (1.0 - w_front) / c2)])
    z = np.concatenate([np.full(candidates, _TIE_Z[0], np.float32), np.full(candidates, _TIE_Z[1], np.float32)])
    o = h.oracle_forward(_tie_gaussians(z, _TIE_SIGMA_PX, *centre(2 * candidates), cand, 1, 0.0), _tie_settings())
    w = o["conic_opacity"][:, 3]
    w1, w2 = w[:candidates], w[candidates:]
    for i in range(candidates // 2, candidates):
        hitj = np.flatnonzero((w2 * (np.float32(1) - w1[i])).astype(np.float32) == w1[i])
        if hitj.size:
            _TIE["pair"] = (float(cand[i]), float(cand[candidates + hitj[0]]), float(w1[i]), float(w2[hitj[0]]))
            return _TIE["pair"]
    raise AssertionError("no tying pair of opacities among the candidates")


def tie_inputs(k, dir_scale=0.0):
    """(ins, settings) of the tie frame with k fillers in front of the tied pair: ids TIE_SECOND = 0 (back), TIE_FIRST = 1 (front),
    fillers 2 ...: 0.6 px Gaussians near pixel (22, 22) of the centre pixel's quadrant, which do not reach the centre pixel."""
    op1, op2, _, _ = tie_opacities()
    g = torch.Generator().manual_seed(4300 + k)
    fz = 1.0 + torch.arange(k, dtype=torch.float32) / 64.0
    fx, fy = 22.0 + (torch.rand(k, generator=g) - 0.5), 22.0 + (torch.rand(k, generator=g) - 0.5)
    fo = 0.1 + 0.5 * torch.rand(k, generator=g)
    z = torch.cat([torch.tensor([_TIE_Z[1], _TIE_Z[0]]), fz])
    px = torch.cat([torch.full((2,), float(TIE_CENTRE[0])), fx])
    py = torch.cat([torch.full((2,), float(TIE_CENTRE[1])), fy])
    sig = torch.cat([torch.full((2,), _TIE_SIGMA_PX), torch.full((k,), 0.6)])
    op = torch.cat([torch.tensor([op2, op1]), fo])
    return _tie_gaussians(z, sig, px, py, op, 4400 + k, dir_scale), _tie_settings()


def tie_quadrant():
    return cc.quadrant_of(TIE_CENTRE[0], TIE_CENTRE[1], TIE_W)


def tie_positions(o, c):
    """Where the census staged the two tied entries in the centre pixel's quadrant: ((chunk, j) of the front one, of the back one), and
    asserts the layout the frame is built for: k fillers in front, all staged, the pair behind them."""
    i = tie_quadrant()
    t = i // 4
    r0 = int(o["ranges"][t, 0])
    lst = c["per_quadrant"]["lists"][i]
    ids = o["point_list"].astype(np.int64)[r0 + lst]
    at = {int(g): int(p) for g, p in zip(ids, np.arange(len(lst)))}
    assert TIE_FIRST in at and TIE_SECOND in at and at[TIE_SECOND] == at[TIE_FIRST] + 1, at
    assert (lst == np.arange(len(lst))).all(), lst                                  # nothing culled: staged index == list position
    first = at[TIE_FIRST]
    return (first // CHUNK, first % CHUNK), ((first + 1) // CHUNK, (first + 1) % CHUNK)
