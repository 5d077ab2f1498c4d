"""GPU parity tests (run with `-m gpu` on an MI355X): the HIP path, called through the C ABI, against the CPU
oracle on the same seeded inputs.  Integers (cull, radii, tiles, depth keys, sort order, ranges, n_contrib,
dominant index) bit-exact; pixels and gradients within 1e-5 (north_star), threshold-flip aware."""
import math

import os
import sys

import numpy as np
import pytest
import torch

from tests import helpers as h

pytestmark = pytest.mark.gpu


_ORACLE_FWD = {}       # (cfg, P, t, degree) -> oracle forward of the unmodified scene: the full-size cases run once with the test
                       # options and once with the library's defaults (the timed configuration) against the same oracle result


def _fwd_bwd(cfg, P=None, t=0, sh_degree=3, grad_acc_zero=False, mutate=None, subpixel=None, seed=3, max_fragile_frac=2e-3, noise_orders=8, dir_scale=0.1, grads=None, **fwd_over):
    """dir_scale = 0: every dir3D is zero, the caller's case (gaussian_renderer/__init__.py:66-70 passes the zero gradient trap) and
    the one bench.py times -- the flow-free forward kernel with the hand-scheduled entry walk is launched; any other value exercises the kernel with flow.
    grads: optional callable(oracle forward) -> the four upstream gradients [colour, depth, flow, acc] (default: scene.upstream_grads); any of
    the last three may be None -- the HIP backward then gets a null pointer, the oracle zeros.  What was passed on, after the
    fragile-pixel mask, comes back as rep["upstream"]."""
    from oracle import oracle
    ins, st = h.scene_inputs(cfg, P=P, t=t, sh_degree=sh_degree, dir_scale=dir_scale)
    st.update(fwd_over)
    if mutate:
        mutate(ins, st)
    key = (cfg, P, t, sh_degree, dir_scale) if (isinstance(cfg, str) and mutate is None and subpixel is None and not fwd_over) else None
    if key is not None and key in _ORACLE_FWD:
        o = _ORACLE_FWD[key]
    else:
        o = h.oracle_forward(ins, st, subpixel_offset=subpixel)
        if key is not None and (o["P"] >= 50_000):
            _ORACLE_FWD.clear()                        # one large scene at a time (a 1.0 M forward holds ~1 GB)
            _ORACLE_FWD[key] = o
    g = h.gpu_forward_raw(ins, st, subpixel_offset=subpixel)
    rep = h.compare_forward(o, g, max_fragile_frac=max_fragile_frac, tag=f"{cfg if isinstance(cfg, str) else cfg.name} P={o['P']} t={t}")
    H, W = st["image_height"], st["image_width"]
    grads = list(h.upstream_grads(torch.from_numpy(o["acc"]), H, W, seed=seed, grad_acc_zero=grad_acc_zero) if grads is None else grads(o))
    solid = torch.from_numpy(o["fragile"] > h.FRAG_EPS)
    passed = [None if x is None else x * solid[None] for x in grads]          # a flipped pair changes the whole pixel: exclude fragile pixels
    grads = [torch.zeros(n, H, W) if x is None else x for x, n in zip(passed, (3, 1, 3, 1))]      # (the oracle's: absent = zeros)
    # The backward consumes the forward's per-pixel state (out_depth, out_acc, final_T, n_contrib).  dL_dalpha contains
    # (final_depth - depth) * dL_ddepth, a difference of nearly equal depths, so a 1e-6 relative difference in out_depth
    # (forward rounding, already checked above) would be amplified ~1e2-1e3x into the gradients.  To test the BACKWARD
    # kernels in isolation the oracle backward therefore runs on the GPU forward's state.
    ob_state = dict(o)
    ob_state.update(depth=h.to_np(g["depth"]), acc=h.to_np(g["acc"]), final_T=np.ascontiguousarray(h.to_np(g["final_T"])),
                    n_contrib=np.ascontiguousarray(h.to_np(g["n_contrib"]).astype(np.uint32)))
    ob = oracle.backward(ob_state, *grads)
    # the reference's own noise floor: the same backward replayed in float32 with the pixels in `noise_orders` random orders
    # (its atomicAdd order changes from run to run, CR/backward.cu:613-679); the HIP error is asserted in multiples of that spread
    noise = oracle.backward_noise(ob_state, *grads, orders=noise_orders) if noise_orders else None
    gb = h.gpu_backward_raw(ins, g, passed)
    rep.update(h.compare_backward(ob, gb, o, noise=noise, tag=f"{cfg if isinstance(cfg, str) else cfg.name} P={o['P']} t={t} (oracle backward on the GPU forward's state)"))
    # end to end: oracle(forward -> backward) against GPU(forward -> backward), nothing shared but the inputs.  The oracle's own
    # forward state differs from the GPU's by forward rounding (<= 1e-5, checked above), which the backward amplifies where a term is
    # ill-conditioned in that state -- (final_depth - depth) dL_ddepth / acc at small acc.  Round 4: that amplification is MODELLED,
    # not absorbed into a wider bar: the oracle's backward takes the measured per-pixel state differences and returns the first-order
    # bound on what they move per accumulator (state13); the bars are the shared-state ones (1e-5, 64 half-ulps) + 2 x state13.
    dstate = [np.abs(o[k].astype(np.float64) - h.to_np(g[k]).astype(np.float64)).astype(np.float32).reshape(H, W) for k in ("depth", "acc", "final_T")]
    # the allowance is computed from the MEASURED state difference, so that difference is capped first (otherwise a larger
    # forward error would buy a wider backward bar): on the pixels that carry gradients it must be inside the forward's own 1e-5 bar
    solid_np = solid.numpy().reshape(H, W)
    rep["state_delta_max"] = {k: float((d * solid_np).max()) for k, d in zip(("depth", "acc", "final_T"), dstate)}
    for k, d in zip(("depth", "acc", "final_T"), dstate):
        cap = 1e-5 * max(1.0, float(np.abs(o[k]).max()))
        assert float((d * solid_np).max()) <= cap, f"forward state {k} differs by {float((d * solid_np).max()):.3e} (> {cap:.1e}) on non-fragile pixels: no backward allowance is derived from that"
    ob_e2e = oracle.backward(o, *grads, state_delta=dstate)
    rep["e2e"] = h.compare_backward(ob_e2e, gb, o, extra13=2.0 * ob_e2e["state13"], tag=f"{cfg if isinstance(cfg, str) else cfg.name} P={o['P']} t={t} END-TO-END")
    # per-Gaussian backward stage in isolation: feed the GPU's own accumulators to the oracle's stage
    h.assert_per_gaussian_stage_bit_exact(o, gb, ob)
    rep["upstream"] = passed
    return o, g, ob, gb, rep


def test_cfg1_forward_backward(hip_lib_both):
    _fwd_bwd("cfg1")


@pytest.mark.parametrize("cfg,P,t", [("cfg1", None, 0), ("cfg2", 20000, 0), ("cfg3", 12000, 137), ("cfg5", 6000, 0)])
def test_zero_dir3D_integer_pixels_fast_path(hip_lib_both, cfg, P, t):
    """What render() and bench.py actually pass: dir3D = 0 (the gradient trap) and a zero subpixel_offset -- the forward kernel's
    flow-free variant with the per-row exponent table, which no other parity case reaches (they carry random dir3D)."""
    o, g, ob, gb, rep = _fwd_bwd(cfg, P=P, t=t, dir_scale=0.0)
    assert float(np.abs(o["flow"]).max()) == 0.0 and float(g["flow"].abs().max()) == 0.0


def test_cfg1_training_grads(hip_lib_both):
    _fwd_bwd("cfg1", grad_acc_zero=True, seed=9)


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_sh_degrees(hip_lib_both, deg):
    _fwd_bwd("cfg1", sh_degree=deg)


def test_static_20k_full_resolution(hip_lib_both):
    o, *_ = _fwd_bwd("cfg2", P=20000)
    assert o["W"] == 1352 and o["H"] == 1014          # 1352 = 84*16+8, 1014 = 63*16+6: partial edge tiles


@pytest.mark.parametrize("t", [0, 137, 299])
def test_dynamic_keyframed_scene(hip_lib_both, t):
    _fwd_bwd("cfg3", P=12000, t=t)


def test_deep_overlap_offcentre_projection(hip_lib_both):
    o, *_ = _fwd_bwd("cfg5", P=6000)
    assert o["num_rendered"] / max(1, (o["radii"] > 0).sum()) > 10


def test_subpixel_offsets_and_scale_modifier(hip_lib_both):
    g = torch.Generator().manual_seed(5)
    sub = (torch.rand(256, 256, 2, generator=g) - 0.5)
    _fwd_bwd("cfg1", subpixel=sub, scale_modifier=1.3)


def test_colors_precomp_and_cov3d_precomp_paths(hip_lib_both):
    def mutate(ins, st):
        P = ins["means3D"].shape[0]
        g = torch.Generator().manual_seed(2)
        ins["colors_precomp"] = torch.rand(P, 3, generator=g)
        ins["shs"] = None
        # cov3D from scale/rotation in numpy (R S^2 R^T, raw quaternion) -> the precomputed path
        s, q = ins["scales"].numpy().astype(np.float64), ins["rotations"].numpy().astype(np.float64)
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z),
                      2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(P, 3, 3)
        S = R * s[:, None, :]
        Sig = S @ S.transpose(0, 2, 1)
        ins["cov3D_precomp"] = torch.tensor(np.stack([Sig[:, 0, 0], Sig[:, 0, 1], Sig[:, 0, 2], Sig[:, 1, 1], Sig[:, 1, 2], Sig[:, 2, 2]], -1), dtype=torch.float32)
        ins["scales"] = None
        ins["rotations"] = None
    _fwd_bwd("cfg1", mutate=mutate)


def test_depth_ties_giant_gaussian_and_degenerates(hip_lib_both):
    def mutate(ins, st):
        m = ins["means3D"]
        m[10:40, 2] = 12.5                          # 30 exact depth ties -> order must fall back to ascending id
        m[10:40, :2] *= 0.2
        ins["scales"][5] = torch.tensor([30.0, 30.0, 30.0])      # one Gaussian covering every tile
        ins["scales"][6] = torch.tensor([1e-9, 1e-9, 1e-9])      # degenerate covariance -> coef == 0
        ins["opacities"][7] = 0.0
        ins["opacities"][8] = 1.0
        ins["means3D"][9] = torch.tensor([0.0, 0.0, 4.6])
        ins["scales"][9] = torch.tensor([0.5, 0.5, 0.5])         # large, opaque, close: alpha clamps at 0.99
    o, g, *_ = _fwd_bwd("cfg1", mutate=mutate)
    T = ((o["W"] + 15) // 16) * ((o["H"] + 15) // 16)
    assert int(o["tiles_touched"][5]) == T


def test_empty_and_invisible(hip_lib_both):
    from ex4dgs_amd import _C
    ins, st = h.scene_inputs("cfg1")
    # P == 0 (DGR/rasterize_points.cu:90,189)
    empty = {k: (v[:0] if v is not None else None) for k, v in ins.items()}
    g = h.gpu_forward_raw(empty, st)
    assert g["num_rendered"] == 0 and g["color"].shape == (3, 256, 256) and float(g["color"].abs().sum()) == 0.0
    assert int((g["idx"] != -1).sum()) == 0
    gb = h.gpu_backward_raw(empty, g, [torch.zeros(3, 256, 256), torch.zeros(1, 256, 256), torch.zeros(3, 256, 256), torch.zeros(1, 256, 256)])
    assert gb["dL_dmeans3D"].shape == (0, 3) and gb["dL_dsh"].shape == (0, 0, 3)
    # nothing visible: everything behind the near plane -> R == 0, image = background, depth = max_depth
    ins2 = dict(ins); ins2["means3D"] = ins["means3D"].clone(); ins2["means3D"][:, 2] = 1.0
    o = h.oracle_forward(ins2, st)
    g = h.gpu_forward_raw(ins2, st)
    assert o["num_rendered"] == 0 and g["num_rendered"] == 0
    h.compare_forward(o, g)
    assert torch.allclose(g["color"].cpu(), st["bg"].view(3, 1, 1).expand(3, 256, 256))
    assert float(g["depth"].min()) == st["max_depth"]
    gb = h.gpu_backward_raw(ins2, g, [torch.randn(3, 256, 256), torch.randn(1, 256, 256), torch.randn(3, 256, 256), torch.randn(1, 256, 256)])
    for k, v in gb.items():
        assert float(v.abs().sum()) == 0.0, k


def test_mark_visible_and_errors(hip_lib):
    from ex4dgs_amd import _C
    from ex4dgs_amd.diff_gaussian_rasterization_df import GaussianRasterizer
    from oracle import oracle
    ins, st = h.scene_inputs("cfg2", P=5000)
    s = h.gpu_settings(st, "cuda")
    r = GaussianRasterizer(s)
    vis = r.markVisible(ins["means3D"].cuda())
    ref = oracle.mark_visible(ins["means3D"], st["viewmatrix"], st["projmatrix"], st["min_depth"], st["max_depth"])
    assert np.array_equal(vis.cpu().numpy(), ref)
    d = {k: v.cuda() for k, v in ins.items()}
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        r(d["means3D"], None, d["dir3D"], d["opacities"], shs=None, colors_precomp=None, scales=d["scales"], rotations=d["rotations"])
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair"):
        r(d["means3D"], None, d["dir3D"], d["opacities"], shs=d["shs"], scales=d["scales"], rotations=d["rotations"], cov3D_precomp=torch.zeros(5000, 6).cuda())
    with pytest.raises(RuntimeError, match="means3D must have dimensions"):
        r(d["means3D"].view(-1), None, d["dir3D"], d["opacities"], shs=d["shs"], scales=d["scales"], rotations=d["rotations"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r(ins["means3D"], None, ins["dir3D"], ins["opacities"], shs=ins["shs"], scales=ins["scales"], rotations=ins["rotations"])
    # prefiltered=True with culled Gaussians: the reference traps on the device, here a RuntimeError
    s2 = s._replace(prefiltered=True)
    behind = d["means3D"].clone(); behind[:10, 2] = 1.0          # 10 Gaussians in front of the near plane -> culled
    with pytest.raises(RuntimeError, match="filtered although prefiltered"):
        GaussianRasterizer(s2)(behind, None, d["dir3D"], d["opacities"], shs=d["shs"], scales=d["scales"], rotations=d["rotations"])


def test_autograd_surface_matches_raw_and_render_glue(hip_lib):
    """GaussianRasterizer through torch autograd + the render() glue == the raw `_C` calls; debug mode works."""
    from ex4dgs_amd.render import render
    from ex4dgs_amd.scene import make_scene
    dev = torch.device("cuda")
    model, cam, bg = make_scene("cfg3", P=8000, device=dev)
    for p in model.parameters():
        p.requires_grad_(True)
    cam = cam.to(dev)
    out = render(cam, model, None, bg, timestamp=137, near=4.0, far=300.0)
    assert set(out) == {"render", "depth", "opticalflow", "acc", "viewspace_points", "viewspace_l1points", "dominent_idxs", "visibility_filter", "radii"}
    H, W = cam.image_height, cam.image_width
    grads = [x.to(dev) for x in h.upstream_grads(out["acc"].detach().cpu(), H, W, seed=1)]
    torch.autograd.backward([out["render"], out["depth"], out["opticalflow"], out["acc"]], grads)
    with torch.no_grad():
        ins = dict(means3D=model.get_xyz_at_t(137), rotations=model.get_rotation_at_t(137), opacities=model.get_opacity_at_t(137),
                   scales=model.get_scaling(), shs=model.get_features(), dir3D=torch.zeros(8000, 3, device=dev))
    st = dict(bg=bg, viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, campos=cam.camera_center,
              image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5), kernel_size=0.1,
              sh_degree=3, min_depth=4.0, max_depth=300.0, scale_modifier=1.0, prefiltered=False)
    g = h.gpu_forward_raw(ins, st)
    assert torch.equal(g["color"], out["render"]) and torch.equal(g["radii"], out["radii"]) and torch.equal(g["idx"], out["dominent_idxs"])
    gb = h.gpu_backward_raw(ins, g, grads)
    # atomics make float sums order-dependent run to run: compare with a tolerance relative to the row scale
    a, b = out["viewspace_points"].grad, gb["dL_dmeans2D"]
    assert float((a - b).abs().max()) <= 1e-4 * max(1.0, float(b.abs().max()))
    assert float((out["viewspace_l1points"].grad - gb["dL_ddir"]).abs().max()) <= 1e-4 * max(1.0, float(gb["dL_ddir"].abs().max()))
    for p in model.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all()
    assert (out["visibility_filter"] == (out["radii"] > 0)).all()
    pipe = type("P", (), dict(convert_SHs_python=False, compute_cov3D_python=False, debug=True))()
    out2 = render(cam, model, pipe, bg, timestamp=137, near=4.0, far=300.0)
    assert torch.equal(out2["render"], out["render"])


def test_forward_is_deterministic(hip_lib):
    ins, st = h.scene_inputs("cfg2", P=30000)
    a = h.gpu_forward_raw(ins, st)
    b = h.gpu_forward_raw(ins, st)
    for k in ("color", "depth", "acc", "flow", "idx", "radii", "point_list", "ranges", "n_contrib", "final_T"):
        assert torch.equal(a[k], b[k]), k


def test_full_size_properties_1M(hip_lib):
    """BASELINE config 3 at full size (1.0M Gaussians, 1352x1014): size-independent invariants of the path."""
    ins, st = h.scene_inputs("cfg3", t=137)
    g = h.gpu_forward_raw(ins, st)
    P, R = ins["means3D"].shape[0], g["num_rendered"]
    H, W = st["image_height"], st["image_width"]
    T = ((W + 15) // 16) * ((H + 15) // 16)
    radii, tiles = g["radii"], g["tiles_touched"].long()
    assert P == 1_000_000 and int(tiles.sum()) == R
    assert bool(((radii > 0) == (tiles > 0)).all())
    V = int((radii > 0).sum())
    assert 4.0 <= R / V <= 10.0, R / V                 # SURVEY.md 8(d) acceptance window
    tile_ids, plist, ranges = g["tile_ids"].long(), g["point_list"].long(), g["ranges"].long()
    assert bool((tile_ids[1:] >= tile_ids[:-1]).all()), "instances not sorted by tile"
    depth_of = g["depths"][plist]
    same = tile_ids[1:] == tile_ids[:-1]
    assert bool((depth_of[1:][same] >= depth_of[:-1][same]).all()), "not depth-sorted inside a tile"
    tie = same & (depth_of[1:] == depth_of[:-1])
    assert bool((plist[1:][tie] > plist[:-1][tie]).all()), "depth ties must keep ascending Gaussian id (stable sort)"
    # ranges partition [0, R): counts per tile match a histogram of the tile ids
    counts = torch.bincount(tile_ids, minlength=T)
    assert torch.equal(ranges[:, 1] - ranges[:, 0], counts)
    nz = counts > 0
    assert torch.equal(ranges[nz][:, 0], (torch.cumsum(counts, 0) - counts)[nz])
    # every Gaussian appears exactly tiles_touched times
    assert torch.equal(torch.bincount(plist, minlength=P), tiles)
    # per-pixel state
    n_contrib = g["n_contrib"].long()
    ty, tx = torch.meshgrid(torch.arange(H, device="cuda") // 16, torch.arange(W, device="cuda") // 16, indexing="ij")
    assert bool((n_contrib <= counts[ty * ((W + 15) // 16) + tx]).all())
    acc, fT = g["acc"][0], g["final_T"]
    assert float((acc + fT - 1.0).abs().max()) < 2e-5, "acc + final_T == 1 (sum of alpha*T telescopes)"
    assert bool(((g["idx"][0] >= 0) == (acc > 0)).all())
    assert bool(torch.isfinite(g["color"]).all())
    # linearity of the backward in the upstream gradient: bwd(g1 + g2) == bwd(g1) + bwd(g2)
    gr1 = [x.cuda() for x in h.upstream_grads(acc.cpu(), H, W, seed=1)]
    gr2 = [x.cuda() for x in h.upstream_grads(acc.cpu(), H, W, seed=2, grad_acc_zero=False)]
    d = {k: v.cuda() for k, v in ins.items()}
    b1 = h.gpu_backward_raw(d, g, gr1)["acc16"].clone()
    b2 = h.gpu_backward_raw(d, g, gr2)["acc16"].clone()
    b12 = h.gpu_backward_raw(d, g, [a + b for a, b in zip(gr1, gr2)])["acc16"].clone()
    # dL_dopacity's grad_acc term compounds T (nonlinear in nothing else): everything is linear in the upstream grads
    err = (b12 - (b1 + b2)).abs()
    scale = b12.abs().max(0)[0].clamp_min(1.0)
    assert float((err / scale).max()) < 1e-3


@pytest.mark.parametrize("P", [1, 63, 65, 257, 1000])
def test_odd_sizes(hip_lib_both, P):
    """Gaussian counts that are not multiples of the wave (64) / workgroup (256) / radix chunk sizes."""
    _fwd_bwd("cfg1", P=P)


def test_sh_storage_smaller_than_16(hip_lib_both):
    """shs[P,4,3] with sh_degree 1: M != 16 takes the un-staged SH path (stride stays M, CR/forward.cu:29)."""
    def mutate(ins, st):
        ins["shs"] = ins["shs"][:, :4, :].contiguous()
    _fwd_bwd("cfg1", sh_degree=1, mutate=mutate)


def _with_tile_sort_rows(rows, run):
    """run() with the option "tile_sort_rows" set to `rows`; what it was comes back whatever run() does"""
    from ex4dgs_amd import _C
    saved = _C.get_option("tile_sort_rows")
    try:
        _C.set_option("tile_sort_rows", rows)
        return run()
    finally:
        _C.set_option("tile_sort_rows", saved)


@pytest.mark.parametrize("tile_sort_rows", [1, 0])
def test_technicolor_resolution_14_bit_tiles(hip_lib, tile_sort_rows):
    """2048x1088 = 128x68 = 8704 tiles, 14 tile bits.  tile_sort_rows = 1 (the default): the row-segment sort -- 68 tile rows
    (rows_seg_scatter_kernel<128, .>), pass B with 7-bit columns.  tile_sort_rows = 0: the MSD pair sort with a 7-bit high and a 7-bit
    low digit (TS_SCATTER_A(7), TS_SCATTER_B(7)), which this test was written for and which the default stopped reaching when the
    row-segment sort became it."""
    o, g, *_ = _with_tile_sort_rows(tile_sort_rows, lambda: _fwd_bwd("cfg5", P=3000, t=0))
    assert o["W"] == 2048 and o["H"] == 1088 and o["ranges"].shape[0] == 8704


def test_backward_reproducible_to_rounding(hip_lib):
    """Float atomics sum in arbitrary order (as in the reference): two runs agree to rounding, not bit-wise."""
    ins, st = h.scene_inputs("cfg2", P=30000)
    g = h.gpu_forward_raw(ins, st)
    grads = h.upstream_grads(g["acc"].cpu(), st["image_height"], st["image_width"], seed=4)
    a = h.gpu_backward_raw(ins, g, grads)
    b = h.gpu_backward_raw(ins, g, grads)
    for k in ("dL_dmeans2D", "dL_dmeans3D", "dL_dsh", "dL_dscales", "dL_drotations", "dL_dopacity"):
        scale = a[k].abs().amax(dim=tuple(range(1, a[k].dim())), keepdim=True).clamp_min(1.0)
        assert float(((a[k] - b[k]).abs() / scale).max()) < 1e-4, k


def test_full_size_deep_overlap_forward_cfg5(hip_lib):
    """BASELINE config 5 at full size (1.0M large-footprint Gaussians, 2048x1088, off-centre projection), forward only."""
    ins, st = h.scene_inputs("cfg5")
    g = h.gpu_forward_raw(ins, st)
    R = g["num_rendered"]
    V = int((g["radii"] > 0).sum())
    assert 15.0 <= R / V <= 40.0, R / V                   # SURVEY.md 8(d) acceptance window for the deep-overlap scene
    tile_ids = g["tile_ids"].long()
    assert bool((tile_ids[1:] >= tile_ids[:-1]).all())
    counts = torch.bincount(tile_ids, minlength=8704)
    rng = g["ranges"].long()
    assert torch.equal(rng[:, 1] - rng[:, 0], counts)
    assert float((g["acc"][0] + g["final_T"] - 1.0).abs().max()) < 5e-5
    assert bool(torch.isfinite(g["color"]).all()) and bool(torch.isfinite(g["depth"]).all())
    assert int(torch.bincount(g["point_list"].long(), minlength=ins["means3D"].shape[0]).sum()) == R


# ------------------------------------------------------------------ 8f-1: fused static+dynamic attribute evaluation
def _np_params(model):
    return {n: getattr(model, n).detach().cpu().numpy() for n in model.PARAM_NAMES}


@pytest.mark.parametrize("t", [0, 7, 137, 290, 299])
def test_fused_attributes_match_reference_goldens(hip_lib, t):
    """HIP op vs the outputs and autograd gradients of the reference's CGaussianModel getters (tests/golden/model_getters.npz)."""
    import os
    from ex4dgs_amd.attributes import evaluate_attributes, PARAM_ORDER
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_getters.npz"))
    shapes = {"_xyz_motion": (0, 35, 3), "_rotation_motion": (0, 35, 4), "_opacity_motion": (0, 1), "_opacity_duration_center": (0, 2, 1),
              "_opacity_duration_var": (0, 2, 1), "_scaling_motion": (0, 3), "_features_dc_motion": (0, 1, 3), "_features_rest_motion": (0, 15, 3)}
    for tag in ("small", "staticonly"):
        params = {}
        for n in PARAM_ORDER:
            a = z[f"{tag}/param/{n}"]
            if a.size == 0:
                a = np.zeros(shapes[n], np.float32)
            params[n] = torch.tensor(a, device="cuda").requires_grad_(True)
        outs = evaluate_attributes(params, t, duration=300, interval=10, time_shift=12, var_pad=3)
        for o, k in zip(outs, ("xyz", "rot", "opa", "scl", "fea")):
            ref = z[f"{tag}/t{t}/{k}"]
            assert o.shape == ref.shape and np.abs(o.detach().cpu().numpy() - ref).max() <= 1e-6, (tag, t, k)
        wts = [torch.tensor(z[f"{tag}/weight/{k}"], device="cuda") for k in ("xyz", "rot", "opa", "scl", "fea")]
        sum((o * w).sum() for o, w in zip(outs, wts)).backward()
        for n in PARAM_ORDER:
            key = f"{tag}/t{t}/grad/{n}"
            if key in z.files:
                ref = z[key]
                got = params[n].grad.cpu().numpy()
                assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max()), (tag, t, n, np.abs(got - ref).max())


def test_fused_attributes_vs_oracle_at_scale_and_render_equivalence(hip_lib):
    """200k Gaussians (20 % dynamic): HIP op vs oracle/model_oracle.py (numpy float32 restatement, itself pinned to the
    goldens), then render() with the fused model == render() with the torch getters."""
    from oracle import model_oracle as mo
    from ex4dgs_amd.attributes import evaluate_attributes
    from ex4dgs_amd.render import render
    from ex4dgs_amd.scene import make_scene
    dev = torch.device("cuda")
    model, cam, bg = make_scene("cfg3", P=200_000, device=dev)
    cam = cam.to(dev)
    for p in model.parameters():
        p.requires_grad_(True)
    t = 137
    params = {n: getattr(model, n) for n in model.PARAM_NAMES}
    outs = evaluate_attributes(params, t)
    ref = mo.forward(_np_params(model), t)
    for o, k in zip(outs, ("means3D", "rotations", "opacities", "scales", "shs")):
        a, b = o.detach().cpu().numpy(), ref[k]
        assert np.abs(a - b).max() <= 2e-6 * max(1.0, np.abs(b).max()), k
    g = torch.Generator().manual_seed(3)
    wts = [torch.randn(o.shape, generator=g).to(dev) for o in outs]
    sum((o * w).sum() for o, w in zip(outs, wts)).backward()
    gref = mo.backward(_np_params(model), t, dict(zip(("means3D", "rotations", "opacities", "scales", "shs"), [w.cpu().numpy() for w in wts])))
    for n in model.PARAM_NAMES:
        a, b = getattr(model, n).grad.cpu().numpy(), gref[n]
        scale = np.maximum(np.abs(b).reshape(b.shape[0], -1).max(1), 1.0).reshape((-1,) + (1,) * (b.ndim - 1))
        assert (np.abs(a - b) / scale).max() <= 2e-5, (n, (np.abs(a - b) / scale).max())
    # the getters of a fused model feed the rasterizer the same tensors as the torch getters
    model.zero_grad = lambda: [setattr(p, "grad", None) for p in model.parameters()]
    model.zero_grad()
    plain = render(cam, model, None, bg, timestamp=t, near=4.0, far=300.0)
    plain["render"].sum().backward()
    g_plain = model._xyz_motion.grad.clone()
    model.zero_grad()
    model.fused = True
    fused = render(cam, model, None, bg, timestamp=t, near=4.0, far=300.0)
    fused["render"].sum().backward()
    assert torch.equal(fused["radii"], plain["radii"])
    assert float((fused["render"] - plain["render"]).abs().max()) <= 1e-5
    ga, gb = model._xyz_motion.grad, g_plain
    assert float((ga - gb).abs().max()) <= 1e-4 * max(1.0, float(gb.abs().max()))


# ------------------------------------------------------------------ 8f-2: fused L1 + SSIM loss
def _check_loss(hip_lib, image, gt, lam, expect=None, flat=False):
    """Against the float64 oracle.  `flat`: SSIM divides by (sigma1^2 + sigma2^2 + C2); in flat image regions float32 rounding
    of the window means (~2^-23 of E[x^2]+E[y^2]) is amplified by up to 1/C2 = 1.1e3, and the reference's own float32 result
    moves by the same amount against exact arithmetic (tests/test_cpu_oracle_and_host.py pins that), so the per-pixel bar is
    5e-4 there; away from flat regions it is 1e-5.  The scalar loss is held to 1e-6 (3e-6 flat) either way."""
    from oracle import loss_oracle
    from ex4dgs_amd.loss import l1_ssim_loss
    x = torch.tensor(image, device="cuda", requires_grad=True)
    y = torch.tensor(gt, device="cuda")
    loss, l1e, sse = l1_ssim_loss(x, y, lam)
    assert not l1e.requires_grad and not sse.requires_grad
    (loss * 1.0).backward()
    o = loss_oracle.l1_ssim(image, gt, lam)
    gmax = np.abs(o["grad"]).max()
    tol_map = 5e-4 if flat else 1e-5
    tol_grad = (2e-3 if flat else 1e-5) * gmax + 1e-9
    assert abs(loss.item() - o["loss"]) < (3e-6 if flat else 1e-6), (loss.item(), o["loss"])
    np.testing.assert_allclose(l1e.cpu().numpy(), o["l1_errors"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(sse.cpu().numpy(), o["ssim_errors"], rtol=0, atol=tol_map)
    np.testing.assert_allclose(x.grad.cpu().numpy(), o["grad"], rtol=0, atol=tol_grad)
    if expect is not None:                         # the reference's own float32 outputs
        assert abs(loss.item() - float(expect["loss"])) < 3e-6
        np.testing.assert_allclose(x.grad.cpu().numpy(), expect["grad"], rtol=0, atol=(4e-3 if flat else 2e-5) * gmax)
        np.testing.assert_allclose(sse.cpu().numpy(), expect["ssim_errors"], rtol=0, atol=1e-3 if flat else 2e-5)
        np.testing.assert_allclose(l1e.cpu().numpy(), expect["l1_errors"], rtol=0, atol=1e-6)
    return loss, x.grad


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["noise", "smooth", "tiny"])
@pytest.mark.parametrize("lam", [0.2, 0.5])
def test_fused_loss_matches_reference_goldens(hip_lib, name, lam):
    g = np.load(os.path.join(h.ROOT, "tests", "golden", "loss_l1_ssim.npz"))
    k = f"{name}/lam{lam}/"
    _check_loss(hip_lib, g[name + "/image"], g[name + "/gt"], lam,
                expect={q: g[k + q] for q in ("loss", "grad", "l1_errors", "ssim_errors")}, flat=(name == "smooth"))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 16, 16), (3, 1, 1), (3, 17, 33), (1, 40, 23), (4, 5, 64), (3, 507, 676)])
def test_fused_loss_vs_oracle_shapes(hip_lib, shape):
    rng = np.random.default_rng(sum(shape))
    gt = rng.random(shape, dtype=np.float32)
    image = np.clip(gt + 0.15 * rng.standard_normal(shape), 0, 1).astype(np.float32)
    image[0, 0, 0] = gt[0, 0, 0]                   # |x - y| has a zero: sign(0) = 0 like torch.abs
    _check_loss(hip_lib, image, gt, 0.2)


@pytest.mark.gpu
def test_fused_loss_on_a_render_full_size_and_upstream_scale(hip_lib):
    """Full N3V resolution on an actual render (large flat background = the ill-conditioned SSIM case), gradient flows
    through the rasterizer, upstream grad scaling is honoured, repeat calls are bit-identical."""
    from ex4dgs_amd.loss import l1_ssim_loss
    from ex4dgs_amd.scene import make_scene
    from ex4dgs_amd.render import render
    model, cam, bg = make_scene("cfg2", P=60000, device="cuda")
    for p_ in model.parameters():
        p_.requires_grad_(True)
    out = render(cam, model, None, bg, timestamp=0, near=4.0, far=300.0)
    image = out["render"]
    gt = (image.detach() * 0.9 + 0.05 * torch.rand_like(image)).clamp(0, 1)
    img_leaf = image.detach().clone().requires_grad_(True)
    l1, a1, s1 = l1_ssim_loss(img_leaf, gt, 0.2)
    (l1 * 3.0).backward()
    g3 = img_leaf.grad.clone()
    img_leaf.grad = None
    l2, a2, s2 = l1_ssim_loss(img_leaf, gt, 0.2)
    l2.backward()
    assert torch.equal(l1, l2) and torch.equal(a1, a2) and torch.equal(s1, s2)
    torch.testing.assert_close(g3, 3.0 * img_leaf.grad, rtol=1e-6, atol=0)
    _check_loss(hip_lib, image.detach().cpu().numpy(), gt.cpu().numpy(), 0.2, flat=True)
    # end to end: the loss backpropagates into the Gaussians through the rasterizer; the hook tensor of train.py:151
    loss, l1e, sse, hook = l1_ssim_loss(image, gt, 0.2, acc=out["acc"])
    assert torch.equal(hook, torch.stack([out["acc"].detach()[0], a1, s1])) and torch.equal(l1e, a1) and torch.equal(loss.detach(), l1.detach())
    loss.backward()
    gsum = sum(float(p.grad.abs().sum()) for p in model.parameters() if p.grad is not None)
    assert np.isfinite(gsum) and gsum > 0


# ------------------------------------------------------------------ 8f-3: fused RAdam
@pytest.mark.gpu
def test_fused_radam_follows_torch_trajectories(hip_lib):
    """tests/golden/radam.npz: 12 steps of torch.optim.RAdam over 4 tensors with per-step learning rates, a tensor without
    gradient on two steps, an all-zero gradient step, crossing the rho_t > 5 switch."""
    from ex4dgs_amd.optim import FusedRAdam
    from tests.test_cpu_oracle_and_host import radam_golden_replay
    g0 = np.load(os.path.join(h.ROOT, "tests", "golden", "radam.npz"))
    n = int(g0["n_params"])
    params = [torch.nn.Parameter(torch.tensor(g0[f"p{i}/init"], device="cuda")) for i in range(n)]
    opt = FusedRAdam([{"params": [p], "lr": 1.0, "name": str(i)} for i, p in enumerate(params)], lr=0.001)

    def step(i, it, grad, lr):
        opt.param_groups[i]["lr"] = lr
        params[i].grad = None if grad is None else torch.tensor(grad, device="cuda")
        if i == n - 1:
            opt.step()
            for j in range(n):
                ref = g0[f"p{j}/after{it}"]
                np.testing.assert_allclose(params[j].detach().cpu().numpy(), ref, rtol=0, atol=1e-6 * max(1.0, np.abs(ref).max()))
    radam_golden_replay(step)
    for j, p in enumerate(params):
        st = opt.state[p]
        assert float(st["step"]) == float(g0[f"p{j}/step"])
        np.testing.assert_allclose(st["exp_avg"].cpu().numpy(), g0[f"p{j}/exp_avg"], rtol=2e-6, atol=2e-6 * np.abs(g0[f"p{j}/exp_avg"]).max())
        np.testing.assert_allclose(st["exp_avg_sq"].cpu().numpy(), g0[f"p{j}/exp_avg_sq"], rtol=2e-6, atol=2e-6 * np.abs(g0[f"p{j}/exp_avg_sq"]).max())


@pytest.mark.gpu
def test_fused_radam_vs_oracle_on_model_sized_groups(hip_lib):
    """The 15 parameter groups of a 200k-Gaussian model (odd sizes, >1 chunk per tensor, unaligned tails), 8 steps against the
    numpy oracle, bit for bit; state tensors stay editable in place like the reference's densification does."""
    from oracle import optim_oracle
    from ex4dgs_amd.optim import FusedRAdam
    from ex4dgs_amd.scene import make_scene
    model, cam, bg = make_scene("cfg3", P=200_003, device="cuda")
    params = model.parameters()
    for p in params:
        p.requires_grad_(True)
    lrs = [1.6e-4, 1e-3, 2.5e-3, 5e-2, 5e-3, 1e-3, 1e-4, 1.6e-4, 2.5e-3, 1.25e-4, 5e-3, 5e-2, 1e-4, 1e-3, 1e-3]
    opt = FusedRAdam([{"params": [p], "lr": lr, "name": str(i)} for i, (p, lr) in enumerate(zip(params, lrs))], lr=0.001)
    P = [p.detach().cpu().numpy().copy() for p in params]
    M = [np.zeros_like(a) for a in P]; V = [np.zeros_like(a) for a in P]
    gen = torch.Generator(device="cuda").manual_seed(3)
    for it in range(1, 9):
        for i, p in enumerate(params):
            p.grad = torch.randn(p.shape, generator=gen, device="cuda") * (0.1 if i % 2 else 1e-4)
            if it == 4:
                p.grad[::3] = 0                      # rows invisible in this frame: momentum still moves them
            optim_oracle.radam_step(P[i], p.grad.cpu().numpy(), M[i], V[i], it, lrs[i])
        opt.step()
    # bit for bit: the restatement does the kernel's float32 operations in the kernel's order (tests/test_gpu_optim_edges.py)
    for i, p in enumerate(params):
        h.assert_same_bits(p, P[i], None, f"parameter {i}")
        h.assert_same_bits(opt.state[p]["exp_avg"], M[i], None, f"exp_avg {i}")
        h.assert_same_bits(opt.state[p]["exp_avg_sq"], V[i], None, f"exp_avg_sq {i}")
    # state edited in place (what _prune_optimizer / cat_tensors_to_optimizer do) is what the next step uses
    p0 = params[0]
    st = opt.state.pop(p0)
    keep = torch.arange(0, p0.shape[0], 2, device="cuda")
    new_p = torch.nn.Parameter(p0.detach()[keep].clone())
    st["exp_avg"] = st["exp_avg"][keep].clone(); st["exp_avg_sq"] = st["exp_avg_sq"][keep].clone()
    opt.param_groups[0]["params"][0] = new_p
    opt.state[new_p] = st
    new_p.grad = torch.ones_like(new_p)
    for p in params[1:]:
        p.grad = None
    before = new_p.detach().clone()
    opt.step()
    assert float(st["step"]) == 9.0 and not torch.equal(before, new_p.detach())
    ref_p, ref_m, ref_v = P[0][::2].copy(), M[0][::2].copy(), V[0][::2].copy()
    optim_oracle.radam_step(ref_p, np.ones_like(ref_p), ref_m, ref_v, 9, lrs[0])
    h.assert_same_bits(new_p, ref_p, None, "pruned parameter 0")
    h.assert_same_bits(st["exp_avg"], ref_m, None, "pruned exp_avg 0")
    h.assert_same_bits(st["exp_avg_sq"], ref_v, None, "pruned exp_avg_sq 0")


# ------------------------------------------------------------------ 8f-4: distCUDA2 (simple-knn)
@pytest.mark.gpu
def test_dist2_bit_exact_vs_bruteforce(hip_lib):
    """The result is a selection (three smallest float32 distances), not a sum over many terms: bit-exact."""
    from oracle import knn_oracle
    from ex4dgs_amd.simple_knn._C import distCUDA2
    from tests.test_cpu_oracle_and_host import knn_point_sets
    sets = knn_point_sets()
    for name, pts in sets.items():
        got = distCUDA2(torch.tensor(pts, device="cuda")).cpu().numpy()
        assert np.array_equal(got, knn_oracle.dist2_bruteforce(pts)), name
    u = sets["uniform"]
    for P in (1, 2, 3, 4, 5, 63, 64, 65, 127, 1023, 1024, 1025, 2049):
        got = distCUDA2(torch.tensor(u[:P], device="cuda")).cpu().numpy()
        assert np.array_equal(got, knn_oracle.dist2_bruteforce(u[:P])), P
    assert distCUDA2(torch.zeros(0, 3, device="cuda")).shape == (0,)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        distCUDA2(torch.zeros(4, 3))


@pytest.mark.gpu
def test_dist2_at_scale_and_initialisation_use(hip_lib):
    """300k points (scene-like: surfaces + clusters + outliers) against the kd-tree formulation; then the reference's use
    (c_gaussian_model.py:395-396): scales = log(sqrt(clamp_min(dist2, 1e-7)))."""
    from oracle import knn_oracle
    from ex4dgs_amd.simple_knn._C import distCUDA2
    rng = np.random.default_rng(8)
    sheet = np.stack([rng.random(150_000) * 20, rng.random(150_000) * 20, 0.01 * rng.standard_normal(150_000)], 1)
    blobs = np.concatenate([c + 0.3 * rng.standard_normal((14_000, 3)) for c in rng.standard_normal((10, 3)) * 8])
    far = rng.standard_normal((10_000, 3)) * 200
    pts = np.concatenate([sheet, blobs, far]).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    x = torch.tensor(pts, device="cuda")
    got = distCUDA2(x)
    assert np.array_equal(got.cpu().numpy(), knn_oracle.dist2_kdtree(pts, k_search=16))
    assert torch.equal(got, distCUDA2(x))                                   # deterministic
    scales = torch.log(torch.sqrt(torch.clamp_min(got, 0.0000001)))[..., None].repeat(1, 3)
    assert torch.isfinite(scales).all()


# ------------------------------------------------------------------ the pieces together: a short training loop
@pytest.mark.gpu
def test_fused_training_loop_end_to_end(hip_lib):
    """getters (fused) -> render -> L1+SSIM (fused) -> backward -> FusedRAdam, same timestamp twice in a row: the optimizer
    must invalidate the per-timestamp attribute cache (parameter version counters), and the loss must go down."""
    from ex4dgs_amd.scene import make_scene
    from ex4dgs_amd.render import render
    from ex4dgs_amd.loss import l1_ssim_loss
    from ex4dgs_amd.optim import FusedRAdam
    target, cam, bg = make_scene("cfg3", P=30_000, device="cuda", fused=True)
    with torch.no_grad():
        gts = {t: render(cam, target, None, bg, timestamp=t, near=4.0, far=300.0)["render"].clone() for t in (40, 200)}
    model, _, _ = make_scene("cfg3", P=30_000, device="cuda", fused=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    with torch.no_grad():
        model._features_dc += 0.3 * torch.randn(model._features_dc.shape, generator=g, device="cuda")
        model._features_dc_motion += 0.3 * torch.randn(model._features_dc_motion.shape, generator=g, device="cuda")
        model._opacity -= 0.5
    for p in model.parameters():
        p.requires_grad_(True)
    lrs = {"_features_dc": 5e-2, "_features_dc_motion": 5e-2, "_opacity": 5e-2, "_opacity_motion": 5e-2}
    opt = FusedRAdam([{"params": [getattr(model, n)], "lr": lrs.get(n, 1e-4), "name": n} for n in model.PARAM_NAMES], lr=0.001)
    losses = []
    for it in range(40):
        t = (40, 40, 200, 200)[it % 4]
        out = render(cam, model, None, bg, timestamp=t, near=4.0, far=300.0)
        loss, l1e, sse, hook = l1_ssim_loss(out["render"], gts[t], 0.2, acc=out["acc"])
        v0 = model._xyz._version
        loss.backward()
        opt.step()
        assert model._xyz._version > v0
        opt.zero_grad(set_to_none=True)
        losses.append(float(loss))
    assert all(np.isfinite(losses))
    assert np.mean(losses[-4:]) < 0.9 * np.mean(losses[:4]), losses


# ------------------------------------------------------------------ zero-copy SH: the four feature tensors instead of cat()
@pytest.mark.gpu
@pytest.mark.parametrize("Ns,Nd,D", [(3000, 1000, 3), (2999, 1001, 3), (4000, 0, 3), (0, 4000, 3), (1, 3999, 2), (3967, 33, 1), (2000, 2000, 0)])
def test_split_sh_is_bit_identical_to_concatenated(hip_lib, Ns, Nd, D):
    """SplitSH(dc, rest, dc_motion, rest_motion) through the autograd surface == the same call with the concatenated [P,16,3]
    tensor: every output bit-identical, dL/dsh bit-identical after splitting, every other gradient bit-identical."""
    from ex4dgs_amd.diff_gaussian_rasterization_df import GaussianRasterizationSettings, GaussianRasterizer, SplitSH
    from ex4dgs_amd.scene import make_scene
    import math as m
    P = Ns + Nd
    model, cam, bg = make_scene("cfg3", P=P, device="cuda")
    t = 137
    with torch.no_grad():
        means3D, opac, scl, rot = model.get_xyz_at_t(t), model.get_opacity_at_t(t), model.get_scaling(), model.get_rotation_at_t(t)
        feats = model.get_features()                                   # [P,16,3]
    parts = [feats[:Ns, :1].clone(), feats[:Ns, 1:].clone(), feats[Ns:, :1].clone(), feats[Ns:, 1:].clone()]
    H, W = 512, 640
    settings = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=m.tan(cam.FoVx * 0.5), tanfovy=m.tan(cam.FoVy * 0.5), kernel_size=0.1,
        subpixel_offset=torch.zeros(H, W, 2, device="cuda"), bg=bg.cuda(), scale_modifier=1.0, viewmatrix=cam.world_view_transform.cuda(),
        projmatrix=cam.full_proj_transform.cuda(), sh_degree=D, campos=cam.camera_center.cuda(), prefiltered=False,
        min_depth=4.0, max_depth=300.0, debug=False)
    ras = GaussianRasterizer(settings)
    g = torch.Generator(device="cuda").manual_seed(1)
    ups = [torch.randn(3, H, W, generator=g, device="cuda"), torch.randn(1, H, W, generator=g, device="cuda") * 0.1,
           torch.rand(3, H, W, generator=g, device="cuda"), torch.randn(1, H, W, generator=g, device="cuda") * 0.1]

    def run(shs_arg, leaves):
        ins = [x.clone().requires_grad_(True) for x in (means3D, opac, scl, rot)]
        m2d = torch.zeros(P, 3, device="cuda", requires_grad=True); d3 = torch.zeros(P, 3, device="cuda", requires_grad=True)
        out = ras(means3D=ins[0], means2D=m2d, dir3D=d3, opacities=ins[1], shs=shs_arg, scales=ins[2], rotations=ins[3])
        torch.autograd.backward([out[0], out[2], out[3], out[4]], ups)
        return out, [x.grad for x in ins + [m2d, d3]], [l.grad for l in leaves]
    whole = feats.clone().requires_grad_(True)
    out_a, g_a, (gsh_a,) = run(whole, [whole])
    leaves = [p_.clone().requires_grad_(True) for p_ in parts]
    out_b, g_b, gsh_b = run(SplitSH(*leaves), leaves)
    for a, b in zip(out_a, out_b):
        assert torch.equal(a, b)
    # gradients accumulate with float atomics in arbitrary order: reproducible to rounding, like two runs of the same call
    for a, b in zip(g_a, g_b):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6 * float(a.abs().max()) + 1e-12)
    ref_parts = [gsh_a[:Ns, :1], gsh_a[:Ns, 1:], gsh_a[Ns:, :1], gsh_a[Ns:, 1:]]
    for a, b in zip(ref_parts, gsh_b):
        assert a.shape == b.shape
        torch.testing.assert_close(b, a, rtol=1e-4, atol=1e-6 * float(gsh_a.abs().max()) + 1e-12)
        assert torch.equal(b == 0, a == 0)                               # inactive degrees / invisible rows are exact zeros


@pytest.mark.gpu
def test_split_sh_argument_checks(hip_lib):
    from ex4dgs_amd import _C
    from ex4dgs_amd._C import SplitSH
    z = lambda *s: torch.zeros(*s, device="cuda")
    good = SplitSH(z(5, 1, 3), z(5, 15, 3), z(3, 1, 3), z(3, 15, 3))
    assert good.n_static == 5 and good.n_dynamic == 3 and good.size(0) == 8 and good.size(1) == 16
    with pytest.raises(RuntimeError, match="expected"):
        _C._split_struct(SplitSH(z(5, 1, 3), z(5, 14, 3), z(3, 1, 3), z(3, 15, 3)), torch.device("cuda", 0), "sh")
    with pytest.raises(RuntimeError, match="same number of rows"):
        _C._split_struct(SplitSH(z(5, 1, 3), z(4, 15, 3), z(3, 1, 3), z(3, 15, 3)), torch.device("cuda", 0), "sh")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["noise", "smooth", "tiny"])
def test_metric_functions_by_reference_name(hip_lib, name):
    """l1_loss / ssim / psnr with the reference's signatures and call forms (train.py:144-150,182; render.py:76-77)."""
    from ex4dgs_amd.loss import l1_loss, ssim, psnr
    g = np.load(os.path.join(h.ROOT, "tests", "golden", "loss_l1_ssim.npz"))
    x = torch.tensor(g[name + "/image"], device="cuda", requires_grad=True)
    y = torch.tensor(g[name + "/gt"], device="cuda")
    flat = name == "smooth"
    s4 = ssim(x.unsqueeze(0), y.unsqueeze(0))
    assert abs(float(s4) - float(g[name + "/ssim"])) < (3e-6 if flat else 1e-6)
    (1.0 - s4).backward()
    assert x.grad is not None and torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0
    m = ssim(x.detach(), y, reduce=False)
    np.testing.assert_allclose(m.cpu().numpy(), g[name + "/ssim_map"], rtol=0, atol=1e-3 if flat else 2e-5)
    assert abs(float(l1_loss(x, y)) - float(g[name + "/Ll1"])) < 1e-7
    np.testing.assert_allclose(psnr(x.detach().unsqueeze(0), y.unsqueeze(0)).cpu().numpy(), g[name + "/psnr"], rtol=1e-6)


@pytest.mark.gpu
def test_absent_upstream_gradients_equal_zero_gradients(hip_lib):
    """A loss that uses only some of the outputs: autograd passes None for the others; the native backward treats a null
    upstream gradient as zeros, so no zero tensors are materialised -- same result as explicit zeros (to summation order)."""
    from ex4dgs_amd.scene import make_scene
    from ex4dgs_amd.render import render
    model, cam, bg = make_scene("cfg3", P=20_000, device="cuda")
    for p_ in model.parameters():
        p_.requires_grad_(True)

    def grads(loss_fn):
        for p_ in model.parameters():
            p_.grad = None
        out = render(cam, model, None, bg, timestamp=137, near=4.0, far=300.0)
        loss_fn(out).backward()
        return [p_.grad.clone() for p_ in model.parameters()], out["viewspace_points"].grad.clone()
    w = torch.rand(3, cam.image_height, cam.image_width, device="cuda")
    a, a2d = grads(lambda o: (o["render"] * w).sum())
    b, b2d = grads(lambda o: (o["render"] * w).sum() + 0.0 * (o["depth"].sum() + o["opticalflow"].sum() + o["acc"].sum()))
    for x, y in zip(a + [a2d], b + [b2d]):
        torch.testing.assert_close(x, y, rtol=1e-4, atol=1e-6 * float(y.abs().max()) + 1e-12)
    c, _ = grads(lambda o: o["depth"].mean() + o["acc"].mean())          # colour gradient absent
    assert all(torch.isfinite(t).all() for t in c) and float(sum(t.abs().sum() for t in c)) > 0


@pytest.mark.gpu
def test_graft_entry_smoke(hip_lib):
    import __graft_entry__
    __graft_entry__.smoke()


@pytest.mark.gpu
def test_more_than_65535_tiles(hip_lib):
    """4112x4112 = 257x257 = 66049 tiles: 17 tile-key bits (three radix passes) and the plain-division path of the
    instance expansion (its exact multiply-high row/column split is only used up to 65535 tiles)."""
    from ex4dgs_amd.scene import SceneConfig
    cfg = SceneConfig("huge: 4112x4112", 1500, 4112, 4112, 2200.0, seed=31, sigma_px_med=30.0)
    o, g, *_ = _fwd_bwd(cfg)
    assert o["ranges"].shape[0] == 257 * 257 and o["num_rendered"] > 20000


@pytest.mark.gpu
@pytest.mark.parametrize("tile_sort_rows", [1, 0])
@pytest.mark.parametrize("side,bits", [(2300, 15), (2900, 16)])
def test_tile_sort_with_15_and_16_tile_bits(hip_lib, side, bits, tile_sort_rows):
    """144x144 = 20 736 and 182x182 = 33 124 tiles.  tile_sort_rows = 0: the MSD pair sort with 8-bit low digits and 7- / 8-bit high
    digits (TS_SCATTER_A(7) / TS_SCATTER_A(8), TS_SCATTER_B(8), ts_locate_block over 128 / 256 buckets: the compile-time digit widths the
    1352x1014 and 2048x1088 configurations do not reach) -- what this test was written for.  tile_sort_rows = 1 (the default, which
    silently took these scenes over when the row-segment sort became it): rows_seg_scatter_kernel<256, .> over 144 / 182 tile rows and
    pass B with 8-bit columns."""
    from ex4dgs_amd.scene import SceneConfig
    cfg = SceneConfig(f"{side}x{side}", 1200, side, side, side * 0.55, seed=37 + bits, sigma_px_med=22.0)
    o, g, *_ = _with_tile_sort_rows(tile_sort_rows, lambda: _fwd_bwd(cfg))
    T = o["ranges"].shape[0]
    assert T == ((side + 15) // 16) ** 2 and (1 << (bits - 1)) < T <= (1 << bits) and o["num_rendered"] > 10000


@pytest.mark.gpu
def test_edge_cases_of_the_fused_training_path(hip_lib):
    """Static-only model through attributes -> SplitSH render -> loss -> FusedRAdam (empty dynamic tensors everywhere), tiny
    images through the loss, coincident points through distCUDA2, P == 0 through the autograd surface."""
    import runpy
    runpy.run_path(os.path.join(h.ROOT, "tools", "dev", "edge_cases.py"), run_name="__main__")


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed,dir_scale", [(16, 3, 0.1), (70, 7, 0.0)])
def test_randomised_parity_sweep(hip_lib, n, seed, dir_scale):
    """Random scenes (image sizes 17..700, 1..6000 Gaussians, footprints 0.3..25 px, SH degrees 0-3, static/dynamic, off-centre
    projection, kernel sizes, scale modifiers, subpixel offsets) through the full forward + backward comparison, shared-state AND
    end to end (tests/fuzz_sweep.py): 16 cases with flow, and the 70 FLOW-FREE cases of seed 7 -- the frames the hand-scheduled
    forward walk serves; round 3 ran that sweep outside the suite and had one case above the un-modelled end-to-end bar."""
    from tests import fuzz_sweep
    fails = fuzz_sweep.run(n, seed, dir_scale)
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.long
@pytest.mark.parametrize("seed,dir_scale", [(11, 0.1), (12, 0.0), (13, 0.0)])
def test_randomised_parity_sweep_long(hip_lib, seed, dir_scale):
    """The 300 extra random scenes of round 4 (seeds 11-13, 100 each) as a committed, opt-in test:
    `python -m pytest tests -m "gpu and long"`.  Its per-case numbers land in gpurun_out/parity_report.json like every other
    comparison (round 5's run: profiles/r05_long_sweep_report.json.gz)."""
    from tests import fuzz_sweep
    fails = fuzz_sweep.run(100, seed, dir_scale, verbose=False)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------ multi-process data path on the GPU (2 ranks share cuda:0)
_DP_WORKER = r"""
import os, sys, torch
sys.path.insert(0, sys.argv[1])
from ex4dgs_amd import dist as xd
from ex4dgs_amd.scene import make_scene
from ex4dgs_amd.render import render
os.environ["LOCAL_RANK"] = "0"                       # both ranks on the one GPU of the box
rank, world, local = xd.init_from_env(backend="gloo")
model, cam, bg = make_scene("cfg3", P=20000, device="cuda", fused=True)
params = model.parameters()
for p in params:
    p.requires_grad_(True)
views = xd.shard_views(4, rank, world)              # 4 timestamps, round-robin
stamps = [0, 100, 200, 299]
w = torch.rand(3, cam.image_height, cam.image_width, generator=torch.Generator().manual_seed(5)).cuda()
for v in views:
    out = render(cam, model, None, bg, timestamp=stamps[v], near=4.0, far=300.0)
    (out["render"] * w).sum().backward()
grads = [p.grad for p in params]
b = xd.GradBuckets([g.shape for g in grads], device="cuda", bucket_bytes=1 << 20, inplace_bytes=1 << 20)
b.launch(grads); b.wait()
if rank == 0:
    torch.save([g.cpu() for g in grads], sys.argv[2])
torch.distributed.barrier(); torch.distributed.destroy_process_group()
print("OK", rank)
"""


@pytest.mark.gpu
def test_frame_sharded_gradients_equal_single_process_sum(hip_lib, tmp_path):
    """SURVEY 8(e) end to end on real kernels: two processes (sharing this box's one GPU, gloo) render the views
    i = rank (mod 2), all-reduce the parameter gradients through GradBuckets; the result equals one process
    accumulating all four views (to float-atomic summation order)."""
    import subprocess
    from ex4dgs_amd.scene import make_scene
    from ex4dgs_amd.render import render
    script = tmp_path / "dp_worker.py"
    script.write_text(_DP_WORKER)
    out_file = str(tmp_path / "grads.pt")
    port = 29700 + (os.getpid() % 2000)
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script), h.ROOT, out_file], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"OK {r}" in o, o
    got = torch.load(out_file)
    model, cam, bg = make_scene("cfg3", P=20000, device="cuda", fused=True)
    params = model.parameters()
    for p in params:
        p.requires_grad_(True)
    w = torch.rand(3, cam.image_height, cam.image_width, generator=torch.Generator().manual_seed(5)).cuda()
    for t in (0, 100, 200, 299):
        out = render(cam, model, None, bg, timestamp=t, near=4.0, far=300.0)
        (out["render"] * w).sum().backward()
    for name, p, g in zip(model.PARAM_NAMES, params, got):
        torch.testing.assert_close(g.cuda(), p.grad, rtol=2e-4, atol=2e-6 * float(p.grad.abs().max()) + 1e-12, msg=lambda m: f"{name}: {m}")
