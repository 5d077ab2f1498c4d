"""GPU tests of round 4's asynchronous forward (Ex4dParams.instance_capacity): no instance-count read-back, host-constant grids,
the frame status in pinned host memory behind an event; overflow detection and recovery; hipGraph capture and replay."""
import numpy as np
import pytest
import torch

from tests import helpers as h

pytestmark = pytest.mark.gpu


def _raw_forward(ins, st, device="cuda", settings=None, **kw):
    from ex4dgs_amd import _C
    s = h.gpu_settings(st, device) if settings is None else settings      # (building them copies host tensors: not inside a capture)
    e = torch.Tensor([])
    d = lambda k: ins[k].to(device) if ins.get(k) is not None else e
    return s, _C.rasterize_gaussians(s.bg, d("means3D"), d("dir3D"), d("colors_precomp"), d("opacities"), d("scales"), d("rotations"),
                                     s.scale_modifier, d("cov3D_precomp"), s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, s.kernel_size,
                                     s.subpixel_offset, s.image_height, s.image_width, d("shs"), s.sh_degree, s.campos, s.prefiltered,
                                     s.min_depth, s.max_depth, s.debug, **kw)


def _raw_backward(ins, s, fwd, grads, device="cuda", **kw):
    from ex4dgs_amd import _C
    e = torch.Tensor([])
    d = lambda k: ins[k].to(device) if ins.get(k) is not None else e
    R, color, radii, geom, binning, img, depth, acc, flow, idx = fwd
    gc, gd, gf, ga = grads
    return _C.rasterize_gaussians_backward(
        s.bg, d("means3D"), radii, d("colors_precomp"), d("scales"), d("rotations"), depth, acc, s.min_depth, s.max_depth, s.scale_modifier,
        d("cov3D_precomp"), s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, s.kernel_size, s.subpixel_offset, gc, gd, gf, ga, d("shs"),
        s.sh_degree, s.campos, geom, R, binning, img, s.debug, **kw)


def _huge():
    from ex4dgs_amd.scene import SceneConfig
    return SceneConfig("huge: 4112x4112", 1500, 4112, 4112, 2200.0, seed=31, sigma_px_med=30.0)


@pytest.mark.parametrize("cfg,P,dir_scale", [("cfg2", 20000, 0.1), ("cfg3", 12000, 0.0), ("cfg1", None, 0.1), ("huge", None, 0.1)])
def test_asynchronous_forward_equals_the_synchronous_one(hip_lib, cfg, P, dir_scale):
    """Same frame through the reference-style forward (blocking instance-count read-back, exact buffer) and through the asynchronous
    one (capacity-sized buffer, count read from device memory by every kernel behind the scan): every output bit-equal, the sorted
    point list and the tile ranges equal, the status word equal to the synchronous count; the backward on the capacity-sized buffers
    returns the same gradients (to the order of the float atomics).  cfg1 (256x256: 256 tiles) takes the key/value tile sort in one
    pass, "huge" (4112x4112 = 66 049 tiles, 17 key bits) in three passes whose ping-pong buffers hold garbage behind the device-side count."""
    from ex4dgs_amd import _C
    ins, st = h.scene_inputs(_huge() if cfg == "huge" else cfg, P=P, dir_scale=dir_scale)
    ins = {k: v.cuda() for k, v in ins.items()}
    s, sync = _raw_forward(ins, st)
    R = sync[0]
    assert isinstance(R, int) and R > 0
    for cap, no_flow in ((R, False), (R + 12345, dir_scale == 0.0), (4 * R, False)):
        s2, asy = _raw_forward(ins, st, instance_capacity=cap, assume_no_flow=no_flow)
        fr = asy[0]
        assert isinstance(fr, _C.PendingFrame) and fr.capacity == cap
        assert int(fr) == R and not fr.overflowed and fr.valid and fr.has_flow == (dir_scale != 0.0)
        for name, a, b in zip(("color", "radii", "depth", "acc", "flow", "idx"), (sync[1], sync[2], sync[6], sync[7], sync[8], sync[9]),
                              (asy[1], asy[2], asy[6], asy[7], asy[8], asy[9])):
            assert torch.equal(a, b), name
        H, W = st["image_height"], st["image_width"]
        va, vb = _C.binning_views(sync[4], R, W, H), _C.binning_views(asy[4], fr, W, H)
        assert torch.equal(va["point_list"][:R], vb["point_list"][:R])
        assert torch.equal(_C.img_views(sync[5], W, H)["ranges"], _C.img_views(asy[5], W, H)["ranges"])
        grads = [x.cuda() for x in h.upstream_grads(sync[7].cpu(), H, W, seed=4)]
        ga = _raw_backward(ins, s, sync, grads)
        gb = _raw_backward(ins, s2, asy, grads)
        for name, a, b in zip(h.GRAD_NAMES, (ga[0], ga[1], ga[2], ga[8], ga[3], ga[4], ga[5], ga[6], ga[7]), (gb[0], gb[1], gb[2], gb[8], gb[3], gb[4], gb[5], gb[6], gb[7])):
            if a.numel():
                tol = 2e-5 * float(a.abs().max()) + 1e-12
                assert float((a - b).abs().max()) <= tol, (name, cap)


def test_overflow_is_reported_and_the_autograd_surface_recovers(hip_lib):
    """An instance count above the capacity: nothing is written out of bounds, the status says so (num_rendered > capacity), the
    policy object of the autograd surface raises at the next forward (strict) or counts and regrows (non-strict), and the frame
    rendered again with the regrown capacity equals the synchronous frame."""
    from ex4dgs_amd import _C
    from ex4dgs_amd.diff_gaussian_rasterization_df import async_frames, rasterize_gaussians
    ins, st = h.scene_inputs("cfg2", P=20000, dir_scale=0.0)
    ins = {k: v.cuda() for k, v in ins.items()}
    s, sync = _raw_forward(ins, st)
    R = sync[0]
    guard = torch.full((1 << 20,), 7, dtype=torch.uint8, device="cuda")          # neighbours in the caching allocator stay untouched
    s2, asy = _raw_forward(ins, st, instance_capacity=R // 3)
    fr = asy[0]
    assert fr.num_rendered == R and fr.overflowed and not fr.valid
    assert bool((guard == 7).all()) and bool(torch.isfinite(asy[1]).all())
    grads = [x.cuda() for x in h.upstream_grads(sync[7].cpu(), st["image_height"], st["image_width"], seed=4)]
    gb = _raw_backward(ins, s2, asy, grads)                                     # truncated lists: finite garbage, no fault
    assert all(bool(torch.isfinite(g).all()) for g in gb if g.numel())
    e = torch.Tensor([])
    call = lambda: rasterize_gaussians(ins["means3D"], torch.zeros_like(ins["means3D"]), ins["dir3D"], ins["shs"], e, ins["opacities"],
                                       ins["scales"], ins["rotations"], e, s)
    try:
        async_frames.enable(headroom=1.25, capacity=R // 3, strict=True)
        out1 = call()                                                           # runs truncated ...
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match="exceed the capacity"):
            call()                                                              # ... and is reported here
        assert async_frames.capacity >= int(1.25 * R)
        async_frames.enable(headroom=1.25, capacity=R // 3, strict=False)
        call(); torch.cuda.synchronize()
        out2 = call()                                                           # regrown: this one is whole
        async_frames.drain()
        assert async_frames.invalid_frames == 1 and async_frames.no_flow
        assert torch.equal(out2[0], sync[1]) and torch.equal(out2[5], sync[9])
        out3 = call()                                                           # now with the flow-free kernel (learned from the status)
        async_frames.drain()
        assert torch.equal(out3[0], sync[1]) and async_frames.invalid_frames == 1
    finally:
        async_frames.enabled = False
        async_frames.pending = []


def test_wrong_no_flow_assertion_is_reported(hip_lib):
    ins, st = h.scene_inputs("cfg1", dir_scale=0.1)
    ins = {k: v.cuda() for k, v in ins.items()}
    s, sync = _raw_forward(ins, st)
    s2, asy = _raw_forward(ins, st, instance_capacity=sync[0] + 10, assume_no_flow=True)
    assert asy[0].has_flow and not asy[0].valid and not asy[0].overflowed
    assert torch.equal(asy[1], sync[1]) and float(asy[8].abs().max()) == 0.0     # colour is right, the flow image was not composited


def test_forward_and_backward_replay_from_a_hip_graph(hip_lib):
    """The asynchronous call sequence has host-constant grids and no host wait: forward + backward are captured into ONE graph
    (torch.cuda.graph = hipStreamBeginCapture underneath), replayed on new input values, and match the eager calls."""
    from ex4dgs_amd import _C
    ins, st = h.scene_inputs("cfg2", P=20000, dir_scale=0.0)
    ins = {k: v.cuda() for k, v in ins.items()}
    s, sync = _raw_forward(ins, st)
    R = sync[0]
    H, W = st["image_height"], st["image_width"]
    grads = [x.cuda() for x in h.upstream_grads(sync[7].cpu(), H, W, seed=4)]
    cap = int(1.5 * R)
    static = {k: v.clone() for k, v in ins.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up on the capture stream (allocator, lazy module loading)
        _, f = _raw_forward(static, st, settings=s, instance_capacity=cap, assume_no_flow=True)
        _raw_backward(static, s, f, grads)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s3, fwd = _raw_forward(static, st, settings=s, instance_capacity=cap, assume_no_flow=True)
        bwd = _raw_backward(static, s3, fwd, grads)
    for shift in (0.0, 0.05):
        moved = ins["means3D"] + shift * torch.tensor([1.0, 0.0, 0.0], device="cuda")
        static["means3D"].copy_(moved)
        g.replay()
        torch.cuda.synchronize()
        eager_in = dict(ins, means3D=moved)
        s4, ref = _raw_forward(eager_in, st)
        assert fwd[0].wait().num_rendered == ref[0] and fwd[0].valid
        assert torch.equal(fwd[1], ref[1]) and torch.equal(fwd[9], ref[9]) and torch.equal(fwd[2], ref[2])
        gref = _raw_backward(eager_in, s4, ref, grads)
        for a, b in zip(bwd, gref):
            if a.numel():
                assert float((a - b).abs().max()) <= 2e-5 * float(b.abs().max()) + 1e-12


def test_compiled_host_path_asynchronous_mode_is_exact_and_replays_overflowing_frames(hip_lib):
    """include/ex4d_trainer.h with ex4d_trainer_set_async: no instance-count read-back inside the frame, the status is checked once
    before the optimizer step.  Two copies of one model, synchronous vs asynchronous, over views whose instance counts differ by much
    more than the 25 % headroom (a wide and a narrow field of view): the asynchronous trainer must re-run the frames that overflow
    (replays > 0) and end with the same parameters (to the order of the rasterizer's float atomics)."""
    from ex4dgs_amd.native_trainer import NativeTrainer
    from ex4dgs_amd.scene import make_scene
    ma, cam, bg = make_scene("cfg3", P=8000, device="cuda", fused=True)
    mb, _, _ = make_scene("cfg3", P=8000, device="cuda", fused=True)
    cam = cam.to("cuda"); bg = bg.cuda()
    gt = torch.rand(3, cam.image_height, cam.image_width, generator=torch.Generator().manual_seed(11)).cuda()
    lrs = {n: 1e-4 for n in ma.PARAM_NAMES}
    p0 = {n: getattr(ma, n).clone() for n in ma.PARAM_NAMES}
    na = NativeTrainer(ma, cam, optimizer=True, lrs=lrs)
    nb = NativeTrainer(mb, cam, optimizer=True, lrs=lrs)
    nb.set_async(True)
    counts_a, counts_b = [], []
    for t in (0, 137, 41, 299, 7, 138, 40, 139, 200, 201):
        na.step(cam, bg, t, gt); counts_a.append(na.num_rendered)
        nb.step(cam, bg, t, gt); counts_b.append(nb.num_rendered)
    torch.cuda.synchronize()
    assert counts_a == counts_b and min(counts_a) > 0
    for n in ma.PARAM_NAMES:
        a, b = getattr(ma, n), getattr(mb, n)
        moved = float((a - p0[n]).abs().max())
        ulp = 2.0 ** -23 * float(a.abs().max())
        assert moved > 0 and float((a - b).abs().max()) <= 1e-3 * moved + 2 * ulp, (n, float((a - b).abs().max()), moved)
    assert float(na.output("loss")) == pytest.approx(float(nb.output("loss")), abs=1e-6)
    na.close(); nb.close()
    # forced overflow: a trainer whose capacity was seeded by a frame with few instances (tiny Gaussians), then the real scene
    mc, _, _ = make_scene("cfg3", P=8000, device="cuda", fused=True)
    md, _, _ = make_scene("cfg3", P=8000, device="cuda", fused=True)
    nc = NativeTrainer(mc, cam, optimizer=True, lrs=lrs)
    nd = NativeTrainer(md, cam, optimizer=True, lrs=lrs)
    nd.set_async(True)
    with torch.no_grad():
        for m in (mc, md):                                # exp(-3): footprints 20x smaller -> far fewer tile instances
            m._scaling -= 3.0; m._scaling_motion -= 3.0
    nc.step(cam, bg, 0, gt); nd.step(cam, bg, 0, gt)      # (synchronous seed frame of nd)
    small = nd.num_rendered
    with torch.no_grad():
        for m in (mc, md):
            m._scaling += 3.0; m._scaling_motion += 3.0
    for t in (5, 137, 250):
        nc.step(cam, bg, t, gt); nd.step(cam, bg, t, gt)
        assert nc.num_rendered == nd.num_rendered
    torch.cuda.synchronize()
    assert nd.num_rendered > 1.5 * small and nd.replays() >= 1, (small, nd.num_rendered, nd.replays())
    for n in mc.PARAM_NAMES:
        a, b = getattr(mc, n), getattr(md, n)
        assert float((a - b).abs().max()) <= 1e-3 * float((a - p0[n]).abs().max()) + 4 * 2.0 ** -23 * float(a.abs().max()) + 1e-12, n
    nc.close(); nd.close()


def test_frame_trainer_asynchronous_forward_replays_and_matches_the_synchronous_trainer(hip_lib):
    """trainer.FrameTrainer(async_forward=True): the Python owner of the iteration checks the frame's status before its gradients are
    applied and re-runs an overflowing frame.  Against the synchronous trainer on a copy of the model: a run over several timestamps,
    then a 20x jump of the instance count (the capacity was seeded by tiny footprints) -- replays >= 1, same parameters."""
    from ex4dgs_amd.diff_gaussian_rasterization_df import async_frames
    from ex4dgs_amd.loss import l1_ssim_loss
    from ex4dgs_amd.scene import make_scene
    from ex4dgs_amd.trainer import FrameTrainer
    assert not async_frames.enabled
    ma, cam, bg = make_scene("cfg3", P=8000, device="cuda", fused=True)
    mb, _, _ = make_scene("cfg3", P=8000, device="cuda", fused=True)
    cam = cam.to("cuda"); bg = bg.cuda()
    gt = torch.rand(3, cam.image_height, cam.image_width, generator=torch.Generator().manual_seed(11)).cuda()
    lrs = {n: 1e-4 for n in ma.PARAM_NAMES}
    p0 = {n: getattr(ma, n).clone() for n in ma.PARAM_NAMES}
    up = lambda out: ([l1_ssim_loss(out["render"], gt, 0.2)[0]], [None])
    try:
        fa = FrameTrainer(ma, optimizer=True, lrs=lrs, async_forward=False)
        fb = FrameTrainer(mb, optimizer=True, lrs=lrs, async_forward=True)
        assert fb.async_forward and not fa.async_forward and not FrameTrainer(ma, optimizer=False).async_forward      # (round 6: opt-in, the default is synchronous)
        with torch.no_grad():
            for m in (ma, mb):
                m._scaling -= 3.0; m._scaling_motion -= 3.0
        fa.step(cam, bg, 0, up); fb.step(cam, bg, 0, up)          # tiny footprints: seeds a small capacity
        fa.flush(); fb.flush()
        with torch.no_grad():
            for m in (ma, mb):
                m._scaling += 3.0; m._scaling_motion += 3.0
        for t in (5, 137, 41, 299, 7, 138):
            fa.step(cam, bg, t, up); fb.step(cam, bg, t, up)
        fa.flush(); fb.flush(); torch.cuda.synchronize()
        assert fb.replays >= 1 and fb._policy.invalid_frames >= 1 and not async_frames.enabled      # (the process-wide policy stayed off)
        for n in ma.PARAM_NAMES:
            a, b = getattr(ma, n), getattr(mb, n)
            moved = float((a - p0[n]).abs().max())
            assert moved > 0 and float((a - b).abs().max()) <= 1e-3 * moved + 4 * 2.0 ** -23 * float(a.abs().max()) + 1e-12, (n, float((a - b).abs().max()), moved)
        with pytest.raises(ValueError, match="single rank"):
            FrameTrainer(mb, exchange="sharded", async_forward=True)
    finally:
        async_frames.enabled = False
        async_frames.pending = []


@pytest.mark.parametrize("mode", ["--async-frames", "--graph"])
def test_bench_asynchronous_and_graph_modes_print_a_valid_line(hip_lib, mode):
    """`bench.py --async-frames` / `--graph` (the asynchronous forward through the autograd surface / forward + backward replayed from one
    hipGraph) run, refuse nothing, and print ONE JSON line that says which mode was timed."""
    import json, os, subprocess, sys
    cmd = [sys.executable, os.path.join(h.ROOT, "bench.py"), "--config", "cfg2", "--points", "20000", "--steps", "6", "--warmup", "3",
           "--no-cpu-baseline", "--no-model-step", mode]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["value"] > 0 and d["n_gpus"] == 1
    assert ("hipGraph" in d["config"]["step"]) if mode == "--graph" else ("asynchronous forward" in d["config"]["step"])


def test_bench_plain_line_and_dumped_outputs(hip_lib, tmp_path):
    """A plain `bench.py` run (no --full) prints the headline fields and nothing that needs runs of its own; `--dump-outputs` writes
    what its last timed step computed as float32 / float64 arrays of at most 64 MB, and two runs with the same arguments agree: the
    forward outputs bit for bit, the gradients to the order of the float atomics."""
    import json, os, subprocess, sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    dumps = []
    for run in ("a", "b"):
        out = tmp_path / run
        cmd = [sys.executable, os.path.join(h.ROOT, "bench.py"), "--gpus", "1", "--config", "cfg2", "--points", "20000", "--steps", "3",
               "--warmup", "2", "--dump-outputs", str(out)]
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert d["ms_per_step"] > 0 and d["value"] == d["ms_per_step"] and d["steps"] == 3 and d["unit"] == "ms/frame"
        assert d["higher_is_better"] is False and d["dtype"] == "f32" and "GaussianRasterizer forward + backward" in d["config"]["step"]
        assert not {"step_ms", "roofline", "model_step", "cpu_baseline"} & set(d), sorted(d)
        arrays = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
        assert {"color", "depth", "acc", "radii", "grad_means3D", "grad_shs", "grad_opacities"} <= set(arrays), sorted(arrays)
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 * 10 ** 6
        dumps.append(arrays)
    a, b = dumps
    assert a.keys() == b.keys()
    for k in a:
        if k.startswith("grad_"):
            assert np.abs(a[k] - b[k]).max() <= 1e-3 * max(np.abs(a[k]).max(), 1e-30), k
        else:
            assert np.array_equal(a[k], b[k]), k


def test_asynchronous_frames_soak_over_changing_views(hip_lib):
    """120 frames through the autograd surface under the asynchronous policy (strict: a truncated frame would raise), the timestamp and the
    camera distance changing from frame to frame so that the instance count moves by tens of percent, every frame's image and gradients
    compared with the synchronous call on the same inputs: images bit-equal, gradients to the order of the float atomics.  Frames that
    outgrow the capacity are allowed at most while it is being learned (the policy then re-seeds synchronously at no loss of frames)."""
    from ex4dgs_amd.diff_gaussian_rasterization_df import AsyncFrames, use_policy, rasterize_gaussians, async_frames
    from ex4dgs_amd.scene import make_scene, focal_camera, CONFIGS
    from ex4dgs_amd.render import render
    model, cam, bg = make_scene("cfg3", P=6000, device="cuda", fused=True)
    cam = cam.to("cuda"); bg = bg.cuda()
    cfg = CONFIGS["cfg3"]
    params = model.parameters()
    for p in params:
        p.requires_grad_(True)
    H, W = cam.image_height, cam.image_width
    w = torch.rand(3, H, W, generator=torch.Generator().manual_seed(3)).cuda()
    pol = AsyncFrames().enable(headroom=1.3, strict=False)
    rng = np.random.default_rng(5)
    counts = []
    for i in range(120):
        t = int(rng.integers(0, 300))
        # move the camera back and forth along its axis: the footprints (and with them the instance count) shrink and grow
        cam = focal_camera(cfg.width, cfg.height, cfg.focal, T=[0.0, 0.0, float(rng.uniform(-1.5, 3.0))], znear=0.01, zfar=100.0,
                           cxr=cfg.cxr, cyr=cfg.cyr).to("cuda")
        for p in params:
            p.grad = None
        with use_policy(pol):
            out = render(cam, model, None, bg, timestamp=t, near=4.0, far=300.0)
        (out["render"] * w).sum().backward()
        ga = [p.grad.clone() for p in params]
        img = out["render"].detach().clone()
        for p in params:
            p.grad = None
        ref = render(cam, model, None, bg, timestamp=t, near=4.0, far=300.0)      # process-wide policy: off -> synchronous
        (ref["render"] * w).sum().backward()
        pol.drain()
        invalid_now = pol.invalid_frames
        counts.append(pol.capacity)
        if invalid_now == getattr(test_asynchronous_frames_soak_over_changing_views, "_seen", 0):
            assert torch.equal(img, ref["render"]), i
            for name, a, p in zip(model.PARAM_NAMES, ga, params):
                assert float((a - p.grad).abs().max()) <= 2e-5 * float(p.grad.abs().max()) + 1e-12, (i, name)
        test_asynchronous_frames_soak_over_changing_views._seen = invalid_now
    assert not async_frames.enabled and pol.frames == 120
    assert pol.invalid_frames <= 6, pol.invalid_frames            # only while the capacity is being learned
    assert counts[-1] >= counts[0]


@pytest.mark.gpu
def test_forced_128_register_build_of_the_per_gaussian_backward_is_correct(hip_lib, tmp_path):
    """VERDICT r03 weak #8.  A build of preprocess_bwd_kernel forced to 128 registers (__launch_bounds__(256, 4): three spills in the
    <false> instantiation) used to return a wrong dL_dmeans3D for ~600 Gaussians per 100 k.  Cause (DESIGN.md section 4 "Round 4",
    tools/dev/micro/topreg_probe.hip): the register allocator had put the per-lane shift amount of a 64-bit shift into the wave's last
    register, where gfx950 replaces it by VGPR0 in waves that share their SIMD -- not the spills.  The sources no longer hold a 64-bit
    shift by a per-lane amount there (mask_bit), so the same forced build -- same register count, same spills -- must agree with the
    default build: both run the same frame in a process of their own, compared on the deterministic per-Gaussian stage's output."""
    import importlib.util, os, subprocess, sys
    from ex4dgs_amd import build
    spec = importlib.util.spec_from_file_location("spill_probe", os.path.join(h.ROOT, "tools", "dev", "spill_probe.py"))
    sp = importlib.util.module_from_spec(spec); spec.loader.exec_module(sp)
    info = {}
    lib = sp.build_variant(str(tmp_path / "forced128"), lambda s: s.replace(*sp.BOUNDS), info)
    regs = {k: v for k, v in info.items() if k != "obj"}
    assert regs and all(v[0] == 128 for v in regs.values()), regs                    # the forced build is what was built ...
    assert any(v[1] > 0 for v in regs.values()), regs                                # ... and it still spills
    assert build.shift_amount_in_last_vgpr(info["obj"]) == []
    outs = {}
    for name, env in (("default", None), ("forced128", lib)):
        out = str(tmp_path / (name + ".npz"))
        e = dict(os.environ, EX4D_SPILL_PROBE_SIZES="100000")
        e.pop("EX4D_HIP_LIB", None)
        if env: e["EX4D_HIP_LIB"] = env
        r = subprocess.run([sys.executable, sp.__file__, "run", out], env=e, stderr=subprocess.PIPE, text=True, cwd=h.ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[name] = np.load(out)
    P = 100000
    radii = outs["default"][f"{P}/radii"]
    assert int((radii > 0).sum()) > 50000
    for k in ("dL_dmeans3D", "dL_dsh", "dL_dscales", "dL_drotations", "dL_dmeans2D", "dL_dopacity"):
        x, y = outs["default"][f"{P}/0/{k}"].reshape(P, -1), outs["forced128"][f"{P}/0/{k}"].reshape(P, -1)
        rel = np.abs(x - y).max(1) / np.maximum(np.abs(x).max(1), 1e-30)
        rerun = np.abs(x - outs["default"][f"{P}/1/{k}"].reshape(P, -1)).max(1) / np.maximum(np.abs(x).max(1), 1e-30)
        bad = ((rel > 1e-3) & (radii > 0)).sum()
        noise = ((rerun > 1e-3) & (radii > 0)).sum()          # float atomics in the compositing backward: the same build twice
        assert bad <= noise + 2, (k, int(bad), int(noise))
