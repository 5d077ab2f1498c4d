"""Scoring rendered views on the GPU (include/ex4d_loss.h: ex4d_frame_metrics / _u8; ex4dgs_amd/evaluate.py) against the float64
reference of tests/metrics_ref.py, at its bars: rows 0, 1, 3 within 1e-6 absolute, the PSNR within the MSE bar carried through the
logarithm plus a few ulps, the non-finite count and every byte equal.  Every shape is from metrics_ref.SHAPES; no case and no pixel
is left out."""
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import metrics_ref as mr

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096
FILL = 0xA5
LUTS = {"u8": None, "u8_1.7": 1.7}


def _lut(kind):
    from ex4dgs_amd.frames import gt_lut
    return None if LUTS[kind] is None else gt_lut(LUTS[kind])


def _table(kind):
    from ex4dgs_amd.frames import gt_lut
    return gt_lut() if LUTS[kind] is None else gt_lut(LUTS[kind])


def _row(*a, **kw):
    from ex4dgs_amd.evaluate import frame_metrics
    return frame_metrics(*a, **kw).cpu().tolist()


def _same_row(a, b):
    """Equality of bits, NaN included."""
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


# ------------------------------------------------------------------------------------------------ 1. rows against the reference
@pytest.mark.parametrize("H, W", mr.SHAPES)
def test_rows_against_the_float64_reference(hip_lib, H, W):
    image, gt = mr.make_pair(H, W)
    x = torch.from_numpy(image).to(DEV)
    for clamp in (False, True):
        mr.within_bars(_row(x, torch.from_numpy(gt).to(DEV), clamp=clamp), mr.case(H, W, "float", clamp), (H, W, "float", clamp))
        for stride in (3, 4):
            gt8 = torch.from_numpy(mr.make_bytes(H, W, stride)).to(DEV)
            for kind in LUTS:
                mr.within_bars(_row(x, gt8, lut=_lut(kind), clamp=clamp), mr.case(H, W, kind, clamp), (H, W, kind, stride, clamp))


# ------------------------------------------------------------------------------------------------ 2. bytes = looked-up floats
@pytest.mark.parametrize("H, W", mr.SHAPES)
def test_the_u8_row_is_the_float_row_on_the_looked_up_image_bit_for_bit(hip_lib, H, W):
    image, _ = mr.make_pair(H, W)
    x = torch.from_numpy(image).to(DEV)
    for stride in (3, 4):
        u8 = mr.make_bytes(H, W, stride)
        block = torch.randint(0, 256, (3, H, W, stride), generator=torch.Generator().manual_seed(6), dtype=torch.uint8)
        block[1] = torch.from_numpy(u8)
        block = block.to(DEV)                                          # frame 1 of 3: an odd base address for odd H W at stride 3
        for kind in LUTS:
            gtf = torch.from_numpy(mr.looked_up(u8, _table(kind))).to(DEV)
            for clamp in (False, True):
                o_f = torch.zeros(H, W, 3, dtype=torch.uint8, device=DEV)
                o_b = torch.ones(H, W, 3, dtype=torch.uint8, device=DEV)
                want = _row(x, gtf, clamp=clamp, out_u8=o_f)
                got = _row(x, block[1], lut=_lut(kind), clamp=clamp, out_u8=o_b)
                assert np.isfinite(want).all() and _same_row(got, want), (stride, kind, clamp, got, want)
                assert torch.equal(o_f, o_b)


# ------------------------------------------------------------------------------------------------ 3. bytes in both quantisations
def _planted(H, W):
    """make_pair's image with every rounding threshold (k + 0.5) / 255 and k / 255, their +-1 ulp neighbours, values below 0 and above 1
    and -0.0 planted at seeded positions."""
    image, gt = mr.make_pair(H, W)
    k = torch.arange(256, dtype=torch.float32)
    t = torch.cat([(k[:255] + 0.5) / 255.0, k / 255.0])
    up, down = torch.nextafter(t, torch.tensor(2.0)), torch.nextafter(t, torch.tensor(-1.0))
    extra = torch.tensor([-0.0, -1e-30, -0.001, -0.5, -7.0, 1.0 + 2.0 ** -23, 1.002, 1.5, 300.0, 0.5 / 255.0 - 1e-9], dtype=torch.float32)
    vals = torch.cat([t, up, down, extra]).numpy()
    flat = image.reshape(-1)
    assert vals.size < flat.size
    pos = np.random.default_rng(5).permutation(flat.size)[:vals.size]
    flat[pos] = vals
    return image, gt


@pytest.mark.parametrize("quant", ["round", "trunc"])
def test_bytes_are_the_torch_ops_bit_for_bit_at_an_odd_address_between_guards(hip_lib, quant):
    H, W = 53, 139
    image, gt = _planted(H, W)
    assert np.signbit(image).any() and (image == 0).any()
    x, y = torch.from_numpy(image).to(DEV), torch.from_numpy(gt).to(DEV)
    gt8 = torch.from_numpy(mr.make_bytes(H, W)).to(DEV)
    n = H * W * 3
    ref_q = mr.quant_round if quant == "round" else mr.quant_trunc
    for clamp in (False, True):
        want = ref_q(mr.clamp01(image) if clamp else image)
        for gt_dev in (y, gt8):
            whole = torch.full((GUARD + 1 + n + GUARD,), FILL, dtype=torch.uint8, device=DEV)
            out = whole[GUARD + 1:GUARD + 1 + n]
            assert out.data_ptr() % 2 == 1
            row = _row(x, gt_dev, clamp=clamp, quant=quant, out_u8=out)
            got = out.cpu().numpy().reshape(H, W, 3)
            bad = np.argwhere(got != want)
            assert bad.size == 0, (quant, clamp, len(bad), bad[:5], [(int(got[tuple(b)]), int(want[tuple(b)]), float(image[b[2], b[0], b[1]])) for b in bad[:5]])
            assert bool((whole[:GUARD + 1] == FILL).all()) and bool((whole[GUARD + 1 + n:] == FILL).all())
            assert _same_row(_row(x, gt_dev, clamp=clamp, quant=quant), row)          # out_u8 = NULL: the same row
            if gt_dev is y:
                mr.within_bars(row, mr.metrics(image, gt, clamp), (quant, clamp))


# ------------------------------------------------------------------------------------------------ 4. non-finite pixels
@pytest.mark.parametrize("quant", ["round", "trunc"])
def test_non_finite_pixels_are_counted_and_get_their_bytes(hip_lib, quant):
    H, W = 53, 139
    image, gt = mr.make_pair(H, W)
    x, y = torch.from_numpy(image).to(DEV), torch.from_numpy(gt).to(DEV)
    clean = torch.zeros(H, W, 3, dtype=torch.uint8, device=DEV)
    assert _row(x, y, quant=quant, out_u8=clean)[4] == 0
    spots = {(0, 2, 3): float("nan"), (1, 50, 130): float("inf"), (2, 47, 64): float("-inf")}      # (channel, row, column): three work items
    for (c, r, q), v in spots.items():
        x[c, r, q] = v
    for clamp, count in ((False, 3), (True, 1)):                        # clamped, +-inf are 1 and 0: finite values of the scored image
        out = torch.full((H, W, 3), 7, dtype=torch.uint8, device=DEV)
        row = _row(x, y, clamp=clamp, quant=quant, out_u8=out)
        assert row[4] == count and all(np.isnan(row[:4])) and row[5:] == [0.0, 0.0, 0.0], row
        want = torch.from_numpy((mr.quant_round if quant == "round" else mr.quant_trunc)(mr.clamp01(image) if clamp else image)).to(DEV)
        assert torch.equal(want, clean) or clamp
        for (c, r, q), b in zip(spots, (0, 255, 0)):
            assert int(out[r, q, c]) == b, (c, r, q, int(out[r, q, c]))
            want[r, q, c] = b
        assert torch.equal(out, want)


# ------------------------------------------------------------------------------------------------ 5. consistency with the training path
@pytest.mark.parametrize("H, W", mr.SHAPES)
def test_ssim_and_l1_agree_with_the_training_loss(hip_lib, H, W):
    from ex4dgs_amd.loss import l1_ssim_loss
    image, gt = mr.make_pair(H, W)
    x, y = torch.from_numpy(image).to(DEV), torch.from_numpy(gt).to(DEV)
    row = _row(x, y)
    ssim = 1.0 - float(l1_ssim_loss(x, y, 1.0)[0])
    l1 = float(l1_ssim_loss(x, y, 0.0)[0])
    print((H, W), abs(row[3] - ssim), abs(row[0] - l1))
    assert abs(row[3] - ssim) <= 2 * 2.0 ** -23
    assert abs(row[0] - l1) <= 2.0 ** -23 * max(1.0, l1)


# ------------------------------------------------------------------------------------------------ 6. the table
def test_five_views_into_one_table_with_one_read_back(hip_lib):
    from ex4dgs_amd.evaluate import Evaluator
    H, W = 49, 65
    ev = Evaluator(6, H, W, keep_frames=True)
    pattern = 0x7FF8DEAD0000BEEF
    ev.table.view(torch.int64).fill_(pattern)
    g = torch.Generator().manual_seed(8)
    views = [(torch.rand(3, H, W, generator=g).to(DEV) * 1.4 - 0.2, torch.rand(3, H, W, generator=g).to(DEV)) for _ in range(5)]
    gt8 = torch.from_numpy(mr.make_bytes(H, W)).to(DEV)
    order = (1, 3, 0, 4, 2)
    for k, i in enumerate(order):
        ev.score(i, views[k][0], gt8 if k == 2 else views[k][1], name=f"v{i}", clamp=bool(k % 2))
    rows = ev.rows()
    assert tuple(rows.shape) == (6, 8) and rows.dtype == torch.float64 and rows.device.type == "cpu"
    for k, i in enumerate(order):
        single = torch.zeros(H, W, 3, dtype=torch.uint8, device=DEV)
        want = _row(views[k][0], gt8 if k == 2 else views[k][1], clamp=bool(k % 2), out_u8=single)
        assert np.isfinite(want).all() and _same_row(rows[i].tolist(), want), (k, i)
        assert torch.equal(ev.frame(i), single)
    assert (rows[5].view(torch.int64) == pattern).all() and ev.names == ["v0", "v1", "v2", "v3", "v4", None]
    mean, per_view = ev.report()
    assert list(per_view["PSNR"]) == ["v0", "v1", "v2", "v3", "v4"] and set(mean) == {"SSIM", "PSNR", "L1"}
    with pytest.raises(RuntimeError, match="view 6"):
        ev.score(6, *views[0])


# ------------------------------------------------------------------------------------------------ 7. graph capture
def test_two_scores_replay_from_one_graph(hip_lib):
    from ex4dgs_amd.evaluate import Evaluator
    from ex4dgs_amd.frames import gt_lut
    H, W = 49, 65
    g = torch.Generator().manual_seed(12)
    contents = [(torch.rand(3, H, W, generator=g) * 1.4 - 0.2, torch.rand(3, H, W, generator=g),
                 torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)) for _ in range(2)]
    x, y, y8 = (t.clone().to(DEV) for t in contents[0])
    ev = Evaluator(2, H, W, keep_frames=True)

    def both():
        lut = gt_lut(1.7)                      # read during the call: the graph holds the table by value
        ev.score(0, x, y, name="a", clamp=True)
        ev.score(1, x, y8, name="b", lut=lut)

    def eager(content):
        xe, ye, y8e = (t.to(DEV) for t in content)
        f0, f1 = (torch.zeros(H, W, 3, dtype=torch.uint8, device=DEV) for _ in range(2))
        return [_row(xe, ye, clamp=True, out_u8=f0), _row(xe, y8e, lut=gt_lut(1.7), out_u8=f1)], [f0, f1]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):              # one eager call first
        both()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    for content in (contents[0], contents[1]):
        for dst, src in zip((x, y, y8), content):
            dst.copy_(src.to(DEV))             # new content in place
        ev.table.fill_(float("nan"))
        ev.frames.fill_(FILL)
        graph.replay()
        torch.cuda.synchronize()
        rows, frames = eager(content)
        got = ev.rows()
        for i in range(2):
            assert np.isfinite(rows[i]).all() and _same_row(got[i].tolist(), rows[i]), i
            assert torch.equal(ev.frame(i), frames[i]), i


# ------------------------------------------------------------------------------------------------ 8. evaluate_set end to end
def _tiny_set():
    from tests import helpers
    from ex4dgs_amd.frames import FrameStore
    cfg = helpers.SceneConfig("metrics: 3000 static + dynamic, 64x48", 3000, 64, 48, 40.0, dyn_frac=0.25, seed=23)
    model, cam, bg = helpers.make_scene(cfg, device=DEV, fused=True)
    with torch.no_grad():                      # colours that overshoot 1 (SH clamps at 0 only), so that clamp=True decides something
        model._features_dc.mul_(2.0)
        model._features_dc_motion.mul_(2.0)
    cam = cam.to(DEV)
    cameras = [types.SimpleNamespace(**cam._replace(timestamp=float(t))._asdict(), image_name=f"cam00_{t:04d}.png") for t in (0, 137, 41)]
    g = torch.Generator().manual_seed(24)
    host = [torch.randint(0, 256, (48, 64, 3), generator=g, dtype=torch.uint8) for _ in cameras]
    store = FrameStore(3, 48, 64, device=DEV)
    for i, f in enumerate(host):
        store.put(i, f)
    return cfg, model, cameras, bg.to(DEV), store, host


def test_evaluate_set_end_to_end(hip_lib, tmp_path):
    from PIL import Image
    from ex4dgs_amd import loss
    from ex4dgs_amd.evaluate import evaluate_set
    from ex4dgs_amd.frames import gt_lut
    from ex4dgs_amd.render import render
    cfg, model, cameras, bg, store, host = _tiny_set()
    lut = gt_lut(1.7)
    kw = dict(lut=lut, background=bg, near=cfg.min_depth, far=cfg.max_depth)
    mean, per_view, ev = evaluate_set(model, cameras, store, out_dir=str(tmp_path), save_img=True, **kw)
    mean_c, per_view_c, _ = evaluate_set(model, cameras, [store.get(i) for i in range(3)], clamp=True, **kw)     # a list of tensors
    names = [c.image_name for c in cameras]
    on_disk = json.load(open(tmp_path / "mean_metrics.json")), json.load(open(tmp_path / "all_metrics.json"))
    assert on_disk == (mean, per_view)
    assert set(mean) == set(per_view) == {"SSIM", "PSNR", "L1"} and all(list(per_view[k]) == names for k in per_view)
    composed = {k: [] for k in ("SSIM", "PSNR", "L1")}
    exceeds, bars = 0, []
    with torch.no_grad():
        for i, cam in enumerate(cameras):
            image = render(cam, model, None, bg, near=cfg.min_depth, far=cfg.max_depth)["render"]
            gt = lut.to(DEV)[store.get(i).long()].permute(2, 0, 1).contiguous()
            assert float(image.std()) > 0.01
            exceeds += int(((image < 0) | (image > 1)).sum())
            # render.py:76-77 on the render as it is, at the bars, against the float64 reference and against the composition
            ref = mr.metrics(image.cpu().numpy(), gt.cpu().numpy())
            name = names[i]
            mr.within_bars([per_view["L1"][name], ref["mse"], per_view["PSNR"][name], per_view["SSIM"][name], 0, 0.0, 0.0, 0.0], ref, ("evaluate_set", name))
            comp = dict(PSNR=float(loss.psnr(image.unsqueeze(0), gt.unsqueeze(0))), SSIM=float(loss.ssim(image.unsqueeze(0), gt.unsqueeze(0))),
                        L1=float(loss.l1_loss(image, gt)))
            for k in composed:
                composed[k].append(torch.tensor(comp[k], dtype=torch.float32))
            assert abs(per_view["L1"][name] - comp["L1"]) <= mr.TOL and abs(per_view["SSIM"][name] - comp["SSIM"]) <= mr.TOL
            bars.append(mr.psnr_bar(ref["mse"], ref["psnr"]))
            assert abs(per_view["PSNR"][name] - comp["PSNR"]) <= bars[-1]
            # train.py:342-348
            clamped = torch.clamp(image, 0.0, 1.0)
            ref_c = mr.metrics(image.cpu().numpy(), gt.cpu().numpy(), clamp=True)
            l1_c = loss.l1_loss(clamped, gt).mean().double().item()
            psnr_c = loss.psnr(clamped.unsqueeze(0), gt.unsqueeze(0)).mean().double().item()
            assert abs(per_view_c["L1"][name] - l1_c) <= mr.TOL and abs(per_view_c["PSNR"][name] - psnr_c) <= mr.psnr_bar(ref_c["mse"], ref_c["psnr"])
            mr.within_bars([per_view_c["L1"][name], ref_c["mse"], per_view_c["PSNR"][name], per_view_c["SSIM"][name], 0, 0.0, 0.0, 0.0], ref_c, ("clamped", name))
            # the PNG is the stored 8-bit frame, which is save_image's conversion of the render
            png = np.array(Image.open(tmp_path / "renders" / name))
            assert png.shape == (48, 64, 3) and np.array_equal(png, ev.frame(i).cpu().numpy())
            assert np.array_equal(png, mr.quant_round(image.cpu().numpy()))
    print("render values outside [0, 1]:", exceeds)
    assert exceeds > 0, "the scene must leave [0, 1] somewhere, or clamp=True decides nothing here"
    for k in composed:                                                  # render.py:98-105: every term within its bar, plus the float32 mean's own rounding
        want = torch.tensor(composed[k]).mean().item()
        assert abs(mean[k] - want) <= (max(bars) if k == "PSNR" else mr.TOL) + 2 * 2.0 ** -23 * abs(want), (k, mean[k], want)
    assert sorted(os.listdir(tmp_path / "renders")) == sorted(names)


def test_evaluate_set_interval_and_refusals(hip_lib):
    from ex4dgs_amd.evaluate import evaluate_set, frame_metrics
    cfg, model, cameras, bg, store, _ = _tiny_set()
    kw = dict(background=bg, near=cfg.min_depth, far=cfg.max_depth)
    _, per_view, ev = evaluate_set(model, cameras, store, interval=2, **kw)
    assert list(per_view["SSIM"]) == [cameras[0].image_name, cameras[2].image_name] and ev.frames is None
    with pytest.raises(RuntimeError, match="keep_frames"):
        ev.frame(0)
    with pytest.raises(RuntimeError, match="out_dir"):
        evaluate_set(model, cameras, store, save_img=True, **kw)
    x = torch.zeros(3, 8, 8, device=DEV)
    for bad_gt, match in ((x[:, :7], "image's shape"), (x.double(), "float32 \\[3,H,W\\] or uint8"), (x.cpu(), "device"),
                          (torch.zeros(8, 8, 2, dtype=torch.uint8, device=DEV), "\\[H,W,3\\] or \\[H,W,4\\]")):
        with pytest.raises(RuntimeError, match=match):
            frame_metrics(x, bad_gt)
    with pytest.raises(RuntimeError, match="lut= belongs to uint8"):
        frame_metrics(x, x, lut=torch.zeros(256))
    with pytest.raises(RuntimeError, match="\\[3,H,W\\]"):
        frame_metrics(x[:2], x[:2])
    with pytest.raises(RuntimeError, match="out_u8"):
        frame_metrics(x, x, out_u8=torch.zeros(8, 8, 4, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="row must be"):
        frame_metrics(x, x, row=torch.zeros(8, device=DEV))
