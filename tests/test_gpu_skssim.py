"""scikit-image's SSIM of a rendered view on the GPU (include/ex4d_loss.h: ex4d_frame_skssim / _u8; ex4dgs_amd/evaluate.py) against the
float64 reference of tests/skssim_ref.py at loss_cases.TOL_LOSS (1e-6 absolute), on the shapes of tests/skssim_cases.py: every edge
of the output-domain tiling.  tests/test_cpu_skssim.py shows on the same inputs that float32 alone has fourfold room under that bar."""
import json

import numpy as np
import pytest
import torch

from tests import metrics_ref as mr
from tests import skssim_cases as sc
from tests import skssim_ref as sr

pytestmark = pytest.mark.gpu

DEV = "cuda"
LUTS = {"u8": None, "u8_1.7": 1.7}


def _lut(kind):
    from ex4dgs_amd.frames import gt_lut
    return None if LUTS[kind] is None else gt_lut(LUTS[kind])


def _table(kind):
    from ex4dgs_amd.frames import gt_lut
    return gt_lut() if LUTS[kind] is None else gt_lut(LUTS[kind])


def _row(*a, **kw):
    from ex4dgs_amd.evaluate import frame_skssim
    return frame_skssim(*a, **kw).cpu().tolist()


def _same_row(a, b):
    """Equality of bits, NaN included."""
    return np.array_equal(np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64))


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


# ------------------------------------------------------------------------------------------------ 1. rows against the reference
@pytest.mark.parametrize("H, W", sc.SHAPES)
def test_rows_against_the_float64_reference(hip_lib, H, W):
    x, y = _dev(*sr.pair("pair", H, W))
    for clamp in (False, True):
        sr.within_bar(_row(x, y, clamp=clamp), sr.case("pair", H, W, clamp), (H, W, clamp))


def test_the_low_variance_pair_against_the_float64_reference(hip_lib):
    H, W = sc.LOW_VARIANCE_SHAPE
    x, y = _dev(*sr.pair("low", H, W))
    sr.within_bar(_row(x, y), sr.case("low", H, W, False), ("low variance", H, W))


# ------------------------------------------------------------------------------------------------ 2. identical image and ground truth
@pytest.mark.parametrize("H, W", ((7, 7), (53, 139), (60, 199)))
def test_equal_images_score_exactly_one(hip_lib, H, W):
    """Numerator and denominator of S are the same float expression on equal inputs (the kernel forms them so), the division is
    correctly rounded, a sum of ones is exact and the finish kernel divides by the count."""
    image, gt = sr.pair("pair", H, W)
    for a in (image, gt):                                              # values in [-0.2, 1.2] and in [0, 1]
        x, = _dev(a)
        assert _row(x, x.clone()) == [1.0, 1.0, 0.0, 0.0]
    x, = _dev(gt)
    assert _row(x, x.clone(), clamp=True) == [1.0, 1.0, 0.0, 0.0]
    gt8, = _dev(mr.make_bytes(H, W))
    looked, = _dev(mr.looked_up(mr.make_bytes(H, W), _table("u8_1.7")))
    assert _row(looked, gt8, lut=_lut("u8_1.7")) == [1.0, 1.0, 0.0, 0.0]


# ------------------------------------------------------------------------------------------------ 3. bytes = looked-up floats
@pytest.mark.parametrize("H, W", ((7, 7), (9, 71), (53, 139), (57, 72)))
def test_the_u8_row_is_the_float_row_on_the_looked_up_image_bit_for_bit(hip_lib, H, W):
    image, _ = mr.make_pair(H, W)
    x, = _dev(image)
    for stride in (3, 4):
        u8 = mr.make_bytes(H, W, stride)
        block = torch.randint(0, 256, (3, H, W, stride), generator=torch.Generator().manual_seed(6), dtype=torch.uint8)
        block[1] = torch.from_numpy(u8)
        block = block.to(DEV)                                          # frame 1 of 3: an odd base address for odd H W at stride 3
        for kind in LUTS:
            gtf, = _dev(mr.looked_up(u8, _table(kind)))
            for clamp in (False, True):
                want = _row(x, gtf, clamp=clamp)
                got = _row(x, block[1], lut=_lut(kind), clamp=clamp)
                assert np.isfinite(want).all() and _same_row(got, want), (stride, kind, clamp, got, want)
                if stride == 3 and (H, W) == sc.ODD[0]:
                    sr.within_bar(got, sr.case(kind, H, W, clamp), (kind, clamp))


# ------------------------------------------------------------------------------------------------ 4. independence of tiling
def test_the_transposed_pair_scores_the_same_and_a_second_call_gives_the_same_bits(hip_lib):
    """Rows and columns are tiled differently (segments of 48 rows, strips of 64 columns), so the transposed pair visits other strip
    and segment boundaries: both are within the bar of the one reference, hence within two bars of each other -- and, asserted
    directly, within one."""
    H, W = sc.TRANSPOSED
    image, gt = sr.pair("pair", H, W)
    x, y = _dev(image, gt)
    xt, yt = _dev(image.transpose(0, 2, 1), gt.transpose(0, 2, 1))
    for clamp in (False, True):
        a, b = _row(x, y, clamp=clamp), _row(xt, yt, clamp=clamp)
        print(clamp, abs(a[0] - b[0]), abs(a[1] - b[1]))
        sr.within_bar(a, sr.case("pair", H, W, clamp), "as is")
        sr.within_bar(b, sr.case("pair", H, W, clamp), "transposed")
        assert abs(a[0] - b[0]) <= sc.TOL and abs(a[1] - b[1]) <= sc.TOL
        assert _same_row(_row(x, y, clamp=clamp), a) and _same_row(_row(xt, yt, clamp=clamp), b)


# ------------------------------------------------------------------------------------------------ 5. non-finite input
def _windows(H, W, r, q):
    """The number of valid 7x7 windows that hold pixel (r, q)."""
    return (min(r, H - sc.WIN) - max(r - sc.WIN + 1, 0) + 1) * (min(q, W - sc.WIN) - max(q - sc.WIN + 1, 0) + 1)


def test_non_finite_pixels(hip_lib):
    H, W = sc.ODD[0]
    assert (_windows(H, W, 20, 66), _windows(H, W, 0, 0), _windows(H, W, 5, 5), _windows(H, W, 50, 130)) == (49, 1, 36, 21)
    image, gt = sr.pair("pair", H, W)
    x, y = _dev(image, gt)
    x[1, 20, 66] = float("nan")                                        # interior: 49 windows of one channel hold it, in both strips
    row = _row(x, y)
    assert np.isnan(row[0]) and np.isnan(row[1]) and row[2:] == [49.0, 0.0], row
    assert _row(x, y, clamp=True)[2:] == [49.0, 0.0]                   # the clamp keeps a NaN
    x, = _dev(image)
    x[0, 0, 0] = float("nan")                                          # the corner lies in one window
    row = _row(x, y)
    assert np.isnan(row[0]) and np.isnan(row[1]) and row[2:] == [1.0, 0.0], row
    x, = _dev(image)
    x[0, 5, 5], x[2, 50, 130] = float("inf"), float("-inf")
    row = _row(x, y)
    assert np.isnan(row[0]) and np.isnan(row[1]) and row[2:] == [float(_windows(H, W, 5, 5) + _windows(H, W, 50, 130)), 0.0], row
    clamped = image.copy()
    clamped[0, 5, 5], clamped[2, 50, 130] = 1.0, 0.0                   # what the clamp makes of +-inf
    row = _row(x, y, clamp=True)
    assert np.isfinite(row).all() and row[2:] == [0.0, 0.0], row
    ref = sr.both(clamped, gt, clamp=True)
    sr.within_bar(row, ref, "clamped +-inf")


# ------------------------------------------------------------------------------------------------ 6. poisoned buffers
@pytest.mark.parametrize("H, W", ((7, 7), (60, 199)))
def test_poisoned_row_and_scratch_give_the_same_result(hip_lib, H, W):
    from ex4dgs_amd import _abi
    from ex4dgs_amd.evaluate import frame_skssim
    x, y = _dev(*sr.pair("pair", H, W))
    want = _row(x, y)
    need = _abi.load().ex4d_frame_skssim_scratch_floats(H, W)
    row = torch.empty(4, dtype=torch.float64, device=DEV)
    scratch = torch.empty(need, dtype=torch.float32, device=DEV)
    row.view(torch.uint8).fill_(0xFF)
    scratch.view(torch.uint8).fill_(0xFF)
    assert torch.isnan(scratch).all()
    got = frame_skssim(x, y, row=row, scratch=scratch)
    assert got is row and np.isfinite(want).all() and _same_row(row.cpu().tolist(), want)


# ------------------------------------------------------------------------------------------------ 7. the table, a graph, evaluate_set
def _views(H, W, n, seed):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(3, H, W, generator=g).to(DEV) * 1.4 - 0.2, torch.rand(3, H, W, generator=g).to(DEV)) for _ in range(n)]


def test_five_views_into_both_tables_with_one_read_back(hip_lib):
    from ex4dgs_amd.evaluate import Evaluator, frame_metrics
    H, W = 49, 75
    ev = Evaluator(6, H, W, skssim=True)
    assert tuple(ev.table_sk.shape) == (6, 4) and ev.table_sk.dtype == torch.float64 and bool(torch.isnan(ev.table_sk).all())
    views = _views(H, W, 5, 8)
    gt8, = _dev(mr.make_bytes(H, W))
    order = (1, 3, 0, 4, 2)
    for k, i in enumerate(order):
        ev.score(i, views[k][0], gt8 if k == 2 else views[k][1], name=f"v{i}", clamp=bool(k % 2))
    rows, rows_sk = ev.rows(), ev.rows_sk()
    assert tuple(rows_sk.shape) == (6, 4) and rows_sk.dtype == torch.float64 and rows_sk.device.type == "cpu"
    for k, i in enumerate(order):
        gt = gt8 if k == 2 else views[k][1]
        want = _row(views[k][0], gt, clamp=bool(k % 2))
        assert np.isfinite(want).all() and _same_row(rows_sk[i].tolist(), want), (k, i)
        assert _same_row(rows[i].tolist(), frame_metrics(views[k][0], gt, clamp=bool(k % 2)).cpu().tolist()), (k, i)
    assert bool(torch.isnan(rows_sk[5]).all()) and bool(torch.isnan(rows[5]).all())
    mean, per_view = ev.report()
    assert list(mean) == ["SSIM", "PSNR", "L1", "SKSSIM", "SKSSIM2"] == list(per_view)
    assert list(per_view["SKSSIM2"]) == ["v0", "v1", "v2", "v3", "v4"]
    for k, i in enumerate(order):
        assert per_view["SKSSIM"][f"v{i}"] == float(np.float32(rows_sk[i, 0].item())) and per_view["SKSSIM2"][f"v{i}"] == float(np.float32(rows_sk[i, 1].item()))
    plain = Evaluator(2, H, W)                                         # the default: no second table, no second launch pair
    assert plain.table_sk is None and plain.scratch_sk is None
    plain.score(0, *views[0])
    assert set(plain.report()[0]) == {"SSIM", "PSNR", "L1"}
    with pytest.raises(RuntimeError, match="skssim=True"):
        plain.rows_sk()
    with pytest.raises(RuntimeError, match="H, W >= 7"):
        Evaluator(2, 6, 40, skssim=True)


def test_a_score_replays_from_a_graph(hip_lib):
    from ex4dgs_amd.evaluate import Evaluator, frame_metrics
    H, W = 49, 75
    contents = _views(H, W, 2, 12)
    x, y = (t.clone() for t in contents[0])
    ev = Evaluator(1, H, W, skssim=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):              # one eager call first
        ev.score(0, x, y, name="a", clamp=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev.score(0, x, y, name="a", clamp=True)
    for content in contents:
        x.copy_(content[0])
        y.copy_(content[1])
        ev.table.fill_(float("nan"))
        ev.table_sk.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        want = _row(content[0], content[1], clamp=True)
        assert np.isfinite(want).all() and _same_row(ev.rows_sk()[0].tolist(), want)
        assert _same_row(ev.rows()[0].tolist(), frame_metrics(content[0], content[1], clamp=True).cpu().tolist())


def test_evaluate_set_writes_the_five_keys_with_the_option_and_three_without(hip_lib, tmp_path):
    from ex4dgs_amd.evaluate import evaluate_set
    from ex4dgs_amd.frames import gt_lut
    from ex4dgs_amd.render import render
    from tests.test_gpu_metrics import _tiny_set
    cfg, model, cameras, bg, store, _ = _tiny_set()
    lut = gt_lut(1.7)
    kw = dict(lut=lut, background=bg, near=cfg.min_depth, far=cfg.max_depth)
    names = [c.image_name for c in cameras]
    mean, per_view, ev = evaluate_set(model, cameras, store, out_dir=str(tmp_path / "sk"), skssim=True, **kw)
    on_disk = json.load(open(tmp_path / "sk" / "mean_metrics.json")), json.load(open(tmp_path / "sk" / "all_metrics.json"))
    assert on_disk == (mean, per_view)
    assert set(mean) == set(per_view) == {"SSIM", "PSNR", "L1", "SKSSIM", "SKSSIM2"} and all(list(per_view[k]) == names for k in per_view)
    mean3, per_view3, ev3 = evaluate_set(model, cameras, store, out_dir=str(tmp_path / "plain"), **kw)
    on_disk3 = json.load(open(tmp_path / "plain" / "mean_metrics.json")), json.load(open(tmp_path / "plain" / "all_metrics.json"))
    assert on_disk3 == (mean3, per_view3) and set(mean3) == set(per_view3) == {"SSIM", "PSNR", "L1"} and ev3.table_sk is None
    assert mean3 == {k: mean[k] for k in mean3} and per_view3 == {k: per_view[k] for k in per_view3}
    with torch.no_grad():
        for i, cam in enumerate(cameras):
            image = render(cam, model, None, bg, near=cfg.min_depth, far=cfg.max_depth)["render"]
            gt = lut.to(DEV)[store.get(i).long()].permute(2, 0, 1).contiguous()
            ref = sr.both(image.cpu().numpy(), gt.cpu().numpy())
            row = ev.rows_sk()[i].tolist()
            sr.within_bar(row, ref, ("evaluate_set", names[i]))
            assert (per_view["SKSSIM"][names[i]], per_view["SKSSIM2"][names[i]]) == (float(np.float32(row[0])), float(np.float32(row[1])))


def test_python_refusals(hip_lib):
    from ex4dgs_amd.evaluate import frame_skssim
    x = torch.zeros(3, 8, 8, device=DEV)
    for shape in ((3, 6, 8), (3, 8, 6)):
        small = torch.zeros(*shape, device=DEV)
        with pytest.raises(RuntimeError, match="win_size exceeds image extent"):
            frame_skssim(small, small)
    for bad_gt, match in ((x[:, :7], "image's shape"), (x.double(), "float32 \\[3,H,W\\] or uint8"), (x.cpu(), "device"),
                          (torch.zeros(8, 8, 2, dtype=torch.uint8, device=DEV), "\\[H,W,3\\] or \\[H,W,4\\]")):
        with pytest.raises(RuntimeError, match=match):
            frame_skssim(x, bad_gt)
    with pytest.raises(RuntimeError, match="lut= belongs to uint8"):
        frame_skssim(x, x, lut=torch.zeros(256))
    with pytest.raises(RuntimeError, match="\\[3,H,W\\]"):
        frame_skssim(x[:2], x[:2])
    with pytest.raises(RuntimeError, match="row must be"):
        frame_skssim(x, x, row=torch.zeros(4, device=DEV))
    with pytest.raises(RuntimeError, match="scratch must be"):
        frame_skssim(x, x, scratch=torch.zeros(4, device=DEV))
