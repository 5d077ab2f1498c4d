"""The tiling-edge sweep of the fused L1 + SSIM loss (tests/loss_cases.py) stays on inputs where its bars are reachable: the
reference formulation itself, run in float32, must sit within HALF of every bar against the float64 oracle on every case, so
that a HIP kernel that is as accurate as the reference passes tests/test_gpu_loss_edges.py with room to spare."""
import torch

from tests import loss_cases as lc


def test_sweep_covers_the_edges_it_names():
    shapes = lc.sweep_shapes()
    assert len(shapes) == len(lc.HEIGHTS) * len(lc.WIDTHS) + len(lc.CHANNELS) * len(lc.CHANNEL_SHAPES) + len(lc.WORK_ITEM_SHAPES) == 318
    assert tuple(lc.work_items(H, W) for _, H, W in lc.WORK_ITEM_SHAPES) == lc.WORK_ITEMS
    assert {n % 8 == 0 for n in lc.WORK_ITEMS} == {True, False}                      # with and without padded workgroups
    last = {(H - 1) % lc.SEG + 1 for H in lc.HEIGHTS}                                 # output rows of the last segment
    assert last >= {1, 4, 5, 6, 10, 11, 47, 48} and {(r + 10) % 4 for r in last if r < 12} == {0, 1, 2, 3}
    assert {(r + 10) % 4 for H in lc.HEIGHTS if H > lc.SEG for r in [(H - 1) % lc.SEG + 1]} == {0, 1, 2, 3}
    assert {C % lc.CG for C in lc.CHANNELS} == {0, 1, 2} and max(lc.CHANNELS) > 2 * lc.CG


def test_float32_reference_sits_within_half_of_every_bar_on_the_sweep():
    from oracle import loss_oracle
    worst = dict(loss=0.0, l1_errors=0.0, ssim_errors=0.0, grad_over_bar=0.0)
    for shape in lc.sweep_shapes():
        image, gt = lc.make_pair(shape)
        for lam in lc.LAMBDAS:
            r64 = loss_oracle.l1_ssim(image, gt, lam)
            r32 = loss_oracle.l1_ssim(image, gt, lam, dtype=torch.float32)
            e = lc.errors(r32, r64)
            lc.assert_within_bars(e, scale=0.5, what=(shape, lam))
            for k in ("loss", "l1_errors", "ssim_errors"):
                worst[k] = max(worst[k], e[k])
            worst["grad_over_bar"] = max(worst["grad_over_bar"], e["grad"] / e["grad_bar"])
    print("float32 reference against float64 over the sweep, worst:", worst)
