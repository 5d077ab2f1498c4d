"""Times the multi-rank statistics merge (ex4d_densify_stats_merge, what DensityStats.sync() runs after its all-gather) at config 3's
row counts (0.8 M static and 0.2 M dynamic Gaussians) for W = 2 and W = 8 ranks on one GPU, against a torch composition of the same
fold on the same buffers: sum, max, min and where over the stacked blocks, and the reset of the own pending block.  One "merge" is
both groups: two launches of the kernel.  The variants take turns in windows of at least a second between device events; the median
window is reported with its min / max, and the bytes the fold has to move -- (W + 1) x 36 B read, 72 B written per Gaussian -- over
that time as a fraction of the 8 TB/s HBM peak of the MI355X.  Every variant rotates over buffer sets that together exceed twice the
Infinity Cache, so the blocks come from HBM.  The all-gather before the merge is not part of it: its wire time on
real links is not measured here (one GPU).

Prints one JSON line; --out writes it to a file as well (profiles/stats_merge_cfg3.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

WINDOW_S, ROUNDS, PEAK_BYTES_PER_S = 1.0, 3, 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from ex4dgs_amd import densify
    from ex4dgs_amd.scene import CONFIGS
    from tests import stats_merge_ref as mr
    dev = torch.device("cuda:0")
    cfg = CONFIGS["cfg3"]
    nd = int(round(cfg.P * cfg.dyn_frac))
    rows = (cfg.P - nd, nd)
    init = torch.tensor(densify.STAT_INIT, dtype=torch.float32, device=dev).view(9, 1)

    def torch_fold(total, pend, own):
        total[:5] += pend[:, :5].sum(0)
        total[5] = torch.maximum(total[5], pend[:, 5].max(0).values)
        total[6] = torch.minimum(total[6], pend[:, 6].min(0).values)
        m, who = pend[:, 7].min(0)                               # the first minimum: the lowest rank on a tie
        ts = pend[:, 8].gather(0, who.unsqueeze(0))[0]
        take = total[7] > m
        total[8] = torch.where(take, ts, total[8])
        total[7] = torch.where(take, m, total[7])
        own.copy_(init.expand_as(own))

    def window(fn, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches              # us per merge

    result = {}
    for W in (2, 8):
        # several sets of buffers, taken in turn: together larger than twice the 256 MiB Infinity Cache, so that a merge finds its blocks
        # in HBM as the first merge after an all-gather of fresh statistics does, not in the cache where the previous launch left them
        footprint = sum(n * (W + 2) * 36 for n in rows)
        sets = []
        for s_ in range(-(-(512 << 20) // footprint)):
            groups = []
            for n in rows:
                total, pend = mr.make_case(W, n, seed=1 + s_)
                pend[:, :5] = abs(pend[:, :5]) * 1e-6            # sums that stay finite over a million folds
                groups.append((torch.from_numpy(mr.neutral(n)).to(dev), torch.nan_to_num(torch.from_numpy(pend)).to(dev), torch.from_numpy(mr.neutral(n)).to(dev)))
            sets.append(groups)
        turn = {"hip": 0, "torch": 0}

        def variant(name, fold):
            def run():
                turn[name] = (turn[name] + 1) % len(sets)
                for t, p, o in sets[turn[name]]:
                    fold(t, p, o)
            return run
        variants = {"hip": variant("hip", densify.merge_stats), "torch": variant("torch", torch_fold)}
        est = {}
        for k, fn in variants.items():
            window(fn, 2 * len(sets))                            # warm-up: code objects, the allocator's blocks of torch's temporaries
            est[k] = window(fn, 20 * len(sets))                  # the launches a window takes
        ts = {k: [] for k in variants}
        for _ in range(ROUNDS):
            for k, fn in variants.items():
                ts[k].append(window(fn, int(WINDOW_S * 1e6 / est[k]) + 1))
        nbytes = sum(n * ((W + 1) * 36 + 72) for n in rows)
        row = {"bytes_moved": nbytes, "buffer_sets": len(sets), "footprint_bytes_per_set": footprint}
        for k, t in ts.items():
            med = sorted(t)[len(t) // 2]
            row[k] = {"median_us": round(med, 2), "min_us": round(min(t), 2), "max_us": round(max(t), 2), "launches_per_window": int(WINDOW_S * 1e6 / est[k]) + 1,
                      "bytes_per_s": round(nbytes / (med * 1e-6)), "fraction_of_hbm_peak": round(nbytes / (med * 1e-6) / PEAK_BYTES_PER_S, 3)}
        row["torch_over_hip"] = round(row["torch"]["median_us"] / row["hip"]["median_us"], 2)
        result[f"W={W}"] = row
    doc = {"config": "cfg3", "device": torch.cuda.get_device_name(0), "static": rows[0], "dynamic": rows[1], "window_s": WINDOW_S, "rounds": ROUNDS,
           "hbm_peak_bytes_per_s": PEAK_BYTES_PER_S, "merge": result,
           "all_gather_wire_time": "not measured beyond one GPU"}
    print(json.dumps(doc))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
