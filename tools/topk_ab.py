#!/usr/bin/env python3
"""A/B of the top-k kernels against the feature blend on the bench frame, interleaved rounds in ONE process (MI355X guide, rule 24).
Stages 1-2 run once, then per round, each between two events on the same lists:
  A  gsr_blend_features with features (z_cam, 1, 0): blend_kernel<FeatureBlend>, the yardstick
  B  gsr_blend_topk HEAVIEST k = 4,  no final T   (blend_topk_kernel<4, false>)
  C  gsr_blend_topk HEAVIEST k = 8,  no final T   (blend_topk_kernel<8, false>)
  D  gsr_blend_topk HEAVIEST k = 16, no final T   (blend_topk_kernel<16, false>)
  E  gsr_blend_topk HEAVIEST k = 8 with final T: walks like A
  F  gsr_blend_topk NEAREST  k = 4,  no final T   (blend_topk_kernel<4, true>)
Median, min, max and spread over the rounds, the ratios to A, each call's wave_entries / fetched_entries, and whether C's and E's
lists agree bit for bit.  Appends what it prints to profiles/topk_ab.txt (--out), under --label.  The measurement runs in a child
process under a time limit (--timeout seconds; tools/ab_harness.py).
The form of the insertion without its wave-uniform guard is the analysis build of the library:
  make -C torch-gaussian-splatting-rasterizer_amd/csrc ../../tools/libgsr_topk_noguard.so
  GSR_LIB_PATH=tools/libgsr_topk_noguard.so tools/topk_ab.py --label "no guard"
usage: tools/topk_ab.py [--workload bicycle] [--rounds 30] [--early-out-T 0] [--label guarded] [--timeout 420]"""
import os

import ab_harness as ab

RUNS = {"B": (4, 0, False), "C": (8, 0, False), "D": (16, 0, False), "E": (8, 0, True), "F": (4, 1, False)}  # k, select, final T


def arguments(argv=None):
    return ab.arguments("topk_ab", rounds=30, label="guarded", argv=argv)


def worker(a):
    import torch

    f = ab.bench_frame(a)
    from gsr_amd import _lib, renderer
    from gsr_amd._lib import check, lib

    n, W, H, dev, sp = f.n, f.W, f.H, f.dev, f.sp
    feats = f.R._depth_features(f.cam)
    o = renderer.make_options(early_out_T=a.early_out_T, colour_stage=0)
    out_map = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    ids = {r: torch.empty((H, W, k), dtype=torch.int32, device=dev) for r, (k, _, _) in RUNS.items()}
    wts = {r: torch.empty((H, W, k), dtype=torch.float32, device=dev) for r, (k, _, _) in RUNS.items()}
    final_T = torch.empty((H, W), dtype=torch.float32, device=dev)
    f.make_lists(o)

    def run_a():
        check(lib.gsr_blend_features(*f.lists(o), feats.data_ptr(), out_map.data_ptr(), None, sp))

    def run_topk(r):
        k, select, with_T = RUNS[r]
        check(lib.gsr_blend_topk(*f.lists(o), k, select, ids[r].data_ptr(), wts[r].data_ptr(), final_T.data_ptr() if with_T else None, sp))

    legs = [("A", run_a)] + [(r, (lambda r=r: run_topk(r))) for r in RUNS]
    times, stats = ab.interleaved(legs, a.rounds, "events", stats=f.R.stats)
    lines = [f"{os.path.basename(_lib.LIB_PATH)}  {a.workload}: {n} gaussians, {W}x{H}, {a.rounds} interleaved rounds after 2 warm-up "
             f"rounds (blend stage alone, tile-order kernel included), early_out_T {a.early_out_T}"]
    what = {"A": "gsr_blend_features (blend_kernel<FeatureBlend>)"}
    for r, (k, select, with_T) in RUNS.items():
        what[r] = f"gsr_blend_topk {'NEAREST' if select else 'HEAVIEST'} k = {k}{', with final T' if with_T else ''}"
    med = {}
    for name, _ in legs:
        line, med[name] = ab.summary(name, times[name], stats[name], what[name])
        lines.append(line)
    lines.append("  ratios to A at the median: " + ab.ratios(med, "A"))
    lines.append("  wave_entries to A's: " + "   ".join(f"{r} {stats[r]['wave_entries'] / max(stats['A']['wave_entries'], 1):.3f}" for r in RUNS)
                 + f"   E's counters are A's: {ab.same_counters(stats, 'E', 'A')}")
    filled = (ids["D"] >= 0).sum(-1)
    lines.append(f"  C's lists == E's: {torch.equal(ids['C'], ids['E']) and torch.equal(wts['C'], wts['E'])};  B's == the first 4 slots of C's: "
                 f"{torch.equal(ids['B'], ids['C'][..., :4]) and torch.equal(wts['B'], wts['C'][..., :4])};  filled slots per pixel at k = 16: "
                 f"mean {float(filled.float().mean()):.1f}, pixels with all 16 {int((filled == 16).sum())} of {W * H};  weight outside the "
                 f"8 heaviest, mean over pixels: {float((1.0 - final_T - wts['E'].sum(-1)).clamp(min=0).mean()):.4f}")
    ab.report(lines, a.out, a.label, append=True)


if __name__ == "__main__":
    ab.main(__file__, arguments(), worker)
