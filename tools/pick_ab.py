#!/usr/bin/env python3
"""A/B of the pick kernel against the feature blend on the bench frame, interleaved rounds in ONE process (MI355X guide, rule 24).
Stages 1-2 run once, then per round, each between two events on the same lists:
  A  gsr_blend_features with features (z_cam, 1, 0): blend_kernel<FeatureBlend>, the baseline
  B  gsr_blend_pick without a count: blend_pick_kernel<false>, which stops once neither id can change
  C  gsr_blend_pick with the count: blend_pick_kernel<true>, which walks to T == 0 like A
Median, min, max and spread over the rounds, B / A and C / A, each call's wave_entries / fetched_entries, and whether B's and C's
ids and weights agree bit for bit.  Writes what it prints to profiles/pick_ab.txt (--out).  The measurement runs in a child process
under a time limit (--timeout seconds; tools/ab_harness.py).
usage: tools/pick_ab.py [--workload bicycle] [--rounds 30] [--early-out-T 0] [--median-T 0.5] [--timeout 420]"""
import ab_harness as ab

WHAT = {"A": "gsr_blend_features (blend_kernel<FeatureBlend>)", "B": "gsr_blend_pick, count = NULL (blend_pick_kernel<false>)",
        "C": "gsr_blend_pick with count (blend_pick_kernel<true>)"}


def arguments(argv=None):
    return ab.arguments("pick_ab", rounds=30, extra=lambda ap: ap.add_argument("--median-T", type=float, default=0.5), argv=argv)


def worker(a):
    import torch

    f = ab.bench_frame(a)
    from gsr_amd import renderer
    from gsr_amd._lib import check, lib

    n, W, H, dev, sp = f.n, f.W, f.H, f.dev, f.sp
    feats = f.R._depth_features(f.cam)
    o = renderer.make_options(early_out_T=a.early_out_T, colour_stage=0)
    out_map = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    ids = {k: [torch.empty((H, W), dtype=torch.int32, device=dev) for _ in range(3)] for k in "BC"}
    wts = {k: torch.empty((H, W), dtype=torch.float32, device=dev) for k in "BC"}
    f.make_lists(o)

    def run_a():
        check(lib.gsr_blend_features(*f.lists(o), feats.data_ptr(), out_map.data_ptr(), None, sp))

    def run_pick(k):
        best, med, cnt = ids[k]
        check(lib.gsr_blend_pick(*f.lists(o), a.median_T, best.data_ptr(), wts[k].data_ptr(), med.data_ptr(),
                                 cnt.data_ptr() if k == "C" else None, sp))

    legs = (("A", run_a), ("B", lambda: run_pick("B")), ("C", lambda: run_pick("C")))
    times, stats = ab.interleaved(legs, a.rounds, "events", stats=f.R.stats)
    lines = [f"{a.workload}: {n} gaussians, {W}x{H}, {a.rounds} interleaved rounds after 2 warm-up rounds (blend stage alone, tile-order kernel "
             f"included), early_out_T {a.early_out_T}, median_T {a.median_T}"]
    med = {}
    for name, _ in legs:
        line, med[name] = ab.summary(name, times[name], stats[name], WHAT[name], ab.COUNTERS + ("colour_evals",))
        lines.append(line)
    same_ids = all(torch.equal(x, y) for x, y in zip(ids["B"][:2], ids["C"][:2])) and torch.equal(wts["B"], wts["C"])
    lines.append(f"  B / A at the median: {med['B'] / med['A']:.3f}   C / A: {med['C'] / med['A']:.3f}   B's median <= A's: {med['B'] <= med['A']}")
    lines.append(f"  wave_entries B / A: {stats['B']['wave_entries'] / max(stats['A']['wave_entries'], 1):.3f}   fetched_entries B / A: "
                 f"{stats['B']['fetched_entries'] / max(stats['A']['fetched_entries'], 1):.3f}   C's counters are A's: "
                 f"{ab.same_counters(stats, 'C', 'A')}")
    lines.append(f"  B's ids and weights == C's: {same_ids};  pixels with a dominant gaussian {int((ids['C'][0] >= 0).sum())} of {W * H}, with a "
                 f"median {int((ids['C'][1] >= 0).sum())}, contributors per pixel: mean {float(ids['C'][2].float().mean()):.1f} max {int(ids['C'][2].max())}")
    ab.report(lines, a.out)


if __name__ == "__main__":
    ab.main(__file__, arguments(), worker)
