#!/usr/bin/env python3
"""A/B of the feature blend against the plain colour blend doing the same work, on the bench frame, interleaved rounds in ONE
process (MI355X guide, rule 24).  Stages 1-2 run once (colour_stage = 1: every record carries its colour), then per round:
  A  gsr_blend with blend_impl = 1, saturation_rule = 1: blend_kernel, the plain-C kernel — same entries, same T == 0 stop rule,
     same blend_one, colours read from the record
  B  gsr_blend_features with features (z_cam, 1, 0): the same kernel under the feature policy
each between two events — median, min, max and spread over the rounds, B / A, and the two blends' counters (they must agree).
Then whole calls, synchronised: Rasterizer.render against render_depth and render_rgbd in ms per frame.
Prints only, unless --out names a file.  The measurement runs in a child process under a time limit (--timeout seconds;
tools/ab_harness.py).
usage: tools/features_ab.py [--workload bicycle] [--rounds 15] [--early-out-T 0] [--timeout 420]"""
import ab_harness as ab

WHAT = {"A": "gsr_blend, blend_impl=1 saturation_rule=1 (blend_kernel)", "B": "gsr_blend_features (blend_kernel<FeatureBlend>)"}


def arguments(argv=None):
    return ab.arguments("features_ab", writes=False, argv=argv)


def worker(a):
    import torch

    f = ab.bench_frame(a)
    from gsr_amd import renderer
    from gsr_amd._lib import check, lib

    n, W, H, dev, sp, R, cam = f.n, f.W, f.H, f.dev, f.sp, f.R, f.cam
    feats = R._depth_features(cam)
    oA = renderer.make_options(early_out_T=a.early_out_T, blend_impl=1, saturation_rule=1, colour_stage=1)
    oB = renderer.make_options(early_out_T=a.early_out_T, colour_stage=1)
    outA, outB = (torch.empty((H, W, 3), dtype=torch.float32, device=dev) for _ in "AB")
    TA, TB = (torch.empty((H, W), dtype=torch.float32, device=dev) for _ in "AB")
    f.make_lists(oA)

    def run_a(T=None):
        check(lib.gsr_blend(None, *f.lists(oA), outA.data_ptr(), T, sp))

    def run_b(T=None):
        check(lib.gsr_blend_features(*f.lists(oB), feats.data_ptr(), outB.data_ptr(), T, sp))

    times, stats = ab.interleaved((("A", run_a), ("B", run_b)), a.rounds, "events", stats=R.stats)
    lines = [f"{a.workload}: {n} gaussians, {W}x{H}, {a.rounds} interleaved rounds (blend stage alone, tile-order kernel included)"]
    med = {}
    for name in "AB":
        line, med[name] = ab.summary(name, times[name], stats[name], WHAT[name], ab.COUNTERS + ("colour_evals",))
        lines.append(line)
    lines.append(f"  B / A at the median: {med['B'] / med['A']:.3f}   counters agree: {ab.same_counters(stats, 'A', 'B', ab.COUNTERS + ('n_pairs',))}")
    # the final T of B against A's blend asked for its T (the colour frame itself differs: other features)
    run_a(TA.data_ptr())
    run_b(TB.data_ptr())
    torch.cuda.synchronize(dev)
    lines.append(f"  final T of B == final T of A: {bool(torch.equal(TA, TB))};  max |alpha - (1 - T)| {float((outB[..., 1] - (1 - TB)).abs().max()):.2e};  "
                 f"depth map max {float(outB[..., 0].max()):.3f}")

    # whole calls (checked frames: each ends with the counters' read-back), ms per frame
    calls = (("render", lambda: R.render(cam)), ("render_depth", lambda: R.render_depth(cam)), ("render_rgbd", lambda: R.render_rgbd(cam)))
    per, _ = ab.interleaved(calls, a.rounds, "wall")
    lines += [ab.summary(k, per[k], what="the whole call, ms per frame")[0] for k, _ in calls]
    ab.report(lines, a.out)


if __name__ == "__main__":
    ab.main(__file__, arguments(), worker)
