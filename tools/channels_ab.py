#!/usr/bin/env python3
"""A/B of many channels per walk against three per walk, on the bench frame, interleaved rounds in ONE process.
Stages 1-2 run once (colour_stage = 0), then per round and per channel count C:
  A  ceil(C / 3) calls of gsr_blend_features on pre-sliced contiguous [n, 3] arrays (the last zero-padded): the three-channel
     kernel, what Rasterizer.render_features did for C > 3 before gsr_blend_channels existed — without its slicing copies
  B  ONE gsr_blend_channels on the [n, C] array: walks of up to 16 channels
each between two events — median, min, max and spread over the rounds, B / A, both sides' counters (they must agree) and whether
the maps agree bit for bit.  B counts as faster for a C when its median is below A's by more than A's own round-to-round spread
(max - min).  Writes what it prints to profiles/channels_ab.txt (--out).  The measurement runs in a child process under a time
limit (--timeout seconds; tools/ab_harness.py).
usage: tools/channels_ab.py [--workload bicycle] [--rounds 15] [--channels 8,16,32] [--early-out-T 0] [--timeout 420]"""
import ab_harness as ab


def arguments(argv=None):
    return ab.arguments("channels_ab", extra=lambda ap: ap.add_argument("--channels", default="8,16,32"), argv=argv)


def worker(a):
    import torch

    f = ab.bench_frame(a)
    from gsr_amd import renderer
    from gsr_amd._lib import check, lib

    n, W, H, dev, sp = f.n, f.W, f.H, f.dev, f.sp
    o = renderer.make_options(early_out_T=a.early_out_T, colour_stage=0)
    f.make_lists(o)
    lines = [f"{a.workload}: {n} gaussians, {W}x{H}, {a.rounds} interleaved rounds after 2 of warm-up (stage 3 alone, its tile-order kernel "
             f"included; early_out_T = {a.early_out_T})"]
    gen = torch.Generator().manual_seed(1)
    for n_ch in [int(x) for x in a.channels.split(",")]:
        F = torch.randn((n, n_ch), generator=gen).to(dev)
        groups = []
        for c0 in range(0, n_ch, 3):
            g = torch.zeros((n, 3), dtype=torch.float32, device=dev)
            g[:, :min(3, n_ch - c0)] = F[:, c0:c0 + 3]
            groups.append(g)
        outA = [torch.empty((H, W, 3), dtype=torch.float32, device=dev) for _ in groups]
        outB = torch.empty((H, W, n_ch), dtype=torch.float32, device=dev)

        def run_a():
            for g, m in zip(groups, outA):
                check(lib.gsr_blend_features(*f.lists(o), g.data_ptr(), m.data_ptr(), None, sp))

        def run_b():
            check(lib.gsr_blend_channels(*f.lists(o), F.data_ptr(), n_ch, n_ch, outB.data_ptr(), None, sp))

        times, stats = ab.interleaved((("A", run_a), ("B", run_b)), a.rounds, "events", stats=f.R.stats)
        same_bits = bool(torch.equal(torch.cat(outA, -1)[..., :n_ch], outB))
        lines.append(f"C = {n_ch}: A = {len(groups)} x gsr_blend_features, B = 1 x gsr_blend_channels")
        med = {}
        for name in "AB":
            line, med[name] = ab.summary(name, times[name], stats[name])
            lines.append(line)
        lines.append(f"  B / A at the median: {med['B'] / med['A']:.3f}   B faster by more than A's spread: "
                     f"{med['B'] < med['A'] - (max(times['A']) - min(times['A']))}   "
                     f"counters agree: {ab.same_counters(stats, 'A', 'B', ab.COUNTERS + ('n_pairs',))}   maps agree bit for bit: {same_bits}")
        del F, groups, outA, outB
    ab.report(lines, a.out)


if __name__ == "__main__":
    ab.main(__file__, arguments(), worker)
