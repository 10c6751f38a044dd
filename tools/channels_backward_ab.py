#!/usr/bin/env python3
"""The channel blend's transpose against the channel blend itself, on the bench frame, interleaved rounds in ONE process.
Stages 1-2 run once (colour_stage = 0), then per round and per channel count C:
  A  ONE gsr_blend_channels on an [n, C] array: the forward, walks of up to 16 channels
  B  ONE gsr_blend_channels_backward of an [H, W, C] upstream gradient into an [n, C] array (zeroed outside the timed span)
each between two events — median, min, max and spread over the rounds, B / A and both sides' counters (they must agree: the
backward walks the forward's lists with the forward's stop rule).  No ratio is fixed in advance; what to compare with is the issue
count of the DPP reduction, (14 + 7 CH) / (14 + CH) = 4.2 at CH = 16, and the atomic floor: fetched_entries x nch x 4 B of float
adds per walk at the chip-wide rate of 1.3 TB/s (an upper bound on the bytes: rows no wave touched are not flushed).
Writes what it prints to profiles/channels_backward_ab.txt (--out).  The measurement runs in a child process under a time limit
(--timeout seconds; tools/ab_harness.py).
usage: tools/channels_backward_ab.py [--workload bicycle] [--rounds 15] [--channels 8,16,32] [--early-out-T 0] [--timeout 420]"""
import ab_harness as ab

ATOMIC_RATE = 1.3e12  # bytes of float adds per second, chip-wide


def arguments(argv=None):
    return ab.arguments("channels_backward_ab", extra=lambda ap: ap.add_argument("--channels", default="8,16,32"), argv=argv)


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
        Gm = torch.randn((H, W, n_ch), generator=gen).to(dev)
        out = torch.empty((H, W, n_ch), dtype=torch.float32, device=dev)
        gF = torch.zeros((n, n_ch), dtype=torch.float32, device=dev)

        def run_a():
            check(lib.gsr_blend_channels(*f.lists(o), F.data_ptr(), n_ch, n_ch, out.data_ptr(), None, sp))

        def run_b():
            check(lib.gsr_blend_channels_backward(*f.lists(o), Gm.data_ptr(), n_ch, gF.data_ptr(), n_ch, sp))

        times, stats = ab.interleaved((("A", run_a), ("B", run_b)), a.rounds, "events", before=gF.zero_, stats=f.R.stats)
        # <A F, G> = <F, A^T G>: the run timed last is the transpose of the forward timed last
        lhs, rhs = float((out.double() * Gm.double()).sum()), float((F.double() * gF.double()).sum())
        lines.append(f"C = {n_ch}: A = 1 x gsr_blend_channels, B = 1 x gsr_blend_channels_backward")
        med = {}
        for name in "AB":
            line, med[name] = ab.summary(name, times[name], stats[name])
            lines.append(line)
        floor_ms = stats["B"]["fetched_entries"] * n_ch * 4 / ATOMIC_RATE * 1e3
        lines.append(f"  B / A at the median: {med['B'] / med['A']:.3f}   counters agree: {ab.same_counters(stats, 'A', 'B', ab.COUNTERS + ('n_pairs',))}   "
                     f"atomic floor (fetched_entries x {n_ch} x 4 B / 1.3 TB/s): "
                     f"{floor_ms:.4f} ms = {floor_ms / med['B'] * 100:.1f} % of B   <AF,G> {lhs:.9g} <F,AtG> {rhs:.9g}")
        del F, Gm, out, gF
    ab.report(lines, a.out)


if __name__ == "__main__":
    ab.main(__file__, arguments(), worker)
