#!/usr/bin/env python3
"""The splat gradient against the two walks it is made of, on the bench frame, interleaved rounds in ONE process.
Stages 1-2 run once (colour_stage = 0), then per round and per channel count C:
  A  gsr_blend_channels on an [n, C] array + gsr_blend_channels_backward of an [H, W, C] upstream gradient: a forward walk and a
     walk with the DPP reduction and the atomic flush, the two things the new kernel does in its two passes
  B  ONE gsr_blend_splat_backward of the same features and upstream gradient, with grad_T, into an [n, 8] array (zeroed outside
     the timed span)
each between two events — median, min, max and spread over the rounds, B / A and both sides' counters (they must agree: the second
pass walks the forward's lists with the forward's stop rule).  No ratio is fixed in advance.  What to compare with is the issue
count per survivor: A = (14 + CH) + (14 + 7 CH) with CH the instantiated width, B = 2 (14 + CH) for the two walks plus, for a
survivor with a nonzero e in some pixel, 8 products and 8 x 9 reduction issues (six DPP adds a value, lane 63's LDS add, the ballot
and e itself).
Writes what it prints to profiles/splat_gradient_ab.txt (--out).  The measurement runs in a child process under a time limit
(--timeout seconds; tools/ab_harness.py).
usage: tools/splat_gradient_ab.py [--workload bicycle] [--rounds 15] [--channels 3,16] [--early-out-T 0] [--abs] [--timeout 420]"""
import ab_harness as ab


def width_of(n_ch, min_width):
    return 16 if n_ch > 8 else 8 if n_ch > 4 or min_width > 4 else 4


def flags(ap):
    ap.add_argument("--channels", default="3,16")
    ap.add_argument("--abs", action="store_true", help="B with want_abs")


def arguments(argv=None):
    return ab.arguments("splat_gradient_ab", extra=flags, argv=argv)


def worker(a):
    import torch

    f = ab.bench_frame(a)
    from gsr_amd import renderer
    from gsr_amd._lib import check, lib

    n, W, H, dev, sp = f.n, f.W, f.H, f.dev, f.sp
    o = renderer.make_options(early_out_T=a.early_out_T, colour_stage=0)
    f.make_lists(o)
    lines = [f"{a.workload}: {n} gaussians, {W}x{H}, {a.rounds} interleaved rounds after 2 of warm-up (stage 3 alone, its tile-order kernel "
             f"included; early_out_T = {a.early_out_T}; want_abs = {int(a.abs)})"]
    gen = torch.Generator().manual_seed(1)
    for n_ch in [int(x) for x in a.channels.split(",")]:
        F = torch.randn((n, n_ch), generator=gen).to(dev)
        Gm = torch.randn((H, W, n_ch), generator=gen).to(dev)
        gT = torch.randn((H, W), generator=gen).to(dev)
        out = torch.empty((H, W, n_ch), dtype=torch.float32, device=dev)
        gF = torch.zeros((n, n_ch), dtype=torch.float32, device=dev)
        gS = torch.zeros((n, 8), dtype=torch.float32, device=dev)

        def run_a():
            check(lib.gsr_blend_channels(*f.lists(o), F.data_ptr(), n_ch, n_ch, out.data_ptr(), None, sp))
            check(lib.gsr_blend_channels_backward(*f.lists(o), Gm.data_ptr(), n_ch, gF.data_ptr(), n_ch, sp))

        def run_b():
            check(lib.gsr_blend_splat_backward(*f.lists(o), F.data_ptr(), n_ch, n_ch, Gm.data_ptr(), gT.data_ptr(), 0.0, int(a.abs), gS.data_ptr(), sp))

        def zero():
            gF.zero_()
            gS.zero_()

        times, stats = ab.interleaved((("A", run_a), ("B", run_b)), a.rounds, "events", before=zero, stats=f.R.stats)
        wa, wb = width_of(n_ch, 8), width_of(n_ch, 4)
        lines.append(f"C = {n_ch}: A = gsr_blend_channels + gsr_blend_channels_backward (width {wa}), B = 1 x gsr_blend_splat_backward (width {wb})")
        med = {}
        for name in "AB":
            line, med[name] = ab.summary(name, times[name], stats[name])
            lines.append(line)
        issues_a, issues_b = (14 + wa) + (14 + 7 * wa), 2 * (14 + wb)
        lines.append(f"  B / A at the median: {med['B'] / med['A']:.3f}   counters agree: {ab.same_counters(stats, 'A', 'B', ab.COUNTERS + ('n_pairs',))}   "
                     f"issues per survivor: A {issues_a}, B {issues_b} "
                     f"+ about {8 + 8 * 9} where e != 0 ({issues_b / issues_a:.2f} .. {(issues_b + 80) / issues_a:.2f} of A)   "
                     f"rows touched {int((gS[:, 0] != 0).sum())} of {n}, finite {bool(torch.isfinite(gS).all())}")
        del F, Gm, gT, out, gF, gS
    ab.report(lines, a.out)


if __name__ == "__main__":
    ab.main(__file__, arguments(), worker)
