#!/usr/bin/env python3
"""A/B of blend kernel variants on the bench frame, interleaved rounds in ONE process (MI355X guide, rule 24):
per variant the blend stage alone (gsr_blend between two events) — median, min, max and spread over the rounds — plus bit-identity
of the frames and the counters.  Prints only, unless --out names a file.  The measurement runs in a child process under a time
limit (--timeout seconds; tools/ab_harness.py).
usage: tools/blend_ab.py [--workload bicycle] [--impls 0,1] [--rounds 15] [--early-out-T 0] [--tile-row-step 1,4,8] [--timeout 420]
--tile-row-step G blends shard 0 of G (bicycle: G = 4 is 2040 tiles, the one-quadrant walk; G = 8 is 1020, the pipelined one)."""
import ab_harness as ab


def flags(ap):
    ap.add_argument("--impls", default="0,1")
    ap.add_argument("--tile-row-step", default="1", help="comma list: each G blends tile rows 0, G, 2G, ... (a multi-GPU rank's shard)")


def arguments(argv=None):
    return ab.arguments("blend_ab", writes=False, extra=flags, argv=argv)


def worker(a):
    import torch

    f = ab.bench_frame(a)
    from gsr_amd import renderer
    from gsr_amd._lib import check, lib

    impls = [int(x) for x in a.impls.split(",")]
    lines = []
    for step in [int(x) for x in a.tile_row_step.split(",")]:
        outs = {i: torch.zeros((f.H, f.W, 3), dtype=torch.float32, device=f.dev) for i in impls}
        f.make_lists(renderer.make_options(early_out_T=a.early_out_T, tile_row_step=step))

        opts = {i: renderer.make_options(early_out_T=a.early_out_T, blend_impl=i, tile_row_step=step) for i in impls}

        def run(i):
            check(lib.gsr_blend(None, *f.lists(opts[i]), outs[i].data_ptr(), None, f.sp))

        times, stats = ab.interleaved([(i, (lambda i=i: run(i))) for i in impls], a.rounds, "events", stats=f.R.stats)
        ref = impls[0]
        for i in impls:
            same, d = bool(torch.equal(outs[i], outs[ref])), float((outs[i] - outs[ref]).abs().max())
            lines.append(ab.summary(f"rows 0/{step} impl {i}", times[i], stats[i], f"frame == impl {ref}: {same} (max abs diff {d:.2e})")[0])
    ab.report(lines, a.out)


if __name__ == "__main__":
    ab.main(__file__, arguments(), worker)
