#!/usr/bin/env python3
"""A/B of whole-frame variants selected by GsrOptions fields (e.g. fine_binning=1, saturation_rule=1, colour_stage=1),
interleaved rounds in ONE process (MI355X guide, rule 24): per variant the three stage times (events around gsr_preprocess /
gsr_bin_sort / gsr_blend; the second of two back-to-back frames is the timed one), median over rounds, plus bit-identity of the
frames.  Prints only, unless --out names a file.  The measurement runs in a child process under a time limit (--timeout seconds;
tools/ab_harness.py).
usage: tools/frame_ab.py [--workload bicycle] [--rounds 12] [--early-out-T 0] [--timeout 600] VARIANT [VARIANT ...]
VARIANT = name[:field=value[,field=value]]     (GSR_MORTON=0: the scene in file order instead of the loaders' Morton order)"""
import os

import ab_harness as ab


def arguments(argv=None):
    return ab.arguments("frame_ab", rounds=12, timeout=600, writes=False, extra=lambda ap: ap.add_argument("variants", nargs="+"), argv=argv)


def worker(a):
    import torch

    import gsr_amd  # noqa: F401
    from gsr_amd._lib import lib

    variants = ab.variants(a)
    # one pair buffer that fits every variant (GSR_MORTON: A/B of the loader option)
    f = ab.bench_frame(a, fit=[o for _, o in variants], spatial_order=os.environ.get("GSR_MORTON", "1") == "1")
    outs = {name: torch.empty((f.H, f.W, 3), dtype=torch.float32, device=f.dev) for name, _ in variants}
    legs = [(name, f.stages(lib, f.R.bounded(o), outs[name])) for name, o in variants]
    times, stats = ab.interleaved(legs, a.rounds, "stages", stats=f.R.stats)
    ref, lines = variants[0][0], []
    for name, _ in variants:
        t = [ab.spans(ab.column(times[name], k))[0] for k in range(3)]
        lines.append(f"{name:14s} preprocess {t[0]:.4f}  bin_sort {t[1]:.4f}  blend {t[2]:.4f}  frame {sum(t):.4f} ms   == {ref}: {bool(torch.equal(outs[name], outs[ref]))}  "
                     f"D {stats[name]['n_pairs_bbox']} E {stats[name]['n_pairs']} fetched {stats[name]['fetched_entries']} evaluated {stats[name]['wave_entries']}")
    ab.report(lines, a.out)


if __name__ == "__main__":
    ab.main(__file__, arguments(), worker)
