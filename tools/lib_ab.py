#!/usr/bin/env python3
"""A/B of two (or more) BUILDS of libgsr.so on the bench frame, interleaved in ONE process on one GPU (MI355X guide, rule 24:
devices differ, so old / new / old / new on the same box): every round renders every variant with every build in turn, on one
shared workspace.  Per (variant, build): the three stage times (events around gsr_preprocess / gsr_bin_sort / gsr_blend; the
second of two back-to-back frames is the timed one) as median [min .. max] and the quartiles of the blend over the rounds,
the counters of a steady-state frame, and bit-identity of the frame with the first build's.
Prints only, unless --out names a file.  The measurement runs in a child process under a time limit (--timeout seconds;
tools/ab_harness.py).
usage: tools/lib_ab.py [--rounds 30] [--timeout 900] --libs old=PATH,new=PATH VARIANT [VARIANT ...]     VARIANT = name[:field=value[,field=value]]
e.g.   tools/lib_ab.py --libs parent=tools/libgsr_parent.so,this=torch-gaussian-splatting-rasterizer_amd/csrc/libgsr.so \\
           default colour1:colour_stage=1 impl1:blend_impl=1 walk1:tile_row_step=4 walk1pipe:tile_row_step=8"""
import os

import ab_harness as ab


def flags(ap):
    ap.add_argument("--libs", required=True, help="name=path[,name=path ...]: the builds, the first is the reference")
    ap.add_argument("variants", nargs="+")


def arguments(argv=None):
    return ab.arguments("lib_ab", rounds=30, timeout=900, writes=False, extra=flags, argv=argv)


def load(path):
    """A second copy of the library under another path is another library to the loader: its own code, its own state."""
    from gsr_amd import _lib

    _lib.LIB_PATH = os.path.abspath(path)
    return _lib._load()


def worker(a):
    import numpy as np
    import torch

    import gsr_amd  # noqa: F401

    libs = [(k, load(p)) for k, p in (e.split("=", 1) for e in a.libs.split(","))]
    variants = ab.variants(a)
    f = ab.bench_frame(a, fit=[o for _, o in variants])  # one pair buffer that fits every variant
    keys = [(v, b) for v, _ in variants for b, _ in libs]
    outs = {k: torch.zeros((f.H, f.W, 3), dtype=torch.float32, device=f.dev) for k in keys}
    legs = [((name, build), f.stages(L, f.R.bounded(o), outs[name, build])) for name, o in variants for build, L in libs]
    times, stats = ab.interleaved(legs, a.rounds, "stages", stats=f.R.stats)
    lines = [f"{a.workload}, {f.n} gaussians, {f.W}x{f.H}, {a.rounds} interleaved rounds; ms: median [min .. max]; blend quartiles q1-q3"]
    ref = libs[0][0]
    span = "%.4f [%.4f .. %.4f]"
    for name, _ in variants:
        for build, _ in libs:
            t = np.array(times[name, build])
            b, s = t[:, 2], stats[name, build]
            lines.append(f"{name:10s} {build:8s} preprocess {ab.spans(t[:, 0])[0]:.4f}  bin_sort {span % ab.spans(t[:, 1])}  "
                         f"blend {span % ab.spans(b)} q {np.percentile(b, 25):.4f}-{np.percentile(b, 75):.4f}  "
                         f"frame {span % ab.spans(t.sum(axis=1))}   == {ref}: {bool(torch.equal(outs[name, build], outs[name, ref]))}  "
                         f"E {s['n_pairs']} fetched {s['fetched_entries']} evaluated {s['wave_entries']} colour_evals {s['colour_evals']}")
        # paired differences round by round, the spread of the DIFFERENCE being what a gain is held against: for the stage the depth
        # sort and the binning live in and, between two builds, for the blend
        for stage, k, builds in (("bin_sort", 1, libs[1:]), ("blend", 2, libs[1:] if len(libs) == 2 else [])):
            for build, _ in builds:
                d = np.array(times[name, build])[:, k] - np.array(times[name, ref])[:, k]
                lines.append(f"{name:10s} {stage} {build} - {ref}: median {ab.spans(d)[0]:+.4f} ms  [{d.min():+.4f} .. {d.max():+.4f}]  "
                             f"{int((d < 0).sum())} of {len(d)} rounds faster")
    ab.report(lines, a.out)


if __name__ == "__main__":
    ab.main(__file__, arguments(), worker)
