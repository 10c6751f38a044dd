#!/usr/bin/env python3
"""A/B of two (or more) BUILDS of libgsr.so on the bench frame, interleaved in ONE process on one GPU (MI355X guide, rule 24:
devices differ, so old / new / old / new on the same box): every round renders every variant with every build in turn, on one
shared workspace.  Per (variant, build): the three stage times (events around gsr_preprocess / gsr_bin_sort / gsr_blend; the
second of two back-to-back frames is the timed one) as median [min .. max] and the quartiles of the blend over the rounds,
the counters of a steady-state frame, and bit-identity of the frame with the first build's.
usage: tools/lib_ab.py [--rounds 30] --libs old=PATH,new=PATH VARIANT [VARIANT ...]     VARIANT = name[:field=value[,field=value]]
e.g.   tools/lib_ab.py --libs parent=tools/libgsr_parent.so,this=torch-gaussian-splatting-rasterizer_amd/csrc/libgsr.so \\
           default colour1:colour_stage=1 impl1:blend_impl=1 walk1:tile_row_step=4 walk1pipe:tile_row_step=8"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
import gsr_amd  # noqa: F401
from gsr_amd import _lib, renderer, utils
from gsr_amd._lib import check


def load(path):
    """A second copy of the library under another path is another library to the loader: its own code, its own state."""
    _lib.LIB_PATH = os.path.abspath(path)
    return _lib._load()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bicycle")
    ap.add_argument("--gaussians", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--camera", type=int, default=0)
    ap.add_argument("--camera-set", default="single")
    ap.add_argument("--libs", required=True, help="name=path[,name=path ...]: the builds, the first is the reference")
    ap.add_argument("variants", nargs="+")
    a = ap.parse_args()
    libs = [(k, load(p)) for k, p in (e.split("=", 1) for e in a.libs.split(","))]
    dev = torch.device("cuda", 0)
    cols, cam_list, n, W, H, _ = bench.build_workload(a.workload, a, a.gaussians)
    packed = utils.pack_gaussians(cols)
    del cols
    scene = renderer.GaussianScene.from_packed(packed, device=dev)
    del packed
    cam = renderer.make_camera(*cam_list[0])
    variants = []
    for v in a.variants:
        name, _, envs = v.partition(":")
        kw = {k: (float(v) if "." in v or "e" in v else int(v)) for k, v in (e.split("=") for e in envs.split(",") if e)}
        variants.append((name, renderer.make_options(**kw)))

    R = renderer.Rasterizer(scene)
    R.max_pairs = max(R.fit_pairs(cam, o) for _, o in variants)  # one pair buffer that fits every variant
    ws = R._workspace(W, H)
    sc = scene.c_struct()
    stream = torch.cuda.current_stream(dev)
    sp = int(stream.cuda_stream)
    keys = [(v, b) for v, _ in variants for b, _ in libs]
    outs = {k: torch.zeros((H, W, 3), dtype=torch.float32, device=dev) for k in keys}
    times = {k: [] for k in keys}
    stats = {}
    for rnd in range(a.rounds + 2):
        for name, o in variants:
            opts = R.bounded(o)
            for build, L in libs:
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                for _ in range(2):  # the second repetition is the timed one (same variant and build back to back)
                    ev[0].record(stream)
                    check(L.gsr_preprocess(C.byref(sc), C.byref(cam), C.byref(opts), ws.data_ptr(), ws.numel(), None, sp))
                    ev[1].record(stream)
                    check(L.gsr_bin_sort(n, C.byref(cam), C.byref(opts), R.max_pairs, ws.data_ptr(), ws.numel(), sp))
                    ev[2].record(stream)
                    check(L.gsr_blend(None, n, C.byref(cam), C.byref(opts), R.max_pairs, ws.data_ptr(), ws.numel(), outs[(name, build)].data_ptr(), None, sp))
                    ev[3].record(stream)
                torch.cuda.synchronize(dev)
                if rnd >= 2:
                    times[(name, build)].append([ev[k].elapsed_time(ev[k + 1]) for k in range(3)])
                if rnd == 1:
                    stats[(name, build)] = R.stats()
    print(f"{a.workload}, {n} gaussians, {W}x{H}, {a.rounds} interleaved rounds; ms: median [min .. max]; blend quartiles q1-q3", flush=True)
    ref = libs[0][0]
    for name, _ in variants:
        for build, _ in libs:
            t = np.array(times[(name, build)])
            fr = t.sum(axis=1)
            b = t[:, 2]
            s = stats[(name, build)]
            bs = t[:, 1]
            print(f"{name:10s} {build:8s} preprocess {np.median(t[:, 0]):.4f}  bin_sort {np.median(bs):.4f} [{bs.min():.4f} .. {bs.max():.4f}]  "
                  f"blend {np.median(b):.4f} [{b.min():.4f} .. {b.max():.4f}] q {np.percentile(b, 25):.4f}-{np.percentile(b, 75):.4f}  "
                  f"frame {np.median(fr):.4f} [{fr.min():.4f} .. {fr.max():.4f}]   == {ref}: {bool(torch.equal(outs[(name, build)], outs[(name, ref)]))}  "
                  f"E {s['n_pairs']} fetched {s['fetched_entries']} evaluated {s['wave_entries']} colour_evals {s['colour_evals']}", flush=True)
        for build, _ in libs[1:]:  # the same for the stage the depth sort and the binning live in
            d = np.array(times[(name, build)])[:, 1] - np.array(times[(name, ref)])[:, 1]
            print(f"{name:10s} bin_sort {build} - {ref}: median {np.median(d):+.4f} ms  [{d.min():+.4f} .. {d.max():+.4f}]  "
                  f"{int((d < 0).sum())} of {len(d)} rounds faster", flush=True)
        if len(libs) == 2:  # paired differences round by round: the spread of the DIFFERENCE is what a gain is held against
            d = np.array(times[(name, libs[1][0])])[:, 2] - np.array(times[(name, libs[0][0])])[:, 2]
            print(f"{name:10s} blend {libs[1][0]} - {libs[0][0]}: median {np.median(d):+.4f} ms  [{d.min():+.4f} .. {d.max():+.4f}]  "
                  f"{int((d < 0).sum())} of {len(d)} rounds faster", flush=True)


if __name__ == "__main__":
    main()
