#!/usr/bin/env python3
"""The splat gradient against the two walks it is made of, on the bench frame, interleaved rounds in ONE process.
Stages 1-2 run once (colour_stage = 0), then per round and per channel count C:
  A  gsr_blend_channels on an [n, C] array + gsr_blend_channels_backward of an [H, W, C] upstream gradient: a forward walk and a
     walk with the DPP reduction and the atomic flush, the two things the new kernel does in its two passes
  B  ONE gsr_blend_splat_backward of the same features and upstream gradient, with grad_T, into an [n, 8] array (zeroed outside
     the timed span)
each between two events — median and min over rounds, the spread, B / A and both sides' counters (they must agree: the second pass
walks the forward's lists with the forward's stop rule).  No ratio is fixed in advance.  What to compare with is the issue count per
survivor: A = (14 + CH) + (14 + 7 CH) with CH the instantiated width, B = 2 (14 + CH) for the two walks plus, for a survivor with a
nonzero e in some pixel, 8 products and 8 x 9 reduction issues (six DPP adds a value, lane 63's LDS add, the ballot and e itself).
Writes what it prints to profiles/splat_gradient_ab.txt (--out).
usage: tools/splat_gradient_ab.py [--workload bicycle] [--rounds 15] [--channels 3,16] [--early-out-T 0] [--abs]"""
import argparse
import ctypes as C
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch

import bench
import gsr_amd  # noqa: F401
from gsr_amd import renderer, utils
from gsr_amd._lib import check, lib


def width_of(n_ch, min_width):
    return 16 if n_ch > 8 else 8 if n_ch > 4 or min_width > 4 else 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bicycle")
    ap.add_argument("--gaussians", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--channels", default="3,16")
    ap.add_argument("--early-out-T", type=float, default=0.0)
    ap.add_argument("--abs", action="store_true", help="B with want_abs")
    ap.add_argument("--camera", type=int, default=0)
    ap.add_argument("--camera-set", default="single")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "splat_gradient_ab.txt"))
    a = ap.parse_args()
    counts = [int(x) for x in a.channels.split(",")]
    dev = torch.device("cuda", 0)
    cols, cam_list, n, W, H, _ = bench.build_workload(a.workload, a, a.gaussians)
    scene = renderer.GaussianScene.from_packed(utils.pack_gaussians(cols), device=dev)
    del cols
    cam = renderer.make_camera(*cam_list[0])
    R = renderer.Rasterizer(scene)
    R.fit_pairs(cam)
    ws = R._workspace(W, H)
    sc = scene.c_struct()
    stream = torch.cuda.current_stream(dev)
    sp = int(stream.cuda_stream)
    o = renderer.make_options(early_out_T=a.early_out_T, colour_stage=0)
    wp, wn, mp = ws.data_ptr(), ws.numel(), R.max_pairs
    check(lib.gsr_preprocess(C.byref(sc), C.byref(cam), C.byref(o), wp, wn, None, sp))
    check(lib.gsr_bin_sort(n, C.byref(cam), C.byref(o), mp, wp, wn, sp))

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"{a.workload}: {n} gaussians, {W}x{H}, {a.rounds} interleaved rounds after 2 of warm-up (stage 3 alone, its tile-order kernel "
        f"included; early_out_T = {a.early_out_T}; want_abs = {int(a.abs)})")
    gen = torch.Generator().manual_seed(1)
    for n_ch in counts:
        F = torch.randn((n, n_ch), generator=gen).to(dev)
        Gm = torch.randn((H, W, n_ch), generator=gen).to(dev)
        gT = torch.randn((H, W), generator=gen).to(dev)
        out = torch.empty((H, W, n_ch), dtype=torch.float32, device=dev)
        gF = torch.zeros((n, n_ch), dtype=torch.float32, device=dev)
        gS = torch.zeros((n, 8), dtype=torch.float32, device=dev)

        def run_a():
            check(lib.gsr_blend_channels(n, C.byref(cam), C.byref(o), mp, wp, wn, F.data_ptr(), n_ch, n_ch, out.data_ptr(), None, sp))
            check(lib.gsr_blend_channels_backward(n, C.byref(cam), C.byref(o), mp, wp, wn, Gm.data_ptr(), n_ch, gF.data_ptr(), n_ch, sp))

        def run_b():
            check(lib.gsr_blend_splat_backward(n, C.byref(cam), C.byref(o), mp, wp, wn, F.data_ptr(), n_ch, n_ch, Gm.data_ptr(),
                                               gT.data_ptr(), 0.0, int(a.abs), gS.data_ptr(), sp))

        times, stats = {"A": [], "B": []}, {}
        for rnd in range(a.rounds + 2):  # the first two rounds warm up (code objects)
            for name, run in (("A", run_a), ("B", run_b)):
                gF.zero_()
                gS.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                run()
                e1.record(stream)
                torch.cuda.synchronize(dev)
                if rnd >= 2:
                    times[name].append(e0.elapsed_time(e1))
                if rnd == 1:
                    stats[name] = R.stats()
        wa, wb = width_of(n_ch, 8), width_of(n_ch, 4)
        say(f"C = {n_ch}: A = gsr_blend_channels + gsr_blend_channels_backward (width {wa}), B = 1 x gsr_blend_splat_backward (width {wb})")
        med = {}
        for name in ("A", "B"):
            t = np.array(times[name])
            med[name] = float(np.median(t))
            spread = float(t.max() - t.min())
            say(f"  {name}: median {med[name]:.4f} ms  min {t.min():.4f} ms  max {t.max():.4f} ms  spread (max - min) {spread:.4f} ms = "
                f"{spread / med[name] * 100:.1f} %   wave_entries {stats[name]['wave_entries']} fetched_entries {stats[name]['fetched_entries']}")
        same = all(stats["A"][k] == stats["B"][k] for k in ("wave_entries", "fetched_entries", "n_pairs"))
        issues_a, issues_b = (14 + wa) + (14 + 7 * wa), 2 * (14 + wb)
        say(f"  B / A at the median: {med['B'] / med['A']:.3f}   counters agree: {same}   issues per survivor: A {issues_a}, B {issues_b} "
            f"+ about {8 + 8 * 9} where e != 0 ({issues_b / issues_a:.2f} .. {(issues_b + 80) / issues_a:.2f} of A)   "
            f"rows touched {int((gS[:, 0] != 0).sum())} of {n}, finite {bool(torch.isfinite(gS).all())}")
        del F, Gm, gT, out, gF, gS
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
