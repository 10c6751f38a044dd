#!/usr/bin/env python3
"""The channel blend's transpose against the channel blend itself, on the bench frame, interleaved rounds in ONE process.
Stages 1-2 run once (colour_stage = 0), then per round and per channel count C:
  A  ONE gsr_blend_channels on an [n, C] array: the forward, walks of up to 16 channels
  B  ONE gsr_blend_channels_backward of an [H, W, C] upstream gradient into an [n, C] array (zeroed outside the timed span)
each between two events — median and min over rounds, the spread, B / A and both sides' counters (they must agree: the backward
walks the forward's lists with the forward's stop rule).  No ratio is fixed in advance; what to compare with is the issue count of
the DPP reduction, (14 + 7 CH) / (14 + CH) = 4.2 at CH = 16, and the atomic floor: fetched_entries x nch x 4 B of float adds per
walk at the chip-wide rate of 1.3 TB/s (an upper bound on the bytes: rows no wave touched are not flushed).
Writes what it prints to profiles/channels_backward_ab.txt (--out).
usage: tools/channels_backward_ab.py [--workload bicycle] [--rounds 15] [--channels 8,16,32] [--early-out-T 0]"""
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

ATOMIC_RATE = 1.3e12  # bytes of float adds per second, chip-wide


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bicycle")
    ap.add_argument("--gaussians", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--channels", default="8,16,32")
    ap.add_argument("--early-out-T", type=float, default=0.0)
    ap.add_argument("--camera", type=int, default=0)
    ap.add_argument("--camera-set", default="single")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "channels_backward_ab.txt"))
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
        f"included; early_out_T = {a.early_out_T})")
    gen = torch.Generator().manual_seed(1)
    for n_ch in counts:
        F = torch.randn((n, n_ch), generator=gen).to(dev)
        Gm = torch.randn((H, W, n_ch), generator=gen).to(dev)
        out = torch.empty((H, W, n_ch), dtype=torch.float32, device=dev)
        gF = torch.zeros((n, n_ch), dtype=torch.float32, device=dev)

        def run_a():
            check(lib.gsr_blend_channels(n, C.byref(cam), C.byref(o), mp, wp, wn, F.data_ptr(), n_ch, n_ch, out.data_ptr(), None, sp))

        def run_b():
            check(lib.gsr_blend_channels_backward(n, C.byref(cam), C.byref(o), mp, wp, wn, Gm.data_ptr(), n_ch, gF.data_ptr(), n_ch, sp))

        times, stats = {"A": [], "B": []}, {}
        for rnd in range(a.rounds + 2):  # the first two rounds warm up (code objects)
            for name, run in (("A", run_a), ("B", run_b)):
                gF.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                run()
                e1.record(stream)
                torch.cuda.synchronize(dev)
                if rnd >= 2:
                    times[name].append(e0.elapsed_time(e1))
                if rnd == 1:
                    stats[name] = R.stats()
        # <A F, G> = <F, A^T G>: the run timed last is the transpose of the forward timed last
        lhs, rhs = float((out.double() * Gm.double()).sum()), float((F.double() * gF.double()).sum())
        say(f"C = {n_ch}: A = 1 x gsr_blend_channels, B = 1 x gsr_blend_channels_backward")
        med, spread = {}, {}
        for name in ("A", "B"):
            t = np.array(times[name])
            med[name], spread[name] = float(np.median(t)), float(t.max() - t.min())
            say(f"  {name}: median {med[name]:.4f} ms  min {t.min():.4f} ms  max {t.max():.4f} ms  spread (max - min) {spread[name]:.4f} ms = "
                f"{spread[name] / med[name] * 100:.1f} %   wave_entries {stats[name]['wave_entries']} fetched_entries {stats[name]['fetched_entries']}")
        same = all(stats["A"][k] == stats["B"][k] for k in ("wave_entries", "fetched_entries", "n_pairs"))
        floor_ms = stats["B"]["fetched_entries"] * n_ch * 4 / ATOMIC_RATE * 1e3
        say(f"  B / A at the median: {med['B'] / med['A']:.3f}   counters agree: {same}   atomic floor (fetched_entries x {n_ch} x 4 B / 1.3 TB/s): "
            f"{floor_ms:.4f} ms = {floor_ms / med['B'] * 100:.1f} % of B   <AF,G> {lhs:.9g} <F,AtG> {rhs:.9g}")
        del F, Gm, out, gF
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
