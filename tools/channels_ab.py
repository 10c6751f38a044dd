#!/usr/bin/env python3
"""A/B of many channels per walk against three per walk, on the bench frame, interleaved rounds in ONE process.
Stages 1-2 run once (colour_stage = 0), then per round and per channel count C:
  A  ceil(C / 3) calls of gsr_blend_features on pre-sliced contiguous [n, 3] arrays (the last zero-padded): the three-channel
     kernel, what Rasterizer.render_features did for C > 3 before gsr_blend_channels existed — without its slicing copies
  B  ONE gsr_blend_channels on the [n, C] array: walks of up to 16 channels
each between two events — median and min over rounds, the spread, B / A, both sides' counters (they must agree) and whether the
maps agree bit for bit.  B counts as faster for a C when its median is below A's by more than A's own round-to-round spread.
Writes what it prints to profiles/channels_ab.txt (--out).
usage: tools/channels_ab.py [--workload bicycle] [--rounds 15] [--channels 8,16,32] [--early-out-T 0]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bicycle")
    ap.add_argument("--gaussians", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--channels", default="8,16,32")
    ap.add_argument("--early-out-T", type=float, default=0.0)
    ap.add_argument("--camera", type=int, default=0)
    ap.add_argument("--camera-set", default="single")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "channels_ab.txt"))
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
        groups = []
        for c0 in range(0, n_ch, 3):
            g = torch.zeros((n, 3), dtype=torch.float32, device=dev)
            g[:, :min(3, n_ch - c0)] = F[:, c0:c0 + 3]
            groups.append(g)
        outA = [torch.empty((H, W, 3), dtype=torch.float32, device=dev) for _ in groups]
        outB = torch.empty((H, W, n_ch), dtype=torch.float32, device=dev)

        def run_a():
            for g, m in zip(groups, outA):
                check(lib.gsr_blend_features(n, C.byref(cam), C.byref(o), mp, wp, wn, g.data_ptr(), m.data_ptr(), None, sp))

        def run_b():
            check(lib.gsr_blend_channels(n, C.byref(cam), C.byref(o), mp, wp, wn, F.data_ptr(), n_ch, n_ch, outB.data_ptr(), None, sp))

        times, stats = {"A": [], "B": []}, {}
        for rnd in range(a.rounds + 2):  # the first two rounds warm up (code objects)
            for name, run in (("A", run_a), ("B", run_b)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                run()
                e1.record(stream)
                torch.cuda.synchronize(dev)
                if rnd >= 2:
                    times[name].append(e0.elapsed_time(e1))
                if rnd == 1:
                    stats[name] = R.stats()
        same_bits = bool(torch.equal(torch.cat(outA, -1)[..., :n_ch], outB))
        say(f"C = {n_ch}: A = {len(groups)} x gsr_blend_features, B = 1 x gsr_blend_channels")
        med, spread = {}, {}
        for name in ("A", "B"):
            t = np.array(times[name])
            med[name], spread[name] = float(np.median(t)), float(t.max() - t.min())
            say(f"  {name}: median {med[name]:.4f} ms  min {t.min():.4f} ms  max {t.max():.4f} ms  spread (max - min) {spread[name]:.4f} ms = "
                f"{spread[name] / med[name] * 100:.1f} %   wave_entries {stats[name]['wave_entries']} fetched_entries {stats[name]['fetched_entries']}")
        same = all(stats["A"][k] == stats["B"][k] for k in ("wave_entries", "fetched_entries", "n_pairs"))
        say(f"  B / A at the median: {med['B'] / med['A']:.3f}   B faster by more than A's spread: {med['B'] < med['A'] - spread['A']}   "
            f"counters agree: {same}   maps agree bit for bit: {same_bits}")
        del F, groups, outA, outB
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
