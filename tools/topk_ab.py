#!/usr/bin/env python3
"""A/B of the top-k kernels against the feature blend on the bench frame, interleaved rounds in ONE process (MI355X guide, rule 24).
Stages 1-2 run once, then per round, each between two events on the same lists:
  A  gsr_blend_features with features (z_cam, 1, 0): blend_kernel<FeatureBlend>, the yardstick
  B  gsr_blend_topk HEAVIEST k = 4,  no final T   (blend_topk_kernel<4, false>)
  C  gsr_blend_topk HEAVIEST k = 8,  no final T   (blend_topk_kernel<8, false>)
  D  gsr_blend_topk HEAVIEST k = 16, no final T   (blend_topk_kernel<16, false>)
  E  gsr_blend_topk HEAVIEST k = 8 with final T: walks like A
  F  gsr_blend_topk NEAREST  k = 4,  no final T   (blend_topk_kernel<4, true>)
Median, min, max and spread over the rounds, the ratios to A, each call's wave_entries / fetched_entries, and whether C's and E's
lists agree bit for bit.  Appends what it prints to profiles/topk_ab.txt (--out), under --label.
The form of the insertion without its wave-uniform guard is the analysis build of the library:
  make -C torch-gaussian-splatting-rasterizer_amd/csrc ../../tools/libgsr_topk_noguard.so
  GSR_LIB_PATH=tools/libgsr_topk_noguard.so tools/topk_ab.py --label "no guard"
usage: tools/topk_ab.py [--workload bicycle] [--rounds 30] [--early-out-T 0] [--label guarded]"""
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
from gsr_amd import _lib, renderer, utils
from gsr_amd._lib import check, lib

RUNS = {"B": (4, 0, False), "C": (8, 0, False), "D": (16, 0, False), "E": (8, 0, True), "F": (4, 1, False)}  # k, select, final T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bicycle")
    ap.add_argument("--gaussians", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--early-out-T", type=float, default=0.0)
    ap.add_argument("--camera", type=int, default=0)
    ap.add_argument("--camera-set", default="single")
    ap.add_argument("--label", default="guarded")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "topk_ab.txt"))
    a = ap.parse_args()
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
    feats = R._depth_features(cam)
    o = renderer.make_options(early_out_T=a.early_out_T, colour_stage=0)
    out_map = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    ids = {r: torch.empty((H, W, k), dtype=torch.int32, device=dev) for r, (k, _, _) in RUNS.items()}
    wts = {r: torch.empty((H, W, k), dtype=torch.float32, device=dev) for r, (k, _, _) in RUNS.items()}
    final_T = torch.empty((H, W), dtype=torch.float32, device=dev)
    wp, wn, mp = ws.data_ptr(), ws.numel(), R.max_pairs
    check(lib.gsr_preprocess(C.byref(sc), C.byref(cam), C.byref(o), wp, wn, None, sp))
    check(lib.gsr_bin_sort(n, C.byref(cam), C.byref(o), mp, wp, wn, sp))

    def run_a():
        check(lib.gsr_blend_features(n, C.byref(cam), C.byref(o), mp, wp, wn, feats.data_ptr(), out_map.data_ptr(), None, sp))

    def run_topk(r):
        k, select, with_T = RUNS[r]
        check(lib.gsr_blend_topk(n, C.byref(cam), C.byref(o), mp, wp, wn, k, select, ids[r].data_ptr(), wts[r].data_ptr(),
                                 final_T.data_ptr() if with_T else None, sp))

    runs = [("A", run_a)] + [(r, (lambda r=r: run_topk(r))) for r in RUNS]
    times, stats = {k: [] for k, _ in runs}, {}
    for rnd in range(a.rounds + 2):  # the first two rounds warm up (code objects, the launch-order hint)
        for name, run in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            run()
            e1.record(stream)
            torch.cuda.synchronize(dev)
            if rnd >= 2:
                times[name].append(e0.elapsed_time(e1))
            if rnd == 1:
                stats[name] = R.stats()
    lines = [f"[{a.label}] {os.path.basename(_lib.LIB_PATH)}  {a.workload}: {n} gaussians, {W}x{H}, {a.rounds} interleaved rounds after 2 warm-up "
             f"rounds (blend stage alone, tile-order kernel included), early_out_T {a.early_out_T}"]
    what = {"A": "gsr_blend_features (blend_kernel<FeatureBlend>)"}
    for r, (k, select, with_T) in RUNS.items():
        what[r] = f"gsr_blend_topk {'NEAREST' if select else 'HEAVIEST'} k = {k}{', with final T' if with_T else ''}"
    med = {}
    for name, _ in runs:
        t = np.array(times[name])
        med[name] = float(np.median(t))
        lines.append(f"  {name}: median {np.median(t):.4f} ms  min {t.min():.4f} ms  max {t.max():.4f} ms  spread (max - min) / median "
                     f"{(t.max() - t.min()) / np.median(t) * 100:.1f} %   wave_entries {stats[name]['wave_entries']} fetched_entries "
                     f"{stats[name]['fetched_entries']}   [{what[name]}]")
    lines.append("  ratios to A at the median: " + "   ".join(f"{r} / A {med[r] / med['A']:.3f}" for r in RUNS))
    lines.append("  wave_entries to A's: " + "   ".join(f"{r} {stats[r]['wave_entries'] / max(stats['A']['wave_entries'], 1):.3f}" for r in RUNS)
                 + f"   E's counters are A's: {all(stats['E'][k] == stats['A'][k] for k in ('wave_entries', 'fetched_entries'))}")
    filled = (ids["D"] >= 0).sum(-1)
    lines.append(f"  C's lists == E's: {torch.equal(ids['C'], ids['E']) and torch.equal(wts['C'], wts['E'])};  B's == the first 4 slots of C's: "
                 f"{torch.equal(ids['B'], ids['C'][..., :4]) and torch.equal(wts['B'], wts['C'][..., :4])};  filled slots per pixel at k = 16: "
                 f"mean {float(filled.float().mean()):.1f}, pixels with all 16 {int((filled == 16).sum())} of {W * H};  weight outside the "
                 f"8 heaviest, mean over pixels: {float((1.0 - final_T - wts['E'].sum(-1)).clamp(min=0).mean()):.4f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
