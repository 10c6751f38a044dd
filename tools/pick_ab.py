#!/usr/bin/env python3
"""A/B of the pick kernel against the feature blend on the bench frame, interleaved rounds in ONE process (MI355X guide, rule 24).
Stages 1-2 run once, then per round, each between two events on the same lists:
  A  gsr_blend_features with features (z_cam, 1, 0): blend_kernel<FeatureBlend>, the baseline
  B  gsr_blend_pick without a count: blend_pick_kernel<false>, which stops once neither id can change
  C  gsr_blend_pick with the count: blend_pick_kernel<true>, which walks to T == 0 like A
Median, min, max and spread over the rounds, B / A and C / A, each call's wave_entries / fetched_entries, and whether B's and C's
ids and weights agree bit for bit.  Writes what it prints to profiles/pick_ab.txt (--out).
usage: tools/pick_ab.py [--workload bicycle] [--rounds 30] [--early-out-T 0] [--median-T 0.5]"""
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
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--early-out-T", type=float, default=0.0)
    ap.add_argument("--median-T", type=float, default=0.5)
    ap.add_argument("--camera", type=int, default=0)
    ap.add_argument("--camera-set", default="single")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pick_ab.txt"))
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
    ids = {k: [torch.empty((H, W), dtype=torch.int32, device=dev) for _ in range(3)] for k in "BC"}
    wts = {k: torch.empty((H, W), dtype=torch.float32, device=dev) for k in "BC"}
    wp, wn, mp = ws.data_ptr(), ws.numel(), R.max_pairs
    check(lib.gsr_preprocess(C.byref(sc), C.byref(cam), C.byref(o), wp, wn, None, sp))
    check(lib.gsr_bin_sort(n, C.byref(cam), C.byref(o), mp, wp, wn, sp))

    def run_a():
        check(lib.gsr_blend_features(n, C.byref(cam), C.byref(o), mp, wp, wn, feats.data_ptr(), out_map.data_ptr(), None, sp))

    def run_pick(k):
        best, med, cnt = ids[k]
        check(lib.gsr_blend_pick(n, C.byref(cam), C.byref(o), mp, wp, wn, a.median_T, best.data_ptr(), wts[k].data_ptr(), med.data_ptr(),
                                 cnt.data_ptr() if k == "C" else None, sp))

    runs = (("A", run_a), ("B", lambda: run_pick("B")), ("C", lambda: run_pick("C")))
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
    lines = [f"{a.workload}: {n} gaussians, {W}x{H}, {a.rounds} interleaved rounds after 2 warm-up rounds (blend stage alone, tile-order kernel "
             f"included), early_out_T {a.early_out_T}, median_T {a.median_T}"]
    med = {}
    what = {"A": "gsr_blend_features (blend_kernel<FeatureBlend>)", "B": "gsr_blend_pick, count = NULL (blend_pick_kernel<false>)",
            "C": "gsr_blend_pick with count (blend_pick_kernel<true>)"}
    for name, _ in runs:
        t = np.array(times[name])
        med[name] = float(np.median(t))
        lines.append(f"  {name}: median {np.median(t):.4f} ms  min {t.min():.4f} ms  max {t.max():.4f} ms  spread (max - min) / median "
                     f"{(t.max() - t.min()) / np.median(t) * 100:.1f} %   wave_entries {stats[name]['wave_entries']} fetched_entries "
                     f"{stats[name]['fetched_entries']} colour_evals {stats[name]['colour_evals']}   [{what[name]}]")
    same_ids = all(torch.equal(x, y) for x, y in zip(ids["B"][:2], ids["C"][:2])) and torch.equal(wts["B"], wts["C"])
    lines.append(f"  B / A at the median: {med['B'] / med['A']:.3f}   C / A: {med['C'] / med['A']:.3f}   B's median <= A's: {med['B'] <= med['A']}")
    lines.append(f"  wave_entries B / A: {stats['B']['wave_entries'] / max(stats['A']['wave_entries'], 1):.3f}   fetched_entries B / A: "
                 f"{stats['B']['fetched_entries'] / max(stats['A']['fetched_entries'], 1):.3f}   C's counters are A's: "
                 f"{all(stats['C'][k] == stats['A'][k] for k in ('wave_entries', 'fetched_entries'))}")
    lines.append(f"  B's ids and weights == C's: {same_ids};  pixels with a dominant gaussian {int((ids['C'][0] >= 0).sum())} of {W * H}, with a "
                 f"median {int((ids['C'][1] >= 0).sum())}, contributors per pixel: mean {float(ids['C'][2].float().mean()):.1f} max {int(ids['C'][2].max())}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
