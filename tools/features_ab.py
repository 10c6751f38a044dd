#!/usr/bin/env python3
"""A/B of the feature blend against the plain colour blend doing the same work, on the bench frame, interleaved rounds in ONE
process (MI355X guide, rule 24).  Stages 1-2 run once (colour_stage = 1: every record carries its colour), then per round:
  A  gsr_blend with blend_impl = 1, saturation_rule = 1: blend_kernel, the plain-C kernel — same entries, same T == 0 stop rule,
     same blend_one, colours read from the record
  B  gsr_blend_features with features (z_cam, 1, 0): the same kernel under the feature policy
each between two events — median and min over rounds, the spread, B / A, and the two blends' counters (they must agree).
Then whole calls, synchronised: Rasterizer.render against render_depth and render_rgbd in ms per frame.
usage: tools/features_ab.py [--workload bicycle] [--rounds 15] [--early-out-T 0]"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
    ap.add_argument("--early-out-T", type=float, default=0.0)
    ap.add_argument("--camera", type=int, default=0)
    ap.add_argument("--camera-set", default="single")
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
    oA = renderer.make_options(early_out_T=a.early_out_T, blend_impl=1, saturation_rule=1, colour_stage=1)
    oB = renderer.make_options(early_out_T=a.early_out_T, colour_stage=1)
    outA = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    outB = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    TB = torch.empty((H, W), dtype=torch.float32, device=dev)
    check(lib.gsr_preprocess(C.byref(sc), C.byref(cam), C.byref(oA), ws.data_ptr(), ws.numel(), None, sp))
    check(lib.gsr_bin_sort(n, C.byref(cam), C.byref(oA), R.max_pairs, ws.data_ptr(), ws.numel(), sp))

    def run_a():
        check(lib.gsr_blend(None, n, C.byref(cam), C.byref(oA), R.max_pairs, ws.data_ptr(), ws.numel(), outA.data_ptr(), None, sp))

    def run_b():
        check(lib.gsr_blend_features(n, C.byref(cam), C.byref(oB), R.max_pairs, ws.data_ptr(), ws.numel(), feats.data_ptr(), outB.data_ptr(), None, sp))

    times, stats = {"A": [], "B": []}, {}
    for rnd in range(a.rounds + 2):  # the first two rounds warm up (code objects, the launch-order hint)
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
    print(f"{a.workload}: {n} gaussians, {W}x{H}, {a.rounds} interleaved rounds (blend stage alone, tile-order kernel included)")
    med = {}
    for name, what in (("A", "gsr_blend, blend_impl=1 saturation_rule=1 (blend_kernel)"), ("B", "gsr_blend_features (blend_kernel<FeatureBlend>)")):
        t = np.array(times[name])
        med[name] = float(np.median(t))
        print(f"  {name}: median {np.median(t):.4f} ms  min {t.min():.4f} ms  max {t.max():.4f} ms  spread (max - min) / median {(t.max() - t.min()) / np.median(t) * 100:.1f} %"
              f"   wave_entries {stats[name]['wave_entries']} fetched_entries {stats[name]['fetched_entries']} colour_evals {stats[name]['colour_evals']}   [{what}]")
    same = all(stats["A"][k] == stats["B"][k] for k in ("wave_entries", "fetched_entries", "n_pairs"))
    print(f"  B / A at the median: {med['B'] / med['A']:.3f}   counters agree: {same}")
    # the final T of B against A's blend asked for its T (the colour frame itself differs: other features)
    TA = torch.empty((H, W), dtype=torch.float32, device=dev)
    check(lib.gsr_blend(None, n, C.byref(cam), C.byref(oA), R.max_pairs, ws.data_ptr(), ws.numel(), outA.data_ptr(), TA.data_ptr(), sp))
    check(lib.gsr_blend_features(n, C.byref(cam), C.byref(oB), R.max_pairs, ws.data_ptr(), ws.numel(), feats.data_ptr(), outB.data_ptr(), TB.data_ptr(), sp))
    torch.cuda.synchronize(dev)
    print(f"  final T of B == final T of A: {bool(torch.equal(TA, TB))};  max |alpha - (1 - T)| {float((outB[..., 1] - (1 - TB)).abs().max()):.2e};  "
          f"depth map max {float(outB[..., 0].max()):.3f}")

    # whole calls (checked frames: each ends with the counters' read-back), ms per frame
    calls = {"render": lambda: R.render(cam), "render_depth": lambda: R.render_depth(cam), "render_rgbd": lambda: R.render_rgbd(cam)}
    per = {k: [] for k in calls}
    for rnd in range(a.rounds + 2):
        for k, f in calls.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize(dev)
            if rnd >= 2:
                per[k].append((time.perf_counter() - t0) * 1e3)
    for k in calls:
        t = np.array(per[k])
        print(f"  {k}: median {np.median(t):.3f} ms per frame  min {t.min():.3f} ms")


if __name__ == "__main__":
    main()
