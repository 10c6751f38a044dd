#!/usr/bin/env python3
"""A/B of the depth-bounded blend against the channel blend on the bench frame, interleaved rounds in ONE process (MI355X guide,
rule 24).  Stages 1-2 run once, then per round, each between two events on the same lists:
  A   gsr_blend_channels, 3 channels (z_cam, 1, 0): blend_channels_kernel<8>, the yardstick
  A8  gsr_blend_channels, 8 channels: the same kernel with every channel in use (B8's peer)
  B4  gsr_blend_slab, 3 channels, both limits NULL: blend_slab_kernel<4> — what the test and the narrower walk cost
  B8  gsr_blend_slab, 8 channels, both limits NULL: blend_slab_kernel<8>
  A16 / B16  the same pair at 16 channels: blend_channels_kernel<16> and blend_slab_kernel<16>, the width that always compares
  C   gsr_blend_slab, 3 channels, far = 1.05 x render_median_depth where a surface was found, +inf elsewhere: the stop rule
  D   gsr_blend_slab, 3 channels, near = that plane (-inf where no surface was found): the skip
Median, min, max and spread over the rounds, the ratios to A, each call's wave_entries / fetched_entries, and whether B's maps are
A's bit for bit.  Appends what it prints to profiles/slab_ab.txt (--out), under --label.
The kernels without the chunk-level bypass of the per-lane depth compares are the analysis build of the library:
  make -C torch-gaussian-splatting-rasterizer_amd/csrc ../../tools/libgsr_slab_nobypass.so
  GSR_LIB_PATH=tools/libgsr_slab_nobypass.so tools/slab_ab.py --label "no bypass"
usage: tools/slab_ab.py [--workload bicycle] [--rounds 30] [--early-out-T 0] [--label bypass]"""
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

#        entry, channels, near, far
RUNS = {"A": ("channels", 3, None, None), "A8": ("channels", 8, None, None), "A16": ("channels", 16, None, None),
        "B4": ("slab", 3, None, None), "B8": ("slab", 8, None, None), "B16": ("slab", 16, None, None),
        "C": ("slab", 3, None, "surface"), "D": ("slab", 3, "surface", None)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bicycle")
    ap.add_argument("--gaussians", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--early-out-T", type=float, default=0.0)
    ap.add_argument("--camera", type=int, default=0)
    ap.add_argument("--camera-set", default="single")
    ap.add_argument("--label", default="bypass")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "slab_ab.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cols, cam_list, n, W, H, _ = bench.build_workload(a.workload, a, a.gaussians)
    scene = renderer.GaussianScene.from_packed(utils.pack_gaussians(cols), device=dev)
    del cols
    cam = renderer.make_camera(*cam_list[0])
    R = renderer.Rasterizer(scene)
    R.fit_pairs(cam)
    zm = R.render_median_depth(cam)  # (its own stages 1-3, before the lists below are built)
    found = zm > 0
    inf = float("inf")
    planes = {("surface", "far"): torch.where(found, 1.05 * zm, torch.full_like(zm, inf)).contiguous(),
              ("surface", "near"): torch.where(found, 1.05 * zm, torch.full_like(zm, -inf)).contiguous()}
    ws = R._workspace(W, H)
    sc = scene.c_struct()
    stream = torch.cuda.current_stream(dev)
    sp = int(stream.cuda_stream)
    feats = torch.rand((n, 16), generator=torch.Generator().manual_seed(1)).to(dev)
    feats[:, :3] = R._depth_features(cam)
    o = renderer.make_options(early_out_T=a.early_out_T, colour_stage=0)
    maps = {r: torch.empty((H, W, ch), dtype=torch.float32, device=dev) for r, (_, ch, _, _) in RUNS.items()}
    final_T = {r: torch.empty((H, W), dtype=torch.float32, device=dev) for r in RUNS}
    wp, wn, mp = ws.data_ptr(), ws.numel(), R.max_pairs
    check(lib.gsr_preprocess(C.byref(sc), C.byref(cam), C.byref(o), wp, wn, None, sp))
    check(lib.gsr_bin_sort(n, C.byref(cam), C.byref(o), mp, wp, wn, sp))

    def run(r):
        entry, ch, near, far = RUNS[r]
        if entry == "channels":
            check(lib.gsr_blend_channels(n, C.byref(cam), C.byref(o), mp, wp, wn, feats.data_ptr(), ch, 16, maps[r].data_ptr(),
                                         final_T[r].data_ptr(), sp))
        else:
            check(lib.gsr_blend_slab(C.byref(sc), n, C.byref(cam), C.byref(o), mp, wp, wn, feats.data_ptr(), ch, 16,
                                     planes[near, "near"].data_ptr() if near else None, planes[far, "far"].data_ptr() if far else None,
                                     maps[r].data_ptr(), final_T[r].data_ptr(), sp))

    times, stats = {r: [] for r in RUNS}, {}
    for rnd in range(a.rounds + 2):  # the first two rounds warm up (code objects, the launch-order hint)
        for r in RUNS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            run(r)
            e1.record(stream)
            torch.cuda.synchronize(dev)
            if rnd >= 2:
                times[r].append(e0.elapsed_time(e1))
            if rnd == 1:
                stats[r] = R.stats()
    lines = [f"[{a.label}] {os.path.basename(_lib.LIB_PATH)}  {a.workload}: {n} gaussians, {W}x{H}, {a.rounds} interleaved rounds after 2 warm-up "
             f"rounds (blend stage alone, tile-order kernel included), early_out_T {a.early_out_T}; a median surface on "
             f"{float(found.float().mean()) * 100:.1f} % of the pixels"]
    what = {"A": "gsr_blend_channels, 3 channels", "A8": "gsr_blend_channels, 8 channels", "A16": "gsr_blend_channels, 16 channels",
            "B4": "gsr_blend_slab, 3 channels, open limits", "B8": "gsr_blend_slab, 8 channels, open limits",
            "B16": "gsr_blend_slab, 16 channels, open limits", "C": "gsr_blend_slab, 3 channels, far = 1.05 x median depth",
            "D": "gsr_blend_slab, 3 channels, near = 1.05 x median depth"}
    med = {}
    for r in RUNS:
        t = np.array(times[r])
        med[r] = float(np.median(t))
        lines.append(f"  {r:3}: median {np.median(t):.4f} ms  min {t.min():.4f} ms  max {t.max():.4f} ms  spread (max - min) / median "
                     f"{(t.max() - t.min()) / np.median(t) * 100:.1f} %   wave_entries {stats[r]['wave_entries']} fetched_entries "
                     f"{stats[r]['fetched_entries']}   [{what[r]}]")
    lines.append("  ratios at the median: " + "   ".join(f"{r} / A {med[r] / med['A']:.3f}" for r in RUNS if r != "A")
                 + f"   B8 / A8 {med['B8'] / med['A8']:.3f}   B16 / A16 {med['B16'] / med['A16']:.3f}")
    lines.append("  wave_entries / fetched_entries to A's: " + "   ".join(
        f"{r} {stats[r]['wave_entries'] / max(stats['A']['wave_entries'], 1):.3f} / {stats[r]['fetched_entries'] / max(stats['A']['fetched_entries'], 1):.3f}"
        for r in ("C", "D")))
    same = all(torch.equal(maps[b], maps[p]) and torch.equal(final_T[b], final_T[p]) for b, p in (("B4", "A"), ("B8", "A8"), ("B16", "A16")))
    counters = all(stats[b][k] == stats["A"][k] for b in ("B4", "B8", "B16") for k in ("wave_entries", "fetched_entries"))
    lines.append(f"  B's maps and T == A's: {same};  B's counters are A's: {counters};  mean T: A {float(final_T['A'].mean()):.4f}  "
                 f"C {float(final_T['C'].mean()):.4f}  D {float(final_T['D'].mean()):.4f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
