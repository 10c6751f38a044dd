#!/usr/bin/env python3
"""A/B of the K-view feature batches against the loop of single-view calls on the bench scene under the 25-camera ring,
interleaved rounds in ONE process (MI355X guide, rule 24).  For each of
  forward   C = 16 feature channels: render_features per camera            | render_features_batch
  backward  C = 16: feature_gradient(out=...) per camera into one buffer   | feature_gradient_batch(out=...)
  stats     sum, max, pixels and the view count: accumulate_view_stats on a Rasterizer of one slice (its per-camera loop)
            | view_stats_batch
A = the loop, the path the parent commit has; B = the batch call on a Rasterizer with views = 4 and views = 8.  Each is the whole
Python call over all 25 cameras (stages 1-2, the walks, the counters' read-backs; wall clock between two device
synchronisations), reported as ms per view: median, min, max and spread over the rounds, and the ratio A / B at the median.
--dispatches N: instead of timing, run N rounds of ONE leg (--leg forward-A, stats-B8, ...) after one warm-up round, for a kernel
trace around this process to count: dispatches per view = (count at N = 2 - count at N = 1) / 25.
The measurement runs in a child process of its own under a time limit (--timeout seconds); this process never opens the GPU.
Writes what it prints to profiles/views_ab.txt (--out).
usage: tools/views_ab.py [--workload bicycle] [--rounds 15] [--timeout 540]"""
import argparse
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CHANNELS = 16


def arguments():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bicycle")
    ap.add_argument("--gaussians", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--camera", type=int, default=0)
    ap.add_argument("--camera-set", default="all")
    ap.add_argument("--timeout", type=int, default=540)
    ap.add_argument("--dispatches", type=int, default=0)
    ap.add_argument("--leg", default="")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "views_ab.txt"))
    return ap.parse_args()


def worker(a):
    import numpy as np
    import torch

    import bench
    import gsr_amd  # noqa: F401
    from gsr_amd import renderer, utils

    dev = torch.device("cuda", 0)
    cols, cam_list, n, W, H, _ = bench.build_workload(a.workload, a, a.gaussians)
    scene = renderer.GaussianScene.from_packed(utils.pack_gaussians(cols), device=dev)
    del cols
    cams = [renderer.make_camera(*c) for c in cam_list]
    B = len(cams)
    R = {1: renderer.Rasterizer(scene), 4: renderer.Rasterizer(scene, views=4), 8: renderer.Rasterizer(scene, views=8)}
    need = 0
    for cam in cams:  # one pair bound for all: the worst view's
        R[1].render(cam)
        need = max(need, int(R[1].last_stats["n_pairs_bbox"]))
    for r in R.values():
        r.max_pairs = int(1.25 * need) + 4096
        r.sort_passes = R[1].sort_passes
    gen = torch.Generator().manual_seed(3)
    F = torch.randn((n, CHANNELS), generator=gen).to(dev)
    Gm = torch.randn((B, H, W, CHANNELS), generator=gen).to(dev)
    grad = torch.zeros((n, CHANNELS), dtype=torch.float32, device=dev)

    def forward_loop():
        return [R[1].render_features(cam, F, scene_order=True) for cam in cams]

    def backward_loop():
        for v, cam in enumerate(cams):
            R[1].feature_gradient(cam, Gm[v], out=grad)

    legs = {"forward-A": forward_loop, "backward-A": backward_loop, "stats-A": lambda: renderer.accumulate_view_stats(R[1], cams)}
    for K in (4, 8):
        legs[f"forward-B{K}"] = lambda K=K: R[K].render_features_batch(cams, F, scene_order=True)
        legs[f"backward-B{K}"] = lambda K=K: R[K].feature_gradient_batch(cams, Gm, out=grad)
        legs[f"stats-B{K}"] = lambda K=K: R[K].view_stats_batch(cams)

    if a.dispatches:
        for _ in range(1 + a.dispatches):
            legs[a.leg]()
            torch.cuda.synchronize(dev)
        return

    times = {k: [] for k in legs}
    for rnd in range(a.rounds + 2):  # the first two rounds warm up (code objects, the allocator, the workspaces)
        for name, run in legs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize(dev)
            if rnd >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3 / B)
    lines = [f"{a.workload}: {n} gaussians, {W}x{H}, {B} cameras, C = {CHANNELS}, {a.rounds} interleaved rounds after 2 warm-up rounds; ms per view"]
    med = {}
    for name in legs:
        t = np.array(times[name])
        med[name] = float(np.median(t))
        lines.append(f"  {name:12s} median {np.median(t):.4f}  min {t.min():.4f}  max {t.max():.4f}  spread (max - min) / median "
                     f"{(t.max() - t.min()) / np.median(t) * 100:.1f} %")
    for kind in ("forward", "backward", "stats"):
        lines.append(f"  {kind}: A / B4 {med[kind + '-A'] / med[kind + '-B4']:.3f}   A / B8 {med[kind + '-A'] / med[kind + '-B8']:.3f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


def main():
    a = arguments()
    if a.worker:
        return worker(a)
    # the one GPU step, in a process of its own and under its own time limit
    rc = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker"] + sys.argv[1:]).returncode
    if rc:
        sys.exit(f"views_ab: the measurement ended with status {rc}" + (" (time limit)" if rc in (124, 137) else ""))


if __name__ == "__main__":
    main()
