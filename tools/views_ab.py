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
Writes what it prints to profiles/views_ab.txt (--out).  The measurement runs in a child process under a time limit (--timeout
seconds; tools/ab_harness.py).
usage: tools/views_ab.py [--workload bicycle] [--rounds 15] [--timeout 540]"""
import ab_harness as ab

CHANNELS = 16


def flags(ap):
    ap.add_argument("--dispatches", type=int, default=0)
    ap.add_argument("--leg", default="")


def arguments(argv=None):
    return ab.arguments("views_ab", timeout=540, camera_set="all", early_out=False, extra=flags, argv=argv)


def worker(a):
    import torch

    f = ab.bench_frame(a, views=(4, 8))
    from gsr_amd import renderer

    n, W, H, dev, R, cams = f.n, f.W, f.H, f.dev, f.R, f.cams
    B = len(cams)
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

    times, _ = ab.interleaved(list(legs.items()), a.rounds, "wall", scale=1.0 / B)
    lines = [f"{a.workload}: {n} gaussians, {W}x{H}, {B} cameras, C = {CHANNELS}, {a.rounds} interleaved rounds after 2 warm-up rounds; ms per view"]
    med = {}
    for name in legs:
        line, med[name] = ab.summary(name, times[name])
        lines.append(line)
    for kind in ("forward", "backward", "stats"):
        lines.append(f"  {kind}: A / B4 {med[kind + '-A'] / med[kind + '-B4']:.3f}   A / B8 {med[kind + '-A'] / med[kind + '-B8']:.3f}")
    ab.report(lines, a.out)


if __name__ == "__main__":
    ab.main(__file__, arguments(), worker)
