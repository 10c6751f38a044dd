#!/usr/bin/env python3
"""A/B of the per-gaussian view statistics against the existing summed-weight path on the bench frame, interleaved rounds in ONE
process (MI355X guide, rule 24).  Per round, each as the whole Python call (stages 1-2, the walk, the counters' read-back and the
return to file order; wall clock between two device synchronisations):
  a  R.blend_weights(cam): feature_gradient of a one-channel map of ones, blend_channels_backward_kernel<8> — the yardstick
  b  R.view_stats(cam, want=("sum",)): blend_gstats_kernel<1>
  c  R.view_stats(cam): all three, blend_gstats_kernel<7>
  d  c under a mask that keeps a centred rectangle of 10 % of the pixels
and, on ONE set of lists (stages 1-2 once), the blend stage alone between two events: A gsr_blend_channels_backward with one
channel of ones, B / C / D gsr_blend_gaussian_stats as above.
Median, min, max and spread over the rounds, the ratios to a / A, each walk's wave_entries / fetched_entries, an upper bound of the
atomic bytes per second (4 B per array and staged entry: a row is flushed at most once per batch that stages it), and whether b's
sums agree with a's.  The gate: b / a <= 1.04 at the median ("read nothing below +-4 %" on this frame).
The measurement runs in a child process of its own under a time limit (--timeout seconds); this process never opens the GPU.
Writes what it prints to profiles/gstats_ab.txt (--out).
usage: tools/gstats_ab.py [--workload bicycle] [--rounds 15] [--early-out-T 0] [--timeout 420]"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def arguments():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="bicycle")
    ap.add_argument("--gaussians", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--early-out-T", type=float, default=0.0)
    ap.add_argument("--camera", type=int, default=0)
    ap.add_argument("--camera-set", default="single")
    ap.add_argument("--timeout", type=int, default=420)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gstats_ab.txt"))
    return ap.parse_args()


def summary(name, t, st, what):
    import numpy as np

    t = np.array(t)
    return (f"  {name}: median {np.median(t):.4f} ms  min {t.min():.4f} ms  max {t.max():.4f} ms  spread (max - min) / median "
            f"{(t.max() - t.min()) / np.median(t) * 100:.1f} %   wave_entries {st['wave_entries']} fetched_entries {st['fetched_entries']}"
            f"   [{what}]"), float(np.median(t))


def worker(a):
    import torch

    import bench
    import gsr_amd  # noqa: F401
    from gsr_amd import renderer, utils
    from gsr_amd._lib import check, lib

    dev = torch.device("cuda", 0)
    cols, cam_list, n, W, H, _ = bench.build_workload(a.workload, a, a.gaussians)
    scene = renderer.GaussianScene.from_packed(utils.pack_gaussians(cols), device=dev)
    del cols
    cam = renderer.make_camera(*cam_list[0])
    R = renderer.Rasterizer(scene)
    R.fit_pairs(cam)
    o = renderer.make_options(early_out_T=a.early_out_T, colour_stage=0)
    mask = torch.zeros((H, W), dtype=torch.uint8, device=dev)
    mh, mw = int(round(H * 0.1 ** 0.5)), int(round(W * 0.1 ** 0.5))
    mask[(H - mh) // 2:(H - mh) // 2 + mh, (W - mw) // 2:(W - mw) // 2 + mw] = 1
    kept = float(mask.float().mean())

    # ---- the whole calls ----
    res = {}
    calls = (("a", lambda: R.blend_weights(cam, o)), ("b", lambda: R.view_stats(cam, o, want=("sum",)).weight_sum),
             ("c", lambda: R.view_stats(cam, o)), ("d", lambda: R.view_stats(cam, o, mask=mask)))
    times, stats = {k: [] for k, _ in calls}, {}
    for rnd in range(a.rounds + 2):  # the first two rounds warm up (code objects, the allocator, the learned depth-sort bound)
        for name, run in calls:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            res[name] = run()
            torch.cuda.synchronize(dev)
            if rnd >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3)
            stats[name] = dict(R.last_stats)
    lines = [f"{a.workload}: {n} gaussians, {W}x{H}, {a.rounds} interleaved rounds after 2 warm-up rounds, early_out_T {a.early_out_T}; "
             f"the mask keeps {kept * 100:.1f} % of the pixels", " whole calls (stages 1-2 + walk + counters + file order):"]
    what = {"a": "R.blend_weights", "b": "R.view_stats, want = sum", "c": "R.view_stats, sum + max + pixels", "d": "c under the 10 % mask"}
    med = {}
    for name, _ in calls:
        line, med[name] = summary(name, times[name], stats[name], what[name])
        lines.append(line)
    lines.append("  ratios at the median: " + "   ".join(f"{k} / a {med[k] / med['a']:.3f}" for k in "bcd")
                 + f"   GATE b / a <= 1.04: {med['b'] / med['a'] <= 1.04}")
    wa, wb = res["a"].double(), res["b"].double()
    err = float((wa - wb).abs().max() / wa.abs().max())
    lines.append(f"  b's sums against a's: max |diff| / max {err:.2e};  c: {int((res['c'].pixels > 0).sum())} of {n} gaussians reach a pixel, "
                 f"d: {int((res['d'].pixels > 0).sum())};  largest weight_max {float(res['c'].weight_max.max()):.6f}")

    # ---- the blend stage alone, on one set of lists ----
    ws = R._workspace(W, H)
    sc = scene.c_struct()
    stream = torch.cuda.current_stream(dev)
    sp = int(stream.cuda_stream)
    wp, wn, mp = ws.data_ptr(), ws.numel(), R.max_pairs
    ones = torch.ones((H, W, 1), dtype=torch.float32, device=dev)
    s, m, p = (torch.zeros(n, dtype=dt, device=dev) for dt in (torch.float32, torch.float32, torch.int32))
    check(lib.gsr_preprocess(C.byref(sc), C.byref(cam), C.byref(o), wp, wn, None, sp))
    check(lib.gsr_bin_sort(n, C.byref(cam), C.byref(o), mp, wp, wn, sp))

    def stats_walk(mask_t, outs):
        check(lib.gsr_blend_gaussian_stats(n, C.byref(cam), C.byref(o), mp, wp, wn, mask_t.data_ptr() if mask_t is not None else None,
                                           *[t.data_ptr() if t is not None else None for t in outs], sp))

    runs = (("A", lambda: check(lib.gsr_blend_channels_backward(n, C.byref(cam), C.byref(o), mp, wp, wn, ones.data_ptr(), 1, s.data_ptr(), 1, sp))),
            ("B", lambda: stats_walk(None, (s, None, None))), ("C", lambda: stats_walk(None, (s, m, p))), ("D", lambda: stats_walk(mask, (s, m, p))))
    times, stats = {k: [] for k, _ in runs}, {}
    for rnd in range(a.rounds + 2):
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
    lines.append(" the blend stage alone (tile-order kernel included), one set of lists:")
    what = {"A": "gsr_blend_channels_backward, 1 channel of ones", "B": "gsr_blend_gaussian_stats, sum", "C": "gsr_blend_gaussian_stats, all three",
            "D": "C under the 10 % mask"}
    arrays = {"A": 1, "B": 1, "C": 3, "D": 3}
    for name, _ in runs:
        line, med[name] = summary(name, times[name], stats[name], what[name])
        lines.append(line)
    lines.append("  ratios at the median: " + "   ".join(f"{k} / A {med[k] / med['A']:.3f}" for k in "BCD"))
    lines.append("  atomic bytes per second, upper bound (4 B x arrays x fetched_entries / median): " + "   ".join(
        f"{k} {4 * arrays[k] * stats[k]['fetched_entries'] / (med[k] * 1e-3) / 1e9:.1f} GB/s" for k in "ABCD"))
    lines.append(f"  B's counters are A's: {all(stats['B'][k] == stats['A'][k] for k in ('wave_entries', 'fetched_entries'))}")
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
        sys.exit(f"gstats_ab: the measurement ended with status {rc}" + (" (time limit)" if rc in (124, 137) else ""))


if __name__ == "__main__":
    main()
