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
A's bit for bit.  Appends what it prints to profiles/slab_ab.txt (--out), under --label.  The measurement runs in a child process
under a time limit (--timeout seconds; tools/ab_harness.py).
The kernels without the chunk-level bypass of the per-lane depth compares are the analysis build of the library:
  make -C torch-gaussian-splatting-rasterizer_amd/csrc ../../tools/libgsr_slab_nobypass.so
  GSR_LIB_PATH=tools/libgsr_slab_nobypass.so tools/slab_ab.py --label "no bypass"
usage: tools/slab_ab.py [--workload bicycle] [--rounds 30] [--early-out-T 0] [--label bypass] [--timeout 420]"""
import ctypes as C
import os

import ab_harness as ab

#        entry, channels, near, far, what
RUNS = {"A": ("channels", 3, None, None, "gsr_blend_channels, 3 channels"), "A8": ("channels", 8, None, None, "gsr_blend_channels, 8 channels"),
        "A16": ("channels", 16, None, None, "gsr_blend_channels, 16 channels"),
        "B4": ("slab", 3, None, None, "gsr_blend_slab, 3 channels, open limits"), "B8": ("slab", 8, None, None, "gsr_blend_slab, 8 channels, open limits"),
        "B16": ("slab", 16, None, None, "gsr_blend_slab, 16 channels, open limits"),
        "C": ("slab", 3, None, "surface", "gsr_blend_slab, 3 channels, far = 1.05 x median depth"),
        "D": ("slab", 3, "surface", None, "gsr_blend_slab, 3 channels, near = 1.05 x median depth")}


def arguments(argv=None):
    return ab.arguments("slab_ab", rounds=30, label="bypass", argv=argv)


def worker(a):
    import torch

    f = ab.bench_frame(a)
    from gsr_amd import _lib, renderer
    from gsr_amd._lib import check, lib

    n, W, H, dev, sp = f.n, f.W, f.H, f.dev, f.sp
    zm = f.R.render_median_depth(f.cam)  # (its own stages 1-3, before the lists below are built)
    found = zm > 0
    inf = float("inf")
    planes = {("surface", "far"): torch.where(found, 1.05 * zm, torch.full_like(zm, inf)).contiguous(),
              ("surface", "near"): torch.where(found, 1.05 * zm, torch.full_like(zm, -inf)).contiguous()}
    feats = torch.rand((n, 16), generator=torch.Generator().manual_seed(1)).to(dev)
    feats[:, :3] = f.R._depth_features(f.cam)
    o = renderer.make_options(early_out_T=a.early_out_T, colour_stage=0)
    maps = {r: torch.empty((H, W, run[1]), dtype=torch.float32, device=dev) for r, run in RUNS.items()}
    final_T = {r: torch.empty((H, W), dtype=torch.float32, device=dev) for r in RUNS}
    f.make_lists(o)

    def run(r):
        entry, ch, near, far, _ = RUNS[r]
        if entry == "channels":
            check(lib.gsr_blend_channels(*f.lists(o), feats.data_ptr(), ch, 16, maps[r].data_ptr(), final_T[r].data_ptr(), sp))
        else:
            check(lib.gsr_blend_slab(C.byref(f.sc), *f.lists(o), feats.data_ptr(), ch, 16,
                                     planes[near, "near"].data_ptr() if near else None, planes[far, "far"].data_ptr() if far else None,
                                     maps[r].data_ptr(), final_T[r].data_ptr(), sp))

    times, stats = ab.interleaved([(r, (lambda r=r: run(r))) for r in RUNS], a.rounds, "events", stats=f.R.stats)
    lines = [f"{os.path.basename(_lib.LIB_PATH)}  {a.workload}: {n} gaussians, {W}x{H}, {a.rounds} interleaved rounds after 2 warm-up "
             f"rounds (blend stage alone, tile-order kernel included), early_out_T {a.early_out_T}; a median surface on "
             f"{float(found.float().mean()) * 100:.1f} % of the pixels"]
    med = {}
    for r in RUNS:
        line, med[r] = ab.summary(f"{r:3}", times[r], stats[r], RUNS[r][4])
        lines.append(line)
    lines.append("  ratios at the median: " + ab.ratios(med, "A") + "   " + ab.ratios(med, "A8", ["B8"]) + "   " + ab.ratios(med, "A16", ["B16"]))
    lines.append("  wave_entries / fetched_entries to A's: " + "   ".join(
        f"{r} {stats[r]['wave_entries'] / max(stats['A']['wave_entries'], 1):.3f} / {stats[r]['fetched_entries'] / max(stats['A']['fetched_entries'], 1):.3f}"
        for r in ("C", "D")))
    same = all(torch.equal(maps[b], maps[p]) and torch.equal(final_T[b], final_T[p]) for b, p in (("B4", "A"), ("B8", "A8"), ("B16", "A16")))
    counters = all(ab.same_counters(stats, b, "A") for b in ("B4", "B8", "B16"))
    lines.append(f"  B's maps and T == A's: {same};  B's counters are A's: {counters};  mean T: A {float(final_T['A'].mean()):.4f}  "
                 f"C {float(final_T['C'].mean()):.4f}  D {float(final_T['D'].mean()):.4f}")
    ab.report(lines, a.out, a.label, append=True)


if __name__ == "__main__":
    ab.main(__file__, arguments(), worker)
