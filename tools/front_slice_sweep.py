#!/usr/bin/env python3
"""The front slice (csrc/binning.hip) against the single pass, on the fused colour-frame entry: saturation_rule = 3 (forced on) and
4 (off) interleaved in one process, K views per launch sequence (gsr_render_batch; the second of two back-to-back batches timed with
events, per frame; median over the rounds), and for camera 0 the counters of each, what slice A alone emits (a progressive frame of its
ranks) and the cells still open after it.  Prints only.
usage: tools/front_slice_sweep.py [--rounds 15] [--views 1,4,6] WxH:n [WxH:n ...]     n: gaussians of synthetic.mip360_like(n, 361), ring cameras 0 ..
Another slice fraction is another build (csrc/Makefile: tools/libgsr_fsfrac%.so), loaded
with GSR_LIB_PATH; the counters' "slice A" line assumes the fraction given with --fraction (default 8)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import gsr_amd  # noqa: F401
from gsr_amd import _lib, renderer, synthetic


def open_cells(img, T):
    """32x32 cells with a pixel the colour-saturation rule has not finished (blend_args.h, pixel_finished; the reference's undrawn last
    column and row count as finished), of a frame and its transmittance after slice A's ranks alone: (open, all)."""
    H, W = T.shape
    cmin = img.min(-1).values
    thr = torch.where(cmin >= 2.0 ** -100, cmin * 2.0 ** -25, torch.zeros_like(cmin))
    live = T > thr
    live[H - 1, :] = False
    live[:, W - 1] = False
    pad = torch.zeros(((H + 31) // 32 * 32, (W + 31) // 32 * 32), dtype=torch.bool, device=T.device)
    pad[:H, :W] = live
    cells = pad.view(pad.shape[0] // 32, 32, pad.shape[1] // 32, 32).any(3).any(1)
    return int(cells.sum()), cells.numel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--fraction", type=int, default=8)
    ap.add_argument("--views", default="1", help="views per launch sequence, comma list (ring cameras 0, 1, ...)")
    ap.add_argument("cases", nargs="+")
    a = ap.parse_args()
    mk = renderer.make_options
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    print(f"library {os.path.relpath(_lib.LIB_PATH, repo)}, fraction 1/{a.fraction}, {a.rounds} interleaved rounds, ms per FRAME: median [min .. max]")
    for case in a.cases:
        size, n = case.split(":")
        W, H = (int(v) for v in size.split("x"))
        n = int(n)
        scene = renderer.GaussianScene.from_columns(synthetic.mip360_like(n, 361))
        fx = synthetic.pinhole_focal(W)
        ring = [renderer.make_camera(p.qvec, p.tvec, 2 * fx, 2 * fx, 2 * W, 2 * H, W, H) for p in synthetic.ring_cameras(25)]
        cam = ring[0]
        one = renderer.Rasterizer(scene)
        stats = {}
        try:
            for r in (4, 3):
                one.render(cam, mk(saturation_rule=r))
                stats[r] = dict(one.last_stats)
        except _lib.GsrError as e:
            print(f"{W}x{H} n {n}: {e}")
            continue
        V = stats[4]["n_visible"]
        L = (V + a.fraction - 1) // a.fraction
        imgA, TA = one.render(cam, mk(saturation_rule=4, draw_limit=L), return_T=True)
        A = dict(one.last_stats)
        oc, nc = open_cells(imgA, TA)
        print(f"{W}x{H} n {n}, camera 0: V {V}  D {stats[4]['n_pairs_bbox']}  E single pass {stats[4]['n_pairs']}, sliced {stats[3]['n_pairs']}"
              f" ({100.0 * stats[3]['n_pairs'] / max(stats[4]['n_pairs'], 1):.1f} %)")
        print(f"    slice A alone: D {A['n_pairs_bbox']}  E {A['n_pairs']}; open cells after it {oc} of {nc};  slice B emitted E "
              f"{stats[3]['n_pairs'] - A['n_pairs']} of the {stats[4]['n_pairs'] - A['n_pairs']} entries of its ranks")
        del one
        for K in (int(v) for v in a.views.split(",")):
            cams = ring[:K]
            R = renderer.Rasterizer(scene, views=K)
            R.max_pairs = max(renderer.Rasterizer(scene).fit_pairs(c, mk(saturation_rule=4)) for c in cams)
            out = {r: torch.empty((K, H, W, 3), device="cuda") for r in (3, 4)}
            for r in (4, 3):
                R.render_batch(cams, mk(saturation_rule=r), out=out[r])
            opts = {r: R.bounded(mk(saturation_rule=r)) for r in (3, 4)}
            times = {3: [], 4: []}
            for _ in range(a.rounds):
                for r in (4, 3):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    R.enqueue_batch(cams, opts[r], out=out[r])
                    e0.record()
                    R.enqueue_batch(cams, opts[r], out=out[r])
                    e1.record()
                    torch.cuda.synchronize()
                    times[r].append(e0.elapsed_time(e1) / K)
            R.stats()
            t = {r: np.array(times[r]) for r in times}
            line = lambda r: f"{np.median(t[r]):.4f} [{t[r].min():.4f} .. {t[r].max():.4f}]"
            print(f"    {K} view(s) per launch sequence: single pass {line(4)}  front slice {line(3)}  ratio {np.median(t[3]) / np.median(t[4]):.4f}"
                  f"  same frames {bool(torch.equal(out[3], out[4]))}")
            del R, out
            torch.cuda.empty_cache()
        del scene
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
