#!/usr/bin/env python3
"""The SH colour backward against what a caller did before it, on the bench frame, interleaved rounds in ONE process.
Stages 1-2 run once (colour_stage = 0), then ONE real gsr_blend_channels_backward of a random three-channel grad_map fills the
[n, 3] array both sides read: d L / d colour of every gaussian the view reaches.  Per round:
  A  the package's float32 sh_to_rgb restated in torch on the GPU (tools/sh_reference.sh_to_rgb_torch: gather the touched rows of
     the means and the SH array, the sixteen basis polynomials as torch ops, clamp, torch.autograd.grad, index_add_ the two gradients
     back): the colour backward a caller chained by hand, over the touched rows only
  B  ONE gsr_sh_backward of the whole array into grad_sh and grad_means (zeroed outside the timed span)
  and, for every tools/libgsr_shb_min<N>.so that has been built (make -C csrc ../../tools/libgsr_shb_min65.so ...), the same call
  in that library: the kernel with another dense-wave threshold (65: every wave per-lane; 1: every full wave through LDS)
each between two events — median, min, max and spread over the rounds — and the bytes moved by B's own count,
12 n + (12 + 192 + 384 + 24) x rows touched, as GB/s on B's time and as a fraction of the device-to-device copy rate measured in the
same process (bench.measured_copy_gbs).  No ratio or time is fixed in advance.  B is also compared with A (the worst difference per
output over that output's largest value: two float32 evaluations of one chain) and with every variant (bit for bit).
Writes what it prints to profiles/sh_backward_timing.txt (--out).  The measurement runs in a child process under a time limit
(--timeout seconds; tools/ab_harness.py).
usage: tools/sh_backward_timing.py [--workload bicycle] [--rounds 15] [--timeout 420]"""
import ctypes as C
import glob
import os
import re

import ab_harness as ab


def arguments(argv=None):
    return ab.arguments("sh_backward_timing", argv=argv, early_out=False)


def moved_bytes(n, touched):
    """B's own count: every row of grad_rgb, and per touched gaussian its mean, its SH row, its row of grad_sh read and written and
    its row of grad_means read and written."""
    return 12 * n + (12 + 192 + 384 + 24) * touched


def traffic_line(name, nbytes, ms, copy_gbs):
    gbs = nbytes / (ms * 1e-3) / 1e9
    return f"  {name}: {nbytes / 1e6:.1f} MB by B's count in {ms:.4f} ms = {gbs:.0f} GB/s, {gbs / copy_gbs:.3f} of the measured copy rate ({copy_gbs:.0f} GB/s)"


def variant_libraries():
    """[(threshold, path)] of the analysis builds found next to this file, by threshold."""
    found = []
    for path in glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "libgsr_shb_min*.so")):
        found.append((int(re.search(r"min(\d+)\.so$", path).group(1)), path))
    return sorted(found)


def worker(a):
    import torch

    f = ab.bench_frame(a)
    import bench
    import sh_reference as shr
    from gsr_amd import _lib, renderer
    from gsr_amd._lib import check, lib

    n, W, H, dev, sp = f.n, f.W, f.H, f.dev, f.sp
    o = renderer.make_options(colour_stage=0)
    f.make_lists(o)
    Gm = torch.randn((H, W, 3), generator=torch.Generator().manual_seed(1)).to(dev)
    g_rgb = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    check(lib.gsr_blend_channels_backward(*f.lists(o), Gm.data_ptr(), 3, g_rgb.data_ptr(), 3, sp))
    f.R.stats()
    del Gm
    idx = g_rgb.ne(0).any(1).nonzero().squeeze(1)
    touched = int(idx.numel())
    per_wave = torch.bincount(idx // 64, minlength=(n + 63) // 64)
    waves, dense48 = int((per_wave > 0).sum()), int((per_wave >= 48).sum())
    g_hit = g_rgb[idx]
    degree = f.scene.sh_degree
    cc = torch.tensor(list(f.cam.cam_center), dtype=torch.float32, device=dev)
    shapes = ((n, 16, 3), (n, 3))
    out_a = [torch.zeros(s, dtype=torch.float32, device=dev) for s in shapes]
    out_b = [torch.zeros(s, dtype=torch.float32, device=dev) for s in shapes]

    def run_a():
        p = f.scene.t["means"][idx].requires_grad_(True)
        sh = f.scene.t["sh"][idx].float().reshape(-1, 16, 3).requires_grad_(True)
        loss = (g_hit * shr.sh_to_rgb_torch(p, sh, cc, degree)).sum()
        g_sh, g_p = torch.autograd.grad(loss, [sh, p])
        out_a[0].index_add_(0, idx, g_sh)
        out_a[1].index_add_(0, idx, g_p)

    def call(L):
        def run():
            check(L.gsr_sh_backward(C.byref(f.sc), C.byref(f.cam), g_rgb.data_ptr(), 3, out_b[0].data_ptr(), out_b[1].data_ptr(), sp))
        return run

    def zero():
        for b in out_a + out_b:
            b.zero_()

    legs = [("A", run_a), ("B", call(lib))]
    for threshold, path in variant_libraries():
        L = C.CDLL(path)
        L.gsr_sh_backward.argtypes, L.gsr_sh_backward.restype = lib.gsr_sh_backward.argtypes, C.c_int
        legs.append((f"B{threshold}", call(L)))
    times, _ = ab.interleaved(legs, a.rounds, "events", before=zero)
    copy_gbs = bench.measured_copy_gbs(dev)
    lines = [f"{a.workload}: {n} gaussians, {W}x{H}, SH degree {degree}, {a.rounds} interleaved rounds after 2 of warm-up; grad_rgb from one "
             f"gsr_blend_channels_backward of 3 channels: {touched} rows touched ({100.0 * touched / n:.1f} %), {waves} of {(n + 63) // 64} "
             f"waves hold one, {dense48} hold 48 or more",
             "A = torch float32 sh_to_rgb + autograd.grad over the touched rows + index_add_, B = 1 x gsr_sh_backward (the library as built), "
             "B<N> = the same call with the dense-wave threshold N (65: per-lane only, 1: every full wave through LDS)"]
    med = {}
    for name, _ in legs:
        line, med[name] = ab.summary(name, times[name])
        lines.append(line)
    lines.append(f"  {ab.ratios(med, 'A')}")
    if len(legs) > 2:
        lines.append(f"  {ab.ratios(med, 'B', [k for k in med if k not in 'AB'])}")
    nbytes = moved_bytes(n, touched)
    for name, _ in legs[1:]:
        lines.append(traffic_line(name, nbytes, med[name], copy_gbs))  # (A moves other bytes: many passes and temporaries)
    zero()  # (every leg of the rounds started from zeroed outputs: one more of each, side by side)
    run_a()
    legs[1][1]()
    torch.cuda.synchronize()
    worst = {}
    for k, name in enumerate(("sh", "means")):
        scale = float(out_b[k].abs().max())
        worst[name] = float((out_a[k] - out_b[k]).abs().max()) / scale if scale else 0.0
    lines.append("  B against A, worst |difference| / largest |value| per output: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items())
                 + f"   B finite {all(bool(torch.isfinite(b).all()) for b in out_b)}")
    kept = [b.clone() for b in out_b]
    for name, run in legs[2:]:
        for b in out_b:
            b.zero_()
        run()
        torch.cuda.synchronize()
        lines.append(f"  {name} against B: bit for bit {all(torch.equal(x, y) for x, y in zip(kept, out_b))}")
    ab.report(lines, a.out)


if __name__ == "__main__":
    ab.main(__file__, arguments(), worker)
