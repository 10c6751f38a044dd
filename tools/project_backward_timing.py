#!/usr/bin/env python3
"""The projection backward against what a caller did before it, on the bench frame, interleaved rounds in ONE process.
Stages 1-2 run once (colour_stage = 0), then ONE real gsr_blend_splat_backward of --channels random channels fills the [n, 8] array
both sides read.  Per round:
  A  the float32 restatement of the projection in torch on the GPU (tools/projection_reference.project64: gather the reached rows
     of the scene, every stage as torch ops, torch.autograd.grad, index_add_ the four gradients back): the projection backward a
     caller chained by hand, over the reached rows only
  B  ONE gsr_project_backward of the whole array into the four outputs (zeroed outside the timed span)
each between two events — median, min, max and spread over the rounds — and the bytes moved by B's own count,
32 n + (44 read + 44 read-modify-written) x rows touched, as GB/s on B's time and as a fraction of the device-to-device
copy rate measured in the same process (bench.measured_copy_gbs).  No ratio or time is fixed in advance.  B is also compared with A
(the worst difference per output over that output's largest value): two float32 evaluations of one chain.
Writes what it prints to profiles/project_backward_ab.txt (--out).  The measurement runs in a child process under a time limit
(--timeout seconds; tools/ab_harness.py).
usage: tools/project_backward_timing.py [--workload bicycle] [--rounds 15] [--channels 3] [--timeout 420]"""
import ctypes as C

import ab_harness as ab

FIELDS = ("means", "log_scales", "quats", "opacity_logit")


def flags(ap):
    ap.add_argument("--channels", type=int, default=3)


def arguments(argv=None):
    return ab.arguments("project_backward_ab", extra=flags, argv=argv, early_out=False)


def moved_bytes(n, touched):
    """B's own count: every row of grad_splat, and per touched gaussian its 44 B read and 44 B read-modify-written."""
    return 32 * n + (44 + 44) * touched


def traffic_line(name, nbytes, ms, copy_gbs):
    gbs = nbytes / (ms * 1e-3) / 1e9
    return f"  {name}: {nbytes / 1e6:.1f} MB by B's count in {ms:.4f} ms = {gbs:.0f} GB/s, {gbs / copy_gbs:.3f} of the measured copy rate ({copy_gbs:.0f} GB/s)"


def worker(a):
    import torch

    f = ab.bench_frame(a)
    import bench
    import projection_reference as pr
    from gsr_amd import renderer
    from gsr_amd._lib import check, lib

    n, W, H, dev, sp = f.n, f.W, f.H, f.dev, f.sp
    o = renderer.make_options(colour_stage=0)
    f.make_lists(o)
    gen = torch.Generator().manual_seed(1)
    F = torch.randn((n, a.channels), generator=gen).to(dev)
    Gm = torch.randn((H, W, a.channels), generator=gen).to(dev)
    gT = torch.randn((H, W), generator=gen).to(dev)
    rows = torch.zeros((n, 8), dtype=torch.float32, device=dev)
    check(lib.gsr_blend_splat_backward(*f.lists(o), F.data_ptr(), a.channels, a.channels, Gm.data_ptr(), gT.data_ptr(), 0.0, 0, rows.data_ptr(), sp))
    f.R.stats()
    del F, Gm, gT
    hit = rows[:, :6].ne(0).any(1)
    idx = hit.nonzero().squeeze(1)
    touched = int(idx.numel())
    waves = int(torch.unique(idx // 64).numel())
    r = rows[idx]
    cam = pr.camera_of(f.cam)
    shapes = ((n, 3), (n, 3), (n, 4), (n,))
    out_a = [torch.zeros(s, dtype=torch.float32, device=dev) for s in shapes]
    out_b = [torch.zeros(s, dtype=torch.float32, device=dev) for s in shapes]

    def run_a():
        t = {k: f.scene.t[k][idx].requires_grad_(True) for k in FIELDS}
        p = pr.project64(t, cam, torch.float32, dev)
        loss = (r[:, 0] * p["opacity"]).sum() + (r[:, 1:3] * p["screen_means"]).sum() + (r[:, 3:6] * p["sigmas"]).sum()
        for k, g in zip(range(4), torch.autograd.grad(loss, [t[k] for k in FIELDS])):
            out_a[k].index_add_(0, idx, g)

    def run_b():
        check(lib.gsr_project_backward(C.byref(f.sc), C.byref(f.cam), C.byref(o), rows.data_ptr(), *[b.data_ptr() for b in out_b], sp))

    def zero():
        for b in out_a + out_b:
            b.zero_()

    times, _ = ab.interleaved((("A", run_a), ("B", run_b)), a.rounds, "events", before=zero)
    copy_gbs = bench.measured_copy_gbs(dev)
    lines = [f"{a.workload}: {n} gaussians, {W}x{H}, {a.rounds} interleaved rounds after 2 of warm-up; grad_splat from one gsr_blend_splat_backward "
             f"of {a.channels} channels with grad_T: {touched} rows touched ({100.0 * touched / n:.1f} %), {waves} of {(n + 63) // 64} waves hold one",
             "A = torch float32 restatement + autograd.grad over the reached rows, B = 1 x gsr_project_backward"]
    med = {}
    for name in "AB":
        line, med[name] = ab.summary(name, times[name])
        lines.append(line)
    nbytes = moved_bytes(n, touched)
    lines.append(f"  {ab.ratios(med, 'A')}   {ab.ratios(med, 'B')}")
    lines.append(traffic_line("B", nbytes, med["B"], copy_gbs))  # (A moves other bytes: many passes and temporaries; its time is its figure)
    zero()  # (every leg of the rounds started from zeroed outputs: one more of each, side by side)
    run_a()
    run_b()
    torch.cuda.synchronize()
    worst = {}
    for k, name in enumerate(FIELDS):
        scale = float(out_b[k].abs().max())
        worst[name] = float((out_a[k] - out_b[k]).abs().max()) / scale if scale else 0.0
    lines.append("  B against A, worst |difference| / largest |value| per output: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items())
                 + f"   B finite {all(bool(torch.isfinite(b).all()) for b in out_b)}")
    ab.report(lines, a.out)


if __name__ == "__main__":
    ab.main(__file__, arguments(), worker)
