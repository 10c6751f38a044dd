#!/usr/bin/env python3
"""The camera backward against what a caller did before it and against its floor, on the bench frame, interleaved rounds in ONE
process.  Stages 1-2 run once (colour_stage = 0), then ONE real gsr_blend_splat_backward of --channels random channels fills the
[n, 8] array all three sides read.  Per round:
  A  the float32 restatement of the projection in torch on the GPU (tools/projection_reference.project64 over the touched rows) with
     w2c, full_proj, fx and fy requiring a gradient, then torch.autograd.grad: the camera gradient a caller chained by hand
  B  ONE gsr_camera_backward of the whole array into its 32 doubles
  C  ONE gsr_project_backward on the same rows into the four per-gaussian outputs (zeroed outside the timed span): the same reads
     and no reduction — the floor B should sit near
each between two events — median, min, max and spread over the rounds — and the bytes moved by B's own count,
32 n + 40 x rows touched (mean 12, log-scales 12, quaternion 16) + one 256-B row per workgroup written and read, as GB/s on B's
time and as a fraction of the device-to-device copy rate measured in the same process (bench.measured_copy_gbs).  No ratio or time
is fixed in advance.  B is also compared with A: the worst |difference| over the largest |value| of the 26 entries (a float32
autograd sum against float32 terms summed in double).
Writes what it prints to profiles/camera_backward_timing.txt (--out).  The measurement runs in a child process under a time limit
(--timeout seconds; tools/ab_harness.py).
usage: tools/camera_backward_timing.py [--workload bicycle] [--rounds 15] [--channels 3] [--timeout 420]"""
import ctypes as C

import ab_harness as ab

FIELDS = ("means", "log_scales", "quats", "opacity_logit")


def flags(ap):
    ap.add_argument("--channels", type=int, default=3)


def arguments(argv=None):
    return ab.arguments("camera_backward_timing", extra=flags, argv=argv, early_out=False)


def moved_bytes(n, touched, workspace):
    """B's own count: every row of grad_splat, per touched gaussian its 40 B of the scene, and the partial sums written and read."""
    return 32 * n + 40 * touched + 2 * workspace


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
    idx = rows[:, :6].ne(0).any(1).nonzero().squeeze(1)
    touched = int(idx.numel())
    waves = int(torch.unique(idx // 64).numel())
    r = rows[idx]
    base = pr.camera_of(f.cam)
    ws = torch.empty(int(lib.gsr_camera_backward_bytes(n)), dtype=torch.uint8, device=dev)
    out_b = torch.zeros(32, dtype=torch.float64, device=dev)
    out_c = [torch.zeros(s, dtype=torch.float32, device=dev) for s in ((n, 3), (n, 3), (n, 4), (n,))]
    got_a = []

    def run_a():
        theta = {k: f.scene.t[k][idx] for k in FIELDS}
        t = {k: torch.tensor(base[k], dtype=torch.float32, device=dev, requires_grad=True) for k in ("V", "F", "fx", "fy")}
        p = pr.project64(theta, dict(base, **t), torch.float32, dev)
        loss = (r[:, 0] * p["opacity"]).sum() + (r[:, 1:3] * p["screen_means"]).sum() + (r[:, 3:6] * p["sigmas"]).sum()
        got_a[:] = torch.autograd.grad(loss, [t[k] for k in ("V", "F", "fx", "fy")])

    def run_b():
        check(lib.gsr_camera_backward(C.byref(f.sc), C.byref(f.cam), C.byref(o), rows.data_ptr(), None, out_b.data_ptr(), ws.data_ptr(), ws.numel(), sp))

    def run_c():
        check(lib.gsr_project_backward(C.byref(f.sc), C.byref(f.cam), C.byref(o), rows.data_ptr(), *[b.data_ptr() for b in out_c], sp))

    def zero():
        for b in out_c:
            b.zero_()

    times, _ = ab.interleaved((("A", run_a), ("B", run_b), ("C", run_c)), a.rounds, "events", before=zero)
    copy_gbs = bench.measured_copy_gbs(dev)
    lines = [f"{a.workload}: {n} gaussians, {W}x{H}, {a.rounds} interleaved rounds after 2 of warm-up; grad_splat from one gsr_blend_splat_backward "
             f"of {a.channels} channels with grad_T: {touched} rows touched ({100.0 * touched / n:.1f} %), {waves} of {(n + 63) // 64} waves hold one",
             "A = torch float32 restatement + autograd.grad with respect to w2c, full_proj, fx, fy over the touched rows, "
             f"B = 1 x gsr_camera_backward ({ws.numel() // 256} workgroups), C = 1 x gsr_project_backward on the same rows"]
    med = {}
    for name in "ABC":
        line, med[name] = ab.summary(name, times[name])
        lines.append(line)
    lines.append(f"  {ab.ratios(med, 'A', ['B'])}   {ab.ratios(med, 'C', ['B'])}")
    lines.append(traffic_line("B", moved_bytes(n, touched, ws.numel()), med["B"], copy_gbs))
    run_a()
    run_b()
    torch.cuda.synchronize()
    got = renderer._camera_gradient_of(out_b)
    have = torch.cat([got.w2c.reshape(-1), got.full_proj.reshape(-1), got.focal]).cpu()
    want = torch.cat([got_a[0].reshape(-1), got_a[1].reshape(-1), got_a[2].reshape(1), got_a[3].reshape(1)]).double().cpu()
    scale = float(have.abs().max())
    lines.append(f"  B against A, worst |difference| / largest |value| over the 26 entries: {float((have - want).abs().max()) / scale if scale else 0.0:.2e}"
                 f"   contributing {int(got.contributing)} of {touched} touched   B finite {bool(torch.isfinite(out_b).all())}")
    ab.report(lines, a.out)


if __name__ == "__main__":
    ab.main(__file__, arguments(), worker)
