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
Writes what it prints to profiles/gstats_ab.txt (--out).  The measurement runs in a child process under a time limit (--timeout
seconds; tools/ab_harness.py).
usage: tools/gstats_ab.py [--workload bicycle] [--rounds 15] [--early-out-T 0] [--timeout 420]"""
import ab_harness as ab


def arguments(argv=None):
    return ab.arguments("gstats_ab", argv=argv)


def worker(a):
    import torch

    f = ab.bench_frame(a)
    from gsr_amd import renderer
    from gsr_amd._lib import check, lib

    n, W, H, dev, sp, R, cam = f.n, f.W, f.H, f.dev, f.sp, f.R, f.cam
    o = renderer.make_options(early_out_T=a.early_out_T, colour_stage=0)
    mask = torch.zeros((H, W), dtype=torch.uint8, device=dev)
    mh, mw = int(round(H * 0.1 ** 0.5)), int(round(W * 0.1 ** 0.5))
    mask[(H - mh) // 2:(H - mh) // 2 + mh, (W - mw) // 2:(W - mw) // 2 + mw] = 1
    kept = float(mask.float().mean())

    # ---- the whole calls ----
    res = {}
    calls = {"a": lambda: R.blend_weights(cam, o), "b": lambda: R.view_stats(cam, o, want=("sum",)).weight_sum,
             "c": lambda: R.view_stats(cam, o), "d": lambda: R.view_stats(cam, o, mask=mask)}
    legs = [(k, (lambda k=k: res.__setitem__(k, calls[k]()))) for k in calls]
    times, stats = ab.interleaved(legs, a.rounds, "wall", stats=lambda: R.last_stats)
    lines = [f"{a.workload}: {n} gaussians, {W}x{H}, {a.rounds} interleaved rounds after 2 warm-up rounds, early_out_T {a.early_out_T}; "
             f"the mask keeps {kept * 100:.1f} % of the pixels", " whole calls (stages 1-2 + walk + counters + file order):"]
    what = {"a": "R.blend_weights", "b": "R.view_stats, want = sum", "c": "R.view_stats, sum + max + pixels", "d": "c under the 10 % mask"}
    med = {}
    for name in calls:
        line, med[name] = ab.summary(name, times[name], stats[name], what[name])
        lines.append(line)
    lines.append(f"  ratios at the median: {ab.ratios(med, 'a')}   GATE b / a <= 1.04: {med['b'] / med['a'] <= 1.04}")
    wa, wb = res["a"].double(), res["b"].double()
    err = float((wa - wb).abs().max() / wa.abs().max())
    lines.append(f"  b's sums against a's: max |diff| / max {err:.2e};  c: {int((res['c'].pixels > 0).sum())} of {n} gaussians reach a pixel, "
                 f"d: {int((res['d'].pixels > 0).sum())};  largest weight_max {float(res['c'].weight_max.max()):.6f}")

    # ---- the blend stage alone, on one set of lists ----
    ones = torch.ones((H, W, 1), dtype=torch.float32, device=dev)
    s, m, p = (torch.zeros(n, dtype=dt, device=dev) for dt in (torch.float32, torch.float32, torch.int32))
    f.make_lists(o)

    def stats_walk(mask_t, outs):
        check(lib.gsr_blend_gaussian_stats(*f.lists(o), mask_t.data_ptr() if mask_t is not None else None,
                                           *[t.data_ptr() if t is not None else None for t in outs], sp))

    legs = (("A", lambda: check(lib.gsr_blend_channels_backward(*f.lists(o), ones.data_ptr(), 1, s.data_ptr(), 1, sp))),
            ("B", lambda: stats_walk(None, (s, None, None))), ("C", lambda: stats_walk(None, (s, m, p))), ("D", lambda: stats_walk(mask, (s, m, p))))
    times, stats = ab.interleaved(legs, a.rounds, "events", stats=R.stats)
    lines.append(" the blend stage alone (tile-order kernel included), one set of lists:")
    what = {"A": "gsr_blend_channels_backward, 1 channel of ones", "B": "gsr_blend_gaussian_stats, sum", "C": "gsr_blend_gaussian_stats, all three",
            "D": "C under the 10 % mask"}
    arrays = {"A": 1, "B": 1, "C": 3, "D": 3}
    med = {}
    for name, _ in legs:
        line, med[name] = ab.summary(name, times[name], stats[name], what[name])
        lines.append(line)
    lines.append("  ratios at the median: " + ab.ratios(med, "A"))
    lines.append("  atomic bytes per second, upper bound (4 B x arrays x fetched_entries / median): " + "   ".join(
        f"{k} {4 * arrays[k] * stats[k]['fetched_entries'] / (med[k] * 1e-3) / 1e9:.1f} GB/s" for k in "ABCD"))
    lines.append(f"  B's counters are A's: {ab.same_counters(stats, 'B', 'A')}")
    ab.report(lines, a.out)


if __name__ == "__main__":
    ab.main(__file__, arguments(), worker)
