"""What every tools/*_ab.py shares: the flags, the bench frame, the interleaved rounds, the summary line, the
write-out and the child process under a time limit.  A tool writes its legs (closures around the calls it compares) and its own
closing lines, and nothing else:
    def arguments(argv=None):  return ab.arguments("x_ab", rounds=15, extra=flags, argv=argv)
    def worker(a):             f = ab.bench_frame(a); ...; times, stats = ab.interleaved(legs, a.rounds, "events", stats=f.R.stats)
                               ...; ab.report(lines, a.out)
    if __name__ == "__main__": ab.main(__file__, arguments(), worker)
Importing this module imports neither torch nor bench nor gsr_amd: the functions that need them import them, so the parent
process of a tool never opens the GPU."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

WARMUP = 2  # rounds that are run and not kept (code objects, the allocator, the launch-order hint, the learned depth-sort bound)
COUNTERS = ("wave_entries", "fetched_entries")


def arguments(tool, rounds=15, timeout=420, extra=None, argv=None, label=None, writes=True, camera_set="single", early_out=True):
    """The common flags (--camera and --camera-set are what bench.build_workload reads off the namespace) and, through extra(ap), the
    tool's own.  writes=False: a tool that only prints unless --out names a file."""
    ap = argparse.ArgumentParser(prog=tool)
    ap.add_argument("--workload", default="bicycle")
    ap.add_argument("--gaussians", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=rounds)
    if early_out:
        ap.add_argument("--early-out-T", type=float, default=0.0)
    ap.add_argument("--camera", type=int, default=0)
    ap.add_argument("--camera-set", default=camera_set)
    ap.add_argument("--label", default=label)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", tool + ".txt") if writes else None)
    ap.add_argument("--timeout", type=int, default=timeout, help="seconds for the measurement, which runs in a child process")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    if extra:
        extra(ap)
    return ap.parse_args(argv)


class Frame:
    """The bench frame of one tool run: dev, scene, n, W, H, cam and cams, R (with views: {1: R, K: R of K views, ...}) and, for a
    single-view frame, sc, stream, sp and the workspace as wp, wn, mp."""

    def make_lists(self, o):
        """Stages 1-2 once: the one set of lists every leg then walks."""
        from gsr_amd._lib import check, lib

        check(lib.gsr_preprocess(C.byref(self.sc), C.byref(self.cam), C.byref(o), self.wp, self.wn, None, self.sp))
        check(lib.gsr_bin_sort(self.n, C.byref(self.cam), C.byref(o), self.mp, self.wp, self.wn, self.sp))

    def lists(self, o):
        """The six leading arguments of every gsr_blend_* entry."""
        return self.n, C.byref(self.cam), C.byref(o), self.mp, self.wp, self.wn


    def stages(self, L, o, out):
        """The three stage calls of one colour frame into `out` with the library L: a leg for the "stages" clock."""
        from gsr_amd._lib import check

        return (lambda: check(L.gsr_preprocess(C.byref(self.sc), C.byref(self.cam), C.byref(o), self.wp, self.wn, None, self.sp)),
                lambda: check(L.gsr_bin_sort(*self.lists(o), self.sp)),
                lambda: check(L.gsr_blend(None, *self.lists(o), out.data_ptr(), None, self.sp)))


def variants(a):
    """[(name, GsrOptions)] of the positional VARIANT = name[:field=value[,field=value]] arguments of the whole-frame tools."""
    from gsr_amd import renderer

    found = []
    for v in a.variants:
        name, _, envs = v.partition(":")
        kw = {k: (float(v) if "." in v or "e" in v else int(v)) for k, v in (e.split("=") for e in envs.split(",") if e)}
        found.append((name, renderer.make_options(**{"early_out_T": a.early_out_T, **kw})))
    return found


def bench_frame(a, views=(), fit=(None,), spatial_order=True):
    """The workload of bench.py on cuda:0 and a Rasterizer whose pair buffer fits the camera under every options struct of `fit`.
    views=(4, 8): all the cameras, a Rasterizer per K as well, and one pair bound for all of them: the worst view's."""
    import torch

    import bench
    import gsr_amd  # noqa: F401
    from gsr_amd import renderer, utils

    f = Frame()
    f.dev = torch.device("cuda", 0)
    cols, cam_list, f.n, f.W, f.H, _ = bench.build_workload(a.workload, a, a.gaussians)
    packed = utils.pack_gaussians(cols)
    del cols
    f.scene = renderer.GaussianScene.from_packed(packed, device=f.dev, spatial_order=spatial_order)
    del packed
    f.cams = [renderer.make_camera(*c) for c in cam_list]
    f.cam = f.cams[0]
    R = renderer.Rasterizer(f.scene)
    if views:
        f.R = {1: R, **{K: renderer.Rasterizer(f.scene, views=K) for K in views}}
        need = 0
        for cam in f.cams:
            R.render(cam)
            need = max(need, int(R.last_stats["n_pairs_bbox"]))
        for r in f.R.values():
            r.max_pairs = int(1.25 * need) + 4096
            r.sort_passes = R.sort_passes
        return f
    f.R = R
    R.max_pairs = max(R.fit_pairs(f.cam, o) for o in fit)
    ws = R._workspace(f.W, f.H)
    f.sc = f.scene.c_struct()
    f.stream = torch.cuda.current_stream(f.dev)
    f.sp = int(f.stream.cuda_stream)
    f.wp, f.wn, f.mp = ws.data_ptr(), ws.numel(), R.max_pairs
    return f


def _events():
    """One leg between two events on the current stream of cuda:0."""
    import torch

    stream = torch.cuda.current_stream()

    def clock(run):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        run()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    return clock


def _wall():
    """One whole call: wall clock between two device synchronisations."""
    import torch

    def clock(run):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    return clock


def _stages():
    """A leg that is a tuple of stage calls: an event before, between and after them, one time per stage.  The second of two
    back-to-back repetitions is the timed one (same leg twice: the caches are warm for it)."""
    import torch

    stream = torch.cuda.current_stream()

    def clock(stages):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(stages) + 1)]
        for _ in range(2):
            ev[0].record(stream)
            for k, stage in enumerate(stages):
                stage()
                ev[k + 1].record(stream)
        torch.cuda.synchronize()
        return [ev[k].elapsed_time(ev[k + 1]) for k in range(len(stages))]
    return clock


CLOCKS = {"events": _events, "wall": _wall, "stages": _stages}


def interleaved(legs, rounds, clock, before=None, stats=None, scale=1.0):
    """WARMUP + rounds rounds, every leg of `legs` ((name, run) pairs) once per round and in their order: A B C A B C.  clock:
    "events", "wall" or "stages", or a callable clock(run) that runs the leg and returns its milliseconds.  before() runs ahead of
    every leg, outside the timed span; stats() is read after each leg in the last warm-up round.  Returns (times, stats), each
    keyed by leg name; the times of the last `rounds` rounds, multiplied by scale."""
    clock = CLOCKS[clock]() if isinstance(clock, str) else clock
    times, counters = {name: [] for name, _ in legs}, {}
    for rnd in range(WARMUP + rounds):
        for name, run in legs:
            if before:
                before()
            t = clock(run)
            if rnd >= WARMUP:
                times[name].append([x * scale for x in t] if isinstance(t, list) else t * scale)
            if stats and rnd == WARMUP - 1:
                counters[name] = dict(stats())
    return times, counters


def spans(t):
    """(median, min, max) of a leg's times."""
    return float(statistics.median(t)), float(min(t)), float(max(t))


def column(times, k):
    """Stage k of the times of a "stages" leg."""
    return [t[k] for t in times]


def summary(name, t, stats=None, what=None, counters=COUNTERS):
    """(the line of one leg, its median): the one format of every tool."""
    med, lo, hi = spans(t)
    line = f"  {name}: median {med:.4f} ms  min {lo:.4f} ms  max {hi:.4f} ms  spread (max - min) / median {(hi - lo) / med * 100:.1f} %"
    if stats is not None:
        line += "   " + " ".join(f"{k} {stats[k]}" for k in counters)
    if what is not None:
        line += f"   [{what}]"
    return line, med


def ratios(med, base, names=None):
    """"B / A 1.500   C / A 0.500": every leg of names (default: all but base) to the leg base, at the median."""
    return "   ".join(f"{k} / {base} {med[k] / med[base]:.3f}" for k in (names or [k for k in med if k != base]))


def same_counters(stats, a, b, keys=COUNTERS):
    return all(stats[a][k] == stats[b][k] for k in keys)


def report(lines, out, label=None, append=False):
    """Print the lines, under [label] if there is one, and write them to out (if any) or append them."""
    text = "\n".join(lines)
    if label:
        text = f"[{label}] " + text
    print(text, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a" if append else "w") as f:
            f.write(text + "\n")
    return text


def in_child(tool_file, timeout, argv=None, command=None):
    """The one GPU step of a tool, in a process of its own and under its own time limit, so that a hung kernel ends the tool
    instead of holding the card: this process never opens the GPU.  (command: what to run in place of the tool's worker.)"""
    tool = os.path.splitext(os.path.basename(tool_file))[0]
    command = command or [sys.executable, os.path.abspath(tool_file), "--worker"] + list(sys.argv[1:] if argv is None else argv)
    rc = subprocess.run(["timeout", "-k", "10", str(timeout)] + command).returncode
    if rc:
        sys.exit(f"{tool}: the measurement ended with status {rc}" + (" (time limit)" if rc in (124, 137) else ""))


def main(tool_file, a, worker):
    return worker(a) if a.worker else in_child(tool_file, a.timeout)
