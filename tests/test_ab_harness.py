"""CPU: tools/ab_harness.py, the one harness of the A/B timing tools — its formatting, its rounds, its flags,
its write-out and its child process, and that the tools leave clocks and the bench setup to it."""
import ast
import glob
import importlib.util
import os
import subprocess
import sys

import pytest
from conftest import REPO

TOOLS = os.path.join(REPO, "tools")


def _tool(name):
    """tools/<name>.py as the module `name`, loaded by its path and entered under its own name (no sys.path here)."""
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(TOOLS, name + ".py"))
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        spec.loader.exec_module(module)
    return sys.modules[name]


ab = _tool("ab_harness")


def test_loading_the_harness_imports_no_torch_bench_or_package():
    code = ("import importlib.util, sys\n"
            f"spec = importlib.util.spec_from_file_location('ab_harness', {os.path.join(TOOLS, 'ab_harness.py')!r})\n"
            "m = importlib.util.module_from_spec(spec); sys.modules['ab_harness'] = m; spec.loader.exec_module(m)\n"
            "bad = [k for k in ('torch', 'bench', 'gsr_amd', 'numpy') if k in sys.modules]\n"
            "assert not bad, bad\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_summary_line_character_for_character():
    line, med = ab.summary("A", [1.0, 2.0, 4.0], {"wave_entries": 5, "fetched_entries": 7}, "what")
    assert line == ("  A: median 2.0000 ms  min 1.0000 ms  max 4.0000 ms  spread (max - min) / median 150.0 %   "
                    "wave_entries 5 fetched_entries 7   [what]")
    assert med == 2.0
    # without counters and without a remark: the line of a whole-call leg; an even count takes the mean of the middle two
    assert ab.summary("x", [1.0, 3.0]) == ("  x: median 2.0000 ms  min 1.0000 ms  max 3.0000 ms  spread (max - min) / median 100.0 %", 2.0)
    # further counters are the tool's choice, in its order
    assert ab.summary("A", [1.0], {"wave_entries": 5, "fetched_entries": 7, "colour_evals": 0, "n_pairs": 9}, None,
                      ab.COUNTERS + ("colour_evals",))[0].endswith("%   wave_entries 5 fetched_entries 7 colour_evals 0")


def test_ratios_line():
    med = {"A": 2.0, "B": 3.0, "C": 1.0}
    assert ab.ratios(med, "A") == "B / A 1.500   C / A 0.500"
    assert ab.ratios(med, "A", ["B", "C"]) == "B / A 1.500   C / A 0.500"
    assert ab.ratios(med, "B", ["C"]) == "C / B 0.333"


@pytest.mark.parametrize("rounds", [1, 3])
def test_interleaved_runs_every_leg_in_order_and_keeps_the_last_rounds(rounds):
    log, tick = [], [0.0]

    def clock(run):  # a fake clock: every leg "takes" as many ms as calls the clock has seen, and says when its span opens and closes
        log.append("open")
        run()
        log.append("close")
        tick[0] += 1.0
        return tick[0]

    legs = [(k, (lambda k=k: log.append(k))) for k in "ABC"]
    times, stats = ab.interleaved(legs, rounds, clock, before=lambda: log.append("before"), stats=lambda: (log.append("stats"), {"at": tick[0]})[1],
                                  scale=0.5)
    total = rounds + 2
    expected = []
    for rnd in range(total):
        for k in "ABC":
            expected += ["before", "open", k, "close"] + (["stats"] if rnd == 1 else [])
    assert log == expected  # A B C A B C ...; before outside the span, once per leg and round; stats once per leg, in round index 1
    for i, k in enumerate("ABC"):
        assert times[k] == [0.5 * (3 * rnd + i + 1) for rnd in range(2, total)]  # the last `rounds`, scaled
        assert stats[k] == {"at": 3.0 + i + 1}
    # stage legs: one time per stage, scaled alike; no stats asked, none returned
    times, stats = ab.interleaved([("f", None)], rounds, lambda run: [1.0, 2.0, 4.0], scale=2.0)
    assert times == {"f": [[2.0, 4.0, 8.0]] * rounds} and stats == {}
    assert ab.column(times["f"], 2) == [8.0] * rounds


def test_arguments():
    a = ab.arguments("x_ab", rounds=12, argv=[])
    assert a.out == os.path.join(REPO, "profiles", "x_ab.txt")
    assert (a.workload, a.gaussians, a.rounds, a.early_out_T, a.camera, a.camera_set, a.label, a.timeout, a.worker) == \
        ("bicycle", 0, 12, 0.0, 0, "single", None, 420, False)  # --camera and --camera-set: bench.build_workload reads them

    def extra(ap):
        ap.add_argument("--channels", default="8,16,32")
        ap.add_argument("--abs", action="store_true")
        ap.add_argument("variants", nargs="*")

    a = ab.arguments("y_ab", rounds=30, timeout=540, extra=extra, label="guarded", camera_set="all", writes=False,
                     argv=["--channels", "3,16", "--abs", "--worker", "--early-out-T", "0.01", "--camera", "3", "v1", "v2:blend_impl=1"])
    assert (a.channels, a.abs, a.variants, a.worker, a.early_out_T, a.camera) == ("3,16", True, ["v1", "v2:blend_impl=1"], True, 0.01, 3)
    assert (a.rounds, a.timeout, a.label, a.camera_set, a.out) == (30, 540, "guarded", "all", None)
    assert ab.arguments("z_ab", argv=["--out", "f.txt", "--label", "l", "--timeout", "9"]).out == "f.txt"


def test_every_tool_parses_its_own_flags_on_the_harness():
    """The defaults that differ stay per tool."""
    want = {"blend_ab": (15, 420, None), "channels_ab": (15, 420, "channels_ab.txt"), "channels_backward_ab": (15, 420, "channels_backward_ab.txt"),
            "features_ab": (15, 420, None), "frame_ab": (12, 600, None), "gstats_ab": (15, 420, "gstats_ab.txt"), "lib_ab": (30, 900, None),
            "pick_ab": (30, 420, "pick_ab.txt"), "slab_ab": (30, 420, "slab_ab.txt"), "splat_gradient_ab": (15, 420, "splat_gradient_ab.txt"),
            "topk_ab": (30, 420, "topk_ab.txt"), "views_ab": (15, 540, "views_ab.txt")}
    own = {"frame_ab": ["default"], "lib_ab": ["--libs", "a=x.so,b=y.so", "default"]}
    assert sorted(want) == sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(TOOLS, "*_ab.py")))
    for name, (rounds, timeout, out) in want.items():
        a = _tool(name).arguments(own.get(name, []))
        assert (a.rounds, a.timeout) == (rounds, timeout), name
        assert a.out == (os.path.join(REPO, "profiles", out) if out else None), name
        assert a.camera_set == ("all" if name == "views_ab" else "single") and a.camera == 0
        assert a.label == {"topk_ab": "guarded", "slab_ab": "bypass"}.get(name)
    assert _tool("pick_ab").arguments(["--median-T", "0.25"]).median_T == 0.25
    assert _tool("splat_gradient_ab").arguments([]).channels == "3,16" and _tool("channels_ab").arguments([]).channels == "8,16,32"
    assert _tool("blend_ab").arguments(["--tile-row-step", "1,4"]).tile_row_step == "1,4"
    assert _tool("views_ab").arguments(["--dispatches", "2", "--leg", "stats-B8"]).leg == "stats-B8"


def test_report_writes_or_appends_under_the_label(tmp_path, capsys):
    out = str(tmp_path / "sub" / "x.txt")
    assert ab.report(["head", "  A: 1"], out) == "head\n  A: 1"
    assert open(out).read() == "head\n  A: 1\n" and capsys.readouterr().out == "head\n  A: 1\n"
    ab.report(["other"], out)  # overwrites
    assert open(out).read() == "other\n"
    ab.report(["head", "  A: 1"], out, "guarded", append=True)
    ab.report(["head", "  A: 2"], out, "no guard", append=True)
    assert open(out).read() == "other\n[guarded] head\n  A: 1\n[no guard] head\n  A: 2\n"
    assert capsys.readouterr().out == "other\n[guarded] head\n  A: 1\n[no guard] head\n  A: 2\n"
    ab.report(["only printed"], None)
    assert capsys.readouterr().out == "only printed\n" and os.listdir(tmp_path / "sub") == ["x.txt"]


def test_in_child_reports_the_status_and_the_time_limit():
    ab.in_child("tools/x_ab.py", 20, command=[sys.executable, "-c", "pass"])  # status 0: returns
    with pytest.raises(SystemExit) as e:
        ab.in_child("tools/x_ab.py", 20, command=[sys.executable, "-c", "import sys; sys.exit(3)"])
    assert e.value.code == "x_ab: the measurement ended with status 3"
    with pytest.raises(SystemExit) as e:
        ab.in_child("tools/x_ab.py", 1, command=["sleep", "30"])
    assert e.value.code in ("x_ab: the measurement ended with status 124 (time limit)", "x_ab: the measurement ended with status 137 (time limit)")


def test_in_child_hands_the_tool_its_own_arguments_as_a_worker(monkeypatch):
    seen = {}
    monkeypatch.setattr(ab.subprocess, "run", lambda cmd: seen.setdefault("cmd", cmd) and type("R", (), {"returncode": 0})())
    ab.in_child("tools/x_ab.py", 7, argv=["--rounds", "2"])
    assert seen["cmd"] == ["timeout", "-k", "10", "7", sys.executable, os.path.abspath("tools/x_ab.py"), "--worker", "--rounds", "2"]


def test_the_tools_leave_clocks_and_setup_to_the_harness():
    files = sorted(glob.glob(os.path.join(TOOLS, "*_ab.py")))
    assert len(files) == 12
    for path in files:
        tree = ast.parse(open(path).read(), path)
        imported = [a.name for node in ast.walk(tree) if isinstance(node, ast.Import) for a in node.names]
        assert "ab_harness" in imported, path
        names = {node.id for node in ast.walk(tree) if isinstance(node, ast.Name)} | {node.attr for node in ast.walk(tree) if isinstance(node, ast.Attribute)} \
            | {k.arg for node in ast.walk(tree) if isinstance(node, ast.Call) for k in node.keywords}
        assert not names & {"perf_counter", "enable_timing", "build_workload", "median"}, (path, names & {"perf_counter", "enable_timing", "build_workload", "median"})
        assert "bench" not in imported and "time" not in imported, path
    harness = open(os.path.join(TOOLS, "ab_harness.py")).read()
    assert all(word in harness for word in ("perf_counter", "enable_timing", "build_workload"))
    # the summary's format exists once
    assert sum(open(p).read().count("spread (max - min) / median {") for p in files + [os.path.join(TOOLS, "ab_harness.py")]) == 1
