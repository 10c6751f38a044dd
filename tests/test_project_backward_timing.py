"""CPU: tools/project_backward_timing.py — its flags on the harness, its byte count and its lines, and that it leaves clocks and
the bench setup to tools/ab_harness.py (in the style of tests/test_ab_harness.py)."""
import ast
import importlib.util
import os
import sys

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
tool = _tool("project_backward_timing")


def test_arguments():
    a = tool.arguments([])
    assert (a.workload, a.gaussians, a.rounds, a.camera, a.camera_set, a.label, a.timeout, a.worker, a.channels) == \
        ("bicycle", 0, 15, 0, "single", None, 420, False, 3)
    assert a.out == os.path.join(REPO, "profiles", "project_backward_ab.txt")
    assert not hasattr(a, "early_out_T")  # the operator has no stop rule: the flag is not offered
    a = tool.arguments(["--channels", "16", "--rounds", "5", "--gaussians", "1000", "--out", "f.txt", "--worker"])
    assert (a.channels, a.rounds, a.gaussians, a.out, a.worker) == (16, 5, 1000, "f.txt", True)


def test_the_byte_count_and_the_traffic_line_character_for_character():
    assert tool.moved_bytes(1000, 0) == 32000 and tool.moved_bytes(1000, 10) == 32000 + 880
    n, touched = 6_130_000, 1_500_000
    assert tool.moved_bytes(n, touched) == 32 * n + 44 * touched + 44 * touched
    assert tool.traffic_line("B", 328_160_000, 0.1, 5000.0) == \
        "  B: 328.2 MB by B's count in 0.1000 ms = 3282 GB/s, 0.656 of the measured copy rate (5000 GB/s)"
    # the legs' own lines are the harness's
    assert ab.summary("B", [0.1, 0.2, 0.4])[0] == "  B: median 0.2000 ms  min 0.1000 ms  max 0.4000 ms  spread (max - min) / median 150.0 %"
    assert ab.ratios({"A": 20.0, "B": 0.1}, "A") == "B / A 0.005"


def test_the_tool_leaves_clocks_and_setup_to_the_harness():
    path = os.path.join(TOOLS, "project_backward_timing.py")
    tree = ast.parse(open(path).read(), path)
    imported = [a.name for node in ast.walk(tree) if isinstance(node, ast.Import) for a in node.names]
    assert "ab_harness" in imported and "time" not in imported
    names = {node.id for node in ast.walk(tree) if isinstance(node, ast.Name)} | {node.attr for node in ast.walk(tree) if isinstance(node, ast.Attribute)}
    assert not names & {"perf_counter", "enable_timing", "build_workload", "median"}
    assert {"interleaved", "bench_frame", "report", "summary", "main", "gsr_project_backward", "measured_copy_gbs"} <= names
    assert "spread (max - min) / median {" not in open(path).read()  # the summary's format exists once, in the harness
