"""CPU: tools/camera_backward_timing.py — its flags on the harness, its byte count and its lines, and that it leaves clocks and the
bench setup to tools/ab_harness.py (in the style of tests/test_sh_backward_timing.py)."""
import ast
import os

from conftest import REPO
from gpu_cases import _tool

TOOLS = os.path.join(REPO, "tools")
ab = _tool("ab_harness")
tool = _tool("camera_backward_timing")


def test_arguments():
    a = tool.arguments([])
    assert (a.workload, a.gaussians, a.rounds, a.camera, a.camera_set, a.label, a.timeout, a.worker, a.channels) == \
        ("bicycle", 0, 15, 0, "single", None, 420, False, 3)
    assert a.out == os.path.join(REPO, "profiles", "camera_backward_timing.txt")
    assert not hasattr(a, "early_out_T")  # the operator has no stop rule: the flag is not offered
    a = tool.arguments(["--channels", "16", "--rounds", "5", "--gaussians", "1000", "--out", "f.txt", "--worker"])
    assert (a.channels, a.rounds, a.gaussians, a.out, a.worker) == (16, 5, 1000, "f.txt", True)


def test_the_byte_count_and_the_traffic_line_character_for_character():
    assert tool.moved_bytes(1000, 0, 256) == 32000 + 512 and tool.moved_bytes(1000, 10, 256) == 32000 + 400 + 512
    n, touched = 6_130_000, 1_500_000
    assert tool.moved_bytes(n, touched, 768 * 256) == 32 * n + (12 + 12 + 16) * touched + 2 * 768 * 256
    assert tool.traffic_line("B", 328_160_000, 0.1, 5000.0) == \
        "  B: 328.2 MB by B's count in 0.1000 ms = 3282 GB/s, 0.656 of the measured copy rate (5000 GB/s)"
    # the legs' own lines are the harness's
    assert ab.summary("B", [0.1, 0.2, 0.4])[0] == "  B: median 0.2000 ms  min 0.1000 ms  max 0.4000 ms  spread (max - min) / median 150.0 %"
    assert ab.ratios({"A": 20.0, "B": 0.1, "C": 0.05}, "C", ["B"]) == "B / C 2.000"


def test_the_tool_leaves_clocks_and_setup_to_the_harness():
    path = os.path.join(TOOLS, "camera_backward_timing.py")
    tree = ast.parse(open(path).read(), path)
    imported = [a.name for node in ast.walk(tree) if isinstance(node, ast.Import) for a in node.names]
    assert "ab_harness" in imported and "time" not in imported
    names = {node.id for node in ast.walk(tree) if isinstance(node, ast.Name)} | {node.attr for node in ast.walk(tree) if isinstance(node, ast.Attribute)}
    assert not names & {"perf_counter", "enable_timing", "build_workload", "median"}
    assert {"interleaved", "bench_frame", "report", "summary", "main", "gsr_camera_backward", "gsr_project_backward", "gsr_blend_splat_backward",
            "measured_copy_gbs", "project64", "gsr_camera_backward_bytes"} <= names
    assert "spread (max - min) / median {" not in open(path).read()  # the summary's format exists once, in the harness
    assert not os.path.basename(path).endswith("_ab.py")  # tests/test_ab_harness.py counts those
