"""CPU: tools/sh_backward_timing.py — its flags on the harness, its byte count and its lines, the analysis builds it finds, and that
it leaves clocks and the bench setup to tools/ab_harness.py (in the style of tests/test_project_backward_timing.py)."""
import ast
import os

import abi_checks as abi
from conftest import REPO
from gpu_cases import _tool

TOOLS = os.path.join(REPO, "tools")
ab = _tool("ab_harness")
tool = _tool("sh_backward_timing")


def test_arguments():
    a = tool.arguments([])
    assert (a.workload, a.gaussians, a.rounds, a.camera, a.camera_set, a.label, a.timeout, a.worker) == \
        ("bicycle", 0, 15, 0, "single", None, 420, False)
    assert a.out == os.path.join(REPO, "profiles", "sh_backward_timing.txt")
    assert not hasattr(a, "early_out_T")  # the operator has no stop rule: the flag is not offered
    a = tool.arguments(["--rounds", "5", "--gaussians", "1000", "--out", "f.txt", "--worker"])
    assert (a.rounds, a.gaussians, a.out, a.worker) == (5, 1000, "f.txt", True)


def test_the_byte_count_and_the_traffic_line_character_for_character():
    assert tool.moved_bytes(1000, 0) == 12000 and tool.moved_bytes(1000, 10) == 12000 + 6120
    n, touched = 6_130_000, 2_200_000
    assert tool.moved_bytes(n, touched) == 12 * n + (12 + 192 + 2 * 192 + 2 * 12) * touched
    assert tool.traffic_line("B", 328_160_000, 0.1, 5000.0) == \
        "  B: 328.2 MB by B's count in 0.1000 ms = 3282 GB/s, 0.656 of the measured copy rate (5000 GB/s)"


def test_the_analysis_builds_have_one_rule_and_the_kernel_one_switch():
    """libgsr_shb_min<N>.so is the library with sh_backward.hip rebuilt at -DGSR_SHB_DENSE_MIN=<N>, the preprocess' flags otherwise."""
    mk = open(os.path.join(abi.CSRC, "Makefile")).read()
    assert "../../tools/libgsr_shb_min%.so:" in mk and "-ffp-contract=off -DGSR_SHB_DENSE_MIN=$* -c sh_backward.hip" in mk
    src = open(os.path.join(abi.CSRC, "sh_backward.hip")).read()
    assert "#ifndef GSR_SHB_DENSE_MIN\n#define GSR_SHB_DENSE_MIN 32 " in src
    assert "tools/libgsr_*.so" in open(os.path.join(REPO, ".gitignore")).read()
    for threshold, path in tool.variant_libraries():
        assert os.path.basename(path) == f"libgsr_shb_min{threshold}.so"


def test_the_tool_leaves_clocks_and_setup_to_the_harness():
    path = os.path.join(TOOLS, "sh_backward_timing.py")
    tree = ast.parse(open(path).read(), path)
    imported = [a.name for node in ast.walk(tree) if isinstance(node, ast.Import) for a in node.names]
    assert "ab_harness" in imported and "time" not in imported
    names = {node.id for node in ast.walk(tree) if isinstance(node, ast.Name)} | {node.attr for node in ast.walk(tree) if isinstance(node, ast.Attribute)}
    assert not names & {"perf_counter", "enable_timing", "build_workload", "median"}
    assert {"interleaved", "bench_frame", "report", "summary", "main", "gsr_sh_backward", "gsr_blend_channels_backward",
            "measured_copy_gbs", "sh_to_rgb_torch"} <= names
    assert "spread (max - min) / median {" not in open(path).read()  # the summary's format exists once, in the harness
