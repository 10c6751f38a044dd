"""GPU: every tools/*_ab.py end to end on the harness, its worker called in this process on the bench frame
with 20 000 gaussians and 2 rounds: one line per leg in the documented order, counters that count, every bit-identity and agreement
flag True, and an out-file that holds what was printed.  No timing is asserted at this size."""
import importlib.util
import os
import re
import sys

import pytest
from conftest import REPO

pytestmark = pytest.mark.gpu

TOOLS = os.path.join(REPO, "tools")
SUMMARY = re.compile(r"^  (\S.*?) *: median \d+\.\d{4} ms  min \d+\.\d{4} ms  max \d+\.\d{4} ms  spread \(max - min\) / median \d+\.\d %")
FRAME = re.compile(r"^(\S+(?: +[ab])?) +preprocess \d+\.\d{4}  bin_sort \d+\.\d{4}")  # the whole-frame tools' own line: variant [build]
COUNTER = re.compile(r"\b(wave_entries|fetched_entries|colour_evals|fetched|evaluated|D|E) (\d+)\b")
AB, CH = ["A", "B"], ["--channels", "3,16"]

#  tool: (its own arguments, the legs in order, the flags that must read True and how often)
CASES = {
    "blend_ab": ([], ["rows 0/1 impl 0", "rows 0/1 impl 1"], {"frame == impl 0": 2}),
    "channels_ab": (CH, AB + AB, {"counters agree": 2, "maps agree bit for bit": 2}),
    "channels_backward_ab": (CH, AB + AB, {"counters agree": 2}),
    "features_ab": ([], AB + ["render", "render_depth", "render_rgbd"], {"counters agree": 1, "final T of B == final T of A": 1}),
    "frame_ab": (["default"], ["default"], {"== default": 1}),
    # (gstats_ab's "B's counters are A's" is no such flag: the statistics walk skips what the mask or a full pixel leaves no use for)
    "gstats_ab": ([], list("abcdABCD"), {}),
    "lib_ab": (["--libs", "a={lib},b={lib}", "default"], ["default    a", "default    b"], {"== a": 2}),
    "pick_ab": ([], list("ABC"), {"C's counters are A's": 1, "B's ids and weights == C's": 1}),
    "slab_ab": ([], ["A", "A8", "A16", "B4", "B8", "B16", "C", "D"], {"B's maps and T == A's": 1, "B's counters are A's": 1}),
    "splat_gradient_ab": (CH, AB + AB, {"counters agree": 2, "finite": 2}),
    "topk_ab": ([], list("ABCDEF"), {"E's counters are A's": 1, "C's lists == E's": 1, "B's == the first 4 slots of C's": 1}),
    "views_ab": (["--camera-set", "all"], [f"{kind}-{leg}" for leg in ("A", "B4", "B8") for kind in ("forward", "backward", "stats")], {}),
}
# the one counter that is 0 where these two tools read it: their lists carry evaluated colours or none, so the blend defers none
NO_DEFERRED_COLOUR = ("features_ab", "pick_ab")


def _tool(name):
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(TOOLS, name + ".py"))
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        spec.loader.exec_module(module)
    return sys.modules[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_tool_on_the_harness(name, gsr, tmp_path, capsys):
    from gsr_amd import _lib

    _tool("ab_harness")
    tool = _tool(name)
    own, legs, flags = CASES[name]
    out = str(tmp_path / (name + ".txt"))
    argv = ["--workload", "bicycle", "--gaussians", "20000", "--rounds", "2", "--out", out] + [x.format(lib=_lib.LIB_PATH) for x in own]
    tool.worker(tool.arguments(argv))
    text = capsys.readouterr().out
    print(text)
    assert open(out).read() == text  # the out-file holds exactly what was printed

    leg_lines = [(m.group(1), line) for line in text.splitlines() for m in [SUMMARY.match(line) or FRAME.match(line)] if m]
    assert [k for k, _ in leg_lines] == legs
    for leg, line in leg_lines:
        counters = COUNTER.findall(line)
        if name not in ("views_ab",) and leg not in ("render", "render_depth", "render_rgbd"):  # whole calls over many frames carry none
            assert {k for k, _ in counters} >= ({"fetched", "evaluated"} if FRAME.match(line) else {"wave_entries", "fetched_entries"}), line
        for k, v in counters:
            if k == "colour_evals" and name in NO_DEFERRED_COLOUR:
                assert int(v) == 0, line
            else:
                assert int(v) > 0, line
    for flag, count in flags.items():
        found = re.findall(re.escape(flag) + r":? (True|False)", text)
        assert found == ["True"] * count, (flag, found)
    listed = sum(flags.values())
    others = len(re.findall(r"\b(True|False)\b", text)) - listed
    # the flags not listed are verdicts on times (a gate, "faster by more than", "median <="), which nothing here holds at this size
    assert others == {"channels_ab": 2, "gstats_ab": 2, "pick_ab": 1}.get(name, 0), text
