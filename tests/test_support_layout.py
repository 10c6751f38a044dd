"""CPU: where the tests' shared material lives.  Scenes, cases and references that more than one test file uses are in
tests/gpu_cases.py, the check bodies the backward tests share between cameras in tests/backward_cases.py, the scaffold of the
test_*_abi.py files in tests/abi_checks.py; no test module is another's library, and
nothing under tests/ but conftest.py arranges the import path."""
import ast
import glob
import importlib.util
import os
import subprocess
import sys

from conftest import REPO

TESTS = os.path.join(REPO, "tests")


def test_no_test_module_is_imported_and_only_conftest_touches_the_path():
    files = sorted(glob.glob(os.path.join(TESTS, "*.py")))
    assert len(files) > 30 and os.path.join(TESTS, "gpu_cases.py") in files
    for path in files:
        name = os.path.basename(path)
        for node in ast.walk(ast.parse(open(path).read(), path)):
            imported = ([a.name for a in node.names] if isinstance(node, ast.Import) else
                        [node.module or ""] if isinstance(node, ast.ImportFrom) else [])
            for module in imported:
                assert not module.split(".")[-1].startswith("test_"), f"{name} imports {module}"
            if isinstance(node, ast.Call) and name != "conftest.py":
                assert ast.unparse(node.func) != "sys.path.insert", f"{name} line {node.lineno} calls sys.path.insert"


def test_the_fuzz_tool_and_the_tests_build_a_case_with_one_function():
    import gpu_cases

    spec = importlib.util.spec_from_file_location("fuzz_parity_by_path", os.path.join(REPO, "tools", "fuzz_parity.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.build_case is gpu_cases.fuzz_case  # (both are tools/fuzz_scene.build_case: the tools need no file of tests/ for it)
    # ... and importing gpu_cases takes no torch: asked of a fresh interpreter, since this one has long imported it
    code = "import sys, gpu_cases; assert 'torch' not in sys.modules and 'gsr_amd' not in sys.modules"
    r = subprocess.run([sys.executable, "-c", code], cwd=TESTS, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
