"""CPU: what the test_*_abi.py files state in common about a pair of entry points added to ABI 0.6.0.  The per-entry tables —
argument positions and types, prototype tails, refusal cases and their words, header sentences, whose recipe a kernel's must
equal — stay in those files; this is the scaffold around them.  A plain module next to the tests; gsr_amd is imported inside the
functions, like in the tests that call them.  Also theirs: a Rasterizer without a workspace, for the checks a call makes before it
reaches for one."""
import ctypes as C
import os
import re
import types

from conftest import REPO

CSRC = os.path.join(REPO, "torch-gaussian-splatting-rasterizer_amd", "csrc")


def header():
    return open(os.path.join(REPO, "include", "gsr.h")).read()


def header_code():
    """include/gsr.h with its comments stripped."""
    return re.sub(r"/\*.*?\*/", "", header(), flags=re.S)


def declared_names():
    """The set of gsr_* names the header declares."""
    return set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", header_code()))


def prototypes():
    """header_code() with every run of white space collapsed: what a prototype pattern is searched in."""
    return re.sub(r"\s+", " ", header_code())


def header_comment_before(what):
    """The text of the comment that ends right before `what` (a regular expression) in include/gsr.h."""
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*" + what, header(), flags=re.S)
    assert m, what
    return m.group(1)


def assert_declared_exported_and_bound(names, n_args=None):
    """Each name is declared once in the header, stands once in _lib.EXPORTS and is bound with restype c_int (and `n_args`
    argtypes); EXPORTS is exactly what the header declares."""
    from gsr_amd import _lib

    declared = declared_names()
    for name in names:
        assert name in declared, f"{name} is not declared in include/gsr.h"
        assert _lib.EXPORTS.count(name) == 1, f"{name} is not (once) in _lib.EXPORTS"
        fn = getattr(_lib.lib, name)                 # AttributeError: libgsr.so does not export it
        assert fn.restype is C.c_int, name
        assert n_args is None or len(fn.argtypes) == n_args, name
    assert sorted(_lib.EXPORTS) == sorted(declared)


def assert_version_and_struct_sizes(names):
    """ABI 0.6.0 in the library, in _lib.py and in the header, whose version comment names the additions; no struct moved."""
    from gsr_amd import _lib

    assert _lib.lib.gsr_version() == 600 and _lib.GSR_VERSION == 600
    m = re.search(r"#define GSR_VERSION 600 /\*(.*?)\*/", header(), flags=re.S)
    assert m and all(name in m.group(1) for name in names)
    assert C.sizeof(_lib.GsrOptions) == 84 and C.sizeof(_lib.GsrStats) == 48 and C.sizeof(_lib.GsrScene) == 64
    assert C.sizeof(_lib.GsrCamera) == 4 * (16 + 16 + 3 + 6) + 8 and C.sizeof(_lib.GsrDebugOut) == 72


def refused(entry):
    """-> refused(rc, *words): rc is GSR_ERR_BAD_ARG and gsr_last_error() holds every word; returns the error text."""
    from gsr_amd import _lib

    def check(rc, *words):
        err = _lib.lib.gsr_last_error().decode()
        assert rc == _lib.GSR_ERR_BAD_ARG, (entry, rc, err)
        assert all(w in err for w in words), (entry, err)
        return err

    return check


def makefile_rule(obj):
    """(prerequisites, recipe) of the rule csrc/Makefile spells out for the object `obj`."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = re.search(rf"^{re.escape(obj)}:(.*)\n\t(.*)$", mk, flags=re.M)
    assert rule, obj
    return rule.group(1), rule.group(2)


def makefile_recipe(obj):
    return makefile_rule(obj)[1]


def assert_own_translation_unit(stem):
    """csrc/<stem>.hip exists and <stem>.o is one of the library's OBJS."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert os.path.exists(os.path.join(CSRC, stem + ".hip"))
    assert re.search(rf"^OBJS\s*=.*\b{re.escape(stem)}\.o\b", mk, flags=re.M)


class NoWorkspace(Exception):
    pass


def rasterizer(n=5, views=4, order_t=None):
    """A Rasterizer on a scene that lives nowhere: whatever reaches for a workspace or the library raises."""
    import torch

    from gsr_amd import renderer

    R = renderer.Rasterizer.__new__(renderer.Rasterizer)
    R.scene = types.SimpleNamespace(n=n, device=torch.device("cpu"), order_t=order_t)
    R.unchecked, R.sort_passes, R.max_pairs, R.views = renderer.UncheckedFrames(), 0, 1 << 20, views

    def no_workspace(*a, **k):
        raise NoWorkspace()

    R._workspace = no_workspace
    return R


def cam(w=40, h=24):
    from gsr_amd import _lib

    c = _lib.GsrCamera()
    c.width, c.height = w, h
    return c
