"""CPU: gsr_blend_channels_backward / gsr_render_channels_backward are additions to ABI 0.6.0 — declared, exported and bound; no
struct or version moved; their argument checks run before any HIP call; the file-order helper of the Python backward."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import REPO

NEW = ("gsr_blend_channels_backward", "gsr_render_channels_backward")


def _header():
    return open(os.path.join(REPO, "include", "gsr.h")).read()


def test_the_two_symbols_are_declared_exported_and_bound():
    from gsr_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/gsr.h"
        assert _lib.EXPORTS.count(name) == 1, f"{name} is not (once) in _lib.EXPORTS"
        fn = getattr(_lib.lib, name)                 # AttributeError: libgsr.so does not export it
        assert fn.restype is C.c_int and len(fn.argtypes) == 11, name
        assert fn.argtypes[7] is C.c_int32 and fn.argtypes[9] is C.c_int64, name   # channels, grad_stride
    assert sorted(_lib.EXPORTS) == sorted(declared)
    flat = re.sub(r"\s+", " ", text)
    tail = (r"const GsrCamera \*cam, const GsrOptions \*opts, int64_t max_pairs, void \*workspace, size_t workspace_bytes, "
            r"const float \*grad_map , int32_t channels, float \*grad_features , int64_t grad_stride, void \*stream\);")
    assert re.search(r"int gsr_blend_channels_backward\(int64_t n, " + tail, flat)
    assert re.search(r"int gsr_render_channels_backward\(const GsrScene \*scene, " + tail, flat)


def test_the_abi_version_stays_and_its_comment_names_the_additions():
    from gsr_amd import _lib

    assert _lib.lib.gsr_version() == 600 and _lib.GSR_VERSION == 600
    m = re.search(r"#define GSR_VERSION 600 /\*(.*?)\*/", _header(), flags=re.S)
    assert m and all(name in m.group(1) for name in NEW)
    assert C.sizeof(_lib.GsrOptions) == 84 and C.sizeof(_lib.GsrStats) == 48 and C.sizeof(_lib.GsrScene) == 64


def test_the_header_states_the_contract():
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int gsr_blend_channels_backward\(", _header(), flags=re.S)
    assert m
    doc = re.sub(r"\s+\*?\s*", " ", m.group(1))
    for words in ("ADDS into grad_features", "order the adds arrive in", "grad_map must be finite", "must not alias grad_map"):
        assert words in doc, words


@pytest.mark.parametrize("entry", NEW)
def test_bad_arguments_are_refused_without_touching_a_gpu(entry):
    """Each refusal comes with its own gsr_last_error() text and before the workspace (NULL here) is even looked at.  The array
    arguments are host addresses nobody may dereference: a check that came too late would fault, not pass."""
    from gsr_amd import _lib

    fn = getattr(_lib.lib, entry)
    cam, o, sc = _lib.GsrCamera(), _lib.default_options(), _lib.GsrScene()
    cam.width, cam.height = 64, 48
    host = (C.c_float * 4)()
    p = C.addressof(host)

    def call(cam_p, opts_p, grad_map, grad_features, channels=7, stride=7):
        head = (C.byref(sc),) if entry == "gsr_render_channels_backward" else (0,)
        return fn(*head, cam_p, opts_p, 100, None, 0, grad_map, channels, grad_features, stride, None)

    def refused(rc, *words):
        err = _lib.lib.gsr_last_error().decode()
        assert rc == _lib.GSR_ERR_BAD_ARG, (entry, rc, err)
        assert all(w in err for w in words), (entry, err)
        return err

    seen = [
        refused(call(C.byref(cam), C.byref(o), None, p), "null", "gradient map"),
        refused(call(C.byref(cam), C.byref(o), p, None), "null", "feature gradient"),
        refused(call(None, C.byref(o), p, p), "null", "camera"),
        refused(call(C.byref(cam), None, p, p), "null", "options"),
        refused(call(C.byref(cam), C.byref(o), p, p, channels=0, stride=4), "channels", "0"),
        refused(call(C.byref(cam), C.byref(o), p, p, channels=_lib.GSR_MAX_FEATURE_CHANNELS + 1, stride=4096), "channels", "1025"),
        refused(call(C.byref(cam), C.byref(o), p, p, channels=7, stride=6), "grad_stride", "6"),
    ]
    b = _lib.default_options()
    b.output_dtype = 1
    seen.append(refused(call(C.byref(cam), C.byref(b), p, p), "output_dtype"))
    b = _lib.default_options()
    b.accum_dtype = 1
    seen.append(refused(call(C.byref(cam), C.byref(b), p, p), "accum_dtype"))
    assert len(set(seen)) == len(seen)  # each case its own words
    # and with everything above in order, the next check is the usual one — a null workspace (gsr_render_channels_backward: the
    # empty scene's arrays) — still no GPU
    assert "null" in refused(call(C.byref(cam), C.byref(o), p, p, channels=_lib.GSR_MAX_FEATURE_CHANNELS, stride=1 << 40), "null")
    assert "null" in refused(call(C.byref(cam), C.byref(o), p, p, channels=1, stride=1), "null")
    for w in ("gradient map", "feature gradient", "channels", "grad_stride", "output_dtype", "accum_dtype"):
        assert w not in _lib.lib.gsr_last_error().decode(), w


def test_the_new_kernel_has_a_translation_unit_of_its_own():
    csrc = os.path.join(REPO, "torch-gaussian-splatting-rasterizer_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert os.path.exists(os.path.join(csrc, "blend_channels_backward.hip"))
    assert re.search(r"^OBJS\s*=.*\bblend_channels_backward\.o\b", mk, flags=re.M)
    rule = re.search(r"^blend_channels_backward\.o:.*\n\t(.*)$", mk, flags=re.M)
    fwd = re.search(r"^blend_channels\.o:.*\n\t(.*)$", mk, flags=re.M)
    assert rule and fwd and "-fno-slp-vectorize" in rule.group(1)  # the weights' bits depend on it: the flags of blend_channels.o
    assert rule.group(1).replace("-munsafe-fp-atomics", "").split() == fwd.group(1).split()


def test_the_file_order_helper_is_the_transpose_of_the_gather():
    from gsr_amd import renderer

    gen = torch.Generator().manual_seed(1)
    buf = torch.randn((37, 5), generator=gen)
    order_t = torch.randperm(37, generator=gen)
    g = renderer.file_order_gradient(buf, order_t)
    assert g.shape == buf.shape and torch.equal(g[order_t], buf) and not torch.equal(g, buf)
    # <rows, buf> = <features, g> for rows = features.index_select(0, order_t): the gather's transpose
    f = torch.randn((37, 5), generator=gen)
    assert torch.allclose((f.index_select(0, order_t) * buf).sum(), (f * g).sum())
    assert renderer.file_order_gradient(buf, None) is buf
    v = torch.randn(37, generator=gen)
    assert torch.equal(renderer.file_order_gradient(v, order_t)[order_t], v)
