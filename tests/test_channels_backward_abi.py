"""CPU: gsr_blend_channels_backward / gsr_render_channels_backward are additions to ABI 0.6.0 — declared, exported and bound; no
struct or version moved; their argument checks run before any HIP call; the file-order helper of the Python backward."""
import ctypes as C
import re

import pytest
import torch

import abi_checks as abi

NEW = ("gsr_blend_channels_backward", "gsr_render_channels_backward")


def test_the_two_symbols_are_declared_exported_and_bound():
    from gsr_amd import _lib

    abi.assert_declared_exported_and_bound(NEW, 11)
    for name in NEW:
        fn = getattr(_lib.lib, name)
        assert fn.argtypes[7] is C.c_int32 and fn.argtypes[9] is C.c_int64, name   # channels, grad_stride
    flat = abi.prototypes()
    tail = (r"const GsrCamera \*cam, const GsrOptions \*opts, int64_t max_pairs, void \*workspace, size_t workspace_bytes, "
            r"const float \*grad_map , int32_t channels, float \*grad_features , int64_t grad_stride, void \*stream\);")
    assert re.search(r"int gsr_blend_channels_backward\(int64_t n, " + tail, flat)
    assert re.search(r"int gsr_render_channels_backward\(const GsrScene \*scene, " + tail, flat)


def test_the_abi_version_stays_and_its_comment_names_the_additions():
    abi.assert_version_and_struct_sizes(NEW)


def test_the_header_states_the_contract():
    doc = re.sub(r"\s+\*?\s*", " ", abi.header_comment_before(r"int gsr_blend_channels_backward\("))
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

    refused = abi.refused(entry)

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
    abi.assert_own_translation_unit("blend_channels_backward")
    rule, fwd = abi.makefile_recipe("blend_channels_backward.o"), abi.makefile_recipe("blend_channels.o")
    assert "-fno-slp-vectorize" in rule  # the weights' bits depend on it: the flags of blend_channels.o
    assert rule.replace("-munsafe-fp-atomics", "").split() == fwd.split()


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
