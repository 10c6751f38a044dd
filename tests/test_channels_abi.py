"""CPU: gsr_blend_channels / gsr_render_channels are additions to ABI 0.6.0 — declared, exported and bound; no struct or version
moved; their argument checks run before any HIP call."""
import ctypes as C
import re

import pytest

import abi_checks as abi

NEW = ("gsr_blend_channels", "gsr_render_channels")


def test_the_two_symbols_are_declared_exported_and_bound():
    from gsr_amd import _lib

    abi.assert_declared_exported_and_bound(NEW, 12)
    for name in NEW:
        fn = getattr(_lib.lib, name)
        assert fn.argtypes[7] is C.c_int32 and fn.argtypes[8] is C.c_int64, name   # channels, feature_stride
    flat = abi.prototypes()
    tail = (r"const GsrCamera \*cam, const GsrOptions \*opts, int64_t max_pairs, void \*workspace, size_t workspace_bytes, "
            r"const float \*features , int32_t channels, int64_t feature_stride, float \*out_map , float \*out_final_T, void \*stream\);")
    assert re.search(r"int gsr_blend_channels\(int64_t n, " + tail, flat)
    assert re.search(r"int gsr_render_channels\(const GsrScene \*scene, " + tail, flat)
    assert re.search(r"#define GSR_MAX_FEATURE_CHANNELS 1024\b", abi.header()) and _lib.GSR_MAX_FEATURE_CHANNELS == 1024


def test_the_abi_version_stays_and_its_comment_names_the_additions():
    abi.assert_version_and_struct_sizes(NEW)


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

    def call(cam_p, opts_p, features, out_map, channels=7, stride=7):
        head = (C.byref(sc),) if entry == "gsr_render_channels" else (0,)
        return fn(*head, cam_p, opts_p, 100, None, 0, features, channels, stride, out_map, None, None)

    refused = abi.refused(entry)

    seen = [
        refused(call(C.byref(cam), C.byref(o), None, p), "null", "features"),
        refused(call(C.byref(cam), C.byref(o), p, None), "null", "output map"),
        refused(call(None, C.byref(o), p, p), "null", "camera"),
        refused(call(C.byref(cam), None, p, p), "null", "options"),
        refused(call(C.byref(cam), C.byref(o), p, p, channels=0, stride=4), "channels", "0"),
        refused(call(C.byref(cam), C.byref(o), p, p, channels=_lib.GSR_MAX_FEATURE_CHANNELS + 1, stride=4096), "channels", "1025"),
        refused(call(C.byref(cam), C.byref(o), p, p, channels=7, stride=6), "feature_stride", "6"),
    ]
    b = _lib.default_options()
    b.output_dtype = 1
    seen.append(refused(call(C.byref(cam), C.byref(b), p, p), "output_dtype"))
    b = _lib.default_options()
    b.accum_dtype = 1
    seen.append(refused(call(C.byref(cam), C.byref(b), p, p), "accum_dtype"))
    assert len(set(seen)) == len(seen)  # each case its own words
    # and with everything above in order (the widest map, rows further apart than wide), the next check is the usual one — a null
    # workspace (gsr_render_channels: the empty scene's arrays) — still no GPU
    assert "null" in refused(call(C.byref(cam), C.byref(o), p, p, channels=_lib.GSR_MAX_FEATURE_CHANNELS, stride=1 << 40), "null")
    assert "null" in refused(call(C.byref(cam), C.byref(o), p, p, channels=1, stride=1), "null")
    for w in ("features", "output map", "channels", "feature_stride", "output_dtype", "accum_dtype"):
        assert w not in _lib.lib.gsr_last_error().decode(), w


def test_the_new_kernel_has_a_translation_unit_of_its_own():
    abi.assert_own_translation_unit("blend_channels")
    assert "-fno-slp-vectorize" in abi.makefile_recipe("blend_channels.o")  # the bits depend on it: the flags of blend_features.o
