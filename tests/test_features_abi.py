"""CPU: gsr_blend_features / gsr_render_features are additions to ABI 0.6.0 — declared, exported and bound; no struct or
version moved; their argument checks run before any HIP call."""
import ctypes as C
import os
import re

import pytest

import abi_checks as abi
from conftest import REPO

NEW = ("gsr_blend_features", "gsr_render_features")


def test_the_two_symbols_are_declared_exported_and_bound():
    abi.assert_declared_exported_and_bound(NEW, 10)
    # the parameter lists the issue gives: (n, cam, opts, max_pairs, workspace, bytes, features, out_map, out_final_T, stream) and the
    # same with the scene in the place of n
    flat = abi.prototypes()
    assert re.search(r"int gsr_blend_features\(int64_t n, const GsrCamera \*cam, const GsrOptions \*opts, int64_t max_pairs, void \*workspace, "
                     r"size_t workspace_bytes, const float \*features , float \*out_map, float \*out_final_T, void \*stream\);", flat)
    assert re.search(r"int gsr_render_features\(const GsrScene \*scene, const GsrCamera \*cam, const GsrOptions \*opts, int64_t max_pairs, "
                     r"void \*workspace, size_t workspace_bytes, const float \*features , float \*out_map, float \*out_final_T, void \*stream\);", flat)


def test_the_abi_version_and_every_struct_stay_where_they_were():
    from gsr_amd import _lib

    abi.assert_version_and_struct_sizes(NEW)  # (the additions are recorded in the version's comment)
    assert re.search(r"#define GSR_VERSION 600\b", abi.header())
    # test_abi.test_struct_sizes_match_header, restated: the feature adds no field anywhere
    assert C.sizeof(_lib.GsrScene) == 64 and _lib.GsrScene.block_bounds.offset == 56
    assert C.sizeof(_lib.GsrCamera) == 4 * (16 + 16 + 3 + 6) + 8
    assert C.sizeof(_lib.GsrOptions) == 84 and _lib.GsrOptions.tile_row_block.offset == 80 and _lib.GsrOptions.batch_views.offset == 76
    assert _lib.GsrOptions.keep_flags.offset == 44 and _lib.GsrOptions.accum_dtype.offset == 40 and _lib.GsrOptions.saturation_rule.offset == 48
    assert _lib.GsrOptions.sh_dense_min.offset == 72 and _lib.GsrOptions.colour_stage.offset == 68 and _lib.GsrOptions.no_order_hint.offset == 64
    assert C.sizeof(_lib.GsrStats) == 48 and _lib.GsrStats.colour_evals.offset == 40 and _lib.GsrStats.wave_entries.offset == 24
    assert _lib.GsrStats.fetched_entries.offset == 32 and C.sizeof(_lib.GsrDebugOut) == 72


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

    def call(cam_p, opts_p, features, out_map):
        head = (C.byref(sc),) if entry == "gsr_render_features" else (0,)
        return fn(*head, cam_p, opts_p, 100, None, 0, features, out_map, None, None)

    refused = abi.refused(entry)

    refused(call(C.byref(cam), C.byref(o), None, p), "null", "features")
    refused(call(C.byref(cam), C.byref(o), p, None), "null", "output map")
    refused(call(None, C.byref(o), p, p), "null", "camera")
    refused(call(C.byref(cam), None, p, p), "null", "options")
    b = _lib.default_options()
    b.output_dtype = 1
    refused(call(C.byref(cam), C.byref(b), p, p), "output_dtype")
    b = _lib.default_options()
    b.accum_dtype = 1
    refused(call(C.byref(cam), C.byref(b), p, p), "accum_dtype")
    # and with everything above in order, the next check is the usual one (a null workspace) — still no GPU
    refused(call(C.byref(cam), C.byref(o), p, p), "null")


def test_python_surface_exists_and_the_product_still_never_imports_the_oracle():
    import inspect

    from gsr_amd import rasterize, renderer

    for name in ("render_features", "render_depth", "render_rgbd"):
        assert callable(getattr(renderer.Rasterizer, name)), name
    sig = inspect.signature(renderer.Rasterizer.render_features)
    assert list(sig.parameters)[1:] == ["cam", "features", "opts", "return_T", "scene_order"]
    assert sig.parameters["return_T"].default is False and sig.parameters["scene_order"].default is False
    assert inspect.signature(renderer.Rasterizer.render_depth).parameters["normalize"].default is False
    assert inspect.signature(rasterize.render_scene).parameters["with_depth"].default is False
    pkg = os.path.join(REPO, "torch-gaussian-splatting-rasterizer_amd")
    seen = []
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(root, f)).read()
                seen.append(f)
                assert "cpu_oracle" not in text and "gsr_oracle" not in text and "torch_loop" not in text, f
                assert not re.search(r"^\s*(from|import)\s+oracle", text, flags=re.M), f
    assert "blend_features.hip" in seen and "blend_common.h" in seen
