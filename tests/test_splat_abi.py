"""CPU: gsr_blend_splat_backward / gsr_render_splat_backward are additions to ABI 0.6.0 — declared, exported and bound; no struct
or version moved; their argument checks run before any HIP call; the kernel has a translation unit of its own; the host helpers
that need no GPU."""
import ctypes as C
import re

import pytest
import torch

import abi_checks as abi

NEW = ("gsr_blend_splat_backward", "gsr_render_splat_backward")


def test_the_two_symbols_are_declared_exported_and_bound():
    from gsr_amd import _lib

    abi.assert_declared_exported_and_bound(NEW, 15)
    for name in NEW:
        fn = getattr(_lib.lib, name)
        assert fn.argtypes[7] is C.c_int64 and fn.argtypes[8] is C.c_int32, name      # feature_stride, channels
        assert fn.argtypes[11] is C.c_float and fn.argtypes[12] is C.c_int32, name    # min_T, want_abs
    flat = abi.prototypes()
    tail = (r"const GsrCamera \*cam, const GsrOptions \*opts, int64_t max_pairs, void \*workspace, size_t workspace_bytes, "
            r"const float \*features , int64_t feature_stride, int32_t channels, const float \*grad_map , const float \*grad_T , "
            r"float min_T, int32_t want_abs, float \*grad_splat , void \*stream\);")
    assert re.search(r"int gsr_blend_splat_backward\(int64_t n, " + tail, flat)
    assert re.search(r"int gsr_render_splat_backward\(const GsrScene \*scene, " + tail, flat)


def test_the_abi_version_stays_and_its_comment_names_the_additions():
    abi.assert_version_and_struct_sizes(NEW)


def test_the_header_states_the_contract():
    doc = re.sub(r"\s+\*?\s*", " ", abi.header_comment_before(r"int gsr_blend_splat_backward\("))
    for words in ("ADDS into grad_splat", "order the adds arrive in", "must be finite", "must not alias", "layout per opts->output_layout",
                  "undrawn last column / row", "columns 6 and 7 are not touched", "cap has derivative 0", "Means are in pixels",
                  "2^-24 |S'| alpha / (1 - alpha)", "describes the second walk", "Single views"):
        assert words in doc, words


@pytest.mark.parametrize("entry", NEW)
def test_bad_arguments_are_refused_without_touching_a_gpu(entry):
    """Each refusal comes with its own gsr_last_error() text and before the workspace (NULL here) is even looked at.  The array
    arguments are host addresses nobody may dereference: a check that came too late would fault, not pass."""
    from gsr_amd import _lib

    fn = getattr(_lib.lib, entry)
    cam, o, sc = _lib.GsrCamera(), _lib.default_options(), _lib.GsrScene()
    cam.width, cam.height = 64, 48
    host = (C.c_float * 8)()
    p = C.addressof(host)

    def call(cam_p, opts_p, features=p, grad_map=p, grad_splat=p, channels=7, stride=7, grad_T=None, min_T=0.0, want_abs=0):
        head = (C.byref(sc),) if entry == "gsr_render_splat_backward" else (0,)
        return fn(*head, cam_p, opts_p, 100, None, 0, features, stride, channels, grad_map, grad_T, min_T, want_abs, grad_splat, None)

    refused = abi.refused(entry)
    cp, op = C.byref(cam), C.byref(o)
    seen = [
        refused(call(cp, op, features=None), "null", "features"),
        refused(call(cp, op, grad_map=None), "null", "gradient map"),
        refused(call(cp, op, grad_splat=None), "null", "splat gradient"),
        refused(call(None, op), "null", "camera"),
        refused(call(cp, None), "null", "options"),
        refused(call(cp, op, channels=0, stride=4), "channels", "0"),
        refused(call(cp, op, channels=_lib.GSR_MAX_FEATURE_CHANNELS + 1, stride=4096), "channels", "1025"),
        refused(call(cp, op, channels=7, stride=6), "feature_stride", "6"),
        refused(call(cp, op, min_T=-1e-3), "min_T", "-0.001"),
        refused(call(cp, op, min_T=float("nan")), "min_T", "nan"),
        refused(call(cp, op, min_T=float("inf")), "min_T", "inf"),
        refused(call(cp, op, channels=17, stride=17, want_abs=1), "want_abs", "17"),
    ]
    b = _lib.default_options()
    b.output_dtype = 1
    seen.append(refused(call(cp, C.byref(b)), "output_dtype"))
    b = _lib.default_options()
    b.accum_dtype = 1
    seen.append(refused(call(cp, C.byref(b)), "accum_dtype"))
    assert len(set(seen)) == len(seen)  # each case its own words
    # and with everything above in order, the next check is the usual one — a null workspace (gsr_render_splat_backward: the empty
    # scene's arrays) — still no GPU.  grad_T may be NULL or not, want_abs is fine at 16 channels, min_T at any finite value >= 0
    for kw in (dict(channels=_lib.GSR_MAX_FEATURE_CHANNELS, stride=1 << 40), dict(channels=1, stride=1), dict(grad_T=p),
               dict(channels=16, stride=16, want_abs=1), dict(min_T=1e-4), dict(min_T=3e38)):
        assert "null" in refused(call(cp, op, **kw), "null"), kw
        for w in ("features", "gradient map", "splat gradient", "channels", "feature_stride", "min_T", "want_abs", "output_dtype", "accum_dtype"):
            assert w not in _lib.lib.gsr_last_error().decode(), (kw, w)


def test_the_new_kernel_has_a_translation_unit_of_its_own():
    abi.assert_own_translation_unit("blend_splat_backward")
    rule, fwd = abi.makefile_recipe("blend_splat_backward.o"), abi.makefile_recipe("blend_channels.o")
    assert "-fno-slp-vectorize" in rule  # the weights' bits depend on it: the flags of blend_channels.o
    assert rule.split() == fwd.split()
    assert "blend_weight_walk.h" in abi.makefile_rule("blend_splat_backward.o")[0] or "$(WALK_HDRS)" in abi.makefile_rule("blend_splat_backward.o")[0]


def test_the_host_side_names_and_the_logit_chain():
    from gsr_amd import renderer

    assert renderer.SplatGradient._fields == ("mean2d", "sigmas", "opacity", "abs_mean2d")
    assert callable(renderer.Rasterizer.splat_gradient)

    class Scene:  # what opacity_logit_gradient reads of a GaussianScene
        pass

    gen = torch.Generator().manual_seed(3)
    sc = Scene()
    sc.t = {"opacity_logit": torch.randn(29, generator=gen, dtype=torch.float64)}
    sc.order_t = torch.randperm(29, generator=gen)
    g_scene = torch.randn(29, generator=gen, dtype=torch.float64)
    o = torch.sigmoid(sc.t["opacity_logit"])
    want_scene = g_scene * o * (1 - o)
    grad = lambda v: renderer.SplatGradient(None, None, v, None)
    assert torch.allclose(renderer.opacity_logit_gradient(sc, grad(g_scene), scene_order=True), want_scene, rtol=1e-14, atol=0)
    in_file = renderer.file_order_gradient(g_scene, sc.order_t)
    got = renderer.opacity_logit_gradient(sc, grad(in_file))
    assert torch.allclose(got, renderer.file_order_gradient(want_scene, sc.order_t), rtol=1e-14, atol=0)
    # against autograd through the activation
    x = sc.t["opacity_logit"].clone().requires_grad_(True)
    (torch.sigmoid(x) * g_scene).sum().backward()
    assert torch.allclose(x.grad, want_scene, rtol=1e-12, atol=0)
