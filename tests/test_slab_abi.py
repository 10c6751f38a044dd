"""CPU: gsr_blend_slab / gsr_render_slab are additions to ABI 0.6.0 — declared, exported and bound with the exact signature; no struct
or version moved; their argument checks (gsr_blend_channels' cases) run before any HIP call; the kernel has a translation unit with
the channel blend's flags; Rasterizer.render_slab refuses bad limits before it makes a workspace; renderer.composite_over is the
sum it says it is."""
import ctypes as C
import os
import re

import pytest
import torch

import abi_checks as abi

NEW = ("gsr_blend_slab", "gsr_render_slab")


def test_the_two_symbols_are_declared_exported_and_bound():
    from gsr_amd import _lib

    vp = C.c_void_p
    tail = [C.POINTER(_lib.GsrCamera), C.POINTER(_lib.GsrOptions), C.c_int64, vp, C.c_size_t, vp, C.c_int32, C.c_int64, vp, vp, vp, vp, vp]
    abi.assert_declared_exported_and_bound(NEW)
    assert list(_lib.lib.gsr_blend_slab.argtypes) == [C.POINTER(_lib.GsrScene), C.c_int64] + tail
    assert list(_lib.lib.gsr_render_slab.argtypes) == [C.POINTER(_lib.GsrScene)] + tail
    flat = abi.prototypes()
    rest = (r"const GsrCamera \*cam, const GsrOptions \*opts, int64_t max_pairs, void \*workspace, size_t workspace_bytes, "
            r"const float \*features, int32_t channels, int64_t feature_stride, const float \*depth_near, const float \*depth_far, "
            r"float \*out_map, float \*out_final_T, void \*stream\);")
    assert re.search(r"int gsr_blend_slab\(const GsrScene \*scene , int64_t n, " + rest, flat)
    assert re.search(r"int gsr_render_slab\(const GsrScene \*scene, " + rest, flat)


def test_the_abi_version_stays_and_its_comment_names_the_additions():
    abi.assert_version_and_struct_sizes(NEW)


def test_the_header_states_the_two_compares_the_depth_and_nan():
    doc = abi.header_comment_before(r"int gsr_blend_slab\(")
    flat = re.sub(r"[\s*]+", " ", doc)
    assert "depth_near[p] <= z_i and z_i < depth_far[p]" in flat
    assert ">= on the near side, < on the far side" in flat
    assert "((x w2c[2] + y w2c[6]) + z w2c[10]) + w2c[14]" in flat and "without fused multiply-adds" in flat
    assert "GsrDebugOut.cam_means[3 i + 2]" in flat
    assert "CAMERA-SPACE LINEAR DEPTH" in flat and "not NDC" in flat
    assert "NaN, or depth_far[p] <= depth_near[p], the pixel draws nothing: its map is 0 and its T is 1" in flat
    assert "SKIPPED, not blended" in flat


@pytest.mark.parametrize("entry", NEW)
def test_bad_arguments_are_refused_without_touching_a_gpu(entry):
    """gsr_blend_channels' cases, each with its own gsr_last_error() text, before the workspace (NULL here) is even looked at.  The
    array arguments are host addresses nobody may dereference: a check that came too late would fault, not pass."""
    from gsr_amd import _lib

    fn = getattr(_lib.lib, entry)
    cam, o, sc = _lib.GsrCamera(), _lib.default_options(), _lib.GsrScene()
    cam.width, cam.height = 64, 48
    host = (C.c_float * 4)()
    p = C.addressof(host)

    def call(cam_p, opts_p, features=p, channels=3, stride=3, near=None, far=None, out=p, scene=True):
        head = (C.byref(sc),) if entry == "gsr_render_slab" else (C.byref(sc) if scene else None, 0)
        return fn(*head, cam_p, opts_p, 100, None, 0, features, channels, stride, near, far, out, p, None)

    refused = abi.refused(entry)

    seen = [
        refused(call(None, C.byref(o)), "null", "camera"),
        refused(call(C.byref(cam), None), "null", "options"),
        refused(call(C.byref(cam), C.byref(o), features=None), "null", "features"),
        refused(call(C.byref(cam), C.byref(o), out=None), "null", "output map"),
    ]
    for bad in (0, -1, _lib.GSR_MAX_FEATURE_CHANNELS + 1):
        assert str(bad) in refused(call(C.byref(cam), C.byref(o), channels=bad, stride=2000), "bad channels")
    seen.append(_lib.lib.gsr_last_error().decode())
    seen.append(refused(call(C.byref(cam), C.byref(o), channels=5, stride=4), "feature_stride", "4"))
    b = _lib.default_options()
    b.output_dtype = 1
    seen.append(refused(call(C.byref(cam), C.byref(b)), "output_dtype"))
    b = _lib.default_options()
    b.accum_dtype = 1
    seen.append(refused(call(C.byref(cam), C.byref(b)), "accum_dtype"))
    assert len(set(seen)) == len(seen)  # each case its own words
    # and with everything above in order — either limit, both, neither, the widest map, a wider stride — the next check is the usual
    # one: a null workspace (still no GPU)
    for kw in (dict(), dict(near=p), dict(far=p), dict(near=p, far=p), dict(channels=1, stride=1), dict(channels=5, stride=64),
               dict(channels=_lib.GSR_MAX_FEATURE_CHANNELS, stride=_lib.GSR_MAX_FEATURE_CHANNELS)):
        assert "null" in refused(call(C.byref(cam), C.byref(o), **kw), "null", "workspace"), kw
    if entry == "gsr_blend_slab":  # the scene is optional there, but one that is given must be this frame's
        assert "null" in refused(call(C.byref(cam), C.byref(o), scene=False), "null", "workspace")
        sc.n = 5
        refused(call(C.byref(cam), C.byref(o)), "scene")
        sc.n = 0


def test_the_new_kernel_has_a_translation_unit_with_the_channel_blends_flags():
    abi.assert_own_translation_unit("blend_slab")
    rule, chan = abi.makefile_recipe("blend_slab.o"), abi.makefile_recipe("blend_channels.o")
    assert "-fno-slp-vectorize" in rule  # the maps' bits depend on it
    assert rule == chan
    src = open(os.path.join(abi.CSRC, "blend_slab.hip")).read()
    for width in (4, 8, 16):
        assert re.search(rf"launch_width<{width}>\(", src), width


def test_render_slab_refuses_bad_limits_and_gradients_before_anything_else():
    """(A scene on the CPU is enough: the checks come before the workspace is made, and before the features are looked at.)"""
    from gsr_amd import renderer

    class _NoScene:
        n, device, order_t = 0, torch.device("cpu"), None

    R = renderer.Rasterizer(_NoScene())
    cam = renderer.GsrCamera()
    cam.width, cam.height = 40, 24
    f = torch.zeros((0, 3))
    ok = torch.zeros((24, 40))
    for name in ("near", "far"):
        for bad in (torch.zeros((40, 24)), torch.zeros((24, 40, 1)), torch.zeros((24, 39)), torch.zeros(24 * 40)):
            with pytest.raises(ValueError, match=f"{name} must be a float32 tensor of shape"):
                R.render_slab(cam, f, **{name: bad})
        for bad in (ok.double(), ok.half(), ok.int(), 1.5, ok.numpy()):
            with pytest.raises(ValueError, match=f"{name} must be a float32 tensor of shape"):
                R.render_slab(cam, f, **{name: bad})
        with pytest.raises(ValueError, match=f"{name} must live on the scene's device"):
            R.render_slab(cam, f, **{name: torch.zeros((24, 40), device="meta")})
    # the limits follow the layout of the final T: [W, H] planes for output_layout = 1, strips for 2
    with pytest.raises(ValueError, match="far must be a float32 tensor of shape"):
        R.render_slab(cam, f, far=ok, opts=renderer.make_options(output_layout=1))
    with pytest.raises(ValueError, match="near must be a float32 tensor of shape"):
        R.render_slab(cam, f, near=ok, opts=renderer.make_options(output_layout=2, tile_row_begin=1, tile_row_step=2))
    with pytest.raises(ValueError, match="no backward"):
        R.render_slab(cam, torch.zeros((0, 3), requires_grad=True), far=ok)
    assert R._ws is None  # nothing was allocated on the way
    assert "NO BACKWARD" in renderer.Rasterizer.render_slab.__doc__


def test_composite_over_against_float64():
    from gsr_amd.renderer import composite_over

    gen = torch.Generator().manual_seed(11)
    H, W, Cn = 9, 7, 5
    m = torch.randn((H, W, Cn), generator=gen)
    T = torch.rand((H, W), generator=gen)
    T[0, 0], T[1, 1] = 0.0, 1.0
    for bg in (torch.randn(Cn, generator=gen), torch.randn((H, W, Cn), generator=gen)):
        out = composite_over(m, T, bg)
        ref = m.double() + T.double().unsqueeze(-1) * bg.double()
        assert out.shape == (H, W, Cn) and out.dtype == torch.float32
        # one product and one sum, each rounded once in fp32: 2^-24 relative per operation on magnitudes |m| + |T bg|
        bound = 2.0 ** -23 * (m.double().abs() + (T.double().unsqueeze(-1) * bg.double()).abs())
        assert bool(((out.double() - ref).abs() <= bound).all())
        assert torch.equal(out[0, 0], m[0, 0])                           # T = 0: the map alone
        assert torch.equal(out[1, 1], m[1, 1] + bg[1, 1] if bg.dim() == 3 else m[1, 1] + bg)
    assert torch.equal(composite_over(m, T, [0.0] * Cn), m)
    for bad in (torch.zeros(Cn + 1), torch.zeros((H, W)), torch.zeros((W, H, Cn))):
        with pytest.raises(ValueError):
            composite_over(m, T, bad)
    with pytest.raises(ValueError):
        composite_over(m, T.t(), torch.zeros(Cn))
    bg = torch.randn(Cn, generator=gen, requires_grad=True)
    (g,) = torch.autograd.grad(composite_over(m, T, bg).sum(), bg)
    assert torch.allclose(g, T.sum().expand(Cn))
