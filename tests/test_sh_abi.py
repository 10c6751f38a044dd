"""CPU: gsr_sh_backward is an addition to ABI 0.6.0 — declared, exported and bound; no struct or version moved; its argument
checks run before any HIP call; the kernel has a translation unit of its own, built with the preprocess' flags, that cross-compiles
for gfx950 without scratch; the host names."""
import ctypes as C
import os
import re
import subprocess

import abi_checks as abi

NEW = ("gsr_sh_backward",)


def test_the_symbol_is_declared_exported_and_bound():
    from gsr_amd import _lib

    abi.assert_declared_exported_and_bound(NEW, 7)
    fn = _lib.lib.gsr_sh_backward
    assert fn.argtypes[0]._type_ is _lib.GsrScene and fn.argtypes[1]._type_ is _lib.GsrCamera
    assert fn.argtypes[3] is C.c_int64 and all(t is C.c_void_p for k, t in enumerate(fn.argtypes[2:], 2) if k != 3)
    assert re.search(r"int gsr_sh_backward\(const GsrScene \*scene, const GsrCamera \*cam, const float \*grad_rgb , "
                     r"int64_t grad_rgb_stride , float \*grad_sh , float \*grad_means , void \*stream\);", abi.prototypes())


def test_the_abi_version_stays_and_its_comment_names_the_addition():
    abi.assert_version_and_struct_sizes(NEW)


def test_the_header_states_the_contract():
    doc = re.sub(r"\s+\*?\s*", " ", abi.header_comment_before(r"int gsr_sh_backward\("))
    for words in ("exact transpose of gsr_sh_to_rgb", "No cull", "Clamp mask", "the edges pass", "the forward's, bit for bit",
                  "k >= (degree + 1)^2 are neither read nor written", "widened values", "(I - u u^T) / r", "Zero at degree 0",
                  "r == 0", "ADDED into", "either may be NULL (not both)", "no atomics", "Skip rule", "neither read nor written",
                  "12 B of grad_rgb", "are clamped writes nothing", "no workspace", "must be finite", "may alias grad_rgb",
                  "before any HIP call", "n = 0 is GSR_OK", "Single views"):
        assert words.lower() in doc.lower(), words
    # the projection's comment says where the colour term now is
    doc = re.sub(r"\s+\*?\s*", " ", abi.header_comment_before(r"int gsr_project_backward\("))
    assert "gsr_sh_backward adds into the same grad_means" in doc


def test_bad_arguments_are_refused_without_touching_a_gpu():
    """Each refusal with its own gsr_last_error() text.  The arrays are host addresses nobody may dereference: a check that came
    too late would fault, not pass."""
    from gsr_amd import _lib

    fn = _lib.lib.gsr_sh_backward
    n = 4
    cam, sc = _lib.GsrCamera(), _lib.GsrScene()
    host = (C.c_float * (256 * n))()
    base = (C.addressof(host) + 15) // 16 * 16
    rows, g_sh, g_means = base, base + 256, base + 256 + 192 * n + 64  # 16-byte aligned, disjoint
    sc.n, sc.sh_degree, sc.sh_dtype = n, 3, 0
    for k in ("means", "log_scales", "quats", "opacity_logit", "sh"):
        setattr(sc, k, base)

    def call(scene=sc, cam_p=C.byref(cam), grad_rgb=rows, stride=3, sh=g_sh, means=g_means):
        return fn(C.byref(scene) if scene is not None else None, cam_p, grad_rgb, stride, sh, means, None)

    refused = abi.refused("gsr_sh_backward")
    seen = [
        refused(call(scene=None), "null", "scene"),
        refused(call(cam_p=None), "null", "camera"),
        refused(call(grad_rgb=None), "null", "colour gradient"),
        refused(call(sh=None, means=None), "null", "both"),
        refused(call(stride=2), "grad_rgb_stride", "2"),
        refused(call(sh=g_sh + 4), "16-byte", "grad_sh"),
    ]
    for name, rows_bytes in (("grad_sh", 192), ("grad_means", 12)):
        for at in (rows, rows + 12 * n - 4, rows - 16 if name == "grad_sh" else rows - 8):  # first row, last bytes, an end that reaches in
            kw = dict(sh=None, means=None)
            kw["sh" if name == "grad_sh" else "means"] = at
            refused(call(**kw), "aliases grad_rgb", name)
        seen.append(_lib.lib.gsr_last_error().decode())
    # a strided window: an output inside the span of the rows is refused, one past its last value is not an alias
    refused(call(stride=17, sh=None, means=rows + 4 * (17 * (n - 1) + 2)), "aliases grad_rgb", "grad_means")
    for field, value in (("sh_dtype", 2), ("sh_degree", 4), ("sh_degree", -1)):
        bad = _lib.GsrScene.from_buffer_copy(sc)
        setattr(bad, field, value)
        seen.append(refused(call(scene=bad), field))
    assert len(set(seen)) == len(seen)  # each case its own words
    # an empty scene is nothing to do: GSR_OK without a kernel; one output alone is a valid call
    empty = _lib.GsrScene()
    assert call(scene=empty, sh=None) == _lib.GSR_OK and call(scene=empty, means=None) == _lib.GSR_OK


def test_the_kernel_has_a_translation_unit_of_its_own_with_the_preprocess_flags():
    abi.assert_own_translation_unit("sh_backward")
    rule, pre = abi.makefile_recipe("sh_backward.o"), abi.makefile_recipe("preprocess.o")
    assert "-ffp-contract=off" in rule and rule.split() == pre.split()
    deps = abi.makefile_rule("sh_backward.o")[0]
    assert "gauss_math.h" in deps and "gsr_internal.h" in deps and "sh_backward.hip" in deps
    src = open(os.path.join(abi.CSRC, "sh_backward.hip")).read()
    assert "sh_backward_kernel" in src and "__launch_bounds__(SHB_THREADS" in src and "SHB_THREADS = 256" in src
    assert "atomic" not in src.replace("no atomics", "")
    # the clamp is decided on the forward's own value, and fp16 rows are read with the forward's loader
    assert "sh_eval_with<false>(" in src and "load_sh48_f16(" in src
    math = open(os.path.join(abi.CSRC, "gauss_math.h")).read()
    assert "template <bool CLAMP = true, typename Get>" in math and "rgb[c] = !CLAMP ? v : v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);" in math


def test_the_translation_unit_cross_compiles_for_gfx950(tmp_path):
    """With preprocess.o's flags, as csrc/Makefile spells them; the resource remarks show no scratch in either instantiation."""
    mk = open(os.path.join(abi.CSRC, "Makefile")).read()
    hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, flags=re.M).group(1)
    common = re.search(r"^COMMON\s*=\s*(.*)$", mk, flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    out = subprocess.run([hipcc, *common, "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c", "sh_backward.hip", "-o",
                          str(tmp_path / "sh_backward.o")], cwd=abi.CSRC, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert os.path.getsize(tmp_path / "sh_backward.o") > 0
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)
    assert len(scratch) == 2 and all(int(s) == 0 for s in scratch), out.stderr


def test_the_host_side_names():
    from gsr_amd import renderer

    assert renderer.ColourGradient._fields == ("sh", "means")
    assert renderer.SceneGradient._fields == ("means", "log_scales", "quats", "opacity_logit", "sh")
    assert callable(renderer.sh_backward) and callable(renderer.Rasterizer.colour_gradient)
    assert "colour clamp" in renderer.Rasterizer.colour_gradient.__doc__ and "Held fixed" in renderer.Rasterizer.colour_gradient.__doc__
    for fn in (renderer.project_backward, renderer.Rasterizer.geometry_gradient):
        assert "sh_backward" in fn.__doc__ or "colour_gradient" in fn.__doc__


def test_host_refusals_come_before_any_work():
    """colour_gradient's and sh_backward's argument checks on a Rasterizer without a workspace."""
    import pytest
    import torch

    from gsr_amd import renderer

    R = abi.rasterizer()
    with pytest.raises(RuntimeError, match="grad_rgb must live on the GPU"):
        renderer.sh_backward(R.scene, abi.cam(), torch.zeros((R.scene.n, 3)))
    with pytest.raises(RuntimeError, match="grad_image must live on the GPU"):
        R.colour_gradient(abi.cam(), torch.zeros((24, 40, 3)))
