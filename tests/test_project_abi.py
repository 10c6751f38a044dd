"""CPU: gsr_project_backward is an addition to ABI 0.6.0 — declared, exported and bound; no struct or version moved; its argument
checks run before any HIP call; the kernel has a translation unit of its own, built with the preprocess' flags, that cross-compiles
for gfx950; the host names."""
import ctypes as C
import os
import re
import subprocess

import pytest

import abi_checks as abi

NEW = ("gsr_project_backward",)


def test_the_symbol_is_declared_exported_and_bound():
    from gsr_amd import _lib

    abi.assert_declared_exported_and_bound(NEW, 9)
    fn = _lib.lib.gsr_project_backward
    assert fn.argtypes[0]._type_ is _lib.GsrScene and fn.argtypes[1]._type_ is _lib.GsrCamera and fn.argtypes[2]._type_ is _lib.GsrOptions
    assert all(t is C.c_void_p for t in fn.argtypes[3:])
    assert re.search(r"int gsr_project_backward\(const GsrScene \*scene, const GsrCamera \*cam, const GsrOptions \*opts, "
                     r"const float \*grad_splat , float \*grad_means , float \*grad_log_scales , float \*grad_quats , "
                     r"float \*grad_opacity_logit , void \*stream\);", abi.prototypes())


def test_the_abi_version_stays_and_its_comment_names_the_addition():
    abi.assert_version_and_struct_sizes(NEW)


def test_the_header_states_the_contract():
    doc = re.sub(r"\s+\*?\s*", " ", abi.header_comment_before(r"int gsr_project_backward\("))
    for words in ("ADDED into four arrays", "columns 6 and 7 are ignored", "may be NULL (not all)", "no atomics", "sigmas <- cov2d",
                  "cov2d <- (T, cov3d)", "J <- cam_mean", "cam_mean <- mean", "screen_mean <- mean", "cov3d <- M", "R <- quaternion",
                  "opacity <- logit", "sigmoid(x) sigmoid(-x)", "Clamp rule", "derivative in x / z is 0", "Held fixed", "Skip rule",
                  "neither read nor written", "z_cam < GSR_CULL_Z", "det is 0", "not finite", "needs no workspace", "must be finite",
                  "may alias grad_splat", "before any HIP call", "Single views"):
        assert words.lower() in doc.lower(), words


def test_bad_arguments_are_refused_without_touching_a_gpu():
    """Each refusal with its own gsr_last_error() text.  The arrays are host addresses nobody may dereference: a check that came
    too late would fault, not pass."""
    from gsr_amd import _lib

    fn = _lib.lib.gsr_project_backward
    n = 4
    cam, o, sc = _lib.GsrCamera(), _lib.default_options(), _lib.GsrScene()
    cam.width, cam.height = 64, 48
    host = (C.c_float * (64 * n))()
    base = (C.addressof(host) + 15) // 16 * 16
    rows, out = base, [base + 4 * 8 * n + 64 + 256 * k for k in range(4)]  # 16-byte aligned, disjoint
    sc.n, sc.sh_degree, sc.sh_dtype = n, 3, 0
    for k in ("means", "log_scales", "quats", "opacity_logit", "sh"):
        setattr(sc, k, base)

    def call(scene=sc, cam_p=C.byref(cam), opts_p=C.byref(o), grad_splat=rows, outs=out):
        return fn(C.byref(scene) if scene is not None else None, cam_p, opts_p, grad_splat, *outs, None)

    refused = abi.refused("gsr_project_backward")
    seen = [
        refused(call(scene=None), "null", "scene"),
        refused(call(cam_p=None), "null", "camera"),
        refused(call(opts_p=None), "null", "options"),
        refused(call(grad_splat=None), "null", "splat gradient"),
        refused(call(outs=[None] * 4), "null", "all four"),
        refused(call(grad_splat=rows + 4), "16-byte", "grad_splat"),
        refused(call(outs=[out[0], out[1], out[2] + 4, out[3]]), "16-byte", "grad_quats"),
    ]
    for k, name in enumerate(("grad_means", "grad_log_scales", "grad_quats", "grad_opacity_logit")):
        for at in (rows, rows + 32 * n - 16, rows - 16):  # its first row, its last bytes, an output whose end reaches into it
            outs = [None] * 4
            outs[k] = at
            if at < rows and k == 3:
                continue  # [n] floats starting 16 bytes before grad_splat end where it begins: no overlap
            refused(call(outs=outs), "aliases grad_splat", name)
        seen.append(_lib.lib.gsr_last_error().decode())
    bad = _lib.GsrScene.from_buffer_copy(sc)
    bad.sh_dtype = 2
    seen.append(refused(call(scene=bad), "sh_dtype"))
    for field in ("output_dtype", "accum_dtype"):
        b = _lib.default_options()
        setattr(b, field, 1)
        seen.append(refused(call(opts_p=C.byref(b)), field))
    assert len(set(seen)) == len(seen)  # each case its own words
    # an empty scene is nothing to do: GSR_OK without a kernel; one output alone is a valid call
    empty = _lib.GsrScene()
    assert call(scene=empty, outs=[None, None, None, out[3]]) == _lib.GSR_OK


def test_the_kernel_has_a_translation_unit_of_its_own_with_the_preprocess_flags():
    abi.assert_own_translation_unit("project_backward")
    rule, pre = abi.makefile_recipe("project_backward.o"), abi.makefile_recipe("preprocess.o")
    assert "-ffp-contract=off" in rule and rule.split() == pre.split()
    deps = abi.makefile_rule("project_backward.o")[0]
    assert "gauss_math.h" in deps and "gsr_internal.h" in deps and "project_backward.hip" in deps and "splat_chain.h" in deps
    src = open(os.path.join(abi.CSRC, "project_backward.hip")).read()
    assert "project_backward_kernel" in src and "__launch_bounds__(PB_THREADS, 5)" in src and "PB_THREADS = 256" in src
    assert "atomic" not in src.replace("no atomics", "") and "__shared__" not in src
    # the chain is the header's: this file includes it, calls its four functions and restates none of the forward
    chain = open(os.path.join(abi.CSRC, "splat_chain.h")).read()
    assert '#include "splat_chain.h"' in src and '#include "gauss_math.h"' in chain
    for call in ("splat_row(", "splat_forward(", "cov2d_grad(", "mean_grad("):
        assert call in src and re.search(rf"__device__ __forceinline__ [\w ]+\b{re.escape(call)}", chain), call
    for shared in ("cam_mean(", "cov3d_of(", "ewa_cov2d(", "conic_of(", "cov2d_det(", "clip_point(", "pixel_mean("):  # the forward's own functions
        assert shared in chain and shared not in src, shared
    assert "quat_to_rot(" in src  # (named where its transpose is written out; cov3d_of calls it)
    holders = [f for f in sorted(os.listdir(abi.CSRC)) if f.endswith((".hip", ".h", ".inc")) and re.search(r"\bdi2\b", open(os.path.join(abi.CSRC, f)).read())]
    assert holders == ["splat_chain.h"]  # sigmas <- cov2d opens the chain: stated in one file


def test_the_translation_unit_cross_compiles_for_gfx950(tmp_path):
    """With preprocess.o's flags, as csrc/Makefile spells them; the resource remarks show no scratch and 5 waves per SIMD."""
    mk = open(os.path.join(abi.CSRC, "Makefile")).read()
    hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, flags=re.M).group(1)
    common = re.search(r"^COMMON\s*=\s*(.*)$", mk, flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    out = subprocess.run([hipcc, *common, "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c", "project_backward.hip", "-o",
                          str(tmp_path / "project_backward.o")], cwd=abi.CSRC, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert os.path.getsize(tmp_path / "project_backward.o") > 0
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)
    assert scratch and all(int(s) == 0 for s in scratch), out.stderr
    assert re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", out.stderr) == ["5"], out.stderr  # what its launch bounds ask for


def test_the_host_side_names():
    from gsr_amd import renderer

    assert renderer.GeometryGradient._fields == ("means", "log_scales", "quats", "opacity_logit")
    assert callable(renderer.project_backward) and callable(renderer.Rasterizer.geometry_gradient)
    assert "build_bounds()" in renderer.project_backward.__doc__
