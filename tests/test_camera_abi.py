"""CPU: gsr_camera_backward / gsr_camera_backward_bytes are additions to ABI 0.6.0 — declared, exported and bound; no struct or
version moved; the argument checks run before any HIP call; the kernel has a translation unit of its own, built with the
preprocess' flags, that cross-compiles for gfx950 without scratch and holds no atomic; the host names."""
import ctypes as C
import os
import re
import subprocess

import abi_checks as abi

NEW = ("gsr_camera_backward", "gsr_camera_backward_bytes")


def test_the_symbols_are_declared_exported_and_bound():
    from gsr_amd import _lib

    abi.assert_declared_exported_and_bound(NEW[:1], 9)
    assert NEW[1] in abi.declared_names() and _lib.EXPORTS.count(NEW[1]) == 1
    fn, nbytes = _lib.lib.gsr_camera_backward, _lib.lib.gsr_camera_backward_bytes
    assert fn.argtypes[0]._type_ is _lib.GsrScene and fn.argtypes[1]._type_ is _lib.GsrCamera and fn.argtypes[2]._type_ is _lib.GsrOptions
    assert all(t is C.c_void_p for t in fn.argtypes[3:7]) and fn.argtypes[8] is C.c_void_p and C.sizeof(fn.argtypes[7]) == C.sizeof(C.c_size_t)
    assert nbytes.restype is C.c_size_t and nbytes.argtypes == [C.c_int64]
    protos = abi.prototypes()
    assert "size_t gsr_camera_backward_bytes(int64_t n);" in protos
    assert re.search(r"int gsr_camera_backward\(const GsrScene \*scene, const GsrCamera \*cam, const GsrOptions \*opts, "
                     r"const float \*grad_splat , const float \*grad_view_means , double \*grad_camera , void \*workspace, "
                     r"size_t workspace_bytes, void \*stream\);", protos)


def test_the_abi_version_stays_and_its_comment_names_the_addition():
    abi.assert_version_and_struct_sizes(NEW)


def test_the_workspace_is_the_documented_function_of_n():
    """256 * max(1, ceil(B / ceil(B / G))) with B = ceil(n / 256) and G the documented cap on workgroups."""
    from gsr_amd import _lib

    src = open(os.path.join(abi.CSRC, "camera_backward.hip")).read()
    threads, groups = (int(re.search(rf"constexpr int {k} = (\d+);", src).group(1)) for k in ("CB_THREADS", "CB_MAX_GROUPS"))
    assert threads == 256 and 256 <= groups <= 4 * 256  # at most about 4 per CU of a 256-CU part
    assert f"ceil(B / {groups})" in abi.header_comment_before(r"size_t gsr_camera_backward_bytes\(")
    for n in (0, 1, 255, 256, 257, 4096, threads * groups, threads * groups + 1, threads * (2 * groups + 5) + 37, 6_130_000, 2**31 - 1):
        blocks = -(-n // threads)
        want = 256 * max(1, -(-blocks // max(1, -(-blocks // groups))))
        got = _lib.lib.gsr_camera_backward_bytes(n)
        assert got == want and got % 256 == 0 and got <= 256 * groups, n


def test_the_header_states_the_contract():
    doc = re.sub(r"\s+\*?\s*", " ", abi.header_comment_before(r"size_t gsr_camera_backward_bytes\("))
    for words in ("array gsr_project_backward reads", "columns 6 and 7 ignored", "bit for bit", "Skip rule", "z_cam < GSR_CULL_Z",
                  "det is 0", "not finite", "Clamp rule", "derivative in x / z is 0", "Held fixed", "the depth order and lim_x / lim_y",
                  "w2c through the camera-space mean", "w2c through T = J A^T", "full_proj", "no division by fx", "cam_center",
                  "grad_sh = NULL", "dcc[k] -= grad_view_means[i][k]", "No SH row is read", "may be NULL (not both)", "Result layout",
                  "32 doubles", "WRITTEN", "[3 k + j]", "[12 + 3 k + jj]", "[24], [25]", "[26 .. 28]", "[29]", "Exact", "[30], [31]",
                  "hand-filled GsrCamera", "every sum across gaussians is done in double", "No atomics", "same bits",
                  "doubles the result exactly", "nothing has to be cleared", "before any HIP call", "n = 0 writes 32 zeros", "Single views"):
        assert words.lower() in doc.lower(), words


def test_bad_arguments_are_refused_without_touching_a_gpu():
    """Each refusal with its own gsr_last_error() text.  The arrays are host addresses nobody may dereference: a check that came
    too late would fault, not pass."""
    from gsr_amd import _lib

    fn = _lib.lib.gsr_camera_backward
    n = 4
    cam, o, sc = _lib.GsrCamera(), _lib.default_options(), _lib.GsrScene()
    cam.width, cam.height = 64, 48
    host = (C.c_float * 2048)()
    base = (C.addressof(host) + 255) // 256 * 256
    rows, view, out, ws = base + 1024, base + 2048, base + 3072, base + 4096  # 128, 48, 256 and 256 bytes, well apart
    need = _lib.lib.gsr_camera_backward_bytes(n)
    assert need == 256
    sc.n, sc.sh_degree, sc.sh_dtype = n, 3, 0
    for k in ("means", "log_scales", "quats", "opacity_logit", "sh"):
        setattr(sc, k, base)

    def call(scene=sc, cam_p=C.byref(cam), opts_p=C.byref(o), grad_splat=rows, grad_view=view, grad_camera=out, workspace=ws, nbytes=need):
        return fn(C.byref(scene) if scene is not None else None, cam_p, opts_p, grad_splat, grad_view, grad_camera, workspace, nbytes, None)

    refused = abi.refused("gsr_camera_backward")
    seen = [
        refused(call(scene=None), "null", "scene"),
        refused(call(cam_p=None), "null", "camera"),
        refused(call(opts_p=None), "null", "options"),
        refused(call(grad_camera=None), "null", "camera gradient"),
        refused(call(workspace=None), "null", "workspace"),
        refused(call(grad_splat=None, grad_view=None), "null", "both"),
        refused(call(nbytes=need - 1), "too small", "255", "256"),
        refused(call(grad_splat=rows + 4), "16-byte", "grad_splat"),
        refused(call(grad_camera=out + 4), "8-byte", "grad_camera"),
        refused(call(workspace=ws + 4), "8-byte", "workspace"),
        refused(call(grad_camera=ws + 8), "grad_camera overlaps the workspace"),
    ]
    for name, at in (("grad_camera", "grad_camera"), ("the workspace", "workspace")):
        for inp, where, size in (("grad_splat", rows, 32 * n), ("grad_view_means", view, 12 * n)):
            for place in (where, where + size - 8, where - 256 + 8):  # its first bytes, its last, an output whose end reaches into it
                refused(call(**{at: place}), f"{name} overlaps {inp}")
            seen.append(_lib.lib.gsr_last_error().decode())
    bad = _lib.GsrScene.from_buffer_copy(sc)
    bad.sh_dtype = 2
    seen.append(refused(call(scene=bad), "sh_dtype"))
    for field in ("output_dtype", "accum_dtype"):
        b = _lib.default_options()
        setattr(b, field, 1)
        seen.append(refused(call(opts_p=C.byref(b)), field))
    assert len(set(seen)) == len(seen)  # each case its own words
    # an output that ends where an input begins does not overlap it: the next refusal in line answers
    refused(call(grad_camera=rows - 256, nbytes=need - 1), "too small")


def test_the_kernel_has_a_translation_unit_of_its_own_with_the_preprocess_flags():
    abi.assert_own_translation_unit("camera_backward")
    rule, pre = abi.makefile_recipe("camera_backward.o"), abi.makefile_recipe("preprocess.o")
    assert "-ffp-contract=off" in rule and rule.split() == pre.split()
    deps = abi.makefile_rule("camera_backward.o")[0]
    assert "gauss_math.h" in deps and "gsr_internal.h" in deps and "camera_backward.hip" in deps and "splat_chain.h" in deps
    src = open(os.path.join(abi.CSRC, "camera_backward.hip")).read()
    assert "camera_backward_kernel" in src and "camera_reduce_kernel" in src and "__launch_bounds__(CB_THREADS)" in src
    assert "atomic" not in src.lower().replace("no atomics", "")
    # the chain is the header's, the one project_backward.hip walks: included, its four functions called, nothing of it restated
    chain, other = (open(os.path.join(abi.CSRC, f)).read() for f in ("splat_chain.h", "project_backward.hip"))
    assert '#include "splat_chain.h"' in src and '#include "gauss_math.h"' in chain
    for call in ("splat_row(", "splat_forward(", "cov2d_grad(", "mean_grad("):
        assert call in src and call in other and re.search(rf"__device__ __forceinline__ [\w ]+\b{re.escape(call)}", chain), call
    for shared in ("cam_mean(", "cov3d_of(", "ewa_cov2d(", "cov2d_det(", "conic_of(", "clip_point(", "pixel_mean("):  # the forward's own functions
        assert shared in chain and shared not in src, shared
    for upstream in ("di2", "V[10]", "in_x", "gnx"):  # sigmas <- cov2d, d / d J = gT A, the clamp decision, d / d clip point: stated once
        assert upstream in chain and upstream not in src and upstream not in other, upstream
    assert "sh_eval" not in src and "sc.sh" not in src  # no SH row is read
    assert "double acc[29]" in src and "float acc" not in src
    assert "camera_backward.hip" in open(os.path.join(abi.REPO, "tools", "kernel_resources.sh")).read()


def test_the_translation_unit_cross_compiles_for_gfx950(tmp_path):
    """With preprocess.o's flags, as csrc/Makefile spells them; the resource remarks show no scratch in either kernel."""
    mk = open(os.path.join(abi.CSRC, "Makefile")).read()
    hipcc = re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, flags=re.M).group(1)
    common = re.search(r"^COMMON\s*=\s*(.*)$", mk, flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    out = subprocess.run([hipcc, *common, "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c", "camera_backward.hip", "-o",
                          str(tmp_path / "camera_backward.o")], cwd=abi.CSRC, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert os.path.getsize(tmp_path / "camera_backward.o") > 0
    scratch = re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)
    assert len(scratch) == 2 and all(int(s) == 0 for s in scratch), out.stderr
    # 3 waves per SIMD is what CB_MAX_GROUPS counts on; the reduction's few registers leave it all eight
    occ = dict(re.findall(r"Function Name: _ZN3gsr\d+(\w+?_kernel)E.*?Occupancy \[waves/SIMD\]: (\d+)", out.stderr, flags=re.S))
    assert occ == {"camera_backward_kernel": "3", "camera_reduce_kernel": "8"}, out.stderr


def test_the_host_side_names():
    import torch

    from gsr_amd import renderer

    assert renderer.CameraGradient._fields == ("w2c", "full_proj", "focal", "cam_center", "contributing")
    assert callable(renderer.camera_backward) and callable(renderer.pose_gradient) and callable(renderer.Rasterizer.camera_gradient)
    # the [32] doubles laid out as the struct's fields; the columns the forward never reads are zeros; one buffer underneath
    buf = torch.arange(1, 33, dtype=torch.float64)
    buf[30:] = 0
    cg = renderer._camera_gradient_of(buf)
    assert cg.w2c.tolist() == [[1, 2, 3, 0], [4, 5, 6, 0], [7, 8, 9, 0], [10, 11, 12, 0]]
    assert cg.full_proj.tolist() == [[13, 14, 0, 15], [16, 17, 0, 18], [19, 20, 0, 21], [22, 23, 0, 24]]
    assert cg.focal.tolist() == [25, 26] and cg.cam_center.tolist() == [27, 28, 29] and float(cg.contributing) == 30 and cg.contributing.dim() == 0
    assert len({t.untyped_storage().data_ptr() for t in cg}) == 1 and all(t.dtype == torch.float64 for t in cg)
    # a pure translation of the camera along its own axes: d L / d v is the translation row of d L / d w2c (identity pose)
    cam = abi.cam()
    for k in range(4):
        cam.w2c[5 * k] = cam.full_proj[5 * k] = 1.0
    cam.focal_x = cam.focal_y = 2.0
    twist, logf = renderer.pose_gradient(cam, cg)
    assert twist.dtype == logf.dtype == torch.float64 and tuple(twist.shape) == (6,) and tuple(logf.shape) == (2,)
    assert twist[3:].tolist() == [10 + 22 - 27, 11 + 23 - 28, 12 - 29]  # w2c row 3 + full_proj row 3 (its column 2 is never read) - cam_center
    assert logf.tolist() == [2 * 25 + 13, 2 * 26 + 17]
