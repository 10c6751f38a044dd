"""CPU: gsr_blend_pick / gsr_render_pick are additions to ABI 0.6.0 — declared, exported and bound; no struct or version moved; their
argument checks run before any HIP call; and the host-side id mapping (renderer.file_order_ids) is the scene's permutation."""
import ctypes as C
import re

import pytest
import torch

import abi_checks as abi

NEW = ("gsr_blend_pick", "gsr_render_pick")


def test_the_two_symbols_are_declared_exported_and_bound():
    from gsr_amd import _lib

    abi.assert_declared_exported_and_bound(NEW, 12)
    for name in NEW:
        fn = getattr(_lib.lib, name)
        assert fn.argtypes[6] is C.c_float, name     # median_T
    flat = abi.prototypes()
    tail = (r"const GsrCamera \*cam, const GsrOptions \*opts, int64_t max_pairs, void \*workspace, size_t workspace_bytes, "
            r"float median_T, int32_t \*out_best_id, float \*out_best_w, int32_t \*out_median_id, int32_t \*out_count, void \*stream\);")
    assert re.search(r"int gsr_blend_pick\(int64_t n, " + tail, flat)
    assert re.search(r"int gsr_render_pick\(const GsrScene \*scene, " + tail, flat)


def test_the_abi_version_stays_and_its_comment_names_the_additions():
    abi.assert_version_and_struct_sizes(NEW)


def test_the_header_states_what_an_id_is():
    doc = abi.header_comment_before(r"int gsr_blend_pick\(")
    flat = re.sub(r"[\s*]+", " ", doc)
    assert "indices into the caller's scene arrays" in flat
    assert "equal weights the earlier gaussian in draw order wins" in flat
    assert "equal depth the draw order is array-index order" in flat


@pytest.mark.parametrize("entry", NEW)
def test_bad_arguments_are_refused_without_touching_a_gpu(entry):
    """Each refusal comes with its own gsr_last_error() text and before the workspace (NULL here) is even looked at.  The output
    arguments are host addresses nobody may dereference: a check that came too late would fault, not pass."""
    from gsr_amd import _lib

    fn = getattr(_lib.lib, entry)
    cam, o, sc = _lib.GsrCamera(), _lib.default_options(), _lib.GsrScene()
    cam.width, cam.height = 64, 48
    host = (C.c_float * 4)()
    p = C.addressof(host)

    def call(cam_p, opts_p, median_T=0.5, outs=(p, p, p, p)):
        head = (C.byref(sc),) if entry == "gsr_render_pick" else (0,)
        return fn(*head, cam_p, opts_p, 100, None, 0, median_T, *outs, None)

    refused = abi.refused(entry)

    seen = [
        refused(call(None, C.byref(o)), "null", "camera"),
        refused(call(C.byref(cam), None), "null", "options"),
        refused(call(C.byref(cam), C.byref(o), outs=(None, None, None, None)), "null", "outputs"),
    ]
    for bad in (float("nan"), 0.0, -0.5, 1.0000001, 2.0, float("inf")):
        assert "median_T" in refused(call(C.byref(cam), C.byref(o), median_T=bad), "median_T")
    seen.append(_lib.lib.gsr_last_error().decode())
    b = _lib.default_options()
    b.output_dtype = 1
    seen.append(refused(call(C.byref(cam), C.byref(b)), "output_dtype"))
    b = _lib.default_options()
    b.accum_dtype = 1
    seen.append(refused(call(C.byref(cam), C.byref(b)), "accum_dtype"))
    assert len(set(seen)) == len(seen)  # each case its own words
    # and with everything above in order — the end values of median_T, any one output alone — the next check is the usual one: a
    # null workspace (gsr_render_pick: the empty scene's arrays) — still no GPU
    for kw in (dict(median_T=1.0), dict(median_T=1e-30), dict(outs=(p, None, None, None)), dict(outs=(None, p, None, None)),
               dict(outs=(None, None, p, None)), dict(outs=(None, None, None, p))):
        assert "null" in refused(call(C.byref(cam), C.byref(o), **kw), "null"), kw
        for w in ("outputs", "median_T", "output_dtype", "accum_dtype"):
            assert w not in _lib.lib.gsr_last_error().decode(), (kw, w)


def test_the_new_kernel_has_a_translation_unit_of_its_own():
    abi.assert_own_translation_unit("blend_pick")
    assert "-fno-slp-vectorize" in abi.makefile_recipe("blend_pick.o")  # the weights' bits depend on it: the flags of blend_features.o


def test_file_order_ids_is_the_scenes_permutation():
    from gsr_amd.renderer import file_order_gradient, file_order_ids

    gen = torch.Generator().manual_seed(11)
    n = 1000
    order = torch.randperm(n, generator=gen)  # scene index -> file index
    ids = torch.randint(-1, n, (37, 53), generator=gen, dtype=torch.int32)
    ids[0, :5] = -1
    out = file_order_ids(ids, order)
    assert out.dtype == torch.int32 and out.shape == ids.shape
    assert torch.equal(out == -1, ids == -1)                            # -1 stays -1, nothing else becomes it
    hit = ids >= 0
    assert torch.equal(out[hit].long(), order[ids[hit].long()])
    # round trip through the inverse permutation, and agreement with the gather the features go through: the value a file-order
    # array holds at the mapped id is the value the scene-order array holds at the kernel's id
    inverse = torch.empty_like(order).index_copy_(0, order, torch.arange(n))
    assert torch.equal(file_order_ids(out, inverse), ids)
    values = torch.randn(n, generator=gen)
    scene_values = values.index_select(0, order)
    assert torch.equal(values[out[hit].long()], scene_values[ids[hit].long()])
    assert torch.equal(file_order_gradient(scene_values, order), values)
    assert file_order_ids(ids, None) is ids                             # a scene in file order: the identity
    assert torch.equal(file_order_ids(torch.full((3, 2), -1, dtype=torch.int32), order), torch.full((3, 2), -1, dtype=torch.int32))
