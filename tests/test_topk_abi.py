"""CPU: gsr_blend_topk / gsr_render_topk are additions to ABI 0.6.0 — declared, exported and bound; no struct or version moved; their
argument checks run before any HIP call; the kernel has a translation unit with the blend's flags; and the two host-side pieces
of the Python surface (renderer.topk_composite, renderer.file_order_ids on [H,W,k] lists) do what they say on CPU tensors."""
import ctypes as C
import re

import pytest
import torch

import abi_checks as abi

NEW = ("gsr_blend_topk", "gsr_render_topk")


def test_the_two_symbols_are_declared_exported_and_bound():
    from gsr_amd import _lib

    abi.assert_declared_exported_and_bound(NEW, 12)
    for name in NEW:
        fn = getattr(_lib.lib, name)
        assert fn.argtypes[6] is C.c_int32 and fn.argtypes[7] is C.c_int32, name  # k, select
    text, flat = abi.header_code(), abi.prototypes()
    tail = (r"const GsrCamera \*cam, const GsrOptions \*opts, int64_t max_pairs, void \*workspace, size_t workspace_bytes, "
            r"int32_t k, int32_t select, int32_t \*out_ids, float \*out_weights, float \*out_final_T, void \*stream\);")
    assert re.search(r"int gsr_blend_topk\(int64_t n, " + tail, flat)
    assert re.search(r"int gsr_render_topk\(const GsrScene \*scene, " + tail, flat)
    assert re.search(r"#define GSR_MAX_TOPK 16\b", text) and _lib.GSR_MAX_TOPK == 16
    assert re.search(r"#define GSR_TOPK_HEAVIEST 0\b", text) and _lib.GSR_TOPK_HEAVIEST == 0
    assert re.search(r"#define GSR_TOPK_NEAREST\s+1\b", text) and _lib.GSR_TOPK_NEAREST == 1


def test_the_abi_version_stays_and_its_comment_names_the_additions():
    abi.assert_version_and_struct_sizes(NEW)


def test_the_header_states_the_order_of_the_slots_and_what_an_id_is():
    doc = abi.header_comment_before(r"#define GSR_MAX_TOPK")
    flat = re.sub(r"[\s*]+", " ", doc)
    assert "indices into the caller's scene arrays" in flat
    assert "equal weights the earlier gaussian in draw order comes first" in flat
    assert "equal depth the draw order is array-index order" in flat
    assert "Unused slots hold id -1 and weight 0" in flat
    assert "the stride is exactly k" in flat


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

    def call(cam_p, opts_p, k=4, select=0, outs=(p, p, p)):
        head = (C.byref(sc),) if entry == "gsr_render_topk" else (0,)
        return fn(*head, cam_p, opts_p, 100, None, 0, k, select, *outs, None)

    refused = abi.refused(entry)

    seen = [
        refused(call(None, C.byref(o)), "null", "camera"),
        refused(call(C.byref(cam), None), "null", "options"),
        refused(call(C.byref(cam), C.byref(o), outs=(None, None, p)), "null", "outputs"),
    ]
    for bad in (0, -1, 17):
        assert str(bad) in refused(call(C.byref(cam), C.byref(o), k=bad), "bad k")
    seen.append(_lib.lib.gsr_last_error().decode())
    for bad in (-1, 2):
        assert str(bad) in refused(call(C.byref(cam), C.byref(o), select=bad), "select")
    seen.append(_lib.lib.gsr_last_error().decode())
    b = _lib.default_options()
    b.output_dtype = 1
    seen.append(refused(call(C.byref(cam), C.byref(b)), "output_dtype"))
    b = _lib.default_options()
    b.accum_dtype = 1
    seen.append(refused(call(C.byref(cam), C.byref(b)), "accum_dtype"))
    assert len(set(seen)) == len(seen)  # each case its own words
    # and with everything above in order — the end values of k, either select, ids alone, weights alone, no final T — the next check
    # is the usual one: a null workspace (gsr_render_topk: the empty scene's arrays) — still no GPU
    for kw in (dict(k=1), dict(k=16), dict(select=0), dict(select=1), dict(outs=(p, None, None)), dict(outs=(None, p, None)),
               dict(outs=(p, p, None)), dict(k=16, select=1, outs=(None, p, p))):
        assert "null" in refused(call(C.byref(cam), C.byref(o), **kw), "null"), kw
        for w in ("outputs", "bad k", "select", "output_dtype", "accum_dtype"):
            assert w not in _lib.lib.gsr_last_error().decode(), (kw, w)


def test_the_new_kernel_has_a_translation_unit_of_its_own():
    abi.assert_own_translation_unit("blend_topk")
    rule, pick = abi.makefile_recipe("blend_topk.o"), abi.makefile_recipe("blend_pick.o")
    assert "-fno-slp-vectorize" in rule  # the weights' bits depend on it: the flags of blend_pick.o
    assert rule == pick


def test_render_topk_refuses_a_bad_k_or_select_before_anything_else():
    """(A scene on the CPU is enough: the checks come before the workspace is made.)"""
    from gsr_amd import renderer

    class _NoScene:
        n, device, order_t = 0, torch.device("cpu"), None

    R = renderer.Rasterizer(_NoScene())
    cam = renderer.GsrCamera()
    for k in (0, -1, 17, 2.5, True):
        with pytest.raises(ValueError, match="k must be"):
            R.render_topk(cam, k)
    for select in ("median", "", None, 0):
        with pytest.raises(ValueError, match="select must be"):
            R.render_topk(cam, 4, select=select)
    assert renderer.TopK._fields == ("ids", "weights", "final_T")


def test_topk_composite_is_the_sparse_sum_and_its_gradient_the_dense_transpose():
    from gsr_amd.renderer import TopK, topk_composite

    gen = torch.Generator().manual_seed(5)
    H, W, k, n, Cn = 7, 5, 4, 23, 6
    ids = torch.randint(0, n - 3, (H, W, k), generator=gen, dtype=torch.int32)   # rows n-3 .. n-1 appear in no slot
    ids[torch.rand((H, W, k), generator=gen) < 0.3] = -1
    ids[0, 0] = -1                                                               # a pixel with nothing in it
    ids[ids == 0] = 1                                                            # row 0 appears in no slot either: -1 must not reach it
    weights = torch.rand((H, W, k), generator=gen, dtype=torch.float32)
    weights = torch.where(ids >= 0, weights, torch.zeros_like(weights))
    weights[1, 1] = torch.where(ids[1, 1] >= 0, weights[1, 1], torch.full((k,), 0.75))  # a -1 slot contributes 0 whatever its weight says
    assert bool((ids == -1).any()) and bool((ids >= 0).any())
    features = torch.randn((n, Cn), generator=gen, dtype=torch.float32, requires_grad=True)
    out = topk_composite(TopK(ids, weights, None), features)
    assert out.shape == (H, W, Cn) and out.dtype == torch.float32
    # dense float64: A[p, i] = the sum of the weights of the slots of p that hold i
    A = torch.zeros((H * W, n), dtype=torch.float64)
    flat_ids, flat_w = ids.reshape(H * W, k).long(), weights.reshape(H * W, k).double()
    for j in range(k):
        ok = flat_ids[:, j] >= 0
        A[ok.nonzero()[:, 0], flat_ids[ok, j]] += flat_w[ok, j]
    ref = (A @ features.detach().double()).reshape(H, W, Cn)
    assert float((out.detach().double() - ref).abs().max()) <= 1e-6 * max(1.0, float(ref.abs().max()))
    assert not out[0, 0].any()
    grad_map = torch.randn((H, W, Cn), generator=gen, dtype=torch.float32)
    (g,) = torch.autograd.grad(out, features, grad_map)
    g_ref = A.t() @ grad_map.reshape(H * W, Cn).double()
    assert float((g.double() - g_ref).abs().max()) <= 1e-6 * float(g_ref.abs().max())
    unused = torch.ones(n, dtype=torch.bool)
    unused[flat_ids[flat_ids >= 0]] = False
    assert unused[0] and bool(unused[n - 3:].all()) and int(unused.sum()) < n
    assert bool((g[unused] == 0).all())  # exactly


def test_file_order_ids_maps_lists_like_maps():
    from gsr_amd.renderer import file_order_ids

    gen = torch.Generator().manual_seed(13)
    n = 500
    order = torch.randperm(n, generator=gen)  # scene index -> file index
    ids = torch.randint(-1, n, (9, 11, 5), generator=gen, dtype=torch.int32)
    ids[2, 3] = -1
    out = file_order_ids(ids, order)
    assert out.dtype == torch.int32 and out.shape == ids.shape
    assert torch.equal(out == -1, ids == -1)                            # -1 stays -1, nothing else becomes it
    hit = ids >= 0
    assert torch.equal(out[hit].long(), order[ids[hit].long()])
    assert file_order_ids(ids, None) is ids
