"""CPU: gsr_blend_gaussian_stats / gsr_render_gaussian_stats are additions to ABI 0.6.0 — declared, exported and bound; no struct or
version moved; their argument checks run before any HIP call; Rasterizer.view_stats refuses bad arguments before it allocates; and
the host-side arithmetic of renderer.accumulate_view_stats."""
import ctypes as C
import re
import types

import pytest
import torch

import abi_checks as abi

NEW = ("gsr_blend_gaussian_stats", "gsr_render_gaussian_stats")


def test_the_two_symbols_are_declared_exported_and_bound():
    from gsr_amd import _lib

    abi.assert_declared_exported_and_bound(NEW, 11)
    for name in NEW:
        fn = getattr(_lib.lib, name)
        assert fn.argtypes[3] is C.c_int64 and fn.argtypes[5] is C.c_size_t, name   # max_pairs, workspace_bytes
        assert all(t is C.c_void_p for t in fn.argtypes[6:]), name                   # mask, the three outputs, the stream
    assert _lib.lib.gsr_blend_gaussian_stats.argtypes[0] is C.c_int64
    flat = abi.prototypes()
    tail = (r"const GsrCamera \*cam, const GsrOptions \*opts, int64_t max_pairs, void \*workspace, size_t workspace_bytes, "
            r"const uint8_t \*pixel_mask , float \*weight_sum, float \*weight_max, uint32_t \*pixels, void \*stream\);")
    assert re.search(r"int gsr_blend_gaussian_stats\(int64_t n, " + tail, flat)
    assert re.search(r"int gsr_render_gaussian_stats\(const GsrScene \*scene, " + tail, flat)


def test_the_abi_version_stays_and_its_comment_names_the_additions():
    abi.assert_version_and_struct_sizes(NEW)


def test_the_header_states_the_contract():
    doc = re.sub(r"\s+\*?\s*", " ", abi.header_comment_before(r"int gsr_blend_gaussian_stats\("))
    for words in ("exact and reproducible to the bit", "order the adds arrive in", "NON-NEGATIVE FINITE floats on entry", "ACCUMULATE",
                  "not all three", "non-zero = the pixel counts", "colour_evals = 0", "Single views"):
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

    def call(cam_p, opts_p, outs=(p, p, p), mask=p):
        head = (C.byref(sc),) if entry == "gsr_render_gaussian_stats" else (0,)
        return fn(*head, cam_p, opts_p, 100, None, 0, mask, *outs, None)

    refused = abi.refused(entry)

    seen = [
        refused(call(None, C.byref(o)), "null", "camera"),
        refused(call(C.byref(cam), None), "null", "options"),
        refused(call(C.byref(cam), C.byref(o), outs=(None, None, None)), "null", "outputs", "three"),
    ]
    b = _lib.default_options()
    b.output_dtype = 1
    seen.append(refused(call(C.byref(cam), C.byref(b)), "output_dtype"))
    b = _lib.default_options()
    b.accum_dtype = 1
    seen.append(refused(call(C.byref(cam), C.byref(b)), "accum_dtype"))
    assert len(set(seen)) == len(seen)  # each case its own words
    # and with everything above in order — any one output alone, with or without a mask — the next check is the usual one: a null
    # workspace (gsr_render_gaussian_stats: the empty scene's arrays) — still no GPU
    for kw in (dict(outs=(p, None, None)), dict(outs=(None, p, None)), dict(outs=(None, None, p)), dict(mask=None), dict()):
        assert "null" in refused(call(C.byref(cam), C.byref(o), **kw), "null"), kw
        for w in ("outputs", "output_dtype", "accum_dtype"):
            assert w not in _lib.lib.gsr_last_error().decode(), (kw, w)


def test_the_new_kernel_has_a_translation_unit_of_its_own():
    abi.assert_own_translation_unit("blend_gstats")
    rule, grad = abi.makefile_rule("blend_gstats.o"), abi.makefile_rule("blend_channels_backward.o")
    assert "-fno-slp-vectorize" in rule[1]  # the weights' bits depend on it: the gradient kernel's flags
    assert rule[1].split() == grad[1].split()
    assert [d for d in rule[0].split() if d != "blend_gstats.hip"] == [d for d in grad[0].split() if d != "blend_channels_backward.hip"]


def test_view_stats_refuses_bad_arguments_before_it_allocates():
    from gsr_amd import renderer

    R, cam = abi.rasterizer(views=1), abi.cam()
    VS = renderer.ViewStats
    good_mask = torch.ones((24, 40), dtype=torch.bool)
    good_out = VS(torch.zeros(5), torch.zeros(5), torch.zeros(5, dtype=torch.int32))
    bad = [
        dict(mask=torch.ones((40, 24), dtype=torch.bool)),                 # the transposed shape
        dict(mask=torch.ones((24, 40), dtype=torch.float32)),              # not bool / uint8
        dict(mask=torch.ones((24, 40), dtype=torch.bool, device="meta")),  # another device
        dict(mask=[[1] * 40] * 24),                                        # not a tensor
        dict(mask=good_mask, opts=renderer.make_options(output_layout=1)), # the screen layout wants [W, H]
        dict(want=()), dict(want=("sum", "mean")), dict(want="sum"), dict(want=(1,)),
        dict(out=(good_out.weight_sum, good_out.weight_max)),
        dict(out=VS(torch.zeros(4), good_out.weight_max, good_out.pixels)),
        dict(out=VS(good_out.weight_sum, torch.zeros(5, dtype=torch.float64), good_out.pixels)),
        dict(out=VS(good_out.weight_sum, good_out.weight_max, torch.zeros(5, dtype=torch.int64))),
        dict(out=VS(good_out.weight_sum, good_out.weight_max, torch.zeros(10, dtype=torch.int32)[::2])),
        dict(out=VS(None, good_out.weight_max, good_out.pixels)),
        dict(out=VS(torch.zeros(5, device="meta"), good_out.weight_max, good_out.pixels)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            R.view_stats(cam, **kw)
    # good arguments get as far as the workspace: the mask in either dtype, the screen layout's shape, a partial `out` for a partial `want`
    for kw in (dict(mask=good_mask), dict(mask=good_mask.to(torch.uint8)), dict(out=good_out),
               dict(mask=good_mask.t().contiguous(), opts=renderer.make_options(output_layout=1)),
               dict(out=VS(None, good_out.weight_max, None), want=("max",)), dict(want=["pixels"])):
        with pytest.raises(abi.NoWorkspace):
            R.view_stats(cam, **kw)
    # nothing to draw: zeros, or `out` as it is, without a workspace
    E = abi.rasterizer(0, views=1)
    st = E.view_stats(cam, want=("max", "pixels"))
    assert st.weight_sum is None and st.weight_max.shape == (0,) and st.pixels.dtype == torch.int32
    empty = renderer.make_options(tile_row_begin=2, tile_row_step=3, output_layout=2)  # two tile rows, the third of three shards
    st = R.view_stats(cam, empty)
    assert all(t.shape == (5,) and not t.any() for t in st)
    out = VS(torch.full((5,), 2.0), torch.full((5,), 1.0), torch.full((5,), 4, dtype=torch.int32))
    got = R.view_stats(cam, empty, out=out)
    assert all(a is b for a, b in zip(got, out)) and bool((out.pixels == 4).all()) and bool((out.weight_sum == 2.0).all())


def test_accumulate_view_stats_counts_the_views_that_reach_a_pixel():
    from gsr_amd import renderer

    n = 6
    order_t = torch.tensor([3, 0, 5, 1, 4, 2])  # scene index -> file index
    per_view = {  # in the scene's order: (sum, max, pixels)
        "a": (torch.tensor([1.0, 0, 2, 0, 0, 4]), torch.tensor([0.5, 0, 0.25, 0, 0, 0.75]), torch.tensor([3, 0, 9, 0, 0, 7])),
        "b": (torch.tensor([0.0, 0, 1, 5, 0, 1]), torch.tensor([0.0, 0, 0.5, 0.125, 0, 0.5]), torch.tensor([0, 0, 2, 40, 0, 1])),
        "c": (torch.tensor([2.0, 0, 0, 0, 0, 8]), torch.tensor([0.25, 0, 0, 0, 0, 0.875]), torch.tensor([1, 0, 0, 0, 0, 11])),
    }
    calls = []

    class Stub:
        scene = types.SimpleNamespace(n=n, device=torch.device("cpu"), order_t=order_t)

        def view_stats(self, cam, opts=None, mask=None, out=None, scene_order=False, want=renderer.VIEW_STATS):
            s, m, p = per_view[cam]
            assert out is not None and tuple(want) == renderer.VIEW_STATS
            out.weight_sum.add_(s)
            torch.maximum(out.weight_max, m, out=out.weight_max)
            out.pixels.add_(p.to(torch.int32))
            calls.append((cam, opts, mask))
            return out

    total, views = renderer.accumulate_view_stats(Stub(), ["a", "b", "c"], opts="O", masks=[None, "M", None])
    assert calls == [("a", "O", None), ("b", "O", "M"), ("c", "O", None)]
    scene_views = torch.tensor([2, 0, 2, 1, 0, 3], dtype=torch.int32)
    assert views.dtype == torch.int32 and torch.equal(views[order_t], scene_views)      # file order: entry order_t[j] is scene row j
    assert torch.equal(total.pixels[order_t], torch.tensor([4, 0, 11, 40, 0, 19], dtype=torch.int32))
    assert torch.equal(total.weight_max[order_t], torch.tensor([0.5, 0, 0.5, 0.125, 0, 0.875]))
    assert torch.equal(total.weight_sum[order_t], torch.tensor([3.0, 0, 3, 5, 0, 13]))
    assert not torch.equal(views, scene_views)
    total, views = renderer.accumulate_view_stats(Stub(), [])
    assert not views.any() and not total.pixels.any() and views.shape == (n,)
    with pytest.raises(ValueError):
        renderer.accumulate_view_stats(Stub(), ["a", "b"], masks=[None])
