"""CPU: the five entry points that take feature maps, their gradient and the view statistics through several views per launch
sequence — gsr_lists_views, gsr_blend_channels_views, gsr_blend_channels_backward_views, gsr_blend_gaussian_stats_views,
gsr_render_channels_batch — are additions to ABI 0.6.0: declared, exported and bound with their exact prototypes; no struct or
version moved; every refusal comes before any HIP call; the Python methods refuse bad arguments before they allocate; and
accumulate_view_stats hands a Rasterizer with several slices all cameras in one call."""
import ctypes as C
import re
import types

import pytest
import torch

import abi_checks as abi

NEW = ("gsr_lists_views", "gsr_blend_channels_views", "gsr_blend_channels_backward_views", "gsr_blend_gaussian_stats_views",
       "gsr_render_channels_batch")
N_ARGS = dict(zip(NEW, (8, 15, 13, 15, 15)))
VIEWS = r"const GsrCamera \*cams , int32_t n_views, const GsrOptions \*opts, int64_t max_pairs, void \*workspace, size_t workspace_bytes, "
MAPS = (r"const float \*features, int32_t channels, int64_t feature_stride, float \*out_maps, int64_t map_stride, float \*out_final_T , "
        r"int64_t T_stride, void \*stream\);")
PROTOTYPES = {
    "gsr_lists_views": r"int gsr_lists_views\(const GsrScene \*scene, " + VIEWS + r"void \*stream\);",
    "gsr_blend_channels_views": r"int gsr_blend_channels_views\(int64_t n, " + VIEWS + MAPS,
    "gsr_blend_channels_backward_views": r"int gsr_blend_channels_backward_views\(int64_t n, " + VIEWS +
        r"const float \*grad_maps, int64_t map_stride, int32_t channels, float \*grad_features, int64_t grad_stride, void \*stream\);",
    "gsr_blend_gaussian_stats_views": r"int gsr_blend_gaussian_stats_views\(int64_t n, " + VIEWS +
        r"const uint8_t \*pixel_masks , int64_t mask_stride, float \*weight_sum, float \*weight_max, uint32_t \*pixels, "
        r"uint32_t \*view_hits, uint32_t \*view_bits, void \*stream\);",
    "gsr_render_channels_batch": r"int gsr_render_channels_batch\(const GsrScene \*scene, " + VIEWS.replace("n_views", "n_cams") + MAPS,
}


def test_the_five_symbols_are_declared_exported_and_bound():
    from gsr_amd import _lib

    flat = abi.prototypes()
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    tails = {
        "gsr_lists_views": [vp],
        "gsr_blend_channels_views": [vp, i32, i64, vp, i64, vp, i64, vp],
        "gsr_blend_channels_backward_views": [vp, i64, i32, vp, i64, vp],
        "gsr_blend_gaussian_stats_views": [vp, i64, vp, vp, vp, vp, vp, vp],
        "gsr_render_channels_batch": [vp, i32, i64, vp, i64, vp, i64, vp],
    }
    for name in NEW:
        abi.assert_declared_exported_and_bound((name,), N_ARGS[name])
        assert re.search(PROTOTYPES[name], flat), name
        fn = getattr(_lib.lib, name)
        head = C.POINTER(_lib.GsrScene) if name in ("gsr_lists_views", "gsr_render_channels_batch") else i64
        assert fn.argtypes[0] is head or fn.argtypes[0] == head, name
        assert fn.argtypes[1] == C.POINTER(_lib.GsrCamera) and fn.argtypes[2] is i32 and fn.argtypes[3] == C.POINTER(_lib.GsrOptions), name
        assert fn.argtypes[4] is i64 and fn.argtypes[5] is vp and fn.argtypes[6] is C.c_size_t, name
        assert list(fn.argtypes[7:]) == tails[name], name


def test_the_abi_version_stays_and_its_comment_names_the_additions():
    abi.assert_version_and_struct_sizes(NEW)


def test_the_single_view_comments_keep_their_words():
    for proto in (r"#define GSR_MAX_FEATURE_CHANNELS 1024\s*int gsr_blend_channels\(", r"int gsr_blend_channels_backward\(", r"int gsr_blend_gaussian_stats\("):
        assert "Single views" in abi.header_comment_before(proto), proto


def test_the_header_states_the_contract():
    doc = re.sub(r"\s+\*?\s*", " ", abi.header_comment_before(r"int gsr_lists_views\("))
    for words in ("exact", "order the adds arrive in", "view_bits", "view_hits[i] +=", "bit for bit", "slice v", "output_layout = 1 is refused",
                  "GSR_ERR_WORKSPACE", "not all four", "required exactly when view_hits is given", "ignored on entry and undefined on return",
                  "before any HIP call"):
        assert words in doc, words


def _cams(n, sizes=None):
    from gsr_amd import _lib

    arr = (_lib.GsrCamera * n)()
    for j in range(n):
        arr[j].width, arr[j].height = (64, 48) if sizes is None else sizes[j]
    return arr


@pytest.mark.parametrize("entry", NEW)
def test_bad_arguments_are_refused_without_touching_a_gpu(entry):
    """Each refusal comes with its own gsr_last_error() text and before the workspace (NULL here) is even looked at.  The array
    arguments are host addresses nobody may dereference: a check that came too late would fault, not pass."""
    from gsr_amd import _lib

    fn = getattr(_lib.lib, entry)
    o, sc = _lib.default_options(), _lib.GsrScene()
    host = (C.c_float * 4)()
    p = C.addressof(host)
    plane = 64 * 48
    kind = {"gsr_lists_views": "lists", "gsr_blend_channels_views": "maps", "gsr_render_channels_batch": "maps",
            "gsr_blend_channels_backward_views": "grad", "gsr_blend_gaussian_stats_views": "stats"}[entry]
    scene_first = entry in ("gsr_lists_views", "gsr_render_channels_batch")

    def call(cams=None, n=2, opts=None, null_cams=False, null_opts=False, **kw):
        cams = _cams(max(n, 1)) if cams is None else cams
        head = (C.byref(sc),) if scene_first else (0,)
        pre = head + (None if null_cams else cams, n, None if null_opts else C.byref(opts or o), 100, None, 0)
        if kind == "lists":
            tail = ()
        elif kind == "maps":
            ch = kw.get("channels", 5)
            tail = (kw.get("features", p), ch, kw.get("feature_stride", 8), kw.get("out", p), kw.get("map_stride", plane * ch),
                    kw.get("T", p), kw.get("T_stride", plane))
        elif kind == "grad":
            ch = kw.get("channels", 5)
            tail = (kw.get("grad_maps", p), kw.get("map_stride", plane * ch), ch, kw.get("grad_features", p), kw.get("grad_stride", 8))
        else:
            tail = (kw.get("masks", p), kw.get("mask_stride", plane)) + kw.get("outs", (p, p, p, p, p))
        return fn(*pre, *tail, None)

    refused = abi.refused(entry)
    seen = [
        refused(call(null_cams=True), "null", "cameras"),
        refused(call(null_opts=True), "null", "options"),
        refused(call(cams=_cams(2, [(64, 48), (64, 32)])), "share one frame size"),
    ]
    if entry == "gsr_render_channels_batch":
        seen.append(refused(call(n=-1), "bad camera count"))
        assert call(n=0) == _lib.GSR_OK  # no camera, nothing to do
    else:
        seen.append(refused(call(n=0), "bad view count"))
        assert refused(call(cams=_cams(9), n=9), "bad view count") == seen[-1].replace(" 0 ", " 9 ")
    b = _lib.default_options()
    b.output_layout = 1
    seen.append(refused(call(opts=b), "output_layout = 1"))
    if kind != "lists":
        for field in ("output_dtype", "accum_dtype"):
            b = _lib.default_options()
            setattr(b, field, 1)
            seen.append(refused(call(opts=b), field))
    if kind == "maps":
        seen += [refused(call(features=None), "null", "features"), refused(call(out=None), "null", "output map"),
                 refused(call(channels=0), "bad channels"), refused(call(channels=5, feature_stride=4), "feature_stride"),
                 refused(call(map_stride=plane * 5 - 1), "map_stride", "smaller"), refused(call(T_stride=plane - 1), "T_stride", "smaller")]
        assert refused(call(channels=1025), "bad channels") != seen[-4]
    if kind == "grad":
        seen += [refused(call(grad_maps=None), "null", "gradient map"), refused(call(grad_features=None), "null", "feature gradient"),
                 refused(call(channels=0), "bad channels"), refused(call(grad_stride=4), "grad_stride"),
                 refused(call(map_stride=plane * 5 - 1), "map_stride", "smaller")]
    if kind == "stats":
        seen += [refused(call(outs=(None,) * 5), "null", "outputs", "four"), refused(call(outs=(p, p, p, p, None)), "view_hits", "view_bits"),
                 refused(call(outs=(p, p, p, None, p)), "view_bits", "without"), refused(call(mask_stride=plane - 1), "mask_stride", "smaller")]
    assert len(set(seen)) == len(seen)  # each case its own words
    # a tile-row shard's plane is its strip: two of the three tile rows of a 48-row frame
    if kind in ("maps", "grad"):
        strip = _lib.default_options()
        strip.output_layout, strip.tile_row_begin, strip.tile_row_step = 2, 0, 2
        refused(call(opts=strip, map_stride=64 * 32 * 5 - 1), "map_stride")
        assert "null" in refused(call(opts=strip, map_stride=64 * 32 * 5, T_stride=64 * 32), "null")
    # and with everything above in order the next check is the usual one: a null workspace (with a scene: the empty scene's
    # arrays) — still no GPU.  One view reads no stride; a final T / masks / any single output are optional
    good = [dict(), dict(n=1), dict(n=8, cams=_cams(8))]
    if kind == "maps":
        good += [dict(T=None, T_stride=0), dict(n=1, map_stride=0, T_stride=0)]
    if kind == "grad":
        good += [dict(n=1, map_stride=0)]
    if kind == "stats":
        good += [dict(masks=None, mask_stride=0), dict(n=1, mask_stride=0), dict(outs=(p, None, None, None, None)),
                 dict(outs=(None, None, None, p, p)), dict(outs=(None, p, p, None, None))]
    for kw in good:
        assert "null" in refused(call(**kw), "null"), kw
        for w in ("stride", "view count", "outputs", "output_dtype", "accum_dtype", "frame size"):
            assert w not in _lib.lib.gsr_last_error().decode(), (kw, w)


def test_the_refusal_of_several_views_stays_where_it_was():
    """pick, top-k, slab and the three-channel feature blend keep the refusal and its wording; the three kernels that take several
    views say so to weight_walk_begin explicitly."""
    src = {f: open(abi.CSRC + "/" + f).read() for f in ("blend_weight_walk.h", "blend_channels.hip", "blend_channels_backward.hip",
                                                        "blend_gstats.hip", "blend_pick.hip", "blend_topk.hip", "blend_slab.hip")}
    assert 'set_error("%s: single views only", noun)' in src["blend_weight_walk.h"]
    for f in ("blend_channels.hip", "blend_channels_backward.hip", "blend_gstats.hip"):
        assert "WalkViews::Several" in src[f] and "(unsigned)views)" in src[f], f
    for f in ("blend_pick.hip", "blend_topk.hip", "blend_slab.hip"):
        assert "WalkViews::Several" not in src[f], f


def test_view_stats_batch_refuses_bad_arguments_before_it_allocates():
    from gsr_amd import renderer

    R, VS = abi.rasterizer(), renderer.ViewStats
    cams = [abi.cam(), abi.cam(), abi.cam()]
    m = torch.ones((24, 40), dtype=torch.bool)
    vs = VS(torch.zeros(5), torch.zeros(5), torch.zeros(5, dtype=torch.int32))
    views = torch.zeros(5, dtype=torch.int32)
    bad = [
        dict(cams=[]), dict(cams=[abi.cam(), abi.cam(40, 32)]), dict(opts=renderer.make_options(output_layout=1)),
        dict(masks=[m, None]),                                           # one entry per camera
        dict(masks=[m, None, torch.ones((40, 24), dtype=torch.bool)]),   # the transposed shape
        dict(masks=[m, m.float(), None]), dict(masks=[m, [[1] * 40] * 24, None]),
        dict(want=()), dict(want=("sum", "mean")), dict(want="views"), dict(want=(3,)),
        dict(out=vs), dict(out=(vs, views, views)), dict(out=(tuple(vs)[:2], views)),
        dict(out=(vs, None)), dict(out=(vs, views.long())), dict(out=(vs, torch.zeros(4, dtype=torch.int32))),
        dict(out=(VS(None, vs.weight_max, vs.pixels), views)), dict(out=(VS(vs.weight_sum, vs.weight_max, vs.pixels.long()), views)),
    ]
    for kw in bad:
        kw = dict(kw)
        with pytest.raises(ValueError):
            R.view_stats_batch(kw.pop("cams", cams), **kw)
    for kw in (dict(), dict(masks=[m, None, m.to(torch.uint8)]), dict(out=(vs, views)), dict(want=["views"]),
               dict(out=(VS(None, None, None), views), want=("views",)), dict(out=(VS(None, vs.weight_max, None), None), want=("max",))):
        with pytest.raises(abi.NoWorkspace):
            R.view_stats_batch(cams, **kw)
    # nothing to draw: zeros, or `out` as it is, without a workspace
    st, v = abi.rasterizer(0).view_stats_batch(cams, want=("max", "views"))
    assert st.weight_sum is None and st.pixels is None and st.weight_max.shape == (0,) and v.dtype == torch.int32
    empty = renderer.make_options(tile_row_begin=2, tile_row_step=3, output_layout=2)  # two tile rows, the third of three shards
    st, v = R.view_stats_batch(cams, empty)
    assert all(t.shape == (5,) and not t.any() for t in tuple(st) + (v,))
    out = (VS(torch.full((5,), 2.0), torch.full((5,), 1.0), torch.full((5,), 4, dtype=torch.int32)), torch.full((5,), 3, dtype=torch.int32))
    got = R.view_stats_batch(cams, empty, out=out)
    assert all(a is b for a, b in zip(got[0], out[0])) and got[1] is out[1] and bool((out[1] == 3).all()) and bool((out[0].pixels == 4).all())


def test_the_map_and_gradient_batches_refuse_bad_views_before_they_allocate():
    from gsr_amd import renderer

    R = abi.rasterizer()
    F = torch.zeros((5, 6))
    for cams, opts in (([], None), ([abi.cam(), abi.cam(40, 32)], None), ([abi.cam()], renderer.make_options(output_layout=1))):
        with pytest.raises(ValueError):
            R.render_features_batch(cams, F, opts)
        with pytest.raises(ValueError):
            R.feature_gradient_batch(cams, torch.zeros((len(cams), 24, 40, 6)), opts)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        R.render_features_batch([abi.cam()], F)  # good views: the features are looked at next (there is no CPU path)
    # groups: `views` cameras at a time, fewer with batch_views or in the last group
    sizes = lambda opts, b: [len(a) for _, a in R._view_groups([abi.cam()] * b, opts)]
    assert sizes(renderer.make_options(), 9) == [4, 4, 1] and sizes(renderer.make_options(batch_views=2), 5) == [2, 2, 1]
    assert sizes(renderer.make_options(), 3) == [3] and [len(a) for _, a in abi.rasterizer(views=1)._view_groups([abi.cam()] * 3, renderer.make_options())] == [1, 1, 1]


def test_accumulate_view_stats_hands_a_rasterizer_with_slices_all_cameras_at_once():
    from gsr_amd import renderer

    calls, answer = [], object()

    class Stub:
        views = 4
        scene = types.SimpleNamespace(n=3, device=torch.device("cpu"), order_t=None)

        def view_stats_batch(self, cams, opts=None, masks=None, **kw):
            calls.append((list(cams), opts, list(masks), kw))
            return answer

        def view_stats(self, *a, **k):
            raise AssertionError("the per-camera loop is the path of a Rasterizer with one slice")

    assert renderer.accumulate_view_stats(Stub(), iter("abcde"), opts="O", masks=[None, "M", None, None, None]) is answer
    assert calls == [(list("abcde"), "O", [None, "M", None, None, None], {})]
    assert renderer.accumulate_view_stats(Stub(), "ab") is answer and calls[1][2] == [None, None]
    with pytest.raises(ValueError):
        renderer.accumulate_view_stats(Stub(), "ab", masks=[None])
    total, views = renderer.accumulate_view_stats(Stub(), [])  # no camera: zeros, no call
    assert len(calls) == 2 and views.shape == (3,) and not views.any() and not total.pixels.any()
