"""GPU: what the host side of every public single-view call of Rasterizer, and of its calls that take several views per launch
sequence, asks of libgsr — which entries, in which order, with which options — read off a recording proxy around renderer.lib that
forwards every call to the real library.

Three things per call, none of them a number the code under test produces:
  a. the entry sequence, written out below (CALLS);
  b. chaining: after an enqueue() that no stats() has read, every options struct the call passes before its first gsr_read_stats
     has keep_flags = 1 (0 with nothing unchecked), and a shard without tile rows calls no render, list or blend entry at all;
  c. the retry: on a rasterizer whose pair buffer (max_pairs = 64) is too small for the scene the attempt runs twice, max_pairs
     grows and the result is the roomy rasterizer's — bit for bit, except the float atomic sums (the gradient, weight_sum), which
     are held to the bar test_gpu_channels_backward applies between two runs of one gradient; a caller's `out` ends as what it
     held before plus ONE view's contribution: the overflowed first attempt added nothing.

Scene: gpu_cases.deep_tile_scene, 40 x 24 (1000 gaussians, two tile rows).  The batch rows (BATCH) take the one camera three times
through a Rasterizer(views=2): two groups, 2 + 1 views, the smallest case with a second group and a slice that is reset.  There
stats() reads one slice per view of the group; render_batch and render_features_batch are one entry for all groups, the other
two check each group's lists (gsr_lists_views) before the group's blend adds, with or without `out`; an `out` ends as what it
held before plus exactly the three views.
"""
import pytest
import torch

from gpu_cases import bar as _bar, deep_tile_scene as _deep_tile_scene

pytestmark = pytest.mark.gpu

STATS = ("gsr_read_stats",)
LISTS = ("gsr_preprocess", "gsr_bin_sort")
Z = ("gsr_project_to_camera_space",)
# call -> (entries before the checked attempt, entries of one attempt (gsr_read_stats follows each), entries after the last check)
CALLS = {
    "render": ((), ("gsr_render_forward",), ()),
    "features2": ((), ("gsr_render_features",), ()),
    "features5": ((), ("gsr_render_channels",), ()),
    "depth": (Z, ("gsr_render_features",), ()),
    "rgbd": (Z, LISTS + ("gsr_blend", "gsr_blend_features"), ()),
    "slab": ((), ("gsr_render_slab",), ()),
    "occluded": (("gsr_sh_to_rgb",), ("gsr_render_slab",), ()),
    "pick": ((), ("gsr_render_pick",), ()),
    "median_depth": ((), ("gsr_render_pick",), Z),
    "topk": ((), ("gsr_render_topk",), ()),
    "gradient": ((), ("gsr_render_channels_backward",), ()),
    "weights": ((), ("gsr_render_channels_backward",), ()),
    "view_stats": ((), ("gsr_render_gaussian_stats",), ()),
    "splat": ((), ("gsr_render_splat_backward",), ()),
    "gradient_out": ((), LISTS, ("gsr_blend_channels_backward",)),
    "weights_out": ((), LISTS, ("gsr_blend_channels_backward",)),
    "view_stats_out": ((), LISTS, ("gsr_blend_gaussian_stats",)),
    "splat_out": ((), LISTS, ("gsr_blend_splat_backward",)),
    # geometry_gradient: the splat gradient into the rasterizer's own [n, 8] scratch, as into any caller's `out`, then the projection
    "geometry": ((), LISTS, ("gsr_blend_splat_backward", "gsr_project_backward")),
    "geometry_out": ((), LISTS, ("gsr_blend_splat_backward", "gsr_project_backward")),
    "render_batch": ((), ("gsr_render_batch",), ()),
    "features_batch5": ((), ("gsr_render_channels_batch",), ()),
    "gradient_batch": ((), ("gsr_lists_views",), ("gsr_blend_channels_backward_views",)),
    "view_stats_batch": ((), ("gsr_lists_views",), ("gsr_blend_gaussian_stats_views",)),
    "gradient_batch_out": ((), ("gsr_lists_views",), ("gsr_blend_channels_backward_views",)),
    "view_stats_batch_out": ((), ("gsr_lists_views",), ("gsr_blend_gaussian_stats_views",)),
}
BATCH = tuple(name for name in CALLS if "batch" in name)  # three cameras through a Rasterizer(views=2); for these the triple is per group
# outputs that are float atomic sums (or, the geometry gradient, derived from them), by position in the result
ATOMIC = {"gradient": (0,), "weights": (0,), "view_stats": (0,), "gradient_batch": (0,), "view_stats_batch": (0,),
          "splat": (0, 1, 2), "geometry": (0, 1, 2, 3)}


class _Recorder:
    """renderer.lib with a note of every call: (entry name, the fields of the GsrOptions it was passed by reference, or None)."""

    def __init__(self, real, options_type):
        self._real, self._options_type, self.calls = real, options_type, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args):
            opts = [a._obj for a in args if isinstance(getattr(a, "_obj", None), self._options_type)]
            self.calls.append((name, {k: getattr(opts[0], k) for k, _ in self._options_type._fields_} if opts else None))
            return fn(*args)

        return call

    def names(self):
        return tuple(name for name, _ in self.calls)

    def options_before_the_first_check(self):
        names = self.names()
        head = self.calls[:names.index("gsr_read_stats")] if "gsr_read_stats" in names else self.calls
        return [o for _, o in head if o is not None]


@pytest.fixture(scope="module")
def S():
    from gsr_amd import renderer

    class NS:
        pass

    s = NS()
    assert torch.cuda.is_available(), "these tests need the MI355X"
    packed, args = _deep_tile_scene()
    s.renderer, s.cam = renderer, renderer.make_camera(*args)
    s.scene = renderer.GaussianScene.from_packed(packed)
    s.R = renderer.Rasterizer(s.scene)
    s.R.render(s.cam)
    s.R2 = renderer.Rasterizer(s.scene, views=2)
    s.R2.render(s.cam)
    gen = torch.Generator().manual_seed(23)
    s.F = torch.randn((s.scene.n, 5), generator=gen).cuda()
    s.G = torch.randn((s.cam.height, s.cam.width, 5), generator=gen).cuda()
    s.G3 = torch.randn((3, s.cam.height, s.cam.width, 5), generator=gen).cuda()
    s.roomy = {}
    return s


@pytest.fixture
def rec(S, monkeypatch):
    r = _Recorder(S.renderer.lib, S.renderer.GsrOptions)
    monkeypatch.setattr(S.renderer, "lib", r)
    return r


def _rows(S, o):
    """Pixel rows of the maps a call with options `o` lays out (a strip: its tile rows)."""
    return S.renderer.shard_rows(S.cam.height, o.tile_row_begin, o.tile_row_step, o.tile_row_block) * 16 if o.output_layout == 2 else S.cam.height


def _flat(res):
    """The tensors of a result, in order (view_stats_batch nests a ViewStats)."""
    return [t for r in (res if isinstance(res, tuple) else (res,)) if r is not None for t in (_flat(r) if isinstance(r, tuple) else (r,))]


def _run(S, R, name, o, outs=None):
    """One public call by its CALLS name -> the list of tensors it returns.  `outs`: the buffers of an accumulating call."""
    cam, rows, VS, GG = S.cam, _rows(S, o), S.renderer.ViewStats, S.renderer.GeometryGradient
    cams = [cam] * 3
    plane = lambda v: torch.full((rows, cam.width), v, dtype=torch.float32, device="cuda")
    if name.endswith("_out") and outs is None:
        outs = _zero_outs(S, name)
    call = {
        "render": lambda: R.render(cam, o, return_T=True),
        "features2": lambda: R.render_features(cam, S.F[:, :2], o, return_T=True),
        "features5": lambda: R.render_features(cam, S.F, o, return_T=True),
        "depth": lambda: R.render_depth(cam, o),
        "rgbd": lambda: R.render_rgbd(cam, o),
        "slab": lambda: R.render_slab(cam, S.F, plane(1.2), plane(2.6), o),
        "occluded": lambda: R.render_occluded(cam, plane(2.2), opts=o),
        "pick": lambda: R.render_pick(cam, o, count=True),
        "median_depth": lambda: R.render_median_depth(cam, o),
        "topk": lambda: R.render_topk(cam, 4, o, return_T=True),
        "gradient": lambda: R.feature_gradient(cam, S.G[:rows], o, scene_order=True),
        "weights": lambda: R.blend_weights(cam, o),
        "view_stats": lambda: R.view_stats(cam, o, scene_order=True),
        "splat": lambda: R.splat_gradient(cam, S.F, S.G[:rows], opts=o, scene_order=True),
        "geometry": lambda: R.geometry_gradient(cam, S.F, S.G[:rows], opts=o, scene_order=True),
        "gradient_out": lambda: R.feature_gradient(cam, S.G[:rows], o, out=outs[0]),
        "weights_out": lambda: R.blend_weights(cam, o, out=outs[0]),
        "view_stats_out": lambda: R.view_stats(cam, o, out=VS(*outs)),
        "splat_out": lambda: _splat_rows_of(R.splat_gradient(cam, S.F, S.G[:rows], opts=o, out=outs[0], scene_order=True), outs[0]),
        "geometry_out": lambda: R.geometry_gradient(cam, S.F, S.G[:rows], opts=o, out=GG(*outs), scene_order=True),
        "render_batch": lambda: R.render_batch(cams, o),
        "features_batch5": lambda: R.render_features_batch(cams, S.F, o, return_T=True),
        "gradient_batch": lambda: R.feature_gradient_batch(cams, S.G3[:, :rows], o, scene_order=True),
        "view_stats_batch": lambda: R.view_stats_batch(cams, o, scene_order=True),
        "gradient_batch_out": lambda: R.feature_gradient_batch(cams, S.G3[:, :rows], o, out=outs[0]),
        "view_stats_batch_out": lambda: R.view_stats_batch(cams, o, out=(VS(*outs[:3]), outs[3])),
    }[name]
    return _flat(call())


def _splat_rows_of(g, rows):
    """splat_gradient(out=rows) returns views of `rows`, columns (opacity, mean x, y, s0, s1, s2, -, -): the buffer itself."""
    assert g.abs_mean2d is None and [(t.data_ptr() - rows.data_ptr()) // 4 for t in g[:3]] == [1, 3, 0]
    assert (tuple(g.mean2d.shape), tuple(g.sigmas.shape), tuple(g.opacity.shape)) == ((len(rows), 2), (len(rows), 3), (len(rows),))
    assert all(t.stride(0) == 8 for t in g[:3]) or len(rows) == 0
    return rows


def _zero_outs(S, name):
    n = S.scene.n
    if name == "splat_out":
        return [torch.zeros((n, 8), device="cuda")]
    if name == "geometry_out":
        return [torch.zeros(s, device="cuda") for s in ((n, 3), (n, 3), (n, 4), (n,))]
    if name in ("gradient_out", "gradient_batch_out"):
        return [torch.zeros((n, 5), device="cuda")]
    if name == "weights_out":
        return [torch.zeros(n, device="cuda")]
    counts = 2 if name == "view_stats_batch_out" else 1  # pixels, and the batch's views
    return [torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")] + [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(counts)]


def _sequence(name, attempts):
    pre, attempt, post = CALLS[name]
    if name not in BATCH:
        return pre + (attempt + STATS) * attempts + post
    if not post:  # one entry for both groups; stats() then reads the two slices
        return (attempt + STATS * 2) * attempts
    # two phases per group: the first group's lists run `attempts` times, the second group (one view) finds the room they made
    return (attempt + STATS * 2) * attempts + post + attempt + STATS + post


def _adds_after_the_check(name):
    """The call's blend adds into a buffer, so it runs after its lists were checked: with `out`, the two batches always, and
    geometry_gradient, whose splat gradient goes into a scratch as into an `out`."""
    return name.endswith("_out") or name in ("gradient_batch", "view_stats_batch", "geometry")


def _rasterizer(S, name):
    return S.R2 if name in BATCH else S.R


def _check_closing_blend(rec, name):
    """An accumulating call's blend runs once, after the last check (first of the entries that follow it), with colour_stage = 0 and
    the depth-sort bound its lists got."""
    k = len(CALLS[name][2])
    (blend, bo), (sort, so) = rec.calls[-k], rec.calls[-k - 2]
    assert blend == CALLS[name][2][0] and sort == ("gsr_lists_views" if name in BATCH else "gsr_bin_sort"), rec.names()
    assert bo["colour_stage"] == 0 and bo["depth_sort_passes"] == so["depth_sort_passes"], (name, bo, so)


@pytest.mark.parametrize("name", list(CALLS))
def test_entries_and_chaining(S, rec, name):
    R, mk = _rasterizer(S, name), S.renderer.make_options
    assert R.unchecked.slices == 0
    # a. nothing unchecked: the sequence, and no struct asks to keep a record.  The accumulating calls get colour_stage = 1 from the
    #    caller, which their lists and their blend must not run with.
    _run(S, R, name, mk(colour_stage=1) if _adds_after_the_check(name) else mk())
    assert rec.names() == _sequence(name, 1), name
    assert rec.options_before_the_first_check() and all(o["keep_flags"] == 0 for o in rec.options_before_the_first_check()), name
    assert R.sort_passes > 0 and all(o["depth_sort_passes"] == R.sort_passes for o in rec.options_before_the_first_check()), name
    if _adds_after_the_check(name):
        _check_closing_blend(rec, name)
    if name in BATCH:  # every struct of the call, the second group's included
        assert all(o["keep_flags"] == 0 for _, o in rec.calls if o is not None), name
    # b. one frame enqueued and not read: the call adds to its record
    R.enqueue(S.cam)
    assert R.unchecked.slices == 1
    del rec.calls[:]
    _run(S, R, name, mk())
    assert rec.names() == _sequence(name, 1), name
    assert rec.options_before_the_first_check() and all(o["keep_flags"] == 1 for o in rec.options_before_the_first_check()), name
    assert R.unchecked.slices == 0
    if name in BATCH:  # the first group adds to the record (its blend runs with its lists' options); the second starts from a read one
        assert [o["keep_flags"] for _, o in rec.calls if o is not None] == ([1, 1, 0, 0] if CALLS[name][2] else [1]), name
    # a shard without tile rows (two tile rows, the third of three shards): no render, list or blend entry is called
    del rec.calls[:]
    outs = [torch.full_like(t, 3) for t in _zero_outs(S, name)] if name.endswith("_out") else None
    res = _run(S, R, name, mk(tile_row_begin=2, tile_row_step=3, output_layout=2), outs)
    assert not [c for c in rec.names() if c.startswith(("gsr_render_", "gsr_blend")) or c in LISTS], (name, rec.names())
    if outs is not None:
        assert all(bool((t == 3).all()) for t in outs)
    else:
        assert all(not t.any() if name in ATOMIC else t.numel() == 0 for t in res), name  # per-gaussian results: zeros; maps: no rows
    R.stats()


def _roomy(S, name):
    """What the roomy rasterizer returns for the call (scene order), computed once."""
    base = name[:-4] if name.endswith("_out") else name
    if base not in S.roomy:
        S.roomy[base] = _run(S, _rasterizer(S, base), base, S.renderer.make_options())
    return S.roomy[base]


@pytest.mark.parametrize("name", list(CALLS))
def test_an_overflowed_attempt_is_run_again_and_leaves_no_trace(S, rec, name):
    ref = _roomy(S, name)
    del rec.calls[:]
    small = S.renderer.Rasterizer(S.scene, max_pairs=64, views=2 if name in BATCH else 1)
    if not name.endswith("_out"):
        got = _run(S, small, name, S.renderer.make_options())
        assert rec.names() == _sequence(name, 2), (name, rec.names())
        assert small.max_pairs > 64
        if _adds_after_the_check(name):
            _check_closing_blend(rec, name)
        assert len(got) == len(ref)
        for k, (g, r) in enumerate(zip(got, ref)):
            if k in ATOMIC.get(name, ()):
                _bar(f"{name}[{k}] after a retry", g.cpu().numpy(), r.cpu().numpy())
            else:
                assert g.dtype == r.dtype and torch.equal(g, r), (name, k)
        return
    # accumulating: `before` + one view.  Sums start from the view's own value (so the bar is taken at twice it), the maximum from
    # the median of the view's positive maxima (gaussians on either side of it), the pixel counts from 7.
    if name == "weights_out":  # blend_weights without `out` answers in file order, `out` is in the scene's
        o_t = S.scene.order_t
        ref = ref if o_t is None else [ref[0].index_select(0, o_t)]
    if name == "splat_out":  # the [n, 8] rows of the three fields; columns 6 and 7 stay as they are without abs_mean
        ref = [torch.cat([ref[2][:, None], ref[0], ref[1], torch.zeros_like(ref[0])], 1)]
    outs = [r.clone() for r in ref] if name in ("splat_out", "geometry_out") else [ref[0].clone()]
    if name in ("view_stats_out", "view_stats_batch_out"):
        mid = float(ref[1][ref[1] > 0].median())
        outs += [torch.full_like(ref[1], mid)] + [torch.full_like(r, 7) for r in ref[2:]]
    got = _run(S, small, name, S.renderer.make_options(), outs)
    assert rec.names() == _sequence(name, 2), (name, rec.names())
    assert small.max_pairs > 64
    _check_closing_blend(rec, name)
    assert all(g is o for g, o in zip(got, outs))
    for k in range(len(outs) if name in ("splat_out", "geometry_out") else 1):
        _bar(f"{name}[{k}] sum after a retry", outs[k].cpu().numpy(), 2.0 * ref[k].double().cpu().numpy())
    if name in ("view_stats_out", "view_stats_batch_out"):
        assert bool((ref[1] > mid).any()) and bool(((ref[1] > 0) & (ref[1] < mid)).any())
        assert torch.equal(outs[1], torch.clamp(ref[1], min=mid)) and all(torch.equal(o, r + 7) for o, r in zip(outs[2:], ref[2:]))


def test_the_per_gaussian_calls_refuse_before_they_allocate_and_an_empty_shard_reaches_no_workspace(S, rec):
    """The accumulating calls a CPU stub cannot reach (their first look is whether a tensor lives on the GPU): a bad `out`, grad_T or
    splat_rows is refused with ValueError, good arguments get as far as the workspace, and a shard without tile rows gets zeros —
    or `out` back, bit for bit as it was — without one.  A five-gaussian scene in file order, 40 x 24; no kernel of the render path
    runs (gsr_project_backward over rows of zeros may: it adds nothing)."""
    renderer, cam, GG = S.renderer, S.cam, S.renderer.GeometryGradient
    gen = torch.Generator().manual_seed(5)
    q = torch.randn((5, 4), generator=gen)
    packed = dict(means=torch.tensor([[0.0, 0.0, 2.0]]) + 0.1 * torch.randn((5, 3), generator=gen), log_scales=torch.full((5, 3), -3.0),
                  quats=q / q.norm(dim=1, keepdim=True), opacity_logit=torch.zeros(5), sh=torch.zeros((5, 16, 3)))
    scene = renderer.GaussianScene.from_packed({k: v.numpy() for k, v in packed.items()}, spatial_order=False)
    R = renderer.Rasterizer(scene, views=2)

    class NoWorkspace(Exception):
        pass

    def no_workspace(*a, **k):
        raise NoWorkspace()

    R._workspace = no_workspace
    z = lambda *shape, **kw: torch.zeros(shape, device="cuda", **kw)
    F, G, T = z(5, 2), z(24, 40, 2), z(24, 40)
    geo = GG(z(5, 3), z(5, 3), z(5, 4), z(5))
    calls = {  # name -> (the call with `out`, a good out, bad ones)
        "gradient": (lambda o, out: R.feature_gradient(cam, G[:_rows(S, o)], o, out=out), z(5, 2),
                     [z(5, 3), z(4, 2), z(5, 2, dtype=torch.float64), torch.zeros((5, 2)), z(2, 5).t(), z(10)]),
        "gradient_batch": (lambda o, out: R.feature_gradient_batch([cam] * 3, z(3, 24, 40, 2)[:, :_rows(S, o)], o, out=out), z(5, 8)[:, 2:4],
                           [z(5, 3), z(5, 2, dtype=torch.float16), torch.zeros((5, 2)), z(5, 4)[:, ::2]]),
        "splat": (lambda o, out: R.splat_gradient(cam, F, G[:_rows(S, o)], T[:_rows(S, o)], o, out=out), z(5, 8),
                  [z(5, 7), z(8, 5), z(5, 8, dtype=torch.float64), torch.zeros((5, 8)), z(5, 16)[:, ::2], z(8, 5).t()]),
        "geometry": (lambda o, out: R.geometry_gradient(cam, F, G[:_rows(S, o)], T[:_rows(S, o)], o, out=out), geo,
                     [GG(None, None, None, None), tuple(geo)[:3], geo._replace(means=z(5, 4)), geo._replace(quats=z(5, 4, dtype=torch.float64)),
                      geo._replace(log_scales=torch.zeros((5, 3))), geo._replace(opacity_logit=z(10)[::2]), geo._replace(quats=z(4, 5).t())]),
    }
    mk = renderer.make_options
    empty = mk(tile_row_begin=2, tile_row_step=3, output_layout=2)  # two tile rows, the third of three shards
    for name, (call, good, bad) in calls.items():
        for out in bad:
            with pytest.raises(ValueError, match="out"):
                call(mk(), out)
        for out in (None, good):
            with pytest.raises(NoWorkspace):
                call(mk(), out)
        res = _flat(call(empty, None))
        assert res and all(t.shape[0] == 5 and t.is_cuda and not t.any() for t in res), name
        outs = _flat(good)
        for t in outs:
            t.fill_(3.0)
        got = _flat(call(empty, good))
        held = {t.untyped_storage().data_ptr() for t in outs}
        assert all(bool((t == 3.0).all()) for t in outs) and all(g.untyped_storage().data_ptr() in held for g in got), name
        assert R.unchecked.slices == 0 and not R.unchecked.empty, name  # the shard left no mark
    # grad_T and the splat rows
    for bad_T in (z(40, 24), torch.zeros((24, 40)), z(24, 40, 1), 1.0):
        with pytest.raises(ValueError, match="grad_T"):
            R.splat_gradient(cam, F, G, bad_T)
        with pytest.raises(ValueError, match="grad_T"):
            R.geometry_gradient(cam, F, G, bad_T)
    for bad_rows in (z(5, 7), z(4, 8), z(5, 8, dtype=torch.float64), z(5, 16)[:, ::2], z(8, 5).t()):
        with pytest.raises(ValueError, match="splat_rows"):
            renderer.project_backward(scene, cam, bad_rows)
    with pytest.raises(RuntimeError, match="no CPU path"):
        renderer.project_backward(scene, cam, torch.zeros((5, 8)))
    for out in calls["geometry"][2]:
        with pytest.raises(ValueError, match="out"):
            renderer.project_backward(scene, cam, z(5, 8), out=out)
    assert set(rec.names()) <= {"gsr_project_backward"}, rec.names()
    assert R._ws is None
