"""GPU: feature maps, their gradient and the view statistics for several views per launch sequence (gsr_lists_views,
gsr_blend_channels_views, gsr_blend_channels_backward_views, gsr_blend_gaussian_stats_views, gsr_render_channels_batch;
Rasterizer.render_features_batch, feature_gradient_batch, view_stats_batch, renderer.accumulate_view_stats).

The reference is always the existing single-view method on a Rasterizer of one slice, never the code under test: maps, final T,
weight_max, pixels and the view count are held bit for bit (torch.equal), the float atomic sums at the project's standing bar
(gpu_cases.bar: 100 dB per channel, peak = max |reference channel|) against float64 sums of the single-view results.

Scenes: gpu_cases.wall_scene() (32x16, two tiles, lists past one 256-entry batch: several flushes per tile) and deep_tile_scene()
(40x24) under five translations of their own camera, and the 60 000-gaussian medium scene at 640x360 under ring_cameras(25)[::3]
— nine views, so the last group is partial for K = 2, 4 and 8.  The tests assert that the views differ and that some gaussian is
reached in some views but not in all: a pass is not vacuous.
"""
import itertools

import numpy as np
import pytest
import torch

from gpu_cases import bar as _bar, deep_tile_scene, medium_columns, namespace, wall_scene

pytestmark = pytest.mark.gpu

# Translations of the small scenes' own camera (added to its tvec).  The focal length is ~28 px (wall) / ~35 px (deep) and the
# gaussians lie at z = 1 .. 3, so the small ones move a few pixels and the last two move the frame by 10 - 40 px: further than the
# 3-sigma reach (< 18 px) of the small gaussians near the far edge, which therefore leave those views while the others stay.
SHIFTS = ((0.0, 0.0, 0.0), (0.12, 0.0, 0.0), (-0.2, 0.08, 0.0), (-0.9, 0.4, 0.04), (1.5, 0.2, 0.0))
SMALL = ("wall", "deep")
STAT_FIELDS = ("n_visible", "n_pairs_bbox", "n_pairs", "sort_passes", "wave_entries", "fetched_entries")
N_F = 36  # feature columns: the widest map (33) and a window that starts at column 2


@pytest.fixture(scope="module")
def G():
    return namespace()


def _case(G, name):
    """The scene (Morton-ordered, like every loaded scene), its cameras, a one-slice Rasterizer for the references, features in
    file order and per-view upstream gradients; computed once and only read."""
    key = "views_" + name
    if key not in G.cases:
        mk = G.renderer.make_camera
        if name == "medium":
            cols, args = medium_columns(G, n=60_000)
            packed = G.utils.pack_gaussians(cols)
            cams = [mk(p.qvec, p.tvec, *args[2:]) for p in G.synthetic.ring_cameras(25)[::3]]
        else:
            packed, args = (wall_scene() if name == "wall" else deep_tile_scene())[:2]
            cams = [mk(args[0], np.asarray(args[1], np.float64) + np.array(s), *args[2:]) for s in SHIFTS]
        scene = G.renderer.GaussianScene.from_packed(packed)
        gen = torch.Generator().manual_seed(41)
        F = (torch.randn((scene.n, N_F), generator=gen) * 20.0).cuda()
        Gm = torch.randn((len(cams), cams[0].height, cams[0].width, 17), generator=gen).cuda()
        G.cases[key] = dict(scene=scene, cams=cams, R1=G.renderer.Rasterizer(scene), F=F, Gm=Gm, ref={})
    return G.cases[key]


def _batch(G, c, K, **kw):
    return G.renderer.Rasterizer(c["scene"], views=K, **kw)


def _single_maps(G, c, C, tag="", **okw):
    """(maps [B,..,C], Ts [B,..], per-view counters) of the single-view render_features under make_options(**okw); cached."""
    key = ("maps", C, tag, tuple(sorted(okw.items())))
    if key not in c["ref"]:
        R1, maps, Ts, stats = c["R1"], [], [], []
        for cam in c["cams"]:
            m, T = R1.render_features(cam, c["F"][:, :C], G.renderer.make_options(**okw), return_T=True)
            maps.append(m), Ts.append(T), stats.append(dict(R1.last_stats))
        c["ref"][key] = (torch.stack(maps), torch.stack(Ts), stats)
    return c["ref"][key]


def _forward_agrees(G, c, K, C, batch_views=0, n_cams=None, check_stats=True, R=None, **okw):
    cams = c["cams"][:n_cams]
    B = len(cams)
    maps, Ts, stats = _single_maps(G, c, C, **okw)
    R = R or _batch(G, c, K)
    out, T = R.render_features_batch(cams, c["F"][:, :C], G.renderer.make_options(batch_views=batch_views, **okw), return_T=True)
    tag = (K, C, batch_views, B, okw)
    assert out.shape == maps[:B].shape and T.shape == Ts[:B].shape, tag
    assert torch.equal(out, maps[:B]), tag
    assert torch.equal(T, Ts[:B]), tag
    alone = R.render_features_batch(cams, c["F"][:, :C], G.renderer.make_options(batch_views=batch_views, **okw))
    assert torch.equal(alone, maps[:B]), tag  # without a final T
    if check_stats and out.numel():  # (a shard without tile rows runs nothing) slice j holds the last view rendered there
        k = min(K, batch_views or K, B)
        assert len(R.last_slice_stats) == k, tag
        for j in range(k):
            i = max(i for i in range(B) if i % k == j)
            assert {f: R.last_slice_stats[j][f] for f in STAT_FIELDS} == {f: stats[i][f] for f in STAT_FIELDS}, (tag, j, i)
    return R


# ---- 1: forward ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_the_small_scenes_views_differ(G, name):
    c = _case(G, name)
    maps, Ts, stats = _single_maps(G, c, 17)
    assert sum(not torch.equal(maps[0], maps[j]) for j in range(1, len(maps))) >= 2, name
    assert len({s["n_pairs"] for s in stats}) >= 2, name
    assert min(s["wave_entries"] for s in stats) > 0, name


@pytest.mark.parametrize("name", SMALL)
@pytest.mark.parametrize("C", (1, 3, 17, 33))
def test_forward_maps_and_T_are_the_single_views(G, name, C):
    c = _case(G, name)
    for K in (2, 3, 4, 8):
        _forward_agrees(G, c, K, C)
    _forward_agrees(G, c, 8, C, n_cams=3)        # fewer views than slices
    _forward_agrees(G, c, 8, C, batch_views=2)   # batch_views caps K
    _forward_agrees(G, c, 1, C)                  # groups of one


@pytest.mark.parametrize("K,C", ((2, 17), (4, 33), (8, 17), (4, 1)))
def test_forward_medium_scene_partial_last_group(G, K, C):
    _forward_agrees(G, _case(G, "medium"), K, C)


@pytest.mark.parametrize("okw", (dict(fine_binning=True), dict(no_footprint_cull=True), dict(draw_limit=120), dict(reference_compat=False),
                                 dict(early_out_T=1e-4), dict(output_layout=2, tile_row_begin=1, tile_row_step=2)),
                         ids=lambda o: "-".join(o))
def test_forward_options(G, okw):
    for name, K in (("wall", 3), ("deep", 4), ("medium", 4)):
        _forward_agrees(G, _case(G, name), K, 17, **okw)


def test_forward_column_window_in_scene_order(G):
    for name in ("wall", "medium"):
        c = _case(G, name)
        window = c["F"][:, 2:19]
        assert not window.is_contiguous()
        ref = torch.stack([c["R1"].render_features(cam, window, scene_order=True) for cam in c["cams"]])
        got = _batch(G, c, 4).render_features_batch(c["cams"], window, scene_order=True)
        assert torch.equal(got, ref), name
        assert not torch.equal(got, _batch(G, c, 4).render_features_batch(c["cams"], window))  # (not in file order: the flag matters)


def test_forward_recovers_from_a_small_pair_buffer_and_a_small_sort_bound(G):
    c = _case(G, "medium")
    R = _batch(G, c, 4, max_pairs=2048)
    _forward_agrees(G, c, 4, 17, R=R, check_stats=False)
    assert R.max_pairs > 2048
    assert R.sort_passes > 1
    R.sort_passes = 1  # a learned bound that is too small: the frames come back short of passes and are re-rendered
    _forward_agrees(G, c, 4, 17, R=R)
    assert R.sort_passes > 1


# ---- 2: backward -----------------------------------------------------------------------------------------------------------------
def _single_gradient(G, c, C=17, scene_order=False):
    """float64 sum over the views of the single-view feature_gradient; cached."""
    key = ("grad", C, scene_order)
    if key not in c["ref"]:
        total = torch.zeros((c["scene"].n, C), dtype=torch.float64, device="cuda")
        for v, cam in enumerate(c["cams"]):
            total += c["R1"].feature_gradient(cam, c["Gm"][v, ..., :C], scene_order=scene_order).double()
        c["ref"][key] = total
    return c["ref"][key]


@pytest.mark.parametrize("name", SMALL + ("medium",))
def test_backward_is_the_sum_of_the_single_view_gradients(G, name):
    c = _case(G, name)
    ref = _single_gradient(G, c).cpu().numpy()
    never = ~ref.any(1)
    assert (~never).sum() >= 50 and (never.any() or name == "wall"), name  # (every gaussian of the wall lies in some view's frame)
    for K in (2, 4, 8):
        got = _batch(G, c, K).feature_gradient_batch(c["cams"], c["Gm"])
        assert got.shape == ref.shape and got.dtype == torch.float32
        _bar(f"{name} K={K}", got.cpu().numpy(), ref)
        assert not got[torch.from_numpy(never).cuda()].any(), (name, K)  # rows of gaussians no view draws stay exactly 0
    for C in (1, 33):  # a narrow walk alone; two wide walks and a narrow one
        Gc = c["Gm"][..., :1].expand(-1, -1, -1, C).contiguous() if C == 1 else torch.cat([c["Gm"], c["Gm"][..., :16] * 0.5], -1)
        want = torch.zeros((c["scene"].n, C), dtype=torch.float64, device="cuda")
        for v, cam in enumerate(c["cams"]):
            want += c["R1"].feature_gradient(cam, Gc[v]).double()
        _bar(f"{name} C={C}", _batch(G, c, 4).feature_gradient_batch(c["cams"], Gc).cpu().numpy(), want.cpu().numpy())


@pytest.mark.parametrize("name", SMALL)
def test_backward_against_the_weights_of_one_hot_maps(G, name):
    """sum_v sum_p W_v[i](p) G_v[p] in float64, the weights from one-hot render_features maps (file order)."""
    c = _case(G, name)
    n = c["scene"].n
    eye = torch.eye(n, dtype=torch.float32, device="cuda")
    ref = torch.zeros((n, 17), dtype=torch.float64, device="cuda")
    for v, cam in enumerate(c["cams"]):
        W = c["R1"].render_features(cam, eye).double().reshape(-1, n)
        ref += W.t() @ c["Gm"][v].double().reshape(-1, 17)
    _bar(name, _batch(G, c, 3).feature_gradient_batch(c["cams"], c["Gm"]).cpu().numpy(), ref.cpu().numpy())


@pytest.mark.parametrize("return_T", (False, True))
def test_autograd_through_the_batch(G, return_T):
    for name in ("wall", "medium"):
        c = _case(G, name)
        F = c["F"][:, :17].clone().requires_grad_(True)
        res = _batch(G, c, 4).render_features_batch(c["cams"], F, return_T=return_T)
        out = res[0] if return_T else res
        assert out.requires_grad and (not return_T or not res[1].requires_grad)
        assert torch.equal(out.detach(), _single_maps(G, c, 17)[0]), name
        (out * c["Gm"]).sum().backward()
        F1 = c["F"][:, :17].clone().requires_grad_(True)
        ref = torch.zeros_like(F1, dtype=torch.float64)
        for v, cam in enumerate(c["cams"]):
            F1.grad = None
            (c["R1"].render_features(cam, F1) * c["Gm"][v]).sum().backward()
            ref += F1.grad.double()
        _bar(f"{name} autograd T={return_T}", F.grad.cpu().numpy(), ref.cpu().numpy())


def test_backward_out_accumulates(G):
    for name in ("deep", "medium"):
        c = _case(G, name)
        ref = _single_gradient(G, c, scene_order=True).cpu().numpy()
        R = _batch(G, c, 4)
        wide = torch.zeros((c["scene"].n, 20), dtype=torch.float32, device="cuda")
        out = wide[:, 1:18]  # rows further apart than their channels
        assert R.feature_gradient_batch(c["cams"], c["Gm"], out=out) is out
        _bar(name + " once", out.cpu().numpy(), ref)
        R.feature_gradient_batch(c["cams"], c["Gm"], out=out)
        _bar(name + " twice", out.cpu().numpy(), 2.0 * ref)
        assert not wide[:, 0].any() and not wide[:, 18:].any()
        _bar(name + " scene order", R.feature_gradient_batch(c["cams"], c["Gm"], scene_order=True).cpu().numpy(), ref)


# ---- 3: statistics ---------------------------------------------------------------------------------------------------------------
def _masks(c, kind):
    """Per-view masks: `some` — a rectangle, None, a checkerboard, ...; `empty` — the same with view 1 masked out whole."""
    cam, B = c["cams"][0], len(c["cams"])
    H, W = cam.height, cam.width
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    pool = [(xx >= W // 4) & (yy < 3 * H // 4), None, ((xx // 3 + yy // 2) % 2 == 0).to(torch.uint8), xx < W // 2, None]
    masks = [pool[j % len(pool)] for j in range(B)]
    if kind == "empty":
        masks[1] = torch.zeros((H, W), dtype=torch.bool, device="cuda")
    return masks


def _single_stats(G, c, kind=None):
    """(sum float64, max, pixels, views) over the single-view view_stats, file order; cached."""
    key = ("stats", kind)
    if key not in c["ref"]:
        n = c["scene"].n
        masks = _masks(c, kind) if kind else [None] * len(c["cams"])
        s = torch.zeros(n, dtype=torch.float64, device="cuda")
        m = torch.zeros(n, dtype=torch.float32, device="cuda")
        p = torch.zeros(n, dtype=torch.int32, device="cuda")
        v = torch.zeros(n, dtype=torch.int32, device="cuda")
        for cam, mask in zip(c["cams"], masks):
            st = c["R1"].view_stats(cam, mask=mask)
            s += st.weight_sum.double()
            m = torch.maximum(m, st.weight_max)
            p += st.pixels
            v += (st.pixels > 0).to(torch.int32)
        c["ref"][key] = (s, m, p, v)
    return c["ref"][key]


def _stats_agree(tag, got, ref):
    (st, views), (s, m, p, v) = got, ref
    if st.weight_max is not None:
        assert st.weight_max.dtype == torch.float32 and torch.equal(st.weight_max, m), tag
    if st.pixels is not None:
        assert st.pixels.dtype == torch.int32 and torch.equal(st.pixels, p), tag
    if views is not None:
        assert views.dtype == torch.int32 and torch.equal(views, v), tag
    if st.weight_sum is not None:
        _bar(tag, st.weight_sum.cpu().numpy()[:, None], s.cpu().numpy()[:, None])


@pytest.mark.parametrize("name", SMALL + ("medium",))
def test_statistics_are_the_single_views_accumulated(G, name):
    c = _case(G, name)
    ref = _single_stats(G, c)
    B, v = len(c["cams"]), ref[3]
    assert bool(((v > 0) & (v < B)).any()), name  # some gaussian is reached in some views but not in all of them
    for K in (2, 4, 8):
        R = _batch(G, c, K)
        got = R.view_stats_batch(c["cams"])
        _stats_agree(f"{name} K={K}", got, ref)
        again = R.view_stats_batch(c["cams"])  # two runs: the exact fields bit for bit
        assert torch.equal(again[0].weight_max, got[0].weight_max) and torch.equal(again[0].pixels, got[0].pixels) and torch.equal(again[1], got[1])
    _stats_agree(name + " groups of one", _batch(G, c, 1).view_stats_batch(c["cams"]), ref)
    _stats_agree(name + " batch_views", _batch(G, c, 8).view_stats_batch(c["cams"], G.renderer.make_options(batch_views=3)), ref)


@pytest.mark.parametrize("name", ("wall", "medium"))
def test_statistics_under_per_view_masks(G, name):
    c = _case(G, name)
    B = len(c["cams"])
    for kind in ("some", "empty"):
        ref = _single_stats(G, c, kind)
        _stats_agree(f"{name} {kind}", _batch(G, c, 4).view_stats_batch(c["cams"], masks=_masks(c, kind)), ref)
    some, empty = _single_stats(G, c, "some")[3], _single_stats(G, c, "empty")[3]
    assert not torch.equal(_single_stats(G, c)[2], _single_stats(G, c, "some")[2])  # the masks leave pixels out
    # a view masked out whole is not counted ("some" leaves that view unmasked)
    assert int(empty.max()) <= B - 1 and bool((empty <= some).all()) and bool((empty < some).any())


def test_statistics_every_want_subset(G):
    c = _case(G, "wall")
    ref = _single_stats(G, c)
    names = G.renderer.VIEW_STATS_BATCH
    R = _batch(G, c, 4)
    for r in range(1, 5):
        for want in itertools.combinations(names, r):
            st, views = R.view_stats_batch(c["cams"], want=want)
            have = tuple(t is not None for t in tuple(st) + (views,))
            assert have == tuple(w in want for w in names), want
            _stats_agree(f"want={want}", (st, views), ref)


def test_statistics_out_accumulates(G):
    for name in ("deep", "medium"):
        c = _case(G, name)
        s, m, p, v = _single_stats(G, c)
        o_t = c["scene"].order_t  # `out` is in the scene's order: row j of the scene is row o_t[j] of the file
        n = c["scene"].n
        VS = G.renderer.ViewStats
        out = (VS(torch.zeros(n, device="cuda"), torch.full((n,), 0.25, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")),
               torch.zeros(n, dtype=torch.int32, device="cuda"))
        R = _batch(G, c, 4)
        got = R.view_stats_batch(c["cams"], out=out)
        assert all(a is b for a, b in zip(got[0], out[0])) and got[1] is out[1]
        R.view_stats_batch(c["cams"], out=out)
        assert torch.equal(out[0].weight_max, torch.maximum(m, torch.full_like(m, 0.25))[o_t]), name
        assert torch.equal(out[0].pixels, 2 * p[o_t]) and torch.equal(out[1], 2 * v[o_t]), name
        _bar(name + " twice", out[0].weight_sum.cpu().numpy()[:, None], 2.0 * s[o_t].cpu().numpy()[:, None])
        assert bool((m < 0.25).any()) and bool((m > 0.25).any()), name  # the preset decides some rows and not others


def test_accumulate_view_stats_takes_the_batch_path(G):
    acc = G.renderer.accumulate_view_stats
    for name in ("wall", "medium"):
        c = _case(G, name)
        for masks in (None, _masks(c, "some")):
            (st1, v1), (st4, v4) = acc(c["R1"], c["cams"], masks=masks), acc(_batch(G, c, 4), c["cams"], masks=masks)
            assert torch.equal(st4.weight_max, st1.weight_max) and torch.equal(st4.pixels, st1.pixels) and torch.equal(v4, v1), name
            _bar(name + " accumulate", st4.weight_sum.cpu().numpy()[:, None], st1.weight_sum.double().cpu().numpy()[:, None])
        assert bool(((v1 > 0) & (v1 < len(c["cams"]))).any()), name


# ---- 4: neighbours on the workspace ------------------------------------------------------------------------------------------------
def test_colour_batches_and_single_view_calls_around_the_feature_batches(G):
    c = _case(G, "medium")
    cams, R1 = c["cams"], c["R1"]
    frames = torch.stack([R1.render(cam) for cam in cams])
    R = _batch(G, c, 4)
    assert torch.equal(R.render_batch(cams), frames)
    _forward_agrees(G, c, 4, 17, R=R)
    R.feature_gradient_batch(cams, c["Gm"])
    _stats_agree("between batches", R.view_stats_batch(cams), _single_stats(G, c))
    assert torch.equal(R.render_batch(cams), frames)
    pick, ref = R.render_pick(cams[2], count=True), R1.render_pick(cams[2], count=True)  # pick stays a single-view walk on slice 0
    assert all(torch.equal(a, b) for a, b in zip(pick, ref))
    assert torch.equal(R.render_features(cams[1], c["F"][:, :17]), _single_maps(G, c, 17)[0][1])
    _forward_agrees(G, c, 4, 17, R=R)
