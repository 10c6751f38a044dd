"""GPU: per-gaussian view statistics (gsr_blend_gaussian_stats / gsr_render_gaussian_stats, csrc/blend_gstats.hip;
Rasterizer.view_stats, visible_ids, renderer.accumulate_view_stats): weight_sum[i] = sum_p w_i(p), weight_max[i] = max_p w_i(p),
pixels[i] = #{p : w_i(p) > 0} over the counted pixels of a view.

The first reference is the feature blend itself: a one-hot feature column through render_features returns a gaussian's weight map
with the walk's own bits (every other gaussian adds fma(w, 0, acc) = acc), 16 gaussians per walk.  Against those maps the maximum
and the count are exact (torch.equal: a maximum over bit patterns and an integer count do not depend on the order the atomics
arrive in); the float atomic sum is held to the project's standing bar, PSNR >= MIN_DB = 100 dB with peak = max of the reference,
against the float64 sums of the maps.  The second reference is the oracle's weight maps (the one-hot orc.composite method of
test_gpu_channels_backward), independent of any GPU path, with the same bar for the maximum and the sum.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_cases import bar as _bar, build as _build, gradient_case as _case, namespace, sample as _sample, weight_maps as _weight_maps

pytestmark = pytest.mark.gpu

SMALL = ["f1", "f3a", "f3b"]
SAMPLED = ["f2", "f5", "medium", "wall"]
PER_WALK = 16


class OneThreadOracle:
    """The oracle with one thread per composite: the small scenes' composites are a few hundred gaussians on a few thousand
    pixels each, less work than handing it to a thread team costs (17 s against 0.04 s per scene late in a whole-suite run)."""
    def __getattr__(self, name):
        from oracle import cpu_oracle as orc

        return getattr(orc, name)

    @staticmethod
    def max_threads():
        return 1


@pytest.fixture(scope="module")
def G():
    return namespace(OneThreadOracle())


def _ids(c, name):
    """Every gaussian on the small scenes, the gradient tests' seeded sample on the others (file order)."""
    return np.arange(c["R"].scene.n) if name in SMALL else _sample(c, name)


def _maps(c, ids, opts=None, cam=None):
    """The feature blend's own weight maps [len(ids), H, W] (float32, on the GPU, in the layout `opts` asks for) of the gaussians
    `ids` (file order): one-hot columns through render_features, PER_WALK per walk."""
    R, cam = c["R"], cam or c["cam"]
    out = []
    for k0 in range(0, len(ids), PER_WALK):
        part = ids[k0:k0 + PER_WALK]
        F = torch.zeros((R.scene.n, PER_WALK), dtype=torch.float32, device="cuda")
        F[torch.from_numpy(part).cuda(), torch.arange(len(part), device="cuda")] = 1.0
        m = R.render_features(cam, F, opts)
        out.append(m.permute(2, 0, 1)[:len(part)].contiguous())
    return torch.cat(out, 0)


def _ref(c, name):
    """(ids, maps) under the default options: computed once per scene and only read."""
    if "gstats_ref" not in c:
        ids = _ids(c, name)
        c["gstats_ref"] = (ids, _maps(c, ids))
    return c["gstats_ref"]


def _agrees(tag, st, ids, maps, scale=1.0):
    """view_stats' result `st` (file order) against weight maps [len(ids), H, W]: max and pixels exact, the sum at the bar."""
    at = torch.from_numpy(ids).cuda()
    flat = maps.reshape(len(ids), -1)
    if st.weight_max is not None:
        assert torch.equal(st.weight_max[at], flat.max(1).values), tag
    if st.pixels is not None:
        assert st.pixels.dtype == torch.int32
        assert torch.equal(st.pixels[at].long(), (flat > 0).sum(1) * int(scale)), tag
    if st.weight_sum is not None:
        ref = flat.double().sum(1).cpu().numpy() * scale
        if ref.max() > 0:
            _bar(tag, st.weight_sum[at].cpu().numpy(), ref)
        else:
            assert not st.weight_sum[at].any(), tag


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL + SAMPLED)
def test_exact_against_the_feature_blends_own_weights(G, name):
    c = _case(G, name)
    R, cam = c["R"], c["cam"]
    ids, maps = _ref(c, name)
    st = R.view_stats(cam)
    stats = dict(R.last_stats)
    n = R.scene.n
    for t, dt in zip(st, (torch.float32, torch.float32, torch.int32)):
        assert t.shape == (n,) and t.dtype == dt and t.is_cuda
    reached = (maps.reshape(len(ids), -1) > 0).any(1)
    print(f"\n{name}: {int(reached.sum())} of {len(ids)} gaussians reach a pixel; stats {stats}", end="")
    assert int(reached.sum()) >= (8 if name in SMALL else 48), name
    _agrees(name, st, ids, maps)
    never = torch.from_numpy(ids).cuda()[~reached]
    assert len(never) > 0, name  # gaussians with an all-zero map: exactly 0 in all three
    assert not st.weight_sum[never].any() and not st.weight_max[never].any() and not st.pixels[never].any(), name
    assert stats["wave_entries"] > 0 and stats["colour_evals"] == 0
    if name == "wall":  # every quadrant stops early, and lists run past one batch of 256 entries
        assert stats["fetched_entries"] < stats["n_pairs"]
    assert torch.equal(R.visible_ids(cam), torch.nonzero(st.pixels > 0)[:, 0])


# ---- 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_against_the_oracle(G, name):
    c = _case(G, name)
    R, cam = c["R"], c["cam"]
    ids = np.arange(R.scene.n)
    w = _weight_maps(G, c, ids, False).reshape(len(ids), -1)
    st = R.view_stats(cam, want=("sum", "max"))
    assert st.pixels is None
    assert (w.max(1) > 0).sum() >= 8, name
    _bar(f"{name} max", st.weight_max.cpu().numpy(), w.max(1))
    _bar(f"{name} sum", st.weight_sum.cpu().numpy(), w.astype(np.float64).sum(1))


# ---- 3 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL + SAMPLED)
def test_identities_with_the_pick_maps(G, name):
    c = _case(G, name)
    R, cam = c["R"], c["cam"]
    st = R.view_stats(cam, want=("max", "pixels"))
    stats = dict(R.last_stats)
    pk = R.render_pick(cam, count=True)
    assert int(st.pixels.long().sum()) == int(pk.count.long().sum()) > 0
    has = pk.best_id >= 0
    assert bool(has.any())
    assert bool((st.weight_max[pk.best_id[has].long()] >= pk.best_w[has]).all())
    assert torch.equal(st.weight_max.max(), pk.best_w.max())
    if name == "wall":
        assert stats["fetched_entries"] < stats["n_pairs"]


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def _second_camera(G, name):
    _, args = _build(G, name)
    tvec = np.asarray(args[1], np.float64) + np.array([0.15, -0.05, 0.1])
    return G.renderer.make_camera(args[0], tvec, *args[2:])


@pytest.mark.parametrize("name", ["f3a", "medium"])
def test_accumulation_over_calls_and_views(G, name):
    c = _case(G, name)
    R, cam = c["R"], c["cam"]
    n, VS = R.scene.n, G.renderer.ViewStats
    one = R.view_stats(cam, scene_order=True)
    out = VS(torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"))
    for _ in range(2):
        got = R.view_stats(cam, out=out)
        assert all(a is b for a, b in zip(got, out))
    assert torch.equal(out.pixels, 2 * one.pixels) and torch.equal(out.weight_max, one.weight_max)
    _bar(f"{name} twice", out.weight_sum.cpu().numpy(), 2.0 * one.weight_sum.double().cpu().numpy())
    cam2 = _second_camera(G, name)
    two = R.view_stats(cam2, scene_order=True)
    assert not torch.equal(two.pixels, one.pixels)  # (another view)
    acc = VS(*[t.clone() for t in one])
    R.view_stats(cam2, out=acc)
    assert torch.equal(acc.weight_max, torch.maximum(one.weight_max, two.weight_max))
    assert torch.equal(acc.pixels, one.pixels + two.pixels)
    _bar(f"{name} two views", acc.weight_sum.cpu().numpy(), (one.weight_sum.double() + two.weight_sum.double()).cpu().numpy())
    total, views = G.renderer.accumulate_view_stats(R, [cam, cam2, cam])
    f1, f2 = R.view_stats(cam), R.view_stats(cam2)
    assert views.dtype == torch.int32 and views.shape == (n,)
    assert torch.equal(views, 2 * (f1.pixels > 0).int() + (f2.pixels > 0).int())
    assert torch.equal(total.pixels, 2 * f1.pixels + f2.pixels)
    assert torch.equal(total.weight_max, torch.maximum(f1.weight_max, f2.weight_max))
    _bar(f"{name} three views", total.weight_sum.cpu().numpy(), (2.0 * f1.weight_sum.double() + f2.weight_sum.double()).cpu().numpy())


# ---- 5 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f3a", "medium"])
def test_pixel_mask(G, name):
    c = _case(G, name)
    R, cam = c["R"], c["cam"]
    H, W, n = cam.height, cam.width, R.scene.n
    ids, maps = _ref(c, name)
    mk, VS = G.renderer.make_options, G.renderer.ViewStats
    full = R.view_stats(cam)
    full_stats = dict(R.last_stats)
    # about half the pixels, seeded; as bool and as uint8 (any non-zero byte counts)
    mask = torch.rand((H, W), generator=torch.Generator().manual_seed(41)) < 0.5
    mask = mask.cuda()
    st = R.view_stats(cam, mask=mask)
    _agrees(f"{name} random mask", st, ids, maps * mask)
    assert not torch.equal(st.pixels, full.pixels)
    st8 = R.view_stats(cam, mask=mask.to(torch.uint8) * 200, want=("max", "pixels"))
    assert torch.equal(st8.weight_max, st.weight_max) and torch.equal(st8.pixels, st.pixels)
    # the screen layout [W, H]: the mask is read transposed
    stT = R.view_stats(cam, mk(output_layout=1), mask=mask.t().contiguous(), want=("max", "pixels"))
    assert torch.equal(stT.weight_max, st.weight_max) and torch.equal(stT.pixels, st.pixels)
    # all ones: the unmasked call
    ones = R.view_stats(cam, mask=torch.ones((H, W), dtype=torch.bool, device="cuda"), want=("max", "pixels"))
    assert torch.equal(ones.weight_max, full.weight_max) and torch.equal(ones.pixels, full.pixels)
    # all zero: nothing is touched and nothing is evaluated
    out = VS(torch.full((n,), 7.0, device="cuda"), torch.full((n,), 3.0, device="cuda"), torch.full((n,), 5, dtype=torch.int32, device="cuda"))
    zero = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    R.view_stats(cam, mask=zero, out=out)
    assert bool((out.weight_sum == 7.0).all()) and bool((out.weight_max == 3.0).all()) and bool((out.pixels == 5).all())
    R.view_stats(cam, mask=zero)
    assert R.last_stats["wave_entries"] == 0 and R.last_stats["fetched_entries"] == 0
    # one 8x8 quadrant, the one in which the sampled gaussians put most weight
    heat = maps.sum(0)[:H // 8 * 8, :W // 8 * 8].reshape(H // 8, 8, W // 8, 8).sum((1, 3))
    qy, qx = divmod(int(heat.argmax()), W // 8)
    quad = torch.zeros((H, W), dtype=torch.bool, device="cuda")
    quad[qy * 8:qy * 8 + 8, qx * 8:qx * 8 + 8] = True
    sq = R.view_stats(cam, mask=quad)
    quad_stats = dict(R.last_stats)
    _agrees(f"{name} one quadrant", sq, ids, maps * quad)
    assert bool(sq.pixels.any()) and int(sq.pixels.max()) <= 64
    assert 0 < quad_stats["wave_entries"] < full_stats["wave_entries"]
    # the undrawn last column and row of reference_compat count for nothing, whatever the mask says
    edge = torch.zeros((H, W), dtype=torch.bool, device="cuda")
    edge[H - 1, :] = True
    edge[:, W - 1] = True
    se = R.view_stats(cam, mask=edge)
    assert not se.weight_sum.any() and not se.weight_max.any() and not se.pixels.any()
    if name == "medium":
        assert bool(R.view_stats(cam, mk(reference_compat=False), mask=edge, want=("pixels",)).pixels.any())


# ---- 6 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [1, 2])
def test_two_tile_row_shards_make_the_frame(G, block):
    c = _case(G, "medium")
    R, cam = c["R"], c["cam"]
    H, W, n = cam.height, cam.width, R.scene.n
    mk, VS = G.renderer.make_options, G.renderer.ViewStats
    mask = (torch.rand((H, W), generator=torch.Generator().manual_seed(43)) < 0.5).cuda()
    whole, whole_m = R.view_stats(cam, scene_order=True), R.view_stats(cam, mask=mask, scene_order=True)
    acc = VS(torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"))
    acc_m = VS(*[torch.zeros_like(t) for t in acc])
    for r in range(2):
        R.view_stats(cam, mk(tile_row_begin=r, tile_row_step=2, tile_row_block=block), out=acc)
        # the strip layout: the mask holds the shard's tile rows, ascending
        rows = G.renderer.shard_row_list(H, r, 2, block)
        strip = torch.zeros((16 * len(rows), W), dtype=torch.bool, device="cuda")
        for k, ty in enumerate(rows):
            h = min(16, H - ty * 16)
            strip[k * 16: k * 16 + h] = mask[ty * 16: ty * 16 + h]
        R.view_stats(cam, mk(tile_row_begin=r, tile_row_step=2, tile_row_block=block, output_layout=2), mask=strip, out=acc_m)
    for got, ref, tag in ((acc, whole, "shards"), (acc_m, whole_m, "masked strips")):
        assert torch.equal(got.weight_max, ref.weight_max) and torch.equal(got.pixels, ref.pixels), (tag, block)
        _bar(f"{tag} block {block}", got.weight_sum.cpu().numpy(), ref.weight_sum.double().cpu().numpy())


# ---- 7 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(early_out_T=1e-4), dict(reference_compat=False)], ids=["early_out_T", "no_compat"])
def test_options_are_the_forwards(G, kw):
    c = _case(G, "medium")
    R, cam = c["R"], c["cam"]
    ids, base = _ref(c, "medium")
    o = G.renderer.make_options(**kw)
    maps = _maps(c, ids, o)
    assert not torch.equal(maps, base)  # (the option took effect)
    _agrees(str(kw), R.view_stats(cam, o), ids, maps)


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_order_and_want(G):
    c = _case(G, "f2")
    R, cam = c["R"], c["cam"]
    o_t, n, VS = R.scene.order_t, R.scene.n, G.renderer.ViewStats
    assert o_t is not None  # the scene was reordered: file order and scene order differ
    base = R.view_stats(cam)
    so = R.view_stats(cam, scene_order=True)
    assert torch.equal(so.weight_max, base.weight_max.index_select(0, o_t)) and torch.equal(so.pixels, base.pixels.index_select(0, o_t))
    assert not torch.equal(so.pixels, base.pixels)
    out = VS(torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"))
    R.view_stats(cam, out=out)
    assert torch.equal(out.weight_max, so.weight_max) and torch.equal(out.pixels, so.pixels)  # `out` is in the scene's order
    _bar("out", out.weight_sum.cpu().numpy(), so.weight_sum.double().cpu().numpy())
    for want in (("sum",), ("max",), ("pixels",), ("sum", "max"), ("sum", "pixels"), ("pixels", "max")):
        st = R.view_stats(cam, want=want)
        assert [t is not None for t in st] == [k in want for k in ("sum", "max", "pixels")], want
        if st.weight_max is not None:
            assert torch.equal(st.weight_max, base.weight_max), want
        if st.pixels is not None:
            assert torch.equal(st.pixels, base.pixels), want
        if st.weight_sum is not None:
            _bar(f"want {want}", st.weight_sum.cpu().numpy(), base.weight_sum.double().cpu().numpy())
    # with `out`, the fields not wanted are neither needed nor touched
    keep = torch.full((n,), 9, dtype=torch.int32, device="cuda")
    got = R.view_stats(cam, out=VS(None, torch.zeros(n, device="cuda"), keep), want=("max",))
    assert got.weight_sum is None and got.pixels is None and torch.equal(got.weight_max, so.weight_max)
    assert bool((keep == 9).all())


# ---- 9 ------------------------------------------------------------------------------------------------------------------
def test_neighbours_on_the_workspace(G):
    """At the ABI: a gsr_blend after a statistics walk on one workspace renders the bits it renders alone, and gsr_read_stats
    afterwards describes the walk."""
    from gsr_amd._lib import check, lib

    c = _case(G, "medium")
    R, cam = c["R"], c["cam"]
    o = G.renderer.make_options(colour_stage=0)
    R.render(cam, o)  # sizes the pair buffers to the frame
    ws = R._workspace(cam.width, cam.height)
    sc, sp = R.scene.c_struct(), int(torch.cuda.current_stream().cuda_stream)
    n, wp, wn, mp = R.scene.n, ws.data_ptr(), ws.numel(), R.max_pairs

    def stages12():
        check(lib.gsr_preprocess(C.byref(sc), C.byref(cam), C.byref(o), wp, wn, None, sp))
        check(lib.gsr_bin_sort(n, C.byref(cam), C.byref(o), mp, wp, wn, sp))

    def blend():
        out = torch.empty((cam.height, cam.width, 3), dtype=torch.float32, device="cuda")
        check(lib.gsr_blend(C.byref(sc), n, C.byref(cam), C.byref(o), mp, wp, wn, out.data_ptr(), None, sp))
        return out

    stages12()
    alone = blend()
    stages12()
    s, m, p = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    check(lib.gsr_blend_gaussian_stats(n, C.byref(cam), C.byref(o), mp, wp, wn, None, s.data_ptr(), m.data_ptr(), p.data_ptr(), sp))
    st = R.stats()
    after = blend()
    m2 = torch.zeros(n, device="cuda")
    check(lib.gsr_blend_gaussian_stats(n, C.byref(cam), C.byref(o), mp, wp, wn, None, None, m2.data_ptr(), None, sp))
    again = blend()
    torch.cuda.synchronize()
    assert torch.equal(after, alone) and torch.equal(again, alone)
    assert st["colour_evals"] == 0 and st["wave_entries"] > 0 and st["fetched_entries"] > 0
    ref = R.view_stats(cam, scene_order=True)
    assert torch.equal(m, ref.weight_max) and torch.equal(m2, ref.weight_max) and torch.equal(p, ref.pixels)
    _bar("abi vs view_stats", s.cpu().numpy(), ref.weight_sum.double().cpu().numpy())


# ---- 10 -----------------------------------------------------------------------------------------------------------------
def test_degenerate_inputs(G):
    """n = 0, and a shard that owns no tile row."""
    p = G.synthetic.look_at_pose((0, -4, 0.5), (0, 0, 0), 1, "x.png")
    W, H = 5, 3
    fx = G.synthetic.pinhole_focal(W)
    cam = G.renderer.make_camera(p.qvec, p.tvec, 2 * fx, 2 * fx, 2 * W, 2 * H, W, H)
    cols = G.synthetic.mip360_like(300, 3)
    for i in range(3):
        cols[f"scale_{i}"] = (cols[f"scale_{i}"] + np.float32(3.0)).astype(np.float32)
    mk, VS = G.renderer.make_options, G.renderer.ViewStats
    for n in (0, 300):
        packed = G.utils.pack_gaussians({k: v[:n] for k, v in cols.items()})
        R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(packed))
        st = R.view_stats(cam)
        assert all(t.shape == (n,) for t in st) and R.visible_ids(cam).dtype == torch.int64
        if n:
            assert bool(st.pixels.any()) and int(st.pixels.max()) <= (W - 1) * (H - 1)
            w = R.blend_weights(cam)
            _bar("5x3 sum vs blend_weights", st.weight_sum.cpu().numpy(), w.double().cpu().numpy())
        # the frame has one tile row: the second of two shards owns none
        empty = mk(tile_row_begin=1, tile_row_step=2, output_layout=2)
        se = R.view_stats(cam, empty)
        assert all(t.shape == (n,) and not t.any() for t in se)
        out = VS(torch.full((n,), 2.0, device="cuda"), torch.full((n,), 1.0, device="cuda"), torch.full((n,), 4, dtype=torch.int32, device="cuda"))
        R.view_stats(cam, empty, out=out)
        assert bool((out.weight_sum == 2.0).all()) and bool((out.weight_max == 1.0).all()) and bool((out.pixels == 4).all())
        total, views = G.renderer.accumulate_view_stats(R, [])
        assert views.shape == (n,) and not views.any() and not total.pixels.any()
