"""GPU: pick maps (gsr_blend_pick / gsr_render_pick, Rasterizer.render_pick / render_median_depth / pick) — per pixel the gaussian
of largest weight, the one after which T first falls below median_T, and the contributor count.

References, none of them the code under test:
  - exact: the feature blend composites one-hot rows, so channel i of R.render_features(cam, eye(n)) IS w_i(p) = fma(w_i, 1, 0) plus
    exact zeros, and the same call with draw_limit = k gives the weights and the transmittance of every prefix of the draw order.
    best / count follow from the full maps, the median from the first prefix whose T is below the threshold, ties in the weight
    from the order the gaussians appear in the prefixes.  Everything is compared bit for bit, no pixel excluded;
  - independent of every GPU kernel: the CPU oracle's compositing loop over one-hot colours (weights) and its prefixes (T), with the
    project's standing 1e-4 bar on a transmittance or a weight.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_cases import (MEDIANS, NEVER, exact as _exact, feature_case as _case, namespace, oracle_maps as _oracle_maps,
                       pick_case as _pick_case, z_cam as _z_cam)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    return namespace()


def _assert_picks(tag, got, exp, median_T, count=True):
    assert got.best_id.dtype == torch.int32 and got.median_id.dtype == torch.int32 and got.best_w.dtype == torch.float32
    assert torch.equal(got.best_w, exp["best_w"]), tag
    assert torch.equal(got.best_id, exp["best_id"]), tag
    assert torch.equal(got.median_id, exp["median_id"][median_T]), tag
    if count:
        assert got.count.dtype == torch.int32 and torch.equal(got.count, exp["count"]), tag
    else:
        assert got.count is None, tag


def _assert_undrawn(got):
    """Q1: the last column and the last row hold -1, 0, -1, 0."""
    for sl in ((-1, slice(None)), (slice(None), -1)):
        assert bool((got.best_id[sl] == -1).all()) and not got.best_w[sl].any() and bool((got.median_id[sl] == -1).all())
        assert got.count is None or not got.count[sl].any()


# ---- 1: bit for bit against the feature blend's own weights -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f1", "f3a", "f3b"])
def test_picks_are_the_exact_weights_argmax_median_and_count(G, name):
    c = _case(G, name)
    R, cam = c["R"], c["cam"]
    exp = _exact(G, c, snapshots=(1, 7, 21, R.scene.n - 1) if name == "f1" else ())
    assert bool((exp["best_w"] > 0).any()) and bool((exp["median_id"][0.5] >= 0).any()) and int(exp["count"].max()) > 1
    for m in MEDIANS:
        for count in (True, False):
            got = R.render_pick(cam, median_T=m, count=count)
            _assert_picks((name, m, count), got, exp, m, count)
            _assert_undrawn(got)
    # median_T = 1: the first gaussian with w > 0 — of a pixel's contributors the one the prefixes show first
    appear = c["appear"]
    first = torch.where(appear > 0, appear, torch.full_like(appear, NEVER)).argmin(-1).to(torch.int32)
    first = torch.where(exp["count"] > 0, first, torch.full_like(first, -1))
    assert torch.equal(R.render_pick(cam, median_T=1.0).median_id, first)


def test_draw_limit_picks_match_the_exact_prefix(G):
    c = _case(G, "f1")
    R, cam = c["R"], c["cam"]
    ks = (1, 7, 21, R.scene.n - 1)
    _exact(G, c, snapshots=ks)
    for k in ks:
        for count in (True, False):
            got = R.render_pick(cam, G.renderer.make_options(draw_limit=k), count=count)
            _assert_picks(("f1 draw_limit", k, count), got, c["exact_at"][k], 0.5, count)


def test_a_deep_tile_reaches_the_later_batches_and_the_ring_refill(G):
    """More than 512 entries in one tile's list before the gaussians that decide some pixels: the second and third batch of 256 staged
    entries and the refill of the ring of filtered cell-list entries.  The precondition is read off the reference, not trusted to
    the construction."""
    c = _pick_case(G, "deep")
    R, cam = c["R"], c["cam"]
    assert R.scene.n <= 1024 and (cam.width, cam.height) == (40, 24)
    exp = _exact(G, c)
    W = c["W"]
    in_tile = (W[:16, :16] > 0).flatten(0, 1).any(0)  # gaussians with weight somewhere in tile (0, 0): all in its list
    assert int(in_tile.sum()) >= 600, int(in_tile.sum())
    best_rank, med_rank = int(exp["best_rank"][:16, :16].max()), int(exp["median_rank"][0.5][:16, :16].max())
    assert best_rank > 512 and med_rank > 512, (best_rank, med_rank)  # the deciding gaussian's rank in the prefix sweep
    # ... and within the tile's own list: more than 512 of the tile's contributors show up in the sweep before it
    appear = c["appear"]
    step = torch.where(appear > 0, appear, torch.full_like(appear, NEVER)).flatten(0, 1).min(0).values  # per gaussian: its prefix
    for r in (best_rank, med_rank):
        assert int((in_tile & (step < r)).sum()) > 512, r
    got = R.render_pick(cam, count=True)
    _assert_picks("deep count", got, exp, 0.5, True)
    _assert_picks("deep", R.render_pick(cam), exp, 0.5, False)
    for m in (0.9, 1.0):
        _assert_picks(("deep", m), R.render_pick(cam, median_T=m), exp, m, False)
    assert R.last_stats["fetched_entries"] > 512
    for kw in (dict(fine_binning=True), dict(no_footprint_cull=True)):  # per-tile lists: no ring; the reference's full rects: longer lists
        _assert_picks(("deep", kw), R.render_pick(cam, G.renderer.make_options(**kw), count=True), exp, 0.5, True)


def test_small_stacks_with_depth_ties(G):
    """tests/order_scenes.py: six gaussians per pixel block at chosen depth keys, exact depth ties among them (drawn in the scene's
    array order, by the pick as by the feature blend it is held against)."""
    c = _pick_case(G, "stacks")
    R, cam = c["R"], c["cam"]
    assert R.scene.n <= 1024
    exp = _exact(G, c)
    assert int(exp["count"].max()) >= 6
    for m in MEDIANS:
        _assert_picks(("stacks", m), R.render_pick(cam, median_T=m, count=True), exp, m, True)
        _assert_picks(("stacks", m), R.render_pick(cam, median_T=m), exp, m, False)


# ---- 2: against the CPU oracle, independent of every GPU kernel -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["f1", "f3a"])
def test_picks_against_the_cpu_oracle(G, name):
    """Measured on the MI355X: see the figures this prints (delta = max |W_gpu - W_oracle| of the one-hot feature maps)."""
    c = _case(G, name)
    R, cam = c["R"], c["cam"]
    _exact(G, c)
    n, H, W = R.scene.n, cam.height, cam.width
    _, _, n_drawn = _oracle_maps(G, c, np.zeros((n, 3), np.float32))  # (leaves the oracle's preprocess and depth order in c)

    def composite(feats, limit=-1):
        """_oracle_maps on one thread: hundreds of calls on a frame this small cost less than as many thread teams."""
        screen, trans, _ = G.orc.composite(c["order"], dict(c["pre"], rgb=feats), W, H, limit=limit, threads=1)
        return screen.transpose(1, 0, 2), trans.transpose(1, 0)

    Wo = np.zeros((H, W, n), np.float32)
    for i0 in range(0, n, 3):
        onehot = np.zeros((n, 3), np.float32)
        ids = np.arange(i0, min(i0 + 3, n))
        onehot[ids, np.arange(len(ids))] = 1.0
        Wo[..., ids] = composite(onehot)[0][..., :len(ids)]
    zeros = np.zeros((n, 3), np.float32)
    To = np.stack([composite(zeros, limit=k)[1] for k in range(n_drawn + 1)])  # [k][H,W]
    # the oracle's draw order: the depth order restricted to what its skip guard lets through = the gaussians it gives weight, in order
    pre, order = c["pre"], c["order"]
    bb, sg = pre["pixel_bboxes"], pre["sigmas"]
    passes = ((bb[:, 2] - bb[:, 0]) * (bb[:, 3] - bb[:, 1]) != 0) & (sg != 0).all(1)
    drawn_order = order[passes[order]]
    assert len(drawn_order) == n_drawn
    step_of = np.zeros(n, np.int64)  # gaussian -> k: composite(limit = k) is the first prefix that holds it
    step_of[drawn_order] = np.arange(1, n_drawn + 1)

    delta = float(np.abs(c["W"].cpu().numpy() - Wo).max())
    wo_max = Wo.max(-1)
    drawn_px = np.zeros((H, W), bool)
    drawn_px[:H - 1, :W - 1] = True
    worst = dict(best_id=0.0, best_w=0.0, before=0.0, after=0.0)
    results = []
    for m in MEDIANS:
        got = R.render_pick(cam, median_T=m)
        bid, bw, mid = got.best_id.cpu().numpy(), got.best_w.cpu().numpy(), got.median_id.cpu().numpy()
        w_at = np.where(bid >= 0, np.take_along_axis(Wo, np.maximum(bid, 0)[..., None], -1)[..., 0], 0.0)
        k = np.where(mid >= 0, step_of[np.maximum(mid, 0)], 0)
        assert (k[mid >= 0] >= 1).all()  # the picked gaussian is one the oracle draws
        yy, xx = np.mgrid[:H, :W]
        before = np.where(mid >= 0, To[np.maximum(k - 1, 0), yy, xx], To[n_drawn])  # no median: the final T is still >= median_T
        after = np.where(mid >= 0, To[k, yy, xx], 0.0)
        worst["best_id"] = max(worst["best_id"], float((wo_max - w_at)[drawn_px].max()))
        worst["best_w"] = max(worst["best_w"], float(np.abs(bw - wo_max)[drawn_px].max()))
        worst["before"] = max(worst["before"], float((m - before)[drawn_px].max()))
        worst["after"] = max(worst["after"], float((after - m)[drawn_px].max()))
        results.append((m, w_at, bw, before, after))
    print(f"\n{name}: delta = max |W_gpu - W_oracle| {delta:.3e}; worst max_i Wo - Wo[best_id] {worst['best_id']:.3e}, |best_w - max_i Wo| "
          f"{worst['best_w']:.3e}, median_T - T_before {worst['before']:.3e}, T_after - median_T {worst['after']:.3e}")
    assert delta <= 1e-4, delta
    for m, w_at, bw, before, after in results:
        assert (w_at >= wo_max - 2 * delta)[drawn_px].all(), (name, m)
        assert (np.abs(bw - wo_max) <= delta)[drawn_px].all(), (name, m)
        assert (before >= m - 1e-4)[drawn_px].all() and (after <= m + 1e-4)[drawn_px].all(), (name, m)


# ---- 3: the early stop is exact -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f2", "f5", "medium"])
def test_the_stop_rule_changes_no_bit(G, name):
    c = _case(G, name)
    R, cam, mk = c["R"], c["cam"], G.renderer.make_options
    R.render_features(cam, c["Ft"])
    st_feat = dict(R.last_stats)
    with_count = R.render_pick(cam, count=True)
    st_count = dict(R.last_stats)
    without = R.render_pick(cam)
    st_plain = dict(R.last_stats)
    every = R.render_pick(cam, mk(early_out_T=-1.0), count=True)  # blends every entry
    st_every = dict(R.last_stats)
    print(f"\n{name}: wave_entries / fetched_entries  feature blend {st_feat['wave_entries']} / {st_feat['fetched_entries']}, pick with count "
          f"{st_count['wave_entries']} / {st_count['fetched_entries']}, pick {st_plain['wave_entries']} / {st_plain['fetched_entries']}, "
          f"every entry {st_every['wave_entries']} / {st_every['fetched_entries']} of n_pairs {st_every['n_pairs']}")
    for other in (without, every):
        assert torch.equal(other.best_id, with_count.best_id) and torch.equal(other.best_w, with_count.best_w)
        assert torch.equal(other.median_id, with_count.median_id)
    assert torch.equal(every.count, with_count.count) and without.count is None
    assert bool((with_count.best_id >= 0).any()) and bool((with_count.median_id >= 0).any())
    assert st_plain["wave_entries"] <= st_count["wave_entries"] and st_plain["fetched_entries"] <= st_count["fetched_entries"]
    assert st_count["wave_entries"] == st_feat["wave_entries"] and st_count["fetched_entries"] == st_feat["fetched_entries"]
    assert st_count["wave_entries"] <= st_every["wave_entries"] and st_count["fetched_entries"] <= st_every["fetched_entries"] <= st_every["n_pairs"]
    assert st_count["colour_evals"] == 0 and st_plain["colour_evals"] == 0


# ---- 4: options ---------------------------------------------------------------------------------------------------------------
def _same(a, b, count=True):
    return (torch.equal(a.best_id, b.best_id) and torch.equal(a.best_w, b.best_w) and torch.equal(a.median_id, b.median_id)
            and (not count or torch.equal(a.count, b.count)))


def test_every_path_builds_the_default_picks(G):
    c = _case(G, "f2")
    R, cam, mk = c["R"], c["cam"], G.renderer.make_options
    base = R.render_pick(cam, count=True)
    H, W = cam.height, cam.width
    assert base.best_id.shape == (H, W) and bool((base.best_id >= 0).any())
    for kw in (dict(fine_binning=True), dict(no_footprint_cull=True), dict(depth_sort_passes=4),
               dict(saturation_rule=1, blend_impl=1, blend_pipe_tiles=-1, no_order_hint=True, colour_stage=1)):  # (the last: ignored options)
        assert _same(R.render_pick(cam, mk(**kw), count=True), base), kw
        assert _same(R.render_pick(cam, mk(**kw)), base, count=False), kw
    full = R.render_pick(cam, mk(reference_compat=False), count=True)
    for a, b in zip(full, base):
        assert torch.equal(a[:-1, :-1], b[:-1, :-1])
    assert bool((full.best_id[-1] >= 0).any()) or bool((full.best_id[:, -1] >= 0).any())
    s = R.render_pick(cam, mk(output_layout=1), count=True)
    assert s.best_id.shape == (W, H) and all(torch.equal(a, b.t()) for a, b in zip(s, base))
    for count in (True, False):
        for step in (2, 3):
            for block in (1, 2):
                out = [torch.full((H, W), -7, dtype=t.dtype, device=t.device) for t in base[:3 + count]]
                for r in range(step):
                    strip = R.render_pick(cam, mk(tile_row_begin=r, tile_row_step=step, output_layout=2, tile_row_block=block), count=count)
                    rows = G.renderer.shard_row_list(H, r, step, block)
                    assert strip.best_id.shape == (16 * len(rows), W)
                    for k, ty in enumerate(rows):
                        h = min(16, H - ty * 16)
                        for o, s_ in zip(out, strip):
                            o[ty * 16: ty * 16 + h] = s_[k * 16: k * 16 + h]
                assert all(torch.equal(o, b) for o, b in zip(out, base)), (count, step, block)


# ---- 5: neighbours on the workspace -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour_stage", [0, 1])
def test_a_colour_blend_next_to_a_pick_renders_its_own_bits(G, colour_stage):
    """At the ABI: gsr_blend before and after gsr_blend_pick on one workspace gives the bits of a gsr_blend alone — the pick neither
    evaluates nor disturbs a record's colour — and the picks do not depend on what ran before them."""
    from gsr_amd._lib import check, lib

    c = _case(G, "f2")
    R, cam = c["R"], c["cam"]
    H, W, n, dev = cam.height, cam.width, R.scene.n, R.scene.device
    sc, o = R.scene.c_struct(), G.renderer.make_options(colour_stage=colour_stage)
    whole = R.render(cam, o)  # (also sizes the pair buffers to the frame)
    expected = R.render_pick(cam, o, count=True, scene_order=True)
    ws = R._workspace(W, H)
    sp = int(torch.cuda.current_stream().cuda_stream)
    wp, wn, mp = ws.data_ptr(), ws.numel(), R.max_pairs

    def stages12():
        check(lib.gsr_preprocess(C.byref(sc), C.byref(cam), C.byref(o), wp, wn, None, sp))
        check(lib.gsr_bin_sort(n, C.byref(cam), C.byref(o), mp, wp, wn, sp))

    def blend():
        out = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        check(lib.gsr_blend(C.byref(sc), n, C.byref(cam), C.byref(o), mp, wp, wn, out.data_ptr(), None, sp))
        return out

    def pick(count):
        bi, mi, ct = (torch.full((H, W), -5, dtype=torch.int32, device=dev) for _ in range(3))
        bw = torch.full((H, W), -5.0, dtype=torch.float32, device=dev)
        check(lib.gsr_blend_pick(n, C.byref(cam), C.byref(o), mp, wp, wn, 0.5, bi.data_ptr(), bw.data_ptr(), mi.data_ptr(),
                                 ct.data_ptr() if count else None, sp))
        return G.renderer.PickMaps(bi, bw, mi, ct)

    stages12()
    alone = blend()
    stages12()
    p1 = pick(True)
    st_pick = R.stats()
    after = blend()
    p2 = pick(False)
    again = blend()
    p3 = pick(True)
    # any output alone
    only = torch.full((H, W), -5, dtype=torch.int32, device=dev)
    check(lib.gsr_blend_pick(n, C.byref(cam), C.byref(o), mp, wp, wn, 0.5, None, None, only.data_ptr(), None, sp))
    torch.cuda.synchronize()
    assert torch.equal(after, alone) and torch.equal(again, alone) and torch.equal(alone, whole)
    assert _same(p1, expected) and _same(p3, expected) and _same(p2, expected, count=False) and torch.equal(only, expected.median_id)
    assert bool((p2.count == -5).all())  # not asked for: not written
    assert st_pick["colour_evals"] == 0 and st_pick["wave_entries"] > 0


def test_a_multi_view_rasterizer_picks_through_the_single_view_path(G):
    c = _case(G, "f2")
    R2 = G.renderer.Rasterizer(c["R"].scene, views=2)
    assert _same(R2.render_pick(c["cam"], count=True), c["R"].render_pick(c["cam"], count=True))


# ---- 6: the Python surface ------------------------------------------------------------------------------------------------------
def test_ids_come_back_in_file_order(G):
    """The deep tile's 1000 depths are distinct, so the scene's storage order decides nothing: the Morton-ordered scene returns, mapped
    through its permutation, the ids of the scene kept in file order."""
    c = _pick_case(G, "deep")
    R, cam = c["R"], c["cam"]
    plain = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(c["packed"], spatial_order=False))
    assert plain.scene.order is None and R.scene.order is not None and not np.array_equal(R.scene.order, np.arange(R.scene.n))
    a, b = plain.render_pick(cam, count=True), R.render_pick(cam, count=True)
    assert _same(a, b) and bool((a.best_id >= 0).any())
    raw = R.render_pick(cam, count=True, scene_order=True)
    assert not torch.equal(raw.best_id, b.best_id)
    assert torch.equal(G.renderer.file_order_ids(raw.best_id, R.scene.order_t), b.best_id)
    assert torch.equal(G.renderer.file_order_ids(raw.median_id, R.scene.order_t), b.median_id)
    assert _same(plain.render_pick(cam, count=True, scene_order=True), a)
    with pytest.raises(ValueError):
        R.render_pick(cam, median_T=0.0)
    with pytest.raises(ValueError):
        R.render_pick(cam, median_T=float("nan"))


@pytest.mark.parametrize("name", ["f2", "deep"])
def test_median_depth_and_single_pixel_picks(G, name):
    c = _pick_case(G, name)
    R, cam = c["R"], c["cam"]
    z = torch.from_numpy(_z_cam(G, cam, c["packed"]["means"])).cuda()
    for m in (0.5, 0.9):
        ids = R.render_pick(cam, median_T=m).median_id
        d = R.render_median_depth(cam, median_T=m)
        assert d.shape == (cam.height, cam.width) and d.dtype == torch.float32
        assert torch.equal(d, torch.where(ids >= 0, z[ids.clamp(min=0).long()], torch.zeros_like(d)))
        assert bool((d > 0).any()) and not d[-1].any() and not d[:, -1].any()
    maps = R.render_pick(cam)
    ys, xs = torch.nonzero(maps.best_id >= 0, as_tuple=True)
    for x, y in [(int(xs[0]), int(ys[0])), (int(xs[-1]), int(ys[-1])), (cam.width - 1, cam.height - 1), (0, 0)]:
        got = R.pick(cam, x, y)
        assert got == (int(maps.best_id[y, x]), int(maps.median_id[y, x])) and all(isinstance(v, int) for v in got)
    assert R.pick(cam, cam.width - 1, cam.height - 1) == (-1, -1)  # Q1: never drawn
    with pytest.raises(ValueError):
        R.pick(cam, cam.width, 0)


# ---- 7: degenerate inputs -------------------------------------------------------------------------------------------------------
def test_degenerate_inputs(G):
    """n = 0, a frame smaller than a tile, everything culled: nothing is picked anywhere."""
    p = G.synthetic.look_at_pose((0, -4, 0.5), (0, 0, 0), 1, "x.png")

    def nothing(got, shape):
        assert got.best_id.shape == shape and bool((got.best_id == -1).all()) and bool((got.median_id == -1).all())
        assert not got.best_w.any() and not got.count.any()

    for (W, H) in ((5, 3), (33, 17)):
        fx = G.synthetic.pinhole_focal(W)
        cam = G.renderer.make_camera(p.qvec, p.tvec, 2 * fx, 2 * fx, 2 * W, 2 * H, W, H)
        cols = G.synthetic.mip360_like(300, 3)
        for i in range(3):
            cols[f"scale_{i}"] = (cols[f"scale_{i}"] + np.float32(3.0)).astype(np.float32)
        empty = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(G.utils.pack_gaussians({k: v[:0] for k, v in cols.items()})))
        nothing(empty.render_pick(cam, count=True), (H, W))
        assert not empty.render_median_depth(cam).any() and empty.pick(cam, 1, 1) == (-1, -1)
        # the same frame with something in it: held to the feature blend's weights
        R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(G.utils.pack_gaussians(cols)))
        Wm = R.render_features(cam, torch.eye(300, device="cuda"))
        got = R.render_pick(cam, count=True)
        assert got.best_id.shape == (H, W) and bool((got.best_id >= 0).any())
        assert torch.equal(got.best_w, Wm.max(-1).values) and torch.equal(got.count, (Wm > 0).sum(-1).to(torch.int32))
        hit = got.best_id >= 0
        assert torch.equal(hit, got.best_w > 0)
        assert torch.equal(Wm.gather(-1, got.best_id.clamp(min=0).long()[..., None])[..., 0][hit], got.best_w[hit])
        _assert_undrawn(got)
        # every gaussian behind the camera (it sits at y = -4 and looks along +y)
        far = dict(cols)
        far["y"] = (far["y"] - np.float32(100.0)).astype(np.float32)
        R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(far))
        nothing(R.render_pick(cam, count=True), (H, W))
        assert R.last_stats["n_visible"] == 0 and R.last_stats["wave_entries"] == 0
        assert not R.render_median_depth(cam).any()
