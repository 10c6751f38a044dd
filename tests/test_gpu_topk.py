"""GPU: top-k contributor lists (gsr_blend_topk / gsr_render_topk, Rasterizer.render_topk) — per pixel the k heaviest or the k
nearest gaussians with w > 0, ids and weights.

References, none of them the code under test:
  - exact: channel i of R.render_features(cam, eye(n)) IS w_i(p), bit for bit (the argument of tests/test_gpu_pick.py's docstring),
    and the draw order of a pixel's contributors is the order they appear in the prefix sweep (gpu_cases.exact -> c["appear"]: the
    value is the gaussian's position in the frame's draw order, the same at every pixel it has weight in).  The deep scene's draw
    order is its construction's: depth rank = `rank`, all depths distinct.  Expected HEAVIEST = the contributors sorted by
    (-w, appearance), first k; NEAREST = sorted by appearance, first k; both padded with -1 / 0.  Bit for bit, no pixel excluded;
  - independent of every GPU kernel: the CPU oracle's compositing loop over one-hot colours, with the project's standing 1e-4 bar on
    a weight.
"""
import numpy as np
import pytest
import torch

from gpu_cases import (NEVER, custom_case as _custom_case, exact as _exact, feature_case as _case, namespace, oracle_maps as _oracle_maps,
                       pick_case as _pick_case, wall_scene as _wall_scene)

pytestmark = pytest.mark.gpu

SELECTS = ("heaviest", "nearest")


@pytest.fixture(scope="module")
def G():
    return namespace()


# ---- the exact reference --------------------------------------------------------------------------------------------------------
def _steps(appear):
    """[n] the position of every gaussian in the frame's draw order, read off the prefix sweep (0: it has weight nowhere)."""
    return appear.flatten(0, 1).max(0).values


def _expected(W, step, k, select):
    """(ids [H,W,k] int32, weights [H,W,k]) of the weights W [H,W,n] under the draw order step [n] (any positive ints; only their
    order matters).  Two stable sorts: by appearance, then (HEAVIEST) by weight, descending — equal weights stay in draw order."""
    key = torch.where(W > 0, step.to(torch.int64).expand_as(W), torch.full((), 2 * NEVER, dtype=torch.int64, device=W.device))
    by_step = key.sort(dim=-1, stable=True).indices
    w = W.gather(-1, by_step)
    ids = by_step
    if select == "heaviest":
        w, by_w = w.sort(dim=-1, descending=True, stable=True)
        ids = by_step.gather(-1, by_w)
    w, ids = w[..., :k].contiguous(), ids[..., :k].to(torch.int32)
    return torch.where(w > 0, ids, torch.full_like(ids, -1)).contiguous(), w


def _assert_lists(tag, got, exp, k):
    ids, w = exp
    assert got.ids.dtype == torch.int32 and got.weights.dtype == torch.float32, tag
    assert got.ids.shape == ids.shape and got.weights.shape == w.shape and got.ids.shape[-1] == k, tag
    assert got.ids.is_contiguous() and got.weights.is_contiguous(), tag
    assert torch.equal(got.weights, w), tag
    assert torch.equal(got.ids, ids), tag


def _assert_undrawn(got):
    """Q1: the last column and the last row hold -1 / 0 in every slot (and T = 1)."""
    for sl in ((-1, slice(None)), (slice(None), -1)):
        assert bool((got.ids[sl] == -1).all()) and not got.weights[sl].any()
        assert got.final_T is None or bool((got.final_T[sl] == 1).all())


# ---- 1: bit for bit against the feature blend's own weights -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f1", "f3a", "f3b"])
def test_lists_are_the_exact_weights_top_k(G, name):
    c = _case(G, name)
    R, cam = c["R"], c["cam"]
    full = _exact(G, c)
    W, step = c["W"], _steps(c["appear"])
    count = full["count"]
    drawn = torch.zeros_like(count, dtype=torch.bool)
    drawn[:-1, :-1] = True
    # on the reference alone: padding and overflow are both exercised — some drawn pixel has fewer contributors than slots, some
    # more than the slots can hold (the CPU oracle's per-pixel maximum: 9 on f1, 26 on f3a, 21 on f3b)
    assert bool((count[drawn] < 4).any()), name
    assert int(count.max()) > (8 if name == "f1" else 16), (name, int(count.max()))
    assert bool((step[(W > 0).flatten(0, 1).any(0)] > 0).all())
    for k in (1, 2, 4, 5, 8, 16):
        assert k < 4 or bool((count[drawn] < k).any()), (name, k)  # some pixel pads
        for select in SELECTS:
            exp = _expected(W, step, k, select)
            for return_T in (False, True):
                got = R.render_topk(cam, k, select=select, return_T=return_T)
                _assert_lists((name, k, select, return_T), got, exp, k)
                _assert_undrawn(got)
                assert (got.final_T is None) != return_T
                if return_T:
                    assert torch.equal(got.final_T, c["T"]), (name, k, select)


# ---- 2: against the existing kernels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f1", "f3a", "f3b", "deep", "stacks"])
def test_k_1_is_the_pick_maps(G, name):
    c = _pick_case(G, name)
    R, cam = c["R"], c["cam"]
    pick = R.render_pick(cam)
    first = R.render_pick(cam, median_T=1.0).median_id
    assert bool((pick.best_id >= 0).any())
    for return_T in (False, True):
        h = R.render_topk(cam, 1, select="heaviest", return_T=return_T)
        assert torch.equal(h.ids[..., 0], pick.best_id) and torch.equal(h.weights[..., 0], pick.best_w), (name, return_T)
        n_ = R.render_topk(cam, 1, select="nearest", return_T=return_T)
        assert torch.equal(n_.ids[..., 0], first), (name, return_T)


# ---- 3: lists deeper than a batch ---------------------------------------------------------------------------------------------
def test_a_deep_tile_displaces_full_lists_in_the_later_batches(G):
    """tests/test_gpu_pick.py's deep tile: ~900 faint gaussians over one quadrant and five strong ones at depth ranks >= 560.  The
    lists have long been full when the strong ones arrive and must take them; a HEAVIEST stop must not fire while they are ahead."""
    c = _pick_case(G, "deep")
    R, cam = c["R"], c["cam"]
    n, dev = R.scene.n, R.scene.device
    assert n == 1000 and (cam.width, cam.height) == (40, 24)
    rank = torch.from_numpy(np.random.default_rng(17).permutation(n)).to(dev)  # deep_tile_scene's first draw: depth rank, file order
    if "W" not in c:
        c["W"], c["T"] = R.render_features(cam, torch.eye(n, dtype=torch.float32, device=dev), return_T=True)
    W, step = c["W"], rank + 1
    R.render_features(cam, torch.ones((n, 3), dtype=torch.float32, device=dev))  # the feature blend's own walk of these lists
    st_feat = dict(R.last_stats)
    # on the reference: some pixel's HEAVIEST list holds a gaussian of rank >= 560 that more than 256 of its tile's contributors
    # precede in the draw order (the tile's list holds them all: its second batch at the earliest)
    in_tile = (W[:16, :16] > 0).flatten(0, 1).any(0)
    ids16, _ = _expected(W, step, 16, "heaviest")
    late = ids16[:16, :16][ids16[:16, :16] >= 0].long().unique()
    late = late[rank[late] >= 560]
    assert late.numel() > 0
    assert max(int((in_tile & (rank < rank[i])).sum()) for i in late) > 256
    assert int((W > 0).sum(-1).max()) > 16  # and more contributors than slots
    stats = {}
    for k in (4, 8, 16):
        for select in SELECTS:
            exp = _expected(W, step, k, select)
            _assert_lists(("deep", k, select), R.render_topk(cam, k, select=select), exp, k)
            stats[k, select] = dict(R.last_stats)
            got = R.render_topk(cam, k, select=select, return_T=True)
            _assert_lists(("deep T", k, select), got, exp, k)
            assert torch.equal(got.final_T, c["T"])
            for key in ("wave_entries", "fetched_entries"):
                assert R.last_stats[key] == st_feat[key], (k, select, key)          # with T: the feature blend's walk
                assert stats[k, select][key] <= st_feat[key], (k, select, key)      # without: no longer
            assert R.last_stats["colour_evals"] == 0
    print(f"\ndeep: wave_entries / fetched_entries  feature blend {st_feat['wave_entries']} / {st_feat['fetched_entries']}; " + "; ".join(
        f"{s} k={k} {v['wave_entries']} / {v['fetched_entries']}" for (k, s), v in stats.items()))
    assert stats[4, "nearest"]["wave_entries"] <= stats[4, "heaviest"]["wave_entries"] <= st_feat["wave_entries"]
    assert st_feat["fetched_entries"] > 512
    # early_out_T > 0 where it cuts: the lists are the top k of the weights the feature blend composites at that threshold, with or
    # without the final T (a quadrant below the threshold is fed for exactly as long as the feature blend feeds it)
    # (the strong gaussian of rank 560 takes every pixel of its quadrant below 0.99 with hundreds of entries still ahead)
    eye = torch.eye(R.scene.n, dtype=torch.float32, device=R.scene.device)
    cut = []
    for e in (0.99, 0.9, 0.5):
        o = G.renderer.make_options(early_out_T=e)
        We, Te = R.render_features(cam, eye, o, return_T=True)
        cut.append(not torch.equal(We, W))
        for k in (4, 8):
            for select in SELECTS:
                exp = _expected(We, step, k, select)
                for return_T in (False, True):
                    got = R.render_topk(cam, k, o, select=select, return_T=return_T)
                    _assert_lists(("deep early", e, k, select, return_T), got, exp, k)
                    assert not return_T or torch.equal(got.final_T, Te)
    print(f"\ndeep: early_out_T 0.99 / 0.9 / 0.5 changes the feature blend's weights: {cut}")
    assert all(cut)


# ---- 3b: the HEAVIEST stop fires, and changes no bit -----------------------------------------------------------------------------
def test_the_heaviest_stop_fires_behind_an_opaque_wall_and_changes_no_bit(G):
    packed, args, rank = _wall_scene()
    c = _custom_case(G, "topk_wall", packed, args)
    R, cam = c["R"], c["cam"]
    n, dev = R.scene.n, R.scene.device
    rank = torch.from_numpy(rank).to(dev)
    W, T = R.render_features(cam, torch.eye(n, dtype=torch.float32, device=dev), return_T=True)
    R.render_features(cam, torch.ones((n, 3), dtype=torch.float32, device=dev))
    st_feat = dict(R.last_stats)
    step = rank + 1
    # on the reference: behind the six front gaussians every drawn pixel's transmittance is below its fourth and its eighth largest
    # weight (so the stop must fire for k = 4 and may not for k = 8: two of the eight come from behind the wall), each tile's list
    # is longer than two 64-entry chunks, and the feature blend walks on: T ends above zero everywhere
    drawn = torch.zeros(W.shape[:2], dtype=torch.bool, device=dev)
    drawn[:-1, :-1] = True
    T6 = 1.0 - W[..., rank < 6].double().sum(-1)
    w4 = W.sort(dim=-1, descending=True).values[..., 3].double()
    assert bool((T6[drawn] < 0.5 * w4[drawn]).all()), (float(T6[drawn].max()), float(w4[drawn].min()))
    assert bool((T[drawn] > 0).all())
    for tx in (0, 1):
        assert int((W[:, 16 * tx: 16 * tx + 16] > 0).flatten(0, 1).any(0).sum()) > 128
    stats = {}
    for k in (4, 8):
        for select in SELECTS:
            exp = _expected(W, step, k, select)
            _assert_lists(("wall", k, select), R.render_topk(cam, k, select=select), exp, k)
            stats[k, select] = dict(R.last_stats)
            got = R.render_topk(cam, k, select=select, return_T=True)
            _assert_lists(("wall T", k, select), got, exp, k)
            assert torch.equal(got.final_T, T)
            assert R.last_stats["wave_entries"] == st_feat["wave_entries"] and R.last_stats["fetched_entries"] == st_feat["fetched_entries"]
    print(f"\nwall: wave_entries / fetched_entries  feature blend {st_feat['wave_entries']} / {st_feat['fetched_entries']}; " + "; ".join(
        f"{s} k={k} {v['wave_entries']} / {v['fetched_entries']}" for (k, s), v in stats.items()))
    assert stats[4, "heaviest"]["wave_entries"] < st_feat["wave_entries"]  # strictly: the stop fired, and the lists above are exact
    assert stats[4, "nearest"]["wave_entries"] <= stats[4, "heaviest"]["wave_entries"]
    assert stats[8, "heaviest"]["wave_entries"] <= st_feat["wave_entries"]


# ---- 4: depth ties ------------------------------------------------------------------------------------------------------------
def test_small_stacks_with_depth_ties(G):
    """tests/order_scenes.py: six gaussians per pixel block at chosen depth keys, exact depth ties among them; the draw order is
    pinned ulp by ulp there, so a swapped NEAREST slot shows."""
    c = _pick_case(G, "stacks")
    R, cam = c["R"], c["cam"]
    full = _exact(G, c)
    assert int(full["count"].max()) >= 6
    W, step = c["W"], _steps(c["appear"])
    for k in (4, 8):
        for select in SELECTS:
            exp = _expected(W, step, k, select)
            for return_T in (False, True):
                _assert_lists(("stacks", k, select, return_T), R.render_topk(cam, k, select=select, return_T=return_T), exp, k)


# ---- 5: options ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 8])  # dword stores / 16-byte stores
def test_layouts_shards_and_list_options(G, k):
    c = _case(G, "f3a")
    R, cam, mk = c["R"], c["cam"], G.renderer.make_options
    _exact(G, c)
    H, Wd = cam.height, cam.width
    step = _steps(c["appear"])
    for select in SELECTS:
        base = R.render_topk(cam, k, select=select, return_T=True)
        _assert_lists(("f3a", k, select), base, _expected(c["W"], step, k, select), k)
        s = R.render_topk(cam, k, mk(output_layout=1), select=select, return_T=True)
        assert s.ids.shape == (Wd, H, k) and s.final_T.shape == (Wd, H)
        assert torch.equal(s.ids, base.ids.transpose(0, 1)) and torch.equal(s.weights, base.weights.transpose(0, 1))
        assert torch.equal(s.final_T, base.final_T.t())
        for kw in (dict(fine_binning=True), dict(no_footprint_cull=True)):
            for return_T in (False, True):
                o = R.render_topk(cam, k, mk(**kw), select=select, return_T=return_T)
                assert torch.equal(o.ids, base.ids) and torch.equal(o.weights, base.weights), (kw, select, return_T)
        for stepr, block in ((2, 1), (3, 2)):
            ids = torch.full((H, Wd, k), -7, dtype=torch.int32, device=base.ids.device)
            wts = torch.full((H, Wd, k), -7.0, dtype=torch.float32, device=base.ids.device)
            for r in range(stepr):
                strip = R.render_topk(cam, k, mk(tile_row_begin=r, tile_row_step=stepr, output_layout=2, tile_row_block=block), select=select)
                rows = G.renderer.shard_row_list(H, r, stepr, block)
                assert strip.ids.shape == (16 * len(rows), Wd, k)
                for j, ty in enumerate(rows):
                    h = min(16, H - ty * 16)
                    ids[ty * 16: ty * 16 + h] = strip.ids[j * 16: j * 16 + h]
                    wts[ty * 16: ty * 16 + h] = strip.weights[j * 16: j * 16 + h]
                    assert bool((strip.ids[j * 16 + h: (j + 1) * 16] == -1).all())  # rows below the frame: nothing drawn
            assert torch.equal(ids, base.ids) and torch.equal(wts, base.weights), (select, stepr, block)


@pytest.mark.parametrize("k", [5, 8])
def test_draw_limit_compat_and_early_out_against_weights_rendered_alike(G, k):
    c = _case(G, "f3a")
    R, cam, mk = c["R"], c["cam"], G.renderer.make_options
    _exact(G, c)
    n, dev = R.scene.n, R.scene.device
    eye = torch.eye(n, dtype=torch.float32, device=dev)
    step = _steps(c["appear"])
    if "W_opts" not in c:  # rendered once, shared by both k
        c["W_opts"] = {}
        for key, kw in [(("draw_limit", d), dict(draw_limit=d)) for d in (1, 7, 21)] + [(("early", 1e-2), dict(early_out_T=1e-2)),
                                                                                        (("compat", 0), dict(reference_compat=False))]:
            c["W_opts"][key] = (kw, *R.render_features(cam, eye, mk(**kw), return_T=True))
    if "step_compat0" not in c:
        # reference_compat = 0 draws gaussians the reference_compat sweep never gave weight (855 of f3a's 13950 pixels hold one): its
        # draw order comes from a prefix sweep under the same options, as _exact's does
        Wfull = c["W_opts"]["compat", 0][1]
        s0 = torch.zeros(n, dtype=torch.int32, device=dev)
        for j in range(1, n + 1):
            Wj = R.render_features(cam, eye, mk(draw_limit=j, reference_compat=False))
            has = (Wj > 0).flatten(0, 1).any(0)
            s0 = torch.where(has & (s0 == 0), torch.full_like(s0, j), s0)
        assert torch.equal(Wj, Wfull)  # the sweep ended on the frame's own weights
        c["step_compat0"] = s0
    for key, (kw, Wo, To) in c["W_opts"].items():
        order = c["step_compat0"] if key[0] == "compat" else step
        assert bool((order[(Wo > 0).flatten(0, 1).any(0)] > 0).all()), key  # every contributor has its place in the draw order
        if key[0] == "compat":
            assert bool((Wo[-1] > 0).any()) or bool((Wo[:, -1] > 0).any())
            assert bool(((Wo > 0) & (step == 0)).any())  # ... and some have none in the reference_compat sweep's
        # (early_out_T = 1e-2 ends no quadrant of this sparse frame early — its weights are the whole draw's; thresholds that do cut
        # are held the same way on the deep tile, test_a_deep_tile_displaces_full_lists_in_the_later_batches)
        for select in SELECTS:
            exp = _expected(Wo, order, k, select)
            for return_T in (False, True):
                got = R.render_topk(cam, k, mk(**kw), select=select, return_T=return_T)
                _assert_lists((key, k, select, return_T), got, exp, k)
                if return_T:
                    assert torch.equal(got.final_T, To), (key, k, select)


# ---- 6: edges -----------------------------------------------------------------------------------------------------------------
def test_degenerate_inputs_overflow_and_scene_order(G):
    p = G.synthetic.look_at_pose((0, -4, 0.5), (0, 0, 0), 1, "x.png")
    W, H = 33, 17
    fx = G.synthetic.pinhole_focal(W)
    cam = G.renderer.make_camera(p.qvec, p.tvec, 2 * fx, 2 * fx, 2 * W, 2 * H, W, H)
    cols = G.synthetic.mip360_like(300, 3)
    for i in range(3):
        cols[f"scale_{i}"] = (cols[f"scale_{i}"] + np.float32(3.0)).astype(np.float32)

    def nothing(got, k):
        assert got.ids.shape == (H, W, k) and bool((got.ids == -1).all()) and not got.weights.any()
        assert bool((got.final_T == 1).all())

    empty = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(G.utils.pack_gaussians({k: v[:0] for k, v in cols.items()})))
    far = dict(cols)
    far["y"] = (far["y"] - np.float32(100.0)).astype(np.float32)  # every gaussian behind the camera
    culled = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(far))
    for k in (3, 16):
        for select in SELECTS:
            nothing(empty.render_topk(cam, k, select=select, return_T=True), k)
            nothing(culled.render_topk(cam, k, select=select, return_T=True), k)
            assert culled.last_stats["n_visible"] == 0 and culled.last_stats["wave_entries"] == 0

    # a pair buffer too small: re-rendered, the same lists as a roomy one
    c = _case(G, "f3a")
    R, cam3 = c["R"], c["cam"]
    small = G.renderer.Rasterizer(R.scene, max_pairs=64)
    for select in SELECTS:
        a, b = small.render_topk(cam3, 5, select=select, return_T=True), R.render_topk(cam3, 5, select=select, return_T=True)
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and bool((a.ids >= 0).any())
    assert small.max_pairs > 64

    # ids in the scene's order map to the default through the scene's permutation
    assert R.scene.order_t is not None
    for select in SELECTS:
        raw = R.render_topk(cam3, 8, select=select, scene_order=True)
        dflt = R.render_topk(cam3, 8, select=select)
        assert not torch.equal(raw.ids, dflt.ids) and torch.equal(raw.weights, dflt.weights)
        assert torch.equal(G.renderer.file_order_ids(raw.ids, R.scene.order_t), dflt.ids)
    with pytest.raises(ValueError):
        R.render_topk(cam3, 17)
    with pytest.raises(ValueError):
        R.render_topk(cam3, 4, select="median")

    # the sparse sum of a pixel's whole list is render_features' map up to the order of the additions
    k = 16
    got = R.render_topk(cam3, k)
    few = (c["W"] > 0).sum(-1) <= k
    sparse = G.renderer.topk_composite(got, c["Ft"])
    dense = R.render_features(cam3, c["Ft"])
    assert bool(few.any()) and torch.allclose(sparse[few], dense[few], rtol=1e-5, atol=1e-5 * float(dense.abs().max()))


# ---- 7: independent of every GPU kernel ---------------------------------------------------------------------------------------
def _oracle_weights(G, c):
    """[H,W,n] float32: the CPU oracle's compositing loop over one-hot colours, three gaussians per call."""
    if "Wo" not in c:
        n, H, W = c["R"].scene.n, c["cam"].height, c["cam"].width
        Wo = np.zeros((H, W, n), np.float32)
        _oracle_maps(G, c, np.zeros((n, 3), np.float32))  # (leaves the oracle's preprocess and depth order in c)
        for i0 in range(0, n, 3):
            onehot = np.zeros((n, 3), np.float32)
            ids = np.arange(i0, min(i0 + 3, n))
            onehot[ids, np.arange(len(ids))] = 1.0
            # _oracle_maps' call on one thread, as in tests/test_gpu_pick.py: hundreds of calls on a frame this small cost less than
            # as many thread teams
            screen, _, _ = G.orc.composite(c["order"], dict(c["pre"], rgb=onehot), W, H, limit=-1, threads=1)
            Wo[..., ids] = screen.transpose(1, 0, 2)[..., :len(ids)]
        c["Wo"] = Wo
    return c["Wo"]


@pytest.mark.parametrize("name", ["f1", "f3a", "f3b"])
@pytest.mark.parametrize("k", [4, 8])
def test_heaviest_lists_against_the_cpu_oracle(G, name, k):
    """Every slot weight within 1e-4 of the oracle's sorted weight in that slot; ids equal on every slot whose oracle weight differs
    from both sorted neighbours (the (k+1)-th included) by more than 2e-4 — a slot closer than that may legitimately swap — and the
    share of filled slots left out is <= 6 %.  The figures are printed."""
    c = _case(G, name)
    R, cam = c["R"], c["cam"]
    Wo = _oracle_weights(G, c)
    order = np.argsort(-Wo, axis=-1, kind="stable")[..., :k + 1]
    so = np.take_along_axis(Wo, order, -1)                      # [H,W,k+1] sorted, descending
    oid = np.where(so > 0, order, -1)[..., :k]
    got = R.render_topk(cam, k)
    gi, gw = got.ids.cpu().numpy(), got.weights.cpu().numpy()
    err = float(np.abs(gw - so[..., :k]).max())
    gap_right = so[..., :k] - so[..., 1:]
    gap_left = np.concatenate([np.full(so.shape[:2] + (1,), np.inf, np.float32), so[..., :k - 1] - so[..., 1:k]], -1)
    distinct = (gap_right > 2e-4) & (gap_left > 2e-4)
    filled = so[..., :k] > 0
    left_out = float((filled & ~distinct).sum()) / max(int(filled.sum()), 1)
    wrong = int(((gi != oid) & distinct & filled).sum())
    print(f"\n{name} k={k}: max |w_gpu - w_oracle| per slot {err:.3e}; filled slots {int(filled.sum())}, left out as closer than 2e-4 to a "
          f"neighbour {100 * left_out:.1f} %; ids differing on the others {wrong}")
    assert err <= 1e-4, (name, k, err)
    assert wrong == 0, (name, k, wrong)
    assert left_out <= 0.06, (name, k, left_out)
    assert int((filled & distinct).sum()) > 0
