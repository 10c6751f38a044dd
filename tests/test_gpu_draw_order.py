"""GPU: the draw order, pinned through the public frame on scenes where any swap shows (tests/order_scenes.py).

Everything drawn goes through two stable radix sorts (csrc/sort.hip, csrc/radix.h): the depth sort, whose digit geometry is planned
on the device from the frame's key range, and the pair sort that must keep that order inside every cell / tile list.  Compositing
is not commutative, so the order IS the result — but on random scenes two swapped neighbours rarely overlap.  On an order scene
every adjacent transposition inside a stack moves a sample by more than 9e-3 (tests/test_order_scenes.py asserts it with the CPU
oracle alone), twice what conftest.assert_frames_close lets a sample be off: in a GPU frame that passes it against the oracle's
frame no two neighbours of any stack are exchanged (not more: colours repeat every three ranks, see tests/order_scenes.py).  No
tolerance of its own is introduced here; between GPU paths frames are compared bit for bit.

Precondition, asserted on the GPU for every scene: the kernel's z_cam is bit for bit the key the builder chose.
"""
import numpy as np
import pytest
import torch

import order_scenes as osc
from conftest import assert_frames_close, psnr
from gpu_cases import namespace

pytestmark = pytest.mark.gpu

BS = (1, 9, 10, 18, 19, 27, 28, 29)
DEPTH_TILE = 512 * 16        # csrc/gsr_internal.h DEPTH_SORT_THREADS * DEPTH_SORT_ITEMS: keys per workgroup of a depth-sort pass
SHARD_TILE = 512 * 8         # csrc/gsr_internal.h DEPTH_SORT_THREADS * DEPTH_SORT_ITEMS_SHARD (GSR_DS_SHARD_ITEMS): a shard's compact records
TILE = 16
_ORACLE = {}   # oracle frames per (scene, camera); the scenes themselves are rebuilt where needed (deterministic, a second or less)


@pytest.fixture(scope="module")
def G():
    return namespace()


def _small(W, H, B, **kw):
    return osc.OrderScene(W, H, B, seed=100 + B, **kw)


def _oracle(G, key, s, vi=0):
    """Frame [H,W,3] of view vi from the CPU oracle, once per (scene, camera)."""
    k = (key, vi)
    if k not in _ORACLE:
        v = s.views[vi]
        img, drawn = G.orc.render(s.packed, G.orc.camera(*v.cam_args))
        assert drawn == v.n_drawn and np.isfinite(img).all(), (key, drawn, v.n_drawn)
        _ORACLE[k] = img
    return _ORACLE[k]


def _precondition(G, R, cam, s, v):
    z = R.preprocess_debug(cam)["cam_means"][:, 2].cpu().numpy()
    want = s.z_cam[v.drawn]
    assert np.array_equal(z[v.drawn].view(np.uint32), want.view(np.uint32)), \
        "the kernel's z_cam is not bit for bit the key the builder chose: the expected order is not defined on this device"


def _file_order(G, s):
    return G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(s.packed, spatial_order=False))


def _strips(G, R, cam, step, block, **kw):
    """tile-row shards rendered one by one and put back where their rows belong (test_tile_row_shards_reassemble_bit_exactly)."""
    H = cam.height
    img = torch.zeros((H, cam.width, 3), dtype=torch.float32, device="cuda")
    for r in range(step):
        o = G.renderer.make_options(tile_row_begin=r, tile_row_step=step, output_layout=2, tile_row_block=block, **kw)
        strip = R.render(cam, o)
        for k, ty in enumerate(G.renderer.shard_row_list(H, r, step, block)):
            h = min(TILE, H - ty * TILE)
            img[ty * TILE: ty * TILE + h] = strip[k * TILE: k * TILE + h]
    return img


@pytest.mark.parametrize("B", BS)
def test_every_plan_shape_draws_in_order(G, B):
    """1920x1080, one stack per quadrant (194 400 drawn gaussians + 24 300 decoys: two dozen depth-sort tiles, the two-quadrant blend
    walk), array order unrelated to depth: every plan the pass-0 rowscan can make — one pass (the result in buffer 1, pass 0 also the
    last and writing no keys), 9+1, 9+9, 9+5+5, 9+9+9, 9+7+7+5, 9+7+7+6 — and the same frame under a depth_sort_passes bound that
    holds; one pass short is refused."""
    W, H = 1920, 1080
    s = _small(W, H, B)
    v = s.views[0]
    mk = G.renderer.make_options
    cam = G.renderer.make_camera(*v.cam_args)
    R = _file_order(G, s)
    _precondition(G, R, cam, s, v)
    plan = osc.plan_passes(B)
    assert plan == 1 + -(-max(B - 9, 0) // 9) == {1: 1, 9: 1, 10: 2, 18: 2, 19: 3, 27: 3, 28: 4, 29: 4}[B]
    img = R.render(cam).clone()                                    # no bound learned yet: four passes enqueued, `plan` run
    st = dict(R.last_stats)
    oimg = _oracle(G, ("small", W, H, B), s)
    print(f"\nB={B}: {s.n} gaussians, stats {st}, PSNR vs oracle {psnr(img.cpu().numpy(), oimg):.1f} dB")
    assert st["sort_passes"] == plan and st["n_visible"] == v.n_drawn and st["overflow"] == 0, st
    assert_frames_close(img.cpu().numpy(), oimg)
    assert R.sort_passes == plan
    assert torch.equal(R.render(cam), img)                          # the learned bound: `plan` passes enqueued
    for k in range(plan, 5):
        assert torch.equal(R.render(cam, mk(depth_sort_passes=k)), img), k
    if plan > 1:
        with pytest.raises(G._lib.GsrSortPasses):
            R.render(cam, mk(depth_sort_passes=plan - 1))
        assert R.last_stats["sort_passes"] == plan and R.last_stats["overflow"] == 2
        assert torch.equal(R.render(cam), img)                      # and a clean frame again
        assert R.last_stats["overflow"] == 0


@pytest.mark.parametrize("W,H", [(640, 360), (960, 540)])
@pytest.mark.parametrize("B", [9, 19, 28])
def test_plan_shapes_on_the_one_quadrant_walks(G, W, H, B):
    """640x360: the pipelined one-quadrant blend walk; 960x540: the plain one.  Per-tile pairs (fine_binning), the plain blend
    kernel and the preprocess-time colours draw the same bits, and those are the oracle's order."""
    s = _small(W, H, B)
    v = s.views[0]
    mk = G.renderer.make_options
    cam = G.renderer.make_camera(*v.cam_args)
    R = _file_order(G, s)
    _precondition(G, R, cam, s, v)
    img = R.render(cam).clone()
    assert R.last_stats["sort_passes"] == osc.plan_passes(B) and R.last_stats["n_visible"] == v.n_drawn
    assert_frames_close(img.cpu().numpy(), _oracle(G, ("small", W, H, B), s))
    for kw in (dict(fine_binning=True), dict(blend_impl=1), dict(colour_stage=1)):
        assert torch.equal(R.render(cam, mk(**kw)), img), kw


@pytest.mark.parametrize("V", [3 * DEPTH_TILE - 1, 3 * DEPTH_TILE, 3 * DEPTH_TILE + 1, 1, 63, 64, 65])
def test_visible_count_on_the_tile_and_wave_boundaries(G, V):
    """The number of gaussians that survive pass 0 lands on, one before and one past a multiple of the 8192-key tile (the later
    passes' last workgroup is full / holds one key / is missing) and of the 64-lane wave; B = 19 (9+5+5)."""
    W, H, B = 960, 540, 19
    s = osc.OrderScene(W, H, B, seed=V, n_drawn=V)
    v = s.views[0]
    assert v.n_drawn == V and s.n > V
    cam = G.renderer.make_camera(*v.cam_args)
    R = _file_order(G, s)
    _precondition(G, R, cam, s, v)
    img = R.render(cam)
    assert R.last_stats["n_visible"] == V and R.last_stats["sort_passes"] == 3, R.last_stats
    assert_frames_close(img.cpu().numpy(), _oracle(G, ("V", V), s))
    assert torch.equal(R.render(cam, G.renderer.make_options(fine_binning=True)), img)


@pytest.mark.parametrize("B", [1, 19, 28])
def test_default_scene_order_draws_ties_in_scene_order(G, B):
    """The loaders' default (Morton) order: the frame is the oracle's fed the arrays in the SCENE's order — exact ties follow it
    (test_depth_ties_at_different_positions_follow_the_scene_order); at B = 1 every stack is nothing but ties."""
    W, H = 640, 360
    s = _small(W, H, B)
    v = s.views[0]
    cam = G.renderer.make_camera(*v.cam_args)
    scene = G.renderer.GaussianScene.from_packed(s.packed)
    assert scene.order is not None and not np.array_equal(scene.order, np.arange(s.n))
    R = G.renderer.Rasterizer(scene)
    _precondition(G, R, cam, s, v)                                   # (preprocess_debug answers in file order)
    img = R.render(cam).cpu().numpy()
    assert R.last_stats["n_visible"] == v.n_drawn and R.last_stats["sort_passes"] == osc.plan_passes(B)
    ordered = {k: np.ascontiguousarray(a[scene.order]) for k, a in s.packed.items()}
    oimg, drawn = G.orc.render(ordered, G.orc.camera(*v.cam_args))
    assert drawn == v.n_drawn
    assert_frames_close(img, oimg)


@pytest.mark.parametrize("B", [19, 28])
def test_progressive_frames_cut_at_the_exact_rank(G, B):
    """draw_limit = k keeps depth ranks < k (binning.hip): the one place where the global order shows directly — a rank error at the
    cut removes or adds a whole gaussian (alpha ~ 0.5).  Cuts inside the first stack, around the first and at the second 8192-key
    tile boundary of the sorted order, and at the end."""
    W, H = 960, 540
    s = _small(W, H, B)
    v = s.views[0]
    V = v.n_drawn
    assert V > 2 * DEPTH_TILE + 1
    cam = G.renderer.make_camera(*v.cam_args)
    R = _file_order(G, s)
    _precondition(G, R, cam, s, v)
    oimg = _oracle(G, ("small", W, H, B), s)
    pre = G.orc.preprocess(s.packed, G.orc.camera(*v.cam_args))
    full = R.render(cam).clone()
    assert_frames_close(full.cpu().numpy(), oimg)
    prev = None
    for k in (1, 5, 6, 7, DEPTH_TILE - 1, DEPTH_TILE, DEPTH_TILE + 1, 2 * DEPTH_TILE, V - 1, V):
        img = R.render(cam, G.renderer.make_options(draw_limit=k)).cpu().numpy()
        screen, _, drawn = G.orc.composite(v.expected_order, pre, W, H, limit=k, threads=G.orc.max_threads())
        assert drawn == k and R.last_stats["n_visible"] == V
        assert_frames_close(img, screen.transpose(1, 0, 2))
        assert prev is None or not np.array_equal(prev, img), k     # every cut shows
        prev = img
    assert torch.equal(R.render(cam, G.renderer.make_options(draw_limit=V)), full)


@pytest.mark.parametrize("B", [19, 28])
def test_shards_keep_the_order(G, B):
    """Tile-row shards, whole-frame (1) and three-phase (2: compact records) shard preprocess, strips reassembled: bit for bit the
    unsharded frame, which is the oracle's.  The tie stacks here straddle multiples of 4096 and 8192 in the WHOLE frame's order:
    that places them on the 8192-key tiles of the unsharded sort only — a shard sorts just the gaussians that touch its rows, and
    its own tiles are aimed at by test_tie_stacks_straddle_the_tiles_of_a_shards_own_sort."""
    W, H = 960, 540
    at = (SHARD_TILE, DEPTH_TILE, 3 * SHARD_TILE, 2 * DEPTH_TILE)
    s = _small(W, H, B, tie_at=at)
    v = s.views[0]
    for p in at:
        a, b = v.expected_order[p - 1], v.expected_order[p]
        assert s.offset[a] == s.offset[b] and s.stack_of[a] == s.stack_of[b]
    cam = G.renderer.make_camera(*v.cam_args)
    R = _file_order(G, s)
    _precondition(G, R, cam, s, v)
    img = R.render(cam).clone()
    assert R.last_stats["n_visible"] == v.n_drawn
    assert_frames_close(img.cpu().numpy(), _oracle(G, ("small", W, H, B, at), s))
    Rm = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(s.packed))     # Morton order with block bounds, as the loaders build it
    img_m = Rm.render(cam).clone()
    for step in (2, 8):
        for block in (1, 2):
            for sp in (1, 2):
                assert torch.equal(_strips(G, R, cam, step, block, shard_preprocess=sp), img), (step, block, sp)
                assert torch.equal(_strips(G, Rm, cam, step, block, shard_preprocess=sp), img_m), (step, block, sp, "morton")


@pytest.mark.parametrize("B,step,block,begin", [(28, 2, 1, 1), (19, 2, 2, 0), (28, 8, 2, 3)])
def test_tie_stacks_straddle_the_tiles_of_a_shards_own_sort(G, B, step, block, begin):
    """A shard's depth sort holds only the gaussians that touch its tile rows (preprocess.hip: RowShard.any_in), so what its
    4096-key tiles (compact records, shard_preprocess = 2) or 8192-key tiles (1) cut is ITS sorted order.  1920x1080 with one stack
    per 16x16 tile: every stack lies in one tile row, the shard's order is the expected order restricted to its rows, and tie
    stacks hold positions p - 1, p, p + 1 of it for every multiple p of 4096 the shard reaches (the same scenes as
    tests/test_order_scenes.py of the same name).  That the shard sorts exactly that subsequence is checked by its n_visible."""
    W, H = 1920, 1080
    mk = G.renderer.make_options
    rows = G.renderer.shard_row_list(H, begin, step, block)
    n_strip = 6 * (W // 16) * len([t for t in rows if 16 * t + 8 <= H - 3])
    at = tuple(range(SHARD_TILE, n_strip - 6, SHARD_TILE))
    s = osc.OrderScene(W, H, B, seed=50 + step, stacks_per=16, tie_at=at, tie_rows=rows)
    v = s.views[0]
    sub = osc.order_in_rows(s, v, rows)
    assert len(at) >= 1 and len(sub) == n_strip
    for p in at:
        assert s.offset[sub[p - 1]] == s.offset[sub[p]] == s.offset[sub[p + 1]] and s.stack_of[sub[p - 1]] == s.stack_of[sub[p]]
    cam = G.renderer.make_camera(*v.cam_args)
    R = _file_order(G, s)
    _precondition(G, R, cam, s, v)
    img = R.render(cam).clone()
    assert R.last_stats["n_visible"] == v.n_drawn
    assert_frames_close(img.cpu().numpy(), _oracle(G, ("shard", B, step, block, begin), s))
    for sp in (1, 2):
        strip = R.render(cam, mk(tile_row_begin=begin, tile_row_step=step, output_layout=2, tile_row_block=block, shard_preprocess=sp))
        assert R.last_stats["n_visible"] == len(sub), (sp, R.last_stats, len(sub))      # the shard sorted exactly that subsequence
        for k, ty in enumerate(rows):
            h = min(TILE, H - ty * TILE)
            assert torch.equal(strip[k * TILE: k * TILE + h], img[ty * TILE: ty * TILE + h]), (sp, ty)


@pytest.mark.parametrize("Bf,Bb", [(9, 28), (28, 9), (1, 19)])
def test_two_plans_in_one_launch_sequence(G, Bf, Bb):
    """One scene in front of and one behind the origin, cameras [front, back, front] through one launch sequence (views = 3), two
    (views = 2) and two streams (FramesInFlight): every view sorts by its own plan in its own workspace slice."""
    W, H = 640, 360
    s = osc.OrderScene.two_sided(W, H, Bf, Bb, seed=7)
    scene = G.renderer.GaussianScene.from_packed(s.packed, spatial_order=False)
    cams = [G.renderer.make_camera(*v.cam_args) for v in s.views]
    plans = [osc.plan_passes(Bf), osc.plan_passes(Bb)]
    R = G.renderer.Rasterizer(scene)
    singles = []
    for vi, v in enumerate(s.views):
        _precondition(G, R, cams[vi], s, v)
        img = R.render(cams[vi]).clone()
        assert R.last_stats["sort_passes"] == plans[vi] and R.last_stats["n_visible"] == v.n_drawn, (vi, R.last_stats)
        assert_frames_close(img.cpu().numpy(), _oracle(G, ("two", Bf, Bb), s, vi))
        singles.append(img)
    assert not torch.equal(singles[0], singles[1])
    seq = [0, 1, 0]
    want = torch.stack([singles[i] for i in seq])
    for views in (2, 3):
        Rb = G.renderer.Rasterizer(scene, views=views)
        assert torch.equal(Rb.render_batch([cams[i] for i in seq]), want), views
        got = [d["sort_passes"] for d in Rb.last_slice_stats]
        assert got == [plans[i] for i in (seq[:3] if views == 3 else (0, 1))], (views, got)   # views = 2: slice 0 last rendered the third view
        assert [d["n_visible"] for d in Rb.last_slice_stats] == [s.views[i].n_drawn for i in (seq if views == 3 else (0, 1))]
        assert torch.equal(Rb.render_batch([cams[i] for i in seq]), want), (views, "with the learned bound")
    fif = G.renderer.FramesInFlight(scene, slots=2)
    assert torch.equal(fif.render_batch([cams[i] for i in seq]), want)
    assert [r.last_stats["sort_passes"] for r in fif.rasterizers] == plans     # slot 0: views 0 and 2 (front), slot 1: view 1 (back)


@pytest.mark.parametrize("W,H", [(1920, 1080), (4200, 2100)])
@pytest.mark.parametrize("B", [19, 28])
def test_wide_stacks_keep_their_order_through_the_pair_sort(G, W, H, B):
    """sigma ~20 px: every gaussian emits a dozen pairs or more, so a stack's order is carried by the pair sort's stability and the
    cell lists' tile masks.  4200x2100 (test_gpu_geometry's row H: gathered rects, per-tile pairs, 4-byte pair keys, three passes)."""
    s = osc.OrderScene(W, H, B, seed=B, wide=True)
    v = s.views[0]
    mk = G.renderer.make_options
    cam = G.renderer.make_camera(*v.cam_args)
    R = _file_order(G, s)
    _precondition(G, R, cam, s, v)
    img = R.render(cam).clone()
    st = dict(R.last_stats)
    assert st["n_visible"] == v.n_drawn and st["sort_passes"] == osc.plan_passes(B) and st["n_pairs"] >= 10 * v.n_drawn, st
    # (alpha >= 1/255 out to 3.1 sigma = 62 px: the disc's area is 11.8 cells of 32x32, a little less for the stacks at the frame's edge)
    assert_frames_close(img.cpu().numpy(), _oracle(G, ("wide", W, H, B), s))
    fine = R.render(cam, mk(fine_binning=True))
    assert torch.equal(fine, img)
    if W <= 4096:   # packed rects: the default frame binned by cell, the other by tile
        assert R.last_stats["n_pairs_bbox"] != st["n_pairs_bbox"]
    assert torch.equal(R.render(cam, mk(blend_impl=1)), img)
    Rm = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(s.packed))
    ordered = {k: np.ascontiguousarray(a[Rm.scene.order]) for k, a in s.packed.items()}
    assert_frames_close(Rm.render(cam).cpu().numpy(), G.orc.render(ordered, G.orc.camera(*v.cam_args))[0])


@pytest.mark.parametrize("B", [10, 28])
def test_a_frame_one_pass_under_an_even_plan_is_flagged_and_harmless(G, B):
    """A bound of ONE pass under a two- or four-pass plan.  By the plan's parity alone binning looked for the ids in val[0], which no
    pass of such a frame writes (pass 0 synthesises its index payload): whatever the workspace held was read as gaussian ids — an
    illegal memory access on a fresh workspace, where a bound learned on a one-pass view met a deeper one (test_two_plans_in_one_launch_sequence
    found it).  FrameCtrl.sort_buf now names the buffer the last pass that RAN wrote.  The C ABI asks nothing of a new
    workspace: filled with 0xFF, the short frame is flagged with the plan it needs and nothing else happens; the same workspace then
    renders the frame."""
    import ctypes as C

    from gsr_amd._lib import GsrStats, check, lib

    # (A test of the fix, on the fixed library: were the fix lost, the 0xFF words would be read as gaussian ids and the card would
    # fault rather than the test turn red — as test_a_fresh_workspace_needs_no_initialisation would for its word.)
    W, H = 640, 360
    s = _small(W, H, B)
    v = s.views[0]
    plan = osc.plan_passes(B)
    assert plan in (2, 4)
    mk = G.renderer.make_options
    cam = G.renderer.make_camera(*v.cam_args)
    R = _file_order(G, s)
    ref = R.render(cam).clone()
    assert_frames_close(ref.cpu().numpy(), _oracle(G, ("small", W, H, B), s))
    ws = torch.full((R._ws.numel(),), 0xFF, dtype=torch.uint8, device="cuda")
    out = torch.empty_like(ref)
    sc, st = R.scene.c_struct(), GsrStats()
    sp = int(torch.cuda.current_stream().cuda_stream)
    check(lib.gsr_render_forward(C.byref(sc), C.byref(cam), C.byref(mk(depth_sort_passes=1)), R.max_pairs, ws.data_ptr(), ws.numel(),
                                 out.data_ptr(), None, sp))
    assert lib.gsr_read_stats(ws.data_ptr(), ws.numel(), C.byref(st), sp) == G._lib.GSR_ERR_SORT_PASSES
    assert st.overflow & 2 and st.sort_passes == plan and st.n_visible == v.n_drawn
    check(lib.gsr_render_forward(C.byref(sc), C.byref(cam), C.byref(mk(depth_sort_passes=plan)), R.max_pairs, ws.data_ptr(), ws.numel(),
                                 out.data_ptr(), None, sp))
    check(lib.gsr_read_stats(ws.data_ptr(), ws.numel(), C.byref(st), sp))
    assert torch.equal(out, ref) and st.overflow == 0
    # the host class with a bound learned elsewhere: detected, raised, re-rendered
    R2 = _file_order(G, s)
    R2.sort_passes = 1
    assert torch.equal(R2.render(cam), ref) and R2.sort_passes == plan
