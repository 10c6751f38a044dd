"""GPU: loads that the radix passes and the blend's colour evaluation request ahead of their dependent chains.

csrc/sort.hip: radix_scatter_kernel requests its keys, its digit's total, its tile's entry of the scanned histogram and the plan's
pass count right after it knows its tile — ahead of the LDS clear — and scans the digit totals while the keys are in flight;
radix_hist_kernel requests its keys ahead of the barrier that publishes the cleared histogram.  No stored byte changes, so what can
go wrong is a load from the wrong place or past an end: a partial tile's keys (its loads are clamped to the last key), a table word
of another view's slice or of a digit value the pass does not have, a pass the plan does not need, a workspace that holds anything.
The shapes below are the smallest that reach each of these.  The colour cases at the end hold csrc/blend.hip q2_resolve, which reads
a pending gaussian's mean and SH row, to the same standard on the row that ends where the array ends: the request of the row's lines
ahead of the evaluation was measured and not kept, and whoever tries it again finds its test here.

Frames are held to the CPU oracle (conftest.assert_frames_close); frames of different GPU paths are compared bit for bit.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import order_scenes as osc
from conftest import assert_frames_close
from gpu_cases import namespace

pytestmark = pytest.mark.gpu

TILE = 16
DEPTH_TILE = 512 * 16         # csrc/gsr_internal.h DEPTH_SORT_THREADS * DEPTH_SORT_ITEMS
PAIR_TILE = 256 * 16          # PAIR_SORT_THREADS * PAIR_SORT_ITEMS
_ORACLE = {}


@pytest.fixture(scope="module")
def G():
    return namespace()


def _file_order(G, packed, **kw):
    return G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(packed, spatial_order=False), **kw)


def _oracle(G, key, packed, args, want_drawn=None):
    if key not in _ORACLE:
        img, drawn = G.orc.render(packed, G.orc.camera(*args))
        assert want_drawn is None or drawn == want_drawn, (key, drawn, want_drawn)
        _ORACLE[key] = img
    return _ORACLE[key]


def _z_cam_is_the_key(R, cam, z_cam, drawn):
    z = R.preprocess_debug(cam)["cam_means"][:, 2].cpu().numpy()
    assert np.array_equal(z[drawn].view(np.uint32), z_cam[drawn].view(np.uint32)), \
        "the kernel's z_cam is not bit for bit the key the builder chose: the expected order is not defined on this device"


# ---- depth sort ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [10, 19, 28])
@pytest.mark.parametrize("V", [5, DEPTH_TILE, DEPTH_TILE + 1])
def test_depth_sort_tiles_and_plans(G, V, B):
    """V drawn gaussians of an order scene at 1920x1080, file order: a lone partial tile, exactly one full tile, one full and one
    partial in the passes after pass 0 (pass 0 runs over the scene's n > V keys and drops the decoys').  Plans of 2, 3 and 4 passes.
    A fresh Rasterizer enqueues four passes (depth_sort_passes at its default): the passes the plan does not need return early; then
    the same frame with exactly the plan's passes enqueued, and with per-tile pairs."""
    W, H = 1920, 1080
    s = osc.OrderScene(W, H, B, seed=100 * B + V % 97, n_drawn=V)
    v = s.views[0]
    plan = osc.plan_passes(B)
    assert v.n_drawn == V and s.n > V and plan == {10: 2, 19: 3, 28: 4}[B]
    mk = G.renderer.make_options
    cam = G.renderer.make_camera(*v.cam_args)
    R = _file_order(G, s.packed)
    _z_cam_is_the_key(R, cam, s.z_cam, v.drawn)
    img = R.render(cam).clone()                                     # no bound learned yet: four passes enqueued, `plan` run
    st = dict(R.last_stats)
    assert st["n_visible"] == V and st["sort_passes"] == plan and st["overflow"] == 0, st
    assert_frames_close(img.cpu().numpy(), _oracle(G, ("depth", V, B), s.packed, v.cam_args, V))
    assert torch.equal(R.render(cam, mk(depth_sort_passes=plan)), img)
    assert torch.equal(R.render(cam, mk(depth_sort_passes=4)), img)
    assert torch.equal(R.render(cam, mk(fine_binning=True)), img)


# ---- pair sort ----------------------------------------------------------------------------------------------------------------------

def test_a_cell_pass_with_fewer_digit_values_than_threads(G):
    """64x48: 2 x 2 cells of 32x32, keys of 1 + 2 bits — the pair sort's one pass has 8 digit values for 256 threads (per-tile pairs:
    4 x 3 tiles, 2 + 2 bits, 16 values), so 248 threads own no digit and must neither count nor contribute a table word."""
    W, H = 64, 48
    s = osc.OrderScene(W, H, 12, seed=5)
    v = s.views[0]
    cam = G.renderer.make_camera(*v.cam_args)
    R = _file_order(G, s.packed)
    _z_cam_is_the_key(R, cam, s.z_cam, v.drawn)
    img = R.render(cam).clone()
    assert R.last_stats["n_visible"] == v.n_drawn and R.last_stats["n_pairs"] >= v.n_drawn
    assert_frames_close(img.cpu().numpy(), _oracle(G, ("cells", W, H), s.packed, v.cam_args, v.n_drawn))
    assert torch.equal(R.render(cam, G.renderer.make_options(fine_binning=True)), img)
    assert torch.equal(R.render(cam, G.renderer.make_options(blend_impl=1)), img)


@pytest.mark.parametrize("W,H,stacks", [(4200, 2100, 20000), (4112, 64, None)])
def test_frames_past_the_packed_rect(G, W, H, stacks):
    """4200x2100: 263 x 132 tiles — the depth sort carries the ids alone (4-byte payload, the rects gathered by id), per-tile pairs
    under 9 + 8 = 17-bit keys, stored as 32-bit words, in three passes; 20 000 stacks of the 137 550 the frame has room for, so the
    depth sort and the pair sort both run over many tiles.  4112x64: 257 tiles across, ids alone again, 9 + 3 bits in 2-byte keys."""
    s = osc.OrderScene(W, H, 19, seed=W, max_stacks=stacks)
    v = s.views[0]
    cam = G.renderer.make_camera(*v.cam_args)
    R = _file_order(G, s.packed)
    _z_cam_is_the_key(R, cam, s.z_cam, v.drawn)
    img = R.render(cam).clone()
    st = dict(R.last_stats)
    assert st["n_visible"] == v.n_drawn and st["sort_passes"] == 3 and st["overflow"] == 0, st
    if stacks:
        assert st["n_pairs"] > 2 * PAIR_TILE and v.n_drawn > 2 * DEPTH_TILE, st
    assert img[:, 4100:].any()                                      # content past tile column 256
    assert_frames_close(img.cpu().numpy(), _oracle(G, ("past", W, H), s.packed, v.cam_args, v.n_drawn))
    assert torch.equal(R.render(cam, G.renderer.make_options(fine_binning=True)), img)


# ---- several views, stale workspaces, shards ----------------------------------------------------------------------------------------

def test_three_views_with_three_visible_counts_in_one_launch_sequence(G):
    """One launch sequence (gridDim.y = 3) over the camera of an order scene with one full and one partial depth-sort tile, the same
    camera moved sideways (part of the scene leaves the frustum: another count) and moved ten units forward (everything behind it:
    zero visible: pass 0 drops every key, the later passes' workgroups have no tile).  Every view reads its own slice's counts and tables: bit
    for bit the three single-view frames, in either order."""
    W, H, V = 1920, 1080, DEPTH_TILE + 1
    s = osc.OrderScene(W, H, 19, seed=3, n_drawn=V)
    q, t, fx, fy, cw, ch, w, h = s.cam_args
    args = [s.cam_args, (q, np.array([0.05, 0.0, 0.0]), fx, fy, cw, ch, w, h), (q, np.array([0.0, 0.0, -10.0]), fx, fy, cw, ch, w, h)]
    scene = G.renderer.GaussianScene.from_packed(s.packed, spatial_order=False)
    cams = [G.renderer.make_camera(*a) for a in args]
    R = G.renderer.Rasterizer(scene)
    singles, counts = [], []
    for k, cam in enumerate(cams):
        img = R.render(cam).clone()
        counts.append(R.last_stats["n_visible"])
        assert_frames_close(img.cpu().numpy(), _oracle(G, ("views", k), s.packed, args[k]))
        singles.append(img)
    assert counts[0] == V and counts[2] == 0 and 0 < counts[1] != V, counts
    assert not singles[2].any() and not torch.equal(singles[0], singles[1])
    Rb = G.renderer.Rasterizer(scene, views=3)
    for seq in ([0, 1, 2], [2, 1, 0], [1, 2, 0]):
        got = Rb.render_batch([cams[i] for i in seq])
        assert torch.equal(got, torch.stack([singles[i] for i in seq])), seq
        assert [d["n_visible"] for d in Rb.last_slice_stats] == [counts[i] for i in seq], seq


def test_a_workspace_that_holds_anything(G):
    """The C ABI on a workspace filled with 0xFF: the first frame (a two-pass plan under four enqueued passes), then on the same
    workspace a frame of a four-pass plan, then the first again: the hoisted loads read only what this frame's kernels wrote."""
    from gsr_amd._lib import GsrStats, check, lib

    W, H = 640, 360
    s = osc.OrderScene.two_sided(W, H, 10, 28, seed=11)
    cams = [G.renderer.make_camera(*v.cam_args) for v in s.views]
    R = _file_order(G, s.packed)
    refs = []
    for vi, v in enumerate(s.views):
        img = R.render(cams[vi]).clone()
        assert R.last_stats["sort_passes"] == (2, 4)[vi] and R.last_stats["n_visible"] == v.n_drawn, (vi, R.last_stats)
        assert_frames_close(img.cpu().numpy(), _oracle(G, ("stale", vi), s.packed, v.cam_args, v.n_drawn))
        refs.append(img)
    ws = torch.full((R._ws.numel(),), 0xFF, dtype=torch.uint8, device="cuda")
    sc, st = R.scene.c_struct(), GsrStats()
    sp = int(torch.cuda.current_stream().cuda_stream)
    for vi in (0, 1, 0):
        out = torch.empty_like(refs[vi])
        check(lib.gsr_render_forward(C.byref(sc), C.byref(cams[vi]), C.byref(G.renderer.make_options(depth_sort_passes=4)), R.max_pairs,
                                     ws.data_ptr(), ws.numel(), out.data_ptr(), None, sp))
        check(lib.gsr_read_stats(ws.data_ptr(), ws.numel(), C.byref(st), sp))
        assert st.overflow == 0 and st.sort_passes == (2, 4)[vi] and st.n_visible == s.views[vi].n_drawn, vi
        assert torch.equal(out, refs[vi]), vi


def test_one_rank_of_an_eight_shard_plan(G):
    """Rank 3 of eight tile-row shards at 1920x1080: the depth sort's 8-keys-per-thread tiles (4096 keys, over the compact records of
    shard_preprocess = 2; with 1, 8192-key tiles over one key per gaussian).  The strip's rows are bit for bit the whole frame's,
    which is the oracle's."""
    W, H, begin, step = 1920, 1080, 3, 8
    s = osc.OrderScene(W, H, 19, seed=58, stacks_per=16)
    v = s.views[0]
    rows = G.renderer.shard_row_list(H, begin, step, 1)
    sub = osc.order_in_rows(s, v, rows)
    assert len(sub) > 4096                                          # more than one of the shard's tiles
    cam = G.renderer.make_camera(*v.cam_args)
    R = _file_order(G, s.packed)
    _z_cam_is_the_key(R, cam, s.z_cam, v.drawn)
    img = R.render(cam).clone()
    assert_frames_close(img.cpu().numpy(), _oracle(G, ("shard",), s.packed, v.cam_args, v.n_drawn))
    for sp in (1, 2):
        strip = R.render(cam, G.renderer.make_options(tile_row_begin=begin, tile_row_step=step, output_layout=2, shard_preprocess=sp))
        assert R.last_stats["n_visible"] == len(sub), (sp, R.last_stats, len(sub))
        for k, ty in enumerate(rows):
            hh = min(TILE, H - ty * TILE)
            assert torch.equal(strip[k * TILE: k * TILE + hh], img[ty * TILE: ty * TILE + hh]), (sp, ty)


@pytest.mark.parametrize("n", [1, PAIR_TILE, PAIR_TILE + 1])
def test_scene_order_on_one_tile_and_one_key_more(G, n):
    """gsr_scene_order (sixteen passes of the 256-thread kernels, the count on the host side) on a lone key, exactly one tile, and one
    tile and one key: means from a 7 x 5 x 3 grid, so that only a stable sort gives renderer.morton_order's permutation."""
    rng = np.random.default_rng(n)
    means = np.stack([rng.integers(0, 7, n), rng.integers(0, 5, n), rng.integers(0, 3, n)], 1).astype(np.float32) * np.float32(0.25) - 1
    want = G.renderer.morton_order(means)
    got = G.renderer.scene_order(torch.from_numpy(means).cuda()).cpu().numpy()
    assert np.array_equal(got, want)


# ---- colours ------------------------------------------------------------------------------------------------------------------------

def _colour_scene(W, H, n=3000, seed=29):
    """Camera at the origin looking along +z.  n - 1 small gaussians at depths 1 .. 3 all over the W x H frame and, LAST in the
    arrays, the nearest one: six pixels wide in the middle of the frame, so every tile around the centre stages it first and needs
    its colour.  Every SH coefficient is set: each band of the row changes the colour."""
    f = W / (2.0 * math.tan(math.radians(60.0) / 2.0))
    args = (np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3), 2.0 * f, 2.0 * f, 2 * W, 2 * H, W, H)
    rng = np.random.default_rng(seed)
    px, py = rng.uniform(0, W, n), rng.uniform(0, H, n)
    z = rng.uniform(1.0, 3.0, n)
    sig = rng.uniform(0.8, 3.0, n)
    op = rng.uniform(0.2, 0.8, n)
    px[-1], py[-1], z[-1], sig[-1], op[-1] = 0.5 * W - 0.7, 0.5 * H + 0.6, 0.5, 6.0, 0.6
    s = np.log(sig * z / f)
    qn = rng.normal(size=(n, 4))
    sh = rng.normal(size=(n, 16, 3)) * 0.15
    sh[:, 0, :] = rng.uniform(-0.5, 1.5, (n, 3))
    packed = dict(means=np.stack([(px + 0.5 - 0.5 * W) * z / f, (py + 0.5 - 0.5 * H) * z / f, z], 1),
                  log_scales=np.stack([s, s + rng.uniform(-0.3, 0.3, n), s], 1), quats=qn / np.linalg.norm(qn, axis=1, keepdims=True),
                  opacity_logit=np.log(op / (1.0 - op)), sh=sh)
    return {k: np.ascontiguousarray(a, dtype=np.float32) for k, a in packed.items()}, args


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
@pytest.mark.parametrize("W,H", [(64, 64), (1024, 768)])
def test_the_last_gaussians_row_is_pending_and_needed(G, W, H, degree, half):
    """The gaussian with the highest id — its SH row ends where the array ends — is the nearest one and drawn by the tiles in the
    middle of the frame, so its colour is pending (colour_stage = 0) and needed.  SH degree 0 .. 3 (12 .. 192 B of the row are read;
    fp16: 6 .. 96), through gsr_blend with the scene handed in and with the scene the preprocess stashed, on the plain kernel and on
    the walk kernels (64x64, 16 tiles: the pipelined one-quadrant walk and, with blend_pipe_tiles = -1, the plain one; 1024x768,
    3072 tiles: two quadrants per wave): every frame equals, bit for bit, the one with the colours evaluated in the preprocess,
    which is the oracle's."""
    from gsr_amd._lib import check, lib

    packed, args = _colour_scene(W, H)
    n = len(packed["means"])
    if half:  # what the fp16 rows hold, for the oracle
        packed = dict(packed, sh=packed["sh"].astype(np.float16).astype(np.float32))
    scene = G.renderer.GaussianScene.from_packed(packed, sh_degree=degree, sh_half=half, spatial_order=False)
    cam = G.renderer.make_camera(*args)
    R = G.renderer.Rasterizer(scene)
    eager = R.render(cam, G.renderer.make_options(colour_stage=1)).clone()
    key = ("colour", W, H, degree, half)
    if key not in _ORACLE:
        _ORACLE[key] = G.orc.render(packed, G.orc.camera(*args), sh_degree=degree)[0]
    assert_frames_close(eager.cpu().numpy(), _ORACLE[key])
    alone = G.orc.render({k: a[-1:] for k, a in packed.items()}, G.orc.camera(*args), sh_degree=degree)[0]
    assert alone[H // 2 - 8: H // 2 + 8, W // 2 - 8: W // 2 + 8].max() > 0.05   # the last gaussian shows in the middle tiles
    ws = R._workspace(cam.width, cam.height)
    sc = scene.c_struct()
    sp = int(torch.cuda.current_stream().cuda_stream)
    variants = (dict(), dict(blend_impl=1)) + ((dict(blend_pipe_tiles=-1),) if W == 64 else ())
    for kw in variants:
        for handed in (True, False):
            o = R.bounded(G.renderer.make_options(**kw))
            check(lib.gsr_preprocess(C.byref(sc), C.byref(cam), C.byref(o), ws.data_ptr(), ws.numel(), None, sp))
            check(lib.gsr_bin_sort(n, C.byref(cam), C.byref(o), R.max_pairs, ws.data_ptr(), ws.numel(), sp))
            out = torch.zeros((cam.height, cam.width, 3), dtype=torch.float32, device="cuda")
            check(lib.gsr_blend(C.byref(sc) if handed else None, n, C.byref(cam), C.byref(o), R.max_pairs, ws.data_ptr(), ws.numel(),
                                out.data_ptr(), None, sp))
            assert R.stats()["colour_evals"] > 0, (kw, handed)
            assert torch.equal(out, eager), (kw, handed)
