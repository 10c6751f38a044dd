"""GPU: the front slice (csrc/binning.hip, FramePlan.front_slice).  A whole colour frame under the exact colour-saturation rule is
built in two rounds: the nearest eighth of the draw order is binned and blended first (slice A), then the rest is binned only where a
tile is still open and blended on from the stored transmittance and colour sums (slice B).  The frame must be the single pass's bit
for bit.

saturation_rule = 3 forces the path on small frames, 4 switches it off.  Every frame is held with torch.equal to two references,
neither of which runs the code under test: (i) the same scene with saturation_rule = 4; (ii) "blend every entry": early_out_T = -1,
saturation_rule = 1.  The scenes are built in pixels (camera at the origin looking along +z, like tests/order_scenes.py): it is
known which gaussians are visible and what a wall in front of them closes.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_cases import medium_columns, namespace
from order_scenes import Q_BACK, camera_args

pytestmark = pytest.mark.gpu

C0 = 0.28209479177387814
FRACTION = 8  # csrc/gsr_internal.h FRONT_SLICE_FRACTION of the default build (the sweep builds of csrc/Makefile are for timing: the wall test's E is this fraction's)


@pytest.fixture(scope="module")
def G():
    return namespace()


def front_ranks(V):
    return (V + FRACTION - 1) // FRACTION


def room(W, H):
    """Gaussians a scene needs for the slice's planes to fit its workspace (they lie over per-gaussian arrays, 16 B per pixel: 257
    gaussians per tile, api.hip carve_workspace); saturation_rule = 3 is refused below that.  The scenes here reach it with gaussians
    that no camera sees: the visible ones stay few."""
    return 260 * ((W + 15) // 16) * ((H + 15) // 16) + 1024


class Pop:
    """Gaussians given in pixels: centre, sigma, opacity, colour; `depth` orders them (nearest first), whatever the array order."""

    def __init__(self):
        self.rows = []

    def add(self, cx, cy, sigma, opacity, rgb, depth):
        cx = np.atleast_1d(np.asarray(cx, np.float64))
        b = lambda v: np.broadcast_to(np.asarray(v, np.float64), cx.shape)
        rgb = np.broadcast_to(np.asarray(rgb, np.float64), cx.shape + (3,))
        self.rows.append(np.concatenate([np.stack([cx, b(cy), b(sigma), b(opacity), b(depth)], 1), rgb], 1))
        return self

    def packed(self, W, H, seed=3, behind=None, side=1.0):
        """The scene for the camera of camera_args(W, H); `behind` (default: room(W, H)) more gaussians on the other side of the
        camera (culled); side = -1: everything at -z, for the camera turned half round."""
        rng = np.random.default_rng(seed)
        r = np.concatenate(self.rows) if self.rows else np.zeros((0, 8))
        behind = room(W, H) if behind is None else behind
        if behind:
            r = np.concatenate([r, np.tile([[W / 2, H / 2, 3.0, 0.5, -1e6, 0.5, 0.5, 0.5]], (behind, 1))])
        r = r[rng.permutation(len(r))]  # array order against depth order
        n = len(r)
        _, f = camera_args(W, H)
        order = np.argsort(np.argsort(np.where(r[:, 4] <= -1e6, np.inf, r[:, 4]), kind="stable"), kind="stable")  # (the culled ones last)
        z = np.where(r[:, 4] <= -1e6, -2.0, 1.0 + 0.002 * order) * side
        x, y = (r[:, 0] + 0.5 - 0.5 * W) * z / f * side, (r[:, 1] + 0.5 - 0.5 * H) * np.abs(z) / f
        s = np.log(r[:, 2] * np.abs(z) / f)
        sh = np.zeros((n, 16, 3), np.float32)
        sh[:, 0, :] = (r[:, 5:8] - 0.5) / C0
        p = dict(means=np.stack([x, y, z], 1), log_scales=np.stack([s, s, s], 1), quats=np.tile([[1.0, 0.0, 0.0, 0.0]], (n, 1)),
                 opacity_logit=np.log(r[:, 3] / (1.0 - r[:, 3])), sh=sh)
        return {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}


def scatter(pop, rng, W, H, n, depth0, sigma=(1.5, 6.0), opacity=(0.05, 0.9), x=None):
    """n random gaussians at the depths depth0, depth0 + 1, ..."""
    x = x or (0, W)
    pop.add(rng.uniform(x[0], x[1], n), rng.uniform(0, H, n), rng.uniform(*sigma, n), rng.uniform(*opacity, n), rng.uniform(0.05, 1.0, (n, 3)),
            depth0 + np.arange(n))
    return pop


def wall(pop, rng, W, H, layers, depth0, x=None, rgb=None):
    """`layers` layers of nearly opaque gaussians (sigma 20 px, alpha capped at 0.99) on a grid 16 px apart over x[0] .. x[1].  A pixel
    lies within 3 px of a centre in each direction or between centres whose alphas are 0.66 and more: a layer leaves at most 1e-3 of
    T, eight layers 1e-24, far below 2^-25 of any colour sum of the wall (colours >= 0.3).  The wall must lie within the nearest eighth
    of the scene to close its tiles in slice A: the callers put seven times as many gaussians behind it."""
    x = x or (0, W)
    gx, gy = np.meshgrid(np.arange(x[0] + 2, x[1], 16.0), np.arange(2, H, 16.0))
    for k in range(layers):
        c = rng.uniform(0.3, 1.0, (gx.size, 3)) if rgb is None else rgb
        pop.add(gx.ravel(), gy.ravel(), 20.0, 0.995, c, depth0 + k + np.linspace(0, 0.5, gx.size))
    return pop


def scene_of(G, packed):
    return G.renderer.GaussianScene.from_packed(packed)


def cam_of(G, W, H, q=None):
    return G.renderer.make_camera(*(camera_args(W, H, q)[0] if q else camera_args(W, H)[0]))


def references(G, R, cam, **kw):
    """(the frame with the slice switched off, its counters); that frame equals blending every entry."""
    mk = G.renderer.make_options
    off = R.render(cam, mk(saturation_rule=4, **kw))
    st = dict(R.last_stats)
    every = R.render(cam, mk(early_out_T=-1.0, saturation_rule=1, **kw))
    assert torch.equal(off, every)
    return off, st


def sliced(G, R, cam, **kw):
    img = R.render(cam, G.renderer.make_options(saturation_rule=3, **kw))
    return img, dict(R.last_stats)


def check_scene(G, packed, W, H, **kw):
    """The forced front slice against both references; -> (counters sliced, counters unsliced)."""
    R, cam = G.renderer.Rasterizer(scene_of(G, packed)), cam_of(G, W, H)
    ref, st_off = references(G, R, cam, **kw)
    img, st_on = sliced(G, R, cam, **kw)
    assert torch.equal(img, ref)
    for k in ("n_visible", "n_pairs_bbox", "sort_passes", "overflow"):
        assert st_on[k] == st_off[k], (k, st_on, st_off)
    assert st_on["n_pairs"] <= st_off["n_pairs"]
    return st_on, st_off


def half_wall(W, H, n=4200, seed=5):
    """A wall over the left half among the nearest ranks, then n gaussians everywhere — one in six wide (rects of more than eight
    cells: the per-cell footprint test of the emit kernel runs), many straddling the wall's edge."""
    rng = np.random.default_rng(seed)
    pop = wall(Pop(), rng, W, H, 8, 0, x=(0, W // 2))
    scatter(pop, rng, W, H, n - n // 6, 100)
    scatter(pop, rng, W, H, n // 6, 100 + n, sigma=(14.0, 30.0), opacity=(0.2, 0.9), x=(W // 4, 3 * W // 4))
    return pop


@pytest.mark.parametrize("V", [0, 1, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 2057])
def test_visible_counts_at_the_slice_and_emit_block_edges(G, V):
    """L = ceil(V / 8) at and next to the edges of the 256-gaussian emit blocks: slice B starts mid-block, in the first block, with
    nothing (V <= 1: every rank is slice A's), or there is no gaussian at all.  200x120: cells cut by the frame's edge, 13 x 8 tiles."""
    W, H = 200, 120
    rng = np.random.default_rng(V)
    pop = scatter(Pop(), rng, W, H, V, 0, sigma=(1.5, 5.0), opacity=(0.3, 0.95)) if V else Pop()
    st_on, _ = check_scene(G, pop.packed(W, H), W, H)
    assert st_on["n_visible"] == V


def test_opaque_wall_closes_every_cell(G):
    """Every tile finishes in slice A: slice B emits no pair, and its blend finds no open tile.  E is then the entries of the first
    L ranks alone — what a progressive frame of L gaussians emits."""
    W, H = 200, 120
    rng = np.random.default_rng(1)
    pop = scatter(wall(Pop(), rng, W, H, 8, 0), rng, W, H, 6500, 100)  # 832 in the wall, L = 917
    packed = pop.packed(W, H)
    st_on, st_off = check_scene(G, packed, W, H)
    R, cam = G.renderer.Rasterizer(scene_of(G, packed)), cam_of(G, W, H)
    R.render(cam, G.renderer.make_options(saturation_rule=4, draw_limit=front_ranks(st_on["n_visible"])))
    print(f"\nwall: n_pairs sliced {st_on['n_pairs']}, unsliced {st_off['n_pairs']}, of the first L ranks {R.last_stats['n_pairs']}")
    assert st_on["n_pairs"] == R.last_stats["n_pairs"] < st_off["n_pairs"]
    assert st_on["fetched_entries"] <= st_off["fetched_entries"]


def test_transparent_scene_closes_no_cell(G):
    """No tile finishes in slice A: slice B emits every pair of its ranks with every bit, E is the single pass's."""
    W, H = 96, 80
    pop = scatter(Pop(), np.random.default_rng(2), W, H, 900, 0, opacity=(0.02, 0.15))
    st_on, st_off = check_scene(G, pop.packed(W, H), W, H)
    assert st_on["n_pairs"] == st_off["n_pairs"] > 0
    assert st_on["fetched_entries"] == st_off["fetched_entries"]  # every tile walks its whole list either way


@pytest.mark.parametrize("W,H", [(96, 80), (200, 120)])
def test_half_wall(G, W, H):
    """Closed and open cells side by side, gaussians across both, wide rects among them; also as a bf16 frame (the sums cross the
    boundary in fp32 whatever the frame's type) and without the reference's undrawn last column and row."""
    packed = half_wall(W, H).packed(W, H)
    st_on, st_off = check_scene(G, packed, W, H)
    print(f"\nhalf wall {W}x{H}: n_pairs sliced {st_on['n_pairs']}, unsliced {st_off['n_pairs']}")
    assert 0 < st_on["n_pairs"] < st_off["n_pairs"]
    check_scene(G, packed, W, H, output_bf16=True)
    check_scene(G, packed, W, H, reference_compat=False)
    check_scene(G, packed, W, H, colour_stage=1)


def test_late_red_keeps_tiles_open(G):
    """The wall has no red at all (the clamp leaves exactly 0): the threshold 2^-25 min(C) is 0 and only T == 0 finishes a pixel.  Four
    layers (120 gaussians, L = 265) leave 1e-22 < T < 1e-12 — the other two channels alone would have finished every pixel — so every
    tile stays open; the gaussians behind add a red far below the other sums, which the frame must hold bit for bit."""
    W, H = 96, 80
    rng = np.random.default_rng(4)
    pop = wall(Pop(), rng, W, H, 4, 0, rgb=(-4.0, 0.6, 0.8))
    scatter(pop, rng, W, H, 2000, 100)
    packed = pop.packed(W, H)
    st_on, st_off = check_scene(G, packed, W, H)
    assert st_on["n_pairs"] == st_off["n_pairs"]  # nothing closed
    R, cam = G.renderer.Rasterizer(scene_of(G, packed)), cam_of(G, W, H)
    red = sliced(G, R, cam)[0][:-1, :-1, 0]
    # (in the frame's far corner, 17 px from the last centre, a layer leaves up to 0.15 of T: 5e-4 after four; inside, below 1e-12)
    assert bool((red > 0).any()) and float(red.max()) < 1e-3 and float(red.median()) < 1e-10


def three_views(G, W, H):
    """One scene, three cameras of one frame size: in front a wall and what it hides; behind the camera (in front of the camera
    turned half round) a transparent population; the third camera stands where everything is behind it."""
    rng = np.random.default_rng(6)
    front = scatter(wall(Pop(), rng, W, H, 8, 0), rng, W, H, 6500, 100).packed(W, H, seed=7, behind=0)
    back = scatter(Pop(), rng, W, H, 1200, 0, opacity=(0.02, 0.15)).packed(W, H, seed=8, behind=0, side=-1.0)
    unseen = Pop().packed(W, H)  # (behind the first camera, and far off the second one's frustum)
    unseen["means"][:, 0] = 1e5
    packed = {k: np.ascontiguousarray(np.concatenate([front[k], back[k], unseen[k]])) for k in front}
    a_front, a_back = camera_args(W, H)[0], camera_args(W, H, Q_BACK)[0]
    a_none = (a_front[0], np.array([0.0, 0.0, -1000.0])) + a_front[2:]
    return packed, [G.renderer.make_camera(*a) for a in (a_front, a_back, a_none)]


def test_three_views_in_one_batch(G):
    W, H = 200, 120
    packed, cams = three_views(G, W, H)
    scene, mk = scene_of(G, packed), G.renderer.make_options
    one = G.renderer.Rasterizer(scene)
    refs, stats = [], []
    for c in cams:
        refs.append(references(G, one, c)[0])
        stats.append(dict(one.last_stats))
    assert stats[0]["n_visible"] > 1000 and stats[1]["n_visible"] > 1000 and stats[2]["n_visible"] == 0
    R = G.renderer.Rasterizer(scene, views=3)
    batch = R.render_batch(cams, mk(saturation_rule=3))
    assert torch.equal(batch, torch.stack(refs))
    per = R.last_slice_stats
    assert [s["n_visible"] for s in per] == [s["n_visible"] for s in stats]
    # the wall view emits less than the single pass, the transparent view the same, the empty view nothing
    off = G.renderer.Rasterizer(scene, views=3)
    assert torch.equal(off.render_batch(cams, mk(saturation_rule=4)), batch)
    assert per[0]["n_pairs"] < off.last_slice_stats[0]["n_pairs"] and per[1]["n_pairs"] == off.last_slice_stats[1]["n_pairs"] > 0
    assert per[2]["n_pairs"] == 0
    assert [s["n_pairs_bbox"] for s in per] == [s["n_pairs_bbox"] for s in off.last_slice_stats]


def test_frames_in_flight_two_slots(G):
    W, H = 200, 120
    packed, cams = three_views(G, W, H)
    scene, mk = scene_of(G, packed), G.renderer.make_options
    one = G.renderer.Rasterizer(scene)
    refs = [references(G, one, c)[0] for c in cams]
    order = [0, 1, 2, 1, 0]
    fif = G.renderer.FramesInFlight(scene, slots=2)
    got = fif.render_batch([cams[i] for i in order], mk(saturation_rule=3))
    assert torch.equal(got, torch.stack([refs[i] for i in order]))
    fif2 = G.renderer.FramesInFlight(scene, slots=2, views=2)
    got = fif2.render_batch([cams[i] for i in order], mk(saturation_rule=3))
    assert torch.equal(got, torch.stack([refs[i] for i in order]))


def test_pair_overflow_in_either_slice_is_reported_and_recovered(G):
    """max_pairs below slice A's pairs, and between slice A's and slice B's: the frame is flagged (the sticky record, the full D as the
    need), and the retried frame is the reference."""
    W, H = 96, 80
    pop = scatter(Pop(), np.random.default_rng(9), W, H, 1600, 0, opacity=(0.02, 0.15))
    packed = pop.packed(W, H)
    scene, cam, mk = scene_of(G, packed), cam_of(G, W, H), G.renderer.make_options
    R = G.renderer.Rasterizer(scene)
    ref, st = references(G, R, cam)
    R.render(cam, mk(saturation_rule=4, draw_limit=front_ranks(st["n_visible"])))
    D, DA = st["n_pairs_bbox"], R.last_stats["n_pairs_bbox"]
    DB = D - DA  # the scene is transparent: no cell closes, slice B emits the rest
    print(f"\noverflow: D {D}, slice A {DA}, slice B {DB}")
    assert 64 < DA < DB
    for max_pairs in (DA // 2, (DA + DB) // 2):
        small = G.renderer.Rasterizer(scene, max_pairs=max_pairs)
        small.enqueue(cam, mk(saturation_rule=3))
        with pytest.raises(G.lib.GsrPairOverflow):
            small.stats()
        assert small.last_stats["overflow"] == 1 and small.last_stats["n_pairs_bbox"] == D
        again = small.render(cam, mk(saturation_rule=3))
        assert small.max_pairs >= D and torch.equal(again, ref)
        assert small.last_stats["overflow"] == 0 and small.last_stats["n_pairs_bbox"] == D


def test_forced_without_room_is_refused(G):
    """saturation_rule = 3 on a scene too small to hold the planes: an error, not a quiet single pass."""
    W, H = 200, 120
    pop = scatter(Pop(), np.random.default_rng(3), W, H, 500, 0)
    R = G.renderer.Rasterizer(scene_of(G, pop.packed(W, H, behind=5)))
    with pytest.raises(G.lib.GsrError, match="no room for the front slice"):
        R.render(cam_of(G, W, H), G.renderer.make_options(saturation_rule=3))
    assert R.render(cam_of(G, W, H)).any()  # the plan itself does not slice it


def test_stale_workspace(G):
    """A workspace filled with 0xFF, and one last used by the other path, by another scene's view and by another frame size."""
    W, H = 200, 120
    packed = half_wall(W, H).packed(W, H)
    scene, cam, mk = scene_of(G, packed), cam_of(G, W, H), G.renderer.make_options
    R = G.renderer.Rasterizer(scene)
    ref, _ = references(G, R, cam)
    fresh = G.renderer.Rasterizer(scene)
    fresh._workspace(W, H).fill_(255)
    assert fresh.unchecked.slices == 0  # no frame to chain onto: the next one clears the 0xFF control block
    assert torch.equal(fresh.render(cam, mk(saturation_rule=3)), ref)
    for rule in (4, 3, 3, 4, 3):
        assert torch.equal(R.render(cam, mk(saturation_rule=rule)), ref), rule
    back = cam_of(G, W, H, Q_BACK)  # another view: the scene's unseen gaussians, all at one spot
    assert torch.equal(R.render(back, mk(saturation_rule=3)), R.render(back, mk(saturation_rule=4)))
    assert torch.equal(R.render(cam, mk(saturation_rule=3)), ref)
    small = cam_of(G, 96, 80)
    assert torch.equal(R.render(small, mk(saturation_rule=3)), R.render(small, mk(saturation_rule=4)))
    assert torch.equal(R.render(cam, mk(saturation_rule=3)), ref)


def test_the_plan_slices_a_large_batch(G):
    """6 000 000 gaussians at 1920x1080, six views per launch sequence: the plan's two measured thresholds (api.hip, FRONT_SLICE_MIN_N
    and FRONT_SLICE_MIN_VIEWS), at which it takes the front slice by itself.  Every frame equals the one the staged calls build
    (gsr_preprocess, gsr_bin_sort, gsr_blend: complete lists, one blend); n_pairs below the staged lists' shows the path ran.  One view
    less, or one view alone, is built in one pass."""
    lib, check = G.lib.lib, G.lib.check
    cols, args = medium_columns(G, n=6_000_000, seed=361, shift=0.0, W=1920, H=1080, pose=0)
    scene, cam, opts = G.renderer.GaussianScene.from_columns(cols), G.renderer.make_camera(*args), G.renderer.make_options()
    del cols
    R = G.renderer.Rasterizer(scene, views=6)
    imgs = R.render_batch([cam] * 6, opts)
    per = [dict(s) for s in R.last_slice_stats]
    assert len(per) == 6
    ws, sc, sp = R._workspace(cam.width, cam.height), scene.c_struct(), G.renderer._stream_ptr(scene.device)
    staged = torch.empty_like(imgs[0])
    check(lib.gsr_preprocess(C.byref(sc), C.byref(cam), C.byref(opts), ws.data_ptr(), ws.numel(), None, sp))
    check(lib.gsr_bin_sort(scene.n, C.byref(cam), C.byref(opts), R.max_pairs, ws.data_ptr(), ws.numel(), sp))
    check(lib.gsr_blend(C.byref(sc), scene.n, C.byref(cam), C.byref(opts), R.max_pairs, ws.data_ptr(), ws.numel(), staged.data_ptr(), None, sp))
    R.unchecked.wrote(1)
    st_staged = dict(R.stats())
    print(f"\nplan: n_pairs of the batch's views {[s['n_pairs'] for s in per]}, of the staged lists {st_staged['n_pairs']}; D {st_staged['n_pairs_bbox']}")
    for k in range(6):
        assert torch.equal(imgs[k], staged), k
        assert per[k]["n_pairs"] < st_staged["n_pairs"], k
        assert per[k]["n_visible"] == st_staged["n_visible"] and per[k]["n_pairs_bbox"] == st_staged["n_pairs_bbox"], k
    five = R.render_batch([cam] * 5, opts)                                                # five views per launch sequence: one pass
    assert torch.equal(five[4], staged) and [s["n_pairs"] for s in R.last_slice_stats] == [st_staged["n_pairs"]] * 5
    one = G.renderer.Rasterizer(scene)
    assert torch.equal(one.render(cam, opts), staged) and one.last_stats["n_pairs"] == st_staged["n_pairs"]   # one view: one pass
    assert torch.equal(one.render(cam, G.renderer.make_options(saturation_rule=3)), staged) and one.last_stats["n_pairs"] < st_staged["n_pairs"]


def test_lists_after_a_fused_frame_are_remade_by_the_staged_calls(G):
    """include/gsr.h, gsr_render_forward: a fused colour-frame entry owes the frame, not the lists — after a sliced frame the workspace
    holds the second slice's remainder.  A list consumer on the same workspace is right again after gsr_preprocess + gsr_bin_sort (what
    the Rasterizer does for every consumer), and with saturation_rule = 4 the fused entry leaves complete lists as it always did."""
    lib, check = G.lib.lib, G.lib.check
    W, H = 200, 120
    packed = half_wall(W, H).packed(W, H)
    scene, cam, mk = scene_of(G, packed), cam_of(G, W, H), G.renderer.make_options
    R = G.renderer.Rasterizer(scene)
    feats = torch.rand((scene.n, 3), device="cuda")
    want = G.renderer.Rasterizer(scene).render_features(cam, feats, scene_order=True)   # staged lists on a workspace of its own
    ws, sc, sp = R._workspace(W, H), scene.c_struct(), G.renderer._stream_ptr(scene.device)

    def features_over_the_workspace(o):
        out = torch.empty((H, W, 3), device="cuda")
        check(lib.gsr_blend_features(scene.n, C.byref(cam), C.byref(o), R.max_pairs, ws.data_ptr(), ws.numel(), feats.data_ptr(), out.data_ptr(), None, sp))
        return out

    R.render(cam, mk(saturation_rule=4))
    assert torch.equal(features_over_the_workspace(mk(saturation_rule=4)), want)   # the single pass leaves the frame's lists
    R.render(cam, mk(saturation_rule=3))
    assert not torch.equal(features_over_the_workspace(mk()), want)                # the remainder: what the header warns of
    o = mk()
    check(lib.gsr_preprocess(C.byref(sc), C.byref(cam), C.byref(o), ws.data_ptr(), ws.numel(), None, sp))
    check(lib.gsr_bin_sort(scene.n, C.byref(cam), C.byref(o), R.max_pairs, ws.data_ptr(), ws.numel(), sp))
    assert torch.equal(features_over_the_workspace(o), want)
    assert torch.equal(R.render_features(cam, feats, scene_order=True), want)      # the Rasterizer's own way
