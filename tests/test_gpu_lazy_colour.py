"""GPU: deferred colours are evaluated only for entries a live quadrant blends (blend.hip, blend_walk_kernel; blend_common.h,
next_batch).  The thread that stages a list entry classifies it against the tile's four 8x8 quadrants and evaluates a pending
colour only when the entry hits a quadrant that has not finished; the record stays pending for the next tile that needs it.

Frames are bit-identical to the colour evaluated in the preprocess (colour_stage = 1) on every kernel variant the plan can pick;
the scenes of the second half are built in pixels (camera at the origin looking along +z, like tests/margin_scenes.py) so that
it is known, from the CPU oracle's own per-pixel evaluation, which colours nobody needs.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import golden_columns, load_golden
from gpu_cases import f5_case, golden_args, namespace

pytestmark = pytest.mark.gpu

SAME_COUNTERS = ("n_pairs", "fetched_entries", "wave_entries")


@pytest.fixture(scope="module")
def G():
    return namespace()


def _ring_args(G, W, H, pose):
    p = G.synthetic.ring_cameras(25)[pose]
    fx = G.synthetic.pinhole_focal(W)
    return (p.qvec, p.tvec, 2 * fx, 2 * fx, 2 * W, 2 * H, W, H)


def _random_cols(G, n=2000, seed=11, shift=2.0):
    cols = G.synthetic.mip360_like(n, seed)
    for i in range(3):
        cols[f"scale_{i}"] = (cols[f"scale_{i}"] + np.float32(shift)).astype(np.float32)
    return cols


def _check_paths(G, R, cam, kw, what, want_T=True):
    """colour_stage 0 == 1 and blend_impl 0 == 1: frames (and final T), and the counters that lazy colours must not move."""
    mk = G.renderer.make_options
    frames, stats = {}, {}
    for impl in (0, 1):
        for stage in (1, 0):
            o = mk(colour_stage=stage, blend_impl=impl, **kw)
            got = R.render(cam, o, return_T=True) if want_T else (R.render(cam, o), None)
            frames[impl, stage] = tuple(None if t is None else t.clone() for t in got)
            stats[impl, stage] = dict(R.last_stats)
    ref_img, ref_T = frames[0, 1]
    for key, (img, T) in frames.items():
        assert torch.equal(img, ref_img), (what, kw, key)
        assert T is None or torch.equal(T, ref_T), (what, kw, key)
    for impl in (0, 1):
        assert stats[impl, 1]["colour_evals"] == 0, (what, kw, impl)
        for k in SAME_COUNTERS:
            assert stats[impl, 0][k] == stats[impl, 1][k], (what, kw, impl, k)
        assert stats[impl, 0]["colour_evals"] <= stats[impl, 0]["fetched_entries"], (what, kw, impl)
    return stats


# whole frame (few tiles: the pipelined one-quadrant walk), the plain one-quadrant walk, the stop rules, "blend every entry"
SMALL_VARIANTS = (dict(), dict(blend_pipe_tiles=-1), dict(saturation_rule=1), dict(saturation_rule=1, early_out_T=-1.0),
                  dict(tile_row_begin=1, tile_row_step=2, output_layout=2))


def _fixture_cases(G):
    out = []
    for name, prefix in (("f2_small.npz", ""), ("f3_edge.npz", "a_"), ("f3_edge.npz", "b_")):
        g = load_golden(name)
        out.append((name + prefix, G.utils.pack_gaussians(golden_columns(g)), G.renderer.make_camera(*golden_args(g, prefix))))
    _, c = f5_case()
    out.append(("f5_deep_stack", c["packed"], G.renderer.make_camera(*c["args"])))
    return out


def test_fixture_frames_equal_across_colour_stage_and_blend_impl(G):
    for name, packed, cam in _fixture_cases(G):
        R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(packed))
        for kw in SMALL_VARIANTS:
            _check_paths(G, R, cam, kw, name)
        _check_paths(G, R, cam, dict(output_bf16=True), name, want_T=False)
    name, packed, cam = _fixture_cases(G)[0]
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(packed, sh_half=True))
    for kw in (dict(), dict(blend_pipe_tiles=-1)):
        _check_paths(G, R, cam, kw, name + " fp16 SH")


def test_random_scene_equal_on_every_blend_variant(G):
    """~2 000 gaussians: as a 64x48-pixel frame (12 tiles: the pipelined walk, the plain one-quadrant walk with blend_pipe_tiles = -1)
    and as a frame of 64x48 tiles (3072 >= 3000: two quadrants per wave; rows 0, 2, .. = 1536 tiles: one quadrant per wave; rows
    1, 5, .. = 768 tiles: the pipelined walk)."""
    cols = _random_cols(G)
    for sh_kw in (dict(), dict(sh_half=True)):
        R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols, **sh_kw))
        cam = G.renderer.make_camera(*_ring_args(G, 64, 48, 4))
        any_saved = False
        for kw in SMALL_VARIANTS:
            st = _check_paths(G, R, cam, kw, "64x48 px")
            any_saved |= st[0, 0]["colour_evals"] < st[0, 0]["fetched_entries"]
        _check_paths(G, R, cam, dict(output_bf16=True), "64x48 px", want_T=False)
        assert any_saved  # (deep enough to stage entries whose colour is already known or not needed)
        big = G.renderer.make_camera(*_ring_args(G, 1024, 768, 4))
        for kw in (dict(), dict(saturation_rule=1), dict(tile_row_begin=0, tile_row_step=2, output_layout=2),
                   dict(tile_row_begin=1, tile_row_step=4, output_layout=2)):
            _check_paths(G, R, big, kw, "64x48 tiles", want_T="tile_row_step" not in kw)
        _check_paths(G, R, big, dict(output_bf16=True), "64x48 tiles", want_T=False)


def test_three_view_batch_equals_three_single_renders(G):
    cols = _random_cols(G)
    scene = G.renderer.GaussianScene.from_columns(cols)
    cams = [G.renderer.make_camera(*_ring_args(G, 64, 48, k)) for k in (4, 9, 17)]
    one = G.renderer.Rasterizer(scene)
    for kw in (dict(), dict(blend_impl=1)):
        single = torch.stack([one.render(c, G.renderer.make_options(**kw)).clone() for c in cams])
        eager = torch.stack([one.render(c, G.renderer.make_options(colour_stage=1, **kw)).clone() for c in cams])
        batch = G.renderer.Rasterizer(scene, views=3).render_batch(cams, G.renderer.make_options(**kw))
        assert torch.equal(batch, single) and torch.equal(batch, eager), kw


# ---- scenes built in pixels -------------------------------------------------------------------------------------------------------

def _pixel_camera_args(W, H):
    f = W / (2.0 * math.tan(math.radians(60.0) / 2.0))
    return (np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3), 2.0 * f, 2.0 * f, 2 * W, 2 * H, W, H), f


def _pixel_cols(W, H, rows):
    """rows: (px, py, z, su, sv, theta, opacity, dc) — a flat gaussian (tiny z scale) at depth z whose screen mean is the pixel
    (px, py) and whose 2-D covariance is R(theta) diag(su^2, sv^2) R(theta)^T + 0.3 I in pixels; colour 0.28 dc + 0.5 per channel."""
    _, f = _pixel_camera_args(W, H)
    a = np.asarray(rows, np.float64)
    px, py, z, su, sv, th, op = (a[:, k] for k in range(7))
    dc = a[:, 7:10]
    n = len(a)
    cols = {"x": ((px + 0.5 - 0.5 * W) * z / f), "y": ((py + 0.5 - 0.5 * H) * z / f), "z": z,
            "scale_0": np.log(su * z / f), "scale_1": np.log(sv * z / f), "scale_2": np.log(1e-4 * np.minimum(su, sv) * z / f),
            "rot_0": np.cos(0.5 * th), "rot_1": np.zeros(n), "rot_2": np.zeros(n), "rot_3": np.sin(0.5 * th),
            "opacity": np.log(op) - np.log1p(-op)}
    for c in range(3):
        cols[f"f_dc_{c}"] = dc[:, c]
    for c in range(45):
        cols[f"f_rest_{c}"] = np.zeros(n)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in cols.items()}


def _touched(G, pre, idx, W, H):
    """[H, W] bool: the pixels some gaussian of `idx` contributes to, by the oracle's own per-pixel loop."""
    if len(idx) == 0:
        return np.zeros((H, W), bool)
    _, trans, _ = G.orc.composite(np.asarray(idx, np.int64), pre, W, H)
    return (trans != 1.0).T


FRONT_LAYERS, N_A, N_B, N_C = 11, 300, 40, 100


def _hidden_scene(rng):
    """32x32, tile (0, 0).  Front: FRONT_LAYERS layers of 48 opaque gaussians on a 2-px grid over the quadrants 0, 1, 2 of the tile
    (x < 16, y < 8 and x < 8, 8 <= y < 16), nearest first.  Behind them, shuffled in depth: N_A small gaussians in the middle of
    those three quadrants, N_B in the middle of quadrant 3, and N_C needles along the line x + y = -6, outside the frame, whose
    rect covers the tile."""
    rows, kind = [], []
    grid = [(x + 0.5, y + 0.5) for y in range(0, 8, 2) for x in range(0, 16, 2)] + [(x + 0.5, y + 0.5) for y in range(8, 16, 2) for x in range(0, 8, 2)]
    assert len(grid) == 48
    z = 1.0
    for _ in range(FRONT_LAYERS):
        for (x, y) in grid:
            z += 1e-3
            rows.append((x, y, z, 1.7, 1.5, 0.4, 0.9997, *rng.uniform(0.3, 1.2, 3)))
            kind.append("front")
    zs = iter(rng.permutation(np.linspace(2.0, 3.0, N_A + N_B + N_C)))
    for k in range(N_A):
        x, y = ((3.5, 3.5), (11.5, 3.5), (3.5, 11.5))[k % 3]
        rows.append((x, y, next(zs), 0.8, 0.6, 0.5, 0.5, *rng.uniform(0.3, 1.2, 3)))
        kind.append("a")
    for _ in range(N_B):
        rows.append((11.5, 11.5, next(zs), 0.8, 0.6, 0.5, 0.3, *rng.uniform(0.3, 1.2, 3)))
        kind.append("b")
    for _ in range(N_C):
        rows.append((-3.0, -3.0, next(zs), 6.0, 0.05, -0.25 * math.pi, 0.9, *rng.uniform(0.3, 1.2, 3)))
        kind.append("c")
    return _pixel_cols(32, 32, rows), np.asarray(kind)


def test_a_colour_nobody_needs_is_not_evaluated(G):
    """Tile (0, 0) of a 32x32 frame: its first two batches (256 entries each: the plain kernel and both one-quadrant walks stage 256)
    are front layer and finish three quadrants by the exact rule; from the third batch on, an entry over those quadrants alone, or
    over no pixel at all, keeps its colour pending.
    Measured (MI355X): see the assertion messages; the bounds below are the construction's, not the measurement's."""
    W = H = 32
    cols, kind = _hidden_scene(np.random.default_rng(5))
    front, n = int((kind == "front").sum()), len(kind)
    assert front == 48 * FRONT_LAYERS and front > 512
    args, _ = _pixel_camera_args(W, H)
    ocam = G.orc.camera(*args)
    packed = G.utils.pack_gaussians(cols)

    # -- the construction, on the CPU
    pre = G.orc.preprocess(packed, ocam)
    order = G.orc.depth_order(pre["cam_means"])
    assert (kind[order[:front]] == "front").all()                      # the front layer is in front
    tb = pre["tile_bboxes"]
    in_tile0 = (tb[:, 0] <= 0) & (tb[:, 2] >= 1) & (tb[:, 1] <= 0) & (tb[:, 3] >= 1)
    assert in_tile0.all()                                              # every rect covers tile (0, 0): its list is the depth order
    tiles = (tb[:, 2] - tb[:, 0]) * (tb[:, 3] - tb[:, 1])
    assert (tiles[kind != "front"] == 1).all()                         # ... and what is hidden is in no other tile's list
    slack = int((tiles[kind == "front"] - 1).sum())                    # racing duplicates: a front gaussian once per further tile
    screen, trans, drawn = G.orc.composite(order, pre, W, H, limit=512)
    assert drawn == 512
    T512, C512 = trans.T.astype(np.float64), screen.transpose(1, 0, 2).astype(np.float64).min(axis=2)
    q012 = np.zeros((H, W), bool)
    q012[:8, :16] = True
    q012[8:16, :8] = True
    q3 = np.zeros((H, W), bool)
    q3[8:16, 8:16] = True
    assert C512[q012].min() > 2.0 ** -100 and (T512[q012] <= 2.0 ** -27 * C512[q012]).all()   # pixel_finished, with a factor 4 to spare
    final = G.orc.composite(order, pre, W, H)[1].T
    assert final[q3].max() > 0.5                                       # quadrant 3 never finishes
    ta = _touched(G, pre, np.nonzero(kind == "a")[0], W, H)
    assert ta.any() and not (ta & ~q012).any()                         # n_a: over the finished quadrants alone
    tb_ = _touched(G, pre, np.nonzero(kind == "b")[0], W, H)
    assert tb_.any() and not (tb_ & ~q3).any()                         # n_b: over the live one alone
    assert not _touched(G, pre, np.nonzero(kind == "c")[0], W, H).any()  # n_c: over no pixel

    # -- the needles are listed and staged, and nobody evaluates them (one gaussian of n_b with them: an empty frame stages nothing):
    #    both one-quadrant walks, the plain kernel and its bf16-accumulator instantiation
    sel = np.concatenate([np.nonzero(kind == "c")[0], np.nonzero(kind == "b")[0][:1]])
    Rn = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed({k: v[sel] for k, v in packed.items()}))
    cam = G.renderer.make_camera(*args)
    for kw in (dict(), dict(blend_pipe_tiles=-1), dict(blend_impl=1), dict(accum_bf16=True)):
        img = Rn.render(cam, G.renderer.make_options(**kw)).clone()
        st = dict(Rn.last_stats)
        print("needles + 1:", kw, st)
        assert st["fetched_entries"] == N_C + 1 and st["colour_evals"] == 1, (kw, st)
        assert torch.equal(img, Rn.render(cam, G.renderer.make_options(colour_stage=1, **kw))), kw

    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(packed))
    eager = R.render(cam, G.renderer.make_options(colour_stage=1)).clone()
    for kw in (dict(), dict(blend_pipe_tiles=-1), dict(blend_impl=1)):
        img = R.render(cam, G.renderer.make_options(**kw))
        ev = R.last_stats["colour_evals"]
        print(kw, "colour_evals", ev, "front", front, "n_a", N_A, "n_b", N_B, "n_c", N_C, "slack", slack, "fetched", R.last_stats["fetched_entries"])
        assert torch.equal(img, eager), kw
        assert R.last_stats["fetched_entries"] >= n, kw                # tile (0, 0) stages its whole list: quadrant 3 stays live
        assert ev <= front + N_B + slack, f"{kw}: {ev} colours evaluated > front {front} + n_b {N_B} + slack {slack} (racing duplicates)"
        assert ev < front + N_A + N_B + N_C, (kw, ev)
    # bf16 accumulators (ColourBlend<true>) stage through the same next_batch: its own frames, colour_stage 0 == 1
    o = G.renderer.make_options
    assert torch.equal(R.render(cam, o(accum_bf16=True)).clone(), R.render(cam, o(accum_bf16=True, colour_stage=1)))
    assert R.last_stats["colour_evals"] == 0


def test_a_pending_colour_survives_for_the_tile_that_needs_it(G):
    """32x16, tiles X = (0, 0) and Y = (1, 0).  One oblique needle through (21, 2) along x - y = 19: its rect covers both tiles, its
    visible pixels lie in Y alone (every pixel of X is >= 2.8 px = 4.5 sigma from the line).  X stages it, needs no colour and
    leaves the record pending; Y evaluates it, whichever tile comes first.  X also holds 200 gaussians of its own, so it is
    launched first (longest list first)."""
    W, H = 32, 16
    rng = np.random.default_rng(8)
    rows = [(21.0, 2.0, 1.5, 8.0, 0.3, 0.25 * math.pi, 0.9, 1.0, 0.2, -0.5)]
    for k in range(200):
        rows.append((4.5 + (k % 3), 5.5 + (k % 2), 2.0 + 1e-3 * k, 0.9, 0.7, 0.3, 0.05, *rng.uniform(0.3, 1.2, 3)))
    cols = _pixel_cols(W, H, rows)
    args, _ = _pixel_camera_args(W, H)
    packed = G.utils.pack_gaussians(cols)
    pre = G.orc.preprocess(packed, G.orc.camera(*args))
    tb = pre["tile_bboxes"]
    assert tb[0, 0] == 0 and tb[0, 2] >= 2 and (tb[1:, 2] == 1).all()  # the needle's rect: both tiles; the rest: X alone
    t0 = _touched(G, pre, [0], W, H)
    assert t0[:, 16:].sum() >= 8 and not t0[:, :16].any()               # visible in Y alone
    cam = G.renderer.make_camera(*args)
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(packed))
    eager = R.render(cam, G.renderer.make_options(colour_stage=1)).clone()
    oimg, _ = G.orc.render(packed, G.orc.camera(*args))
    for kw in (dict(), dict(blend_pipe_tiles=-1), dict(blend_impl=1), dict(no_order_hint=True)):
        img = R.render(cam, G.renderer.make_options(**kw))
        assert torch.equal(img, eager), kw
        assert R.last_stats["fetched_entries"] == 202, kw             # staged by X (with its 200) and by Y
        assert R.last_stats["colour_evals"] == 201, kw                # ... evaluated by Y alone: never twice
        y = img[:, 16:].cpu().numpy()
        assert y[..., 0].max() > 0.3 and abs(float(y[..., 0].max()) - float(oimg[:, 16:, 0].max())) < 5e-3   # its own colour (red 0.78, blue 0.36), as bright as the oracle's
        assert y[..., 0].max() > 1.5 * y[..., 2].max()


def test_repeated_blend_on_one_preprocess_renders_the_same_frame(G):
    """gsr_blend twice on one gsr_preprocess + gsr_bin_sort: the records the first blend left pending are still nobody's need in the
    second, and those it evaluated are found evaluated."""
    lib, check = G.lib.lib, G.lib.check
    W = H = 32
    cols, _ = _hidden_scene(np.random.default_rng(5))
    cases = [("hidden", G.utils.pack_gaussians(cols), _pixel_camera_args(W, H)[0]),
             ("random", G.utils.pack_gaussians(_random_cols(G)), _ring_args(G, 64, 48, 4))]
    for name, packed, args in cases:
        cam = G.renderer.make_camera(*args)
        scene = G.renderer.GaussianScene.from_packed(packed)
        R = G.renderer.Rasterizer(scene)
        eager = R.render(cam, G.renderer.make_options(colour_stage=1)).clone()
        ws = R._workspace(cam.width, cam.height)
        sc = scene.c_struct()
        sp = int(torch.cuda.current_stream().cuda_stream)
        for impl in (0, 1):
            o = R.bounded(G.renderer.make_options(blend_impl=impl))
            check(lib.gsr_preprocess(C.byref(sc), C.byref(cam), C.byref(o), ws.data_ptr(), ws.numel(), None, sp))
            check(lib.gsr_bin_sort(scene.n, C.byref(cam), C.byref(o), R.max_pairs, ws.data_ptr(), ws.numel(), sp))
            outs, evs = [], []
            for _ in range(3):
                out = torch.zeros((cam.height, cam.width, 3), dtype=torch.float32, device="cuda")
                check(lib.gsr_blend(None, scene.n, C.byref(cam), C.byref(o), R.max_pairs, ws.data_ptr(), ws.numel(), out.data_ptr(), None, sp))
                evs.append(R.stats()["colour_evals"])
                outs.append(out)
            print(name, "impl", impl, "colour_evals of three blends:", evs)
            assert all(torch.equal(x, eager) for x in outs), (name, impl)
            assert evs[0] > 0 and evs[1] == 0 and evs[2] == 0, (name, impl, evs)
