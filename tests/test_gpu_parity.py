"""GPU: the HIP path (through the C ABI) against the CPU oracle and the reference's golden frames.

Tolerances (north_star: PSNR >= 50 dB vs the torch reference): we hold the HIP frames to >= 100 dB against
both the reference's own frames and the oracle, max-abs error < 1e-4, integer outputs (tile / pixel rects,
skip decisions) bit-exact on the fixtures.
"""
import numpy as np
import pytest
import torch

from conftest import assert_frames_close, golden_columns, load_golden, psnr
from gpu_cases import (assert_preprocess_matches, assert_same_camera, f5_case, fuzz_case, golden_cameras as _cams,
                       medium_cameras as _medium, namespace)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    return namespace()


def _rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def test_camera_setup_matches_oracle(G):
    g = load_golden("f1_unit.npz")
    assert_same_camera(*_cams(G, g))


@pytest.mark.parametrize("name,prefix", [("f1_unit.npz", ""), ("f3_edge.npz", "a_"), ("f3_edge.npz", "b_")])
def test_preprocess_intermediates(G, name, prefix):
    g = load_golden(name)
    cols = golden_columns(g)
    cam, ocam = _cams(G, g, prefix)
    scene = G.renderer.GaussianScene.from_columns(cols)
    dbg = {k: v.cpu().numpy() for k, v in G.renderer.Rasterizer(scene).preprocess_debug(cam).items()}
    pre = G.orc.preprocess(G.utils.pack_gaussians(cols), ocam)
    # integer outputs: bit-exact against the oracle AND the reference
    assert_preprocess_matches(dbg, pre)
    assert np.array_equal(dbg["pixel_bboxes"], g[prefix + "pixel_bboxes"])
    assert _rel(dbg["rgb"], g[prefix + "rgb"]) < 1e-6


@pytest.mark.parametrize("name,prefix", [("f1_unit.npz", ""), ("f2_small.npz", ""), ("f3_edge.npz", "a_"), ("f3_edge.npz", "b_")])
def test_frame_matches_reference_and_oracle(G, name, prefix):
    g = load_golden(name)
    cols = golden_columns(g)
    cam, ocam = _cams(G, g, prefix)
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols))
    img, T = R.render(cam, return_T=True)
    img, T = img.cpu().numpy(), T.cpu().numpy()
    ref = g[prefix + "image"]
    oimg, oT, drawn = G.orc.render(G.utils.pack_gaussians(cols), ocam, want_T=True)
    assert psnr(img, ref) >= 100.0, psnr(img, ref)
    assert psnr(img, oimg) >= 100.0
    assert np.abs(img - oimg).max() < 1e-4
    assert np.abs(T - oT).max() < 1e-4
    assert not img[-1].any() and not img[:, -1].any()           # Q1
    assert (T[-1] == 1).all() and (T[:, -1] == 1).all()
    assert R.last_stats["n_visible"] <= drawn                    # footprint culling only ever drops gaussians


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_sh_degrees_vs_oracle(G, degree):
    g = load_golden("f2_small.npz")
    cols = golden_columns(g)
    cam, ocam = _cams(G, g)
    img = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols, sh_degree=degree)).render(cam).cpu().numpy()
    oimg, _ = G.orc.render(G.utils.pack_gaussians(cols), ocam, sh_degree=degree)
    assert_frames_close(img, oimg)
    if degree == 3:
        assert psnr(img, g["image"]) >= 100.0


def test_fp16_sh_storage(G):
    """BASELINE configs[2]: SH coefficients stored as fp16 (evaluated in fp32).  == rendering the fp16-rounded
    coefficients exactly, and >= 75 dB from the fp32-coefficient frame (SURVEY measured 91 dB on its scene)."""
    cols, cam, ocam = _medium(G)
    full = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols)).render(cam).cpu().numpy()
    half = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols, sh_half=True)).render(cam).cpu().numpy()
    packed = G.utils.pack_gaussians(cols)
    packed["sh"] = packed["sh"].astype(np.float16).astype(np.float32)
    rounded = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(packed)).render(cam).cpu().numpy()
    assert np.array_equal(half, rounded)
    assert psnr(half, full) >= 75.0, psnr(half, full)


def test_degenerate_inputs(G):
    """n = 0, a frame smaller than one tile, everything culled, a single gaussian."""
    p = G.synthetic.look_at_pose((0, -4, 0.5), (0, 0, 0), 1, "x.png")
    for (W, H) in ((10, 7), (16, 16), (33, 17)):
        fx = G.synthetic.pinhole_focal(W)
        args = (p.qvec, p.tvec, 2 * fx, 2 * fx, 2 * W, 2 * H, W, H)
        cam, ocam = G.renderer.make_camera(*args), G.orc.camera(*args)
        for n in (0, 1, 300):
            cols = G.synthetic.mip360_like(max(n, 1), 3)
            for i in range(3):
                cols[f"scale_{i}"] = (cols[f"scale_{i}"] + np.float32(3.0)).astype(np.float32)
            cols = {k: v[:n] for k, v in cols.items()}
            packed = G.utils.pack_gaussians(cols)
            R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(packed))
            img, T = R.render(cam, return_T=True)
            oimg, oT, _ = G.orc.render(packed, ocam, want_T=True) if n else (np.zeros((H, W, 3), np.float32), np.ones((H, W), np.float32), 0)
            assert_frames_close(img.cpu().numpy(), oimg)
            assert np.abs(T.cpu().numpy() - oT).max() < 1e-5
    # every gaussian behind the camera
    cols = G.synthetic.mip360_like(500, 4)
    cols["y"] = (cols["y"] - np.float32(100.0)).astype(np.float32)  # camera at y = -4 looks along +y
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols))
    assert not R.render(cam).any() and R.last_stats["n_visible"] == 0 and R.last_stats["n_pairs"] == 0


def test_multi_camera_batch(G):
    """several views of the resident scene in one call == the views rendered one by one."""
    cols, cam0, _ = _medium(G, n=60_000)
    W, H = cam0.width, cam0.height
    fx = G.synthetic.pinhole_focal(W)
    cams = [G.renderer.make_camera(p.qvec, p.tvec, 2 * fx, 2 * fx, 2 * W, 2 * H, W, H) for p in G.synthetic.ring_cameras(25)[::5]]
    scene = G.renderer.GaussianScene.from_columns(cols)
    singles = torch.stack([G.renderer.Rasterizer(scene).render(c) for c in cams])
    R = G.renderer.Rasterizer(scene, max_pairs=2048)               # too small: an overflow in ANY view must be caught
    batch = R.render_batch(cams)
    assert R.max_pairs > 2048 and torch.equal(batch, singles)
    assert not torch.equal(singles[0], singles[1])


def test_views_per_launch_sequence_render_the_single_view_frames(G):
    """gsr_render_batch with a workspace of K slices: K views through ONE preprocess / sort / blend launch sequence (ABI 0.6.0).  The
    same kernels on the same per-view values, so every frame must equal the single-view render bit for bit: K = 2, 3, 4, 8, batches
    that do not fill their last group, GsrOptions.batch_views capping K, the overflow and depth-sort-bound recovery (the worst view
    decides), colours in the preprocess, fp16 SH, fine binning, bf16 store, shards through both preprocess kernels, frames in flight."""
    cols, cam0, _ = _medium(G, n=60_000)
    W, H = cam0.width, cam0.height
    fx = G.synthetic.pinhole_focal(W)
    mk = G.renderer.make_options
    cams = [G.renderer.make_camera(p.qvec, p.tvec, 2 * fx, 2 * fx, 2 * W, 2 * H, W, H) for p in G.synthetic.ring_cameras(25)[::3]]  # 9 views
    scene = G.renderer.GaussianScene.from_columns(cols)
    ref = G.renderer.Rasterizer(scene)
    singles = torch.stack([ref.render(c) for c in cams])
    need = ref.max_pairs
    for K in (2, 3, 4, 8):
        R = G.renderer.Rasterizer(scene, views=K)
        assert torch.equal(R.render_batch(cams), singles), K
        assert len(R.last_slice_stats) == min(K, len(cams))
        # the counters of slice j are those of the last view it rendered: views j, j + K, ...
        for j, st in enumerate(R.last_slice_stats):
            last = max(i for i in range(len(cams)) if i % K == j)
            ref.render(cams[last])
            for k in ("n_visible", "n_pairs_bbox", "n_pairs", "sort_passes", "max_list_len"):  # (what the blend stages depends on its batch size)
                assert st[k] == ref.last_stats[k], (K, j, k)
        assert torch.equal(R.render_batch(cams[:K - 1]), singles[:K - 1])            # fewer views than slices
        assert torch.equal(R.render_batch(cams, mk(batch_views=2)), singles)          # the option caps K
        assert torch.equal(R.render(cams[1]), singles[1])                             # single frames on slice 0 of the same workspace
    R = G.renderer.Rasterizer(scene, max_pairs=2048, views=4)                          # too small: an overflow in ANY view of ANY group must be caught
    assert torch.equal(R.render_batch(cams), singles) and R.max_pairs > 2048
    R = G.renderer.Rasterizer(scene, views=4)
    R.sort_passes = 1                                                                 # a learned bound that is too small for these views
    assert torch.equal(R.render_batch(cams), singles) and R.sort_passes >= 2
    for kw in (dict(colour_stage=1), dict(fine_binning=True), dict(output_bf16=True), dict(blend_impl=1), dict(reference_compat=False),
               dict(saturation_rule=1), dict(no_footprint_cull=True), dict(draw_limit=5000)):
        one = torch.stack([ref.render(c, mk(**kw)) for c in cams[:5]])
        assert torch.equal(G.renderer.Rasterizer(scene, views=4).render_batch(cams[:5], mk(**kw)), one), kw
    half = G.renderer.GaussianScene.from_columns(cols, sh_half=True)
    one = torch.stack([G.renderer.Rasterizer(half).render(c) for c in cams[:5]])
    assert torch.equal(G.renderer.Rasterizer(half, views=4).render_batch(cams[:5]), one)
    assert torch.equal(G.renderer.Rasterizer(half, views=4).render_batch(cams[:5], mk(colour_stage=1)), one)
    # tile-row shards (a multi-GPU rank's frames): strips [B, rows * 16, W, 3]; step 2 goes through the whole-frame preprocess kernel,
    # step 8 through the three-phase one
    for begin, step in ((1, 2), (3, 8), (0, 5)):
        o = mk(tile_row_begin=begin, tile_row_step=step, output_layout=2)
        strips = torch.stack([ref.render(c, o) for c in cams])
        R = G.renderer.Rasterizer(scene, views=4)
        assert torch.equal(R.render_batch(cams, o), strips), (begin, step)
    # frames in flight: each slot takes `views` consecutive cameras per launch sequence
    fif = G.renderer.FramesInFlight(scene, slots=2, max_pairs=need, views=4)
    assert torch.equal(fif.render_batch(cams), singles)
    outs = torch.empty((2, 4, H, W, 3), device="cuda")
    for rnd in range(2):
        for g in range(2):
            fif.submit_batch(cams[4 * g: 4 * g + 4], ref.bounded(mk()), out=outs[g])
    fif.synchronize()
    for g in range(2):
        fif.stats(g)
    assert torch.equal(outs.view(8, H, W, 3), singles[:8])
    small = G.renderer.FramesInFlight(scene, slots=2, max_pairs=2048, views=3)
    assert torch.equal(small.render_batch(cams), singles) and small.rasterizers[0].max_pairs > 2048


def test_block_culling_is_exact(G):
    """GsrScene.block_bounds (gsr_scene_bounds; the loaders build them): the preprocess skips, unread, every block of 64 consecutive
    gaussians that its camera-independent box proves undrawable in a view (cull plane rasterize.py:377, frame, this rank's tile rows).
    (1) Conservative against the reference-parity intermediates: no gaussian of a skipped block passes the reference's skip guard
    (rasterize.py:441: bbox area > 0, all conic entries != 0) — Morton and file order, several cameras, whole frames and every rank
    of 2 / 5 / 8 shards (there: no gaussian of a skipped block has one of the rank's tile rows in its rect).
    (2) The frame with bounds == the frame without, bit for bit: whole frames, shards through both preprocess kernels, batches of
    views, progressive prefixes, culling off, non-compat, colours in the preprocess.  (3) It skips something (this scene's gaussians are
    inflated 3.3x; the 6 M-gaussian bench scene: tools/block_cull_stats.py)."""
    mk = G.renderer.make_options
    cols, cam0, _ = _medium(G, n=200_000)
    W, H = cam0.width, cam0.height
    fx = G.synthetic.pinhole_focal(W)
    cams = [G.renderer.make_camera(p.qvec, p.tvec, 2 * fx, 2 * fx, 2 * W, 2 * H, W, H) for p in G.synthetic.ring_cameras(25)[::6]]
    # a camera inside the cloud looking outwards (blocks behind the cull plane, blocks straddling it) and one far away (tiny frame footprint)
    pz = G.synthetic.ring_cameras(25)[3]
    cams.append(G.renderer.make_camera(pz.qvec, np.asarray(pz.tvec) * 0.05, 2 * fx, 2 * fx, 2 * W, 2 * H, W, H))
    cams.append(G.renderer.make_camera(pz.qvec, np.asarray(pz.tvec) * 6.0, 2 * fx, 2 * fx, 2 * W, 2 * H, W, H))
    for spatial in (True, False):
        scene = G.renderer.GaussianScene.from_columns(cols, spatial_order=spatial)
        assert (scene.bounds is not None) == spatial   # the loaders build bounds with the spatial order
        scene.build_bounds()
        assert scene.bounds.shape == ((scene.n + 63) // 64, 8)
        bare = G.renderer.GaussianScene({k: scene.t[k] for k in scene.FIELDS})  # the same arrays, no bounds
        bare.order_t = scene.order_t
        R, Rb = G.renderer.Rasterizer(scene), G.renderer.Rasterizer(bare)
        skipped = []
        for cam in cams:
            dbg = R.preprocess_debug(cam)   # file order; the debug kernels never skip
            pb, sg, z = dbg["pixel_bboxes"], dbg["sigmas"], dbg["cam_means"][:, 2]
            drawn = (z >= 0.2) & ((pb[:, 2] - pb[:, 0]) > 0) & ((pb[:, 3] - pb[:, 1]) > 0) & (sg != 0).all(dim=1)   # rasterize.py:377,:441
            tb = dbg["tile_bboxes"]
            if scene.order_t is not None:
                drawn, tb = drawn[scene.order_t], tb[scene.order_t]
            pad = (-scene.n) % 64
            blocks = lambda m: torch.nn.functional.pad(m, (0, pad)).view(-1, 64)
            dead = scene.blocks_skipped(cam).bool()
            assert not (blocks(drawn) & dead[:, None]).any(), "a skipped block holds a gaussian the reference draws"
            skipped.append(float(dead.float().mean()))
            for step in (2, 5, 8):
                for begin in range(step):
                    o = mk(tile_row_begin=begin, tile_row_step=step, output_layout=2)
                    dead_r = scene.blocks_skipped(cam, o).bool()
                    # tile rows of the reference rect (an upper bound of the rows the refined rect keeps): [tb1, tb3) in tile units
                    rows = torch.arange((H + 15) // 16, device=tb.device)
                    mine = ((rows - begin) % step == 0)[None, :] & (rows[None, :] >= tb[:, 1:2]) & (rows[None, :] < tb[:, 3:4])
                    reach = drawn & mine.any(dim=1)
                    assert not (blocks(reach) & dead_r[:, None]).any(), (step, begin)
                    assert (dead_r | ~dead).all()   # a rank skips at least what the whole frame skips
            assert torch.equal(R.render(cam), Rb.render(cam))
            for kw in (dict(tile_row_begin=1, tile_row_step=2, output_layout=2), dict(tile_row_begin=3, tile_row_step=8, output_layout=2),
                       dict(tile_row_begin=0, tile_row_step=5, output_layout=2), dict(draw_limit=3000), dict(draw_limit=3000, tile_row_begin=1, tile_row_step=2, output_layout=2),
                       dict(no_footprint_cull=True), dict(reference_compat=False), dict(colour_stage=1)):
                assert torch.equal(R.render(cam, mk(**kw)), Rb.render(cam, mk(**kw))), kw
            assert R.last_stats["n_visible"] == Rb.last_stats["n_visible"]
        R4, Rb4 = G.renderer.Rasterizer(scene, views=4), G.renderer.Rasterizer(bare, views=4)
        assert torch.equal(R4.render_batch(cams), Rb4.render_batch(cams))
        o8 = mk(tile_row_begin=5, tile_row_step=8, output_layout=2)
        assert torch.equal(R4.render_batch(cams, o8), Rb4.render_batch(cams, o8))
        print(f"\n{'morton' if spatial else 'file'} order: blocks skipped per view " + " ".join(f"{x:.2f}" for x in skipped))
        if spatial:
            assert max(skipped) > 0.2 and sum(skipped) / len(skipped) > 0.08, skipped
    # an unbounded box (a non-finite mean) is never skipped; the frame is unchanged
    bad = {k: v.copy() for k, v in cols.items()}
    bad["x"][1000] = np.inf
    sb = G.renderer.GaussianScene.from_columns(bad, spatial_order=False).build_bounds()
    assert torch.isinf(sb.bounds[1000 // 64, 3]) and not sb.blocks_skipped(cams[0])[1000 // 64]


def test_frames_in_flight_are_bit_identical_to_single_stream(G):
    """renderer.FramesInFlight / gsr_render_batch_slots: independent frames on separate HIP streams, one workspace each
    (bench.py's throughput mode).  Same kernels on the same inputs, so every frame must equal the single-stream render bit
    for bit — whole frames and shards, submit() and the batch entry point, including its overflow recovery."""
    cols, cam0, _ = _medium(G, n=60_000)
    W, H = cam0.width, cam0.height
    fx = G.synthetic.pinhole_focal(W)
    cams = [G.renderer.make_camera(p.qvec, p.tvec, 2 * fx, 2 * fx, 2 * W, 2 * H, W, H) for p in G.synthetic.ring_cameras(25)[::3]]
    scene = G.renderer.GaussianScene.from_columns(cols)
    ref = G.renderer.Rasterizer(scene)
    singles = torch.stack([ref.render(c) for c in cams])
    fif = G.renderer.FramesInFlight(scene, slots=3, max_pairs=ref.max_pairs)
    outs = [torch.empty((H, W, 3), device="cuda") for _ in cams]
    for _ in range(2):                                   # twice: every slot's workspace is reused
        for c, o in zip(cams, outs):
            fif.submit(c, out=o)
    fif.synchronize()
    assert torch.equal(torch.stack(outs), singles)
    assert torch.equal(fif.render_batch(cams), singles)
    small = G.renderer.FramesInFlight(scene, slots=2, max_pairs=2048)   # too small: an overflow in ANY slot must be caught
    assert torch.equal(small.render_batch(cams), singles) and small.rasterizers[0].max_pairs > 2048
    # shards (the multi-GPU ranks' mode), 8 rows apart: the three-phase shard preprocess on every slot
    mk = G.renderer.make_options
    o8 = mk(tile_row_begin=3, tile_row_step=8, output_layout=2)
    strip = ref.render(cams[1], o8)
    strips = [torch.zeros_like(strip) for _ in range(4)]
    for s_ in strips:
        fif.submit(cams[1], o8, out=s_)
    fif.synchronize()
    assert all(torch.equal(s_, strip) for s_ in strips) and strip.any()
    lib = G.renderer.lib
    import ctypes as C
    sc = scene.c_struct()
    arr = (G.renderer.GsrCamera * 2)(cams[0], cams[1])
    ws = fif.rasterizers[0]._workspace(W, H)
    out = torch.empty((2, H, W, 3), device="cuda")
    two = (C.c_void_p * 2)(ws.data_ptr(), ws.data_ptr())
    st = (C.c_void_p * 2)(0, 0)
    assert lib.gsr_render_batch_slots(C.byref(sc), arr, 2, C.byref(mk()), fif.rasterizers[0].max_pairs, two, ws.numel(), st, 2,
                                      out.data_ptr(), H * W * 3) != 0 and b"share a workspace" in lib.gsr_last_error()


@pytest.mark.parametrize("name,prefix", [("f2_small.npz", ""), ("f3_edge.npz", "a_")])
def test_progressive_render_matches_reference_draw_order(G, name, prefix):
    """draw_limit = k blends exactly the first k gaussians of the reference's draw order (rasterize.py:440-450):
    checked against the oracle's loop stopped after k drawn gaussians, k spanning the whole order."""
    g = load_golden(name)
    cols = golden_columns(g)
    cam, ocam = _cams(G, g, prefix)
    packed = G.utils.pack_gaussians(cols)
    pre = G.orc.preprocess(packed, ocam)
    order = G.orc.depth_order(pre["cam_means"])
    n_drawn = len(g[prefix + "draw_order"])
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols))
    full = R.render(cam)
    for k in (1, 2, 7, n_drawn // 3, n_drawn - 1, n_drawn, n_drawn + 50):
        img = R.render(cam, G.renderer.make_options(draw_limit=k)).cpu().numpy()
        screen, _, drawn = G.orc.composite(order, pre, cam.width, cam.height, limit=k)
        assert drawn == min(k, n_drawn)
        assert_frames_close(img, screen.transpose(1, 0, 2))
        assert R.last_stats["n_visible"] == n_drawn                # the sort keeps every gaussian the reference draws
    assert torch.equal(R.render(cam, G.renderer.make_options(draw_limit=n_drawn)), full)


def test_very_wide_frame_uses_the_gathered_rect_path(G):
    """More than 256 tiles per row: the tile rect no longer fits the packed 4 x u8 sort payload and is gathered by id."""
    W, H = 4200, 40
    cols = G.synthetic.mip360_like(40_000, 12)
    for i in range(3):
        cols[f"scale_{i}"] = (cols[f"scale_{i}"] + np.float32(1.0)).astype(np.float32)
    p = G.synthetic.look_at_pose((0.0, -2.0, 0.1), (0, 0, 0), 1, "w.png")   # close: the foreground blob spans the full width
    fx = G.synthetic.pinhole_focal(W, 100.0)
    args = (p.qvec, p.tvec, 2 * fx, 2 * fx, 2 * W, 2 * H, W, H)
    cam, ocam = G.renderer.make_camera(*args), G.orc.camera(*args)
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols))
    img = R.render(cam).cpu().numpy()
    oimg, _ = G.orc.render(G.utils.pack_gaussians(cols), ocam)
    assert R.last_stats["n_pairs"] > 1000 and img[:, 4100:].any()     # content beyond tile column 256
    assert_frames_close(img, oimg)


def test_reference_screen_layout(G):
    g = load_golden("f2_small.npz")
    cam, _ = _cams(G, g)
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(golden_columns(g)))
    a = R.render(cam)
    b = R.render(cam, G.renderer.make_options(output_layout=1))  # `screen` [W,H,3], rasterize.py:437
    assert torch.equal(a, b.permute(1, 0, 2))


def test_medium_scene_vs_oracle(G):
    cols, cam, ocam = _medium(G)
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols))
    img = R.render(cam).cpu().numpy()
    oimg, drawn = G.orc.render(G.utils.pack_gaussians(cols), ocam)
    st = R.last_stats
    assert 0 < st["n_visible"] <= drawn and st["n_visible"] < st["n_pairs"] and 0 < st["n_pairs_bbox"] and st["overflow"] == 0
    assert 0 < st["wave_entries"] <= 4 * st["fetched_entries"] and 0 < st["fetched_entries"] <= st["n_pairs"]
    assert_frames_close(img, oimg)


def test_odd_frame_size_vs_oracle(G):
    cols, cam, ocam = _medium(G, n=50_000, W=333, H=197, pose=9)
    img = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols)).render(cam).cpu().numpy()
    oimg, _ = G.orc.render(G.utils.pack_gaussians(cols), ocam)
    assert_frames_close(img, oimg)


def test_pair_overflow_is_reported_and_recovered(G):
    cols, cam, _ = _medium(G, n=50_000)
    scene = G.renderer.GaussianScene.from_columns(cols)
    good = G.renderer.Rasterizer(scene).render(cam)
    small = G.renderer.Rasterizer(scene, max_pairs=4096)
    small.enqueue(cam)
    with pytest.raises(Exception) as e:
        small.stats()
    assert "overflow" in str(e.value)
    # at most max_pairs pair slots were filled (each expands into at most four tile-list entries), and the need is reported
    assert small.last_stats["overflow"] == 1 and 0 < small.last_stats["n_pairs"] <= 4 * 4096 and 4096 < small.last_stats["n_pairs_bbox"]
    again = small.render(cam)                                    # grows max_pairs and re-renders
    assert small.max_pairs > 4096 and torch.equal(again, good)


def test_a_reported_overflow_is_not_reported_again(G):
    """Each slice of a workspace keeps its own overflow record.  A batch overflows in slice 2 and stats() reports it; a single
    frame (slice 0), then a batch that fits (slices 0-2, chained behind the single frame) must read clean — slice 2's record was
    reported already — and render the single-view frames bit for bit."""
    from gsr_amd import _lib

    cols, cam, _ = _medium(G, n=60_000)
    W, H = cam.width, cam.height
    fx = G.synthetic.pinhole_focal(W)
    far = [G.renderer.make_camera(p.qvec, np.asarray(p.tvec) * 6.0, 2 * fx, 2 * fx, 2 * W, 2 * H, W, H)   # the scene small in the frame
           for p in G.synthetic.ring_cameras(25)[::12]]
    scene = G.renderer.GaussianScene.from_columns(cols)
    ref = G.renderer.Rasterizer(scene)
    singles, needs = [], []
    for c in far + [cam]:
        singles.append(ref.render(c))
        needs.append(ref.last_stats["n_pairs_bbox"])
    assert max(needs[:3]) < needs[3], needs                     # few pairs in the far views, many in `cam`
    R = G.renderer.Rasterizer(scene, max_pairs=(max(needs[:3]) + needs[3]) // 2, views=3)
    R.enqueue_batch([far[0], far[1], cam])                      # slice 2 overflows
    with pytest.raises(_lib.GsrPairOverflow):
        R.stats()
    assert [st["overflow"] for st in R.last_slice_stats] == [0, 0, 1]
    R.enqueue(far[2])                                           # slice 0
    batch = R.enqueue_batch([far[1], far[2], far[0]])           # slices 0-2, chained behind the single frame
    assert R.stats()["overflow"] == 0 and len(R.last_slice_stats) == 3
    assert torch.equal(batch, torch.stack([singles[1], singles[2], singles[0]]))


def test_stats_after_an_empty_shard_checks_the_frames_before_it(G):
    """A shard that owns no tile row runs no kernel and its counters are zeros, but the frames enqueued before it are still
    unchecked: stats() must read them and raise their overflow."""
    from gsr_amd import _lib

    cols, cam, _ = _medium(G, n=30_000, W=200, H=40)             # three tile rows: of 8 ranks, rank 5 owns none
    scene = G.renderer.GaussianScene.from_columns(cols)
    empty = G.renderer.make_options(tile_row_begin=5, tile_row_step=8, output_layout=2)
    R = G.renderer.Rasterizer(scene, max_pairs=64)
    R.enqueue(cam)                                               # overflows, unchecked
    assert R.enqueue(cam, empty).numel() == 0
    with pytest.raises(_lib.GsrPairOverflow):
        R.stats()
    assert R.last_stats["n_pairs_bbox"] > 64
    assert not any(R.stats().values())                           # the empty shard's own counters
    ok = G.renderer.Rasterizer(scene)                            # behind frames that fit: zeros, in every slice read
    ok.enqueue(cam)
    ok.enqueue(cam, empty)
    assert not any(ok.stats().values()) and ok.last_slice_stats == [ok.last_stats]


def test_saturation_early_out_is_exact(G):
    """The T == 0.0f rule (saturation_rule = 1; also what runs whenever the final T is requested): early_out_T = 0 stops a wave
    when all its pixels have T == 0.0f; a negative threshold never stops.  An opaque wall in front of a long list makes the
    early-out fire; the frames must be identical."""
    cols, cam, _ = _medium(G, n=300_000, shift=1.6)
    cols["opacity"] = np.full_like(cols["opacity"], 6.0)        # sigmoid(6) = 0.9975 -> alpha capped at 0.99
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols))
    a, Ta = R.render(cam, return_T=True)
    early = R.last_stats["wave_entries"]
    b, Tb = R.render(cam, G.renderer.make_options(early_out_T=-1.0), return_T=True)
    assert torch.equal(a, b) and torch.equal(Ta, Tb)
    assert (Ta == 0).any() and early < R.last_stats["wave_entries"]
    everything = R.last_stats["wave_entries"]
    # the same three without the T output: blend everything (rule 1, never stops) == T underflow rule == colour-saturation rule
    c = R.render(cam, G.renderer.make_options(early_out_T=-1.0, saturation_rule=1))
    assert torch.equal(c, a) and R.last_stats["wave_entries"] == everything
    d = R.render(cam, G.renderer.make_options(saturation_rule=1))
    assert torch.equal(d, a) and R.last_stats["wave_entries"] == early
    e = R.render(cam)
    assert torch.equal(e, a) and R.last_stats["wave_entries"] < early
    print(f"\nopaque wall: evaluated (quadrant, entry) pairs: blend everything {everything}, T == 0 rule {early}, "
          f"colour rule {R.last_stats['wave_entries']}")


def _rule_cases(G):
    """(name, columns, camera): frames that exercise every blend kernel variant (two quadrants per wave from 3000 tiles, the
    pipelined one-quadrant walk up to 1280, the plain one-quadrant walk between) and the fixtures' edge cases."""
    out = [("medium 640x360", *_medium(G)[:2]), ("dense 640x360", *_medium(G, n=300_000, shift=1.6, pose=7)[:2]),
           ("960x540", *_medium(G, n=250_000, shift=1.4, W=960, H=540, pose=4)[:2]),
           ("1080p", *_medium(G, n=600_000, seed=360, shift=0.8, W=1920, H=1080, pose=0)[:2]),
           ("odd 333x197", *_medium(G, n=50_000, W=333, H=197, pose=9)[:2])]
    wall = _medium(G, n=300_000, shift=1.6)
    wall[0]["opacity"] = np.full_like(wall[0]["opacity"], 6.0)
    out.append(("opaque wall", wall[0], wall[1]))
    # colour sums in the denormal range (blend_args.h, pixel_finished): the nearest 30 % of an opaque wall have NO red at all (the
    # clamp of spherical_harmonics.py:71 leaves exactly 0), the rest a red of 1-3 x 2^-25 — so a pixel's red sum starts growing only
    # after T has decayed by dozens of orders of magnitude: on this frame ~40 000 pixels end with 0 < Cr < 1e-30, half of them denormal
    late, cam_l, ocam_l = _medium(G, n=300_000, shift=1.6)
    late["opacity"] = np.full_like(late["opacity"], 6.0)
    z = G.orc.preprocess(G.utils.pack_gaussians(late), ocam_l)["cam_means"][:, 2]
    near = z < np.quantile(z[z >= 0.2], 0.3)
    f = np.where(near, np.float32(-10.0), np.float32(-0.5 / 0.28209479177387814)).astype(np.float32)
    k = np.arange(len(z)) % 4 + 1
    for _ in range(4):
        f = np.where(~near & (k > 0), np.nextafter(f, np.float32(0), dtype=np.float32), f)
        k = k - 1
    late["f_dc_0"] = f
    for j in range(15):
        late[f"f_rest_{j}"] = np.zeros_like(late[f"f_rest_{j}"])
    out.append(("late red (denormal sums)", late, cam_l))
    for name, prefix in (("f2_small.npz", ""), ("f3_edge.npz", "a_"), ("f3_edge.npz", "b_")):
        g = load_golden(name)
        out.append((name + prefix, golden_columns(g), _cams(G, g, prefix)[0]))
    # f5: the deep-stack fuzz case (hundreds of semi-transparent layers per pixel), rebuilt from its seed like its own test does
    _, c = f5_case()
    out.append(("f5_deep_stack", c["packed"], G.renderer.make_camera(*c["args"])))
    return out


def test_colour_saturation_rule_is_exact(G):
    """GsrOptions.saturation_rule = 0 (default): a quadrant stops once T <= 2^-25 min(Cr, Cg, Cb) for all its pixels — every later
    C = fma(w, c, C) has w c <= T < ulp(C) / 2 and returns C (blend_args.h, pixel_finished).  Must be bit-identical to rule 1
    (stop at T == 0.0f) and to blending every entry: whole frames through all three walk kernels and the plain one, shards, the
    bf16 store, bf16 accumulators, non-compat, both layouts, culling off, fine binning, progressive prefixes.  And it must
    remove work wherever rule 1 did."""
    mk = G.renderer.make_options
    saved = []
    for name, cols, cam in _rule_cases(G):
        scene = G.renderer.GaussianScene.from_packed(cols) if "means" in cols else G.renderer.GaussianScene.from_columns(cols)
        R = G.renderer.Rasterizer(scene)
        every = R.render(cam, mk(early_out_T=-1.0, saturation_rule=1))
        n_every = R.last_stats["wave_entries"]
        for kw in (dict(), dict(blend_impl=1), dict(tile_row_begin=2, tile_row_step=5, output_layout=2), dict(tile_row_begin=1, tile_row_step=2, output_layout=2),
                   dict(output_bf16=True), dict(accum_bf16=True), dict(reference_compat=False), dict(output_layout=1),
                   dict(no_footprint_cull=True), dict(fine_binning=True), dict(draw_limit=997), dict(blend_pipe_tiles=-1),
                   dict(blend_pipe_tiles=1 << 30)):
            a = R.render(cam, mk(saturation_rule=1, **kw))
            n1 = R.last_stats["wave_entries"]
            b = R.render(cam, mk(**kw))
            n0 = R.last_stats["wave_entries"]
            assert torch.equal(a, b), (name, kw)
            assert n0 <= n1, (name, kw, n0, n1)
            if not kw:
                assert torch.equal(b, every) and n1 <= n_every, name
                saved.append((name, n_every, n1, n0))
                if name.startswith("late red"):  # the case is what it claims to be
                    r = b[..., 0]
                    assert int(((r > 0) & (r < 1e-30)).sum()) > 10_000 and int(((r > 0) & (r < 1.17e-38)).sum()) > 1000
    print()
    for name, n_every, n1, n0 in saved:
        print(f"{name:>22}: evaluated (quadrant, entry) pairs: everything {n_every}, T == 0 rule {n1}, colour rule {n0}")
    assert any(n0 < n1 for _, _, n1, n0 in saved)


def test_deferred_colour_is_exact(G):
    """GsrOptions.colour_stage = 0 (default): sh_to_rgb is evaluated when a tile first stages a gaussian (blend.hip, staged_q2) and
    remembered in its record; 1: for every visible gaussian in the preprocess (rounds 1-3).  Same code (gauss_math.h sh_eval_with),
    same operation order, contraction off in both translation units: frames must be bit-identical — every blend kernel variant,
    shards (whole-frame and three-phase preprocess), SH degrees 0-3, fp16 SH storage, the T output, batches."""
    mk = G.renderer.make_options
    for name, cols, cam in _rule_cases(G):
        packed = cols if "means" in cols else G.utils.pack_gaussians(cols)
        for sh_kw in (dict(), dict(sh_degree=0), dict(sh_degree=2), dict(sh_half=True)):
            if sh_kw and name not in ("medium 640x360", "960x540", "f2_small.npz"):
                continue
            R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(packed, **sh_kw))
            for kw in (dict(), dict(blend_impl=1), dict(tile_row_begin=2, tile_row_step=5, output_layout=2), dict(tile_row_begin=1, tile_row_step=2, output_layout=2),
                       dict(saturation_rule=1), dict(fine_binning=True), dict(draw_limit=997), dict(blend_pipe_tiles=-1), dict(accum_bf16=True)):
                a, Ta = R.render(cam, mk(colour_stage=1, **kw), return_T=True)
                assert R.last_stats["colour_evals"] == 0, (name, sh_kw, kw)
                b, Tb = R.render(cam, mk(**kw), return_T=True)
                assert torch.equal(a, b) and torch.equal(Ta, Tb), (name, sh_kw, kw)
                # a gaussian is evaluated when a tile first stages it: at most once per staged entry, at least once if anything was staged
                assert 0 < R.last_stats["colour_evals"] <= R.last_stats["fetched_entries"] or R.last_stats["fetched_entries"] == 0, (name, sh_kw, kw)
                assert torch.equal(R.render(cam, mk(**kw)), R.render(cam, mk(colour_stage=1, **kw))), (name, sh_kw, kw)
    cols, cam, _ = _medium(G, n=60_000)
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols))
    cams = [cam, _medium(G, n=10, pose=5)[1], _medium(G, n=10, pose=11)[1]]
    assert torch.equal(R.render_batch(cams), R.render_batch(cams, mk(colour_stage=1)))


def test_launch_order_hint_changes_no_bit(G):
    """blend.hip, tile_order_kernel: tiles are launched heaviest first by what each staged in the LAST frame rendered on the
    workspace (GsrOptions.no_order_hint = 1: by list length).  A schedule only: the same bits after a frame of the same view, of
    another view, of another frame size's leftovers (a re-carved workspace holds anything) and in a workspace filled with 0xFF."""
    mk = G.renderer.make_options
    cols, cam, _ = _medium(G, n=250_000, shift=1.4, W=960, H=540, pose=4)
    other = _medium(G, n=10, W=960, H=540, pose=15)[1]
    small = _medium(G, n=10, W=640, H=360, pose=2)[1]
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols))
    ref = R.render(cam, mk(no_order_hint=True)).clone()
    st = dict(R.last_stats)
    assert torch.equal(R.render(cam), ref)                      # hint: the same view
    R.render(other)
    assert torch.equal(R.render(cam), ref)                      # hint: another view's work
    R.render(small)
    assert torch.equal(R.render(cam), ref)                      # another frame size in between: the workspace is carved anew
    R._workspace(cam.width, cam.height).fill_(255)
    assert R.unchecked.slices == 0                              # no frame to chain onto: the next one clears the 0xFF control block
    assert torch.equal(R.render(cam), ref)                      # garbage where the hint lives
    assert all(R.last_stats[k] == st[k] for k in st if k != "colour_evals")


def test_early_out_is_a_bounded_approximation(G):
    cols, cam, _ = _medium(G)
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols))
    exact = R.render(cam).cpu().numpy()
    fast = R.render(cam, G.renderer.make_options(early_out_T=1e-4)).cpu().numpy()
    assert np.abs(fast - exact).max() <= 1.01e-4                 # what is dropped is at most the remaining transmittance
    assert psnr(fast, exact) >= 70.0


@pytest.mark.parametrize("size", ["medium", "fullhd"])
def test_footprint_culling_is_exact(G, size):
    """Tightening tile rects / quadrant tests to the alpha > 1/255 footprint must not change a single bit:
    the frame with culling == the frame binned over the reference's full 3-sigma tile rects."""
    if size == "medium":
        cols, cam, _ = _medium(G)
    else:
        cols, cam, _ = _medium(G, n=1_000_000, seed=360, shift=0.0, W=1920, H=1080, pose=0)
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols))
    a, Ta = R.render(cam, return_T=True)
    culled = dict(R.last_stats)
    b, Tb = R.render(cam, G.renderer.make_options(no_footprint_cull=True), return_T=True)
    assert torch.equal(a, b) and torch.equal(Ta, Tb)
    assert culled["n_pairs"] < R.last_stats["n_pairs"]           # and it does remove work


def test_non_compat_differs_only_in_last_row_and_column(G):
    cols, cam, _ = _medium(G, n=50_000)
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols))
    a = R.render(cam)
    b = R.render(cam, G.renderer.make_options(reference_compat=False))
    assert torch.equal(a[:-1, :-1], b[:-1, :-1])
    assert b[-1].any() or b[:, -1].any()


def test_frames_are_bitwise_reproducible(G):
    cols, cam, _ = _medium(G)
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols))
    a = R.render(cam).clone()
    for _ in range(3):
        assert torch.equal(R.render(cam), a)


@pytest.mark.parametrize("step,block", [(2, 1), (3, 1), (8, 1), (2, 2), (3, 2), (4, 2), (8, 2)])
def test_tile_row_shards_reassemble_bit_exactly(G, step, block):
    """Multi-GPU sharding: interleaved tile rows — single rows, or pairs of rows = whole 32x32 cell rows
    (GsrOptions.tile_row_block) — rendered separately == the full frame."""
    cols, cam, _ = _medium(G, n=100_000, W=640, H=360)
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols))
    full = R.render(cam)
    tiles_y = (cam.height + 15) // 16
    out = torch.zeros_like(full)
    R.render(cam)
    full_visible = R.last_stats["n_visible"]
    pairs = 0
    for r in range(step):
        strip = R.render(cam, G.renderer.make_options(tile_row_begin=r, tile_row_step=step, output_layout=2, tile_row_block=block))
        pairs += R.last_stats["n_pairs"]
        assert 0 < R.last_stats["n_visible"] < full_visible       # a shard only preprocesses/sorts what touches its rows
        rows = G.renderer.shard_row_list(cam.height, r, step, block)
        assert rows == [t for t in range(tiles_y) if (t // block) % step == r] and strip.shape[0] == 16 * len(rows)
        for k, ty in enumerate(rows):
            h = min(16, cam.height - ty * 16)
            out[ty * 16: ty * 16 + h] = strip[k * 16: k * 16 + h]
    assert torch.equal(out, full)
    R.render(cam)
    assert pairs >= R.last_stats["n_pairs"] > 0                 # shards cull per-tile a little less (smaller rects)


def test_shards_of_a_frame_with_fewer_row_blocks_than_ranks(G):
    """A 200x40 frame has three tile rows = two cell rows: of 8 ranks most own nothing.  Their calls must render an empty strip and
    leave the others' rows alone; the plan's strips still assemble into the frame (both row plans, both preprocess kernels, a batch)."""
    from gsr_amd import dist as gdist

    cols, cam, _ = _medium(G, n=30_000, W=200, H=40)
    scene = G.renderer.GaussianScene.from_columns(cols)
    R = G.renderer.Rasterizer(scene)
    full = R.render(cam)
    assert bool(full.any())
    for block in (1, 2):
        plan = gdist.TileRowPlan(40, 200, 8, block)
        assert sum(1 for rows in plan.rows if not rows) == (5 if block == 1 else 6)
        strips = []
        for r in range(8):
            so = plan.shard_options(r)
            strip = R.render(cam, G.renderer.make_options(**so))
            assert tuple(strip.shape) == plan.strip_shape(r)
            if plan.rows[r]:
                assert torch.equal(G.renderer.Rasterizer(scene, views=2).render_batch([cam, cam], G.renderer.make_options(**so))[1], strip)
                assert torch.equal(R.render(cam, G.renderer.make_options(shard_preprocess=1, **so)), strip)
            else:
                assert R.last_stats["n_visible"] == 0 and R.last_stats["n_pairs"] == 0
            padded = torch.zeros(plan.padded_shape(), device="cuda")
            padded[: strip.shape[0]] = strip
            strips.append(padded)
        assert torch.equal(plan.assemble(strips), full)


def test_three_phase_shard_preprocess_on_its_other_paths(G):
    """preprocess.hip: ranks of 5+ shards find their gaussians with shard_preprocess_kernel (bound -> geometry -> colour, runs
    compacted for the depth sort).  test_tile_row_shards_reassemble_bit_exactly covers it at step 8 on the packed-rect fp32
    path; here the remaining instantiations, all bit for bit against the whole frame: fp16 SH storage, a frame wider than
    256 tiles (rects gathered by id, no packed payload through the sort), debug outputs that do not depend on the shard's path
    (a debug call on a shard still fills every gaussian's intermediates, then renders the shard correctly)."""
    mk = G.renderer.make_options

    def reassembles(R, cam, step, block=1):
        full = R.render(cam)
        out = torch.zeros_like(full)
        for r in range(step):
            strip = R.render(cam, mk(tile_row_begin=r, tile_row_step=step, output_layout=2, tile_row_block=block))
            for k, ty in enumerate(G.renderer.shard_row_list(cam.height, r, step, block)):
                h = min(16, cam.height - ty * 16)
                out[ty * 16: ty * 16 + h] = strip[k * 16: k * 16 + h]
        return torch.equal(out, full) and bool(full.any())

    cols, cam, _ = _medium(G, n=80_000, W=640, H=360)
    assert reassembles(G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols, sh_half=True)), cam, 5)
    assert reassembles(G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols, sh_half=True)), cam, 5, block=2)
    # wide frame: 263 tile columns x 13 tile rows
    W, H = 4200, 200
    wcols = G.synthetic.mip360_like(60_000, 12)
    for i in range(3):
        wcols[f"scale_{i}"] = (wcols[f"scale_{i}"] + np.float32(1.0)).astype(np.float32)
    p = G.synthetic.look_at_pose((0.0, -2.0, 0.1), (0, 0, 0), 1, "w.png")
    fx = G.synthetic.pinhole_focal(W, 100.0)
    wcam = G.renderer.make_camera(p.qvec, p.tvec, 2 * fx, 2 * fx, 2 * W, 2 * H, W, H)
    assert reassembles(G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(wcols)), wcam, 6)
    assert reassembles(G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(wcols)), wcam, 6, block=2)   # per-tile pairs, rows in pairs
    # debug outputs on a shard: every gaussian's intermediates, identical to the whole-frame call's
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols))
    o8 = mk(tile_row_begin=2, tile_row_step=8, output_layout=2)
    strip = R.render(cam, o8)
    whole, shard = R.preprocess_debug(cam), R.preprocess_debug(cam, o8)
    for k in whole:
        assert torch.equal(whole[k], shard[k]), k
    assert torch.equal(R.render(cam, o8), strip)
    # GsrOptions.shard_preprocess forces either kernel for any step: the same strip from both, also where the default picks the other
    for step, r in ((3, 1), (8, 5), (2, 0)):
        so = dict(tile_row_begin=r, tile_row_step=step, output_layout=2)
        a, b = R.render(cam, mk(shard_preprocess=1, **so)), R.render(cam, mk(shard_preprocess=2, **so))
        assert torch.equal(a, b) and torch.equal(a, R.render(cam, mk(**so))) and bool(a.any()), (step, r)
        assert torch.equal(R.render(cam, mk(shard_preprocess=2, colour_stage=1, **so)), a)
    # phase 1 reads a thread's four consecutive gaussians as 16-B pieces when means and log-scales are 16-B aligned, word by word
    # otherwise (and in the last workgroup of a scene whose size is no multiple of four): the same strips from arrays that start 4 bytes
    # into their buffers, and from a scene of 79 997 gaussians against the whole frame
    cut = {k: v[:79_997] for k, v in cols.items()}
    Rc = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cut, spatial_order=False))
    assert reassembles(Rc, cam, 8)
    so = dict(tile_row_begin=3, tile_row_step=8, output_layout=2)
    aligned = Rc.render(cam, mk(**so)).clone()
    keep = []
    for k in ("means", "log_scales"):
        buf = torch.zeros(Rc.scene.t[k].numel() + 1, dtype=torch.float32, device="cuda")
        buf[1:] = Rc.scene.t[k].reshape(-1)
        keep.append(buf)
        Rc.scene.t[k] = buf[1:].view(-1, 3)
        assert Rc.scene.t[k].data_ptr() % 16 == 4 and Rc.scene.t[k].is_contiguous()
    assert torch.equal(Rc.render(cam, mk(**so)), aligned) and bool(aligned.any())
    assert torch.equal(G.renderer.Rasterizer(Rc.scene, views=2).render_batch([cam, cam], mk(**so))[1], aligned)   # two views per launch sequence


def test_full_hd_one_million(G):
    """BASELINE-size frame (1920x1080), 1 M gaussians: oracle parity at full resolution."""
    cols, cam, ocam = _medium(G, n=1_000_000, seed=360, shift=0.0, W=1920, H=1080, pose=0)
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols))
    img = R.render(cam).cpu().numpy()
    oimg, _ = G.orc.render(G.utils.pack_gaussians(cols), ocam)
    assert_frames_close(img, oimg)


def test_depth_ties_resolve_by_index(G):
    """Thousands of exactly equal depth keys (500 gaussians stacked on each of 40 positions): the radix passes see one digit
    value per wave, the worst case for the per-digit ranking, and the stable sort must keep index order inside every tie
    (the oracle's order is stable too)."""
    cols, cam, ocam = _medium(G, n=20_000, shift=2.0)
    for k in "xyz":
        cols[k] = np.ascontiguousarray(cols[k][np.arange(20_000) % 40])
    packed = G.utils.pack_gaussians(cols)
    # (file order: ties resolve by SCENE index, and the oracle's scene is the file)
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(packed, spatial_order=False))
    img = R.render(cam).cpu().numpy()
    oimg, _ = G.orc.render(packed, ocam)
    assert R.last_stats["n_visible"] > 5_000
    # the loaders' default order keeps gaussians at one POSITION in file order (equal ranks are consecutive on every axis, the
    # curve is sorted stably): the same frame
    assert torch.equal(G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(packed)).render(cam).cpu(), torch.from_numpy(img))
    assert_frames_close(img, oimg)
    # and it is the order, not luck: reversing the gaussians inside the ties changes the frame
    rev = {k: np.ascontiguousarray(v[::-1]) for k, v in cols.items()}
    img_rev = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(rev, spatial_order=False)).render(cam).cpu().numpy()
    assert np.abs(img_rev - img).max() > 1e-3


def test_depth_ties_at_different_positions_follow_the_scene_order(G):
    """Exact depth ties between gaussians at DIFFERENT positions (rasterize.py:424-425: torch.sort leaves their mutual order undefined;
    libgsr and the oracle draw them in array-index order).  Camera on the z axis looking down +z, every gaussian's z drawn from 24
    values: depth = z + 14 exactly, ~800 gaussians per depth, spread over the frame and overlapping.  A file-order scene must
    reproduce the oracle fed the file; the loaders' default (Morton) order changes which of two tied, overlapping gaussians is
    drawn first — it must reproduce the oracle fed the arrays in the SCENE's order, and the two frames differ."""
    n, W, H = 20_000, 320, 192
    cols = G.synthetic.uniform_box(n, 77)
    rng = np.random.default_rng(5)
    cols["z"] = rng.choice(np.linspace(-6.0, 6.0, 24).astype(np.float32), n).astype(np.float32)
    for i in range(3):
        cols[f"scale_{i}"] = (cols[f"scale_{i}"] + np.float32(2.3)).astype(np.float32)
    p = G.synthetic.box_camera()
    fx = G.synthetic.pinhole_focal(W)
    args = (p.qvec, p.tvec, 2 * fx, 2 * fx, 2 * W, 2 * H, W, H)
    cam, ocam = G.renderer.make_camera(*args), G.orc.camera(*args)
    packed = G.utils.pack_gaussians(cols)
    depth = G.orc.preprocess(packed, ocam)["cam_means"][:, 2]
    assert len(np.unique(depth)) <= 24   # the ties are exact in fp32
    in_file = G.renderer.GaussianScene.from_packed(packed, spatial_order=False)
    img_file = G.renderer.Rasterizer(in_file).render(cam).cpu().numpy()
    assert_frames_close(img_file, G.orc.render(packed, ocam)[0])
    in_curve = G.renderer.GaussianScene.from_packed(packed)
    R = G.renderer.Rasterizer(in_curve)
    img_curve = R.render(cam).cpu().numpy()
    assert R.last_stats["n_visible"] > 5_000
    ordered = {k: np.ascontiguousarray(v[in_curve.order]) for k, v in packed.items()}
    assert_frames_close(img_curve, G.orc.render(ordered, ocam)[0])
    d = np.abs(img_curve - img_file).max()
    print(f"\nexact depth ties, file order vs Morton order of the same scene: max abs difference {d:.4f}")
    assert d > 1e-3   # the storage order decides tied draws: documented in include/gsr.h (GsrScene) and README


def test_blend_counters_describe_the_last_blend(G):
    """wave_entries / fetched_entries are per-workgroup stores totalled by gsr_read_stats: no accumulation across frames,
    zero before any blend ran, the same staging count from both blend kernels."""
    import ctypes as C

    from gsr_amd._lib import check, lib

    cols, cam, _ = _medium(G, n=100_000)
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols))
    # the first frame on a fresh workspace launches its tiles in an order taken from whatever the allocator left in tile_work (never
    # cleared, never trusted), and the deferred colours' race count follows the launch order: compare frames launched from a real hint
    R.render(cam)
    R.render(cam)
    first = dict(R.last_stats)
    R.render(cam)
    same = lambda a, b: all(a[k] == b[k] for k in a if k != "colour_evals")
    assert same(R.last_stats, first) and first["wave_entries"] > 0
    # deferred colours: tiles racing for a gaussian may each evaluate it (same value), so the count varies a little from run to run
    assert 0 < first["colour_evals"] <= first["fetched_entries"] and abs(R.last_stats["colour_evals"] - first["colour_evals"]) <= 0.05 * first["colour_evals"]
    R.render(cam, G.renderer.make_options(blend_impl=1))
    assert first["fetched_entries"] <= R.last_stats["fetched_entries"] <= 1.05 * first["fetched_entries"]   # batches of 256 vs 128
    assert abs(R.last_stats["wave_entries"] - first["wave_entries"]) <= 0.05 * first["wave_entries"]
    # stages 1 and 2 only: the frame reset cleared the totals and no blend has refilled them
    ws = R._workspace(cam.width, cam.height)
    sc, opts = R.scene.c_struct(), G.renderer.make_options()
    sp = int(torch.cuda.current_stream().cuda_stream)
    check(lib.gsr_preprocess(C.byref(sc), C.byref(cam), C.byref(opts), ws.data_ptr(), ws.numel(), None, sp))
    check(lib.gsr_bin_sort(R.scene.n, C.byref(cam), C.byref(opts), R.max_pairs, ws.data_ptr(), ws.numel(), sp))
    st = R.stats()
    assert st["wave_entries"] == 0 and st["fetched_entries"] == 0 and st["colour_evals"] == 0 and st["n_pairs"] == first["n_pairs"]
    # shards: every tile is blended by exactly one shard (lists can only grow where a rect falls under the per-tile test)
    tot = 0
    for r in range(3):
        R.render(cam, G.renderer.make_options(tile_row_begin=r, tile_row_step=3, output_layout=2))
        tot += R.last_stats["fetched_entries"]
    assert first["fetched_entries"] <= tot <= 1.1 * first["fetched_entries"]


def test_bf16_frame_storage_is_the_rounded_fp32_frame(G):
    """GsrOptions.output_dtype = 1 (BASELINE configs[2]): accumulation stays fp32, only the store is bfloat16 —
    bit for bit torch's round-to-nearest-even of the fp32 frame, in every layout and through the batch entry."""
    cols, cam, ocam = _medium(G, n=60_000)
    packed = G.utils.pack_gaussians(cols)
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(packed))
    mk = G.renderer.make_options
    ref = R.render(cam)
    got = R.render(cam, mk(output_bf16=True))
    assert got.dtype == torch.bfloat16 and torch.equal(got, ref.to(torch.bfloat16))
    oimg, _ = G.orc.render(packed, ocam)
    assert psnr(got.float().cpu().numpy(), oimg) >= 55.0     # 8 mantissa bits of storage; the bar is 50 dB
    for extra in (dict(output_layout=1), dict(tile_row_begin=1, tile_row_step=3, output_layout=2), dict(blend_impl=1)):
        a = R.render(cam, mk(**extra))
        b = R.render(cam, mk(output_bf16=True, **extra))
        assert torch.equal(b, a.to(torch.bfloat16))
    batch = R.render_batch([cam, cam], mk(output_bf16=True))
    assert batch.dtype == torch.bfloat16 and torch.equal(batch[0], got) and torch.equal(batch[1], got)
    with pytest.raises(ValueError):
        R.render(cam, mk(output_bf16=True), out=torch.empty_like(ref))


def test_c_abi_rejects_bad_arguments(G):
    """Error behaviour of the boundary (include/gsr.h): a negative GsrStatus plus gsr_last_error() text, nothing enqueued,
    and the workspace / output untouched — never a fault on the device."""
    import ctypes as C

    from gsr_amd import _lib
    from gsr_amd._lib import lib

    cols, cam, _ = _medium(G, n=5_000, W=160, H=96)
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols))
    ref = R.render(cam)
    ws = R._workspace(cam.width, cam.height)
    sc, mk = R.scene.c_struct(), G.renderer.make_options
    out = torch.full_like(ref, 7.0)
    sp = int(torch.cuda.current_stream().cuda_stream)

    def call(scene=sc, camera=cam, opts=None, max_pairs=R.max_pairs, wsp=ws.data_ptr(), wsn=ws.numel(), o=out.data_ptr()):
        opts = opts or mk()
        return lib.gsr_render_forward(C.byref(scene), C.byref(camera), C.byref(opts), max_pairs, wsp, wsn, o, None, sp)

    def bad_opts(**kw):
        o = mk()
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def bad_cam(**kw):
        c = type(cam).from_buffer_copy(cam)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def bad_scene(**kw):
        s = type(sc).from_buffer_copy(sc)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    cases = {
        "short workspace": dict(wsn=ws.numel() // 2), "null workspace": dict(wsp=None), "null output": dict(o=None),
        "negative max_pairs": dict(max_pairs=-1), "zero width": dict(camera=bad_cam(width=0)), "negative height": dict(camera=bad_cam(height=-3)),
        "row begin >= step": dict(opts=bad_opts(tile_row_begin=3, tile_row_step=3)), "negative row step": dict(opts=bad_opts(tile_row_step=-1)),
        "bad layout": dict(opts=bad_opts(output_layout=5)), "bad dtype": dict(opts=bad_opts(output_dtype=2)),
        "negative draw_limit": dict(opts=bad_opts(draw_limit=-1)), "negative n": dict(scene=bad_scene(n=-1)),
        "null means": dict(scene=bad_scene(means=None)), "misaligned sh": dict(scene=bad_scene(sh=sc.sh + 4)),
        "bad sh degree": dict(scene=bad_scene(sh_degree=4)), "bad sh dtype": dict(scene=bad_scene(sh_dtype=9)),
        # the size limits of include/gsr.h, the same gsr_workspace_bytes applies (tests/test_abi.py)
        "width past the limit": dict(camera=bad_cam(width=_lib.GSR_MAX_FRAME_SIDE + 1)),
        "height past the limit": dict(camera=bad_cam(height=_lib.GSR_MAX_FRAME_SIDE + 1)),
        "n past 2^31 - 1": dict(scene=bad_scene(n=_lib.GSR_MAX_GAUSSIANS + 1)),
        "max_pairs past GSR_MAX_PAIRS": dict(max_pairs=_lib.GSR_MAX_PAIRS + 1),
    }
    for name, kw in cases.items():
        rc = call(**kw)
        assert rc < 0, f"{name}: status {rc}"
        assert lib.gsr_last_error(), name
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a rejected call wrote to the output"
    assert call() == 0 and torch.equal(out, ref)   # and the library is still usable
    with pytest.raises(_lib.GsrError):
        _lib.workspace_bytes(10, 0, 10, 10)
    with pytest.raises(_lib.GsrError):
        _lib.workspace_bytes(10, _lib.GSR_MAX_FRAME_SIDE + 1, 10, 10)


def test_depth_sort_plans_its_passes_from_the_key_range(G):
    """sort.hip: the depth sort runs on key - bits(0.2f) and only over the bits the frame uses.  An ordinary scene (depths
    0.2 .. 64) sorts in 3 passes (9 + 9 + 9 bits); the same scene blown up 1000x needs the fourth.  Both against the oracle at
    frame tolerance — which on these random scenes would not show neighbours a few ulps apart drawn out of order: that the order
    is exact under every plan and digit split is shown by tests/test_gpu_draw_order.py, on scenes where any swap moves a pixel by
    more than twice the tolerance (tests/test_order_scenes.py).  GsrStats.sort_passes reports the
    plan; GsrOptions.depth_sort_passes bounds what is enqueued, verified on the device: the same frame when the bound
    holds, GSR_ERR_SORT_PASSES when it does not, and the Rasterizer learns the bound from the counters it reads."""
    from gsr_amd import _lib

    mk = G.renderer.make_options
    cols, cam, ocam = _medium(G, n=120_000)
    packed = G.utils.pack_gaussians(cols)
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(packed))
    assert R.sort_passes == 0
    img = R.render(cam)                                    # no bound yet: four passes enqueued, three run
    assert R.last_stats["sort_passes"] == 3 and R.sort_passes == 3 and R.last_stats["overflow"] == 0
    oimg, _ = G.orc.render(packed, ocam)
    assert_frames_close(img.cpu().numpy(), oimg)
    assert torch.equal(R.render(cam), img)                  # now with the learned bound: three passes enqueued
    for k in (3, 4):
        assert torch.equal(R.render(cam, mk(depth_sort_passes=k)), img)
    with pytest.raises(_lib.GsrSortPasses):                 # the caller's own bound is not second-guessed
        R.render(cam, mk(depth_sort_passes=2))
    assert R.last_stats["sort_passes"] == 3 and R.last_stats["overflow"] == 2
    assert torch.equal(R.render(cam), img)
    far = {k: v.copy() for k, v in cols.items()}
    for k in "xyz":
        far[k] = (far[k] * np.float32(1000.0)).astype(np.float32)
    for i in range(3):
        far[f"scale_{i}"] = (far[f"scale_{i}"] + np.float32(np.log(1000.0) - 1.5)).astype(np.float32)
    fpacked = G.utils.pack_gaussians(far)
    Rf = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(fpacked))
    Rf.sort_passes = 3                                      # a bound learned elsewhere that does not hold here: detected, raised, re-rendered
    fimg = Rf.render(cam).cpu().numpy()
    assert Rf.last_stats["sort_passes"] == 4 and Rf.sort_passes == 4 and Rf.last_stats["n_visible"] > 1000
    foimg, _ = G.orc.render(fpacked, ocam)
    assert_frames_close(fimg, foimg)
    out = torch.empty_like(img)
    Rf.sort_passes = 3
    Rf.enqueue(cam, Rf.bounded(), out=out)                  # enqueue() takes opts as given and does not check: the counters do
    with pytest.raises(_lib.GsrSortPasses):
        Rf.stats()
    # the plan is per frame: the near scene goes back to 3 passes whatever the workspace rendered before
    assert torch.equal(R.render(cam), img) and R.last_stats["sort_passes"] == 3


def _two_depth_clusters(G):
    """A scene with two clusters and two cameras at the origin: cam_near (looking +z) sees only the cluster at depth ~10
    (a 3-pass depth sort: 27 key bits), cam_far (looking -z) only the one at depth ~20 000 (28 bits: 4 passes)."""
    rng = np.random.default_rng(11)
    m = 4000
    cols = G.synthetic.mip360_like(2 * m, 3)
    near = rng.normal(0, 1.0, (m, 3)) + np.array([0, 0, 10.0])
    far = rng.normal(0, 150.0, (m, 3)) + np.array([0, 0, -20000.0])
    xyz = np.concatenate([near, far]).astype(np.float32)
    for i, k in enumerate("xyz"):
        cols[k] = np.ascontiguousarray(xyz[:, i])
    for i in range(3):
        cols[f"scale_{i}"] = np.concatenate([np.full(m, np.log(0.08)), np.full(m, np.log(60.0))]).astype(np.float32)
    W, H = 320, 192
    fx = G.synthetic.pinhole_focal(W)
    mkc = lambda q: G.renderer.make_camera(q, (0.0, 0.0, 0.0), 2 * fx, 2 * fx, 2 * W, 2 * H, W, H)
    return cols, mkc((1.0, 0.0, 0.0, 0.0)), mkc((0.0, 0.0, 1.0, 0.0))


def test_batches_report_the_worst_views_depth_sort_plan(G):
    """A learned depth-sort bound that is too small for ONE view of a batch (round 2: an endless retry loop — the flag was
    batch-sticky, the reported plan the LAST view's).  FrameCtrl.batch_sort_passes carries the worst view's plan:
    gsr_read_stats reports it with GSR_ERR_SORT_PASSES, Rasterizer / FramesInFlight re-run once with it."""
    import ctypes as C

    from gsr_amd import _lib
    from gsr_amd._lib import GsrCamera, lib

    cols, cam_near, cam_far = _two_depth_clusters(G)
    scene = G.renderer.GaussianScene.from_columns(cols)
    mk = G.renderer.make_options
    R = G.renderer.Rasterizer(scene)
    near, far = R.render(cam_near), R.render(cam_far, mk(depth_sort_passes=4))
    assert R.last_stats["sort_passes"] == 4 and float(near.max()) > 0.05 and float(far.max()) > 0.05
    R1 = G.renderer.Rasterizer(scene)
    assert torch.equal(R1.render(cam_near), near) and R1.sort_passes == 3
    # the C ABI: [far, near] with the bound 3 — the flag is set by view 0, the last view's own plan (3) fits
    ws = R1._workspace(cam_near.width, cam_near.height)
    arr = (GsrCamera * 2)(cam_far, cam_near)
    out = torch.empty((2,) + tuple(near.shape), device="cuda")
    sc, st = scene.c_struct(), _lib.GsrStats()
    sp = int(torch.cuda.current_stream().cuda_stream)
    assert lib.gsr_render_batch(C.byref(sc), arr, 2, C.byref(mk(depth_sort_passes=3)), R1.max_pairs, ws.data_ptr(), ws.numel(),
                                out.data_ptr(), near.numel(), sp) == 0
    assert lib.gsr_read_stats(ws.data_ptr(), ws.numel(), C.byref(st), sp) == _lib.GSR_ERR_SORT_PASSES
    assert st.overflow & 2 and st.sort_passes == 4            # what to re-render with, not the last view's 3
    # the host classes: preset bound 3, batch = [4-pass view, 3-pass view]
    for views in ([cam_far, cam_near], [cam_near, cam_far, cam_near]):
        Rb = G.renderer.Rasterizer(scene)
        Rb.sort_passes = 3
        b = Rb.render_batch(views)
        assert Rb.sort_passes == 4
        for v, img in zip(views, b):
            assert torch.equal(img, far if v is cam_far else near)
    fif = G.renderer.FramesInFlight(scene, slots=2)
    fif.set_sort_passes(3)
    views = [cam_near, cam_far, cam_near, cam_near, cam_near]   # slot 1 renders far, then near: its last view fits the bound
    b = fif.render_batch(views)
    for v, img in zip(views, b):
        assert torch.equal(img, far if v is cam_far else near)
    # unchecked frames are chained (GsrOptions.keep_flags): ONE stats() after a run speaks for all of them
    Rc = G.renderer.Rasterizer(scene)
    Rc.sort_passes = 3
    o = Rc.bounded()
    assert o.depth_sort_passes == 3
    Rc.enqueue(cam_near, o); Rc.enqueue(cam_far, o); Rc.enqueue(cam_near, o)
    with pytest.raises(_lib.GsrSortPasses):
        Rc.stats()
    assert Rc.last_stats["sort_passes"] == 4
    Rc.enqueue(cam_near, o)                                   # the record was cleared by stats(): a clean frame reads clean
    assert Rc.stats()["overflow"] == 0
    tiny = G.renderer.Rasterizer(scene, max_pairs=64)         # the same chain for the pair bound: [overflows, fits]
    tiny.enqueue(cam_near); tiny.enqueue(cam_near, mk(draw_limit=1))
    with pytest.raises(_lib.GsrPairOverflow):
        tiny.stats()
    assert tiny.last_stats["n_pairs_bbox"] > 64
    assert torch.equal(tiny.render(cam_near), near)           # render() grows the buffer and returns the complete frame


def test_fuzz_case_that_stalled_round_2_replays(G):
    """tools/fuzz_parity.py seed 606, case 208 (case-seed 1607415101109889117: ONE gaussian on a 160x360 frame): `cam` sees
    nothing (depth-sort plan 1 pass), the shifted `cam2` sees the gaussian (3 passes).  render_batch([cam, cam2, cam]) with
    the bound learned from `cam` looped forever in round 2; it must return and equal the three single renders — through
    Rasterizer and through FramesInFlight with more views than slots."""
    c = fuzz_case(1607415101109889117, 120000)
    assert c["n"] == 1 and (c["W"], c["H"]) == (160, 360)
    args, pose = c["args"], c["pose"]
    cam = G.renderer.make_camera(*args)
    cam2 = G.renderer.make_camera(pose.qvec, np.asarray(pose.tvec) + np.array([0.05, -0.02, 0.1]), *args[2:])
    scene = G.renderer.GaussianScene.from_packed(c["packed"], sh_degree=c["degree"])
    R = G.renderer.Rasterizer(scene)
    img = R.render(cam)
    assert R.sort_passes == 1 and R.last_stats["n_visible"] == 0
    b = R.render_batch([cam, cam2, cam])
    assert R.sort_passes == 3
    img2 = G.renderer.Rasterizer(scene).render(cam2)
    assert float(img2.max()) > 0 and torch.equal(b[0], img) and torch.equal(b[1], img2) and torch.equal(b[2], img)
    fif = G.renderer.FramesInFlight(scene, slots=2)
    fif.set_sort_passes(1)
    views = [cam, cam2, cam, cam2, cam]
    b = fif.render_batch(views)
    for v, got in zip(views, b):
        assert torch.equal(got, img2 if v is cam2 else img)


def test_f5_deep_stacks_against_the_reference_frame(G):
    """The HIP frame of fixture f5 (see tests/test_oracle_golden.py: the reference's own frame of the deep-stack fuzz case)
    against the REFERENCE, not the oracle: no further from it than the plain-C oracle is (111.7 dB, worst pixel 3.3e-5)."""
    g, c = f5_case()
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(c["packed"]))
    img = R.render(G.renderer.make_camera(*c["args"])).cpu().numpy()
    assert R.last_stats["n_visible"] <= int(g["n_drawn"])
    d = np.abs(img.astype(np.float64) - g["image"]).max(axis=2)
    oimg, _ = G.orc.render(c["packed"], G.orc.camera(*c["args"]))
    do = np.abs(img.astype(np.float64) - oimg).max(axis=2)
    print(f"\nf5 HIP vs reference: {(d > 1e-5).sum()} of {d.size} pixels off by > 1e-5, worst {d.max():.2e}, {psnr(img, g['image']):.1f} dB; "
          f"HIP vs oracle: {(do > 1e-5).sum()} pixels, worst {do.max():.2e}")
    assert d.max() <= 1e-4 and psnr(img, g["image"]) >= 105.0
    assert do.max() <= 1e-4


def test_spatial_order_renders_the_same_frame(G):
    """The loaders upload the arrays in Morton order of the means (GaussianScene.sort_spatially, on the device; the default since
    round 4) — the same permutation as the numpy statement renderer.morton_order.  The reference's result does not depend on
    storage order — its depth sort orders the draw — except for gaussians at exactly equal depth, so: same counters; the frame
    bit-identical when no two visible gaussians share a depth, and within the usual tolerance of the oracle either way."""
    cols, cam, ocam = _medium(G, n=150_000)
    packed = G.utils.pack_gaussians(cols)
    plain_scene = G.renderer.GaussianScene.from_packed(packed, spatial_order=False)
    assert plain_scene.order is None
    plain = G.renderer.Rasterizer(plain_scene)
    scene = G.renderer.GaussianScene.from_packed(packed)
    assert sorted(scene.order.tolist()) == list(range(150_000)) and not np.array_equal(scene.order, np.arange(150_000))
    assert np.array_equal(scene.order, G.renderer.morton_order(packed["means"]))      # gsr_scene_order == the numpy statement
    # ... also with repeated coordinates, signed zeros and a count that fills no sort tile (stable ranks, -0.0 == +0.0)
    rng = np.random.default_rng(11)
    for n_ in (1, 2, 255, 4097, 70_001):
        m_ = rng.normal(size=(n_, 3)).astype(np.float32)
        m_[rng.integers(0, n_, n_ // 3)] = m_[rng.integers(0, n_, n_ // 3)]
        m_[rng.integers(0, n_, max(1, n_ // 7)), rng.integers(0, 3)] = np.float32(-0.0)
        m_[rng.integers(0, n_, max(1, n_ // 7)), rng.integers(0, 3)] = np.float32(0.0)
        dev = torch.from_numpy(m_).cuda()
        want = G.renderer.morton_order(m_)
        assert np.array_equal(G.renderer.scene_order(dev).cpu().numpy(), want), n_
        assert np.array_equal(G.renderer.morton_order_device(dev).cpu().numpy(), want), n_
    for k in scene.FIELDS:
        assert np.array_equal(scene.t[k].cpu().numpy(), packed[k][scene.order]), k
    assert scene.sort_spatially() is scene and scene.order_ms > 0
    R = G.renderer.Rasterizer(scene)
    a, b = plain.render(cam), R.render(cam)
    for k in ("n_visible", "n_pairs_bbox", "n_pairs"):
        assert plain.last_stats[k] == R.last_stats[k], k
    z = plain.preprocess_debug(cam)["cam_means"][:, 2].cpu().numpy()
    vis = z[z >= 0.2]
    ties = len(vis) - len(np.unique(vis))
    if ties == 0:
        assert torch.equal(a, b)
    assert float((a - b).abs().max()) < 1e-4 and psnr(b.cpu().numpy(), a.cpu().numpy()) >= 110.0, ties
    oimg, _ = G.orc.render(packed, ocam)
    assert_frames_close(b.cpu().numpy(), oimg)
    # per-gaussian outputs come back in FILE order whatever the scene's order
    da, db = plain.preprocess_debug(cam), R.preprocess_debug(cam)
    for k in da:
        assert torch.equal(da[k], db[k]), k


def test_a_fresh_workspace_needs_no_initialisation(G):
    """The C ABI asks nothing of a new workspace: every word of the control block is cleared by the frame itself, also the
    depth sort's key maximum (round 2 left that word to the caller: garbage there made a bounded first frame mis-sort).
    A workspace filled with 0xFF renders the same frame, with depth_sort_passes = 3, and reads clean counters."""
    import ctypes as C

    from gsr_amd import _lib
    from gsr_amd._lib import check, lib

    cols, cam, _ = _medium(G, n=80_000)
    scene = G.renderer.GaussianScene.from_columns(cols)
    R = G.renderer.Rasterizer(scene)
    ref = R.render(cam)
    ws = torch.full((R._ws.numel(),), 0xFF, dtype=torch.uint8, device="cuda")
    out = torch.empty_like(ref)
    sc, st = scene.c_struct(), _lib.GsrStats()
    sp = int(torch.cuda.current_stream().cuda_stream)
    check(lib.gsr_render_forward(C.byref(sc), C.byref(cam), C.byref(G.renderer.make_options(depth_sort_passes=3)), R.max_pairs,
                                 ws.data_ptr(), ws.numel(), out.data_ptr(), None, sp))
    check(lib.gsr_read_stats(ws.data_ptr(), ws.numel(), C.byref(st), sp))
    assert torch.equal(out, ref) and st.overflow == 0 and st.sort_passes == 3 and st.n_visible == R.last_stats["n_visible"]


def test_hand_scheduled_blend_walk_equals_the_plain_kernel(G):
    """blend.hip: the default kernel (two quadrants per wave) walks its survivors in one hand-written asm statement
    (EXEC-masked update, unguarded fast path, shared terms of the quadratic, rolling LDS prefetch); blend_impl = 1 is the
    plain-C kernel (one quadrant per wave).  Same operations on the same values, so frames, transmittance and the evaluated
    counts must be identical bit for bit — whole frames, shards, early-out, bf16 store, non-compat, the
    fixtures with their edge cases (a frame-covering gaussian, the 0.99 cap, frames not a multiple of 16)."""
    mk = G.renderer.make_options
    # 640x360: the pipelined one-quadrant walk; 960x540 (2040 tiles): the plain one-quadrant walk; 1080p: two quadrants per wave
    # (and its tile_row_step = 4 shard: 2040 tiles again)
    cases = [_medium(G)[:2], _medium(G, n=300_000, shift=1.6, pose=7)[:2], _medium(G, n=250_000, shift=1.4, W=960, H=540, pose=4)[:2],
             _medium(G, n=400_000, seed=360, shift=0.8, W=1920, H=1080, pose=0)[:2]]
    for name, prefix in (("f2_small.npz", ""), ("f3_edge.npz", "a_"), ("f3_edge.npz", "b_")):
        g = load_golden(name)
        cases.append((golden_columns(g), _cams(G, g, prefix)[0]))
    for cols, cam in cases:
        R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols))
        for kw in (dict(), dict(early_out_T=1e-4), dict(tile_row_begin=2, tile_row_step=5, output_layout=2), dict(output_bf16=True),
                   dict(reference_compat=False), dict(output_layout=1), dict(no_footprint_cull=True),
                   dict(tile_row_begin=1, tile_row_step=4, output_layout=2)):
            # without the T output the colour-saturation rule runs (GsrOptions.saturation_rule): same frames, same counts
            c = R.render(cam, mk(**kw))
            sc = dict(R.last_stats)
            d = R.render(cam, mk(blend_impl=1, **kw))
            assert torch.equal(c, d), kw
            assert all(sc[k] == R.last_stats[k] for k in sc if k not in ("fetched_entries", "colour_evals")) and sc["fetched_entries"] <= R.last_stats["fetched_entries"], kw
            a, Ta = R.render(cam, mk(**kw), return_T=True)
            sa = dict(R.last_stats)
            b, Tb = R.render(cam, mk(blend_impl=1, **kw), return_T=True)
            assert torch.equal(a, b) and torch.equal(Ta, Tb), kw
            assert "early_out_T" in kw or torch.equal(a, c), kw  # (an approximate threshold stops the two rules' quadrants at different entries)
            sb = R.last_stats
            # same lists, same evaluations; the product kernel stages 128 entries per batch, the plain one 256, so a tile that
            # saturates stops fetching a little earlier in the former
            assert all(sa[k] == sb[k] for k in sa if k not in ("fetched_entries", "colour_evals")) and sa["fetched_entries"] <= sb["fetched_entries"], kw


@pytest.mark.parametrize("name,prefix", [("medium", ""), ("960x540", ""), ("f3_edge.npz", "a_"), ("f3_edge.npz", "b_")])
def test_coarse_binning_builds_the_same_frame_as_fine_binning(G, name, prefix):
    """binning.hip: pairs are generated and sorted per 32x32 cell, and the blend of a tile keeps the cell-list entries that carry
    its bit (blend.hip, TileList); with GsrOptions.fine_binning = 1 pairs are generated per tile directly (the path frames wider than
    4096 px always take).  Every tile walks the same gaussians in the same order up to entries whose footprint misses the tile (coarser emit-time culling keeps
    a few more; the blend's quadrant test rejects them): frames, T and the evaluated count must be identical — whole frame,
    shards (odd and even steps), progressive prefixes, culling off, a frame-covering gaussian (f3a), a frame that is not a
    multiple of 16 or 32 (f3b)."""
    if name == "medium":
        cols, cam, _ = _medium(G, n=150_000, W=650, H=370)
    elif name == "960x540":  # 2040 tiles: the one-quadrant walk without the pipelining (blend_walk_kernel<1, false>)
        cols, cam, _ = _medium(G, n=250_000, shift=1.4, W=960, H=540, pose=4)
    else:
        g = load_golden(name)
        cols = golden_columns(g)
        cam, _ = _cams(G, g, prefix)
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols))
    mk = G.renderer.make_options
    variants = [dict(), dict(tile_row_begin=1, tile_row_step=3, output_layout=2), dict(tile_row_begin=3, tile_row_step=8, output_layout=2),
                dict(draw_limit=37), dict(no_footprint_cull=True), dict(reference_compat=False)]
    coarse = []
    for kw in variants:
        img, T = R.render(cam, mk(**kw), return_T=True)
        st = dict(R.last_stats)
        coarse.append((img.clone(), T.clone(), st, R.render(cam, mk(**kw)).clone(), R.last_stats["wave_entries"]))
    for kw, (img, T, st, img0, ev0) in zip(variants, coarse):
        fimg, fT = R.render(cam, mk(fine_binning=True, **kw), return_T=True)
        assert torch.equal(fimg, img) and torch.equal(fT, T) and torch.equal(img0, img)
        # the lists may differ in entries that touch no pixel of their tile (the two paths cull at emission on different
        # rectangles); what the blend evaluates after its exact per-quadrant test is the same — up to where a saturated quadrant
        # stops: that is tested per 64 LIST entries, and entries that touch no pixel shift the chunk boundaries (the dense 960x540
        # frame saturates, the others do not)
        assert R.last_stats["n_visible"] == st["n_visible"]
        if name == "960x540":
            assert abs(R.last_stats["wave_entries"] - st["wave_entries"]) <= 0.005 * st["wave_entries"]
        else:
            assert R.last_stats["wave_entries"] == st["wave_entries"]
        assert torch.equal(R.render(cam, mk(fine_binning=True, **kw)), img)
    assert torch.equal(R.render(cam), coarse[0][0])
