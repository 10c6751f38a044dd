"""The rasterizer's exact shortcuts on scenes built on their margins (tests/margin_scenes.py).

Six shortcuts skip work and claim to change no bit of the frame, each on an fp32 error margin argued in a comment: the footprint
AABB (preprocess.hip), the per-tile / per-cell pair test (binning.hip, footprint_hits_rect), the per-quadrant ballot in the blend,
the unguarded fast path (footprint_classify), block culling from the scene's bounds (block_dead) and the row test of the
three-phase shard preprocess.  Random scenes almost never put a pixel within 1e-5 of the alpha = 1/255 ellipse or a conic within
1e-4 of the fast path's correlation limit; these scenes do, on both sides, and every shortcut is compared with its disabled twin
bit for bit (frame and T), then the frame with the CPU oracle with every difference accounted for.
"""
import numpy as np
import pytest
import torch

import margin_scenes as ms
from conftest import assert_frames_close
from gpu_cases import namespace

SIZES = [(650, 370), (960, 540), (1283, 723)]   # pipelined one-quadrant walk (984 tiles), plain one-quadrant walk (2040), two per wave (3726)
_CACHE = {}


def scene_of(W, H):
    if (W, H) not in _CACHE:
        _CACHE[(W, H)] = ms.MarginScene(W, H, seed=W * 7 + H)
    return _CACHE[(W, H)]


def _counts(s, mx, my, sg, op, z):
    return ms.population_counts(s.meta, mx, my, sg[:, 0], sg[:, 1], sg[:, 2], op, z)


def _check_floors(counts, where):
    print(f"\n{where}: " + ", ".join(f"{k}: {v}" for k, v in counts.items()))
    low = {k: (counts.get(k), f) for k, f in ms.FLOORS.items() if counts.get(k, 0) < f}
    assert not low, f"{where}: populations below their floors (count, floor): {low}"


@pytest.mark.parametrize("W,H", SIZES)
def test_margin_scenes_sit_on_the_boundaries(W, H):
    """CPU: the oracle's fp32 intermediates, evaluated in float64, put enough (gaussian, pixel) / (gaussian, quadrant) pairs within a
    small band of every unloosened boundary, on each side — a drifting generator cannot quietly turn these into random scenes."""
    s = scene_of(W, H)
    p = s.pre
    _check_floors(_counts(s, p["screen_means"][:, 0], p["screen_means"][:, 1], p["sigmas"], p["opacity"], p["cam_means"][:, 2]),
                  f"oracle {W}x{H}")
    # deterministic: the same seed builds the same columns
    again = ms.MarginScene(W, H, seed=W * 7 + H)
    assert all(np.array_equal(again.cols[k], s.cols[k]) for k in s.cols)


# ---------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def G():
    return namespace()


def _setup(G, W, H):
    s = scene_of(W, H)
    cam = G.renderer.make_camera(*s.cam_args)
    scene = G.renderer.GaussianScene.from_columns(s.cols)          # Morton order with block bounds, as the loaders build it
    return s, cam, scene


def _strips(G, R, cam, step, block, kw, want_T):
    """tile-row shards rendered one by one and reassembled into the frame (and T)."""
    H = cam.height
    img = torch.zeros((H, cam.width, 3), dtype=torch.float32, device="cuda")
    T = torch.zeros((H, cam.width), dtype=torch.float32, device="cuda")
    for r in range(step):
        o = G.renderer.make_options(tile_row_begin=r, tile_row_step=step, output_layout=2, tile_row_block=block, **kw)
        got = R.render(cam, o, return_T=want_T)
        strip, tstrip = got if want_T else (got, None)
        for k, ty in enumerate(G.renderer.shard_row_list(H, r, step, block)):
            h = min(16, H - ty * 16)
            img[ty * 16: ty * 16 + h] = strip[k * 16: k * 16 + h]
            if want_T:
                T[ty * 16: ty * 16 + h] = tstrip[k * 16: k * 16 + h]
    return img, T


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", SIZES)
def test_kernel_intermediates_sit_on_the_boundaries(G, W, H):
    """The same population counts from the kernel's own intermediates (Rasterizer.preprocess_debug): its conics can differ from
    the oracle's by ulps."""
    s, cam, scene = _setup(G, W, H)
    d = {k: v.cpu().numpy() for k, v in G.renderer.Rasterizer(scene).preprocess_debug(cam).items()}
    _check_floors(_counts(s, d["screen_means"][:, 0], d["screen_means"][:, 1], d["sigmas"], d["opacity"], d["cam_means"][:, 2]),
                  f"kernel {W}x{H}")


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", SIZES)
def test_every_shortcut_equals_its_disabled_twin(G, W, H):
    """Frame and T, bit for bit: footprint culling (AABB, emit-time and quadrant tests) vs no_footprint_cull; the hand-scheduled
    walk with its unguarded fast path vs the plain kernel; block culling with vs without bounds (Morton and file order); the
    three-phase and the whole-frame shard preprocess (steps 5 and 8, single rows and row pairs) reassembled vs the whole frame;
    coarse vs fine binning; each with reference_compat 1 and 0; the colour-saturation rule (no T) as well."""
    mk = G.renderer.make_options
    s, cam, scene = _setup(G, W, H)
    bare = G.renderer.GaussianScene({k: scene.t[k] for k in scene.FIELDS})   # the same arrays without block bounds
    bare.order_t = scene.order_t
    file_scene = G.renderer.GaussianScene.from_columns(s.cols, spatial_order=False)
    file_bounded = G.renderer.GaussianScene.from_columns(s.cols, spatial_order=False).build_bounds()
    R, Rb, Rf, Rfb = (G.renderer.Rasterizer(x) for x in (scene, bare, file_scene, file_bounded))
    assert scene.bounds is not None and file_bounded.bounds is not None
    print(f"\n{W}x{H}: {s.n} gaussians, blocks skipped {float(scene.blocks_skipped(cam).float().mean()):.3f} (morton), "
          f"{float(file_bounded.blocks_skipped(cam).float().mean()):.3f} (file)")
    # the cluster off the top-left corner: block culling has something to skip in one of the orders
    assert scene.blocks_skipped(cam).any() or file_bounded.blocks_skipped(cam).any()
    for compat in (True, False):
        base_kw = dict(reference_compat=compat)
        img, T = R.render(cam, mk(**base_kw), return_T=True)
        img, T = img.clone(), T.clone()
        stats = dict(R.last_stats)
        img0 = R.render(cam, mk(**base_kw)).clone()          # saturation rule 0 (no T output)
        assert torch.equal(img0, img), compat
        assert float(img.amax()) > 0.1

        def same(Rx, kw, name):
            a, Ta = Rx.render(cam, mk(**base_kw, **kw), return_T=True)
            assert torch.equal(a, img) and torch.equal(Ta, T), (name, compat, float((a - img).abs().amax()), int((a != img).any(-1).sum()))
            assert torch.equal(Rx.render(cam, mk(**base_kw, **kw)), img), (name, compat, "saturation rule 0")

        same(R, dict(no_footprint_cull=True), "no_footprint_cull")
        assert R.last_stats["n_pairs"] >= stats["n_pairs"]
        same(R, dict(blend_impl=1), "blend_impl=1")
        same(R, dict(blend_impl=1, no_footprint_cull=True), "blend_impl=1 + no_footprint_cull")
        same(R, dict(blend_pipe_tiles=-1), "blend_pipe_tiles=-1")
        same(R, dict(blend_pipe_tiles=1 << 30), "blend_pipe_tiles=max")
        same(R, dict(fine_binning=True), "fine_binning")
        same(R, dict(fine_binning=True, no_footprint_cull=True), "fine_binning + no_footprint_cull")
        same(Rb, dict(), "morton order without bounds")
        same(Rf, dict(), "file order")
        same(Rfb, dict(), "file order with bounds")
        for step, block in ((5, 1), (8, 1), (5, 2), (8, 2)):
            for sp in (1, 2):
                for Rx, name in ((R, "bounds"), (Rb, "no bounds")):
                    a, Ta = _strips(G, Rx, cam, step, block, dict(shard_preprocess=sp, **base_kw), True)
                    assert torch.equal(a, img) and torch.equal(Ta, T), (step, block, sp, name, compat)
            a, _ = _strips(G, R, cam, step, block, dict(no_footprint_cull=True, **base_kw), False)
            assert torch.equal(a, img), (step, block, "no_footprint_cull", compat)
    # three views through one launch sequence: the camera and two sideways shifts, == the single-view frames
    cams = [cam] + [G.renderer.make_camera(s.cam_args[0], np.array([dx, dy, 0.0]), *s.cam_args[2:]) for dx, dy in ((0.013, -0.007), (-0.021, 0.011))]
    singles = torch.stack([R.render(c).clone() for c in cams])
    assert torch.equal(G.renderer.Rasterizer(scene, views=3).render_batch(cams), singles)
    assert torch.equal(G.renderer.Rasterizer(bare, views=3).render_batch(cams, mk(no_footprint_cull=True)), singles)
    assert torch.equal(G.renderer.Rasterizer(scene, views=3).render_batch(cams, mk(blend_impl=1)), singles)


def _explain(s, img, ref, pre, tol=1e-5):
    """Every pixel where the kernel's frame differs from the oracle's by more than `tol` must hold a gaussian the oracle draws whose
    float64 alpha is within 1e-5 relative of 1/255, whose power is within 1e-6 of 0, or whose alpha is within 1e-6 of 0.99 — or,
    for an ill-conditioned conic, within e = 2^-18 (|sx dx^2| / 2 + |sy dy^2| / 2 + |sxy dx dy|), a few ulps of the power's terms,
    of one of those (the kernel evaluates it in a different order, log2 domain, with FMA).  Returns (unexplained, by_kind)."""
    d = np.abs(img.astype(np.float64) - ref.astype(np.float64)).max(axis=-1)
    ys, xs = np.nonzero(d > tol)
    if len(ys) == 0:
        return [], {}
    sg = pre["sigmas"].astype(np.float64)
    mxy = pre["screen_means"].astype(np.float64)
    op = pre["opacity"].astype(np.float64)
    pb = pre["pixel_bboxes"]
    drawn = ((pb[:, 2] - pb[:, 0]) * (pb[:, 3] - pb[:, 1]) != 0) & (sg != 0).all(axis=1) & (pre["cam_means"][:, 2] >= 0.2)
    idx = np.nonzero(drawn)[0]
    unexplained, kinds = [], {"alpha~1/255": 0, "power~0": 0, "alpha~0.99": 0, "ill-conditioned": 0}
    for y, x in zip(ys, xs):
        g = idx[(pb[idx, 0] <= x) & (x < pb[idx, 2]) & (pb[idx, 1] <= y) & (y < pb[idx, 3])]
        dx, dy = mxy[g, 0] - x, mxy[g, 1] - y
        sx, sy, sxy = sg[g, 0], sg[g, 1], sg[g, 2]
        pw = -0.5 * (sx * dx * dx + sy * dy * dy) - sxy * dx * dy
        a = op[g] * np.exp(pw)
        e = 2.0 ** -18 * (np.abs(0.5 * sx * dx * dx) + np.abs(0.5 * sy * dy * dy) + np.abs(sxy * dx * dy))
        c1 = np.abs(255.0 * a - 1.0) < 1e-5
        c2 = np.abs(pw) < 1e-6
        c3 = np.abs(a - 0.99) < 1e-6
        with np.errstate(divide="ignore"):
            c4 = (e > 1e-6) & ((np.abs(np.log(255.0 * a)) < e) | (np.abs(pw) < e) | (np.abs(np.log(a / 0.99)) < e))
        # the conditioning bound also covers the value of a contribution that is drawn by both: 2 alpha (e^e - 1) per gaussian
        c5 = d[y, x] <= 2.0 * np.sum(a * np.expm1(e) * (a > 1.0 / 255.0)) + tol
        for k, c in (("alpha~1/255", c1), ("power~0", c2), ("alpha~0.99", c3), ("ill-conditioned", c4)):
            if c.any():
                kinds[k] += 1
                break
        else:
            if c5:
                kinds["ill-conditioned"] += 1
            else:
                unexplained.append((int(x), int(y), float(d[y, x]), [(int(i), s.meta["pop"][i], float(255 * ai), float(pi), float(ei))
                                                                      for i, ai, pi, ei in zip(g, a, pw, e) if ai > 1e-4][:8]))
    return unexplained, kinds


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", SIZES)
def test_frame_against_the_oracle_accounts_for_every_difference(G, W, H):
    """Flips at the 1/255 step are expected on these scenes, and frequent: every pixel that differs from the oracle by more than 1e-5
    must be explained by a gaussian on a threshold (see _explain); none may differ by more than 4.5e-3.  assert_frames_close holds on
    none of these frames, and is only reported: the scenes put hundreds of pixels on the 1/255 step on purpose (PSNR 95-99 dB against
    its 100) and the needles' ill-conditioned conics make the two fp32 evaluation orders disagree (> 1e-4 of the samples off at
    1283x723)."""
    from gsr_amd import utils

    s, cam, scene = _setup(G, W, H)
    R = G.renderer.Rasterizer(scene)
    img = R.render(cam).cpu().numpy()
    ref, drawn = G.orc.render(utils.pack_gaussians(s.cols), G.orc.camera(*s.cam_args))
    d = np.abs(img.astype(np.float64) - ref)
    unexplained, kinds = _explain(s, img, ref, s.pre)
    n_off = int((d.max(-1) > 1e-5).sum())
    try:
        assert_frames_close(img, ref)
        close = "holds"
    except AssertionError as e:
        close = f"does not hold ({e})"
    print(f"\n{W}x{H}: oracle drew {drawn}; {n_off} pixels off by > 1e-5 (explained: {kinds}), max {d.max():.3g}; "
          f"assert_frames_close {close}")
    assert not unexplained, f"{len(unexplained)} unexplained pixels, e.g. {unexplained[:10]}"
    assert d.max() <= 4.5e-3, d.max()
