"""GPU: feature, depth and alpha maps (gsr_blend_features / gsr_render_features, Rasterizer.render_features / render_depth /
render_rgbd) against the CPU oracle's compositing loop with the features in the place of the colours.

The reference throughout is orc.preprocess -> orc.depth_order -> orc.composite with pre["rgb"] replaced; the product is compared
with itself only where bit-identity of two product paths is the claim.  Bars: per channel PSNR >= 100 dB with peak = max |oracle
channel| (the project's standing bar for fp32 compositing: the sums are linear in the feature), |T - T_oracle| < 1e-4,
|alpha - (1 - T)| < 1e-5, no pixel excluded.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import psnr
from gpu_cases import MIN_DB, feature_case as _case, medium as _medium, namespace, oracle_maps as _oracle_maps, z_cam as _z_cam

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    return namespace()


def _check_against_oracle(tag, m, T, om, oT):
    dbs = [psnr(m[..., ch], om[..., ch], peak=float(np.abs(om[..., ch]).max())) for ch in range(3)]
    print(f"\n{tag}: depth {dbs[0]:.1f} dB (peak {np.abs(om[..., 0]).max():.3g}), alpha {dbs[1]:.1f} dB, signed {dbs[2]:.1f} dB "
          f"(peak {np.abs(om[..., 2]).max():.3g}); max |T - T_oracle| {np.abs(T - oT).max():.2e}; "
          f"max |alpha - (1 - T)| {np.abs(m[..., 1].astype(np.float64) - (1.0 - T.astype(np.float64))).max():.2e}")
    for ch in range(3):
        assert dbs[ch] >= MIN_DB, (tag, ch, dbs[ch])
    assert np.abs(T - oT).max() < 1e-4, tag
    assert np.abs(m[..., 1].astype(np.float64) - (1.0 - T.astype(np.float64))).max() < 1e-5, tag
    return dbs


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f2", "f3a", "f3b", "medium", "1080p"])
def test_colours_as_features_render_the_colour_frame_bit_for_bit(G, name):
    """Same arithmetic as the colour frame: with the GPU's own per-gaussian colours as features the map is render()'s frame and the
    final T render()'s T, bit for bit — through every colour kernel variant (>= 3000 tiles: two quadrants per wave; <= 1280:
    the pipelined walk; between: the plain walk) and both stop rules (the colour frame without T stops on its colour rule)."""
    c = _case(G, name)
    R, cam = c["R"], c["cam"]
    rgb = R.preprocess_debug(cam)["rgb"]  # file order, like the features render_features expects by default
    rgb = torch.where(torch.isfinite(rgb), rgb, torch.zeros_like(rgb))
    img = R.render(cam)
    img_T, T = R.render(cam, return_T=True)
    m, mT = R.render_features(cam, rgb, return_T=True)
    tiles = ((cam.width + 15) // 16) * ((cam.height + 15) // 16)
    print(f"\n{name}: {tiles} tiles, stats {R.last_stats}")
    assert m.shape == img.shape and m.dtype == torch.float32
    assert torch.equal(m, img) and torch.equal(m, img_T), name
    assert torch.equal(mT, T), name
    assert R.last_stats["colour_evals"] == 0 and R.last_stats["wave_entries"] > 0
    assert torch.equal(R.render_features(cam, rgb), img)  # without the T output too
    if R.scene.order_t is not None:  # ... and told that the features are already in the scene's order
        assert torch.equal(R.render_features(cam, rgb.index_select(0, R.scene.order_t), scene_order=True), img)


# ---- 2, 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f1", "f2", "f3a", "f3b", "f5", "medium"])
def test_depth_alpha_and_a_signed_channel_against_the_oracle(G, name):
    """Features (z_cam, 1, 1000 - 3.5 z_cam) against the oracle's loop over the same values; render_depth is channels 0 and 1 of
    that map bit for bit, and its normalised depth the same torch division of them.
    Measured (MI355X): see DESIGN.md §5.9 for the range of the dB figures this prints."""
    c = _case(G, name)
    R, cam = c["R"], c["cam"]
    m, T = R.render_features(cam, c["Ft"], return_T=True)
    om, oT, _ = _oracle_maps(G, c, c["F"])
    mn, Tn = m.cpu().numpy(), T.cpu().numpy()
    _check_against_oracle(name, mn, Tn, om, oT)
    # Q1: the last column and the last row are never drawn
    assert not mn[-1].any() and not mn[:, -1].any() and (Tn[-1] == 1).all() and (Tn[:, -1] == 1).all()
    assert R.last_stats["colour_evals"] == 0
    # the oracle run is what it should be: something was drawn
    assert (oT < 1).any() and np.abs(om[..., 0]).max() > 0
    depth, alpha = R.render_depth(cam)
    assert depth.shape == (cam.height, cam.width) and torch.equal(depth, m[..., 0]) and torch.equal(alpha, m[..., 1])
    nd, na = R.render_depth(cam, normalize=True)
    assert torch.equal(na, alpha)
    assert torch.equal(nd, torch.where(alpha > 0, depth / alpha, torch.zeros_like(depth)))
    assert bool(torch.isfinite(nd).all()) and float(nd[alpha == 0].abs().max() if (alpha == 0).any() else 0.0) == 0.0


# ---- 4 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f2", "medium"])
def test_rgbd_is_the_colour_frame_plus_the_depth_maps(G, name):
    c = _case(G, name)
    R, cam = c["R"], c["cam"]
    img = R.render(cam)
    depth, alpha = R.render_depth(cam)
    i2, d2, a2 = R.render_rgbd(cam)
    assert torch.equal(i2, img) and torch.equal(d2, depth) and torch.equal(a2, alpha)
    assert R.last_stats["colour_evals"] == 0  # the last blend of render_rgbd is the feature blend
    mk = G.renderer.make_options
    for kw in (dict(reference_compat=False), dict(early_out_T=1e-4), dict(tile_row_begin=1, tile_row_step=2, output_layout=2)):
        i3, d3, a3 = R.render_rgbd(cam, mk(**kw))
        d4, a4 = R.render_depth(cam, mk(**kw))
        assert torch.equal(i3, R.render(cam, mk(**kw))) and torch.equal(d3, d4) and torch.equal(a3, a4), kw


@pytest.mark.parametrize("colour_stage", [0, 1])
def test_a_colour_blend_next_to_a_feature_blend_renders_its_own_bits(G, colour_stage):
    """At the ABI: gsr_blend after (and between) gsr_blend_features on one workspace gives the bits of a gsr_blend alone — the
    feature blend neither evaluates nor disturbs a record's colour — and the feature maps do not depend on what ran before them."""
    from gsr_amd._lib import check, lib

    c = _case(G, "medium")
    R, cam = c["R"], c["cam"]
    H, W, n, dev = cam.height, cam.width, R.scene.n, R.scene.device
    sc, o = R.scene.c_struct(), G.renderer.make_options(colour_stage=colour_stage)
    whole = R.render(cam, o)  # (also sizes the pair buffers to the frame)
    ws = R._workspace(W, H)
    sp = int(torch.cuda.current_stream().cuda_stream)
    F = c["Ft"].index_select(0, R.scene.order_t).contiguous()
    wp, wn, mp = ws.data_ptr(), ws.numel(), R.max_pairs

    def stages12():
        check(lib.gsr_preprocess(C.byref(sc), C.byref(cam), C.byref(o), wp, wn, None, sp))
        check(lib.gsr_bin_sort(n, C.byref(cam), C.byref(o), mp, wp, wn, sp))

    def blend():
        out = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        check(lib.gsr_blend(C.byref(sc), n, C.byref(cam), C.byref(o), mp, wp, wn, out.data_ptr(), None, sp))
        return out

    def features():
        out, T = torch.empty((H, W, 3), dtype=torch.float32, device=dev), torch.empty((H, W), dtype=torch.float32, device=dev)
        check(lib.gsr_blend_features(n, C.byref(cam), C.byref(o), mp, wp, wn, F.data_ptr(), out.data_ptr(), T.data_ptr(), sp))
        return out, T

    stages12()
    alone = blend()
    st_colour = R.stats()
    stages12()
    m1, T1 = features()
    st_feat = R.stats()
    after = blend()
    m2, T2 = features()
    again = blend()
    torch.cuda.synchronize()
    assert torch.equal(after, alone) and torch.equal(again, alone)
    assert torch.equal(m1, m2) and torch.equal(T1, T2)
    assert torch.equal(alone, whole)
    m, T = R.render_features(cam, c["Ft"], o, return_T=True)
    assert torch.equal(m, m1) and torch.equal(T, T1)
    # gsr_read_stats describes the last blend: the feature blend evaluates no colour and stages at least what the colour rule stages
    assert st_feat["colour_evals"] == 0 and st_feat["n_pairs"] == st_colour["n_pairs"]
    assert 0 < st_colour["fetched_entries"] <= st_feat["fetched_entries"] <= st_feat["n_pairs"]
    if colour_stage == 0:
        assert st_colour["colour_evals"] > 0


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def test_every_path_builds_the_default_map(G):
    c = _case(G, "medium")
    R, cam, Ft = c["R"], c["cam"], c["Ft"]
    mk = G.renderer.make_options
    base, baseT = R.render_features(cam, Ft, return_T=True)
    for kw in (dict(fine_binning=True), dict(no_footprint_cull=True), dict(depth_sort_passes=4),
               dict(saturation_rule=1, blend_impl=1, blend_pipe_tiles=-1, no_order_hint=True, colour_stage=1)):  # (the last: ignored options)
        m, T = R.render_features(cam, Ft, mk(**kw), return_T=True)
        assert torch.equal(m, base) and torch.equal(T, baseT), kw
    s, sT = R.render_features(cam, Ft, mk(output_layout=1), return_T=True)
    assert s.shape == (cam.width, cam.height, 3) and torch.equal(s, base.permute(1, 0, 2)) and torch.equal(sT, baseT.t())
    for step in (2, 3, 8):
        for block in (1, 2):
            out, outT = torch.zeros_like(base), torch.zeros_like(baseT)
            for r in range(step):
                strip, sT = R.render_features(cam, Ft, mk(tile_row_begin=r, tile_row_step=step, output_layout=2, tile_row_block=block), return_T=True)
                rows = G.renderer.shard_row_list(cam.height, r, step, block)
                assert strip.shape == (16 * len(rows), cam.width, 3) and sT.shape == (16 * len(rows), cam.width)
                for k, ty in enumerate(rows):
                    h = min(16, cam.height - ty * 16)
                    out[ty * 16: ty * 16 + h] = strip[k * 16: k * 16 + h]
                    outT[ty * 16: ty * 16 + h] = sT[k * 16: k * 16 + h]
            assert torch.equal(out, base) and torch.equal(outT, baseT), (step, block)
    full = R.render_features(cam, Ft, mk(reference_compat=False))
    assert torch.equal(full[:-1, :-1], base[:-1, :-1]) and bool(full[-1].any()) and bool(full[:, -1].any())
    # early_out_T > 0: the bounded approximation of the colour path (a pixel loses at most early_out_T of weight)
    approx = R.render_features(cam, Ft, mk(early_out_T=1e-4))
    assert float((approx[..., 1] - base[..., 1]).abs().max()) <= 1e-4 + 1e-6
    assert R.last_stats["wave_entries"] > 0


@pytest.mark.parametrize("name", ["f2", "f3a"])
def test_progressive_maps_match_the_oracle_prefix(G, name):
    """draw_limit = k composites the first k gaussians of the reference's draw order: the oracle's loop stopped after k."""
    c = _case(G, name)
    R, cam = c["R"], c["cam"]
    _, _, n_drawn = _oracle_maps(G, c, c["F"])
    for k in (1, 7, n_drawn // 3, n_drawn - 1, n_drawn + 50):
        m, T = R.render_features(cam, c["Ft"], G.renderer.make_options(draw_limit=k), return_T=True)
        om, oT, drawn = _oracle_maps(G, c, c["F"], limit=k)
        assert drawn == min(k, n_drawn)
        _check_against_oracle(f"{name} draw_limit={k}", m.cpu().numpy(), T.cpu().numpy(), om, oT)


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_channel_counts_agree_with_single_group_calls(G):
    c = _case(G, "f2")
    R, cam = c["R"], c["cam"]
    gen = torch.Generator().manual_seed(7)
    F7 = (torch.randn((R.scene.n, 7), generator=gen) * 50.0).cuda()
    m7, T7 = R.render_features(cam, F7, return_T=True)
    assert m7.shape == (cam.height, cam.width, 7)
    _, T = R.render(cam, return_T=True)
    assert torch.equal(T7, T)
    for ch in range(7):
        one = R.render_features(cam, F7[:, ch:ch + 1])
        assert one.shape == (cam.height, cam.width, 1) and torch.equal(one[..., 0], m7[..., ch]), ch
    m4 = R.render_features(cam, F7[:, :4])
    assert m4.shape[-1] == 4 and torch.equal(m4, m7[..., :4])
    m3 = R.render_features(cam, F7[:, 3:6].contiguous())
    assert torch.equal(m3, m7[..., 3:6])
    for bad in (F7.double(), F7[:-1], F7[:, :0], F7.cpu(), F7.view(-1)):
        with pytest.raises((ValueError, RuntimeError)):
            R.render_features(cam, bad)


def test_spatial_order_changes_no_bit_of_a_tie_free_scene(G):
    """File-order features on the Morton-ordered scene (gathered through GaussianScene.order) against the file-order scene: the
    same map bit for bit once no two gaussians share a depth (ties are drawn in storage order, include/gsr.h)."""
    packed, args = _medium(G, n=150_000)
    cam = G.renderer.make_camera(*args)
    z = _z_cam(G, cam, packed["means"])
    _, first = np.unique(z, return_index=True)  # one gaussian per depth value: removing the others changes nobody else's depth
    keep = np.sort(first)
    packed = {k: np.ascontiguousarray(v[keep]) for k, v in packed.items()}
    z = z[keep]
    assert len(np.unique(z)) == len(z) > 140_000
    F = torch.from_numpy(np.stack([z, np.ones_like(z), np.float32(1000.0) - np.float32(3.5) * z], 1).astype(np.float32)).cuda()
    plain_scene = G.renderer.GaussianScene.from_packed(packed, spatial_order=False)
    scene = G.renderer.GaussianScene.from_packed(packed)
    assert plain_scene.order is None and scene.order is not None and not np.array_equal(scene.order, np.arange(len(z)))
    a, Ta = G.renderer.Rasterizer(plain_scene).render_features(cam, F, return_T=True)
    b, Tb = G.renderer.Rasterizer(scene).render_features(cam, F, return_T=True)
    assert torch.equal(a, b) and torch.equal(Ta, Tb)
    assert float(a[..., 1].max()) > 0.5


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_late_saturation_is_exact(G):
    """An opaque wall in front of a long list: the T == 0.0f stop fires (fewer entries staged than the lists hold) and changes no
    bit — the map equals the one built from the reference's full 3-sigma rects, whose longer lists stop elsewhere — and the map
    holds the oracle's, which blends every gaussian."""
    c = _case(G, "wall")
    R, cam = c["R"], c["cam"]
    m, T = R.render_features(cam, c["Ft"], G.renderer.make_options(early_out_T=0.0), return_T=True)
    st = dict(R.last_stats)
    m2, T2 = R.render_features(cam, c["Ft"], G.renderer.make_options(no_footprint_cull=True), return_T=True)
    assert torch.equal(m, m2) and torch.equal(T, T2)
    every, Te = R.render_features(cam, c["Ft"], G.renderer.make_options(early_out_T=-1.0), return_T=True)  # never stops
    assert torch.equal(every, m) and torch.equal(Te, T) and R.last_stats["fetched_entries"] > st["fetched_entries"]
    print(f"\nopaque wall: staged {st['fetched_entries']} of {st['n_pairs']} entries, evaluated {st['wave_entries']} (quadrant, entry) pairs; "
          f"without the stop {R.last_stats['fetched_entries']} / {R.last_stats['wave_entries']}")
    assert st["fetched_entries"] < st["n_pairs"] and bool((T == 0).any())
    om, oT, _ = _oracle_maps(G, c, c["F"])
    _check_against_oracle("opaque wall", m.cpu().numpy(), T.cpu().numpy(), om, oT)


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_degenerate_inputs(G):
    """n = 0, frames smaller than a tile, a single gaussian, everything culled."""
    p = G.synthetic.look_at_pose((0, -4, 0.5), (0, 0, 0), 1, "x.png")
    for (W, H) in ((10, 7), (16, 16), (33, 17)):
        fx = G.synthetic.pinhole_focal(W)
        args = (p.qvec, p.tvec, 2 * fx, 2 * fx, 2 * W, 2 * H, W, H)
        cam, ocam = G.renderer.make_camera(*args), G.orc.camera(*args)
        for n in (0, 1, 300):
            cols = G.synthetic.mip360_like(max(n, 1), 3)
            for i in range(3):
                cols[f"scale_{i}"] = (cols[f"scale_{i}"] + np.float32(3.0)).astype(np.float32)
            packed = G.utils.pack_gaussians({k: v[:n] for k, v in cols.items()})
            R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(packed))
            z = _z_cam(G, cam, packed["means"]) if n else np.zeros(0, np.float32)
            F = np.stack([z, np.ones_like(z), np.float32(1000.0) - np.float32(3.5) * z], 1).astype(np.float32).reshape(n, 3)
            m, T = R.render_features(cam, torch.from_numpy(F).cuda(), return_T=True)
            assert m.shape == (H, W, 3) and T.shape == (H, W)
            if n == 0:
                assert not m.any() and bool((T == 1).all())
                d, a = R.render_depth(cam)
                assert not d.any() and not a.any()
                i3, d3, a3 = R.render_rgbd(cam)
                assert not i3.any() and not d3.any() and not a3.any()
                continue
            cs = dict(packed=packed, cam=cam, ocam=ocam)
            om, oT, drawn = _oracle_maps(G, cs, F)
            if drawn:
                _check_against_oracle(f"{W}x{H} n={n}", m.cpu().numpy(), T.cpu().numpy(), om, oT)
            else:
                assert not m.any() and bool((T == 1).all())
    # every gaussian behind the camera
    cols = G.synthetic.mip360_like(500, 4)
    cols["y"] = (cols["y"] - np.float32(100.0)).astype(np.float32)  # the camera at y = -4 looks along +y
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols))
    m, T = R.render_features(cam, torch.ones((500, 5), device="cuda"), return_T=True)
    assert m.shape == (cam.height, cam.width, 5) and not m.any() and bool((T == 1).all())
    assert R.last_stats["n_visible"] == 0 and R.last_stats["n_pairs"] == 0 and R.last_stats["wave_entries"] == 0
    d, a = R.render_depth(cam, normalize=True)
    assert not d.any() and not a.any()
