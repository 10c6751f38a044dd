"""GPU: renderer.sh_backward (gsr_sh_backward) — the gradient of a view's per-gaussian colours carried to the SH coefficients and,
through the view direction, to the means — and Rasterizer.colour_gradient, the gradient of the colour frame in every array the scene
stores, against the float64 chain of tools/sh_reference.py (with splat_reference's closed form and projection_reference's stage
chain end to end) on the pinned fuzz cases of tools/fuzz_maps.py, in file order and in Morton order, at every SH degree.

tests/test_sh_reference.py holds that chain to autograd and to finite differences first, without a GPU.  The bound is
|err| <= 1e-5 B per element, B = bound64: the same chain with every factor and the upstream in absolute value; entries within
CLAMP_BAND of a clamp edge are left out.  End to end the upstream of the projection's bound is |g| + A + B_splat and that of the SH
chain's |g_rgb| + sum_p w |G|, the feature gradient's own allowance.  Every figure is printed ("sh ..." lines).
"""
import numpy as np
import pytest
import torch

from backward_cases import (DEGREES, FIVE, ORDERS, PINNED, check_colour_end_to_end, check_five as _check_five, check_sh_operator_parity,
                            check_the_dense_and_the_per_lane_path_give_the_same_bits, dev as _dev, fm, pr, sh_case as _case,
                            sh_e2e_case as _e2e_case, sh_expected as _expected, sh_filled as _filled, sh_into as _into,
                            sh_masked as _masked, shr)
from gpu_cases import namespace
from order_scenes import camera_args

pytestmark = pytest.mark.gpu

SIZES = {297: 1, 324: 63, 322: 64, 264: 65, 282: 257, 369: 4096}  # the wave edges of a per-wave LDS path; 282 and 369 hold all-clamped rows


@pytest.fixture(scope="module")
def G():
    return namespace()


def _zeros(n):
    return [torch.zeros((n, 16, 3), device="cuda"), torch.zeros((n, 3), device="cuda")]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_operator_parity(G, seed, order):
    """sh_backward on unit-normal rows on EVERY gaussian against vjp64 at every degree: |err| <= 1e-5 B per element outside the
    band; the file-order result is the scene-order one through scene.order_t."""
    check_sh_operator_parity(G, seed, order)


@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("seed", list(SIZES))
def test_what_is_skipped_is_exact(G, seed, degree):
    """n = 1, 63, 64, 65, 257, 4096: zero rows leave a prefilled out bit for bit, alone and next to touched rows; a clamped channel
    adds nothing to its column of grad_sh; a row with every channel clamped writes nothing; degree d leaves the coefficients
    k >= (d + 1)^2 and, at d = 0, all of grad_means bit for bit."""
    c = _case(G, seed, "morton" if seed != 297 else "file", degree)
    n, K = c["n"], shr.coefficients(degree)
    assert n == SIZES[seed]
    fill = _filled(n)
    out = [f.clone() for f in fill]
    _into(G, c, np.zeros((n, 3), np.float32), out)
    assert all(torch.equal(a, b) for a, b in zip(out, fill))
    g = c["g"].copy()
    g[np.random.default_rng(seed).random(n) < 0.5] = 0.0  # about 32 touched lanes a wave: some waves sparse, some dense, zero rows in both
    _into(G, c, g, out)
    zero = _dev(~g.any(1))
    fw = shr.sh64(c["theta"], c["ocam"], degree)
    clear = fw["band"] > shr.CLAMP_BAND
    clamped = _dev(~fw["m"] & clear)                    # [n, 3]: decided the same way in fp32
    all_clamped = _dev((~fw["m"] & clear).all(1))
    for k, (a, b) in enumerate(zip(out, fill)):
        assert torch.equal(a[zero], b[zero]) and torch.equal(a[all_clamped], b[all_clamped])
        if bool((~zero & ~all_clamped).any()) and (k == 0 or degree > 0):
            assert not torch.equal(a, b)
    sh_out, sh_fill = out[0], fill[0]
    assert torch.equal(sh_out.transpose(1, 2)[clamped], sh_fill.transpose(1, 2)[clamped])
    assert torch.equal(sh_out[:, K:], sh_fill[:, K:])
    passed = _dev(fw["m"] & clear & (g != 0))
    assert not bool((sh_out[:, 0][passed] == sh_fill[:, 0][passed]).any())  # b_0 is never zero: what passes does add
    if degree == 0:
        assert torch.equal(out[1], fill[1])
    if seed in (282, 369) and degree == 3:
        assert bool(all_clamped.any())
    print(f"\nsh seed={seed} degree={degree} kind=skip n={n} zero rows={int(zero.sum())} clamped entries={int(clamped.sum())} "
          f"all-clamped rows={int(all_clamped.sum())}", end="")


@pytest.mark.parametrize("seed", [354, 369])
def test_null_outputs_accumulation_and_repeatability(G, seed):
    """Each output alone is bit for bit that output of the two-output call; two calls into a zeroed out are exactly 2 x one call;
    a second run is bit-identical (no atomics)."""
    c = _case(G, seed, "morton")
    g = _dev(c["g"])
    full = G.renderer.sh_backward(c["scene"], c["cam"], g, scene_order=True)
    again = G.renderer.sh_backward(c["scene"], c["cam"], g, scene_order=True)
    for k, name in enumerate(shr.FIELDS):
        bufs = [None, None]
        bufs[k] = torch.zeros_like(full[k])
        got = _into(G, c, g, bufs)
        assert got[1 - k] is None
        assert torch.equal(got[k], full[k]) and torch.equal(again[k], full[k]) and bool(full[k].any()), name
    with pytest.raises(ValueError, match="at least one"):
        _into(G, c, g, [None, None])
    out = _zeros(c["n"])
    for _ in range(2):
        _into(G, c, g, out)
    assert all(torch.equal(o, 2 * f) for o, f in zip(out, full))


@pytest.mark.parametrize("seed", [264, 369])
def test_a_strided_window_is_read_where_it_lies(G, seed):
    """Columns 7-9 of an [n, 17] tensor give the bits of their contiguous copy."""
    c = _case(G, seed, "morton")
    wide = torch.randn((c["n"], 17), generator=torch.Generator().manual_seed(3)).cuda()
    window = wide[:, 7:10]
    assert window.stride(0) == 17 and not window.is_contiguous()
    a = G.renderer.sh_backward(c["scene"], c["cam"], window, scene_order=True)
    b = G.renderer.sh_backward(c["scene"], c["cam"], window.contiguous(), scene_order=True)
    assert all(torch.equal(x, y) and bool(x.any()) for x, y in zip(a, b))


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("seed,degree", [(369, 3), (369, 2), (369, 1), (369, 0), (282, 3), (322, 3)])
def test_the_dense_and_the_per_lane_path_give_the_same_bits(G, seed, degree, half):
    """Every row touched: each full wave takes the LDS path.  The same rows in four calls, each keeping the lanes of one residue
    mod 4 and zeroing the rest: every wave then has 16 touched lanes, below the dense threshold, and takes the per-lane path.  Row
    for row the same bits, into a prefilled out."""
    check_the_dense_and_the_per_lane_path_give_the_same_bits(G, _case(G, seed, "morton", degree, half))


def test_the_clamp_decision_is_the_forwards(G):
    """The edge scene (degree 0): a value exactly on an edge passes, strictly inside passes, beyond gets nothing — and that is what
    gsr_sh_to_rgb's own output says of the same gaussians."""
    packed, passes = shr.edge_scene()
    scene = G.renderer.GaussianScene.from_packed(packed, sh_degree=0, spatial_order=False)
    R = G.renderer.Rasterizer(scene)
    cam = G.renderer.make_camera(*camera_args(32, 16)[0])
    n = len(passes)
    got = G.renderer.sh_backward(scene, cam, torch.ones((n, 3), device="cuda"), scene_order=True)
    rgb = R._view_colours(cam)[:, 0].cpu().numpy()
    assert rgb[0] == 1 and 0 < rgb[1] < 1 and rgb[2] == 1 and rgb[3] == 0 and 0 < rgb[4] < 1 and rgb[5] == 0
    moved = (got.sh[:, 0, 0] != 0).cpu().numpy()
    assert np.array_equal(moved, passes)
    assert np.array_equal(moved[(rgb > 0) & (rgb < 1)], np.ones(2, bool))  # strictly inside always passes
    assert bool((got.sh[:, 0, 1:] == np.float32(shr.C0)).all()) and not got.sh[:, 1:].any() and not got.means.any()


def test_fp16_storage_is_the_fp32_path_on_the_widened_values(G):
    """seed 354 with the SH rows stored as float16: bit for bit the result of a float32 scene holding the widened coefficients."""
    c = _case(G, 354, "morton", 3, half=True)
    p = dict(c["c"]["packed"])
    p["sh"] = np.ascontiguousarray(np.asarray(p["sh"], np.float32).astype(np.float16).astype(np.float32))
    wide = G.renderer.GaussianScene.from_packed(p, sh_degree=3, spatial_order=True)
    for rows in (c["g"], np.where((np.arange(c["n"]) % 3 == 0)[:, None], c["g"], 0.0).astype(np.float32)):  # dense waves; 21 or 22 touched lanes: sparse waves
        a = G.renderer.sh_backward(c["scene"], c["cam"], _dev(rows), scene_order=True)
        b = G.renderer.sh_backward(wide, c["cam"], _dev(rows), scene_order=True)
        assert all(torch.equal(x, y) and bool(x.any()) for x, y in zip(a, b))
    want, B = shr.vjp64(c["theta"], c["ocam"], 3, c["g"]), shr.bound64(c["theta"], c["ocam"], 3, c["g"])
    keep_sh, keep_means, _ = shr.keep_mask(c["theta"], c["ocam"], 3)
    got = G.renderer.sh_backward(c["scene"], c["cam"], _dev(c["g"]), scene_order=True)
    shr.check_colour("seed=354 kind=fp16 storage", shr.as_dict(got), want, B, dict(sh=keep_sh, means=keep_means))


# ---- end to end: Rasterizer.colour_gradient ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [264, 301, 354, 327, 252])
def test_end_to_end(G, seed):
    """colour_gradient, with grad_T and without, against the float64 chain in all five arrays."""
    check_colour_end_to_end(_e2e_case(G, seed))


@pytest.mark.parametrize("seed", [290, 324, 263])
def test_nothing_passes_gives_exact_zeros(G, seed):
    c = _e2e_case(G, seed, "file")
    got = c["R"].colour_gradient(c["cam"], _dev(c["Gm"]), _dev(c["gT"]))
    assert all(tuple(t.shape)[0] == c["n"] and not t.any() for t in got)


def test_scene_order_and_file_order_agree(G):
    """Through scene.order_t, within the two runs' allowances (the blends' sums are atomic)."""
    c = _e2e_case(G, 252)
    order_t = c["scene"].order_t
    Gz, gTz = _masked(c)
    want, B, keep = _expected(c["geo_file"], c["theta_file"], c["ocam"], c["ref"], Gz, gTz)
    filed = c["R"].colour_gradient(c["cam"], _dev(Gz), _dev(gTz))
    scened = c["R"].colour_gradient(c["cam"], _dev(Gz), _dev(gTz), scene_order=True)
    back = G.renderer.SceneGradient(*[G.renderer.file_order_gradient(t, order_t) for t in scened])
    _check_five("seed=252 kind=scene-order", back, want, B, keep)
    _check_five("seed=252 kind=scene-order against file-order", back, {k: getattr(filed, k).cpu().numpy().astype(np.float64) for k in FIVE},
                {k: 2 * B[k] for k in FIVE}, keep)


def test_out_accumulates_over_two_cameras(G):
    """out= over two cameras of fm.case_views is the sum of the single calls' references, within the sum of their allowances."""
    c = _e2e_case(G, 264)
    R, scene, n = c["R"], c["scene"], c["n"]
    views = fm.case_views(G.orc, c["c"], scene.order)[:2]
    out = G.renderer.SceneGradient(*[torch.zeros((n,) + s, device="cuda") for s in ((3,), (3,), (4,), (), (16, 3))])
    total, bound, kept = None, None, None
    for args, ref in views:
        cam, ocam = G.renderer.make_camera(*args), G.orc.camera(*args)
        Gz, gTz = _masked(c, ref)
        want, B, keep = _expected(c["geo"], c["theta"], ocam, dict(ref, kept=ref["kept_in"]), Gz, gTz)  # everything in the scene's order
        assert R.colour_gradient(cam, _dev(Gz), _dev(gTz), out=out, scene_order=True) is out
        total = want if total is None else {k: total[k] + want[k] for k in FIVE}
        bound = B if bound is None else {k: bound[k] + B[k] for k in FIVE}
        kept = keep if kept is None else {k: kept[k] & keep[k] for k in FIVE}
    assert np.any(total["means"]) and np.any(total["sh"])
    _check_five("seed=264 kind=two cameras", out, total, bound, kept)
    # a field that is None is not computed, and the others are what they are in the full call up to the atomic sums
    part = G.renderer.SceneGradient(None, None, None, None, torch.zeros((n, 16, 3), device="cuda"))
    assert R.colour_gradient(G.renderer.make_camera(*views[0][0]), _dev(_masked(c, views[0][1])[0]), out=part, scene_order=True) is part
    assert part.means is None and bool(part.sh.any())
    with pytest.raises(ValueError, match="at least one"):
        R.colour_gradient(c["cam"], _dev(c["Gm"]), out=G.renderer.SceneGradient(None, None, None, None, None))


def _quadrant_scene():
    """32x16 (two tiles), one small gaussian in the middle of each of the eight 8x8 quadrants, at eight depths: every gaussian's
    pixels lie in one wave of one tile, so the blends' atomic sums have one addend each and are the same in every run.  The SH
    coefficients are small and random: colours inside (0, 1), and a view-direction term that is not zero."""
    W, H = 32, 16
    args, f = camera_args(W, H)
    rng = np.random.default_rng(41)
    cx, cy = np.meshgrid(np.arange(4) * 8 + 3.5, np.arange(2) * 8 + 3.5)
    cx, cy = cx.ravel(), cy.ravel()
    n = len(cx)
    z = 1.0 + 0.01 * rng.permutation(n)
    s = np.log(0.6 * z / f)
    q = rng.normal(size=(n, 4))
    packed = dict(means=np.stack([(cx + 0.5 - 0.5 * W) * z / f, (cy + 0.5 - 0.5 * H) * z / f, z], 1).astype(np.float32),
                  log_scales=np.stack([s + 0.1, s, s - 0.1], 1).astype(np.float32), quats=q.astype(np.float32),
                  opacity_logit=np.zeros(n, np.float32), sh=(0.2 * rng.normal(size=(n, 16, 3))).astype(np.float32))
    return {k: np.ascontiguousarray(v) for k, v in packed.items()}, args


def test_the_one_call_is_the_separate_calls_and_nothing_else_moved(G):
    """colour_gradient equals geometry_gradient on the view's colours, feature_gradient and sh_backward run one after the other, bit
    for bit, on a scene whose atomic sums have one addend; render, render_features and splat_gradient before and after a
    colour_gradient on one Rasterizer are bit for bit the same."""
    packed, args = _quadrant_scene()
    scene = G.renderer.GaussianScene.from_packed(packed)
    R = G.renderer.Rasterizer(scene)
    cam, n = G.renderer.make_camera(*args), len(packed["means"])
    gen = torch.Generator().manual_seed(5)
    Gm = torch.randn((cam.height, cam.width, 3), generator=gen).cuda()
    gT = torch.randn((cam.height, cam.width), generator=gen).cuda()
    F = torch.randn((n, 17), generator=gen).cuda()
    G17 = torch.randn((cam.height, cam.width, 17), generator=gen).cuda()
    before = R.render(cam), R.render_features(cam, F), R.splat_gradient(cam, F, G17, gT)
    got = R.colour_gradient(cam, Gm, gT, scene_order=True)
    assert all(bool(t.any()) for t in got)
    after = R.render(cam), R.render_features(cam, F), R.splat_gradient(cam, F, G17, gT)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]) and bool(before[0].any())
    for a, b in zip(before[2][:3], after[2][:3]):
        assert torch.equal(a, b) and bool(a.any())
    colours = R._view_colours(cam)
    assert bool(((colours > 0) & (colours < 1)).all())
    geo = R.geometry_gradient(cam, colours, Gm, gT, scene_order=True)
    g_rgb = R.feature_gradient(cam, Gm, scene_order=True)
    col = G.renderer.sh_backward(scene, cam, g_rgb, out=G.renderer.ColourGradient(torch.zeros((n, 16, 3), device="cuda"), geo.means))
    assert col.means is geo.means
    for k, name in enumerate(FIVE[:4]):
        assert torch.equal(got[k], geo[k]), name
    assert torch.equal(got.sh, col.sh)
    again = R.colour_gradient(cam, Gm, gT, scene_order=True)  # the scratch is zeroed per call
    assert all(torch.equal(a, b) for a, b in zip(got, again))
