"""GPU: the depth-bounded feature blend (gsr_blend_slab / gsr_render_slab, Rasterizer.render_slab / render_occluded) — per pixel the
gaussians with near[p] <= z_i < far[p] only, T starting at 1 at the near limit.

References, none of them the code under test:
  - open limits: R.render_features itself (the three-channel and the many-channel blend), bit for bit, counters included;
  - far limits: channel i of R.render_features(cam, eye(n)) IS w_i(p), and a far limit removes only LATER gaussians,
    so the slab's weights are W * (z_i < far[p]) exactly, whatever the limit of the pixel is;
  - near and far: the same scene with opacity_logit = -30 for the gaussians outside a constant slab [a, b) — they are culled
    (opacity <= 1/255) while the scene order, the tie order and the draw count stay — rendered by R.render_features under the same
    options; per-pixel planes draw a slab per pixel and expect each pixel from its slab's render.  torch.equal on map and T;
  - independent of every GPU kernel: the CPU oracle's compositing loop over the masked arrays, with the standing bars of
    tests/test_gpu_features.py (per channel PSNR >= 100 dB, |T - T_oracle| < 1e-4).
z_i is preprocess_debug(cam)["cam_means"][:, 2]; "visible" gaussians are those with a positive weight somewhere in the frame.
"""
import numpy as np
import pytest
import torch

from conftest import psnr
from gpu_cases import custom_case as _custom_case, feature_case as _case, namespace, pick_case as _pick_case, wall_scene as _wall_scene

pytestmark = pytest.mark.gpu

INF = float("inf")
FIXTURES = ["f1", "f3a", "f3b"]
WIDTH_OF = {"f1": 5, "f3a": 3, "f3b": 19, "deep": 8, "wall": 4}  # channels of the near-and-far tests: every walk width (8, 4, 16 + 4, 8, 4)


@pytest.fixture(scope="module")
def G():
    return namespace()


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def _slab_case(G, name):
    """The fixture's case with z (file order, device), the one-hot weights W1 / T1, the visible gaussians and their sorted depths."""
    if name == "wall":
        packed, args, _ = _wall_scene()
        c = _custom_case(G, "slab_wall", packed, args)
    else:
        c = _pick_case(G, name)
    if "z" not in c:
        R, cam = c["R"], c["cam"]
        n, dev = R.scene.n, R.scene.device
        c["z"] = R.preprocess_debug(cam)["cam_means"][:, 2].contiguous()
        c["eye"] = torch.eye(n, dtype=torch.float32, device=dev)
        c["W1"], c["T1"] = R.render_features(cam, c["eye"], return_T=True)
        c["seen"] = (c["W1"] > 0).flatten(0, 1).any(0)
        c["zs"] = c["z"][c["seen"]].sort().values
        gen = torch.Generator().manual_seed(1234)
        c["Fwide"] = torch.randn((n, 19), generator=gen, dtype=torch.float32).to(dev)  # file order
        c["masked"] = {}
    return c


def _features(c, C):
    return c["Fwide"][:, :C].contiguous()


def _masked(G, c, a, b):
    """A Rasterizer on the scene with the gaussians outside [a, b) switched off (opacity_logit = -30), and its packed arrays."""
    key = (float(a), float(b))
    if key not in c["masked"]:
        z = c["z"].cpu().numpy()
        keep = (z >= np.float32(a)) & (z < np.float32(b))
        packed = dict(c["packed"])
        packed["opacity_logit"] = np.where(keep, packed["opacity_logit"], np.float32(-30.0)).astype(np.float32)
        c["masked"][key] = (G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(packed)), packed)
    return c["masked"][key]


def _reference(G, c, a, b, F, opts=None, **kw):
    """(map, T, stats) of the masked scene under the same options."""
    Rm, _ = _masked(G, c, a, b)
    m, T = Rm.render_features(c["cam"], F, opts, return_T=True, **kw)
    return m, T, dict(Rm.last_stats)


def _quantile_z(c, q):
    """The depth of a visible gaussian at quantile q of the visible depths: every edge lies exactly on a gaussian's z."""
    zs = c["zs"]
    return float(zs[min(int(q * len(zs)), len(zs) - 1)])


def _slabs(c):
    z10, z30, z50, z70, z90 = (_quantile_z(c, q) for q in (0.1, 0.3, 0.5, 0.7, 0.9))
    assert z10 < z30 < z50 < z70 < z90
    #        far only      near only    both        empty (far < near)  both, narrow  both, late
    return [(-INF, z50), (z30, INF), (z10, z70), (z70, z30), (z30, z50), (z50, z90)]


def _plane(shape, value, dev):
    return torch.full(shape, value, dtype=torch.float32, device=dev)


def _limits(a, b, shape, dev):
    """Constant planes for the slab [a, b); an open side is passed as None."""
    return (None if a == -INF else _plane(shape, a, dev)), (None if b == INF else _plane(shape, b, dev))


# ---- 1: open limits change no bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_open_limits_are_the_feature_blend_bit_for_bit(G, name):
    c = _slab_case(G, name)
    R, cam = c["R"], c["cam"]
    dev, shape = R.scene.device, (cam.height, cam.width)
    for C in (3, 5, 8, 19):  # the three-channel blend; the channel blend's walks of 8, 8 and 16 + 3 — against walks of 4, 8, 8, 16 + 4
        F = _features(c, C)
        m, T = R.render_features(cam, F, return_T=True)
        st = dict(R.last_stats)
        for near, far in ((None, None), (_plane(shape, -INF, dev), _plane(shape, INF, dev)), (None, _plane(shape, INF, dev))):
            sm, sT = R.render_slab(cam, F, near=near, far=far)
            assert sm.shape == m.shape and sm.dtype == torch.float32
            assert torch.equal(sm, m) and torch.equal(sT, T), (name, C)
            assert R.last_stats["wave_entries"] == st["wave_entries"] and R.last_stats["fetched_entries"] == st["fetched_entries"], (name, C)
            assert R.last_stats["colour_evals"] == 0
        assert torch.equal(R.render_slab(cam, F, return_T=False), m)
        assert st["wave_entries"] > 0


# ---- 2: arbitrary per-pixel far limits, exact -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_per_pixel_far_limits_keep_exactly_the_weights_in_front(G, name):
    """far[p] is drawn, with a fixed seed, from the z of the pixel's own heaviest gaussian (which excludes it) and its nextafter (which
    includes it), from every visible z_i and its nextafter, and from +inf, -1, 0.2 and NaN: neighbouring pixels of one quadrant
    disagree, and a z that differed from the sort's by one ulp would move a gaussian across its own limit."""
    c = _slab_case(G, name)
    R, cam = c["R"], c["cam"]
    dev, H, Wd = R.scene.device, cam.height, cam.width
    z, W1, zs = c["z"], c["W1"], c["zs"]
    gen = torch.Generator().manual_seed(77)
    up = lambda t: torch.nextafter(t, torch.full_like(t, INF))
    pool = torch.cat([zs, up(zs)])
    far = pool[torch.randint(0, len(pool), (H, Wd), generator=gen).to(dev)]
    r = torch.rand((H, Wd), generator=gen).to(dev)
    covered = (W1 > 0).any(-1)
    zbest = z[W1.argmax(-1)]
    far = torch.where(covered & (r < 0.35), zbest, far)
    far = torch.where(covered & (r >= 0.35) & (r < 0.70), up(zbest), far)
    special = torch.tensor([INF, -1.0, 0.2, float("nan")], dtype=torch.float32, device=dev)
    pick = torch.randint(0, 4, (H, Wd), generator=gen).to(dev)
    far = torch.where(r >= 0.90, special[pick], far).contiguous()
    inside = z.view(1, 1, -1) < far.unsqueeze(-1)  # NaN: nobody
    exp = W1 * inside
    # on the reference: covered pixels with contributors on both sides of their limit, pixels whose limit is a contributor's own z
    # and ones whose limit is the float after it, and a quadrant that holds a NaN next to a finite limit
    has = W1 > 0
    assert int(((has & inside).any(-1) & (has & ~inside).any(-1)).sum()) > 20
    assert int((covered & (far == zbest)).sum()) > 20 and int((covered & (far == up(zbest))).sum()) > 20
    blocks = far[: H // 8 * 8, : Wd // 8 * 8].reshape(H // 8, 8, Wd // 8, 8).permute(0, 2, 1, 3).reshape(H // 8, Wd // 8, 64)
    assert bool((blocks.isnan().any(-1) & blocks.isfinite().any(-1)).any())
    got, T = R.render_slab(cam, c["eye"], far=far)
    assert torch.equal(got, exp), name
    assert not got[far.isnan()].any() and bool((T[far.isnan()] == 1).all())
    assert bool((T[far == -1.0] == 1).all()) and bool((T[far == 0.2] == 1).all())
    assert torch.equal(T[far == INF], c["T1"][far == INF])


# ---- 3: near and far, map and T, exact ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_near_and_far_limits_against_the_masked_scene(G, name):
    c = _slab_case(G, name)
    R, cam = c["R"], c["cam"]
    dev, shape = R.scene.device, (cam.height, cam.width)
    F = _features(c, WIDTH_OF[name])
    slabs = _slabs(c)
    refs = []
    for a, b in slabs:
        m, T, st = _reference(G, c, a, b, F)
        refs.append((m, T))
        near, far = _limits(a, b, shape, dev)
        sm, sT = R.render_slab(cam, F, near=near, far=far)
        print(f"\n{name} [{a}, {b}): wave_entries / fetched_entries {R.last_stats['wave_entries']} / {R.last_stats['fetched_entries']}, "
              f"masked scene {st['wave_entries']} / {st['fetched_entries']}")
        assert torch.equal(sm, m) and torch.equal(sT, T), (name, a, b)
        assert R.last_stats["wave_entries"] == st["wave_entries"], (name, a, b)
    # the inputs are not trivial: with far at the median visible z most of the frame's T differs from the unbounded one
    changed = float((refs[0][1] != c["T1"]).float().mean())
    print(f"{name}: far at the median visible z changes T on {changed:.3f} of the pixels")
    assert changed > {"f1": 0.4, "f3a": 0.9, "f3b": 0.9}[name]
    assert not refs[3][0].any() and bool((refs[3][1] == 1).all())  # the empty slab
    # per-pixel planes: a slab per pixel, each pixel expected from its slab's render
    gen = torch.Generator().manual_seed(5)
    idx = torch.randint(0, len(slabs), shape, generator=gen).to(dev)
    lo = torch.tensor([s[0] for s in slabs], dtype=torch.float32, device=dev)[idx].contiguous()
    hi = torch.tensor([s[1] for s in slabs], dtype=torch.float32, device=dev)[idx].contiguous()
    exp_m = torch.stack([m for m, _ in refs])[idx, torch.arange(shape[0], device=dev).view(-1, 1), torch.arange(shape[1], device=dev).view(1, -1)]
    exp_T = torch.stack([T for _, T in refs])[idx, torch.arange(shape[0], device=dev).view(-1, 1), torch.arange(shape[1], device=dev).view(1, -1)]
    sm, sT = R.render_slab(cam, F, near=lo, far=hi)
    assert torch.equal(sm, exp_m) and torch.equal(sT, exp_T), name
    assert bool((sm != refs[0][0]).any()) and bool((sm != refs[1][0]).any())


# ---- 4: stop and skip -----------------------------------------------------------------------------------------------------------
def test_a_far_limit_stops_the_fetch_and_a_near_limit_skips_the_walk(G):
    c = _slab_case(G, "deep")
    R, cam = c["R"], c["cam"]
    dev, shape = R.scene.device, (cam.height, cam.width)
    F = _features(c, WIDTH_OF["deep"])
    R.render_features(cam, F)
    st = dict(R.last_stats)
    zall = c["z"].sort().values
    assert len(zall) == 1000 and st["fetched_entries"] > 1000  # more than one batch per tile, more than one tile
    zf, zn = float(zall[300]), float(zall[700])
    m, T, _ = _reference(G, c, -INF, zf, F)
    sm, sT = R.render_slab(cam, F, far=_plane(shape, zf, dev))
    far_st = dict(R.last_stats)
    assert torch.equal(sm, m) and torch.equal(sT, T)
    assert far_st["fetched_entries"] < st["fetched_entries"] and far_st["wave_entries"] < st["wave_entries"]
    m, T, _ = _reference(G, c, zn, INF, F)
    sm, sT = R.render_slab(cam, F, near=_plane(shape, zn, dev))
    near_st = dict(R.last_stats)
    assert torch.equal(sm, m) and torch.equal(sT, T)
    assert near_st["wave_entries"] < st["wave_entries"]
    print(f"\ndeep: wave_entries / fetched_entries  feature blend {st['wave_entries']} / {st['fetched_entries']}, far at rank 300 "
          f"{far_st['wave_entries']} / {far_st['fetched_entries']}, near at rank 700 {near_st['wave_entries']} / {near_st['fetched_entries']}")


def test_behind_an_opaque_wall(G):
    """near just behind the sixth (last nearly opaque) gaussian: what the wall hides from the unbounded frame is drawn at full T."""
    c = _slab_case(G, "wall")
    R, cam = c["R"], c["cam"]
    dev, shape = R.scene.device, (cam.height, cam.width)
    F = _features(c, WIDTH_OF["wall"])
    zall = c["z"].sort().values
    near = float(torch.nextafter(zall[5], torch.tensor(INF, device=dev)))
    m, T, _ = _reference(G, c, near, INF, F)
    sm, sT = R.render_slab(cam, F, near=_plane(shape, near, dev))
    assert torch.equal(sm, m) and torch.equal(sT, T)
    full_T = c["T1"]
    assert bool((sT[:-1, :-1] > full_T[:-1, :-1]).all())  # the wall is gone
    # ... and with near ON the sixth gaussian's z it is still part of the slab
    m6, T6, _ = _reference(G, c, float(zall[5]), INF, F)
    s6, sT6 = R.render_slab(cam, F, near=_plane(shape, float(zall[5]), dev))
    assert torch.equal(s6, m6) and torch.equal(sT6, T6) and not torch.equal(sT6, sT)


# ---- 5: options -----------------------------------------------------------------------------------------------------------------
def _strip(G, plane, H, rows, fill):
    """An [H, W, ...] image-layout tensor in the strip layout of the tile rows `rows`; rows below the frame hold `fill`."""
    out = torch.full((16 * len(rows),) + tuple(plane.shape[1:]), fill, dtype=plane.dtype, device=plane.device)
    for j, ty in enumerate(rows):
        h = min(16, H - ty * 16)
        out[j * 16: j * 16 + h] = plane[ty * 16: ty * 16 + h]
    return out


def test_layouts_shards_and_list_options(G):
    c = _slab_case(G, "f3a")
    R, cam, mk = c["R"], c["cam"], G.renderer.make_options
    dev, H, Wd = R.scene.device, cam.height, cam.width
    F = _features(c, 5)
    slabs = [_slabs(c)[i] for i in (0, 1, 2)]
    gen = torch.Generator().manual_seed(9)
    idx = torch.randint(0, len(slabs), (H, Wd), generator=gen).to(dev)
    lo = torch.tensor([s[0] for s in slabs], dtype=torch.float32, device=dev)[idx].contiguous()
    hi = torch.tensor([s[1] for s in slabs], dtype=torch.float32, device=dev)[idx].contiguous()
    ii, jj = torch.arange(H, device=dev).view(-1, 1), torch.arange(Wd, device=dev).view(1, -1)

    def expected(opts, sel=None, **kw):
        refs = [_reference(G, c, a, b, F, opts, **kw) for a, b in slabs]
        sel = idx if sel is None else sel
        r, q = torch.arange(sel.shape[0], device=dev).view(-1, 1), torch.arange(sel.shape[1], device=dev).view(1, -1)
        return torch.stack([m for m, _, _ in refs])[sel, r, q], torch.stack([T for _, T, _ in refs])[sel, r, q]

    base_m, base_T = expected(None)
    sm, sT = R.render_slab(cam, F, near=lo, far=hi)
    assert torch.equal(sm, base_m) and torch.equal(sT, base_T)
    assert bool((sm != 0).any())
    # [W, H]: the planes follow the layout of T
    em, eT = expected(mk(output_layout=1), sel=idx.t().contiguous())
    sm, sT = R.render_slab(cam, F, near=lo.t().contiguous(), far=hi.t().contiguous(), opts=mk(output_layout=1))
    assert sm.shape == (Wd, H, 5) and torch.equal(sm, em) and torch.equal(sT, eT)
    assert torch.equal(sm, base_m.transpose(0, 1)) and torch.equal(sT, base_T.t())
    # strips: the whole frame, and tile-row shards (begin 1, step 2) in blocks of 1 and 2 rows; rows below the frame are never read
    for begin, step, block in ((0, 1, 0), (1, 2, 1), (1, 2, 2)):
        o = mk(tile_row_begin=begin, tile_row_step=step, output_layout=2, tile_row_block=block)
        rows = G.renderer.shard_row_list(H, begin, step, block)
        assert rows and (step == 1 or len(rows) < (H + 15) // 16)
        em, eT = expected(o, sel=_strip(G, idx, H, rows, 0))
        sm, sT = R.render_slab(cam, F, near=_strip(G, lo, H, rows, float("nan")), far=_strip(G, hi, H, rows, float("nan")), opts=o)
        assert sm.shape == (16 * len(rows), Wd, 5) and torch.equal(sm, em) and torch.equal(sT, eT), (begin, step, block)
        assert torch.equal(sm, _strip(G, base_m, H, rows, 0.0)) and torch.equal(sT, _strip(G, base_T, H, rows, 1.0))
    # the lists built another way, the frame's last column / row drawn, a draw limit, an approximate early out
    for kw in (dict(fine_binning=True), dict(no_footprint_cull=True)):
        sm, sT = R.render_slab(cam, F, near=lo, far=hi, opts=mk(**kw))
        assert torch.equal(sm, base_m) and torch.equal(sT, base_T), kw
    for kw in (dict(reference_compat=False), dict(draw_limit=7), dict(draw_limit=60), dict(draw_limit=150), dict(early_out_T=1e-2)):
        em, eT = expected(mk(**kw))
        sm, sT = R.render_slab(cam, F, near=lo, far=hi, opts=mk(**kw))
        assert torch.equal(sm, em) and torch.equal(sT, eT), kw
        if "draw_limit" in kw or "reference_compat" in kw:
            assert not torch.equal(sm, base_m), kw
    assert bool((expected(mk(reference_compat=False))[0][-1] != 0).any())  # the last row is drawn there
    # features in the scene's order, and a column window of a wider tensor read in place
    assert R.scene.order_t is not None
    Fs = F.index_select(0, R.scene.order_t)
    sm, sT = R.render_slab(cam, Fs, near=lo, far=hi, scene_order=True)
    assert torch.equal(sm, base_m) and torch.equal(sT, base_T)
    wide = torch.full((R.scene.n, 12), 7.5, dtype=torch.float32, device=dev)
    wide[:, 2:7] = Fs
    window = wide[:, 2:7]
    assert not window.is_contiguous()
    sm, sT = R.render_slab(cam, window, near=lo, far=hi, scene_order=True)
    assert torch.equal(sm, base_m) and torch.equal(sT, base_T)


def test_degenerate_inputs_and_overflow(G):
    p = G.synthetic.look_at_pose((0, -4, 0.5), (0, 0, 0), 1, "x.png")
    W, H = 33, 17
    fx = G.synthetic.pinhole_focal(W)
    cam = G.renderer.make_camera(p.qvec, p.tvec, 2 * fx, 2 * fx, 2 * W, 2 * H, W, H)
    cols = G.synthetic.mip360_like(300, 3)
    for i in range(3):
        cols[f"scale_{i}"] = (cols[f"scale_{i}"] + np.float32(3.0)).astype(np.float32)
    empty = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(G.utils.pack_gaussians({k: v[:0] for k, v in cols.items()})))
    behind = dict(cols)
    behind["y"] = (behind["y"] - np.float32(100.0)).astype(np.float32)  # every gaussian behind the camera
    culled = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(behind))
    lo, hi = torch.full((H, W), 1.0, device="cuda"), torch.full((H, W), 5.0, device="cuda")
    for R, n in ((empty, 0), (culled, 300)):
        for C in (3, 9):
            m, T = R.render_slab(cam, torch.ones((n, C), device="cuda"), near=lo, far=hi)
            assert m.shape == (H, W, C) and not m.any() and bool((T == 1).all())
    assert culled.last_stats["n_visible"] == 0 and culled.last_stats["wave_entries"] == 0
    # a pair buffer too small: re-rendered, the same map as a roomy one
    c = _slab_case(G, "f3a")
    R, cam3 = c["R"], c["cam"]
    shape, dev = (cam3.height, cam3.width), R.scene.device
    a, b = _slabs(c)[2]
    F = _features(c, 5)
    small = G.renderer.Rasterizer(R.scene, max_pairs=64)
    got = small.render_slab(cam3, F, near=_plane(shape, a, dev), far=_plane(shape, b, dev))
    want = R.render_slab(cam3, F, near=_plane(shape, a, dev), far=_plane(shape, b, dev))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and bool(got[0].any())
    assert small.max_pairs > 64
    with pytest.raises(ValueError):
        R.render_slab(cam3, F, far=_plane((cam3.width, cam3.height), b, dev))
    with pytest.raises(ValueError):
        R.render_slab(cam3, F, far=_plane(shape, b, dev).cpu())
    with pytest.raises(ValueError):
        R.render_slab(cam3, F.clone().requires_grad_(True))


def test_the_blend_alone_with_and_without_the_scene(G):
    """gsr_blend_slab after gsr_preprocess and gsr_bin_sort: handed the scene, or NULL (the means are then found through the pointer
    the preprocess left in the workspace), several times on the same lists — the map gsr_render_slab renders."""
    import ctypes as C

    from gsr_amd._lib import check, lib

    c = _slab_case(G, "f3a")
    R, cam = c["R"], c["cam"]
    dev, H, Wd = R.scene.device, cam.height, cam.width
    F = _features(c, 5)
    a, b = _slabs(c)[2]
    near, far = _plane((H, Wd), a, dev), _plane((H, Wd), b, dev)
    want_m, want_T = R.render_slab(cam, F, near=near, far=far)
    full_m, full_T = R.render_features(cam, F, return_T=True)
    R2 = G.renderer.Rasterizer(R.scene)
    ws, sc, o = R2._workspace(Wd, H), R.scene.c_struct(), G.renderer.make_options()
    sp = int(torch.cuda.current_stream(dev).cuda_stream)
    rows = F.index_select(0, R.scene.order_t).contiguous()
    n, mp, wp, wn = R.scene.n, R2.max_pairs, ws.data_ptr(), ws.numel()
    check(lib.gsr_preprocess(C.byref(sc), C.byref(cam), C.byref(o), wp, wn, None, sp))
    check(lib.gsr_bin_sort(n, C.byref(cam), C.byref(o), mp, wp, wn, sp))
    for scene_p, lo, hi, em, eT in ((None, near, far, want_m, want_T), (C.byref(sc), near, far, want_m, want_T),
                                    (None, None, None, full_m, full_T), (None, near, far, want_m, want_T)):
        m = torch.full((H, Wd, 5), -7.0, dtype=torch.float32, device=dev)
        T = torch.full((H, Wd), -7.0, dtype=torch.float32, device=dev)
        check(lib.gsr_blend_slab(scene_p, n, C.byref(cam), C.byref(o), mp, wp, wn, rows.data_ptr(), 5, 5,
                                 lo.data_ptr() if lo is not None else None, hi.data_ptr() if hi is not None else None,
                                 m.data_ptr(), T.data_ptr(), sp))
        assert torch.equal(m, em) and torch.equal(T, eT), scene_p is None
    # without the final T
    m = torch.full((H, Wd, 5), -7.0, dtype=torch.float32, device=dev)
    check(lib.gsr_blend_slab(None, n, C.byref(cam), C.byref(o), mp, wp, wn, rows.data_ptr(), 5, 5, near.data_ptr(), far.data_ptr(),
                             m.data_ptr(), None, sp))
    assert torch.equal(m, want_m)


# ---- 6: the colour frame in front of a depth buffer -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f2", "f3a"])
def test_render_occluded(G, name):
    c = _case(G, name)
    R, cam = c["R"], c["cam"]
    dev, shape = R.scene.device, (cam.height, cam.width)
    img, T = R.render(cam, return_T=True)
    oi, oT = R.render_occluded(cam, _plane(shape, INF, dev))
    assert torch.equal(oi, img) and torch.equal(oi, R.render(cam)) and torch.equal(oT, T), name
    # a real depth buffer: the median surface, pushed back by 5 %, nothing where no surface was found
    zm = R.render_median_depth(cam)
    depth = torch.where(zm > 0, 1.05 * zm, torch.full_like(zm, INF)).contiguous()
    oi, oT = R.render_occluded(cam, depth)
    rgb = R.preprocess_debug(cam)["rgb"]
    rgb = torch.where(torch.isfinite(rgb), rgb, torch.zeros_like(rgb))
    sm, sT = R.render_slab(cam, rgb, far=depth)
    assert torch.equal(oi, sm) and torch.equal(oT, sT)
    assert bool((oT[:-1, :-1] >= T[:-1, :-1]).all()) and bool((oT > T).any())
    for bg in (torch.tensor([0.25, 0.5, 1.0], device=dev), torch.rand(shape + (3,), generator=torch.Generator().manual_seed(3)).to(dev)):
        bi, bT = R.render_occluded(cam, depth, bg)
        assert torch.equal(bT, oT) and torch.equal(bi, G.renderer.composite_over(oi, oT, bg))
        assert torch.equal(bi, oi + oT.unsqueeze(-1) * bg)


# ---- 7: independent of every GPU kernel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_slabs_against_the_cpu_oracle(G, name):
    """The oracle's compositing loop over the masked arrays with (z_cam, 1, 1000 - 3.5 z_cam) in the place of the colours."""
    c = _slab_case(G, name)
    _case(G, name)  # (the features F / Ft)
    R, cam, orc = c["R"], c["cam"], G.orc
    dev, shape = R.scene.device, (cam.height, cam.width)
    for a, b in [_slabs(c)[i] for i in (0, 1, 2)]:
        _, packed = _masked(G, c, a, b)
        pre = orc.preprocess(packed, c["ocam"])
        pre["rgb"] = np.ascontiguousarray(c["F"], np.float32)
        screen, trans, drawn = orc.composite(orc.depth_order(pre["cam_means"]), pre, cam.width, cam.height, threads=orc.max_threads())
        om, oT = screen.transpose(1, 0, 2), trans.transpose(1, 0)
        near, far = _limits(a, b, shape, dev)
        m, T = R.render_slab(cam, c["Ft"], near=near, far=far)
        m, T = m.cpu().numpy(), T.cpu().numpy()
        dbs = [psnr(m[..., ch], om[..., ch], peak=float(np.abs(om[..., ch]).max())) for ch in range(3)]
        print(f"\n{name} [{a}, {b}): {dbs[0]:.1f} / {dbs[1]:.1f} / {dbs[2]:.1f} dB, max |T - T_oracle| {np.abs(T - oT).max():.2e}, oracle drew {drawn}")
        assert np.abs(om[..., 1]).max() > 0.1
        assert all(db >= 100.0 for db in dbs), (name, a, b, dbs)
        assert np.abs(T - oT).max() < 1e-4, (name, a, b)
