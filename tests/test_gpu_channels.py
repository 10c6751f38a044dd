"""GPU: many channels per walk of the tile lists (gsr_blend_channels / gsr_render_channels, csrc/blend_channels.hip;
Rasterizer.render_features with more than three channels).

The claim is bit-identity with the three-channel feature kernel (gsr_blend_features, which these tests reach through
render_features with one to three channels — the code of that kernel is the parent's), channel by channel, at any option; the
oracle (orc.composite with pre["rgb"] replaced, three channels at a time) is the second, independent reference with the project's
standing bars: per channel PSNR >= 100 dB with peak = max |oracle channel|, |T - T_oracle| < 1e-4.

Channel counts: with the instantiated widths CH_MIN = 8 and CH_MAX = 16, C in {4, 7, 8, 9, 16, 17, 33} is a lone partial group, a
full narrow group, a remainder of one after a full group, and three groups.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import psnr
from gpu_cases import MIN_DB, build as _build, namespace, z_cam as _z_cam

pytestmark = pytest.mark.gpu

CH_MIN, CH_MAX = 8, 16  # the widths csrc/blend_channels.hip instantiates
COUNTS = (4, CH_MIN - 1, CH_MIN, CH_MIN + 1, CH_MAX, CH_MAX + 1, 2 * CH_MAX + 1)
C_ALL = max(COUNTS)


@pytest.fixture(scope="module")
def G():
    return namespace()


def _case(G, name):
    """The scene, its Rasterizer, and C_ALL feature columns in file order: randn * 50 with column 1 = z_cam and column 2 = ones.
    The references are computed once and only read: `one(c)`, channel c as a map of its own through the three-channel kernel, and
    render()'s T."""
    if name not in G.cases:
        packed, args = _build(G, name)
        cam, ocam = G.renderer.make_camera(*args), G.orc.camera(*args)
        R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(packed))
        n = R.scene.n
        F = (torch.randn((n, C_ALL), generator=torch.Generator().manual_seed(11)) * 50.0).numpy()
        z = _z_cam(G, cam, packed["means"])
        F[:, 1] = np.where(np.isfinite(z), z, 0.0)
        F[:, 2] = 1.0
        c = dict(packed=packed, cam=cam, ocam=ocam, R=R, F=F, Ft=torch.from_numpy(F).cuda(), ones={})
        _, c["T"] = R.render(cam, return_T=True)

        def one(ch, c=c):
            if ch not in c["ones"]:
                c["ones"][ch] = R.render_features(cam, c["Ft"][:, ch:ch + 1])[..., 0].clone()
            return c["ones"][ch]

        c["one"] = one
        G.cases[name] = c
    return G.cases[name]


def _scene_order(c, F):
    """File-order values -> the order of the scene's resident arrays."""
    o = c["R"].scene.order_t
    return (F if o is None else F.index_select(0, o)).contiguous()


def _groups_of_three(R, cam, F, o, return_T=False):
    """The parent's path under the same options: ceil(C / 3) maps of at most three channels, joined."""
    maps = [R.render_features(cam, F[:, c0:c0 + 3], o) for c0 in range(0, F.shape[1], 3)]
    m = torch.cat(maps, -1)
    if return_T:
        return m, R.render_features(cam, F[:, :1], o, return_T=True)[1]
    return m


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_ch", [(s, k) for s in ("f2", "f3a", "f3b", "f5") for k in COUNTS]
                         + [(s, k) for s in ("medium", "wall") for k in (CH_MIN - 1, CH_MAX, 2 * CH_MAX + 1)])
def test_every_channel_is_the_three_channel_kernels_bit_for_bit(G, name, n_ch):
    c = _case(G, name)
    R, cam = c["R"], c["cam"]
    m, T = R.render_features(cam, c["Ft"][:, :n_ch], return_T=True)
    st = dict(R.last_stats)
    assert m.shape == (cam.height, cam.width, n_ch) and m.dtype == torch.float32 and m.is_contiguous()
    assert torch.equal(T, c["T"]), (name, n_ch)
    for ch in range(n_ch):
        assert torch.equal(m[..., ch], c["one"](ch)), (name, n_ch, ch)
    assert torch.equal(R.render_features(cam, c["Ft"][:, :n_ch]), m)  # without the T output too
    assert st["colour_evals"] == 0 and st["wave_entries"] > 0
    assert bool((m[..., 2] > 0).any()) and float((m[..., 2] - (1 - T)).abs().max()) < 1e-5  # the column of ones is the alpha map
    if name == "wall":  # every quadrant reaches T == 0 long before its list ends: the stop fires, and no bit moves (above)
        assert st["fetched_entries"] < st["n_pairs"] and bool((T == 0).any())


# ---- 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f1", "f2", "f3a", "f5"])
def test_against_the_oracle(G, name):
    """CH_MAX + 1 channels (a full wide walk and a narrow walk of one) against the oracle's loop over the same values, three at a
    time.  Measured (MI355X): DESIGN.md §5.11 has the range of the dB figures this prints."""
    c = _case(G, name)
    R, cam, n_ch = c["R"], c["cam"], CH_MAX + 1
    m, T = R.render_features(cam, c["Ft"][:, :n_ch], return_T=True)
    mn, Tn = m.cpu().numpy(), T.cpu().numpy()
    pre = G.orc.preprocess(c["packed"], c["ocam"])
    order = G.orc.depth_order(pre["cam_means"])
    for c0 in range(0, n_ch, 3):
        f3 = np.zeros((len(c["F"]), 3), np.float32)
        k = min(3, n_ch - c0)
        f3[:, :k] = c["F"][:, c0:c0 + k]
        screen, trans, drawn = G.orc.composite(order, dict(pre, rgb=f3), cam.width, cam.height, limit=-1, threads=G.orc.max_threads())
        om, oT = screen.transpose(1, 0, 2), trans.transpose(1, 0)
        assert drawn > 0 and (oT < 1).any()
        for j in range(k):
            peak = float(np.abs(om[..., j]).max())
            db = psnr(mn[..., c0 + j], om[..., j], peak=peak)
            print(f"\n{name}: channel {c0 + j}: {db:.1f} dB (peak {peak:.3g})", end="")
            assert peak > 0 and db >= MIN_DB, (name, c0 + j, db)
        dT = float(np.abs(Tn - oT).max())
        print(f"\n{name}: max |T - T_oracle| {dT:.2e}", end="")
        assert dT < 1e-4, name


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def _abi(G, c, o=None):
    """Stages 1-2 on the Rasterizer's workspace, and callables for the stage-3 entry points on it."""
    from gsr_amd._lib import check, lib

    R, cam = c["R"], c["cam"]
    o = o or G.renderer.make_options()
    R.render(cam, o)  # sizes the pair buffers to the frame
    ws = R._workspace(cam.width, cam.height)
    sc, sp = R.scene.c_struct(), int(torch.cuda.current_stream().cuda_stream)
    H, W, n, dev = cam.height, cam.width, R.scene.n, R.scene.device
    wp, wn, mp = ws.data_ptr(), ws.numel(), R.max_pairs

    class A:
        pass

    a = A()

    def stages12():
        check(lib.gsr_preprocess(C.byref(sc), C.byref(cam), C.byref(o), wp, wn, None, sp))
        check(lib.gsr_bin_sort(n, C.byref(cam), C.byref(o), mp, wp, wn, sp))

    def channels(ptr, n_ch, stride, want_T=True):
        out = torch.empty((H, W, n_ch), dtype=torch.float32, device=dev)
        T = torch.empty((H, W), dtype=torch.float32, device=dev) if want_T else None
        check(lib.gsr_blend_channels(n, C.byref(cam), C.byref(o), mp, wp, wn, ptr, n_ch, stride, out.data_ptr(),
                                     T.data_ptr() if want_T else None, sp))
        return out, T

    def features(F3):
        out, T = torch.empty((H, W, 3), dtype=torch.float32, device=dev), torch.empty((H, W), dtype=torch.float32, device=dev)
        check(lib.gsr_blend_features(n, C.byref(cam), C.byref(o), mp, wp, wn, F3.data_ptr(), out.data_ptr(), T.data_ptr(), sp))
        return out, T

    def blend():
        out = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        check(lib.gsr_blend(C.byref(sc), n, C.byref(cam), C.byref(o), mp, wp, wn, out.data_ptr(), None, sp))
        return out

    a.stages12, a.channels, a.features, a.blend = stages12, channels, features, blend
    return a


def test_strides_and_alignment_change_no_bit(G):
    """A column window F12[:, 1:8] of an [n, 12] tensor (base 4 B off a 16-byte boundary, rows 48 B apart), its contiguous copy
    (stride 7: odd, no row but the first on a 16-byte boundary) and the same values in the first 7 columns of an [n, 8] tensor (every
    row aligned: 16-byte loads for the first four channels) give one map; so do 8 channels read through 16-byte loads and through
    the window.  Once at the ABI, once through render_features(scene_order=True), which hands the window over without a copy."""
    c = _case(G, "f2")
    R, cam = c["R"], c["cam"]
    n = R.scene.n
    F12 = _scene_order(c, c["Ft"][:, :12])
    assert F12.data_ptr() % 16 == 0 and F12.stride() == (12, 1)
    win7, win8 = F12[:, 1:8], F12[:, 1:9]
    odd7 = win7.contiguous()
    pad8 = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    pad8[:, :7] = win7
    al8 = win8.contiguous()
    assert win7.data_ptr() % 16 == 4 and odd7.stride(0) == 7 and al8.data_ptr() % 16 == 0
    a = _abi(G, c)
    a.stages12()
    m_win, T_win = a.channels(win7.data_ptr(), 7, 12)
    m_odd, T_odd = a.channels(odd7.data_ptr(), 7, 7)
    m_pad, T_pad = a.channels(pad8.data_ptr(), 7, 8)
    m_w8, _ = a.channels(win8.data_ptr(), 8, 12)
    m_a8, _ = a.channels(al8.data_ptr(), 8, 8)
    torch.cuda.synchronize()
    assert torch.equal(m_win, m_odd) and torch.equal(m_win, m_pad) and torch.equal(m_w8, m_a8) and torch.equal(m_w8[..., :7], m_win)
    assert torch.equal(T_win, c["T"]) and torch.equal(T_odd, c["T"]) and torch.equal(T_pad, c["T"])
    for ch in range(8):
        assert torch.equal(m_w8[..., ch], c["one"](1 + ch)), ch  # ... and that map is the three-channel kernel's
    # the host path: no copy of a tensor the library can read where it lies, one copy otherwise
    assert R._feature_rows(win7, True).data_ptr() == win7.data_ptr() and R._feature_rows(odd7, True).data_ptr() == odd7.data_ptr()
    wide = F12[:, ::2]  # element stride 2: one .contiguous()
    rows = R._feature_rows(wide, True)
    assert rows.data_ptr() != wide.data_ptr() and rows.is_contiguous() and torch.equal(rows, wide)
    assert torch.equal(R.render_features(cam, win7, scene_order=True), m_win)
    assert torch.equal(R.render_features(cam, odd7, scene_order=True), m_win)
    assert torch.equal(R.render_features(cam, win8, scene_order=True), m_w8)
    assert torch.equal(R.render_features(cam, wide, scene_order=True)[..., 1], c["one"](2))


# ---- 4 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f2", "medium"])
def test_every_path_builds_the_default_map(G, name):
    c = _case(G, name)
    R, cam, F = c["R"], c["cam"], c["Ft"][:, :7]
    mk = G.renderer.make_options
    base, baseT = R.render_features(cam, F, return_T=True)
    n_drawn = R.last_stats["n_visible"]
    assert n_drawn > 8
    for kw in (dict(fine_binning=True), dict(no_footprint_cull=True), dict(depth_sort_passes=4)):
        m, T = R.render_features(cam, F, mk(**kw), return_T=True)
        assert torch.equal(m, base) and torch.equal(T, baseT), kw
    s, sT = R.render_features(cam, F, mk(output_layout=1), return_T=True)
    assert s.shape == (cam.width, cam.height, 7) and torch.equal(s, base.permute(1, 0, 2)) and torch.equal(sT, baseT.t())
    for step in (2, 3):
        for block in (1, 2):
            out, outT = torch.zeros_like(base), torch.zeros_like(baseT)
            for r in range(step):
                strip, sT = R.render_features(cam, F, mk(tile_row_begin=r, tile_row_step=step, output_layout=2, tile_row_block=block), return_T=True)
                rows = G.renderer.shard_row_list(cam.height, r, step, block)
                assert strip.shape == (16 * len(rows), cam.width, 7) and sT.shape == (16 * len(rows), cam.width)
                for k, ty in enumerate(rows):
                    h = min(16, cam.height - ty * 16)
                    out[ty * 16: ty * 16 + h] = strip[k * 16: k * 16 + h]
                    outT[ty * 16: ty * 16 + h] = sT[k * 16: k * 16 + h]
            assert torch.equal(out, base) and torch.equal(outT, baseT), (step, block)
    full = R.render_features(cam, F, mk(reference_compat=False))
    assert torch.equal(full[:-1, :-1], base[:-1, :-1]) and bool(full[-1].any()) and bool(full[:, -1].any())
    assert not base[-1].any() and not base[:, -1].any() and bool((baseT[-1] == 1).all()) and bool((baseT[:, -1] == 1).all())  # Q1
    # options that change the map: bit for bit the three-channel path's under the same option
    for kw in (dict(draw_limit=1), dict(draw_limit=7), dict(draw_limit=n_drawn - 1), dict(early_out_T=1e-4)):
        m, T = R.render_features(cam, F, mk(**kw), return_T=True)
        m3, T3 = _groups_of_three(R, cam, F, mk(**kw), return_T=True)
        assert torch.equal(m, m3) and torch.equal(T, T3), kw
        if "draw_limit" in kw and kw["draw_limit"] <= 7:
            assert not torch.equal(m, base), kw  # (the option took effect)


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def test_neighbours_on_the_workspace(G):
    """At the ABI with colour_stage = 0: a gsr_blend after gsr_blend_channels renders the bits of a gsr_blend alone (the records'
    colour words and the launch-order hint are left alone), and gsr_read_stats describes one walk: the counters of
    gsr_blend_features on the same lists."""
    c = _case(G, "medium")
    R = c["R"]
    a = _abi(G, c, G.renderer.make_options(colour_stage=0))
    F = _scene_order(c, c["Ft"][:, :CH_MAX + 1])
    a.stages12()
    alone = a.blend()
    a.stages12()
    m1, T1 = a.channels(F.data_ptr(), CH_MAX + 1, CH_MAX + 1)
    st_ch = R.stats()
    after = a.blend()
    m2, T2 = a.channels(F.data_ptr(), CH_MAX + 1, CH_MAX + 1)
    again = a.blend()
    a.stages12()
    m3, T3 = a.features(F[:, :3].contiguous())
    st_f3 = R.stats()
    torch.cuda.synchronize()
    assert torch.equal(after, alone) and torch.equal(again, alone)
    assert torch.equal(m1, m2) and torch.equal(T1, T2)
    assert torch.equal(m1[..., :3], m3) and torch.equal(T1, T3)
    assert st_ch["colour_evals"] == 0 and st_ch["wave_entries"] > 0
    for k in ("wave_entries", "fetched_entries", "n_pairs", "n_visible"):
        assert st_ch[k] == st_f3[k], (k, st_ch, st_f3)


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_degenerate_inputs(G):
    """n = 0, a 5x3 frame, everything culled, one channel at the ABI, GSR_MAX_FEATURE_CHANNELS channels."""
    p = G.synthetic.look_at_pose((0, -4, 0.5), (0, 0, 0), 1, "x.png")
    W, H = 5, 3
    fx = G.synthetic.pinhole_focal(W)
    cam = G.renderer.make_camera(p.qvec, p.tvec, 2 * fx, 2 * fx, 2 * W, 2 * H, W, H)
    cols = G.synthetic.mip360_like(300, 3)
    for i in range(3):
        cols[f"scale_{i}"] = (cols[f"scale_{i}"] + np.float32(3.0)).astype(np.float32)
    gen = torch.Generator().manual_seed(3)
    for n in (0, 300):
        packed = G.utils.pack_gaussians({k: v[:n] for k, v in cols.items()})
        R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(packed))
        F = (torch.randn((n, CH_MIN + 1), generator=gen) * 50.0).cuda()
        m, T = R.render_features(cam, F, return_T=True)
        assert m.shape == (H, W, CH_MIN + 1) and T.shape == (H, W)
        if n == 0:
            assert not m.any() and bool((T == 1).all())
        else:
            _, T0 = R.render(cam, return_T=True)
            assert torch.equal(T, T0)
            for ch in range(CH_MIN + 1):
                assert torch.equal(m[..., ch], R.render_features(cam, F[:, ch:ch + 1])[..., 0]), ch
    # every gaussian behind the camera
    cols = G.synthetic.mip360_like(500, 4)
    cols["y"] = (cols["y"] - np.float32(100.0)).astype(np.float32)  # the camera at y = -4 looks along +y
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols))
    m, T = R.render_features(cam, torch.ones((500, CH_MAX + 1), device="cuda"), return_T=True)
    assert m.shape == (H, W, CH_MAX + 1) and not m.any() and bool((T == 1).all())
    assert R.last_stats["n_visible"] == 0 and R.last_stats["n_pairs"] == 0 and R.last_stats["wave_entries"] == 0
    # one channel at the ABI (render_features sends it to the three-channel kernel)
    c = _case(G, "f1")
    a = _abi(G, c)
    a.stages12()
    col = _scene_order(c, c["Ft"][:, 4:5])
    m1, T1 = a.channels(col.data_ptr(), 1, 1)
    torch.cuda.synchronize()
    assert m1.shape[-1] == 1 and torch.equal(m1[..., 0], c["one"](4)) and torch.equal(T1, c["T"])
    # the widest map: channel j carries column j % C_ALL
    R, cam = c["R"], c["cam"]
    n_max = G.lib.GSR_MAX_FEATURE_CHANNELS
    Fmax = c["Ft"].repeat(1, -(-n_max // C_ALL))[:, :n_max].contiguous()
    mm, Tm = R.render_features(cam, Fmax, return_T=True)
    assert mm.shape == (cam.height, cam.width, n_max) and torch.equal(Tm, c["T"])
    ref = torch.stack([c["one"](ch) for ch in range(C_ALL)], -1)
    assert torch.equal(mm, ref.repeat(1, 1, -(-n_max // C_ALL))[..., :n_max])
    with pytest.raises(ValueError):
        R.render_features(cam, torch.zeros((R.scene.n, n_max + 1), device="cuda"))
