"""GPU: the gradient of a feature map with respect to the per-gaussian features (gsr_blend_channels_backward /
gsr_render_channels_backward, csrc/blend_channels_backward.hip; Rasterizer.feature_gradient, blend_weights and autograd through
render_features).

out[p][c] = sum_i w_i(p) f_i[c] is linear in f, so the gradient is the exact transpose gF[i][c] = sum_p w_i(p) G[p][c] and can be
checked against the oracle without touching it: orc.composite with pre["rgb"] set to three one-hot columns returns the weight maps
w_i(.) of three gaussians, and the reference is sum_p w_i(p) G[p, c] in float64.  A gaussian writes only inside its pixel bbox, so
for the large scenes the depth order handed to orc.composite ends with the last of the three and is restricted to the gaussians
whose bbox meets one of theirs: for the three's weights the oracle then performs the same operations in the same order (one
triple per scene is checked bit for bit against the whole order).

The bar is the project's standing one: per channel PSNR >= MIN_DB = 100 dB of the GPU block against the oracle block with
peak = max |oracle block channel|, no gaussian excluded.  G is randn from a seeded generator, C = 17: a full wide walk plus a narrow
walk of one.  Float atomic sums depend on arrival order: equality between two runs is never asserted.
Measured (MI355X): DESIGN.md §5.12 has the range of the dB figures these tests print.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_cases import N_CH, N_SAMPLE, bar as _bar, gradient_case as _case, namespace, sample as _sample, weight_maps as _weight_maps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    return namespace()


def _reference(G, c, ids, restrict):
    """For the gaussians `ids` (file order): (sum_p w_i(p) Gm[p, :] [len(ids), N_CH], sum_p w_i(p) [len(ids)]) in float64."""
    key = (tuple(ids[:4]), len(ids), restrict)
    if key not in c["refs"]:
        if restrict:  # the restriction changes no bit
            assert np.array_equal(_weight_maps(G, c, ids[:3], False), _weight_maps(G, c, ids[:3], True))
        w = _weight_maps(G, c, ids, restrict).astype(np.float64).reshape(len(ids), -1)
        gm = c["Gm"].numpy().astype(np.float64).reshape(-1, N_CH)
        c["refs"][key] = (w @ gm, w.sum(1))
    return c["refs"][key]


# ---- 1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f1", "f3a", "f3b"])
def test_against_the_oracle_every_gaussian(G, name):
    c = _case(G, name)
    R, cam = c["R"], c["cam"]
    ids = np.arange(R.scene.n)
    ref, wsum = _reference(G, c, ids, False)
    g = R.feature_gradient(cam, c["Gt"])
    assert g.shape == (R.scene.n, N_CH) and g.dtype == torch.float32
    gn = g.cpu().numpy()
    assert (wsum > 0).sum() >= 8, name
    _bar(name, gn, ref)
    never = wsum == 0
    assert never.any() and not gn[never].any(), name  # gaussians the oracle never draws: exactly 0
    assert R.last_stats["wave_entries"] > 0 and R.last_stats["colour_evals"] == 0


# ---- 2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f2", "f5", "medium", "wall"])
def test_against_the_oracle_sampled(G, name):
    c = _case(G, name)
    R, cam = c["R"], c["cam"]
    ids = _sample(c, name)
    ref, wsum = _reference(G, c, ids, True)
    assert len(ids) == N_SAMPLE and (wsum > 0).sum() >= N_SAMPLE // 2, (name, len(ids), int((wsum > 0).sum()))
    gn = R.feature_gradient(cam, c["Gt"]).cpu().numpy()
    st = dict(R.last_stats)
    _bar(name, gn[ids], ref)
    if name == "wall":  # every quadrant stops early, and lists run past one batch of 256 entries
        assert st["fetched_entries"] < st["n_pairs"]


# ---- 3 ------------------------------------------------------------------------------------------------------------------
def _adjoint(tag, maps, Fs, Gm, gF, gFabs):
    """|<A F, G> - <F, A^T G>| <= 1e-5 sum |F| (A^T |G|) for every (map = A F, F) pair, sums in float64."""
    Gd, gd, ga = Gm.double(), gF.double(), gFabs.double()
    for k, (m, F) in enumerate(zip(maps, Fs)):
        lhs = float((m.double() * Gd).sum())
        rhs = float((F.double() * gd).sum())
        bound = 1e-5 * float((F.double().abs() * ga).sum())
        print(f"\n{tag}[{k}]: <AF,G> {lhs:.9g}  <F,AtG> {rhs:.9g}  |diff| {abs(lhs - rhs):.3g}  bound {bound:.3g}", end="")
        assert bound > 0 and abs(lhs - rhs) <= bound, (tag, k, lhs, rhs, bound)


@pytest.mark.parametrize("name", ["medium", "wall"])
def test_adjoint_identity_against_the_oracles_forward(G, name):
    c = _case(G, name)
    R, cam = c["R"], c["cam"]
    Gm = c["Gt"][..., :3].contiguous()
    gF, gFabs = R.feature_gradient(cam, Gm), R.feature_gradient(cam, Gm.abs())
    gen = torch.Generator().manual_seed(31)
    Fs = [torch.randn((R.scene.n, 3), generator=gen) * (1.0 + 10.0 * k) for k in range(4)]
    maps = []
    for F in Fs:
        screen, _, _ = G.orc.composite(c["order"], dict(c["pre"], rgb=F.numpy()), cam.width, cam.height, limit=-1, threads=G.orc.max_threads())
        maps.append(torch.from_numpy(np.ascontiguousarray(screen.transpose(1, 0, 2))))
    _adjoint(name, maps, Fs, Gm.cpu(), gF.cpu(), gFabs.cpu())


# ---- 4 ------------------------------------------------------------------------------------------------------------------
def test_autograd_through_render_features(G):
    c = _case(G, "f2")
    R, cam = c["R"], c["cam"]
    f = c["Ft"][:, :N_CH].clone().requires_grad_()
    m = R.render_features(cam, f)
    assert m.requires_grad and m.grad_fn is not None
    assert torch.equal(m.detach(), R.render_features(cam, f.detach()))
    (m * c["Gt"]).sum().backward()
    assert f.grad is not None and f.grad.shape == f.shape
    ids = _sample(c, "f2")  # test_against_the_oracle_sampled's reference
    ref, _ = _reference(G, c, ids, True)
    _bar("f2 autograd", f.grad.cpu().numpy()[ids], ref)
    for n_ch in (1, 3, 2 * N_CH - 1):
        gm = torch.randn((cam.height, cam.width, n_ch), generator=torch.Generator().manual_seed(n_ch)).cuda()
        f = c["Ft"][:, :n_ch].clone().requires_grad_()
        m = R.render_features(cam, f)
        assert m.requires_grad and torch.equal(m.detach(), R.render_features(cam, f.detach()))
        (m * gm).sum().backward()
        _bar(f"f2 autograd C={n_ch}", f.grad.cpu().numpy(), R.feature_gradient(cam, gm).cpu().numpy())
        assert bool(f.grad.any())
    f = c["Ft"][:, :N_CH].clone().requires_grad_()
    m, T = R.render_features(cam, f, return_T=True)
    assert m.requires_grad and not T.requires_grad
    with torch.no_grad():
        assert R.render_features(cam, f).grad_fn is None
    assert R.render_features(cam, f.detach()).grad_fn is None


# ---- 5 ------------------------------------------------------------------------------------------------------------------
def test_order_and_layout(G):
    c = _case(G, "f2")
    R, cam, Gt = c["R"], c["cam"], c["Gt"]
    o_t, n = R.scene.order_t, R.scene.n
    assert o_t is not None  # the scene was reordered: file order and scene order differ
    base = R.feature_gradient(cam, Gt)
    bn = base.cpu().numpy()
    so = R.feature_gradient(cam, Gt, scene_order=True)
    _bar("scene_order", so.cpu().numpy(), base.index_select(0, o_t).cpu().numpy())
    # autograd with scene_order=True on a column window of a wider tensor: read in place, gradient in those columns only
    wide = torch.zeros((n, 40), device="cuda")
    wide[:, 4:4 + N_CH] = c["Ft"][:, :N_CH].index_select(0, o_t)
    wide.requires_grad_()
    m = R.render_features(cam, wide[:, 4:4 + N_CH], scene_order=True)
    assert torch.equal(m.detach(), R.render_features(cam, c["Ft"][:, :N_CH]))
    (m * Gt).sum().backward()
    assert not wide.grad[:, :4].any() and not wide.grad[:, 4 + N_CH:].any()
    _bar("window", wide.grad[:, 4:4 + N_CH].cpu().numpy(), so.cpu().numpy())
    mk = G.renderer.make_options
    g1 = R.feature_gradient(cam, Gt.permute(1, 0, 2).contiguous(), mk(output_layout=1))
    _bar("layout 1", g1.cpu().numpy(), bn)
    acc = torch.zeros((n, N_CH), device="cuda")
    for r in range(2):
        rows = G.renderer.shard_row_list(cam.height, r, 2, 1)
        strip = torch.zeros((16 * len(rows), cam.width, N_CH), device="cuda")
        for k, ty in enumerate(rows):
            h = min(16, cam.height - ty * 16)
            strip[k * 16: k * 16 + h] = Gt[ty * 16: ty * 16 + h]
        assert R.feature_gradient(cam, strip, mk(tile_row_begin=r, tile_row_step=2, output_layout=2), out=acc) is acc
    _bar("two strips", acc.cpu().numpy(), so.cpu().numpy())


# ---- 6 ------------------------------------------------------------------------------------------------------------------
def test_options_keep_it_the_transpose_of_the_forward(G):
    """Under each option the gradient is the transpose of what the GPU forward (the parent's code) computes under that option."""
    c = _case(G, "medium")
    R, cam = c["R"], c["cam"]
    Gm = c["Gt"][..., :3].contiguous()
    R.render(cam)
    n_drawn = R.last_stats["n_visible"]
    assert n_drawn > 8
    gen = torch.Generator().manual_seed(37)
    Fs = [(torch.randn((R.scene.n, 3), generator=gen) * 20.0).cuda() for _ in range(2)]
    mk = G.renderer.make_options
    base = R.feature_gradient(cam, Gm)
    for kw in (dict(fine_binning=True), dict(no_footprint_cull=True), dict(draw_limit=n_drawn // 2), dict(reference_compat=False),
               dict(early_out_T=1e-4)):
        gF, gFabs = R.feature_gradient(cam, Gm, mk(**kw)), R.feature_gradient(cam, Gm.abs(), mk(**kw))
        maps = [R.render_features(cam, F, mk(**kw)) for F in Fs]
        _adjoint(str(kw), [m.cpu() for m in maps], [F.cpu() for F in Fs], Gm.cpu(), gF.cpu(), gFabs.cpu())
        if "draw_limit" in kw or "reference_compat" in kw:
            assert not torch.equal(gF, base), kw  # (the option took effect)


# ---- 7 ------------------------------------------------------------------------------------------------------------------
def test_blend_weights(G):
    c = _case(G, "f3a")
    R, cam = c["R"], c["cam"]
    n = R.scene.n
    _, wsum = _reference(G, c, np.arange(n), False)
    w = R.blend_weights(cam)
    assert w.shape == (n,) and w.dtype == torch.float32
    _bar("blend_weights", w.cpu().numpy(), wsum)
    out = torch.zeros(n, device="cuda")
    assert R.blend_weights(cam, out=out) is out
    R.blend_weights(cam, out=out)
    o_t = R.scene.order_t
    scene_w = w if o_t is None else w.index_select(0, o_t)
    _bar("blend_weights twice", out.cpu().numpy(), 2.0 * scene_w.cpu().numpy().astype(np.float64))
    _, T = R.render(cam, return_T=True)
    total, alpha = float(w.double().sum()), float((1.0 - T.double()).sum())  # undrawn pixels keep T = 1
    print(f"\nsum of blend weights {total:.9g}, sum of 1 - T {alpha:.9g}", end="")
    assert alpha > 0 and abs(total - alpha) <= 1e-5 * alpha


# ---- 8 ------------------------------------------------------------------------------------------------------------------
def test_neighbours_on_the_workspace(G):
    """At the ABI: a gsr_blend before and after a backward on one workspace renders its own bits, and gsr_read_stats afterwards
    describes the walk with the forward's counters."""
    from gsr_amd._lib import check, lib

    c = _case(G, "medium")
    R, cam = c["R"], c["cam"]
    o = G.renderer.make_options(colour_stage=0)
    R.render(cam, o)  # sizes the pair buffers to the frame
    ws = R._workspace(cam.width, cam.height)
    sc, sp = R.scene.c_struct(), int(torch.cuda.current_stream().cuda_stream)
    n, wp, wn, mp = R.scene.n, ws.data_ptr(), ws.numel(), R.max_pairs

    def stages12():
        check(lib.gsr_preprocess(C.byref(sc), C.byref(cam), C.byref(o), wp, wn, None, sp))
        check(lib.gsr_bin_sort(n, C.byref(cam), C.byref(o), mp, wp, wn, sp))

    def blend():
        out = torch.empty((cam.height, cam.width, 3), dtype=torch.float32, device="cuda")
        check(lib.gsr_blend(C.byref(sc), n, C.byref(cam), C.byref(o), mp, wp, wn, out.data_ptr(), None, sp))
        return out

    def backward(stride):
        g = torch.zeros((n, stride), dtype=torch.float32, device="cuda")
        check(lib.gsr_blend_channels_backward(n, C.byref(cam), C.byref(o), mp, wp, wn, c["Gt"].data_ptr(), N_CH, g.data_ptr(), stride, sp))
        return g

    stages12()
    alone = blend()
    stages12()
    g1 = backward(N_CH)
    st_b = R.stats()
    after = blend()
    g2 = backward(N_CH + 3)  # rows further apart than wide
    again = blend()
    F = torch.zeros((n, N_CH), device="cuda")
    m = torch.empty((cam.height, cam.width, N_CH), dtype=torch.float32, device="cuda")
    check(lib.gsr_blend_channels(n, C.byref(cam), C.byref(o), mp, wp, wn, F.data_ptr(), N_CH, N_CH, m.data_ptr(), None, sp))
    st_f = R.stats()
    torch.cuda.synchronize()
    assert torch.equal(after, alone) and torch.equal(again, alone)
    assert not g2[:, N_CH:].any()
    _bar("two runs", g2[:, :N_CH].cpu().numpy(), g1.cpu().numpy())
    _bar("abi vs feature_gradient", g1.cpu().numpy(), R.feature_gradient(cam, c["Gt"], scene_order=True).cpu().numpy())
    for k in ("wave_entries", "fetched_entries", "n_pairs", "n_visible"):
        assert st_b[k] == st_f[k] and st_b[k] > 0, (k, st_b, st_f)


def test_degenerate_inputs(G):
    """n = 0, a 5x3 frame, everything culled, GSR_MAX_FEATURE_CHANNELS channels."""
    p = G.synthetic.look_at_pose((0, -4, 0.5), (0, 0, 0), 1, "x.png")
    W, H = 5, 3
    fx = G.synthetic.pinhole_focal(W)
    cam = G.renderer.make_camera(p.qvec, p.tvec, 2 * fx, 2 * fx, 2 * W, 2 * H, W, H)
    cols = G.synthetic.mip360_like(300, 3)
    for i in range(3):
        cols[f"scale_{i}"] = (cols[f"scale_{i}"] + np.float32(3.0)).astype(np.float32)
    gm = torch.randn((H, W, 9), generator=torch.Generator().manual_seed(3)).cuda()
    for n in (0, 300):
        packed = G.utils.pack_gaussians({k: v[:n] for k, v in cols.items()})
        R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(packed))
        g = R.feature_gradient(cam, gm)
        assert g.shape == (n, 9)
        f = torch.randn((n, 9), generator=torch.Generator().manual_seed(5)).cuda().requires_grad_()
        m = R.render_features(cam, f)
        (m * gm).sum().backward()
        assert f.grad.shape == (n, 9)
        if n:
            assert bool(g.any())
            _bar("5x3", f.grad.cpu().numpy(), g.cpu().numpy())
            # the frame is small enough for the dense transpose through the forward itself, one gaussian's one-hot row at a time
            w = R.blend_weights(cam)
            eye = torch.zeros((n, 1), device="cuda")
            for i in torch.nonzero(w)[:4, 0].tolist():
                eye.zero_()
                eye[i] = 1.0
                wi = R.render_features(cam, eye)[..., 0]
                assert abs(float(wi.double().sum()) - float(w[i])) <= 1e-5 * float(w.max())
    # every gaussian behind the camera
    cols = G.synthetic.mip360_like(500, 4)
    cols["y"] = (cols["y"] - np.float32(100.0)).astype(np.float32)  # the camera at y = -4 looks along +y
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_columns(cols))
    g = R.feature_gradient(cam, gm)
    assert g.shape == (500, 9) and not g.any() and not R.blend_weights(cam).any()
    assert R.last_stats["n_visible"] == 0 and R.last_stats["wave_entries"] == 0
    # the widest map on f1: channel j of the upstream gradient carries column j % N_CH
    c = _case(G, "f1")
    R, cam = c["R"], c["cam"]
    n_max = G.lib.GSR_MAX_FEATURE_CHANNELS
    reps = -(-n_max // N_CH)
    gmax = c["Gt"].repeat(1, 1, reps)[..., :n_max].contiguous()
    gw = R.feature_gradient(cam, gmax).cpu().numpy()
    ref = np.tile(R.feature_gradient(cam, c["Gt"]).cpu().numpy(), (1, reps))[:, :n_max]
    assert gw.shape == (R.scene.n, n_max)
    _bar("1024 channels", gw, ref)
    with pytest.raises(ValueError):
        R.feature_gradient(cam, torch.zeros((cam.height, cam.width, n_max + 1), device="cuda"))
