"""GPU: Rasterizer.splat_gradient — the gradient of a feature map and of the final T with respect to every gaussian's opacity, 2-D
mean and inverse 2-D covariance (gsr_render_splat_backward / gsr_blend_splat_backward) — against the float64 closed form of
tools/splat_reference.py on the pinned fuzz cases of tools/fuzz_maps.py, in file order and in Morton order.

tests/test_splat_reference.py holds the closed form to finite differences first, without a GPU.  The bound is |err| <=
1e-5 (A + B) per row and column (A: the row's own terms in absolute value; B: the magnitude the kernel's subtraction S' - P_i
works at), rows the reference never reaches are exactly 0, and the plain 100 dB bar is asserted wherever the fp32 emulation reaches
110 dB.  Pixels on the 1/255 band and on the cap band carry G = 0 and gT = 0 on both sides.  Every figure is printed ("splat ..."
lines).  Seed 354 (one entry past a batch), seeds 252 and 324 (tiles sharing gaussians) are among the pins.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_cases import _tool, fuzz_case, namespace

pytestmark = pytest.mark.gpu

fm = _tool("fuzz_maps")
sr = _tool("splat_reference")
PINNED = [s for s in fm.PINS if s not in fm.IDENTITIES_ONLY]
ORDERS = ["file", "morton"]
SIX = list(range(6))
EIGHT = list(range(8))


@pytest.fixture(scope="module")
def G():
    return namespace()


def _case(G, seed, order):
    """The pinned case as a scene in `order` with its Rasterizer, camera and reference (the oracle fed the arrays in the scene's
    order), the features, the upstream gradients; built once and only read."""
    key = (seed, order)
    if key not in G.cases:
        c = fuzz_case(seed, fm.MAX_N)
        scene = G.renderer.GaussianScene.from_packed(c["packed"], spatial_order=order == "morton")
        assert (scene.order is None) == (order == "file")
        ref = fm.build_reference(G.orc, c["packed"], c["args"], scene.order)
        assert ((c["W"] <= 160 and c["H"] <= 96) or (c["W"] <= 33 and c["H"] <= 360)) and c["n"] <= 4096  # small frames: quick cases
        G.cases[key] = dict(seed=seed, R=G.renderer.Rasterizer(scene), cam=G.renderer.make_camera(*c["args"]), ref=ref, n=c["n"],
                            F=fm.features_of(seed, c["n"]), Gm=fm.upstream_of(seed, c["H"], c["W"])[0], gT=sr.gT_of(seed, c["H"], c["W"]))
    return G.cases[key]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _masked(c, C, min_T=0.0, ref=None):
    """(F, G, gT) at C channels as numpy, G and gT zeroed on the pixels the comparison leaves out."""
    keep = ~sr.left_out(ref if ref is not None else c["ref"], min_T)
    return c["F"][:, :C], (c["Gm"][..., :C] * keep[..., None]).astype(np.float32), (c["gT"] * keep).astype(np.float32)


def _report(seed, order, kind, fig):
    print(f"\nsplat seed={seed} order={order} kind={kind} " + " ".join(f"{k}={v:.3g}" for k, v in fig.items()), end="")


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_parity(G, seed, order):
    """C = 17, 16, 3 and 1, with grad_T and without: the bound per row and column, exact zeros on the rows the reference never
    reaches, the plain bar where the emulation reaches 110 dB."""
    c = _case(G, seed, order)
    fig = sr.run_parity(c["R"], c["cam"], c["ref"], c["F"], c["Gm"], c["gT"])
    if seed in (290, 324, 263):  # nothing passes 1/255, or nothing is drawn: zeros
        g = c["R"].splat_gradient(c["cam"], _dev(c["F"]), _dev(c["Gm"]), _dev(c["gT"]), abs_mean=False)
        assert not g.mean2d.any() and not g.sigmas.any() and not g.opacity.any()
    _report(seed, order, "parity", fig)


@pytest.mark.parametrize("seed", [264, 354, 252, 277])
def test_abs_mean(G, seed):
    """abs_mean2d against the reference at C = 3 and 16; refused at C = 17; columns 6 and 7 untouched when it is off."""
    c = _case(G, seed, "morton")
    R, cam, ref, n = c["R"], c["cam"], c["ref"], c["n"]
    fig = {}
    for Cw in (3, 16):
        F, Gz, gTz = _masked(c, Cw)
        got = R.splat_gradient(cam, _dev(F), _dev(Gz), _dev(gTz), abs_mean=True)
        assert got.abs_mean2d is not None and tuple(got.abs_mean2d.shape) == (n, 2)
        sr.check_gradient(f"abs seed={seed} C={Cw}", sr.as_rows(got), sr.closed_form(ref, F, Gz, gTz), EIGHT, fig)
        assert bool((got.abs_mean2d >= got.mean2d.abs() * (1 - 1e-5)).all())
    F, Gz, gTz = _masked(c, 17)
    with pytest.raises(ValueError, match="abs_mean"):
        R.splat_gradient(cam, _dev(F), _dev(Gz), _dev(gTz), abs_mean=True)
    out = torch.full((n, 8), 7.0, device="cuda")
    g = R.splat_gradient(cam, _dev(F), _dev(Gz), _dev(gTz), out=out)
    assert g.abs_mean2d is None and bool((out[:, 6:] == 7.0).all()) and bool((out[:, :6] != 7.0).any())
    _report(seed, "morton", "abs", fig)


@pytest.mark.parametrize("seed", [264, 354])
def test_exact_zeros(G, seed):
    """G = 0 with gT = 0, and features = 0 without grad_T, add exactly nothing to a prefilled out."""
    c = _case(G, seed, "file")
    R, cam, n = c["R"], c["cam"], c["n"]
    fill = torch.randn((n, 8), generator=torch.Generator().manual_seed(1)).cuda()
    for Cw in (17, 3):
        F, Gm = _dev(c["F"][:, :Cw]), _dev(c["Gm"][..., :Cw])
        out = fill.clone()
        R.splat_gradient(cam, F, torch.zeros_like(Gm), torch.zeros_like(_dev(c["gT"])), abs_mean=Cw <= 16, out=out)
        assert torch.equal(out, fill), (seed, Cw, "G = 0")
        R.splat_gradient(cam, torch.zeros_like(F), Gm, None, abs_mean=Cw <= 16, out=out)
        assert torch.equal(out, fill), (seed, Cw, "features = 0")
        g = R.splat_gradient(cam, F, Gm, _dev(c["gT"]), out=out)  # ... and something where neither is zero
        assert not torch.equal(out, fill) and g.opacity.data_ptr() == out.data_ptr()


@pytest.mark.parametrize("seed", [296, 378, 351, 327])
def test_min_T_and_early_out(G, seed):
    """min_T = 1e-4: pairs behind it contribute 0, against the reference with the same mask.  early_out_T = 1e-4: against the
    reference truncated where the forward stops — the pairs the forward's own one-hot weights show as drawn under the same
    options."""
    c = _case(G, seed, "file")
    R, cam, ref, n = c["R"], c["cam"], c["ref"], c["n"]
    fig = {}
    F, Gz, gTz = _masked(c, 17, min_T=1e-4)
    got = R.splat_gradient(cam, _dev(F), _dev(Gz), _dev(gTz), min_T=1e-4)
    cut = sr.closed_form(ref, F, Gz, gTz, min_T=1e-4)
    sr.check_gradient(f"min_T seed={seed}", sr.as_rows(got), cut, SIX, fig)
    full = sr.closed_form(ref, F, Gz, gTz)
    assert (cut["A"] < full["A"]).any()  # the mask took something out

    o = G.renderer.make_options(early_out_T=1e-4)
    onehot = np.zeros((n, len(ref["kept"])), np.float32)
    onehot[ref["kept"], np.arange(len(ref["kept"]))] = 1.0
    Wg = R.render_features(cam, _dev(onehot), o).cpu().numpy()
    sub = sr.truncated(ref, Wg > 0)
    fig["pairs_behind_the_stop"] = int((ref["alpha"] > 0).sum() - (sub["alpha"] > 0).sum())
    assert seed != 351 or fig["pairs_behind_the_stop"] > 0  # there a whole quadrant gets below 1e-4: the forward does stop early
    F, Gz, gTz = _masked(c, 17, ref=sub)
    Gz, gTz = Gz * ~sr.left_out(ref)[..., None], gTz * ~sr.left_out(ref)
    got = R.splat_gradient(cam, _dev(F), _dev(Gz), _dev(gTz), o)
    sr.check_gradient(f"early_out_T seed={seed}", sr.as_rows(got), sr.closed_form(sub, F, Gz, gTz), SIX, fig)
    _report(seed, "file", "min_T", fig)


@pytest.mark.parametrize("seed", [354, 252])
def test_out_accumulates_and_runs_agree(G, seed):
    c = _case(G, seed, "morton")
    R, cam, ref, n = c["R"], c["cam"], c["ref"], c["n"]
    F, Gz, gTz = _masked(c, 17)
    cf = sr.closed_form(ref, F, Gz, gTz)
    lim = sr.REL * (cf["A"] + cf["B"])[:, :6]
    Fs = _dev(F)[R.scene.order_t]  # out= is in the scene's order; so are the features with scene_order=True
    out = torch.zeros((n, 8), device="cuda")
    for _ in range(2):
        R.splat_gradient(cam, Fs, _dev(Gz), _dev(gTz), out=out, scene_order=True)
    one = R.splat_gradient(cam, Fs, _dev(Gz), _dev(gTz), scene_order=True)
    two = R.splat_gradient(cam, _dev(F), _dev(Gz), _dev(gTz))

    def back(rows):  # scene order -> file order
        filed = np.empty_like(rows)
        filed[R.scene.order] = rows
        return filed

    a, b = back(sr.as_rows(one))[:, :6], sr.as_rows(two)[:, :6]
    twice = back(out.cpu().numpy().astype(np.float64))[:, :6]
    print(f"\nsplat seed={seed} two runs: worst |a - b| / bound {np.max(np.abs(a - b) / np.maximum(lim, 1e-300)):.3g}; "
          f"out twice: worst |out - 2 a| / bound {np.max(np.abs(twice - 2 * a) / np.maximum(2 * lim, 1e-300)):.3g}", end="")
    assert (np.abs(a - b) <= lim).all()
    assert (np.abs(twice - 2 * a) <= 2 * lim).all()
    sr.check_gradient(f"seed={seed} scene_order", np.concatenate([a, np.zeros((n, 2))], 1), cf, SIX, {})


def test_column_window_and_screen_layout(G):
    """A column window of a wider feature tensor is read where it lies; [W, H, C] maps (output_layout = 1) give the same gradient."""
    c = _case(G, 252, "file")
    R, cam, ref, n = c["R"], c["cam"], c["ref"], c["n"]
    for Cw in (16, 5):
        F, Gz, gTz = _masked(c, Cw)
        cf = sr.closed_form(ref, F, Gz, gTz)
        wide = torch.randn((n, 40), generator=torch.Generator().manual_seed(2)).cuda()
        wide[:, 3:3 + Cw] = _dev(F)
        window = wide[:, 3:3 + Cw]
        assert not window.is_contiguous()
        got = R.splat_gradient(cam, window, _dev(Gz), _dev(gTz), scene_order=True)
        sr.check_gradient(f"window C={Cw}", sr.as_rows(got), cf, SIX, {})
        o = G.renderer.make_options(output_layout=1)
        got = R.splat_gradient(cam, _dev(F), _dev(Gz.transpose(1, 0, 2)), _dev(gTz.T), o)
        sr.check_gradient(f"[W, H, C] C={Cw}", sr.as_rows(got), cf, SIX, {})


def test_neighbours_on_the_workspace(G):
    """At the ABI: a gsr_blend before and after the splat backward on one workspace renders its own bits; gsr_read_stats afterwards
    carries the forward's counters; render_features afterwards is unchanged bit for bit."""
    from gsr_amd._lib import check, lib

    c = _case(G, 252, "morton")
    R, cam, n = c["R"], c["cam"], c["n"]
    Fs = _dev(c["F"])[R.scene.order_t].contiguous()
    Gm, gT = _dev(c["Gm"]), _dev(c["gT"])
    before = R.render_features(cam, Fs, scene_order=True)
    o = G.renderer.make_options(colour_stage=0)
    R.render(cam, o)  # sizes the pair buffers to the frame
    ws = R._workspace(cam.width, cam.height)
    sc, sp = R.scene.c_struct(), int(torch.cuda.current_stream().cuda_stream)
    wp, wn, mp = ws.data_ptr(), ws.numel(), R.max_pairs
    check(lib.gsr_preprocess(C.byref(sc), C.byref(cam), C.byref(o), wp, wn, None, sp))
    check(lib.gsr_bin_sort(n, C.byref(cam), C.byref(o), mp, wp, wn, sp))

    def blend():
        out = torch.empty((cam.height, cam.width, 3), dtype=torch.float32, device="cuda")
        check(lib.gsr_blend(C.byref(sc), n, C.byref(cam), C.byref(o), mp, wp, wn, out.data_ptr(), None, sp))
        return out

    alone = blend()
    g = torch.zeros((n, 8), dtype=torch.float32, device="cuda")
    check(lib.gsr_blend_splat_backward(n, C.byref(cam), C.byref(o), mp, wp, wn, Fs.data_ptr(), fm.N_CH, fm.N_CH, Gm.data_ptr(),
                                       gT.data_ptr(), 0.0, 0, g.data_ptr(), sp))
    st_b = R.stats()
    after = blend()
    m = torch.empty((cam.height, cam.width, fm.N_CH), dtype=torch.float32, device="cuda")
    check(lib.gsr_blend_channels(n, C.byref(cam), C.byref(o), mp, wp, wn, Fs.data_ptr(), fm.N_CH, fm.N_CH, m.data_ptr(), None, sp))
    st_f = R.stats()
    torch.cuda.synchronize()
    assert torch.equal(after, alone)
    for k in ("wave_entries", "fetched_entries", "n_pairs", "n_visible"):
        assert st_b[k] == st_f[k] and st_b[k] > 0, (k, st_b, st_f)
    assert torch.equal(R.render_features(cam, Fs, scene_order=True), before)
    # the ABI call is what the host call makes (two runs: within the bound of one another)
    host = R.splat_gradient(cam, Fs, Gm, gT, scene_order=True)
    F, Gz, gTz = c["F"], c["Gm"], c["gT"]
    cf = sr.closed_form(c["ref"], F, Gz, gTz)
    lim = sr.REL * (cf["A"] + cf["B"])[:, :6][R.scene.order]
    assert (np.abs(g.cpu().numpy().astype(np.float64)[:, :6] - sr.as_rows(host)[:, :6]) <= lim).all() and bool(g.any())
    assert not g[:, 6:].any()


@pytest.mark.parametrize("seed", [264, 277])
def test_opacity_logit_gradient(G, seed):
    """g.opacity o (1 - o) against the reference's chain through the sigmoid."""
    c = _case(G, seed, "morton")
    R, cam, ref = c["R"], c["cam"], c["ref"]
    F, Gz, gTz = _masked(c, 3)
    g = R.splat_gradient(cam, _dev(F), _dev(Gz), _dev(gTz))
    got = G.renderer.opacity_logit_gradient(R.scene, g).cpu().numpy().astype(np.float64)
    cf = sr.closed_form(ref, F, Gz, gTz)
    logit = fuzz_case(seed, fm.MAX_N)["packed"]["opacity_logit"].astype(np.float64)
    o = 1.0 / (1.0 + np.exp(-logit))
    chain = o * (1.0 - o)
    lim = sr.REL * (cf["A"][:, 0] + cf["B"][:, 0]) * chain + 1e-6 * np.abs(cf["g"][:, 0] * chain)  # (+ the fp32 sigmoids' rounding)
    assert (np.abs(got - cf["g"][:, 0] * chain) <= lim).all() and bool(np.any(got))
    # ... and the preprocess' opacity is that sigmoid: the chain is taken in the right variable
    op = R.preprocess_debug(cam)["opacity"].cpu().numpy()
    drawn = ref["kept"]
    assert np.allclose(op[drawn], o[drawn], rtol=1e-5, atol=0)
