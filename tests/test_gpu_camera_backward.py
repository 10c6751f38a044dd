"""GPU: gsr_camera_backward, renderer.camera_backward / pose_gradient and Rasterizer.camera_gradient — the splat gradient of a view
summed into the gradient with respect to the camera — against the float64 stage chain of tools/camera_reference.py on the pinned
fuzz cases of tools/fuzz_maps.py, in file order and in Morton order, under each pin's own camera and the rolled, oblique, anamorphic
variants.

tests/test_camera_reference.py holds that chain to autograd and to finite differences first, without a GPU.  The bound is
|err| <= 1e-5 B per entry, B = bound64: the same chain with every Jacobian entry and the upstream in absolute value, summed over
the gaussians.  End to end the upstream of the bound is |g| + A + B_splat (splat_reference's per-row terms) and, for the view
rows, |g_rgb| + sum_p w |G| through the SH chain in absolute values.  Every figure is printed ("camera ..." lines).
"""
import numpy as np
import pytest
import torch

from camera_cases import (CAMERAS, ORDERS, PINNED, check_operator_parity, cr, dev as _dev, fm, kernel_constants, packed_gradient, pr,
                          project_case as _case, project_rows as _rows, raw_camera_backward as _raw, sh_e2e_case, sh_masked, shr, sr,
                          view_rows_of)
from backward_cases import project_masked
from gpu_cases import namespace

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    return namespace()


@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_operator_parity(G, seed, order, camera):
    """|err| <= 1e-5 B per entry, slot 29 exact, slots 30-31 zero.  Seed 351 under tilt_b has the ray clamp active on all its 89."""
    c = _case(G, seed, order, camera)
    check_operator_parity(G, c)
    if (seed, camera) == (351, "tilt_b"):
        k = c["ref"]["kept_in"]
        assert len(k) == 89 and pr.clamp_state(pr.rows_of(c["theta"], k), c["ocam"])[0].any(1).all()


@pytest.mark.parametrize("seed", [354, 369])
def test_each_input_alone_is_its_part_of_the_call_with_both(G, seed):
    """Bit for bit: the splat rows feed slots 0-25 and 29, the view rows slots 26-28; the other's slots are zero."""
    c = _case(G, seed, "morton")
    rows, view = _dev(_rows(c)), _dev(view_rows_of(seed, c["n"]))
    both, a, b = (_raw(G, c["scene"], c["cam"], r, v) for r, v in ((rows, view), (rows, None), (None, view)))
    assert np.array_equal(a[:26], both[:26]) and a[29] == both[29] > 0 and not a[26:29].any() and both[:26].all()
    assert np.array_equal(b[26:29], both[26:29]) and not b[:26].any() and not b[29:].any() and both[26:29].all()
    with pytest.raises(ValueError, match="splat_rows, view_mean_rows or both"):
        G.renderer.camera_backward(c["scene"], c["cam"])


@pytest.mark.parametrize("seed", [290, 324, 263])
def test_nothing_passes_gives_exact_zeros(G, seed):
    """The pins on which no pair passes the blend (geometry_gradient gives exact zeros there): Rasterizer.camera_gradient gives 32
    exact zeros, with the caller's features and for the colour frame at degree 0 (no view term)."""
    c = _case(G, seed, "file")
    got = c["R"].camera_gradient(c["cam"], _dev(c["Gm"]), _dev(c["gT"]), features=_dev(c["F"]))
    assert not packed_gradient(got).any() and all(t.device.type == "cuda" for t in got)
    assert not _raw(G, c["scene"], c["cam"], torch.zeros((c["n"], 8), device="cuda"), torch.zeros((c["n"], 3), device="cuda")).any()


@pytest.mark.parametrize("seed,order", [(297, "file"), (264, "morton"), (354, "file"), (369, "morton")])
def test_the_skip_and_the_cull_are_exact(G, seed, order):
    """Culled gaussians (well clear of the plane) with nonzero rows add nothing; columns 6 and 7 alone do not touch a row."""
    c = _case(G, seed, order)
    n = c["n"]
    z = pr.project64(c["theta"], c["ocam"])["cam_means"][:, 2].numpy()
    culled = np.flatnonzero(z < pr.CULL_Z - 1e-3)
    assert seed != 369 or len(culled) > 1000
    assert not _raw(G, c["scene"], c["cam"], _dev(pr.unit_rows(seed + 1, n, culled))).any()
    tail = np.zeros((n, 8), np.float32)
    tail[:, 6:] = 5.0
    assert not _raw(G, c["scene"], c["cam"], _dev(tail)).any()
    rows = _rows(c)
    marked = rows.copy()
    marked[:, 6:] = 5.0
    assert np.array_equal(_raw(G, c["scene"], c["cam"], _dev(marked)), _raw(G, c["scene"], c["cam"], _dev(rows)))


def _tiled_case(G):
    """Pin 369 (n = 4096, file order) with its rows, view rows and per-gaussian float64 contributions: what every size is cut or
    tiled from, so the CPU cost stays that of 4096 gaussians."""
    key = ("camera tiled",)
    if key not in G.cases:
        c = _case(G, 369, "file")
        rows, view = _rows(c), view_rows_of(369, c["n"])
        G.cases[key] = dict(c=c, rows=rows, view=view, per=cr.vjp64(c["theta"], c["ocam"], rows, view)[0],
                            perB=cr.bound64(c["theta"], c["ocam"], rows, view)[0],
                            passes=(rows[:, :6].any(1) & pr.contributes(pr._forward(c["theta"], c["ocam"])).numpy()))
    return G.cases[key]


def _sized(G, n):
    """(scene of the first n gaussians of pin 369 tiled, rows, view rows, want, B, count)."""
    t = _tiled_case(G)
    base = t["c"]["n"]
    idx = np.arange(n) % base
    packed = {k: np.ascontiguousarray(np.asarray(v)[idx]) for k, v in t["c"]["c"]["packed"].items()}
    scene = G.renderer.GaussianScene.from_packed(packed, spatial_order=False)
    reps, rest = divmod(n, base)
    total = lambda per: reps * per.sum(0) + per[:rest].sum(0)
    return scene, t["rows"][idx], t["view"][idx], total(t["per"]), total(t["perB"]), reps * int(t["passes"].sum()) + int(t["passes"][:rest].sum())


def _two_trips_and_a_ragged_tail():
    threads, groups = kernel_constants()
    return threads * (2 * groups + 5) + 37  # 2 groups + 6 blocks over (2 groups + 6) / 3 workgroups: each makes 3 trips, the last block is ragged


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4096, "two trips"])
def test_sizes_and_reduction_edges(G, n):
    """One lane, one short of a wave, a wave, one past it, one past a workgroup, sixteen workgroups, and a size at which every
    workgroup makes at least two trips with a ragged last block: |err| <= 1e-5 B, the count exact.  At the largest size a second
    run is bit-identical and rows x 2 give exactly 2 x the result (the count stays)."""
    big = n == "two trips"
    n = _two_trips_and_a_ragged_tail() if big else n
    threads, groups = kernel_constants()
    blocks = -(-n // threads)
    launched = -(-blocks // -(-blocks // groups))  # workgroups, as camera_backward.hip sizes the grid; each takes every launched-th block
    assert not big or (n % threads and blocks // launched >= 2)
    scene, rows, view, want, B, count = _sized(G, n)
    cam = _tiled_case(G)["c"]["cam"]
    got = _raw(G, scene, cam, _dev(rows), _dev(view))
    cr.check_camera(f"seed=369 tiled n={n} kind=sizes", got, want, B)
    assert got[29] == count and not got[30:].any()
    if big:
        assert np.array_equal(_raw(G, scene, cam, _dev(rows), _dev(view)), got)
        twice = _raw(G, scene, cam, _dev(2 * rows), _dev(2 * view))
        assert np.array_equal(twice[:29], 2 * got[:29]) and twice[29] == got[29] and got[:29].all()


def _colour_expected(c, Gz, gTz):
    n, ref, ocam = c["ref"]["n"], c["ref"], c["ocam"]
    fw = shr.sh64(c["theta_file"], ocam, 3)
    assert shr.keep_mask(c["theta_file"], ocam, 3)[2] == 0  # the SH band leaves out nothing on these pins
    cf = sr.closed_form(ref, fw["rgb"], Gz, gTz)
    g_rgb = fm.gradient(ref, Gz, n)
    own = fm.gradient(dict(ref, w=np.abs(ref["w"])), np.abs(Gz), n)
    view = shr.vjp64(c["theta_file"], ocam, 3, g_rgb)["means"]
    viewB = shr.bound64(c["theta_file"], ocam, 3, np.abs(g_rgb) + own)["means"]
    return (cr.vjp64(c["geo_file"], ocam, cf["g"], view)[1], cr.bound64(c["geo_file"], ocam, np.abs(cf["g"]) + cf["A"] + cf["B"], viewB)[1])


def _check_pose(G, tag, c, got, want, B):
    """pose_gradient of the result within the same bound carried through the linear chain in absolute values."""
    twist, logf = G.renderer.pose_gradient(c["cam"], got)
    assert twist.dtype == logf.dtype == torch.float64 and twist.device.type == logf.device.type == "cpu"
    have = np.concatenate([twist.numpy(), logf.numpy()])
    ref = np.concatenate(cr.twist_chain64(c["ocam"], want))
    lim = np.concatenate(cr.twist_chain64(c["ocam"], B, absolute=True))
    worst = float((np.abs(have - ref) / (cr.REL * lim)).max())
    print(f"\ncamera {tag} kind=pose: worst |err| / (1e-05 chain(B)) {worst:.3g}", end="")
    assert worst <= 1.0 and have.all()


@pytest.mark.parametrize("seed,camera", [(264, None), (301, None), (354, None), (327, None), (252, None), (354, "tilt_a")])
def test_end_to_end(G, seed, camera):
    """Rasterizer.camera_gradient, with grad_T and without: the colour frame at degree 3 (the SH view term included), and
    features= at C = 3 and 17, against vjp64 of the closed form's rows."""
    c = sh_e2e_case(G, seed, camera=camera)
    Gz, gTz = sh_masked(c)
    for with_T in (True, False):
        got = c["R"].camera_gradient(c["cam"], _dev(Gz), _dev(gTz) if with_T else None)
        want, B = _colour_expected(c, Gz, gTz if with_T else None)
        tag = f"{c['tag']} kind=end-to-end colour gT={int(with_T)}"
        cr.check_camera(tag, packed_gradient(got), want, B)
        assert got.w2c.device.type == "cuda" and got.w2c.dtype == torch.float64 and tuple(got.w2c.shape) == tuple(got.full_proj.shape) == (4, 4)
        assert got.cam_center.cpu().numpy().all() and float(got.contributing) > 0
        _check_pose(G, tag, c, got, want, B)
    p = _case(G, seed, "morton", camera)
    for Cw in (3, 17):
        F, Gz, gTz = project_masked(p, Cw)
        for with_T in (True, False):
            got = p["R"].camera_gradient(p["cam"], _dev(Gz), _dev(gTz) if with_T else None, features=_dev(F))
            cf = sr.closed_form(p["ref"], F, Gz, gTz if with_T else None)
            want = cr.vjp64(p["theta_file"], p["ocam"], cf["g"])[1]
            B = cr.bound64(p["theta_file"], p["ocam"], np.abs(cf["g"]) + cf["A"] + cf["B"])[1]
            tag = f"{p['tag']} kind=end-to-end C={Cw} gT={int(with_T)}"
            cr.check_camera(tag, packed_gradient(got), want, B)
            assert not got.cam_center.any()  # the features are the caller's: nothing flows through the SH evaluation
            _check_pose(G, tag, p, got, want, B)


def test_the_translation_rows_are_the_column_sums_of_grad_means(G):
    """Both kernels take gcm and gpt from ONE statement of the upstream chain (splat_chain.h); what each does with them — the
    mean's combination in project_backward.hip, the camera's rows in camera_backward.hip — is checked here against the other.
    d cm / d mean = A^T and d cm / d w2c[3] = I, d clip / d mean = F[:3] and d clip / d F[3] = I, so the column sums of
    gsr_project_backward's grad_means are (w2c translation row) A^T + (full_proj translation row) F[:3]^T: to 1e-5 B, B the same
    combination of the camera bound's rows in absolute values plus the means' own bound summed."""
    for seed in (354, 369):
        c = _case(G, seed, "morton")
        rows = _rows(c)
        means = G.renderer.project_backward(c["scene"], c["cam"], _dev(rows), scene_order=True).means.double().sum(0).cpu().numpy()
        got = _raw(G, c["scene"], c["cam"], _dev(rows))
        base = pr.camera_of(c["ocam"])
        V, F = np.asarray(base["V"]), np.asarray(base["F"])
        implied = lambda t, ab: ab(V[:3, :3]) @ t[9:12] + ab(F[:3][:, cr.FCOLS]) @ t[21:24]
        B = implied(cr.bound64(c["theta"], c["ocam"], rows)[1], np.abs) + pr.bound64(c["theta"], c["ocam"], rows)["means"].sum(0)
        worst = float((np.abs(means - implied(got, lambda x: x)) / (cr.REL * B)).max())
        print(f"\ncamera seed={seed} kind=translation rows against grad_means: worst |diff| / (1e-05 B) {worst:.3g}", end="")
        assert worst <= 1.0 and means.all()


def test_nothing_else_moved(G):
    """render, project_backward and sh_backward before and after a camera_gradient on one Rasterizer are bit for bit the same."""
    c = sh_e2e_case(G, 354)
    R, cam, scene = c["R"], c["cam"], c["scene"]
    Gz, gTz = sh_masked(c)
    rows, g = _dev(_rows(_case(G, 354, "morton"))), _dev(c["g"])

    def around():
        return [R.render(cam).clone(), *G.renderer.project_backward(scene, cam, rows), *G.renderer.sh_backward(scene, cam, g)]

    before = around()
    got = R.camera_gradient(cam, _dev(Gz), _dev(gTz))
    after = around()
    assert all(torch.equal(a, b) and bool(a.any()) for a, b in zip(before, after))
    assert packed_gradient(got)[:29].all()
