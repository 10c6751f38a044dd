"""GPU: renderer.project_backward and Rasterizer.geometry_gradient (gsr_project_backward) — the splat gradient of a view chained
through the projection to the scene's means, log-scales, quaternions and opacity logits — against the float64 stage chain of
tools/projection_reference.py on the pinned fuzz cases of tools/fuzz_maps.py, in file order and in Morton order.

tests/test_projection_reference.py holds that chain to autograd and to finite differences first, without a GPU.  The bound is
|err| <= 1e-5 B per element, B = bound64: the same chain with every stage's Jacobian and the upstream in absolute value.  End to
end the upstream of the bound is |g| + A + B_splat, splat_reference's per-row terms: the chain in absolute values is linear in a
non-negative upstream, so that is the splat gradient's own allowance carried through plus the projection's.  Every figure is
printed ("project ..." lines).
"""
import numpy as np
import pytest
import torch

from backward_cases import (PINNED, ORDERS, check_project_end_to_end, check_project_operator_parity, dev as _dev, fm, pr,
                            project_case as _case, project_expected as _expected, project_masked as _masked, project_rows as _rows)
from gpu_cases import namespace
from order_scenes import camera_args

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    return namespace()


def _filled(n, seed=1):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=gen).cuda() for s in ((n, 3), (n, 3), (n, 4), (n,))]


def _into(G, c, rows, bufs):
    return G.renderer.project_backward(c["scene"], c["cam"], _dev(rows), out=G.renderer.GeometryGradient(*bufs))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_operator_parity(G, seed, order):
    """project_backward on unit-normal rows against vjp64: |err| <= 1e-5 B per element; the file-order result is the scene-order
    one through scene.order_t."""
    check_project_operator_parity(G, _case(G, seed, order))


@pytest.mark.parametrize("seed,order", [(297, "file"), (306, "file"), (264, "morton"), (296, "morton"), (354, "file"), (369, "morton"), (369, "file")])
def test_the_skip_is_exact(G, seed, order):
    """n = 1, 65 (one lane past a wave), 257 (one past a workgroup), 4096: rows that are zero leave a prefilled out bit for bit,
    alone and next to touched rows; culled gaussians with nonzero rows add nothing."""
    c = _case(G, seed, order)
    n = c["n"]
    assert n == {297: 1, 306: 1, 264: 65, 296: 257, 354: 257, 369: 4096}[seed]
    fill = _filled(n)
    out = [f.clone() for f in fill]
    _into(G, c, np.zeros((n, 8), np.float32), out)
    assert all(torch.equal(a, b) for a, b in zip(out, fill))
    rows = _rows(c)
    rows[:, 6:] = 5.0  # columns 6 and 7 are not looked at: they alone do not make a row touched
    _into(G, c, rows, out)
    zero = _dev(~rows[:, :6].any(1))
    for a, b in zip(out, fill):
        assert torch.equal(a[zero], b[zero]) and (not len(c["ref"]["kept_in"]) or not torch.equal(a, b))
    # behind the cull plane (well clear of it, so that fp32 decides as float64 does): whatever the row holds
    z = pr.project64(c["theta"], c["ocam"])["cam_means"][:, 2].numpy()
    culled = np.flatnonzero(z < pr.CULL_Z - 1e-3)
    print(f"\nproject seed={seed} order={order} kind=skip n={n} untouched={int(zero.sum())} culled={len(culled)}", end="")
    assert seed != 369 or len(culled) > 1000
    rows = pr.unit_rows(seed + 1, n, culled)
    out = [f.clone() for f in fill]
    _into(G, c, rows, out)
    assert all(torch.equal(a, b) for a, b in zip(out, fill))


@pytest.mark.parametrize("seed", [354, 369])
def test_null_outputs(G, seed):
    """Each output alone is bit for bit that output of the four-output call."""
    c = _case(G, seed, "morton")
    rows = _dev(_rows(c))
    full = G.renderer.project_backward(c["scene"], c["cam"], rows, scene_order=True)
    for k, name in enumerate(pr.FIELDS):
        bufs = [None] * 4
        bufs[k] = torch.zeros_like(full[k])
        got = G.renderer.project_backward(c["scene"], c["cam"], rows, out=G.renderer.GeometryGradient(*bufs))
        assert all(got[j] is None for j in range(4) if j != k)
        assert torch.equal(got[k], full[k]) and bool(full[k].any()), name
    with pytest.raises(ValueError, match="at least one"):
        G.renderer.project_backward(c["scene"], c["cam"], rows, out=G.renderer.GeometryGradient(None, None, None, None))


@pytest.mark.parametrize("seed", [354, 252])
def test_accumulation_is_exact_and_runs_are_identical(G, seed):
    """Two calls into one out are 2 x one call (x + x is exact); a second run is bit-identical: no atomics."""
    c = _case(G, seed, "morton")
    rows = _dev(_rows(c))
    one = G.renderer.project_backward(c["scene"], c["cam"], rows, scene_order=True)
    again = G.renderer.project_backward(c["scene"], c["cam"], rows, scene_order=True)
    out = G.renderer.GeometryGradient(*[torch.zeros_like(t) for t in one])
    for _ in range(2):
        G.renderer.project_backward(c["scene"], c["cam"], rows, out=out)
    for k in range(4):
        assert torch.equal(one[k], again[k]) and torch.equal(out[k], 2 * one[k]), pr.FIELDS[k]


@pytest.mark.parametrize("seed", [264, 301, 354, 327, 252])
def test_end_to_end(G, seed):
    """geometry_gradient at C = 3 and 17, with grad_T and without, against vjp64(closed form)."""
    check_project_end_to_end(_case(G, seed, "morton"))


@pytest.mark.parametrize("seed", [290, 324, 263])
def test_nothing_passes_gives_exact_zeros(G, seed):
    c = _case(G, seed, "file")
    got = c["R"].geometry_gradient(c["cam"], _dev(c["F"]), _dev(c["Gm"]), _dev(c["gT"]))
    assert all(tuple(t.shape)[0] == c["n"] and not t.any() for t in got)


def test_scene_order_and_file_order_agree(G):
    """Through scene.order_t, within the two runs' allowances (the splat gradient's sums are atomic)."""
    c = _case(G, 252, "morton")
    R, cam, order_t = c["R"], c["cam"], c["scene"].order_t
    F, Gz, gTz = _masked(c, 17)
    want, B = _expected(c["theta_file"], c["ocam"], c["ref"], F, Gz, gTz)
    filed = R.geometry_gradient(cam, _dev(F), _dev(Gz), _dev(gTz))
    scened = R.geometry_gradient(cam, _dev(F)[order_t], _dev(Gz), _dev(gTz), scene_order=True)
    back = G.renderer.GeometryGradient(*[G.renderer.file_order_gradient(t, order_t) for t in scened])
    pr.check_geometry("seed=252 kind=scene-order", pr.as_dict(back), want, B)
    pr.check_geometry("seed=252 kind=scene-order against file-order", pr.as_dict(back), pr.as_dict(filed), pr.sum_bounds(B, B))


def test_out_accumulates_over_two_cameras(G):
    """out= over two cameras of fm.case_views is the sum of the single calls, within the sum of their allowances."""
    c = _case(G, 264, "morton")
    R, scene = c["R"], c["scene"]
    views = fm.case_views(G.orc, c["c"], scene.order)[:2]
    out = G.renderer.GeometryGradient(*[torch.zeros(s, device="cuda") for s in ((c["n"], 3), (c["n"], 3), (c["n"], 4), (c["n"],))])
    wants, bounds, singles = [], [], []
    Fs = _dev(c["F"])[scene.order_t]
    for args, ref in views:
        cam, ocam = G.renderer.make_camera(*args), G.orc.camera(*args)
        F, Gz, gTz = _masked(c, 17, ref)
        want, B = _expected(c["theta"], ocam, dict(ref, kept=ref["kept_in"]), F[scene.order], Gz, gTz)  # everything in the scene's order
        wants.append(want), bounds.append(B)
        assert R.geometry_gradient(cam, Fs, _dev(Gz), _dev(gTz), out=out, scene_order=True) is out
        singles.append(pr.as_dict(R.geometry_gradient(cam, Fs, _dev(Gz), _dev(gTz), scene_order=True)))
    assert all(np.any(w["means"]) for w in wants)
    total = {k: wants[0][k] + wants[1][k] for k in pr.FIELDS}
    pr.check_geometry("seed=264 kind=two cameras against the reference", pr.as_dict(out), total, pr.sum_bounds(*bounds))
    both = {k: singles[0][k] + singles[1][k] for k in pr.FIELDS}
    pr.check_geometry("seed=264 kind=two cameras against the single calls", pr.as_dict(out), both, pr.sum_bounds(*bounds))


def _quadrant_scene():
    """32x16 (two tiles), one small gaussian in the middle of each of the eight 8x8 quadrants, at eight depths: every gaussian's
    pixels lie in one wave of one tile, so the splat gradient's atomic sums have one addend each and are the same in every run."""
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
                  opacity_logit=np.zeros(n, np.float32), sh=np.zeros((n, 16, 3), np.float32))
    return {k: np.ascontiguousarray(v) for k, v in packed.items()}, args


def test_nothing_else_moved(G):
    """render_features and splat_gradient before and after a geometry_gradient on one Rasterizer are bit for bit the same."""
    packed, args = _quadrant_scene()
    R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(packed))
    cam, n = G.renderer.make_camera(*args), len(packed["means"])
    gen = torch.Generator().manual_seed(5)
    F, Gm = torch.randn((n, 17), generator=gen).cuda(), torch.randn((cam.height, cam.width, 17), generator=gen).cuda()
    gT = torch.randn((cam.height, cam.width), generator=gen).cuda()
    before = R.render_features(cam, F), R.splat_gradient(cam, F, Gm, gT)
    g = R.geometry_gradient(cam, F, Gm, gT)
    assert all(bool(t.any()) for t in g)
    after = R.render_features(cam, F), R.splat_gradient(cam, F, Gm, gT)
    assert torch.equal(before[0], after[0]) and bool(before[0].any())
    for a, b in zip(before[1][:3], after[1][:3]):
        assert torch.equal(a, b) and bool(a.any())
    # the scratch is the Rasterizer's and is zeroed per call: a second call gives what the first gave
    again = R.geometry_gradient(cam, F, Gm, gT)
    assert all(torch.equal(a, b) for a, b in zip(g, again))
