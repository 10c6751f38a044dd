"""CPU: the float64 reference of the SH colour backward (tools/sh_reference.py) on the pinned fuzz cases, before the kernel is held
to it.

Per pin, scene order and degree 0-3, over EVERY gaussian (the operator has no cull): sh64's clamped colour against the oracle's
rgb; vjp64 (the transpose written out) against torch's float64 autograd of a monolithic sh_to_rgb, and against central finite
differences in the 51 parameters of eight gaussians; the fp32 emulation within 1e-5 B of it per element, B = bound64.  The entries
within CLAMP_BAND of a clamp edge are left out and capped.  Then the clamp's edges on a scene built on them.  The figures are
printed ("sh ..." lines): DESIGN.md's table is this printout.
"""
import numpy as np
import pytest
import torch

from backward_cases import (DEGREES, ORDERS, PINNED, check_sh_fp32_emulation_within_the_bound, check_sh_vjp64_against_autograd, fm,
                            sh_inputs as _inputs, shr, sr)
from gpu_cases import modules


@pytest.fixture(scope="module")
def G():
    return modules()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_sh64_against_the_oracle(G, seed, order):
    """|diff| <= 1e-5 max(|value|, the column's largest |value|) on rgb, at every degree."""
    c = _inputs(G, seed, order)
    worst = 0.0
    for degree in DEGREES:
        want = G.orc.preprocess(c["packed"], c["cam"], sh_degree=degree)["rgb"].astype(np.float64)
        got = shr.sh64(c["theta"], c["cam"], degree)["rgb"]
        lim = np.maximum(np.abs(want), np.abs(want).max(0, keepdims=True))
        worst = max(worst, float((np.abs(got - want) / np.maximum(lim, 1e-300)).max()))
        assert (np.abs(got - want) <= shr.ORACLE_REL * lim).all(), (seed, order, degree)
    print(f"\nsh oracle seed={seed} {order}: worst |diff| / max(|value|, column max) {worst:.2e}", end="")


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_vjp64_against_autograd(G, seed, order):
    """Autograd of the monolithic statement: |diff| <= 1e-10 |value| per element; B covers |value|; nothing beyond the degree."""
    check_sh_vjp64_against_autograd(_inputs(G, seed, order))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_vjp64_against_finite_differences(G, seed, order):
    """Eight gaussians per pin, all 51 parameters, of L = <g, clamp(v)>: |fd - g| <= FD_REL max_rows |g column| per parameter column
    (projection_reference's rule), at every degree.  Entries on the clamp band are not differenced."""
    c = _inputs(G, seed, order)
    n = c["n"]
    at = np.arange(n) if n <= sr.FD_ROWS else np.linspace(0, n - 1, sr.FD_ROWS).round().astype(int)
    worst = 0.0
    for degree in DEGREES:
        v = shr.vjp64(c["theta"], c["cam"], degree, c["g"])
        near = shr.near_clamp(c["theta"], c["cam"], degree).any(1)
        cols = dict(sh=v["sh"].reshape(n, -1), means=v["means"])
        for k in shr.FIELDS:
            scale = np.abs(cols[k]).max(0)
            for i in at:
                if near[i]:
                    continue
                t0 = shr.rows_of(c["theta"], [i])
                gi = c["g"][i].astype(np.float64)
                flat = t0[k].reshape(-1)
                for j in range(flat.size):
                    h = sr.FD_STEP * max(1.0, abs(flat[j]))
                    side = []
                    for sign in (1.0, -1.0):
                        t = {kk: a.copy() for kk, a in t0.items()}
                        t[k].reshape(-1)[j] += sign * h
                        side.append((gi * shr.sh64(t, c["cam"], degree)["rgb"][0]).sum())
                    fd = (side[0] - side[1]) / (2.0 * h)
                    err = abs(fd - cols[k][i, j])
                    worst = max(worst, err / max(scale[j], 1e-300)) if scale[j] else worst
                    assert err <= sr.FD_REL * scale[j] + 1e-300, (seed, order, degree, k, i, j, fd, cols[k][i, j])
    print(f"\nsh fd seed={seed} {order}: rows {len(at)}, worst |fd - g| / max |g column| {worst:.2e}", end="")


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_fp32_emulation_within_the_bound(G, seed, order):
    """|emulation - vjp64| <= 1e-5 B per element outside the band, from the scene's float32 arrays; at most CAP_LEFT_OUT entries
    left out per pin and degree; on a pin with n >= 64 a clamped and an unclamped channel are both compared."""
    check_sh_fp32_emulation_within_the_bound(_inputs(G, seed, order))


def test_the_clamp_is_covered(G):
    """4-12 % of the (gaussian, channel) entries of the larger pins are clamped at degree 3; seeds 378, 282 and 369 hold rows with all
    three channels clamped; the smallest |mean - cam_center| of any pin is above 0.05."""
    share, r_min = {}, np.inf
    for seed in PINNED:
        c = _inputs(G, seed, "file")
        fw = shr.sh64(c["theta"], c["cam"], 3)
        r_min = min(r_min, float(fw["r"].min()))
        if c["n"] >= 64:
            share[seed] = float((~fw["m"]).mean())
        if seed in (378, 282, 369):
            assert (~fw["m"]).all(1).any(), seed
    print(f"\nsh coverage: clamped share {min(share.values()):.3f} .. {max(share.values()):.3f}, smallest r {r_min:.3g}", end="")
    assert all(0.02 <= s <= 0.2 for s in share.values()), share
    assert r_min > 0.05


def test_the_clamp_edges_pass_and_beyond_stops(G):
    """The edge scene at degree 0: exactly 1 and exactly 0 pass, strictly inside passes, beyond gets nothing — in the emulation, in
    the float64 reference (the float32 products are exact in float64 only up to their rounding: the reference is asked at the
    float32 value) and in torch.clamp's autograd on the float32 forward."""
    packed, passes = shr.edge_scene()
    n = len(passes)
    cam = [0.0, 0.0, 0.0]
    g = np.ones((n, 3), np.float32)
    theta = shr.theta_of(packed)
    emu = shr.emulate_fp32(theta, cam, 0, g)
    assert np.array_equal(emu["sh"][:, 0, 0] != 0, passes)
    assert (emu["sh"][:, 0, 1:] != 0).all() and not emu["sh"][:, 1:].any() and not emu["means"].any()
    assert emu["v"][0, 0] == 1.0 and emu["v"][3, 0] == 0.0 and 0 < emu["v"][1, 0] < 1 and 0 < emu["v"][4, 0] < 1
    assert emu["v"][2, 0] > 1.0 and emu["v"][5, 0] < 0.0
    sh = torch.tensor(packed["sh"], requires_grad=True)
    v = torch.tensor(np.float32(shr.C0)) * sh[:, 0, :] + 0.5
    torch.clamp(v, 0.0, 1.0).sum().backward()
    assert np.array_equal(sh.grad.numpy()[:, 0, 0] != 0, passes)
