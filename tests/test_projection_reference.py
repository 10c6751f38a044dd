"""CPU: the float64 reference of the projection backward (tools/projection_reference.py) on the pinned fuzz cases, before the
kernel is held to it.  The bodies of the checks live in tests/backward_cases.py: tests/test_camera_variants.py runs them again under
rolled, oblique, anamorphic cameras.

Per pin and scene order, over every gaussian the oracle's loop draws: project64 against the oracle's own opacity, screen means and
conics; vjp64 (the chain of explicit stage Jacobians) against torch's float64 autograd of the monolithic project64, against the
kernel's fused arrangement of the chain in float64, and against central finite differences; the fp32 emulation within 1e-5 B of it
per element, B = bound64, the chain in absolute values.  Then end to end: the loss of splat_reference.loss_pixels through
project64, differenced in the scene's parameters, against vjp64 of the closed-form splat rows.  The figures are printed
("project ..." lines): DESIGN.md's table is this printout.
"""
import numpy as np
import pytest

from backward_cases import (PINNED, PINS, ORDERS, check_end_to_end_against_finite_differences, check_fp32_emulation_within_the_bound,
                            check_project64_against_the_oracle, check_vjp64_against_autograd_and_the_fused_form,
                            check_vjp64_against_finite_differences, fm, pr, projection_inputs as _inputs, splat_inputs as _splat_inputs, sr)
from gpu_cases import modules


@pytest.fixture(scope="module")
def G():
    return modules()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINS)
def test_project64_against_the_oracle(G, seed, order):
    """|diff| <= 1e-5 max(|value|, the column's largest |value|) on opacity, screen means and conics."""
    check_project64_against_the_oracle(_inputs(G, seed, order))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINS)
def test_vjp64_against_autograd_and_the_fused_form(G, seed, order):
    """Autograd of the monolithic project64: |diff| <= 1e-10 |value| per element.  The kernel's fused arrangement in float64 (a check
    of this project's own, beyond the autograd one): |diff| <= 1e-10 B, the magnitude its differently ordered sums work at."""
    check_vjp64_against_autograd_and_the_fused_form(_inputs(G, seed, order))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINS)
def test_vjp64_against_finite_differences(G, seed, order):
    """Eight drawn gaussians per pin, all eleven parameters, of L = <rows, (opacity, screen mean, conic)>."""
    check_vjp64_against_finite_differences(_inputs(G, seed, order))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINS)
def test_fp32_emulation_within_the_bound(G, seed, order):
    """|emulation - vjp64| <= 1e-5 B per element, from the scene's float32 arrays."""
    check_fp32_emulation_within_the_bound(_inputs(G, seed, order))


def test_the_clamp_and_the_quaternion_norms_are_covered(G):
    """No drawn gaussian of any pin sits on the clamp's band; seed 301 has 26 REACHED gaussians with the clamp active and six more
    pins have some; the stored quaternion norms span 0.16 .. 4.8."""
    active, norms = {}, []
    for seed in PINS:
        c = _inputs(G, seed, "file")
        if not len(c["k"]):
            continue
        act, near = pr.clamp_state(c["drawn"], c["cam"])
        assert not near.any(), seed
        active[seed] = act.any(1)
        norms.append(np.linalg.norm(c["drawn"]["quats"], axis=1))
    for seed in (322, 277, 354, 327, 283, 369):
        assert active[seed].any(), seed
    c = _inputs(G, 301, "file")
    F, Gz, gTz = _splat_inputs(c, 301)
    reached = sr.closed_form(c["ref"], F, Gz, gTz)["reached"][c["ref"]["kept"]]
    assert int((active[301] & reached).sum()) == 26
    norms = np.concatenate(norms)
    print(f"\nproject coverage: clamp active on {({s: int(a.sum()) for s, a in active.items() if a.any()})}; |q| {norms.min():.3g} .. {norms.max():.3g}", end="")
    assert norms.min() < 0.17 and norms.max() > 4.7


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_end_to_end_against_finite_differences(G, seed, order):
    """L = sum_p splat_reference.loss_pixels(ref, project64(theta), F, G, gT), the support frozen, differenced in the eleven
    parameters of eight reached gaussians, against vjp64 of the closed form's rows."""
    # every pin by the plain rule but the one-gaussian pin 297: there |fd - g| is 3 .. 7e-10 on all three log-scale entries, whatever
    # their size (1e-5 .. 1.6e-4): the floor of differencing 256 pixel losses of size ~25 at h = 3e-6 in float64, against a column
    # "maximum" of 1.1e-5
    rows = check_end_to_end_against_finite_differences(_inputs(G, seed, order), seed, own_rounding=seed == 297)
    assert bool(rows) == bool(fm.PINS[seed]["reached"])
