"""CPU: the float64 reference of the camera backward (tools/camera_reference.py) on the pinned fuzz cases, before the kernel is held
to it.  The bodies of the checks live in tests/camera_cases.py.

Per pin outside IDENTITIES_ONLY, scene order and camera (the pin's own and each of fuzz_maps.CAMERAS), over every gaussian the
oracle's loop draws — none is left out: vjp64 (explicit stage Jacobians with respect to w2c, full_proj, fx, fy) against torch's
float64 autograd of the monolithic project64 and against central finite differences in all 26 entries; the fp32 emulation of the
kernel's arrangement within 1e-5 B of it per entry, B = bound64, the chain in absolute values summed over the gaussians; and
renderer.pose_gradient's chain to a twist and a log-focal step against central differences of the loss with the camera fields
rebuilt in float64, the SH colours at the moved camera centre included.  The figures are printed ("camera ..." lines)."""
import pytest

from camera_cases import (CAMERAS, ORDERS, PINNED, assert_no_gaussian_on_the_clamp_band, camera_inputs as _inputs,
                          check_end_to_end_against_finite_differences, check_fp32_emulation_within_the_bound,
                          check_pose_gradient_against_finite_differences,
                          check_vjp64_against_autograd, check_vjp64_against_finite_differences, fm, sh_inputs, shr)
from gpu_cases import modules


@pytest.fixture(scope="module")
def G():
    return modules()


@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_vjp64_against_autograd(G, seed, order, camera):
    """|diff| <= 1e-10 |value| on the 26 sums; the columns the forward never reads get nothing."""
    check_vjp64_against_autograd(_inputs(G, seed, order, camera))


@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_vjp64_against_finite_differences(G, seed, order, camera):
    """Eight drawn gaussians per pin, all 26 camera entries, under splat_reference's rule (the one-gaussian pin 297 with the
    differences' own rounding, as tests/test_projection_reference.py differences it end to end)."""
    check_vjp64_against_finite_differences(_inputs(G, seed, order, camera), own_rounding=seed == 297)


@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_fp32_emulation_within_the_bound(G, seed, order, camera):
    """|emulation - vjp64| <= 1e-5 B per entry; the same arrangement in float64 is vjp64 to 1e-10 B."""
    check_fp32_emulation_within_the_bound(_inputs(G, seed, order, camera))


@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_pose_gradient_against_finite_differences(G, seed, order, camera):
    """The twist and the log-focal step against central differences of L(xi, log f), cam_center's term included."""
    check_pose_gradient_against_finite_differences(G, _inputs(G, seed, order, camera), sh_inputs(G, seed, order, camera))


@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", [s for s in PINNED if fm.PINS[s]["n"] <= 257])
def test_end_to_end_against_finite_differences(G, seed, order, camera):
    """The colour frame's loss through project64 and the SH colours at the moved camera, the support frozen, differenced in the
    twist and the two log-focals, against pose_gradient of vjp64 of the closed form's rows."""
    done = check_end_to_end_against_finite_differences(G, _inputs(G, seed, order, camera), seed)
    assert camera is not None or done == bool(fm.PINS[seed]["reached"])


@pytest.mark.parametrize("camera", CAMERAS)
def test_no_gaussian_is_left_out(G, camera):
    """No drawn gaussian of any pin lies within CLAMP_BAND of the ray clamp, under its own camera or a variant: every comparison
    above covers every drawn gaussian.  (The view rows pass no clamp: the SH band concerns the colours' own clamp, which the
    camera backward does not evaluate.)  Seed 351 under tilt_b has the clamp active on all its 89."""
    import numpy as np

    from camera_cases import pr
    for seed in PINNED:
        assert_no_gaussian_on_the_clamp_band(_inputs(G, seed, "file", camera))
    if camera == "tilt_b":
        c = _inputs(G, 351, "file", camera)
        assert len(c["k"]) == 89 and pr.clamp_state(c["drawn"], c["cam"])[0].any(1).all()
