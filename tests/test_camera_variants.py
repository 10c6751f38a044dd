"""CPU: the pinned fuzz cases under rolled, oblique, anamorphic cameras (fuzz_maps.CAMERAS), before the kernels that read GsrCamera
are held to them (tests/test_gpu_camera_variants.py).

Every pinned camera comes from synthetic.look_at_pose or box_camera, which never roll: the rotation block of w2c always holds an
exactly zero entry (w2c[2][0] in every view; six of nine under box_camera), and focal_x == focal_y.  A backward that indexes
V[4 k + m], fx / fy and lim_x / lim_y by hand can be wrong in exactly those places and pass.  fuzz_maps.camera_variant turns the
world about its origin, rolls the image and scales focal_y; this file holds, per (pin, variant):

  - gsr_camera_setup's struct equal to the oracle's, field for field;
  - what the GPU comparisons rest on, on the references alone: no rotation entry at zero, the draw order pinned, the shares the map
    comparisons leave out under their caps, no drawn gaussian on the ray clamp's band, no SH entry on the colour clamp's band;
  - the references themselves by the checks of test_projection_reference.py and test_sh_reference.py (tests/backward_cases.py holds
    the bodies: one rule, one tolerance): project64 against the oracle, vjp64 against autograd, the fp32 emulation within 1e-5 B;
    finite differences on tilt_a;
  - that the inputs discriminate: three one-token mutants of the kernel's fused form, two of which every pinned camera lets pass.
"""
import numpy as np
import pytest

from backward_cases import (PINNED, check_end_to_end_against_finite_differences, check_fp32_emulation_within_the_bound,
                            check_project64_against_the_oracle, check_sh_fp32_emulation_within_the_bound,
                            check_sh_vjp64_against_autograd, check_vjp64_against_autograd_and_the_fused_form,
                            check_vjp64_against_finite_differences, fm, pr, projection_inputs, sh_inputs, shr)
from gpu_cases import assert_same_camera, modules

CAMERAS = list(fm.CAMERAS)
SHARES = ("pixels", "tiny", "best", "median")  # no pick or top-k checks run under the variants: the slot caps are not claimed
ROTATION_FLOOR = 1e-3                          # the smallest |w2c[:3, :3]| entry on a pin that draws something is 0.007


@pytest.fixture(scope="module")
def G():
    return modules()


def test_the_variants_are_what_the_issue_names_and_the_pins_are_untouched():
    assert fm.CAMERAS == {"tilt_a": (33.0, 1.3, (1, 2, 3), 25.0), "tilt_b": (-117.0, 0.75, (3, -1, 2), -40.0)}
    args = (np.array([1.0, 0.0, 0.0, 0.0]), np.array([1.0, 2.0, 3.0]), 10.0, 10.0, 32, 16, 32, 16)
    q, t, fx, fy = fm.camera_variant(args, 90.0, 1.5, (0, 0, 1), -90.0)[:4]  # a roll and the opposite orbit about z cancel
    assert np.allclose(q, [1, 0, 0, 0], atol=1e-15) and np.allclose(t, [-2.0, 1.0, 3.0], atol=1e-15) and (fx, fy) == (10.0, 15.0)
    assert fm.camera_variant(args, 0.0, 1.0, (1, 0, 0), 0.0)[4:] == args[4:]


@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("seed", PINNED)
def test_camera_setup_matches_the_oracle(G, seed, camera):
    """Field for field, bit for bit; and the variant is what camera_variant says: w2c's rotation is R_z(roll) R R(axis, orbit)."""
    c = projection_inputs(G, seed, "file", camera)
    args = fm.camera_variant(c["c"]["args"], *fm.CAMERAS[camera])
    cam = G.renderer.make_camera(*args)
    assert_same_camera(cam, c["cam"])
    own = pr.camera_of(G.orc.camera(*c["c"]["args"]))
    got = pr.camera_of(cam)
    roll, ratio, axis, orbit = fm.CAMERAS[camera]

    def rot(axis, deg):  # Rodrigues
        a, th = np.asarray(axis, np.float64) / np.linalg.norm(axis), np.deg2rad(deg)
        K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
        return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)

    # (w2c is stored for row vectors: its rotation block is R^T and its last row the translation)
    assert np.abs(got["V"][:3, :3].T - rot((0, 0, 1), roll) @ own["V"][:3, :3].T @ rot(axis, orbit)).max() <= 1e-6
    assert np.abs(got["V"][3, :3] - rot((0, 0, 1), roll) @ own["V"][3, :3]).max() <= 1e-6 * max(1.0, np.abs(own["V"][3, :3]).max())
    assert got["fx"] == own["fx"] and abs(got["fy"] / own["fy"] - ratio) <= 1e-6
    assert got["limx"] == own["limx"] and got["limy"] != own["limy"] and (got["W"], got["H"]) == (own["W"], own["H"])


@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("seed", PINNED)
def test_what_the_gpu_comparisons_rest_on(G, seed, camera):
    """On the references alone: no zero in w2c's rotation; the reference is the C oracle's compositing loop to 1e-6 and its draw
    order is pinned (>= 16 ulps between drawn neighbours of different depth); the shares left out are under fuzz_maps.CAPS; no
    drawn gaussian is on the ray clamp's band; no SH entry is on the colour clamp's band at any degree."""
    c = projection_inputs(G, seed, "file", camera)
    pin, ref = fm.PINS[seed], c["ref"]
    R = np.abs(pr.camera_of(c["cam"])["V"][:3, :3])
    f, share = fm.facts(ref), fm.shares(ref)
    assert R.min() > 0.0 and (R.min() >= ROTATION_FLOOR or not pin["drawn"]), R.min()
    assert pr.camera_of(c["cam"])["fx"] != pr.camera_of(c["cam"])["fy"]
    dw, dT = fm.oracle_agreement(G.orc, ref)
    assert dw <= 1e-6 and dT <= 1e-6
    assert f["min_gap_ulps"] >= 16
    assert bool(f["drawn"]) == bool(pin["drawn"]) and bool(f["reached"]) == bool(pin["reached"])
    for k in SHARES:
        assert share[k] <= fm.CAPS[k], (seed, camera, k, share[k])
    active = 0
    if f["drawn"]:
        act, near = pr.clamp_state(c["drawn"], c["cam"])
        assert not near.any()
        active = int(act.any(1).sum())
    s = sh_inputs(G, seed, "file", camera)
    left_out = [shr.keep_mask(s["theta"], s["cam"], degree)[2] for degree in (0, 1, 2, 3)]
    assert max(left_out) == 0 <= shr.CAP_LEFT_OUT
    print(f"\ncamera {camera} seed={seed}: min |R| {R.min():.3f}, drawn {f['drawn']} ({pin['drawn']}), reached {f['reached']} ({pin['reached']}), "
          f"clamp active on {active}, min gap {f['min_gap_ulps']} ulps; left out: " + ", ".join(f"{k} {100 * share[k]:.2f} %" for k in SHARES), end="")
    if (seed, camera) == (369, "tilt_b"):
        assert (f["drawn"], f["reached"]) == (398, 279)
    if (seed, camera) == (351, "tilt_b"):  # every drawn gaussian with the ray clamp active
        assert (f["drawn"], f["reached"], active) == (89, 46, 89)


@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("seed", PINNED)
def test_the_projection_reference_holds(G, seed, camera):
    """test_projection_reference.py's oracle, autograd / fused-form and fp32-emulation checks, at their own bars."""
    c = projection_inputs(G, seed, "file", camera)
    check_project64_against_the_oracle(c)
    check_vjp64_against_autograd_and_the_fused_form(c)
    check_fp32_emulation_within_the_bound(c)


@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("seed", PINNED)
def test_the_sh_reference_holds(G, seed, camera):
    """test_sh_reference.py's autograd and fp32-emulation checks at degrees 0 to 3 (the SH chain reads the camera's centre only)."""
    c = sh_inputs(G, seed, "file", camera)
    check_sh_vjp64_against_autograd(c)
    check_sh_fp32_emulation_within_the_bound(c)


@pytest.mark.parametrize("seed", [264, 301, 354, 252])
def test_vjp64_against_finite_differences_under_tilt_a(G, seed):
    check_vjp64_against_finite_differences(projection_inputs(G, seed, "file", "tilt_a"))


@pytest.mark.parametrize("seed", [264, 354])
def test_end_to_end_against_finite_differences_under_tilt_a(G, seed):
    assert check_end_to_end_against_finite_differences(projection_inputs(G, seed, "file", "tilt_a"), seed) > 0


# ---- the inputs discriminate ---------------------------------------------------------------------------------------------------------
class _References:
    """The namespace projection_inputs needs in file order, and nothing else: the oracle and a cache."""

    def __init__(self):
        from oracle import cpu_oracle

        self.orc, self.cases = cpu_oracle, {}


def test_the_pinned_cameras_pass_two_mutants_that_the_variants_catch():
    """Three one-token slips of the hand-indexed backward, applied to projection_reference.fused_vjp (the fp32 statement of the
    kernel's arrangement) and held to vjp64 by the GPU test's own rule, worst |err| / (1e-5 B) over the four arrays:
      fx_for_fy       d cam_mean_y takes J00 for J11           own cameras 0.41 (passes)   tilt_a 1.0e4   tilt_b 9.7e3
      w2c20_dropped   the V[8] = w2c[2][0] terms are missing   own cameras 0.41 (passes)   tilt_a 2.8e4   tilt_b 5.6e4
      limx_for_limy   the y clamp is decided against lim_x     own cameras 1.3e4           tilt_a 7.6e3   tilt_b 3.2e4
    The first two stay within the bound on EVERY pin under its own camera — what the suite could not see; all three exceed it on at
    least five pins under each variant.  Only the references take part: no kernel, nothing of the GPU library."""
    H = _References()
    worst = {(m, cam): [] for m in (None,) + pr.MUTANTS for cam in [None] + CAMERAS}
    for camera in [None] + CAMERAS:
        for seed in PINNED:
            c = projection_inputs(H, seed, "file", camera)
            if not len(c["k"]):
                continue
            v, B = pr.vjp64(c["drawn"], c["cam"], c["rows"]), pr.bound64(c["drawn"], c["cam"], c["rows"])
            for m in (None,) + pr.MUTANTS:
                worst[(m, camera)].append(max(pr.worst_ratios(pr.fused_vjp(c["drawn"], c["cam"], c["rows"], mutant=m), v, B).values()))
    for m in (None,) + pr.MUTANTS:
        print(f"\nmutant {m}: worst |err| / (1e-05 B) " + "  ".join(
            f"{cam or 'own'} {max(worst[(m, cam)]):.3g} ({sum(w > 1.0 for w in worst[(m, cam)])} of {len(worst[(m, cam)])} pins over)"
            for cam in [None] + CAMERAS), end="")
    for camera in [None] + CAMERAS:
        assert max(worst[(None, camera)]) <= 1.0
    for m in ("fx_for_fy", "w2c20_dropped"):
        assert max(worst[(m, None)]) <= 1.0 and worst[(m, None)] == worst[(None, None)]  # the hole: not one bit moves
    assert max(worst[("limx_for_limy", None)]) > 1.0
    for m in pr.MUTANTS:
        for camera in CAMERAS:
            assert sum(w > 1.0 for w in worst[(m, camera)]) >= 5, (m, camera, worst[(m, camera)])
