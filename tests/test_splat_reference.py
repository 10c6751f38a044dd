"""CPU: the float64 closed form of the splat gradient (tools/splat_reference.py) on the pinned fuzz cases, before the kernel is
held to it.

Per pin (all but the identities-only seed) and scene order: the closed form against central finite differences of the loss with
the support frozen; the share of pixels a comparison leaves out (the 1/255 band and the cap band) under fuzz_maps.CAP_PIXELS; and
the fp32 emulation of the kernel's arithmetic order — sequential P, S' - P_i — within 1e-5 (A + B) of the closed form per row and
column, A the row's own terms in absolute value and B the magnitude the subtraction works at.  The figures are printed: DESIGN.md's
table is this printout.
"""
import numpy as np
import pytest

from gpu_cases import _tool, fuzz_case, modules

fm = _tool("fuzz_maps")
sr = _tool("splat_reference")
PINNED = [s for s in fm.PINS if s not in fm.IDENTITIES_ONLY]
ORDERS = ["file", "morton"]


@pytest.fixture(scope="module")
def G():
    return modules()


def _inputs(G, seed, order):
    """The pin's reference with the features, the upstream gradients (zeroed on the left-out pixels) and the closed form at 17
    channels; built once and only read."""
    key = (seed, order)
    if key not in G.cases:
        c = fuzz_case(seed, fm.MAX_N)
        perm = G.renderer.morton_order(c["packed"]["means"]) if order == "morton" else None
        ref = fm.build_reference(G.orc, c["packed"], c["args"], perm)
        F = fm.features_of(seed, c["n"])
        Gz, gTz = sr.masked_inputs(ref, fm.upstream_of(seed, c["H"], c["W"])[0], sr.gT_of(seed, c["H"], c["W"]))
        G.cases[key] = dict(ref=ref, F=F, Gz=Gz, gTz=gTz, cf=sr.closed_form(ref, F, Gz, gTz))
    return G.cases[key]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_closed_form_against_finite_differences(G, seed, order):
    """Central differences in float64, step 1e-6 max(1, |value|), the support frozen at the base point, eight reached gaussians per
    pin, all six parameters: |fd - g| <= 1e-5 max_rows |g column|."""
    c = _inputs(G, seed, order)
    ref, cf = c["ref"], c["cf"]
    reached_d = cf["reached"][ref["kept"]]
    rows = sr.fd_rows(ref, reached_d)
    assert bool(len(rows)) == bool(fm.PINS[seed]["reached"])
    if not len(rows):
        assert not cf["g"].any()
        return
    fd = sr.finite_differences(ref, c["F"], c["Gz"], c["gTz"], rows)
    g = cf["g"][ref["kept"][rows], :6]
    scale = np.abs(cf["g"][:, :6]).max(0)
    rel = np.abs(fd - g) / np.maximum(scale, 1e-300)
    print(f"\nsplat fd seed={seed} {order}: rows {len(rows)}, worst |fd - g| / max |g column| {rel.max():.2e}", end="")
    assert (np.abs(fd - g) <= sr.FD_REL * scale).all(), (seed, order, rel.max(0))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_the_share_left_out_stays_under_the_cap(G, seed, order):
    ref = _inputs(G, seed, order)["ref"]
    band, cap = fm.excluded(ref), sr.cap_band(ref)
    print(f"\nsplat left out seed={seed} {order}: 1/255 band {100 * band.mean():.2f} %, cap band {100 * cap.mean():.2f} %, "
          f"together {100 * sr.left_out(ref).mean():.2f} %", end="")
    assert sr.left_out(ref).mean() <= fm.CAP_PIXELS
    assert not sr.left_out(ref).any() or not _inputs(G, seed, order)["Gz"][sr.left_out(ref)].any()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_fp32_emulation_against_the_closed_form(G, seed, order):
    """|err| <= 1e-5 (A + B) per row and column at C = 17, 3 and 1; rows the closed form never reaches are exactly 0."""
    c = _inputs(G, seed, order)
    ref, fig = c["ref"], {}
    for C in (17, 3, 1):
        cf = c["cf"] if C == 17 else sr.closed_form(ref, c["F"][:, :C], c["Gz"][..., :C], c["gTz"])
        emu = sr.emulate_fp32(ref, c["F"][:, :C], c["Gz"][..., :C], c["gTz"])
        sr.check_gradient(f"emulation seed={seed} {order} C={C}", emu, cf, list(range(8)), fig)


def test_the_bound_without_B_fails_on_the_deep_stacks(G):
    """Why B is part of the bound: on the deep-stack pins the emulation exceeds 1e-5 A alone, by construction of S' - P_i."""
    worst = 0.0
    for seed in (351, 327):
        c = _inputs(G, seed, "file")
        emu = sr.emulate_fp32(c["ref"], c["F"], c["Gz"], c["gTz"])
        cf = dict(c["cf"], B=np.zeros_like(c["cf"]["B"]))
        worst = max(worst, sr.bound_ratio(emu, cf, list(range(6))))
    print(f"\nsplat emulation without B: |err| / (1e-5 A) up to {worst:.3g}", end="")
    assert worst > 1.0


def test_min_T_masks_the_pairs_behind_it(G):
    """closed_form(min_T): pairs with T_i < min_T carry e = 0 but still count in what lies in front of the others."""
    c = _inputs(G, 327, "file")
    ref = c["ref"]
    full, cut = c["cf"], sr.closed_form(ref, c["F"], c["Gz"], c["gTz"], min_T=1e-2)
    assert (cut["A"] <= full["A"]).all() and (cut["A"] < full["A"]).any() and cut["reached"].sum() <= full["reached"].sum()
    first = ref["kept"][0]  # the nearest drawn gaussian sees T = 1 everywhere: untouched by the mask
    assert np.array_equal(cut["g"][first], full["g"][first])
