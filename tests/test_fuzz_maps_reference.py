"""CPU: the float64 reference of the map kinds (tools/fuzz_maps.py) on the pinned fuzz cases, before any GPU kernel is held to it.

Per pin (all but the identities-only seed) and scene order: the reference equals the C oracle's own fp32 compositing loop — one-hot
weights and final T — to 1e-6; the pin still is what its row of fuzz_maps.PINS says (size, drawn, reached, deepest pixel, tied
neighbours); drawn neighbours of different depth are >= 16 fp32 ulps apart, so that the draw order is pinned; and every share a GPU
comparison leaves out stays under its cap on the reference alone.  The shares are printed: DESIGN.md's table is this printout.
"""
import numpy as np
import pytest

from gpu_cases import _tool, fuzz_case, modules

fm = _tool("fuzz_maps")
PINNED = [s for s in fm.PINS if s not in fm.IDENTITIES_ONLY]


@pytest.fixture(scope="module")
def G():
    return modules()


def _reference(G, seed, order):
    key = (seed, order)
    if key not in G.cases:
        c = fuzz_case(seed, fm.MAX_N)
        perm = G.renderer.morton_order(c["packed"]["means"]) if order == "morton" else None
        G.cases[key] = (c, fm.build_reference(G.orc, c["packed"], c["args"], perm))
    return G.cases[key]


def test_the_table_names_every_case_of_the_issue():
    assert len(fm.PINS) == 20 and fm.IDENTITIES_ONLY == (283,)
    sizes = {p["n"] for p in fm.PINS.values()}
    assert {1, 2, 63, 64, 65, 256, 257, 4096} <= sizes
    assert {15, 16, 17, 31, 33} <= {p["W"] for p in fm.PINS.values()} | {p["H"] for p in fm.PINS.values()}
    assert any(p["H"] == 1 for p in fm.PINS.values())
    for seed in fm.PINS:  # the identities-only seed too: its size and its aim
        c = fuzz_case(seed, fm.MAX_N)
        assert (c["n"], c["W"], c["H"]) == tuple(fm.PINS[seed][k] for k in "nWH"), seed
    assert {fuzz_case(s, fm.MAX_N)["gen"].__name__ for s in fm.PINS} == {"mip360_like", "uniform_box"}


@pytest.mark.parametrize("order", ["file", "morton"])
@pytest.mark.parametrize("seed", PINNED)
def test_reference_against_the_c_oracle_and_the_caps(G, seed, order):
    c, ref = _reference(G, seed, order)
    pin = fm.PINS[seed]
    dw, dT = fm.oracle_agreement(G.orc, ref)
    f, sh = fm.facts(ref), fm.shares(ref)
    print(f"\nseed {seed} {order}: |w - w_oracle| {dw:.2e}, |T - T_oracle| {dT:.2e}; drawn {f['drawn']}, reached {f['reached']}, deepest "
          f"{f['deepest']}, ties {f['ties']}, min gap {f['min_gap_ulps']} ulps, min T {f['min_T']:.1e}; left out: "
          + ", ".join(f"{k} {100 * v:.2f} %" for k, v in sh.items()), end="")
    assert dw <= 1e-6 and dT <= 1e-6
    assert {k: f[k] for k in ("drawn", "reached", "deepest", "ties")} == {k: pin[k] for k in ("drawn", "reached", "deepest", "ties")}
    assert f["min_gap_ulps"] >= 16
    assert f["empty"] == (pin["reached"] == 0)
    for k, cap in fm.CAPS.items():
        assert sh[k] <= cap, (seed, k, sh[k])
    # the same weights under the names the checks use: the map of ones is 1 - T up to rounding, the gradient its transpose
    ones = np.ones((ref["n"], 1))
    assert np.abs(fm.feature_map(ref, ones)[..., 0] + fm.final_T(ref) - 1.0).max(initial=0.0) <= 1e-12
    st = fm.stats(ref, ref["n"])
    assert np.allclose(fm.gradient(ref, np.ones((ref["H"], ref["W"], 1)), ref["n"])[:, 0], st["weight_sum"], rtol=1e-12, atol=0)
    p = fm.pick(ref, 0.5)
    assert int(st["pixels_hi"].sum()) == int(p["count_hi"].sum())
    for select in ("heaviest", "nearest"):
        t = fm.topk(ref, 1, select)
        want = p if select == "heaviest" else fm.pick(ref, 1.0)
        assert np.array_equal(t["ids"][..., 0], want["best_id" if select == "heaviest" else "median_id"])


def test_what_the_pins_are_aimed_at(G):
    for seed in (290, 324, 263):  # full lists (or a frame that draws nothing), and not one pair above 1/255
        _, ref = _reference(G, seed, "file")
        assert not (ref["alpha"] > 0).any() and (fm.final_T(ref) == 1).all()
        assert seed == 263 or np.isfinite(ref["band"]).sum() > 1000  # ... though the bboxes hold plenty of pairs
    for seed in (301, 277):  # logit 12: every gaussian's peak alpha is at the cap
        c, ref = _reference(G, seed, "file")
        assert (c["packed"]["opacity_logit"] == 12).all() and float(ref["alpha"].max()) == fm.MAX_ALPHA
    for seed in (264, 322, 351, 327):  # one slab edge lies on a depth two reached gaussians share
        _, ref = _reference(G, seed, "file")
        z = ref["z"][(ref["w"] > 0).any((0, 1))]
        near, far = fm.slab_edges(ref)[0][1], fm.slab_edges(ref)[1][0]
        assert near == far and (z == np.float32(near)).sum() >= 2
        front, back = (len(fm.slab(ref, *fm.slab_edges(ref)[i])["kept"]) for i in (0, 1))
        assert front + back == len(ref["kept"]) and back >= 2 and (front > 0 or len(np.unique(z)) == 1), (seed, front, back)
    _, ref = _reference(G, 354, "file")  # one tile, one entry past a 256-entry batch
    assert ref["W"] <= 16 and ref["H"] <= 16 and len(ref["kept"]) == 257
    _, ref = _reference(G, 351, "file")
    assert float(fm.final_T(ref).min()) < 1e-45  # below the smallest fp32 denormal: fp32 T is 0 there
    assert fm.tiny(ref).any()
    for seed in PINNED:  # the translated views of the K-view tests still draw something
        c, ref = _reference(G, seed, "file")
        views = fm.case_views(G.orc, c)
        assert len(views) == 3 and all(((r["w"] > 0).any() for _, r in views)) == bool((ref["w"] > 0).any()), seed
