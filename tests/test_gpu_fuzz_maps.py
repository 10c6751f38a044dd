"""GPU: every map kernel against the float64 reference of tools/fuzz_maps.py, on the fuzz campaign's edge shapes.

The feature / channel blend, its backward, the pick maps, the top-k lists, the slab blend, the view statistics and the K-views-per-
launch variants, per pinned case (fuzz_maps.PINS: n = 1 .. 4096, frames of 15 - 33 pixels and one pixel high, equal-depth stacks,
opacity logits of -8 and 12, both generators) and per scene order: file order, where depth ties follow the file like the oracle's,
and the loaders' Morton order, with the reference built from the arrays in the scene's order.  tests/test_fuzz_maps_reference.py
holds the reference itself to the C oracle first, without a GPU.

The reference, the rules of what a comparison leaves out, the caps on that and the check functions live in tools/fuzz_maps.py
(`tools/fuzz_parity.py --maps` runs the same functions on fresh seeds); this file builds the cases, adds the exact layer — the prefix
sweep of gpu_cases.exact, bit for bit and with no pixel left out — and prints every measured figure ("fuzz-maps ..." lines).
Seed 283 has drawn neighbours closer than 8 ulps in depth: its draw order is not pinned by the reference, and it gets the
identities between the kernels only.
"""
import numpy as np
import pytest
import torch

from gpu_cases import NEVER, _tool, bar, exact, fuzz_case, namespace, z_cam

pytestmark = pytest.mark.gpu

fm = _tool("fuzz_maps")
PINNED = [s for s in fm.PINS if s not in fm.IDENTITIES_ONLY]
SWEPT = [s for s in PINNED if fm.PINS[s]["n"] <= fm.MAX_SWEEP_N]
ORDERS = ["file", "morton"]


@pytest.fixture(scope="module")
def G():
    return namespace()


def _case(G, seed, order):
    """The pinned case as a scene in `order` with its Rasterizer, the case's camera and two translated copies, each with its
    reference (the oracle fed the arrays in the scene's order), the features, the upstream gradients and the library's z_cam."""
    key = (seed, order)
    if key not in G.cases:
        c = fuzz_case(seed, fm.MAX_N)
        scene = G.renderer.GaussianScene.from_packed(c["packed"], spatial_order=order == "morton")
        assert (scene.order is None) == (order == "file")
        if scene.order is not None:
            assert np.array_equal(scene.order, G.renderer.morton_order(c["packed"]["means"]))
        views = [(G.renderer.make_camera(*args), ref) for args, ref in fm.case_views(G.orc, c, scene.order)]
        cam, ref = views[0]
        G.cases[key] = dict(seed=seed, R=G.renderer.Rasterizer(scene), cam=cam, ref=ref, views=views, packed=c["packed"],
                            F=fm.features_of(seed, c["n"]), Gm=fm.upstream_of(seed, c["H"], c["W"], len(views)),
                            z=z_cam(G, cam, c["packed"]["means"]))
    return G.cases[key]


def _report(seed, order, kind, fig):
    print(f"\nfuzz-maps seed={seed} order={order} kind={kind} " + " ".join(f"{k}={v:.3g}" for k, v in fig.items()), end="")


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_forward(G, seed, order):
    """render_features at 1, 3 and 17 channels with its final T, render_slab with open limits, and the drawn gaussians' own
    weights: the 100 dB bar, |T - T_ref| and |w - w_ref| <= 1e-4 (one threshold step on the excluded pixels), exactly 0 / 1 where
    the reference blends nothing."""
    c = _case(G, seed, order)
    fig = fm.run_forward(c["R"], c["cam"], c["ref"], c["F"], bar)
    assert ("w_err" in fig) == (fm.PINS[seed]["drawn"] > 0)  # the drawn gaussians' own weights were compared
    _report(seed, order, "forward", fig)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_slab(G, seed, order):
    c = _case(G, seed, order)
    _report(seed, order, "slab", fm.run_slab(c["R"], c["cam"], c["ref"], c["F"], c["z"], bar))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_backward(G, seed, order):
    c = _case(G, seed, order)
    _report(seed, order, "backward", fm.run_backward(c["R"], c["cam"], c["ref"], c["Gm"][0], bar))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_statistics(G, seed, order):
    c = _case(G, seed, order)
    _report(seed, order, "stats", fm.run_stats(c["R"], c["cam"], c["ref"], bar))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_pick(G, seed, order):
    c = _case(G, seed, order)
    _report(seed, order, "pick", fm.run_pick(c["R"], c["cam"], c["ref"]))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_topk(G, seed, order):
    c = _case(G, seed, order)
    _report(seed, order, "topk", fm.run_topk(c["R"], c["cam"], c["ref"]))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_k_views(G, seed, order):
    c = _case(G, seed, order)
    fig = fm.run_views(G.renderer, c["R"], c["views"], c["F"], c["Gm"], bar)
    assert fig["views_drawing"] == (3 if fm.PINS[seed]["reached"] else 0)
    _report(seed, order, "views", fig)


def _sorted_lists(W, appear, k, select):
    """The k heaviest (ties: the earlier in the prefix sweep) or the first k of the sweep among W > 0, as (ids, weights)."""
    n = W.shape[-1]
    if n < k:
        pad = W.new_zeros(W.shape[:2] + (k - n,))
        W, appear = torch.cat([W, pad], -1), torch.cat([appear, pad.to(appear.dtype)], -1)
    first = torch.argsort(torch.where(W > 0, appear, torch.full_like(appear, NEVER)), dim=-1, stable=True)
    if select == "heaviest":
        first = first.gather(-1, torch.argsort(-W.gather(-1, first), dim=-1, stable=True))
    idx = first[..., :k]
    ws = W.gather(-1, idx)
    return torch.where(ws > 0, idx.to(torch.int32), torch.full_like(idx, -1, dtype=torch.int32)), ws


@pytest.mark.parametrize("seed", SWEPT)
def test_exact_layer(G, seed):
    """Pick, count, top-k, weight_max and pixels bit for bit against the prefix sweep over render_features(eye(n)) — itself held to
    the reference by test_forward — on the file-order scene, no pixel left out."""
    c = _case(G, seed, "file")
    R, cam = c["R"], c["cam"]
    want = exact(G, c)
    for m in fm.MEDIANS:
        p = R.render_pick(cam, median_T=m, count=True)
        assert torch.equal(p.best_id, want["best_id"]) and torch.equal(p.best_w, want["best_w"]) and torch.equal(p.count, want["count"]), (seed, m)
        assert torch.equal(p.median_id, want["median_id"][m]), (seed, m)
    W, appear = c["W"], c["appear"]
    for select in ("heaviest", "nearest"):
        for k in fm.KS:
            ids, ws = _sorted_lists(W, appear, k, select)
            t = R.render_topk(cam, k, select=select, return_T=True)
            assert torch.equal(t.ids, ids) and torch.equal(t.weights, ws) and torch.equal(t.final_T, c["T"]), (seed, select, k)
    s = R.view_stats(cam)
    flat = W.flatten(0, 1)
    assert torch.equal(s.weight_max, flat.max(0).values) and torch.equal(s.pixels, (flat > 0).sum(0).to(torch.int32)), seed
    # ... and the sweep's weights are the reference's: what was just compared is not one kernel against itself
    err = np.abs(W.cpu().numpy()[..., c["ref"]["kept"]] - c["ref"]["w"])
    assert float(err.max(initial=0.0)) <= fm.STEP and float(err[~fm.excluded(c["ref"])].max(initial=0.0)) <= fm.W_TOL


@pytest.mark.parametrize("order", ORDERS)
def test_identities_where_the_draw_order_is_not_pinned(G, order):
    seed = fm.IDENTITIES_ONLY[0]
    c = _case(G, seed, order)
    f = fm.facts(c["ref"])
    assert f["drawn"] == fm.PINS[seed]["drawn"] and f["min_gap_ulps"] < 8  # why this seed gets identities only
    fig = fm.run_identities(G.renderer, c["R"], [cam for cam, _ in c["views"]], c["F"], c["Gm"][0])
    assert fig["drawn_px"] > 0 and fig["one_hot"] == 1
    _report(seed, order, "identities", fig)
