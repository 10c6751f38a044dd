"""CPU: the float64 reference of the projection backward (tools/projection_reference.py) on the pinned fuzz cases, before the
kernel is held to it.

Per pin and scene order, over every gaussian the oracle's loop draws: project64 against the oracle's own opacity, screen means and
conics; vjp64 (the chain of explicit stage Jacobians) against torch's float64 autograd of the monolithic project64, against the
kernel's fused arrangement of the chain in float64, and against central finite differences; the fp32 emulation within 1e-5 B of it
per element, B = bound64, the chain in absolute values.  Then end to end: the loss of splat_reference.loss_pixels through
project64, differenced in the scene's parameters, against vjp64 of the closed-form splat rows.  The figures are printed
("project ..." lines): DESIGN.md's table is this printout.
"""
import numpy as np
import pytest
import torch

from gpu_cases import _tool, fuzz_case, modules

fm = _tool("fuzz_maps")
sr = _tool("splat_reference")
pr = _tool("projection_reference")
PINS = list(fm.PINS)
PINNED = [s for s in fm.PINS if s not in fm.IDENTITIES_ONLY]
ORDERS = ["file", "morton"]
E2E_CH = 3  # channels of the end-to-end loss: the chain does not depend on them


@pytest.fixture(scope="module")
def G():
    return modules()


def _inputs(G, seed, order):
    """The pin's reference, the oracle's camera, theta in the scene's order and its drawn gaussians `k` (draw order) with their
    seeded unit-normal rows; built once and only read."""
    key = (seed, order)
    if key not in G.cases:
        c = fuzz_case(seed, fm.MAX_N)
        perm = G.renderer.morton_order(c["packed"]["means"]) if order == "morton" else None
        ref = fm.build_reference(G.orc, c["packed"], c["args"], perm)
        theta, k = pr.theta_of(c["packed"], perm), ref["kept_in"]
        assert len(k) == fm.PINS[seed]["drawn"]
        G.cases[key] = dict(c=c, ref=ref, cam=G.orc.camera(*c["args"]), theta=theta, k=k, drawn=pr.rows_of(theta, k),
                            rows=pr.unit_rows(seed, len(k), np.arange(len(k))))
    return G.cases[key]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINS)
def test_project64_against_the_oracle(G, seed, order):
    """|diff| <= 1e-5 max(|value|, the column's largest |value|) on opacity, screen means and conics."""
    c = _inputs(G, seed, order)
    if not len(c["k"]):
        return
    fw, pre, worst = pr.project64(c["drawn"], c["cam"]), c["ref"]["pre"], 0.0
    assert bool(pr.contributes(fw).all())  # what the oracle draws, the backward carries
    for name in ("opacity", "screen_means", "sigmas"):
        got = fw[name].numpy().reshape(len(c["k"]), -1)
        want = pre[name][c["k"]].astype(np.float64).reshape(len(c["k"]), -1)
        lim = np.maximum(np.abs(want), np.abs(want).max(0, keepdims=True))
        worst = max(worst, float((np.abs(got - want) / lim).max()))
        assert (np.abs(got - want) <= pr.ORACLE_REL * lim).all(), (seed, order, name)
    print(f"\nproject oracle seed={seed} {order}: worst |diff| / max(|value|, column max) {worst:.2e}", end="")


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINS)
def test_vjp64_against_autograd_and_the_fused_form(G, seed, order):
    """Autograd of the monolithic project64: |diff| <= 1e-10 |value| per element.  The kernel's fused arrangement in float64 (a check
    of this project's own, beyond the autograd one): |diff| <= 1e-10 B, the magnitude its differently ordered sums work at."""
    c = _inputs(G, seed, order)
    if not len(c["k"]):
        return
    v, B = pr.vjp64(c["drawn"], c["cam"], c["rows"]), pr.bound64(c["drawn"], c["cam"], c["rows"])
    t = {k: torch.tensor(a, dtype=torch.float64, requires_grad=True) for k, a in c["drawn"].items()}
    o, r = pr.project64(t, c["cam"]), torch.as_tensor(c["rows"], dtype=torch.float64)
    ((r[:, 0] * o["opacity"]).sum() + (r[:, 1:3] * o["screen_means"]).sum() + (r[:, 3:6] * o["sigmas"]).sum()).backward()
    auto = {k: t[k].grad.numpy() for k in pr.FIELDS}
    fused = pr.fused_vjp(c["drawn"], c["cam"], c["rows"], torch.float64)
    fa = pr.worst_ratios(auto, v, {k: np.abs(v[k]) for k in pr.FIELDS}, pr.AUTOGRAD_REL)
    ff = pr.worst_ratios(fused, v, B, pr.AUTOGRAD_REL)
    print(f"\nproject autograd seed={seed} {order}: worst |diff| / (1e-10 |value|) autograd {max(fa.values()):.2e}; "
          f"|diff| / (1e-10 B) fused {max(ff.values()):.2e}", end="")
    assert max(fa.values()) <= 1.0 and max(ff.values()) <= 1.0
    for k in pr.FIELDS:
        assert (B[k] >= np.abs(v[k]) * (1 - 1e-12)).all() and np.any(v[k])


def _fd(value_of, theta_i):
    """Central differences of value_of(theta of one gaussian) — an array of per-pixel or per-term losses, differenced before it is
    summed — in its eleven parameters, step FD_STEP max(1, |value|).  -> (the differences, their own rounding): every differenced
    term is a float64 good to no better than one rounding, 2^-53 |term|, and the quotient divides that by 2 h."""
    out, noise = {}, {}
    for k in pr.FIELDS:
        flat, own = np.zeros(theta_i[k].size), np.zeros(theta_i[k].size)
        for j in range(theta_i[k].size):
            h = sr.FD_STEP * max(1.0, abs(theta_i[k].reshape(-1)[j]))
            side = []
            for sign in (1.0, -1.0):
                t = {kk: v.copy() for kk, v in theta_i.items()}
                t[k].reshape(-1)[j] += sign * h
                side.append(value_of(t))
            flat[j] = (side[0] - side[1]).sum() / (2.0 * h)
            own[j] = 2.0 ** -53 * (np.abs(side[0]) + np.abs(side[1])).sum() / (2.0 * h)
        out[k], noise[k] = flat, own
    return out, noise


def _fd_against(tag, fd_rows, g, at, own_rounding=False):
    """splat_reference's rule: |fd - g| <= FD_REL max_rows |g column|, per parameter column.  own_rounding: plus the differences'
    own rounding (_fd): for the one-gaussian pin alone, whose column "maximum" is its only entry and itself a sum that cancels."""
    worst = 0.0
    for k in pr.FIELDS:
        col = g[k].reshape(len(g[k]), -1)
        scale = np.abs(col).max(0)
        for (fd, own), i in zip(fd_rows, at):
            worst = max(worst, float((np.abs(fd[k] - col[i]) / np.maximum(scale, 1e-300)).max()))
            assert (np.abs(fd[k] - col[i]) <= sr.FD_REL * scale + (own[k] if own_rounding else 0.0)).all(), (tag, k, i, fd[k], col[i], own[k])
    print(f"\nproject fd {tag}: rows {len(at)}, worst |fd - g| / max |g column| {worst:.2e}", end="")


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINS)
def test_vjp64_against_finite_differences(G, seed, order):
    """Eight drawn gaussians per pin, all eleven parameters, of L = <rows, (opacity, screen mean, conic)>."""
    c = _inputs(G, seed, order)
    if not len(c["k"]):
        return
    v = pr.vjp64(c["drawn"], c["cam"], c["rows"])
    at = sr.fd_rows(c["ref"], np.ones(len(c["k"]), bool))
    fds = []
    for i in at:
        row = c["rows"][i].astype(np.float64)

        def value_of(t):
            o = pr.project64(t, c["cam"])
            return np.concatenate([row[:1] * o["opacity"].numpy(), row[1:3] * o["screen_means"].numpy()[0], row[3:6] * o["sigmas"].numpy()[0]])

        fds.append(_fd(value_of, pr.rows_of(c["drawn"], [i])))
    _fd_against(f"seed={seed} {order}", fds, v, at)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINS)
def test_fp32_emulation_within_the_bound(G, seed, order):
    """|emulation - vjp64| <= 1e-5 B per element, from the scene's float32 arrays."""
    c = _inputs(G, seed, order)
    if not len(c["k"]):
        return
    v, B = pr.vjp64(c["drawn"], c["cam"], c["rows"]), pr.bound64(c["drawn"], c["cam"], c["rows"])
    pr.check_geometry(f"emulation seed={seed} {order}", pr.emulate_fp32(c["drawn"], c["cam"], c["rows"]), v, B)


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


def _splat_inputs(c, seed):
    cc, ref = c["c"], c["ref"]
    Gz, gTz = sr.masked_inputs(ref, fm.upstream_of(seed, cc["H"], cc["W"])[0], sr.gT_of(seed, cc["H"], cc["W"]))
    return fm.features_of(seed, cc["n"])[:, :E2E_CH], Gz[..., :E2E_CH], gTz


def _reference_at_project64(c):
    """The pin's reference recomposed AT project64's values of the drawn gaussians' opacity, screen means and conics (the oracle's
    are fp32: 1e-7 away, which a gradient of exp(power) shows at 1e-5), so that the closed form and the differenced loss are
    taken at one point.  The drawn set and its order are the oracle's."""
    if "ref64" not in c:
        ref, k = c["ref"], c["k"]
        fw = pr.project64(c["drawn"], c["cam"])
        pre = dict(ref["pre"])
        for name in ("opacity", "screen_means", "sigmas"):
            pre[name] = ref["pre"][name].astype(np.float64)
            pre[name][k] = fw[name].numpy()
        at = fm.reference(pre, ref["order"], ref["W"], ref["H"])
        assert np.array_equal(at["kept"], ref["kept_in"])
        at.update(pre=pre, order=ref["order"], kept_in=at["kept"], kept=ref["kept"], n=ref["n"], W=ref["W"], H=ref["H"])
        c["ref64"] = at
    return c["ref64"]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("seed", PINNED)
def test_end_to_end_against_finite_differences(G, seed, order):
    """L = sum_p splat_reference.loss_pixels(ref, project64(theta), F, G, gT), the support frozen, differenced in the eleven
    parameters of eight reached gaussians, against vjp64 of the closed form's rows."""
    c = _inputs(G, seed, order)
    cam = c["cam"]
    ref = _reference_at_project64(c)
    F, Gz, gTz = _splat_inputs(dict(c, ref=ref), seed)
    cf = sr.closed_form(ref, F, Gz, gTz)
    at = sr.fd_rows(ref, cf["reached"][ref["kept"]])
    assert bool(len(at)) == bool(fm.PINS[seed]["reached"])
    if not len(at):
        return
    rows = cf["g"][ref["kept"]]  # draw order, as c["drawn"]
    v = pr.vjp64(c["drawn"], cam, rows)
    base = sr.params_of(ref)
    fds = []
    for i in at:
        # only the pixels gaussian i is kept in can change (the support is frozen): their bounding rectangle, means shifted to it
        ys, xs = np.nonzero(ref["alpha"][..., i] > 0)
        y0, y1, x0, x1 = ys.min(), ys.max() + 1, xs.min(), xs.max() + 1
        sub = dict(alpha=ref["alpha"][y0:y1, x0:x1], kept=ref["kept"], W=x1 - x0, H=y1 - y0)
        Gs, gTs, shift = Gz[y0:y1, x0:x1], gTz[y0:y1, x0:x1], np.array([x0, y0], np.float64)

        def value_of(t):
            o = pr.project64(t, cam)
            p = [base[0] - shift, base[1].copy(), base[2].copy()]
            p[0][i], p[1][i], p[2][i] = o["screen_means"].numpy()[0] - shift, o["sigmas"].numpy()[0], o["opacity"].numpy()[0]
            return sr.loss_pixels(sub, tuple(p), F, Gs, gTs)

        fds.append(_fd(value_of, pr.rows_of(c["drawn"], [i])))
    # every pin by the plain rule but the one-gaussian pin 297: there |fd - g| is 3 .. 7e-10 on all three log-scale entries, whatever
    # their size (1e-5 .. 1.6e-4): the floor of differencing 256 pixel losses of size ~25 at h = 3e-6 in float64, against a column
    # "maximum" of 1.1e-5
    _fd_against(f"end to end seed={seed} {order}", fds, v, at, own_rounding=seed == 297)
