"""What the tests of the projection backward and of the SH colour backward share: the pinned fuzz case under a camera — its own,
or one of fuzz_maps.CAMERAS applied to it — and the bodies of the checks, on the float64 references (CPU) and on the kernels (GPU).
A plain module next to the tests, like gpu_cases.py: test_projection_reference.py, test_sh_reference.py,
test_gpu_project_backward.py and test_gpu_sh_backward.py run these checks under each pin's own camera, test_camera_variants.py and
test_gpu_camera_variants.py under the rolled, oblique, anamorphic ones.  One body each, so a variant is held to exactly the rule and
the tolerance the pinned camera is.

Every function takes the `G` of gpu_cases.modules() / namespace() and caches in G.cases under a key that starts with its own tag.
Nothing in the first two sections touches the GPU or names the GPU library.
"""
import numpy as np
import torch

from gpu_cases import _tool, fuzz_case

fm = _tool("fuzz_maps")
sr = _tool("splat_reference")
pr = _tool("projection_reference")
shr = _tool("sh_reference")
PINS = list(fm.PINS)
PINNED = [s for s in fm.PINS if s not in fm.IDENTITIES_ONLY]
ORDERS = ["file", "morton"]
DEGREES = [0, 1, 2, 3]
E2E_CH = 3  # channels of the end-to-end loss: the chain does not depend on them
FIVE = ("means", "log_scales", "quats", "opacity_logit", "sh")


def variant_args(c, camera=None):
    """The case's camera arguments: its own, or the variant `camera` of fuzz_maps.CAMERAS applied to them."""
    return c["args"] if camera is None else fm.camera_variant(c["args"], *fm.CAMERAS[camera])


def _tag(seed, order, camera):
    return f"seed={seed} {order}" + ("" if camera is None else f" camera={camera}")


# ---- the projection's float64 reference (CPU) ----------------------------------------------------------------------------------------
def projection_inputs(G, seed, order, camera=None):
    """The pin's reference, the oracle's camera, theta in the scene's order and its drawn gaussians `k` (draw order) with their
    seeded unit-normal rows; built once and only read."""
    key = ("projection", seed, order, camera)
    if key not in G.cases:
        c = fuzz_case(seed, fm.MAX_N)
        args = variant_args(c, camera)
        perm = G.renderer.morton_order(c["packed"]["means"]) if order == "morton" else None
        ref = fm.build_reference(G.orc, c["packed"], args, perm)
        theta, k = pr.theta_of(c["packed"], perm), ref["kept_in"]
        assert camera is not None or len(k) == fm.PINS[seed]["drawn"]
        G.cases[key] = dict(c=c, ref=ref, cam=G.orc.camera(*args), theta=theta, k=k, drawn=pr.rows_of(theta, k),
                            rows=pr.unit_rows(seed, len(k), np.arange(len(k))), tag=_tag(seed, order, camera))
    return G.cases[key]


def check_project64_against_the_oracle(c):
    """|diff| <= 1e-5 max(|value|, the column's largest |value|) on opacity, screen means and conics."""
    if not len(c["k"]):
        return
    fw, pre, worst = pr.project64(c["drawn"], c["cam"]), c["ref"]["pre"], 0.0
    assert bool(pr.contributes(fw).all())  # what the oracle draws, the backward carries
    for name in ("opacity", "screen_means", "sigmas"):
        got = fw[name].numpy().reshape(len(c["k"]), -1)
        want = pre[name][c["k"]].astype(np.float64).reshape(len(c["k"]), -1)
        lim = np.maximum(np.abs(want), np.abs(want).max(0, keepdims=True))
        worst = max(worst, float((np.abs(got - want) / lim).max()))
        assert (np.abs(got - want) <= pr.ORACLE_REL * lim).all(), (c["tag"], name)
    print(f"\nproject oracle {c['tag']}: worst |diff| / max(|value|, column max) {worst:.2e}", end="")


def check_vjp64_against_autograd_and_the_fused_form(c):
    """Autograd of the monolithic project64: |diff| <= 1e-10 |value| per element.  The kernel's fused arrangement in float64 (a check
    of this project's own, beyond the autograd one): |diff| <= 1e-10 B, the magnitude its differently ordered sums work at."""
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
    print(f"\nproject autograd {c['tag']}: worst |diff| / (1e-10 |value|) autograd {max(fa.values()):.2e}; "
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


def check_vjp64_against_finite_differences(c):
    """Eight drawn gaussians per pin, all eleven parameters, of L = <rows, (opacity, screen mean, conic)>."""
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
    _fd_against(c["tag"], fds, v, at)


def check_fp32_emulation_within_the_bound(c):
    """|emulation - vjp64| <= 1e-5 B per element, from the scene's float32 arrays."""
    if not len(c["k"]):
        return None
    v, B = pr.vjp64(c["drawn"], c["cam"], c["rows"]), pr.bound64(c["drawn"], c["cam"], c["rows"])
    return pr.check_geometry(f"emulation {c['tag']}", pr.emulate_fp32(c["drawn"], c["cam"], c["rows"]), v, B)


def splat_inputs(c, seed):
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


def check_end_to_end_against_finite_differences(c, seed, own_rounding=False):
    """L = sum_p splat_reference.loss_pixels(ref, project64(theta), F, G, gT), the support frozen, differenced in the eleven
    parameters of eight reached gaussians, against vjp64 of the closed form's rows.  -> how many rows were differenced."""
    cam = c["cam"]
    ref = _reference_at_project64(c)
    F, Gz, gTz = splat_inputs(dict(c, ref=ref), seed)
    cf = sr.closed_form(ref, F, Gz, gTz)
    at = sr.fd_rows(ref, cf["reached"][ref["kept"]])
    if not len(at):
        return 0
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
    _fd_against(f"end to end {c['tag']}", fds, v, at, own_rounding=own_rounding)
    return len(at)


# ---- the SH colour backward's float64 reference (CPU) ----------------------------------------------------------------------------------
def sh_inputs(G, seed, order, camera=None):
    """The pin's arrays in the scene's order, the oracle's camera and the seeded unit-normal rows; built once and only read."""
    key = ("sh", seed, order, camera)
    if key not in G.cases:
        c = fuzz_case(seed, fm.MAX_N)
        perm = G.renderer.morton_order(c["packed"]["means"]) if order == "morton" else None
        packed = c["packed"] if perm is None else {k: np.ascontiguousarray(v[perm]) for k, v in c["packed"].items()}
        G.cases[key] = dict(c=c, packed=packed, cam=G.orc.camera(*variant_args(c, camera)), theta=shr.theta_of(c["packed"], perm),
                            g=shr.unit_rows(seed, c["n"]), n=c["n"], tag=_tag(seed, order, camera))
    return G.cases[key]


def check_sh_vjp64_against_autograd(c):
    """Autograd of the monolithic statement: |diff| <= 1e-10 |value| per element; B covers |value|; nothing beyond the degree."""
    worst = 0.0
    for degree in DEGREES:
        v, B = shr.vjp64(c["theta"], c["cam"], degree, c["g"]), shr.bound64(c["theta"], c["cam"], degree, c["g"])
        p = torch.tensor(c["theta"]["means"], dtype=torch.float64, requires_grad=True)
        sh = torch.tensor(c["theta"]["sh"], dtype=torch.float64, requires_grad=True)
        rgb = shr.sh_to_rgb_torch(p, sh, torch.tensor(shr.centre_of(c["cam"])), degree)
        (rgb * torch.tensor(c["g"], dtype=torch.float64)).sum().backward()
        auto = dict(sh=sh.grad.numpy(), means=p.grad.numpy() if degree > 0 else np.zeros((c["n"], 3)))
        fa = shr.worst_ratios(auto, v, {k: np.abs(v[k]) for k in shr.FIELDS}, rel=shr.AUTOGRAD_REL)
        worst = max(worst, max(fa.values()))
        assert max(fa.values()) <= 1.0, (c["tag"], degree, fa)
        for k in shr.FIELDS:
            assert (B[k] >= np.abs(v[k]) * (1 - 1e-12)).all()
        assert np.any(v["sh"]) and bool(np.any(v["means"])) == (degree > 0)
        assert not v["sh"][:, shr.coefficients(degree):].any()
    print(f"\nsh autograd {c['tag']}: worst |diff| / (1e-10 scale) {worst:.2e}", end="")


def check_sh_fp32_emulation_within_the_bound(c):
    """|emulation - vjp64| <= 1e-5 B per element outside the band, from the scene's float32 arrays; at most CAP_LEFT_OUT entries
    left out per pin and degree; on a pin with n >= 64 a clamped and an unclamped channel are both compared."""
    worst = 0.0
    for degree in DEGREES:
        v, B = shr.vjp64(c["theta"], c["cam"], degree, c["g"]), shr.bound64(c["theta"], c["cam"], degree, c["g"])
        keep_sh, keep_means, left_out = shr.keep_mask(c["theta"], c["cam"], degree)
        assert left_out <= shr.CAP_LEFT_OUT, (c["tag"], degree, left_out)
        emu = shr.emulate_fp32(c["theta"], c["cam"], degree, c["g"])
        fig = shr.check_colour(f"emulation {c['tag']} degree={degree}", emu, v, B, dict(sh=keep_sh, means=keep_means))
        worst = max(worst, max(fig.values())) if fig else worst
        fw = shr.sh64(c["theta"], c["cam"], degree)
        compared = keep_sh[:, 0, :]
        if c["n"] >= 64:
            assert (compared & fw["m"]).any() and (compared & ~fw["m"]).any(), (c["tag"], degree)
        # the float32 decision is the float64 one outside the band
        m32 = (emu["v"] >= 0) & (emu["v"] <= 1)
        assert np.array_equal(m32[compared], fw["m"][compared])
    return worst


# ---- the kernels (GPU) -------------------------------------------------------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _small(c):
    return ((c["W"] <= 160 and c["H"] <= 96) or (c["W"] <= 33 and c["H"] <= 360)) and c["n"] <= 4096  # small frames: quick cases


def project_case(G, seed, order, camera=None):
    """The pinned case as a scene in `order` with its Rasterizer, cameras and reference, theta in the scene's order and in the
    file's, the features and the upstream gradients; built once and only read."""
    key = ("project", seed, order, camera)
    if key not in G.cases:
        c = fuzz_case(seed, fm.MAX_N)
        args = variant_args(c, camera)
        scene = G.renderer.GaussianScene.from_packed(c["packed"], spatial_order=order == "morton")
        assert (scene.order is None) == (order == "file")
        assert _small(c)
        ref = fm.build_reference(G.orc, c["packed"], args, scene.order)
        G.cases[key] = dict(seed=seed, c=c, args=args, scene=scene, R=G.renderer.Rasterizer(scene), cam=G.renderer.make_camera(*args),
                            ocam=G.orc.camera(*args), ref=ref, n=c["n"], theta=pr.theta_of(c["packed"], scene.order),
                            theta_file=pr.theta_of(c["packed"]), F=fm.features_of(seed, c["n"]),
                            Gm=fm.upstream_of(seed, c["H"], c["W"])[0], gT=sr.gT_of(seed, c["H"], c["W"]),
                            tag=f"seed={seed} order={order}" + ("" if camera is None else f" camera={camera}"))
    return G.cases[key]


def project_rows(c):
    """Seeded unit-normal rows [n, 8] in the scene's order, nonzero on the gaussians the oracle's loop draws."""
    return pr.unit_rows(c["seed"], c["n"], c["ref"]["kept_in"])


def check_project_operator_parity(G, c):
    """project_backward on unit-normal rows against vjp64: |err| <= 1e-5 B per element; the file-order result is the scene-order
    one through scene.order_t."""
    rows = project_rows(c)
    got = G.renderer.project_backward(c["scene"], c["cam"], dev(rows), scene_order=True)
    want, B = pr.vjp64(c["theta"], c["ocam"], rows), pr.bound64(c["theta"], c["ocam"], rows)
    fig = pr.check_geometry(f"{c['tag']} kind=operator", pr.as_dict(got), want, B)
    untouched = ~rows.any(1)
    for k in pr.FIELDS:
        assert not getattr(got, k)[dev(untouched)].any(), k
        assert bool(getattr(got, k).any()) == bool(len(c["ref"]["kept_in"])), k
    filed = G.renderer.project_backward(c["scene"], c["cam"], dev(rows))
    for k in pr.FIELDS:
        a, b = getattr(filed, k), getattr(got, k)
        assert torch.equal(a if c["scene"].order_t is None else a[c["scene"].order_t], b), k
    return fig


def project_masked(c, C, ref=None):
    keep = ~sr.left_out(ref if ref is not None else c["ref"])
    return c["F"][:, :C], (c["Gm"][..., :C] * keep[..., None]).astype(np.float32), (c["gT"] * keep).astype(np.float32)


def project_expected(theta_file, ocam, ref, F, Gz, gTz):
    """(vjp64 of the closed form's rows, 1e-5's bound: bound64 of |g| + A + B_splat), file order."""
    cf = sr.closed_form(ref, F, Gz, gTz)
    return pr.vjp64(theta_file, ocam, cf["g"]), pr.bound64(theta_file, ocam, np.abs(cf["g"]) + cf["A"] + cf["B"])


def check_project_end_to_end(c):
    """geometry_gradient at C = 3 and 17, with grad_T and without, against vjp64(closed form)."""
    R, cam = c["R"], c["cam"]
    for Cw in (3, 17):
        F, Gz, gTz = project_masked(c, Cw)
        for with_T in (True, False):
            got = R.geometry_gradient(cam, dev(F), dev(Gz), dev(gTz) if with_T else None)
            want, B = project_expected(c["theta_file"], c["ocam"], c["ref"], F, Gz, gTz if with_T else None)
            pr.check_geometry(f"{c['tag']} kind=end-to-end C={Cw} gT={int(with_T)}", pr.as_dict(got), want, B)
            assert all(bool(t.any()) for t in got)


def sh_case(G, seed, order, degree=3, half=False, camera=None):
    """The pinned case as a scene in `order` at `degree` with its Rasterizer and cameras, theta in the scene's order and in the
    file's, the upstream rows; built once and only read."""
    key = ("sh", seed, order, degree, half, camera)
    if key not in G.cases:
        if ("packed", seed) not in G.cases:
            G.cases[("packed", seed)] = fuzz_case(seed, fm.MAX_N)
        c = G.cases[("packed", seed)]
        args = variant_args(c, camera)
        scene = G.renderer.GaussianScene.from_packed(c["packed"], sh_degree=degree, sh_half=half, spatial_order=order == "morton")
        assert (scene.order is None) == (order == "file")
        assert _small(c)
        G.cases[key] = dict(seed=seed, c=c, args=args, scene=scene, R=G.renderer.Rasterizer(scene), cam=G.renderer.make_camera(*args),
                            ocam=G.orc.camera(*args), n=c["n"], degree=degree,
                            theta=shr.theta_of(c["packed"], scene.order, widen_f16=half), theta_file=shr.theta_of(c["packed"]),
                            g=shr.unit_rows(seed, c["n"]), tag=f"seed={seed} order={order}" + ("" if camera is None else f" camera={camera}"))
    return G.cases[key]


def check_sh_operator_parity(G, seed, order, camera=None):
    """sh_backward on unit-normal rows on EVERY gaussian against vjp64 at every degree: |err| <= 1e-5 B per element outside the
    band; the file-order result is the scene-order one through scene.order_t."""
    worst = 0.0
    for degree in DEGREES:
        c = sh_case(G, seed, order, degree, camera=camera)
        got = G.renderer.sh_backward(c["scene"], c["cam"], dev(c["g"]), scene_order=True)
        want, B = shr.vjp64(c["theta"], c["ocam"], degree, c["g"]), shr.bound64(c["theta"], c["ocam"], degree, c["g"])
        keep_sh, keep_means, left_out = shr.keep_mask(c["theta"], c["ocam"], degree)
        assert left_out <= shr.CAP_LEFT_OUT
        fig = shr.check_colour(f"{c['tag']} degree={degree} kind=operator", shr.as_dict(got), want, B, dict(sh=keep_sh, means=keep_means))
        worst = max(worst, max(fig.values()))
        assert bool(got.sh.any()) and bool(got.means.any()) == (degree > 0)
        assert not got.sh[:, shr.coefficients(degree):].any()
    filed = G.renderer.sh_backward(c["scene"], c["cam"], dev(c["g"]))
    for a, b in zip(filed, got):
        assert torch.equal(a if c["scene"].order_t is None else a[c["scene"].order_t], b)
    return worst


def sh_filled(n, seed=1):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=gen).cuda() for s in ((n, 16, 3), (n, 3))]


def sh_into(G, c, g, bufs):
    return G.renderer.sh_backward(c["scene"], c["cam"], g if isinstance(g, torch.Tensor) else dev(g), out=G.renderer.ColourGradient(*bufs))


def check_the_dense_and_the_per_lane_path_give_the_same_bits(G, c):
    """Every row touched: each full wave takes the LDS path.  The same rows in four calls, each keeping the lanes of one residue
    mod 4 and zeroing the rest: every wave then has 16 touched lanes, below the dense threshold, and takes the per-lane path.  Row
    for row the same bits, into a prefilled out."""
    n = c["n"]
    g = c["g"].copy()
    g[~g.any(1)] = 1.0
    fill = sh_filled(n, seed=2)
    dense = [f.clone() for f in fill]
    sh_into(G, c, g, dense)
    sparse = [f.clone() for f in fill]
    for part in range(4):
        sh_into(G, c, np.where((np.arange(n) % 4 == part)[:, None], g, 0.0).astype(np.float32), sparse)
    assert all(torch.equal(a, b) for a, b in zip(dense, sparse))
    assert not torch.equal(dense[0], fill[0])


def sh_e2e_case(G, seed, order="morton", camera=None):
    key = ("sh e2e", seed, order, camera)
    if key not in G.cases:
        c = sh_case(G, seed, order, camera=camera)
        cc = c["c"]
        ref = fm.build_reference(G.orc, cc["packed"], c["args"], c["scene"].order)
        G.cases[key] = dict(c, ref=ref, geo_file=pr.theta_of(cc["packed"]), geo=pr.theta_of(cc["packed"], c["scene"].order),
                            Gm=fm.upstream_of(seed, cc["H"], cc["W"])[0][..., :3], gT=sr.gT_of(seed, cc["H"], cc["W"]))
    return G.cases[key]


def sh_masked(c, ref=None):
    keep = ~sr.left_out(ref if ref is not None else c["ref"])
    return (c["Gm"] * keep[..., None]).astype(np.float32), (c["gT"] * keep).astype(np.float32)


def sh_expected(geo, theta, ocam, ref, Gz, gTz):
    """(the float64 chain, 1e-5's bound, what to compare) in the order of `geo` / `theta` and ref["kept"]: the float64 colours as
    features; the closed form's rows through the projection; sum_p w G through the SH transpose, summed into means."""
    n = ref["n"]
    fw = shr.sh64(theta, ocam, 3)
    cf = sr.closed_form(ref, fw["rgb"], Gz, gTz)
    want, B = pr.vjp64(geo, ocam, cf["g"]), pr.bound64(geo, ocam, np.abs(cf["g"]) + cf["A"] + cf["B"])
    g_rgb = fm.gradient(ref, Gz, n)
    own = fm.gradient(dict(ref, w=np.abs(ref["w"])), np.abs(Gz), n)  # sum_p w |G|: the feature gradient's own allowance
    s_want, s_B = shr.vjp64(theta, ocam, 3, g_rgb), shr.bound64(theta, ocam, 3, np.abs(g_rgb) + own)
    want, B = dict(want), dict(B)
    want["means"], B["means"] = want["means"] + s_want["means"], B["means"] + s_B["means"]
    want["sh"], B["sh"] = s_want["sh"], s_B["sh"]
    keep_sh, keep_means, left_out = shr.keep_mask(theta, ocam, 3)
    assert left_out <= shr.CAP_LEFT_OUT
    keep = {k: np.ones(want[k].shape, bool) for k in FIVE}
    keep["sh"], keep["means"] = keep_sh, keep_means
    return want, B, keep


def check_five(tag, got, want, B, keep):
    fig = {}
    for k in FIVE:
        err = np.abs(getattr(got, k).detach().cpu().numpy().astype(np.float64) - want[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where((err == 0) | ~keep[k], 0.0, err / (shr.REL * B[k]))
        fig[k] = float(r.max(initial=0.0))
    print(f"\nsh {tag}: worst |err| / (1e-05 B) " + " ".join(f"{k}={v:.3g}" for k, v in fig.items()), end="")
    for k, v in fig.items():
        assert v <= 1.0, f"{tag}: {k} exceeds 1e-5 B by a factor of {v:.3g}"


def check_colour_end_to_end(c):
    """colour_gradient, with grad_T and without, against the float64 chain in all five arrays."""
    Gz, gTz = sh_masked(c)
    for with_T in (True, False):
        got = c["R"].colour_gradient(c["cam"], dev(Gz), dev(gTz) if with_T else None)
        want, B, keep = sh_expected(c["geo_file"], c["theta_file"], c["ocam"], c["ref"], Gz, gTz if with_T else None)
        check_five(f"{c['tag']} kind=end-to-end gT={int(with_T)}", got, want, B, keep)
        assert all(bool(t.any()) for t in got)
