"""Deterministic scenes built on the decision boundaries of the rasterizer's exact shortcuts (tests/test_exact_shortcuts.py).

Camera at the origin looking along +z (qvec = (1,0,0,0), tvec = 0): a gaussian with a tiny z scale rotated about z projects to
cov2d ~ (f/z)^2 R diag(su^2, sv^2) R^T + 0.3 I, so the geometry can be designed in pixels. Every mean is placed by three linear
corrections against the CPU oracle's own fp32 screen mean and conic (means wanted exactly on a pixel centre or edge then walk by
ulps); the opacity, which moves no geometry, is set last from the conic read back, so that the chosen pixel lands where it should
(alpha = 1/255 (1 + delta), delta spread over +-1e-7 .. 1e-3).

Populations (POPS): one small gaussian per 16x16 tile, so that no margin pixel hides behind a saturated one, plus needles (behind
everything), three 64-gaussian clusters at the cull plane and gaussians just outside the frame.
  ring    a pixel centre on the alpha = 1/255 contour at the contour's x or y extreme (what the footprint AABB hx, hy must hold)
  qedge   the mean just outside an 8x8 quadrant / 16x16 tile / 32x32 cell (1e-5 .. 3 px), the facing-edge pixel that maximises
          the quadratic at alpha = 1/255; means exactly on a pixel centre / quadrant edge (dxn == 0) among them
  rho     qedge geometry with the conic correlation rho^2 = B^2 / 4AC around 0.99 (footprint_classify: 3.96)
  fastop  opacities around 2^-0.0146, around 0.99 and 1, the mean outside a quadrant with the edge's best around -1e-3 .. -1e-2
  best    generic opacity, best (log2 domain) around -1e-3
  nearmu  the mean 1e-6 .. 1e-3 px outside a quadrant next to a pixel centre: the computed power rounds to +-tiny there
  tiny    opacity (1/255)(1 +- eps): the footprint shrinks to the 0.05 px pad
  needle  long thin gaussians (conic condition 1e2 .. 1e7, diagonal and near axis-aligned), a pixel at the x / y extreme
  near    camera depth within 1e-5 relative of the cull plane 0.2, whole 64-gaussian blocks below, straddling, above
  edge    outside the frame beyond the lim_x / lim_y ray clamp, large isotropic scale, the reference rect one tile row / column
  last    ring pixels in the last tile row / column of the frame
"""
from __future__ import annotations

import math

import numpy as np

POPS = ("ring", "qedge", "rho", "fastop", "best", "nearmu", "tiny", "needle", "near", "edge", "last")
LOG2E = 1.0 / math.log(2.0)
CULL_Z = np.float32(0.2)


def camera_args(W, H):
    f = W / (2.0 * math.tan(math.radians(60.0) / 2.0))
    return (np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3), 2.0 * f, 2.0 * f, 2 * W, 2 * H, W, H), f


def _deltas(rng, n, lo=1e-7, hi=1e-3):
    """delta spread logarithmically over +-[lo, hi], both signs."""
    return rng.choice([-1.0, 1.0], n) * np.exp(rng.uniform(math.log(lo), math.log(hi), n))


def _conic(pre):
    s = pre["sigmas"].astype(np.float64)
    return s[:, 0], s[:, 1], s[:, 2]


def power_at(mx, my, sx, sy, sxy, px, py):
    """rasterize.py:279-283 in float64."""
    dx, dy = mx - px, my - py
    return -0.5 * (sx * dx * dx + sy * dy * dy) - sxy * dx * dy


def _rho_theta(a2, b2, rho2):
    """rotation angle (radians, in (0, pi/4]) at which cov = R diag(a2, b2) R^T + 0.3 I has cov_xy^2 / (cov_xx cov_yy) = rho2."""
    lo, hi = 1e-9, math.pi / 4
    def r2(t):
        c, s = math.cos(t), math.sin(t)
        xx, yy, xy = a2 * c * c + b2 * s * s + 0.3, a2 * s * s + b2 * c * c + 0.3, (a2 - b2) * s * c
        return xy * xy / (xx * yy)
    if r2(hi) < rho2:
        return None
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if r2(mid) < rho2 else (lo, mid)
    return 0.5 * (lo + hi)


class MarginScene:
    """Columns (INRIA ply names) plus, per gaussian: population, target pixel, target edge, wanted opacity rule."""

    def __init__(self, W, H, seed):
        from oracle import cpu_oracle as orc
        from gsr_amd import utils

        self.W, self.H, self.seed = W, H, seed
        args, f = camera_args(W, H)
        self.cam_args, self.f = args, f
        rng = np.random.default_rng(seed)
        tx, ty = (W + 15) // 16, (H + 15) // 16
        g = {k: [] for k in ("pop", "z", "su", "sv", "th", "mode", "px", "py", "par", "sgn", "cx", "op_rule", "opv", "dlt")}

        def add(pop, z, su, sv, th, mode, px, py, par, sgn, cx, op_rule, opv, dlt):
            for k, v in zip(g, (pop, z, su, sv, th, mode, px, py, par, sgn, cx, op_rule, opv, dlt)):
                g[k].append(v)

        # tiles of the last row / column host `last`, three clusters of tiles host `near`, the rest the small populations
        interior = [(i, j) for j in range(ty - 1) for i in range(tx - 1)]
        rng.shuffle(interior)
        n_near = 3 * 64
        near_tiles = sorted(interior[:n_near], key=lambda t: t[0] + 1000 * t[1])
        rest = interior[n_near:]
        share = {"ring": 0.26, "qedge": 0.26, "rho": 0.10, "fastop": 0.12, "best": 0.08, "nearmu": 0.08, "tiny": 0.10}
        order, k0 = [], 0
        for p, s in share.items():
            k1 = k0 + int(round(s * len(rest)))
            order += [(p, t) for t in rest[k0:k1]]
            k0 = k1
        zs = iter(rng.permutation(np.linspace(1.5, 3.0, len(order) + 8)))

        def small_sig():
            return rng.uniform(0.7, 2.2), rng.uniform(0.7, 2.2), rng.uniform(0.1, 3.0)

        for p, (i, j) in order:
            X0, Y0 = 16 * i, 16 * j
            z = float(next(zs))
            su, sv, th = small_sig()
            if p == "ring":
                # x or y extreme, either side; tau = ln(255 op) in [0.05, 4] keeps the pixel inside the reference's 3-sigma rect
                add(p, z, su, sv, th, "ring", X0 + 8, Y0 + 8, math.exp(rng.uniform(math.log(0.05), math.log(4.0))),
                    int(rng.integers(0, 4)), 0, "thresh", 0.0, _deltas(rng, 1)[0])
            elif p in ("qedge", "rho", "fastop", "best", "nearmu"):
                # the facing edge: a quadrant edge inside the tile, or the tile's (cell's, for even i / j) own left / top edge
                vert = bool(rng.integers(0, 2))
                c = (X0 if vert else Y0) + int(rng.choice([0, 8]))
                other = (Y0 if vert else X0) + int(rng.integers(2, 14))
                if p == "qedge":
                    u = rng.random()
                    d = 0.0 if u < 0.06 else math.exp(rng.uniform(math.log(1e-5), math.log(3.0)))
                    rule = "thresh" if d > 0 else "fixed"
                    opv = 0.0 if d > 0 else rng.uniform(0.2, 0.9)
                    if u < 0.03:  # exactly on a pixel centre inside the tile, not only on the edge
                        c += 3
                    add(p, z, su, sv, th, "edge_v" if vert else "edge_h", c if vert else other, other if vert else c, d, 0, 0, rule, opv,
                        _deltas(rng, 1)[0])
                elif p == "rho":
                    rho2 = 0.99 + _deltas(rng, 1, 1e-6, 3e-3)[0]
                    a2, b2 = rng.uniform(20.0, 28.0) ** 2, rng.uniform(0.1, 0.3) ** 2   # (the + 0.3 px^2 dilation needs a long axis)
                    t = _rho_theta(a2, b2, rho2)
                    su, sv, th = math.sqrt(a2), math.sqrt(b2), (t or math.pi / 4) * rng.choice([-1.0, 1.0])
                    d = math.exp(rng.uniform(math.log(0.02), math.log(2.0)))
                    add(p, z, su, sv, th, "edge_v" if vert else "edge_h", c if vert else other, other if vert else c, d, 0, 0, "thresh",
                        0.0, _deltas(rng, 1)[0])
                elif p in ("fastop", "best"):
                    # d set from the conic so that the edge's maximum (log2 domain) is `best`
                    best = -1e-3 * (1.0 + _deltas(rng, 1, 1e-4, 0.5)[0]) if rng.random() < 0.7 else -math.exp(rng.uniform(math.log(1e-4), math.log(3e-2)))
                    if p == "fastop":
                        kind = rng.choice(4, p=[0.3, 0.3, 0.1, 0.3])
                        opv = (2.0 ** -0.0146 * (1 + _deltas(rng, 1, 1e-7, 1e-4)[0]) if kind == 0 else
                               0.99 * (1 + _deltas(rng, 1, 1e-7, 1e-3)[0]) if kind == 1 else 1.0 if kind == 2 else rng.uniform(0.992, 0.9995))
                    else:
                        opv = rng.uniform(0.05, 0.98)
                    add(p, z, su, sv, th, "edge_v" if vert else "edge_h", c if vert else other, other if vert else c, -best, 0, 0, "fixed",
                        min(opv, 1.0), 0.0)
                else:  # nearmu: strongly correlated, well conditioned, the mean a hair outside the edge next to a pixel centre
                    rho2 = rng.uniform(0.5, 0.9)
                    a2, b2 = rng.uniform(2.0, 4.0) ** 2, rng.uniform(0.3, 0.8) ** 2
                    t = _rho_theta(a2, b2, rho2) or math.pi / 4
                    d = math.exp(rng.uniform(math.log(1e-6), math.log(1e-3)))
                    add(p, z, math.sqrt(a2), math.sqrt(b2), t * rng.choice([-1.0, 1.0]), "near_v" if vert else "near_h",
                        c if vert else other, other if vert else c, d, int(rng.integers(0, 2)), 0, "fixed", rng.uniform(0.05, 0.98), 0.0)
            else:  # tiny: the mean at (or next to) a pixel centre
                d = 0.0 if rng.random() < 0.2 else math.exp(rng.uniform(math.log(1e-4), math.log(0.08)))
                add(p, z, su, sv, th, "tiny", X0 + 8, Y0 + 8, d, 0, 0, "tiny", 0.0, _deltas(rng, 1)[0])

        # last tile row and column (frames that are not multiples of 16: partial tiles); ring pixels at most W-2 / H-2 (Q1)
        for i in range(tx):
            py = min(16 * (ty - 1) + 4, H - 3)
            add("last", float(next(zs, 2.9)) + 0.001 * i, *small_sig(), "ring", min(16 * i + 8, W - 3), py,
                math.exp(rng.uniform(math.log(0.05), math.log(4.0))), int(rng.integers(0, 4)), 0, "thresh", 0.0, _deltas(rng, 1)[0])
        for j in range(ty - 1):
            add("last", 2.95 + 0.001 * j, *small_sig(), "ring", min(16 * (tx - 1) + 4, W - 3), 16 * j + 8,
                math.exp(rng.uniform(math.log(0.05), math.log(4.0))), int(rng.integers(0, 4)), 0, "thresh", 0.0, _deltas(rng, 1)[0])

        # the cull plane: three clusters of 64 (all below, straddling, all above), camera depth 0.2 (1 +- 1e-7 .. 1e-5)
        for k, (i, j) in enumerate(near_tiles):
            r = math.exp(rng.uniform(math.log(1e-7), math.log(1e-5)))
            side = -1.0 if k < 64 else 1.0 if k >= 128 else (-1.0 if k % 2 else 1.0)
            z = float(np.float32(0.2 * (1.0 + side * r)))
            if k % 7 == 0:   # the float32 neighbours of 0.2f themselves
                z = float(np.nextafter(CULL_Z, np.float32(-1 if side < 0 else 1)))
            su, sv, th = small_sig()
            add("near", z, su, sv, th, "centre", 16 * i + 8, 16 * j + 8, 0.3, 0, 0, "fixed", rng.uniform(0.3, 0.9), 0.0)

        # needles, behind everything: condition 1e2 .. 1e7, diagonal or near axis-aligned (sxy != 0, Q2); a pixel at the extreme
        for k in range(30):
            lo, hi = ((2e6, 1e7), (4e4, 2e6), (1e2, 4e4), (1e2, 1e4))[min(k // 8, 3)]
            kappa = math.exp(rng.uniform(math.log(lo), math.log(hi)))
            b = rng.uniform(0.0, 1.0)
            lam2 = b * b + 0.3
            a = math.sqrt(kappa * lam2)
            th = (math.pi / 4 + rng.uniform(-0.05, 0.05)) if k < 24 else rng.uniform(1e-3, 1e-2)
            th *= rng.choice([-1.0, 1.0])
            px, py = int(rng.integers(W // 4, 3 * W // 4)), int(rng.integers(H // 4, 3 * H // 4))
            add("needle", 4.0 + 0.01 * k, a, b, th, "needle", px, py, rng.uniform(30.0, 250.0), int(rng.integers(0, 4)), 0, "thresh",
                0.0, _deltas(rng, 1)[0])

        # just outside the frame, past the ray clamp (|x/z| > lim), large isotropic scale: the reference rect reaches one tile row
        # or column of the frame and the true radius comes close to the shard / block bounds (Rb)
        for k in range(32):
            sig = rng.uniform(12.0, 40.0)
            spread = math.ceil(3.0 * math.sqrt(sig * sig + 0.3))
            side = k % 4
            off = rng.uniform(-spread + 1.0, -spread + 15.0)   # mean + spread + 15 in [16, 30]: one tile row / column
            if side == 0:
                mx, my = rng.uniform(0, W), off
            elif side == 1:
                mx, my = rng.uniform(0, W), H - 1 - off
            elif side == 2:
                mx, my = off, rng.uniform(0, H)
            else:
                mx, my = W - 1 - off, rng.uniform(0, H)
            add("edge", 3.5 + 0.01 * k, sig, sig, 0.3, "free", mx, my, 0.0, 0, 0, "fixed", rng.uniform(0.7, 0.95), 0.0)
        # and far outside, beyond the clamp of the EWA Jacobian (lim = 1.3 tan(fov / 2)) with radii up to the frame's size
        for k in range(16):
            sig = rng.uniform(0.2, 0.5) * W
            side = k % 4
            far = rng.uniform(0.2, 0.45) * W
            mx = -far if side == 0 else W - 1 + far if side == 1 else rng.uniform(0, W)
            my = -far if side == 2 else H - 1 + far if side == 3 else rng.uniform(0, H)
            add("edge", 3.8 + 0.01 * k, sig, sig * rng.uniform(0.7, 1.0), rng.uniform(0.1, 1.4), "free", mx, my, 0.0, 0, 0, "fixed",
                rng.uniform(0.5, 0.95), 0.0)

        # 192 small gaussians off the frame's top-left corner (means 12 .. 80 px out in x and y), behind the rest: extreme in every
        # coordinate, they fill whole Morton blocks that block culling can skip, near its screen bound
        for k in range(192):
            sig = rng.uniform(1.0, 2.5)
            add("edge", 6.0 + 0.001 * k, sig, sig * rng.uniform(0.7, 1.0), rng.uniform(0.1, 1.4), "free", -rng.uniform(12.0, 80.0),
                -rng.uniform(12.0, 80.0), 0.0, 0, 0, "fixed", rng.uniform(0.7, 0.95), 0.0)

        # every camera depth distinct: gaussians at EXACTLY equal depth blend in scene-index order (renderer.GaussianScene), which
        # differs between file and Morton order; the near-plane population moves away from the plane, everything else up
        z32 = np.asarray(g["z"], np.float32)
        seen = set()
        for i in range(len(z32)):
            up = not (g["pop"][i] == "near" and z32[i] < CULL_Z)
            while float(z32[i]) in seen:
                z32[i] = np.nextafter(z32[i], np.float32(np.inf if up else -np.inf))
            seen.add(float(z32[i]))
        g["z"] = [float(v) for v in z32]
        self.meta = {k: np.asarray(v) for k, v in g.items()}
        self.meta["W"], self.meta["H"] = W, H
        m = self.meta
        n = len(m["pop"])
        self.n = n
        z = m["z"].astype(np.float64)
        # world scales: su, sv in pixels at depth z; the z scale is tiny
        su_w, sv_w = m["su"] * z / f, m["sv"] * z / f
        cols = {}
        for c in range(3):
            cols[f"f_dc_{c}"] = rng.uniform(0.2, 1.2, n).astype(np.float32)   # colour 0.28 dc + 0.5 in [0.55, 0.84]: every channel counts
        for c in range(45):
            cols[f"f_rest_{c}"] = np.zeros(n, np.float32)
        cols["scale_0"] = np.log(su_w).astype(np.float32)
        cols["scale_1"] = np.log(sv_w).astype(np.float32)
        cols["scale_2"] = np.log(1e-4 * np.minimum(su_w, sv_w)).astype(np.float32)
        half = 0.5 * m["th"]
        cols["rot_0"] = np.cos(half).astype(np.float32)
        cols["rot_1"] = np.zeros(n, np.float32)
        cols["rot_2"] = np.zeros(n, np.float32)
        cols["rot_3"] = np.sin(half).astype(np.float32)
        cols["z"] = z.astype(np.float32)
        cols["opacity"] = np.full(n, 2.0, np.float32)
        self.cols = cols
        tgt = np.stack([m["px"], m["py"]], 1).astype(np.float64)   # first guess: the pixel
        self._place(tgt, f, z, W, H)
        cam = orc.camera(*args)
        for _ in range(3):
            pre = orc.preprocess(utils.pack_gaussians(cols), cam)
            tgt = self._targets(pre)
            self._place(tgt, f, z, W, H, pre["screen_means"].astype(np.float64))
        pre = orc.preprocess(utils.pack_gaussians(cols), cam)
        self._snap(pre, orc, utils, cam)
        pre = orc.preprocess(utils.pack_gaussians(cols), cam)
        self.target = self._targets(pre)
        cols["opacity"] = self._logits(pre)
        self.pre = orc.preprocess(utils.pack_gaussians(cols), cam)
        self.cam = cam

    def _place(self, tgt, f, z, W, H, cur=None):
        c = self.cols
        if cur is None:
            c["x"] = ((tgt[:, 0] + 0.5 - 0.5 * W) * z / f).astype(np.float32)
            c["y"] = ((tgt[:, 1] + 0.5 - 0.5 * H) * z / f).astype(np.float32)
        else:
            c["x"] = (c["x"].astype(np.float64) + (tgt[:, 0] - cur[:, 0]) * z / f).astype(np.float32)
            c["y"] = (c["y"].astype(np.float64) + (tgt[:, 1] - cur[:, 1]) * z / f).astype(np.float32)

    def _snap(self, pre, orc, utils, cam):
        """means wanted EXACTLY on a pixel centre or an edge (qedge with d == 0, tiny with d == 0): walk x, y by ulps."""
        m = self.meta
        want = ((m["pop"] == "qedge") | (m["pop"] == "tiny")) & (m["par"] == 0.0)
        idx = np.nonzero(want)[0]
        tgt = self._targets(pre)
        for axis, key in ((0, "x"), (1, "y")):
            best = np.abs(pre["screen_means"][idx, axis].astype(np.float64) - tgt[idx, axis])
            base = self.cols[key][idx].copy()
            chosen = base.copy()
            for k in range(-6, 7):
                trial = base.copy()
                for _ in range(abs(k)):
                    trial = np.nextafter(trial, np.float32(np.sign(k) * np.inf)).astype(np.float32)
                self.cols[key][idx] = trial
                sm = orc.preprocess(utils.pack_gaussians({kk: v[idx] for kk, v in self.cols.items()}), cam)["screen_means"][:, axis]
                err = np.abs(sm.astype(np.float64) - tgt[idx, axis])
                better = err < best
                chosen[better], best[better] = trial[better], err[better]
            self.cols[key][idx] = chosen

    def _targets(self, pre):
        """the wanted screen mean of every gaussian from its current conic."""
        m = self.meta
        sx, sy, sxy = _conic(pre)
        D = sx * sy - sxy * sxy
        px, py, par = m["px"].astype(np.float64), m["py"].astype(np.float64), m["par"].astype(np.float64)
        tx, ty = px.copy(), py.copy()
        mode = m["mode"]
        with np.errstate(all="ignore"):
            # ring / needle: the pixel at the contour's extreme; tau = par (ring) or the extent in px (needle)
            ring = (mode == "ring") | (mode == "needle")
            tau = np.where(mode == "needle", 0.0, par)
            # needle: tau from the wanted extent along the axis of the extreme, capped so that op <= 1
            ext_x, ext_y = par * par * D / (2.0 * sy), par * par * D / (2.0 * sx)
            xs = (m["sgn"] % 2) == 0
            tau = np.where(mode == "needle", np.minimum(np.where(xs, ext_x, ext_y), 5.0), tau)
            sg = np.where(m["sgn"] < 2, 1.0, -1.0)
            dxr = sg * np.sqrt(2 * tau * sy / D)
            dyr = sg * np.sqrt(2 * tau * sx / D)
            rx = np.where(xs, dxr, -sxy * dyr / sx)
            ry = np.where(xs, -sxy * dxr / sy, dyr)
            tx = np.where(ring, px + rx, tx)
            ty = np.where(ring, py + ry, ty)
            # edges: the mean d px before the edge column / row, the pixel on the edge at the maximiser of the quadratic
            ev, eh = (mode == "edge_v") | (mode == "near_v"), (mode == "edge_h") | (mode == "near_h")
            d = par.copy()
            fixed_best = np.isin(m["pop"], ("fastop", "best"))
            # best = -0.5 log2e d^2 D / sy (vertical edge)  ->  d
            d = np.where(fixed_best & ev, np.sqrt(2.0 * par / (LOG2E * D / sy)), d)
            d = np.where(fixed_best & eh, np.sqrt(2.0 * par / (LOG2E * D / sx)), d)
            # qedge / rho on the threshold: keep tau = 0.5 d^2 D / s below 5 (op <= 1)
            thr = m["op_rule"] == "thresh"
            d = np.where(thr & ev, np.minimum(d, np.sqrt(10.0 * sy / D)), d)
            d = np.where(thr & eh, np.minimum(d, np.sqrt(10.0 * sx / D)), d)
            dxe = -d
            tx = np.where(ev, px + dxe, tx)
            ty = np.where(ev, py - sxy * dxe / sy, ty)
            ty = np.where(eh, py + dxe, ty)
            tx = np.where(eh, px - sxy * dxe / sx, tx)
            # nearmu: the pixel itself a hair from the mean (sgn picks the offset's other component: 0 or +-d)
            o2 = np.where(m["sgn"] == 1, d, 0.0)
            tx = np.where(mode == "near_v", px - d, np.where(mode == "near_h", px + o2, tx))
            ty = np.where(mode == "near_v", py + o2, np.where(mode == "near_h", py - d, ty))
            # tiny: the mean d px from the pixel, diagonally
            tn = mode == "tiny"
            tx = np.where(tn, px + par * 0.6, tx)
            ty = np.where(tn, py + par * 0.8, ty)
            # free / centre: where asked
            fr = (mode == "free") | (mode == "centre")
            tx, ty = np.where(fr, px, tx), np.where(fr, py, ty)
        assert np.isfinite(tx).all() and np.isfinite(ty).all()
        return np.stack([tx, ty], 1)

    def _logits(self, pre):
        m = self.meta
        sx, sy, sxy = _conic(pre)
        mx, my = pre["screen_means"][:, 0].astype(np.float64), pre["screen_means"][:, 1].astype(np.float64)
        pw = power_at(mx, my, sx, sy, sxy, m["px"].astype(np.float64), m["py"].astype(np.float64))
        dl = m["dlt"].astype(np.float64)
        op = np.where(m["op_rule"] == "thresh", np.exp(-pw) / 255.0 * (1.0 + dl), m["opv"].astype(np.float64))
        op = np.where(m["op_rule"] == "tiny", (1.0 + dl) / 255.0, op)
        op = np.clip(op, 1e-6, 1.0)
        with np.errstate(divide="ignore"):
            logit = np.where(op >= 1.0, 40.0, np.log(op) - np.log1p(-op))
        return logit.astype(np.float32)

    def n_of(self, pop):
        return int((self.meta["pop"] == pop).sum())


def quad_best(mx, my, A, B, C, x0, x1, y0, y1):
    """footprint.h's `best` in float64: the maximum of A dx^2 + B dx dy + C dy^2 (log2 domain) over the rectangle of pixel
    centres [x0,x1]x[y0,y1]; 0 with the mean inside."""
    dxn = mx - np.clip(mx, x0, x1)
    dyn = my - np.clip(my, y0, y1)
    best = np.full(np.shape(mx), -np.inf)
    with np.errstate(all="ignore"):
        dy = np.clip(-B / (2 * C) * dxn, my - y1, my - y0)
        bv = dxn * (A * dxn + B * dy) + C * dy * dy
        dx = np.clip(-B / (2 * A) * dyn, mx - x1, mx - x0)
        bh = dx * (A * dx + B * dyn) + C * dyn * dyn
    best = np.where(dxn != 0, np.maximum(best, bv), best)
    best = np.where(dyn != 0, np.maximum(best, bh), best)
    return np.where((dxn == 0) & (dyn == 0), 0.0, best)


def population_counts(meta, mx, my, sx, sy, sxy, op, zc):
    """How many gaussians / (gaussian, pixel) / (gaussian, quadrant) pairs sit within a small band of each UNLOOSENED boundary, on
    either side, from the fp32 intermediates (oracle or kernel) evaluated in float64."""
    mx, my, sx, sy, sxy, op, zc = (np.asarray(a, np.float64) for a in (mx, my, sx, sy, sxy, op, zc))
    pop, mode = meta["pop"], meta["mode"]
    px, py = meta["px"].astype(np.float64), meta["py"].astype(np.float64)
    pw = power_at(mx, my, sx, sy, sxy, px, py)
    a255 = 255.0 * op * np.exp(pw) - 1.0
    with np.errstate(all="ignore"):
        D = sx * sy - sxy * sxy
        rho2 = sxy * sxy / (sx * sy)
        ex = np.abs(my - py + sxy * (mx - px) / sy)    # distance (px) of the pixel from the contour's x-extreme line
        ey = np.abs(mx - px + sxy * (my - py) / sx)
    out = {}

    def both(name, sel, v, band):
        out[name + "-"] = int((sel & (v < 0) & (v > -band)).sum())
        out[name + "+"] = int((sel & (v >= 0) & (v < band)).sum())

    ringlike = np.isin(pop, ("ring", "last", "needle")) & ((ex < 1e-3) | (ey < 1e-3))
    both("ring |255a-1|<1e-4", np.isin(pop, ("ring", "last")) & ringlike, a255, 1e-4)
    both("needle |255a-1|<1e-4", (pop == "needle") & ringlike, a255, 1e-4)
    both("last-tile |255a-1|<1e-4", (pop == "last") & ringlike, a255, 1e-4)
    # qedge: the facing-edge pixel's alpha on the threshold, per offset of the mean from the edge
    ev = mode == "edge_v"
    dist = np.where(ev, px - mx, py - my)
    qe = np.isin(pop, ("qedge", "rho")) & (meta["op_rule"] == "thresh")
    both("qedge d<1e-3 |255a-1|<1e-4", qe & (dist > 0) & (dist < 1e-3), a255, 1e-4)
    both("qedge d>=1e-3 |255a-1|<1e-4", qe & (dist >= 1e-3), a255, 1e-4)
    out["qedge mean on edge (dxn == 0)"] = int(((pop == "qedge") & (dist == 0)).sum())
    out["mean on a pixel centre"] = int((np.isin(pop, ("qedge", "tiny")) & (mx == np.round(mx)) & (my == np.round(my))).sum())
    both("rho2-0.99 (|.|<1e-4)", pop == "rho", rho2 - 0.99, 1e-4)
    both("rho2-0.99 (|.|<1e-3)", pop == "rho", rho2 - 0.99, 1e-3)
    L = np.log2(op)
    both("log2(op)+0.0146 (|.|<1e-6)", pop == "fastop", L + 0.0146, 1e-6)
    both("op-0.99 (|.|<1e-6)", pop == "fastop", op - 0.99, 1e-6)
    out["op == 1"] = int(((pop == "fastop") & (op == 1.0)).sum())
    # best of the quadrant the edge faces (8x8 rect of pixel centres whose first column / row is the edge)
    A, B, C = -0.5 * sx * LOG2E, -sxy * LOG2E, -0.5 * sy * LOG2E
    x0 = np.where(ev, px, np.floor(px / 8) * 8)
    y0 = np.where(ev, np.floor(py / 8) * 8, py)
    bq = quad_best(mx, my, A, B, C, x0, x0 + 7, y0, y0 + 7)
    eb = np.isin(pop, ("fastop", "best"))
    both("best+1e-3 (|.|<1e-5)", eb, bq + 1e-3, 1e-5)
    both("best+1e-3 (|.|<1e-4)", eb, bq + 1e-3, 1e-4)
    out["fastop alpha>0.99 at best<=-1e-3, op<1"] = int((eb & (op < 1.0) & (op * np.exp2(bq) > 0.99) & (bq <= -1e-3)).sum())
    nm = pop == "nearmu"
    dnm = np.hypot(mx - px, my - py)
    out["nearmu mean outside, |pixel-mean|<1e-4"] = int((nm & (dnm < 1e-4) & (dnm > 0)).sum())
    both("tiny 255op-1 (|.|<1e-4)", pop == "tiny", 255.0 * op - 1.0, 1e-4)
    ne = pop == "needle"
    with np.errstate(all="ignore"):
        dr = D / (sx * sy)
    out["needle D/sxsy < 1e-6"] = int((ne & (dr <= 1e-6)).sum())
    out["needle D/sxsy in (1e-6, 2e-6]"] = int((ne & (dr > 1e-6) & (dr <= 2e-6)).sum())
    out["needle D/sxsy in (2e-6, 1e-4]"] = int((ne & (dr > 2e-6) & (dr <= 1e-4)).sum())
    out["needle D/sxsy > 1e-4"] = int((ne & (dr > 1e-4)).sum())
    out["needle near axis (|rho|<0.2)"] = int((ne & (rho2 < 0.04)).sum())
    both("near z/0.2-1 (|.|<1e-5)", pop == "near", zc / 0.2 - 1.0, 1e-5)
    out["edge outside the frame"] = int(((pop == "edge") & ((mx < 0) | (my < 0) | (mx > meta["W"] - 1) | (my > meta["H"] - 1))).sum()) \
        if "W" in meta else int((pop == "edge").sum())
    return out


# floors: what every scene of the module must contain (the smallest frame, 650x370, sets them)
FLOORS = {
    "ring |255a-1|<1e-4-": 30, "ring |255a-1|<1e-4+": 30,
    "needle |255a-1|<1e-4-": 4, "needle |255a-1|<1e-4+": 4,
    "last-tile |255a-1|<1e-4-": 8, "last-tile |255a-1|<1e-4+": 8,
    "qedge d<1e-3 |255a-1|<1e-4-": 4, "qedge d<1e-3 |255a-1|<1e-4+": 4,
    "qedge d>=1e-3 |255a-1|<1e-4-": 20, "qedge d>=1e-3 |255a-1|<1e-4+": 20,
    "qedge mean on edge (dxn == 0)": 2, "mean on a pixel centre": 2,
    "rho2-0.99 (|.|<1e-4)-": 2, "rho2-0.99 (|.|<1e-4)+": 2, "rho2-0.99 (|.|<1e-3)-": 10, "rho2-0.99 (|.|<1e-3)+": 10,
    "log2(op)+0.0146 (|.|<1e-6)-": 2, "log2(op)+0.0146 (|.|<1e-6)+": 2, "op-0.99 (|.|<1e-6)-": 1, "op-0.99 (|.|<1e-6)+": 1,
    "op == 1": 5, "best+1e-3 (|.|<1e-5)-": 1, "best+1e-3 (|.|<1e-5)+": 1, "best+1e-3 (|.|<1e-4)-": 8, "best+1e-3 (|.|<1e-4)+": 8,
    "fastop alpha>0.99 at best<=-1e-3, op<1": 5,
    "nearmu mean outside, |pixel-mean|<1e-4": 20,
    "tiny 255op-1 (|.|<1e-4)-": 10, "tiny 255op-1 (|.|<1e-4)+": 10,
    "needle D/sxsy < 1e-6": 1, "needle D/sxsy in (1e-6, 2e-6]": 1, "needle D/sxsy in (2e-6, 1e-4]": 3, "needle D/sxsy > 1e-4": 2,
    "needle near axis (|rho|<0.2)": 1,
    "near z/0.2-1 (|.|<1e-5)-": 60, "near z/0.2-1 (|.|<1e-5)+": 60,
    "edge outside the frame": 30,
}
