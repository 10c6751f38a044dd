"""A float64 reference of every map kind, and the checks that hold the map kernels to it on the fuzz campaign's edge shapes.

The operation (oracle/gsr_oracle.c, composite_band): per (pixel, gaussian) pair inside the gaussian's pixel bbox,
alpha = min(0.99, o * exp(power)), kept where alpha > 1/255 and power <= 0, in depth order; w = alpha * T, T <- T (1 - alpha).
`reference` evaluates that in float64 over the oracle's preprocess outputs and depth order, for every pair of a small frame at
once; the feature map, its gradient, the view statistics, the pick maps, the top-k lists and the slab maps are plain functions
of its alpha / w / T arrays.  Nothing in the first half of this file needs a GPU or torch (numpy only, and the oracle through the
`orc` module a caller hands in); the `run_*` functions of the second half take a Rasterizer, render a kind and check it, and
are what tests/test_gpu_fuzz_maps.py and `tools/fuzz_parity.py --maps` both call.  Needs nothing from tests/.

What a comparison leaves out, and why:
  - a pixel that holds a pair with |255 alpha - 1| <= BAND: there fp32 may legitimately decide `alpha > 1/255` the other way, which
    also moves every later weight of the pixel (each by at most STEP, which is still asserted);
  - pairs with 0 < w < TINY in positivity checks (count, pixels, ids of -1): fp32 T has underflowed there;
  - ids where two candidates are closer than ID_MARGIN in weight (or a T closer than that to median_T).
The shares left out are capped (CAP_*); tests/test_fuzz_maps_reference.py asserts the caps on the reference alone.
"""
import numpy as np

MIN_ALPHA = float(np.float32(1.0 / 255.0))
MAX_ALPHA = float(np.float32(0.99))
BAND = 1e-3          # |255 alpha - 1| at or below this: the pixel is left out of the comparisons
STEP = 4.5e-3        # one threshold step (tests/conftest.py): the most a flipped pair moves a weight or T
TINY = 1e-30         # float64 weights below this take no part in positivity checks
W_TOL = 1e-4         # weights, T, weight_max
ID_MARGIN = 2e-4     # ids are compared where the runner-up is further away than this
MIN_DB = 100.0
CAP_PIXELS, CAP_TINY, CAP_BEST, CAP_MEDIAN, CAP_SLOTS = 0.03, 0.02, 0.02, 0.02, 0.06
MEDIANS = (0.5, 0.9, 1.0)
KS = (4, 8, 16)
WIDTHS = (1, 3, 17)  # channels: the three-channel blend below and at its width, a wide walk of 16 plus a narrow one
N_CH = 17
MAX_N = 5000         # build_case(seed, max_n=MAX_N)
MAX_SWEEP_N = 257    # the exact layer's prefix sweep renders n maps of n channels
IDENTITIES_ONLY = (283,)

# seed -> what build_case(seed, MAX_N) is and what it is aimed at.  drawn: gaussians the oracle's loop does not skip; reached: of
# those, the ones with w > 0 somewhere; deepest: most contributors of one pixel; ties: neighbours of equal depth in drawn order;
# reached = 0: nothing passes alpha > 1/255.  (The same in file and in Morton order; tests/test_fuzz_maps_reference.py asserts every entry.)
PINS = {
    297: dict(n=1, W=16, H=16, drawn=1, reached=1, deepest=1, ties=0, aim="one gaussian"),
    306: dict(n=1, W=17, H=15, drawn=1, reached=1, deepest=1, ties=0, aim="one gaussian, partial tiles"),
    311: dict(n=2, W=33, H=197, drawn=2, reached=2, deepest=1, ties=0, aim="two gaussians; a third tile column of one pixel"),
    269: dict(n=64, W=31, H=15, drawn=6, reached=2, deepest=1, ties=0, aim="one exact 64-block; partial tile both ways"),
    264: dict(n=65, W=31, H=16, drawn=45, reached=45, deepest=13, ties=36, aim="equal-depth stacks"),
    322: dict(n=64, W=31, H=16, drawn=41, reached=39, deepest=17, ties=36, aim="equal-depth stacks"),
    301: dict(n=65, W=16, H=16, drawn=53, reached=40, deepest=17, ties=0, aim="logit 12: every alpha at the cap"),
    277: dict(n=256, W=16, H=17, drawn=101, reached=96, deepest=19, ties=0, aim="logit 12; a tile row of one pixel"),
    290: dict(n=65, W=15, H=16, drawn=35, reached=0, deepest=0, ties=0, aim="logit -8: full lists, nothing passes"),
    324: dict(n=63, W=160, H=96, drawn=51, reached=0, deepest=0, ties=0, aim="logit -8: full lists, nothing passes"),
    263: dict(n=65, W=15, H=1, drawn=0, reached=0, deepest=0, ties=0, aim="one-row frame"),
    296: dict(n=257, W=31, H=16, drawn=170, reached=165, deepest=53, ties=0, aim="deep pixels"),
    378: dict(n=256, W=15, H=15, drawn=186, reached=171, deepest=123, ties=0, aim="deep pixels"),
    354: dict(n=257, W=15, H=15, drawn=257, reached=256, deepest=98, ties=0, aim="all drawn in one tile: one entry past a 256-entry batch"),
    351: dict(n=257, W=33, H=15, drawn=140, reached=136, deepest=128, ties=138, aim="stacks; T underflows"),
    327: dict(n=257, W=16, H=96, drawn=210, reached=204, deepest=141, ties=195, aim="stacks; T reaches 3e-35"),
    252: dict(n=256, W=33, H=360, drawn=206, reached=203, deepest=49, ties=0, aim="3x23 tiles, tall"),
    282: dict(n=257, W=15, H=197, drawn=227, reached=208, deepest=19, ties=0, aim="1x13 tiles, tall"),
    369: dict(n=4096, W=17, H=16, drawn=228, reached=162, deepest=11, ties=0, aim="64 full blocks"),
    283: dict(n=4095, W=17, H=17, drawn=3864, reached=3827, deepest=2600, ties=2, aim="~15 batches per tile: identities between kernels only"),
}


# ---- the reference (numpy, float64) -----------------------------------------------------------------------------------------------
def _compose(alpha, band, kept, z):
    T_after = np.cumprod(1.0 - alpha, axis=-1)
    T_before = np.concatenate([np.ones(alpha.shape[:2] + (1,)), T_after[..., :-1]], -1) if alpha.shape[-1] else T_after
    return dict(alpha=alpha, w=alpha * T_before, T_after=T_after, kept=kept, band=band, z=z)


def reference(pre, order, W, H):
    """alpha, w, T_after, band [H, W, d] (float64) and kept [d] — the ids the oracle's loop draws, in draw order — from the oracle's
    preprocess outputs `pre` and depth order `order`.  alpha is 0 where the pair is not blended; band is |255 alpha - 1| where the
    pair is inside the bbox with power <= 0, else inf.  z [d]: the fp32 camera depth of the kept."""
    bb, sg = pre["pixel_bboxes"], pre["sigmas"]
    drawable = ((bb[:, 2] - bb[:, 0]) * (bb[:, 3] - bb[:, 1]) != 0) & (sg != 0).all(1)
    order = np.asarray(order, np.int64)
    kept = order[drawable[order]]
    x, y = np.arange(W, dtype=np.float64)[None, :, None], np.arange(H, dtype=np.float64)[:, None, None]
    mean, s, b = pre["screen_means"][kept].astype(np.float64), sg[kept].astype(np.float64), bb[kept]
    dx, dy = mean[:, 0] - x, mean[:, 1] - y
    power = -0.5 * (s[:, 0] * dx * dx + s[:, 1] * dy * dy) - s[:, 2] * dx * dy
    with np.errstate(over="ignore"):
        raw = np.minimum(MAX_ALPHA, pre["opacity"][kept].astype(np.float64) * np.exp(power))
    inside = (x >= b[:, 0]) & (x < b[:, 2]) & (y >= b[:, 1]) & (y < b[:, 3]) & (power <= 0)
    band = np.where(inside, np.abs(255.0 * raw - 1.0), np.inf)
    alpha = np.where(inside & (raw > MIN_ALPHA), raw, 0.0)
    return _compose(alpha, band, kept, pre["cam_means"][kept, 2].copy())


def build_reference(orc, packed, args, perm=None):
    """The reference of a scene under the camera `args`, with the oracle fed the arrays in the order `perm` (scene index -> file
    index, a Morton-ordered scene's `order`; None: file order) so that exact depth ties resolve as the scene resolves them.  kept
    holds FILE ids either way.  The oracle's inputs ride along (pre, order: in the permuted indexing) for oracle_agreement."""
    W, H = int(args[6]), int(args[7])
    if perm is not None:
        packed = {k: np.ascontiguousarray(v[perm]) for k, v in packed.items()}
    pre = orc.preprocess(packed, orc.camera(*args))
    order = orc.depth_order(pre["cam_means"])
    ref = reference(pre, order, W, H)
    ref.update(pre=pre, order=order, kept_in=ref["kept"], n=len(order), W=W, H=H)
    if perm is not None:
        ref["kept"] = np.asarray(perm, np.int64)[ref["kept"]]
    return ref


def final_T(ref):
    return ref["T_after"][..., -1] if len(ref["kept"]) else np.ones(ref["alpha"].shape[:2])


def excluded(ref):
    """[H, W] bool: pixels holding a pair on the alpha threshold's band."""
    return (ref["band"] <= BAND).any(-1)


def tiny(ref):
    return (ref["w"] > 0) & (ref["w"] < TINY)


def feature_map(ref, F):
    """sum_i w_i F[i]: [H, W, C] for F [n, C] in file order."""
    return ref["w"] @ np.asarray(F, np.float64)[ref["kept"]]


def gradient(ref, G, n):
    """gF [n, C] = sum_p w(p) G[p]."""
    out = np.zeros((n, G.shape[-1]))
    out[ref["kept"]] = np.einsum("hwd,hwc->dc", ref["w"], np.asarray(G, np.float64))
    return out


def stats(ref, n, mask=None):
    """weight_sum, weight_max [n] float64; pixels as the range (lo, hi) [n] int: pairs with w >= TINY, pairs with w > 0."""
    w = ref["w"] if mask is None else ref["w"] * np.asarray(mask, bool)[..., None]
    out = [np.zeros(n), np.zeros(n), np.zeros(n, np.int64), np.zeros(n, np.int64)]
    if len(ref["kept"]):
        flat = w.reshape(-1, w.shape[-1])
        for o, v in zip(out, (flat.sum(0), flat.max(0, initial=0.0), (flat >= TINY).sum(0), (flat > 0).sum(0))):
            o[ref["kept"]] = v
    return dict(weight_sum=out[0], weight_max=out[1], pixels_lo=out[2], pixels_hi=out[3])


def pick(ref, median_T):
    """best_id, best_w, second_w (the runner-up's weight), count as (count_lo, count_hi), median_id and median_safe (no T_after of a
    contributing pair within ID_MARGIN of median_T).  Ties in weight go to the earlier in draw order."""
    w, kept = ref["w"], ref["kept"]
    shape = w.shape[:2]
    if not len(kept):
        none, zero = np.full(shape, -1, np.int64), np.zeros(shape)
        return dict(best_id=none, best_w=zero, second_w=zero, count_lo=none + 1, count_hi=none + 1, median_id=none, median_safe=zero == 0)
    j = w.argmax(-1)  # (the first of several maximisers)
    best_w = w.max(-1)
    second = np.sort(w, -1)[..., -2] if len(kept) > 1 else np.zeros(shape)
    hit = (ref["T_after"] < median_T) & (np.maximum.accumulate(ref["alpha"] > 0, -1))
    near = ((ref["alpha"] > 0) & (np.abs(ref["T_after"] - median_T) <= ID_MARGIN)).any(-1)
    return dict(best_id=np.where(best_w > 0, kept[j], -1), best_w=best_w, second_w=second, count_lo=(w >= TINY).sum(-1),
                count_hi=(w > 0).sum(-1), median_id=np.where(hit.any(-1), kept[hit.argmax(-1)], -1), median_safe=~near)


def topk(ref, k, select):
    """ids [H, W, k] (-1: unused), weights [H, W, k], and gap [H, W, k]: the slot's distance in weight to its nearer neighbour in
    the pixel's FULL sorted list (heaviest; inf for nearest, whose order is the draw order)."""
    w, kept = ref["w"], ref["kept"]
    d = len(kept)
    pad = max(0, k + 1 - d)
    wp = np.concatenate([w, np.zeros(w.shape[:2] + (pad,))], -1)
    idp = np.concatenate([kept, np.full(pad, -1, np.int64)])
    idx = np.argsort(-wp if select == "heaviest" else ~(wp > 0), axis=-1, kind="stable")[..., :k + 1]
    ws = np.take_along_axis(wp, idx, -1)
    ids = np.where(ws > 0, idp[idx], -1)
    if select == "heaviest":
        up = np.concatenate([np.full(ws.shape[:2] + (1,), np.inf), ws[..., :-1] - ws[..., 1:]], -1)
        gap = np.minimum(up[..., :k], up[..., 1:k + 1])
    else:
        gap = np.full(ws.shape[:2] + (k,), np.inf)
    return dict(ids=ids[..., :k], weights=ws[..., :k], gap=gap)


def slab(ref, near, far):
    """The reference of the kept subset near <= z < far (fp32 compares, uniform planes): T restarts at 1."""
    z = ref["z"]
    sel = (z >= np.float32(near)) & (z < np.float32(far))
    sub = _compose(ref["alpha"][..., sel], ref["band"][..., sel], ref["kept"][sel], z[sel])
    sub.update(n=ref["n"], W=ref["W"], H=ref["H"])
    return sub


def slab_edges(ref):
    """Three [near, far) pairs whose edges lie ON the z of gaussians the reference reaches; where two reached gaussians share a
    depth exactly, the first two pairs put a limit on that depth (the whole stack then falls on one side)."""
    inf = float("inf")
    zs = np.sort(ref["z"][(ref["w"] > 0).any((0, 1))])
    if not len(zs):
        return [(-inf, 1.0), (1.0, inf), (1.0, 2.0)]
    q = lambda f: float(zs[min(int(f * len(zs)), len(zs) - 1)])
    tied = np.unique(zs[1:][zs[1:] == zs[:-1]])
    behind = tied[tied > zs[0]]  # (a limit on the nearest depth of all would leave the far-only slab empty)
    tied = behind if len(behind) else tied
    mid = float(tied[len(tied) // 2]) if len(tied) else q(0.5)
    return [(-inf, mid), (mid if len(tied) else q(0.3), inf), (q(0.1), q(0.7))]


# ---- facts and shares of a reference (CPU) ------------------------------------------------------------------------------------------
def ulps_apart(a, b):
    """How many fp32 values lie between the positive floats a and b."""
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


def facts(ref):
    z = ref["z"]
    gaps = ulps_apart(z[1:], z[:-1]) if len(z) > 1 else np.zeros(0, np.int64)
    pos = ref["w"] > 0
    return dict(drawn=len(ref["kept"]), reached=int(pos.any((0, 1)).sum()), deepest=int(pos.sum(-1).max(initial=0)),
                ties=int((gaps == 0).sum()), min_gap_ulps=int(gaps[gaps > 0].min(initial=1 << 30)), empty=not bool(pos.any()),
                min_T=float(final_T(ref).min()))


def shares(ref):
    """The share each comparison leaves out, on the reference alone: what the CAP_* bound."""
    ex = excluded(ref)
    keep = ~ex
    pos = ref["w"] > 0
    out = dict(pixels=float(ex.mean()), tiny=float(tiny(ref).sum() / max(1, pos.sum())))
    p = pick(ref, 0.5)
    hitp = keep & (p["best_w"] > 0)
    out["best"] = float((hitp & (p["best_w"] - p["second_w"] <= ID_MARGIN)).sum() / max(1, keep.sum()))
    out["median"] = max(float((keep & ~pick(ref, m)["median_safe"]).sum() / max(1, keep.sum())) for m in MEDIANS)
    for k in KS:
        t = topk(ref, k, "heaviest")
        filled = (t["weights"] > 0) & keep[..., None]
        out[f"slots{k}"] = float((filled & (t["gap"] <= ID_MARGIN)).sum() / max(1, filled.sum()))
    return out


# The slot cap is held at k = 4 and 8, where tests/test_gpu_topk.py holds it.  At k = 16 no cap of this kind can hold on these
# scenes: slots 9 - 16 of a pixel with 50 - 140 contributors carry weights that lie closer than ID_MARGIN to one another (up to
# 17 % of the filled slots, seed 351; DESIGN.md has every pin's share).  So a slot within the margin is not simply left out, at
# any k: its id must still be one of the reference's candidates for it, a gaussian whose weight in that pixel is within
# ID_MARGIN of the slot's (run_topk).
CAPPED_KS = (4, 8)
CAPS = dict(pixels=CAP_PIXELS, tiny=CAP_TINY, best=CAP_BEST, median=CAP_MEDIAN, slots4=CAP_SLOTS, slots8=CAP_SLOTS)


def oracle_agreement(orc, ref):
    """(max |w - w_oracle|, max |T - T_oracle|): the C oracle's fp32 compositing loop with one-hot colours, three gaussians a
    pass over the depth order up to the last of the three, against the reference's weights; its final T against the reference's."""
    pre, order, W, H, kin = ref["pre"], ref["order"], ref["W"], ref["H"], ref["kept_in"]
    _, trans, drawn = orc.composite(order, pre, W, H, threads=orc.max_threads())
    assert drawn == len(kin)
    dT = float(np.abs(trans.T - final_T(ref)).max())
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    dw = 0.0
    for k0 in range(0, len(kin), 3):
        trio = kin[k0:k0 + 3]
        onehot = np.zeros((len(order), 3), np.float32)
        onehot[trio, np.arange(len(trio))] = 1.0
        sub = np.ascontiguousarray(order[:rank[trio].max() + 1])
        screen, _, _ = orc.composite(sub, dict(pre, rgb=onehot), W, H, threads=orc.max_threads())
        got = screen.transpose(1, 0, 2)[..., :len(trio)]
        dw = max(dw, float(np.abs(got - ref["w"][..., k0:k0 + len(trio)]).max()))
    return dw, dT


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
SHIFTS = ((0.05, -0.02, 0.1), (-0.03, 0.04, -0.05), (0.01, 0.01, 0.02), (-0.01, 0.0, 0.01), (0.0, 0.0, 0.001), (0.0, 0.0, -0.001))


def case_views(orc, case, perm=None):
    """[(args, ref)] x 3: the case's camera and two translated copies, the first two of SHIFTS under which the reference still
    draws something (a pin that draws nothing takes the first two)."""
    args = case["args"]
    views = [(args, build_reference(orc, case["packed"], args, perm))]
    spare = []
    for s in SHIFTS:
        a = (args[0], np.asarray(args[1], np.float64) + np.asarray(s)) + tuple(args[2:])
        r = build_reference(orc, case["packed"], a, perm)
        (views if (r["w"] > 0).any() else spare).append((a, r))
        if len(views) == 3:
            return views
    return (views + spare)[:3]


def _hamilton(a, b):
    """The Hamilton product of two quaternions (w, x, y, z)."""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def _axis_angle(axis, deg):
    axis, half = np.asarray(axis, np.float64), 0.5 * np.deg2rad(deg)
    return np.concatenate([[np.cos(half)], np.sin(half) * axis / np.linalg.norm(axis)])


def camera_variant(args, roll_deg, fy_ratio, orbit_axis, orbit_deg):
    """The camera `args` (make_camera's parameter list) rolled, orbited and made anamorphic: qvec' = q_z(roll) (x) qvec (x)
    q(orbit_axis, orbit), tvec' = R_z(roll) tvec, fy_full' = fy_ratio fy_full.  The orbit turns the world about its origin — which
    every pinned camera looks at — before the original pose; the roll turns the image about the optical axis.  With both, no entry
    of w2c's rotation block is zero, and focal_y, lim_y and tan_fov_y differ from their x counterparts."""
    qvec, tvec, fx_full, fy_full = args[:4]
    q = _hamilton(_hamilton(_axis_angle((0, 0, 1), roll_deg), np.asarray(qvec, np.float64)), _axis_angle(orbit_axis, orbit_deg))
    c, s = np.cos(np.deg2rad(roll_deg)), np.sin(np.deg2rad(roll_deg))
    t = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.asarray(tvec, np.float64)
    return (q, t, fx_full, fy_ratio * fy_full) + tuple(args[4:])


# name -> (roll_deg, fy_ratio, orbit_axis, orbit_deg).  Measured on every pin but the identities-only one, under both
# (tests/test_camera_variants.py asserts each): every entry of w2c's rotation block is nonzero; the caps, the clamp band and the SH
# left-out cap hold on the reference alone as they do under the pin's own camera.
CAMERAS = {"tilt_a": (33.0, 1.3, (1, 2, 3), 25.0), "tilt_b": (-117.0, 0.75, (3, -1, 2), -40.0)}


def features_of(seed, n):
    return (np.random.default_rng(1000 + seed).standard_normal((n, N_CH)) * 50.0).astype(np.float32)


def upstream_of(seed, H, W, views=1):
    return np.random.default_rng(2000 + seed).standard_normal((views, H, W, N_CH)).astype(np.float32)


def rect_mask(H, W):
    """A rectangle that is not tile-aligned (and not empty on a one-row frame)."""
    x0, y0 = min(5, W // 3), min(3, H // 3)
    m = np.zeros((H, W), bool)
    m[y0:max(y0 + 1, H - 2), x0:max(x0 + 1, W - 3)] = True
    return m


# ---- GPU: render a kind and check it against the reference -----------------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().numpy()


def _psnr(a, b, peak):
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return float("inf") if mse == 0 else 10.0 * np.log10(peak * peak / mse)


def plain_bar(tag, got, ref):
    """tests/gpu_cases.bar for a caller without tests/: per channel PSNR, peak = max |ref channel|, at least MIN_DB."""
    got, ref = np.asarray(got, np.float64).reshape(len(ref), -1), np.asarray(ref, np.float64).reshape(len(ref), -1)
    dbs = []
    for ch in range(ref.shape[1]):
        peak = float(np.abs(ref[:, ch]).max())
        dbs.append(_psnr(got[:, ch], ref[:, ch], peak) if peak > 0 else (float("inf") if not got[:, ch].any() else 0.0))
    assert min(dbs) >= MIN_DB, (tag, dbs)
    return dbs


def _note(fig, key, value, worst=max):
    fig[key] = value if key not in fig else worst(fig[key], value)


def _within(tag, err, where, tol, fig, key):
    e = float(err[where].max(initial=0.0))
    _note(fig, key, e)
    assert e <= tol, f"{tag}: {key} {e:.3e} > {tol:.1e} at {np.argwhere(where & (err > tol))[:4].tolist()}"


def check_map(tag, m, T, ref, F, bar, fig):
    """A feature map and its final T: the bar outside the excluded pixels, |T - T_ref| <= W_TOL there and <= STEP on them, and
    exactly 0 / 1 where the reference blends nothing."""
    ex = excluded(ref)
    keep = ~ex
    want, T_ref = feature_map(ref, F), final_T(ref)
    if keep.any():
        _note(fig, "dB", min(bar(tag, m[keep], want[keep])), min)
    err = np.abs(T.astype(np.float64) - T_ref)
    _within(tag, err, keep, W_TOL, fig, "T_err")
    _within(tag, err, ex, STEP, fig, "T_err_excluded")
    none = keep & ~(ref["alpha"] > 0).any(-1)
    assert not m[none].any() and (T[none] == 1).all(), f"{tag}: not exactly empty where the reference blends nothing"
    _note(fig, "excluded_px", float(ex.mean()))


def _dev(R, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(R.scene.device)


def run_forward(R, cam, ref, F, bar=plain_bar):
    """render_features at every width with return_T, render_slab with open limits, and the one-hot weights of the drawn
    gaussians themselves: each |w_gpu - w| <= W_TOL, and <= STEP on the excluded pixels."""
    fig = {}
    Ft = _dev(R, F)
    for C in WIDTHS:
        rows = Ft[:, :C].contiguous()
        m, T = R.render_features(cam, rows, return_T=True)
        check_map(f"features C={C}", _np(m), _np(T), ref, F[:, :C], bar, fig)
        sm, sT = R.render_slab(cam, rows)
        check_map(f"slab open C={C}", _np(sm), _np(sT), ref, F[:, :C], bar, fig)
    kept = ref["kept"]
    if 0 < len(kept) <= 1024:  # (one map's channel limit: every pinned case is far below it, a campaign case may not be)
        onehot = np.zeros((ref["n"], len(kept)), np.float32)
        onehot[kept, np.arange(len(kept))] = 1.0
        Wg = _np(R.render_features(cam, _dev(R, onehot))).astype(np.float64)
        ex = excluded(ref)[..., None] & np.ones(len(kept), bool)
        err = np.abs(Wg - ref["w"])
        _within("weights", err, ~ex, W_TOL, fig, "w_err")
        _within("weights", err, ex, STEP, fig, "w_err_excluded")
    return fig


def run_slab(R, cam, ref, F, z_gpu, bar=plain_bar):
    """Three [near, far) plane pairs with their edges ON drawn gaussians' z.  z_gpu [n]: the library's fp32 depths in file order;
    they must be the oracle's, bit for bit, on the drawn gaussians — the limits compare against them."""
    fig = {}
    assert np.array_equal(np.asarray(z_gpu, np.float32)[ref["kept"]], ref["z"]), "the library's z_cam is not the oracle's on the drawn gaussians"
    Ft = _dev(R, F)
    shape = (ref["H"], ref["W"])
    for near, far in slab_edges(ref):
        planes = [None if not np.isfinite(v) else _dev(R, np.full(shape, v, np.float32)) for v in (near, far)]
        sub = slab(ref, near, far)
        m, T = R.render_slab(cam, Ft, near=planes[0], far=planes[1])
        check_map(f"slab [{near}, {far})", _np(m), _np(T), sub, F, bar, fig)
        _note(fig, "slab_kept_min", len(sub["kept"]), min)
    return fig


def _gradient_bar(bar, tag, got, want, reach, lenient, fig, key):
    """The bar on a gradient.  Its peak is the largest |reference| of a channel over the ROWS: with one or two reached gaussians
    that is the row's own value, and where the terms w G of that row cancel, the bar measures a relative error of a cancelling fp32
    sum (a plain fp32 sum of the same terms on the CPU drops to 97 dB on campaign case 2495968322525521986).  lenient — the
    campaign only, never the suite — lets such a row pass as ill-conditioned while the error stays under 100 dB of the terms'
    own magnitude, 1e-5 sum_p w |G|; the share is tallied."""
    try:
        _note(fig, key, min(bar(tag, got, want)), min)
    except AssertionError:
        rel = float((np.abs(got - want) / np.maximum(reach, 1e-300)).max())
        if not lenient or rel > 1e-5:
            raise
        _note(fig, "ill_conditioned_rel", rel)


def run_backward(R, cam, ref, G, bar=plain_bar, lenient=False):
    """feature_gradient (17 channels and 1) and blend_weights against sum_p w G, the excluded pixels zeroed in G on both sides; rows
    the reference never reaches are exactly 0.  blend_weights takes no G: through the bar where no pixel is excluded, and always
    within W_TOL per reached pixel plus STEP per excluded pixel."""
    fig = {}
    ex = excluded(ref)
    keep, n = ~ex, ref["n"]
    Gz = G * keep[..., None]
    reached = np.zeros(n, bool)
    reached[ref["kept"]] = (ref["w"] * keep[..., None] > 0).any((0, 1))
    for C in (N_CH, 1):
        got = _np(R.feature_gradient(cam, _dev(R, Gz[..., :C])))
        want = gradient(ref, Gz[..., :C], n)
        _gradient_bar(bar, f"gradient C={C}", got, want, gradient(ref, np.abs(Gz[..., :C]), n), lenient, fig, "dB")
        assert not got[~reached].any(), f"gradient C={C}: a row the reference never reaches is not exactly 0"
    bw = _np(R.blend_weights(cam)).astype(np.float64)
    st = stats(ref, n)
    if not ex.any():
        _note(fig, "dB_blend_weights", min(bar("blend_weights", bw[:, None], st["weight_sum"][:, None])), min)
        reached_all = np.zeros(n, bool)
        reached_all[ref["kept"]] = (ref["w"] > 0).any((0, 1))
        assert not bw[~reached_all].any()
    err = np.abs(bw - st["weight_sum"])
    _note(fig, "blend_weights_err", float(err.max(initial=0.0)))
    assert (err <= W_TOL * st["pixels_hi"] + STEP * ex.sum() + 1e-12).all(), "blend_weights"
    return fig


def check_stats(tag, got, ref, mask, bar, fig):
    n = ref["n"]
    st = stats(ref, n, mask)
    _note(fig, "dB_sum", min(bar(f"{tag} weight_sum", got[0][:, None], st["weight_sum"][:, None])), min)
    _within(f"{tag} weight_max", np.abs(got[1].astype(np.float64) - st["weight_max"]), np.ones(n, bool), W_TOL, fig, "max_err")
    px = got[2].astype(np.int64)
    bad = (px < st["pixels_lo"]) | (px > st["pixels_hi"])
    assert not bad.any(), f"{tag} pixels: gaussians {np.flatnonzero(bad)[:6].tolist()} got {px[bad][:6].tolist()} want {st['pixels_hi'][bad][:6].tolist()}"


def run_stats(R, cam, ref, bar=plain_bar):
    """view_stats over the frame (the excluded pixels masked out through mask=; no mask at all where none is excluded), and again
    under a rectangular mask that is not tile-aligned."""
    fig = {}
    keep = ~excluded(ref)
    for tag, user in (("frame", None), ("rect", rect_mask(ref["H"], ref["W"]))):
        mask = keep if user is None else keep & user
        s = R.view_stats(cam, mask=None if (user is None and keep.all()) else _dev(R, mask))
        check_stats(f"stats {tag}", [_np(t) for t in s], ref, mask, bar, fig)
    return fig


def run_pick(R, cam, ref):
    """render_pick at every median_T with count=True; at 0.5 also without (the walk then stops early: the same ids and weight)."""
    fig = {}
    ex = excluded(ref)
    keep = ~ex
    for m in MEDIANS:
        p = R.render_pick(cam, median_T=m, count=True)
        bid, bw, mid, cnt = (_np(t) for t in p)
        want = pick(ref, m)
        err = np.abs(bw.astype(np.float64) - want["best_w"])
        _within(f"pick {m} best_w", err, keep, W_TOL, fig, "best_w_err")
        _within(f"pick {m} best_w", err, ex, STEP, fig, "best_w_err_excluded")
        sure = keep & ((want["best_w"] - want["second_w"] > ID_MARGIN) | (want["best_w"] == 0))
        _note(fig, "best_left_out", float((keep & ~sure).sum() / max(1, keep.sum())))
        assert fig["best_left_out"] <= CAP_BEST
        bad = sure & (bid != want["best_id"])
        assert not bad.any(), f"pick {m} best_id at {np.argwhere(bad)[:4].tolist()}: got {bid[bad][:4].tolist()} want {want['best_id'][bad][:4].tolist()}"
        bad = keep & ((cnt < want["count_lo"]) | (cnt > want["count_hi"]))
        assert not bad.any(), f"pick {m} count at {np.argwhere(bad)[:4].tolist()}: got {cnt[bad][:4].tolist()} want {want['count_hi'][bad][:4].tolist()}"
        safe = keep & want["median_safe"]
        _note(fig, "median_left_out", float((keep & ~safe).sum() / max(1, keep.sum())))
        assert fig["median_left_out"] <= CAP_MEDIAN
        bad = safe & (mid != want["median_id"])
        assert not bad.any(), f"pick {m} median_id at {np.argwhere(bad)[:4].tolist()}: got {mid[bad][:4].tolist()} want {want['median_id'][bad][:4].tolist()}"
        if m == 0.5:
            q = R.render_pick(cam, median_T=m)
            assert q.count is None and all(np.array_equal(_np(a), b) for a, b in zip(q[:3], (bid, bw, mid))), "pick without count differs"
    return fig


def run_topk(R, cam, ref):
    """render_topk, heaviest and nearest, at every k of KS with the final T; at k = 8 also without it (the same lists)."""
    fig = {}
    ex = excluded(ref)
    keep, T_ref = ~ex, final_T(ref)
    for select in ("heaviest", "nearest"):
        for k in KS:
            t = R.render_topk(cam, k, select=select, return_T=True)
            ids, ws, T = (_np(a) for a in t)
            want = topk(ref, k, select)
            tag = f"topk {select} k={k}"
            err = np.abs(ws.astype(np.float64) - want["weights"])
            k3 = keep[..., None] & np.ones(k, bool)
            _within(tag, err, k3, W_TOL, fig, f"{select}_w_err")
            if select == "heaviest":  # (sorted weights move by no more than the weights do; a flipped pair SHIFTS a nearest list)
                _within(tag, err, ~k3, STEP, fig, "heaviest_w_err_excluded")
            _within(tag + " T", np.abs(T.astype(np.float64) - T_ref), keep, W_TOL, fig, "T_err")
            filled = k3 & (want["weights"] > 0)
            sure = k3 & (want["gap"] > ID_MARGIN) & ~((want["weights"] > 0) & (want["weights"] < TINY))
            if select == "heaviest":
                share = float((filled & ~sure).sum() / max(1, filled.sum()))
                _note(fig, f"slots{k}_left_out", share)
                assert k not in CAPPED_KS or share <= CAP_SLOTS, (tag, share)
            bad = sure & (ids != want["ids"])
            assert not bad.any(), f"{tag} ids at {np.argwhere(bad)[:4].tolist()}: got {ids[bad][:4].tolist()} want {want['ids'][bad][:4].tolist()}"
            # a slot within the margin: the id is a candidate for it (its reference weight there is within ID_MARGIN of the slot's)
            pos = np.full(ref["n"] + 1, -1, np.int64)
            pos[ref["kept"]] = np.arange(len(ref["kept"]))
            at = pos[ids]  # (-1 -> the spare last entry, -1)
            w_of = np.take_along_axis(np.concatenate([ref["w"], np.zeros(ref["w"].shape[:2] + (1,))], -1), at, -1)
            ok = (np.abs(w_of - want["weights"]) <= ID_MARGIN) & ((at >= 0) | (want["weights"] < TINY))
            bad = filled & ~sure & ~ok
            assert not bad.any(), f"{tag} ids within the margin at {np.argwhere(bad)[:4].tolist()}: got {ids[bad][:4].tolist()}"
            assert not ws[ids < 0].any(), f"{tag}: an unused slot carries a weight"
            if k == 8:
                u = R.render_topk(cam, k, select=select)
                assert u.final_T is None and np.array_equal(_np(u.ids), ids) and np.array_equal(_np(u.weights), ws), f"{tag} without T differs"
    return fig


def run_views(renderer, R, views, F, Gs, bar=plain_bar, lenient=False):
    """A Rasterizer(views=3) over `views` = [(cam, ref)] x 3: every single view's map against its own reference first, then
    render_features_batch and view_stats_batch (max, pixels, views) bit for bit the singles, weight_sum and
    feature_gradient_batch through the bar."""
    import torch

    fig = {}
    RK = renderer.Rasterizer(R.scene, views=len(views))
    cams = [cam for cam, _ in views]
    Ft = _dev(R, F)
    for C in (N_CH, 3):
        rows = Ft[:, :C].contiguous()
        singles = [R.render_features(cam, rows, return_T=True) for cam in cams]
        if C == N_CH:
            for v, ((m, T), (_, ref)) in enumerate(zip(singles, views)):
                check_map(f"view {v}", _np(m), _np(T), ref, F, bar, fig)
        bm, bT = RK.render_features_batch(cams, rows, return_T=True)
        assert torch.equal(bm, torch.stack([m for m, _ in singles])) and torch.equal(bT, torch.stack([T for _, T in singles])), f"batch C={C}"
    keeps = [~excluded(ref) for _, ref in views]
    masks = None if all(k.all() for k in keeps) else [_dev(R, k) for k in keeps]
    per = [R.view_stats(cam, mask=None if masks is None else masks[v]) for v, cam in enumerate(cams)]
    for v, (s, (_, ref)) in enumerate(zip(per, views)):
        check_stats(f"view {v} stats", [_np(t) for t in s], ref, keeps[v], bar, fig)
    bs, hits = RK.view_stats_batch(cams, masks=masks)
    assert torch.equal(bs.weight_max, torch.stack([s.weight_max for s in per]).max(0).values), "batch weight_max"
    assert torch.equal(bs.pixels, torch.stack([s.pixels for s in per]).sum(0).to(torch.int32)), "batch pixels"
    assert torch.equal(hits, torch.stack([s.pixels > 0 for s in per]).sum(0).to(torch.int32)), "batch views"
    n = views[0][1]["n"]
    want_sum = sum(stats(ref, n, keeps[v])["weight_sum"] for v, (_, ref) in enumerate(views))
    _note(fig, "dB_sum", min(bar("batch weight_sum", _np(bs.weight_sum)[:, None], want_sum[:, None])), min)
    Gz = np.stack([Gs[v] * keeps[v][..., None] for v in range(len(views))]).astype(np.float32)
    got = _np(RK.feature_gradient_batch(cams, _dev(R, Gz)))
    want = sum(gradient(ref, Gz[v], n) for v, (_, ref) in enumerate(views))
    reach = sum(gradient(ref, np.abs(Gz[v]), n) for v, (_, ref) in enumerate(views))
    _gradient_bar(bar, "batch gradient", got, want, reach, lenient, fig, "dB_gradient")
    fig["views_drawing"] = sum(bool((ref["w"] > 0).any()) for _, ref in views)
    return fig


def run_identities(renderer, R, cams, F, G):
    """What holds between the kernels whatever the draw order of near-equal depths is (a scene whose order the reference does not
    pin): top-k k = 1 is the pick maps; sum_i pixels_i = sum_p count; weight_max[i] >= best_w wherever best_id == i, and weight_max,
    pixels, best_w and count are bit for bit those of the one-hot weights; the slab with open limits is the channel blend; <G, render_features(F)> =
    <feature_gradient(G), F> to 1e-5 relative; the K = 3 batch equals the singles."""
    import torch

    fig = {}
    cam = cams[0]
    Ft, Gt = _dev(R, F), _dev(R, G)
    p = R.render_pick(cam, count=True, scene_order=True)
    t = R.render_topk(cam, 1, scene_order=True)
    assert torch.equal(t.ids[..., 0], p.best_id) and torch.equal(t.weights[..., 0], p.best_w), "top-1 is not the pick"
    near = R.render_topk(cam, 1, select="nearest", scene_order=True)
    first = R.render_pick(cam, median_T=1.0, scene_order=True)
    assert torch.equal(near.ids[..., 0], first.median_id), "nearest-1 is not the first hit"
    s = R.view_stats(cam, scene_order=True)
    assert int(s.pixels.sum()) == int(p.count.sum()), "sum of pixels is not the sum of counts"
    hit = p.best_id >= 0
    ids, bw = p.best_id[hit].long(), p.best_w[hit]
    assert bool((s.weight_max[ids] >= bw).all()), "weight_max below a best weight"
    assert float(s.weight_max.max()) == float(p.best_w.max()), "the frame's largest weight"
    # (weight_max[i] need not BE one of i's best weights: i may reach its largest weight under a heavier gaussian — 3 of the 119
    # ids that are somebody's best on seed 283, in the float64 reference itself.  What does hold for every id: the statistics and
    # the pick maps are plain functions of the one-hot weights, bit for bit.)
    n = R.scene.n
    fig["one_hot"] = int(G.shape[0] * G.shape[1] * n <= 50_000_000)  # (a campaign case may be too large for its n weight maps)
    if fig["one_hot"]:
        parts = []
        for a in range(0, n, 1024):
            eye = torch.zeros((n, min(1024, n - a)), dtype=torch.float32, device=R.scene.device)
            eye[a:a + eye.shape[1]].fill_diagonal_(1.0)
            parts.append(R.render_features(cam, eye, scene_order=True))
        Wg = torch.cat(parts, -1)
        flat = Wg.flatten(0, 1)
        assert torch.equal(s.weight_max, flat.max(0).values) and torch.equal(s.pixels, (flat > 0).sum(0).to(torch.int32)), "stats are not the one-hot weights'"
        assert torch.equal(p.best_w, Wg.max(-1).values) and torch.equal(p.count, (Wg > 0).sum(-1).to(torch.int32)), "pick is not the one-hot weights'"
        assert torch.equal(Wg[hit].gather(-1, ids[:, None])[:, 0], bw), "best_id does not carry best_w"
    assert bool(((s.pixels > 0) == (s.weight_max > 0)).all()) and bool(((s.pixels > 0) == (s.weight_sum > 0)).all())
    for C in (3, N_CH):
        rows = Ft[:, :C].contiguous()
        m, T = R.render_features(cam, rows, return_T=True)
        sm, sT = R.render_slab(cam, rows)
        assert torch.equal(sm, m) and torch.equal(sT, T), f"open slab C={C}"
    m = R.render_features(cam, Ft).double()
    gF = R.feature_gradient(cam, Gt).double()
    a, b = float((Gt.double() * m).sum()), float((gF * Ft.double()).sum())
    fig["adjoint_rel"] = abs(a - b) / max(abs(a), abs(b), 1e-300)
    assert fig["adjoint_rel"] <= 1e-5, (a, b)
    fig["drawn_px"] = int(hit.sum())
    RK = renderer.Rasterizer(R.scene, views=len(cams))
    singles = [R.render_features(c, Ft, return_T=True) for c in cams]
    bm, bT = RK.render_features_batch(cams, Ft, return_T=True)
    assert torch.equal(bm, torch.stack([x for x, _ in singles])) and torch.equal(bT, torch.stack([x for _, x in singles])), "batch"
    per = [R.view_stats(c) for c in cams]
    bs, hits = RK.view_stats_batch(cams)
    assert torch.equal(bs.weight_max, torch.stack([x.weight_max for x in per]).max(0).values)
    assert torch.equal(bs.pixels, torch.stack([x.pixels for x in per]).sum(0).to(torch.int32))
    assert torch.equal(hits, torch.stack([x.pixels > 0 for x in per]).sum(0).to(torch.int32))
    return fig
