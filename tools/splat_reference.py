"""A float64 reference of the splat gradient — the derivative of L = sum_p G[p] . map[p] + sum_p gT[p] T_final[p] in every
gaussian's opacity, 2-D mean and inverse 2-D covariance — an fp32 emulation of the kernel's arithmetic order, the bound that
holds either of them to the closed form, and the checks tests/test_gpu_splat_gradient.py calls.

Built on tools/fuzz_maps.py's arrays (build_reference: alpha, w, T_after [H, W, d] in draw order, kept [d], the oracle's preprocess
outputs).  Notation as there: dx = mean_x - x, dy = mean_y - y, power = -(s0 dx^2 + s1 dy^2) / 2 - s2 dx dy, u = o exp(power),
alpha = min(0.99, u) kept where alpha > 1/255 and power <= 0 inside the bbox; w = alpha T, T <- T (1 - alpha).  With
s_i(p) = G[p] . f_i:  R_i = sum_{j > i} w_j s_j + gT T_final,  dL/dalpha_i = T_i s_i - R_i / (1 - alpha_i),  e_i = dL/dalpha_i alpha_i,
0 where the pair is not kept, where the cap is active (u >= 0.99) and where T_i < min_T.  The support is held fixed.

Columns of a result [n, 8] (file order): opacity, mean x, mean y, s0, s1, s2, |mean x|, |mean y| (per-pixel absolute values).
numpy only in the first half; the run_* functions take a Rasterizer.  Needs nothing from tests/.
"""
import numpy as np

import fuzz_maps as fm

COLUMNS = ("opacity", "mean_x", "mean_y", "s0", "s1", "s2", "abs_mean_x", "abs_mean_y")
REL = 1e-5            # the project's standing "100 dB of the terms' own magnitude" (fuzz_maps._gradient_bar)
CAP_BAND = 1e-4       # |u / 0.99 - 1| at or below this: fp32 may decide `cap active` the other way; the pixel is left out
T_BAND = 1e-3         # |T_i / min_T - 1| at or below this: fp32 may decide `T_i < min_T` the other way
FD_STEP = 1e-6
FD_REL = 1e-5
FD_ROWS = 8
EMU_DB = 110.0        # the plain 100 dB bar is asserted on the device where the emulation reaches this


def gT_of(seed, H, W):
    return (50.0 * np.random.default_rng(3000 + seed).standard_normal((H, W))).astype(np.float32)


# ---- geometry of the pairs ------------------------------------------------------------------------------------------------------------
def params_of(ref):
    """(mean [d, 2], s [d, 3], o [d]) float64 of the drawn gaussians, in draw order: what the gradient is taken in."""
    pre, k = ref["pre"], ref["kept_in"]
    return (pre["screen_means"][k].astype(np.float64), pre["sigmas"][k].astype(np.float64), pre["opacity"][k].astype(np.float64))


def pair_geometry(ref, params=None):
    """dx, dy, power [H, W, d] and u = o exp(power) (uncapped) for `params` (default: the reference's own)."""
    mean, s, o = params_of(ref) if params is None else params
    x, y = np.arange(ref["W"], dtype=np.float64)[None, :, None], np.arange(ref["H"], dtype=np.float64)[:, None, None]
    dx, dy = mean[:, 0] - x, mean[:, 1] - y
    power = -0.5 * (s[:, 0] * dx * dx + s[:, 1] * dy * dy) - s[:, 2] * dx * dy
    with np.errstate(over="ignore"):
        u = o * np.exp(power)
    return dx, dy, power, u


def cap_band(ref):
    """[H, W] bool: pixels holding a kept pair whose u lies within CAP_BAND (relative) of the cap."""
    if not len(ref["kept"]):
        return np.zeros((ref["H"], ref["W"]), bool)
    u = pair_geometry(ref)[3]
    return ((ref["alpha"] > 0) & (np.abs(u / fm.MAX_ALPHA - 1.0) <= CAP_BAND)).any(-1)


def left_out(ref, min_T=0.0):
    """[H, W] bool: the pixels a comparison leaves out (G = 0 and gT = 0 there on both sides, which removes them exactly): the 1/255
    band of fuzz_maps.excluded, the cap band, and with min_T > 0 the pixels holding a kept pair with T_i within T_BAND of it."""
    out = fm.excluded(ref) | cap_band(ref)
    if min_T > 0 and len(ref["kept"]):
        T_in = ref["w"] / np.where(ref["alpha"] > 0, ref["alpha"], 1.0)
        out = out | ((ref["alpha"] > 0) & (np.abs(T_in / min_T - 1.0) <= T_BAND)).any(-1)
    return out


def truncated(ref, drawn):
    """The reference with the pairs outside `drawn` [H, W, d] taken out of the draw (alpha = 0 there) and T recomposed: what a
    forward that stopped early blended."""
    sub = fm._compose(np.where(drawn, ref["alpha"], 0.0), ref["band"], ref["kept"], ref["z"])
    for k in ("pre", "order", "kept_in", "n", "W", "H"):
        sub[k] = ref[k]
    return sub


# ---- the closed form (float64) --------------------------------------------------------------------------------------------------------
def _T_before(ref):
    d = ref["alpha"].shape[-1]
    return np.concatenate([np.ones(ref["alpha"].shape[:2] + (1,)), ref["T_after"][..., :-1]], -1) if d else ref["T_after"]


def _dpower(ref, dx, dy):
    """|d power / d theta| needs these: the six derivatives [6][H, W, d] of log u in (o, mean x, mean y, s0, s1, s2)."""
    _, s, o = params_of(ref)
    return [np.broadcast_to(1.0 / o, dx.shape), -s[:, 0] * dx - s[:, 2] * dy, -s[:, 1] * dy - s[:, 2] * dx, -0.5 * dx * dx,
            -0.5 * dy * dy, -dx * dy]


def closed_form(ref, F, G, gT=None, min_T=0.0):
    """dict(g [n, 8], A [n, 8], B [n, 8], reached [n] bool) in file order.  F [n, C] in file order, G [H, W, C], gT [H, W] or None.
    A = sum_p |term|, the row's own terms in absolute value; B = sum_p alpha / (1 - alpha) (sum_j w_j |s_j| + |gT| T_final)
    |d power / d theta|, the magnitude the kernel's subtraction S' - P_i works at (both over the pairs whose e is not forced to 0).
    Columns 6 and 7 carry the bound of columns 1 and 2."""
    n, d = ref["n"], len(ref["kept"])
    out = dict(g=np.zeros((n, 8)), A=np.zeros((n, 8)), B=np.zeros((n, 8)), reached=np.zeros(n, bool))
    if not d:
        return out
    G = np.asarray(G, np.float64)
    gT = np.zeros(G.shape[:2]) if gT is None else np.asarray(gT, np.float64)
    dx, dy, _, u = pair_geometry(ref)
    alpha, w, Tb, Tf = ref["alpha"], ref["w"], _T_before(ref), fm.final_T(ref)
    S = np.einsum("hwc,dc->hwd", G, np.asarray(F, np.float64)[ref["kept"]])
    ws = w * S
    behind = np.flip(np.cumsum(np.flip(ws, -1), -1), -1) - ws  # sum_{j > i}
    R = behind + (gT * Tf)[..., None]
    moves = (alpha > 0) & (u < fm.MAX_ALPHA) & (Tb >= min_T)
    ratio = alpha / (1.0 - alpha)
    e = np.where(moves, ws - R * ratio, 0.0)
    mag = np.where(moves, ratio * ((w * np.abs(S)).sum(-1) + np.abs(gT) * Tf)[..., None], 0.0)
    rows = {k: np.zeros((d, 8)) for k in ("g", "A", "B")}
    for c, dp in enumerate(_dpower(ref, dx, dy)):
        term = e * dp
        rows["g"][:, c] = term.sum((0, 1))
        rows["A"][:, c] = np.abs(term).sum((0, 1))
        rows["B"][:, c] = (mag * np.abs(dp)).sum((0, 1))
    for c in (1, 2):
        rows["g"][:, 5 + c] = rows["A"][:, c]
        rows["A"][:, 5 + c], rows["B"][:, 5 + c] = rows["A"][:, c], rows["B"][:, c]
    for k in rows:
        out[k][ref["kept"]] = rows[k]
    out["reached"][ref["kept"]] = (e != 0).any((0, 1))
    return out


def loss_pixels(ref, params, F, G, gT):
    """L per pixel [H, W] (float64) at `params`, the support (which pairs are kept) frozen at the reference's: what the finite
    differences difference.  The cap stays live: a pair moves across it only inside the cap band, which the caller has left out."""
    u = pair_geometry(ref, params)[3]
    alpha = np.where(ref["alpha"] > 0, np.minimum(fm.MAX_ALPHA, u), 0.0)
    T_after = np.cumprod(1.0 - alpha, -1)
    T_before = np.concatenate([np.ones(alpha.shape[:2] + (1,)), T_after[..., :-1]], -1)
    S = np.einsum("hwc,dc->hwd", np.asarray(G, np.float64), np.asarray(F, np.float64)[ref["kept"]])
    return (alpha * T_before * S).sum(-1) + np.asarray(gT, np.float64) * T_after[..., -1]


def finite_differences(ref, F, G, gT, rows):
    """Central differences of L in the six parameters of the drawn gaussians `rows` (indices in draw order): [len(rows), 6], step
    FD_STEP max(1, |value|).  The per-pixel losses are differenced before they are summed."""
    mean, s, o = params_of(ref)
    out = np.zeros((len(rows), 6))
    for a, i in enumerate(rows):
        for c in range(6):
            arr, j = ((o, None), (mean, 0), (mean, 1), (s, 0), (s, 1), (s, 2))[c]
            at = (i,) if j is None else (i, j)
            h = FD_STEP * max(1.0, abs(arr[at]))
            side = []
            for sign in (1.0, -1.0):
                p = [mean.copy(), s.copy(), o.copy()]
                p[(2, 0, 0, 1, 1, 1)[c]][at] += sign * h
                side.append(loss_pixels(ref, tuple(p), F, G, gT))
            out[a, c] = (side[0] - side[1]).sum() / (2.0 * h)
    return out


def fd_rows(ref, reached_d, count=FD_ROWS):
    """`count` of the drawn gaussians the gradient reaches, spread evenly over the draw order."""
    idx = np.flatnonzero(reached_d)
    return idx if len(idx) <= count else idx[np.linspace(0, len(idx) - 1, count).round().astype(int)]


# ---- the kernel's arithmetic order in fp32 ------------------------------------------------------------------------------------------------
def emulate_fp32(ref, F, G, gT=None, min_T=0.0):
    """[n, 8]: the gradient as the kernel forms it, in numpy float32 — alpha, T and w sequentially in draw order, the dot over the
    channels in channel order, P = P + w s sequentially, S' = P_last + gT T_final, and in a second pass over the same order
    R_i = S' - P_i, e = w s - R alpha / (1 - alpha); the sums over the pixels in fp32.  The support (which pairs are kept, which sit on
    the cap) is the reference's.  It does not model the device's exp2 or the order of its atomic sums."""
    f32 = np.float32
    n, d, H, W = ref["n"], len(ref["kept"]), ref["H"], ref["W"]
    out = np.zeros((n, 8), f32)
    if not d:
        return out
    pre, k = ref["pre"], ref["kept_in"]
    mean, s, o = pre["screen_means"][k].astype(f32), pre["sigmas"][k].astype(f32), pre["opacity"][k].astype(f32)
    G = np.asarray(G, f32)
    Fk = np.asarray(F, f32)[ref["kept"]]
    gT = np.zeros((H, W), f32) if gT is None else np.asarray(gT, f32)
    x, y = np.arange(W, dtype=f32)[None, :], np.arange(H, dtype=f32)[:, None]
    kept, capped = ref["alpha"] > 0, pair_geometry(ref)[3] >= fm.MAX_ALPHA
    half = f32(0.5)

    def pair(i):
        dx, dy = mean[i, 0] - x, mean[i, 1] - y
        power = -half * (s[i, 0] * dx * dx + s[i, 1] * dy * dy) - s[i, 2] * dx * dy
        with np.errstate(over="ignore"):
            a = np.minimum(f32(fm.MAX_ALPHA), o[i] * np.exp(power, dtype=f32))
        a = np.where(kept[..., i], a, f32(0)).astype(f32)
        sv = np.zeros((H, W), f32)
        for c in range(G.shape[-1]):
            sv = sv + G[..., c] * Fk[i, c]
        return dx, dy, a, sv

    T, P = np.ones((H, W), f32), np.zeros((H, W), f32)
    for i in range(d):
        _, _, a, sv = pair(i)
        P = P + (a * T) * sv
        T = T - T * a
    Sp = P + gT * T
    T, P = np.ones((H, W), f32), np.zeros((H, W), f32)
    rows = np.zeros((d, 8), f32)
    for i in range(d):
        dx, dy, a, sv = pair(i)
        w = a * T
        P = P + w * sv
        R = Sp - P
        e = w * sv - R * (a / (f32(1) - a))
        e = np.where(kept[..., i] & ~capped[..., i] & (T >= f32(min_T)), e, f32(0)).astype(f32)
        T = T - T * a
        mx, my = -s[i, 0] * dx - s[i, 2] * dy, -s[i, 1] * dy - s[i, 2] * dx
        terms = [e / o[i], e * mx, e * my, e * (-half * dx * dx), e * (-half * dy * dy), e * (-(dx * dy))]
        terms += [np.abs(terms[1]), np.abs(terms[2])]
        rows[i] = [t.astype(f32).sum(dtype=f32) for t in terms]
    out[ref["kept"]] = rows
    return out


# ---- comparing a result with the closed form ------------------------------------------------------------------------------------------------
def column_db(got, want):
    """The plain bar per column: PSNR over the rows, peak = max |reference column| (inf where both are zero)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    dbs = []
    for c in range(want.shape[1]):
        peak = float(np.abs(want[:, c]).max(initial=0.0))
        mse = float(np.mean((got[:, c] - want[:, c]) ** 2)) if len(want) else 0.0
        dbs.append(float("inf") if mse == 0 else (10.0 * np.log10(peak * peak / mse) if peak > 0 else 0.0))
    return dbs


def bound_ratio(got, cf, columns):
    """max over rows and `columns` of |got - g| / (REL (A + B)): at most 1 where the bound holds.  0 / 0 counts as 0."""
    err = np.abs(np.asarray(got, np.float64)[:, columns] - cf["g"][:, columns])
    lim = REL * (cf["A"][:, columns] + cf["B"][:, columns])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / lim)
    return float(r.max(initial=0.0))


def check_gradient(tag, got, cf, columns, fig, plain=False):
    """The bound per row and column; rows the reference never reaches exactly 0; the plain bar where asked for.  Prints first."""
    got = np.asarray(got, np.float64)
    ratio = bound_ratio(got, cf, columns)
    dbs = [column_db(got, cf["g"])[c] for c in columns]
    fm._note(fig, "bound_ratio", ratio)
    fm._note(fig, "dB", min(dbs, default=float("inf")), min)
    print(f"\nsplat {tag}: |err| / (1e-5 (A + B)) {ratio:.3g}; dB " + " ".join(f"{COLUMNS[c]}={v:.1f}" for c, v in zip(columns, dbs)), end="")
    assert ratio <= 1.0, f"{tag}: |err| exceeds 1e-5 (A + B) by a factor of {ratio:.3g}"
    assert not got[~cf["reached"]][:, columns].any(), f"{tag}: a row the reference never reaches is not exactly 0"
    if plain:
        assert min(dbs) >= fm.MIN_DB, (tag, dbs)


# ---- GPU: Rasterizer.splat_gradient against the closed form -----------------------------------------------------------------------------------
def as_rows(g):
    """A SplatGradient as [n, 8] float64 (columns 6 and 7 zero without abs_mean2d)."""
    cols = [fm._np(g.opacity)[:, None], fm._np(g.mean2d), fm._np(g.sigmas)]
    cols.append(fm._np(g.abs_mean2d) if g.abs_mean2d is not None else np.zeros_like(cols[1]))
    return np.concatenate(cols, 1).astype(np.float64)


def masked_inputs(ref, G, gT, min_T=0.0):
    keep = ~left_out(ref, min_T)
    return (np.asarray(G, np.float32) * keep[..., None]).astype(np.float32), (np.asarray(gT, np.float32) * keep).astype(np.float32)


def run_parity(R, cam, ref, F, G, gT, widths=(17, 16, 3, 1)):
    """splat_gradient at every width, with grad_T and without, against the closed form; the left-out pixels zeroed in G and gT on
    both sides.  The plain 100 dB bar per column is asserted too wherever the fp32 emulation of the same inputs reaches EMU_DB
    (the 10 dB between them are for the device's exp2, which the emulation does not model); fig["plain"] counts those."""
    fig = {"plain": 0}
    Gz, gTz = masked_inputs(ref, G, gT)
    Ft = fm._dev(R, F)
    six = list(range(6))
    for C in widths:
        for with_T in (True, False):
            t = gTz if with_T else None
            got = R.splat_gradient(cam, Ft[:, :C].contiguous(), fm._dev(R, Gz[..., :C]), fm._dev(R, gTz) if with_T else None)
            assert got.abs_mean2d is None
            cf = closed_form(ref, F[:, :C], Gz[..., :C], t)
            emu_db = min(column_db(emulate_fp32(ref, F[:, :C], Gz[..., :C], t), cf["g"])[:6])
            plain = emu_db >= EMU_DB
            fig["plain"] += int(plain)
            fm._note(fig, "emu_dB", emu_db, min)
            check_gradient(f"C={C} gT={int(with_T)} (emulation {emu_db:.1f} dB)", as_rows(got), cf, six, fig, plain)
    return fig
