"""A float64 reference of the SH colour backward — the gradient of a view's per-gaussian colours carried to the SH coefficients and,
through the view direction, to the means: the transpose of sh_to_rgb (csrc/gauss_math.h, sh_eval_with) — an fp32 emulation of
the kernel's arrangement, the bound that holds either of them to the reference, and the checks tests/test_gpu_sh_backward.py calls.

The forward, per gaussian:  d = mean - cam_center, r = |d|, u = d / r;  v_c = sum_k b_k(u) sh[k][c] + 0.5 over k < (degree + 1)^2;
colour_c = clamp(v_c, 0, 1).  b_k are the sixteen real SH polynomials as spherical_harmonics.py writes them, b_3 with the sign the
forward applies it with (it SUBTRACTS (c1 x) sh_3).  The clamp has derivative m_c = [0 <= v_c <= 1]: the edges pass, as
torch.clamp's autograd passes them.

sh64 evaluates the forward; vjp64 is the transpose written out — the basis for grad_sh, the analytic grad_u b_k (the polynomials
differentiated as they stand, x, y, z independent), then du / dd = (I - u u^T) / r; bound64 is the same chain with every factor and
the upstream in absolute value — every MONOMIAL of a basis polynomial and of its derivative, not the polynomial's value: 2 z^2 -
x^2 - y^2 cancels, and an fp32 evaluation works at the size of its terms — which gives the componentwise magnitude B an fp32
evaluation is held to: |err| <= 1e-5 B per element.  emulate_fp32 is the kernel's arrangement in torch float32.

An entry (gaussian, channel) with min(|v|, |v - 1|) <= CLAMP_BAND is left out: fp32 may decide the clamp the other way.
r = 0 (a mean on the camera centre): the forward is NaN above degree 0 and the gaussian contributes nothing.

theta: dict(means [m, 3], sh [m, 16, 3]).  cam: anything with a cam_center (the oracle's camera is one), or the three numbers.
numpy in and out.  Needs nothing from tests/.
"""
import numpy as np

FIELDS = ("sh", "means")
REL = 1e-5            # the project's standing bar (splat_reference.REL, projection_reference.REL)
ORACLE_REL = 1e-5     # sh64's clamped colour against the fp32 oracle's rgb: of max(|value|, the column's largest |value|)
AUTOGRAD_REL = 1e-10
CLAMP_BAND = 1e-5     # min(|v|, |v - 1|) at or below this: fp32 may decide the clamp the other way; the entry is left out
CAP_LEFT_OUT = 2      # entries left out per pin and degree, at most

C0, C1 = 0.28209479177387814, 0.4886025119029199
K2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
K3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
      -0.5900435899266435)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def theta_of(packed, perm=None, widen_f16=False):
    """means and sh of a packed scene as float64, in the order `perm` (scene index -> file index; None: the file's).  widen_f16:
    the coefficients as a scene that stores them in float16 holds them."""
    sh = np.asarray(packed["sh"], np.float32).reshape(-1, 16, 3)
    if widen_f16:
        sh = sh.astype(np.float16).astype(np.float32)
    t = dict(means=np.asarray(packed["means"], np.float64), sh=sh.astype(np.float64))
    return t if perm is None else {k: v[np.asarray(perm, np.int64)] for k, v in t.items()}


def rows_of(theta, idx):
    return {k: v[idx] for k, v in theta.items()}


def centre_of(cam):
    return np.array(list(cam.cam_center) if hasattr(cam, "cam_center") else list(cam), np.float64)


def coefficients(degree):
    return (int(degree) + 1) ** 2


# ---- the basis: every polynomial as a list of signed monomials coefficient * x^a y^b z^c ---------------------------------------------
def _poly(*terms):
    return tuple(terms)


BASIS = (
    _poly((C0, 0, 0, 0)),
    _poly((-C1, 0, 1, 0)), _poly((C1, 0, 0, 1)), _poly((-C1, 1, 0, 0)),
    _poly((K2[0], 1, 1, 0)), _poly((K2[1], 0, 1, 1)), _poly((2 * K2[2], 0, 0, 2), (-K2[2], 2, 0, 0), (-K2[2], 0, 2, 0)),
    _poly((K2[3], 1, 0, 1)), _poly((K2[4], 2, 0, 0), (-K2[4], 0, 2, 0)),
    _poly((3 * K3[0], 2, 1, 0), (-K3[0], 0, 3, 0)), _poly((K3[1], 1, 1, 1)),
    _poly((4 * K3[2], 0, 1, 2), (-K3[2], 2, 1, 0), (-K3[2], 0, 3, 0)),
    _poly((2 * K3[3], 0, 0, 3), (-3 * K3[3], 2, 0, 1), (-3 * K3[3], 0, 2, 1)),
    _poly((4 * K3[4], 1, 0, 2), (-K3[4], 3, 0, 0), (-K3[4], 1, 2, 0)),
    _poly((K3[5], 2, 0, 1), (-K3[5], 0, 2, 1)), _poly((K3[6], 3, 0, 0), (-3 * K3[6], 1, 2, 0)),
)


def _monomial(u, a, b, c):
    return u[:, 0] ** a * u[:, 1] ** b * u[:, 2] ** c


def basis(u, absolute=False):
    """[m, 16]: b_k(u); absolute: every monomial in absolute value."""
    out = np.zeros((len(u), 16))
    v = np.abs(u) if absolute else u
    for k, poly in enumerate(BASIS):
        for coef, a, b, c in poly:
            out[:, k] += (abs(coef) if absolute else coef) * _monomial(v, a, b, c)
    return out


def basis_gradient(u, absolute=False):
    """[m, 16, 3]: d b_k / d (x, y, z), the polynomials differentiated as they stand; absolute: every monomial in absolute value."""
    out = np.zeros((len(u), 16, 3))
    v = np.abs(u) if absolute else u
    for k, poly in enumerate(BASIS):
        for coef, *powers in poly:
            for j in range(3):
                if powers[j]:
                    p = list(powers)
                    p[j] -= 1
                    out[:, k, j] += (abs(coef) if absolute else coef) * powers[j] * _monomial(v, *p)
    return out


# ---- (a) the forward ---------------------------------------------------------------------------------------------------------------------
def sh64(theta, cam, degree):
    """dict(u [m, 3], r [m], b [m, 16] (zero beyond the degree), v [m, 3] before the clamp, m [m, 3] bool the clamp passes, rgb [m, 3],
    band [m, 3] = min(|v|, |v - 1|)) in float64."""
    p, sh = np.asarray(theta["means"], np.float64), np.asarray(theta["sh"], np.float64).reshape(-1, 16, 3)
    d = p - centre_of(cam)
    r = np.sqrt((d * d).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        u = d / r[:, None]
    b = basis(u)
    b[:, coefficients(degree):] = 0.0
    v = np.einsum("mk,mkc->mc", b[:, :coefficients(degree)], sh[:, :coefficients(degree)]) + 0.5
    with np.errstate(invalid="ignore"):
        m = (v >= 0.0) & (v <= 1.0)
        band = np.minimum(np.abs(v), np.abs(v - 1.0))
    return dict(u=u, r=r, b=b, v=v, m=m, rgb=np.clip(v, 0.0, 1.0), band=band)


def near_clamp(theta, cam, degree):
    """[m, 3] bool: the entries within CLAMP_BAND of a clamp edge."""
    return sh64(theta, cam, degree)["band"] <= CLAMP_BAND


def sh_to_rgb_torch(p, sh, cc, degree):
    """sh_to_rgb as one torch statement, clamp included, in the dtype and on the device of its arguments (p [m, 3], sh [m, 16, 3],
    cc [3]): what autograd differentiates in the tests, and in float32 on the GPU what a caller without the operator writes."""
    import torch

    d = p - cc
    u = d / torch.sqrt((d * d).sum(1, keepdim=True))
    x, y, z = u.unbind(1)
    b = [torch.full_like(x, C0), -C1 * y, C1 * z, -C1 * x,
         K2[0] * x * y, K2[1] * y * z, K2[2] * (2 * z * z - x * x - y * y), K2[3] * x * z, K2[4] * (x * x - y * y),
         K3[0] * y * (3 * x * x - y * y), K3[1] * x * y * z, K3[2] * y * (4 * z * z - x * x - y * y),
         K3[3] * z * (2 * z * z - 3 * x * x - 3 * y * y), K3[4] * x * (4 * z * z - x * x - y * y), K3[5] * z * (x * x - y * y),
         K3[6] * x * (x * x - 3 * y * y)]
    K = coefficients(degree)
    v = (torch.stack(b[:K], 1)[:, :, None] * sh[:, :K]).sum(1) + 0.5
    return torch.clamp(v, 0.0, 1.0)


# ---- (b) the transpose and its bound ------------------------------------------------------------------------------------------------------
def _chain(theta, cam, degree, g, absolute):
    fw = sh64(theta, cam, degree)
    K = coefficients(degree)
    sh = np.asarray(theta["sh"], np.float64).reshape(-1, 16, 3)
    g = np.asarray(g, np.float64)[:, :3]
    u, r = fw["u"], fw["r"]
    alive = np.isfinite(u).all(1) if degree > 0 else np.ones(len(r), bool)
    u = np.where(alive[:, None], u, 0.0)
    mg = np.where(fw["m"] & alive[:, None], g, 0.0)
    if absolute:
        mg, sh = np.abs(mg), np.abs(sh)
    b, db = basis(u, absolute), basis_gradient(u, absolute)
    b[:, K:], db[:, K:] = 0.0, 0.0
    g_sh = b[:, :, None] * mg[:, None, :]
    out_means = np.zeros((len(r), 3))
    if degree > 0:
        w = np.einsum("mc,mkc->mk", mg, sh)
        gu = np.einsum("mkj,mk->mj", db, w)
        ua = np.abs(u) if absolute else u
        dot = (gu * ua).sum(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            out_means = (gu + ua * dot[:, None] if absolute else gu - u * dot[:, None]) / r[:, None]
        out_means = np.where(alive[:, None], out_means, 0.0)
    return dict(sh=g_sh, means=out_means)


def vjp64(theta, cam, degree, g):
    """dict(sh [m, 16, 3], means [m, 3]) float64: the transpose of sh_to_rgb applied to g [m, >= 3]."""
    return _chain(theta, cam, degree, g, False)


def bound64(theta, cam, degree, g):
    """The same chain with every factor (each monomial of the basis and of its derivative, the coefficients, u in the projection)
    and the upstream in absolute value: B, per element."""
    return _chain(theta, cam, degree, g, True)


# ---- (c) the kernel's arrangement in float32 ---------------------------------------------------------------------------------------------
def emulate_fp32(theta, cam, degree, g):
    """The gradient as sh_backward.hip forms it, in torch float32 from the scene's float32 arrays: the direction by a divide, the
    basis in the forward's association, w_k = (m g_0 sh_k0 + m g_1 sh_k1) + m g_2 sh_k2, the three sums over k in k order, the
    projection (g - u (u . g)) / r.  The clamp decision is taken on the float32 v."""
    import torch

    f32 = torch.float32
    p = torch.as_tensor(np.asarray(theta["means"]), dtype=f32)
    sh = torch.as_tensor(np.asarray(theta["sh"]), dtype=f32).reshape(-1, 16, 3)
    cc = torch.as_tensor(centre_of(cam), dtype=f32)
    g = torch.as_tensor(np.asarray(g), dtype=f32)[:, :3]
    K = coefficients(degree)
    d = p - cc
    n = torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    x, y, z = d[:, 0] / n, d[:, 1] / n, d[:, 2] / n
    xx, yy, zz = x * x, y * y, z * z
    c1 = np.float32(C1)
    k2, k3 = [np.float32(k) for k in K2], [np.float32(k) for k in K3]
    B = [torch.full_like(x, np.float32(C0)), -c1 * y, c1 * z, -(c1 * x),
         (k2[0] * x) * y, (k2[1] * y) * z, k2[2] * (((2 * z) * z - xx) - yy), (k2[3] * x) * z, k2[4] * (xx - yy),
         (k3[0] * y) * ((3 * x) * x - yy), ((k3[1] * x) * y) * z, (k3[2] * y) * (((4 * z) * z - xx) - yy),
         (k3[3] * z) * (((2 * z) * z - (3 * x) * x) - (3 * y) * y), (k3[4] * x) * (((4 * z) * z - xx) - yy), (k3[5] * z) * (xx - yy),
         (k3[6] * x) * (xx - (3 * y) * y)]
    v = torch.zeros_like(g)
    for k in range(K):
        v = v + B[k][:, None] * sh[:, k]
    v = v + 0.5
    mg = torch.where((v >= 0) & (v <= 1), g, torch.zeros_like(g))
    g_sh = torch.zeros((len(p), 16, 3), dtype=f32)
    for k in range(K):
        g_sh[:, k] = B[k][:, None] * mg
    g_mean = torch.zeros((len(p), 3), dtype=f32)
    if degree > 0:
        w = [(mg[:, 0] * sh[:, k, 0] + mg[:, 1] * sh[:, k, 1]) + mg[:, 2] * sh[:, k, 2] for k in range(16)]
        gx, gy, gz = -(c1 * w[3]), -c1 * w[1], c1 * w[2]
        if degree > 1:
            gx = gx + ((((k2[0] * y) * w[4] - ((2 * k2[2]) * x) * w[6]) + (k2[3] * z) * w[7]) + ((2 * k2[4]) * x) * w[8])
            gy = gy + ((((k2[0] * x) * w[4] + (k2[1] * z) * w[5]) - ((2 * k2[2]) * y) * w[6]) - ((2 * k2[4]) * y) * w[8])
            gz = gz + (((k2[1] * y) * w[5] + ((4 * k2[2]) * z) * w[6]) + (k2[3] * x) * w[7])
        if degree > 2:
            xy, q4 = x * y, (4 * zz - xx) - yy
            gx = gx + (((6 * k3[0]) * xy) * w[9] + ((k3[1] * y) * z) * w[10] - ((2 * k3[2]) * xy) * w[11] - (((6 * k3[3]) * z) * x) * w[12]
                       + (k3[4] * (q4 - 2 * xx)) * w[13] + (((2 * k3[5]) * z) * x) * w[14] + ((3 * k3[6]) * (xx - yy)) * w[15])
            gy = gy + (((3 * k3[0]) * (xx - yy)) * w[9] + ((k3[1] * x) * z) * w[10] + (k3[2] * (q4 - 2 * yy)) * w[11]
                       - (((6 * k3[3]) * z) * y) * w[12] - ((2 * k3[4]) * xy) * w[13] - (((2 * k3[5]) * z) * y) * w[14] - ((6 * k3[6]) * xy) * w[15])
            gz = gz + ((k3[1] * xy) * w[10] + (((8 * k3[2]) * y) * z) * w[11] + (k3[3] * ((6 * zz - 3 * xx) - 3 * yy)) * w[12]
                       + (((8 * k3[4]) * x) * z) * w[13] + (k3[5] * (xx - yy)) * w[14])
        dot = (gx * x + gy * y) + gz * z
        g_mean = torch.stack([(gx - x * dot) / n, (gy - y * dot) / n, (gz - z * dot) / n], 1)
        g_mean = torch.where(torch.isfinite(n)[:, None] & (n > 0)[:, None] & mg.ne(0).any(1)[:, None], g_mean, torch.zeros_like(g_mean))
    return dict(sh=g_sh.numpy().astype(np.float64), means=g_mean.numpy().astype(np.float64), v=v.numpy())


# ---- (d) checks ---------------------------------------------------------------------------------------------------------------------------
def unit_rows(seed, n, cols=3):
    """[n, cols] float32: seeded unit-normal rows on EVERY gaussian (the operator has no cull)."""
    return np.random.default_rng(5000 + seed).standard_normal((n, cols)).astype(np.float32)


def keep_mask(theta, cam, degree):
    """(keep_sh [m, 16, 3], keep_means [m, 3]) bool: the elements a comparison keeps — grad_sh[i][k][c] unless entry (i, c) is on
    the band, grad_means[i] unless any channel of gaussian i is — and how many entries were left out."""
    near = near_clamp(theta, cam, degree)
    keep_sh = np.broadcast_to(~near[:, None, :], (len(near), 16, 3))
    keep_means = np.broadcast_to(~near.any(1)[:, None], (len(near), 3))
    return keep_sh, keep_means, int(near.sum())


def worst_ratios(got, want, bound, keep=None, rel=REL):
    """Per output array: max over its kept elements of |got - want| / (rel bound); 0 / 0 counts as 0."""
    fig = {}
    for k in FIELDS:
        err = np.abs(np.asarray(got[k], np.float64).reshape(want[k].shape) - want[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / (rel * bound[k]))
        if keep is not None:
            r = np.where(keep[k], r, 0.0)
        fig[k] = float(r.max(initial=0.0))
    return fig


def check_colour(tag, got, want, bound, keep=None, rel=REL):
    """|got - want| <= rel bound per kept element of the two arrays.  Prints the worst ratio per array first ("sh ..." lines)."""
    fig = worst_ratios(got, want, bound, keep, rel)
    print(f"\nsh {tag}: worst |err| / ({rel:g} B) " + " ".join(f"{k}={v:.3g}" for k, v in fig.items()), end="")
    for k, v in fig.items():
        assert v <= 1.0, f"{tag}: {k} exceeds {rel:g} B by a factor of {v:.3g}"
    return fig


def as_dict(g):
    """A ColourGradient (device tensors) as a dict of float64 numpy arrays."""
    return {k: getattr(g, k).detach().cpu().numpy().astype(np.float64) for k in FIELDS}


# ---- (e) the clamp's edges at degree 0 -----------------------------------------------------------------------------------------------------
def edge_scene():
    """A degree-0 scene of six gaussians, one channel each of interest (the other two sit at v = 0.5): float32 sh[0] values found
    by a search over neighbouring floats such that fl(fl(c0 s) + 0.5) is exactly 1, the float below 1, a value above 1; exactly 0,
    the smallest value above 0 the sum reaches, a value below 0.  -> (packed arrays, expected pass [6] bool)."""
    f32 = np.float32
    c0 = f32(C0)

    def value(s):
        return f32(f32(c0 * s) + f32(0.5))

    def search(start, want):
        s = f32(start)
        for _ in range(1 << 16):
            v = value(s)
            if want(v):
                return s
            s = np.nextafter(s, f32(np.inf) if v < want.target else f32(-np.inf), dtype=f32)
        raise AssertionError("no float32 found")

    def at(target):
        def want(v):
            return v == target
        want.target = target
        return want

    one, below_one = f32(1.0), np.nextafter(f32(1.0), f32(0.0), dtype=f32)
    s_one = search(0.5 / C0, at(one))
    s_below = search(0.5 / C0, at(below_one))
    s_above = s_one
    while value(s_above) <= one:
        s_above = np.nextafter(s_above, f32(np.inf), dtype=f32)
    s_zero = search(-0.5 / C0, at(f32(0.0)))
    s_inside = s_zero
    while value(s_inside) <= 0:
        s_inside = np.nextafter(s_inside, f32(np.inf), dtype=f32)
    s_under = s_zero
    while value(s_under) >= 0:
        s_under = np.nextafter(s_under, f32(-np.inf), dtype=f32)
    firsts = np.array([s_one, s_below, s_above, s_zero, s_inside, s_under], f32)
    n = len(firsts)
    sh = np.zeros((n, 16, 3), f32)
    sh[:, 0, 0] = firsts
    rng = np.random.default_rng(77)
    packed = dict(means=rng.normal(size=(n, 3)).astype(f32) + f32(3.0), log_scales=np.full((n, 3), -3.0, f32),
                  quats=np.tile(np.array([1, 0, 0, 0], f32), (n, 1)), opacity_logit=np.zeros(n, f32), sh=sh)
    vals = np.array([value(s) for s in firsts])
    assert vals[0] == 1 and vals[1] == below_one and vals[2] > 1 and vals[3] == 0 and vals[4] > 0 and vals[5] < 0
    return {k: np.ascontiguousarray(v) for k, v in packed.items()}, np.array([True, True, False, True, True, False])
