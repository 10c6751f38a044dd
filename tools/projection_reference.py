"""A float64 reference of the projection backward — the splat gradient of a view (d L / d opacity, 2-D mean, inverse 2-D covariance
per gaussian) chained through the preprocess' projection to what the scene stores: mean, log-scales, quaternion, opacity logit —
an fp32 emulation of the kernel's arithmetic, the bound that holds either of them to the reference, and the checks
tests/test_gpu_project_backward.py calls.

The projection as eight explicit stages (csrc/preprocess.hip, gauss_math.h; quirks as there: +tvec in w2c's last row, stored
quaternions not normalised, the Q3 focal, the 1.3 tan(fov / 2) ray clamp, + 1e-7 in the perspective divide, the 0.3 low-pass, the
b10 b01 determinant):
  1 normalise   n = q / max(|q|, 1e-12)                 5 cam mean     cm = p A + t  (row-vector convention)
  2 R           quat_to_rot(n), n = (w, x, y, z)         6 screen mean  through full_proj, 1 / (w + 1e-7), NDC -> pixel
  3 M           R diag(exp(log_scales))                  7 cov2d        T cov3d T^T + 0.3 I, T = J A^T: (a, b01, b10, c)
  4 cov3d       M M^T (its upper triangle is what 7 reads)  8 conic     (c, a, -b01) / det, det = a c - b10 b01
and a ninth, scalar one: opacity = sigmoid(logit).

project64 evaluates them (torch, so that autograd can differentiate the monolithic statement); vjp64 chains the explicit stage
Jacobians, transposed, last to first; bound64 is the SAME chain with every Jacobian entry replaced by its absolute value and the
upstream by |g|: the componentwise magnitude B a first-order forward-error analysis works at, so that an fp32 evaluation is held to
|err| <= 1e-5 B per element.  B must be built from these stages: a Jacobian of several of them lumped together cancels inside the
lump, and its absolute value no longer covers what an fp32 evaluation of the single stages does.  emulate_fp32 is the kernel's own arrangement of the chain
(project_backward.hip: fused products instead of stored Jacobians) in float32; the same function in float64 is a second,
independent statement of vjp64.

Held fixed, as the splat gradient holds it: the tile rect, the footprint, the 1/255 threshold and the cull.  Where the ray clamp is
active the derivative in x / z is 0 and t_x = +-lim z still depends on z.  A gaussian contributes nothing when z_cam < 0.2, when
det = 0, when a conic entry is not finite, or (reference_compat) when a conic entry is 0.

Rows are [m, 8] (or [m, 6]) in the order of theta: opacity, mean x, mean y, s0, s1, s2.  theta: dict(means [m, 3], log_scales
[m, 3], quats [m, 4], opacity_logit [m]).  cam: anything with the fields of GsrCamera (the oracle's camera is one).  numpy in and
out; torch inside.  Needs nothing from tests/.
"""
import functools

import numpy as np
import torch

FIELDS = ("means", "log_scales", "quats", "opacity_logit")
REL = 1e-5            # the project's standing bar (splat_reference.REL)
ORACLE_REL = 1e-5     # project64 against the fp32 oracle: of max(|value|, the column's largest |value|)
AUTOGRAD_REL = 1e-10
CLAMP_BAND = 1e-4     # ||x / z| / lim - 1| at or below this on either axis: fp32 may decide the clamp the other way; left out
CULL_Z = 0.2
LOWPASS = 0.3
NRM_FLOOR = 1e-12
f64 = torch.float64


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def theta_of(packed, perm=None):
    """The four arrays of a packed scene as float64, in the order `perm` (scene index -> file index; None: the file's)."""
    t = {k: np.asarray(packed[k], np.float64) for k in FIELDS}
    return t if perm is None else {k: v[np.asarray(perm, np.int64)] for k, v in t.items()}


def rows_of(theta, idx):
    return {k: v[idx] for k, v in theta.items()}


def camera_of(cam):
    """dict(V [4, 4], F [4, 4], fx, fy, limx, limy, W, H) of a GsrCamera-like struct (the fp32 values, as float64)."""
    if isinstance(cam, dict):
        return cam
    return dict(V=np.array(list(cam.w2c), np.float64).reshape(4, 4), F=np.array(list(cam.full_proj), np.float64).reshape(4, 4),
                fx=float(cam.focal_x), fy=float(cam.focal_y), limx=float(cam.lim_x), limy=float(cam.lim_y),
                W=int(cam.width), H=int(cam.height))


def _one_thread(fn):
    """Run fn with torch's CPU thread pool at one thread (and put the setting back): every op here is a small batched one, and a
    process whose pool was sized for a whole machine (rasterize.py's drop-in does that) otherwise spends seconds in its wake-ups."""
    @functools.wraps(fn)
    def run(*args, **kw):
        before = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            return fn(*args, **kw)
        finally:
            torch.set_num_threads(before)
    return run


def _t(a, dtype, device=None):
    return a.to(dtype) if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a), dtype=dtype, device=device)


# ---- (a) the forward: eight stages and the sigmoid ----------------------------------------------------------------------------------------
def quat_to_rot(n):
    w, x, y, z = n[:, 0], n[:, 1], n[:, 2], n[:, 3]
    return torch.stack([1 - 2 * (y * y) - 2 * (z * z), 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w,
                        2 * x * y + 2 * z * w, 1 - 2 * (x * x) - 2 * (z * z), 2 * y * z - 2 * x * w,
                        2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w, 1 - 2 * (x * x) - 2 * (y * y)], 1).reshape(-1, 3, 3)


@_one_thread
def project64(theta, cam, dtype=f64, device=None):
    """Every stage's output for the gaussians of theta (torch tensors of `dtype`; theta's entries may be tensors that require a
    gradient, and with `device` tensors on that device: the float32 restatement a caller of the library would write): n, R, s, M,
    cov3d, cam_means, clip, p_w, screen_means, u, J, T, cov2d [m, 4] = (a, b01, b10, c), det, sigmas, opacity."""
    c = camera_of(cam)
    V, F = _t(c["V"], dtype, device), _t(c["F"], dtype, device)
    p, ls, q, x = (_t(theta[k], dtype, device) for k in FIELDS)
    o = {}
    o["nrm"] = torch.sqrt((q * q).sum(1)).clamp(min=NRM_FLOOR)                                   # 1
    o["n"] = q / o["nrm"][:, None]
    o["R"] = quat_to_rot(o["n"])                                                                 # 2
    o["s"] = torch.exp(ls)
    o["M"] = o["R"] * o["s"][:, None, :]                                                         # 3
    o["cov3d"] = o["M"] @ o["M"].transpose(1, 2)                                                 # 4
    o["cam_means"] = p @ V[:3, :3] + V[3, :3]                                                    # 5
    o["clip"] = p @ F[:3] + F[3]                                                                 # 6
    o["p_w"] = 1.0 / (o["clip"][:, 3] + 1e-7)
    ndc = o["clip"][:, :2] * o["p_w"][:, None]
    size = _t([c["W"], c["H"]], dtype, device)
    o["screen_means"] = ((ndc + 1.0) * size - 1.0) / 2.0
    cm = o["cam_means"]                                                                          # 7
    tz = cm[:, 2]
    lim = _t([c["limx"], c["limy"]], dtype, device)
    o["ratio"] = cm[:, :2] / tz[:, None]
    o["u"] = torch.minimum(lim, torch.maximum(-lim, o["ratio"]))  # zero gradient where the clamp is active
    t = o["u"] * tz[:, None]
    J = torch.zeros((len(tz), 2, 3), dtype=dtype, device=device)
    J[:, 0, 0], J[:, 1, 1] = c["fx"] / tz, c["fy"] / tz
    J[:, 0, 2], J[:, 1, 2] = -(c["fx"] * t[:, 0]) / (tz * tz), -(c["fy"] * t[:, 1]) / (tz * tz)
    o["J"] = J
    o["T"] = J @ V[:3, :3].T                                     # T[r][k] = sum_m J[r][m] V[k][m]
    iu = torch.triu_indices(3, 3, device=device)
    vrk = torch.zeros_like(o["cov3d"])
    vrk[:, iu[0], iu[1]] = o["cov3d"][:, iu[0], iu[1]]           # the upper triangle, mirrored
    vrk = vrk + torch.triu(vrk, 1).transpose(1, 2)
    o["vrk"] = vrk
    PC = o["T"] @ vrk @ o["T"].transpose(1, 2)
    o["cov2d"] = torch.stack([PC[:, 0, 0] + LOWPASS, PC[:, 0, 1], PC[:, 1, 0], PC[:, 1, 1] + LOWPASS], 1)
    a, b01, b10, cc = o["cov2d"].unbind(1)                                                       # 8
    o["det"] = a * cc - b10 * b01
    o["sigmas"] = torch.stack([cc / o["det"], a / o["det"], -b01 / o["det"]], 1)
    o["opacity"] = torch.sigmoid(x)                                                              # 9
    return o


def contributes(fw, compat=True):
    """[m] bool: the gaussians whose rows the backward carries (torch, from a forward)."""
    sg = fw["sigmas"]
    ok = (fw["cam_means"][:, 2] >= CULL_Z) & (fw["det"] != 0) & torch.isfinite(sg).all(1)
    return ok & (sg != 0).all(1) if compat else ok


@_one_thread
def clamp_state(theta, cam):
    """(active [m, 2] bool: the ray clamp is active on the axis; near [m] bool: within CLAMP_BAND of its edge on either axis)."""
    fw, c = project64(theta, cam), camera_of(cam)
    lim = np.array([c["limx"], c["limy"]])
    r = np.abs(fw["ratio"].numpy())
    return r > lim, (np.abs(r / lim - 1.0) <= CLAMP_BAND).any(1)


# ---- (b), (c) the stage Jacobians and their chain ------------------------------------------------------------------------------------------
UPPER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # stage 4's outputs: what stage 7 reads of cov3d


def stage_jacobians(fw, cam):
    """The explicit Jacobian of every stage at the forward `fw` (float64): normalise [m, 4, 4], R [m, 9, 4], M_R [m, 3] (the
    diagonal d M_ij / d R_ij = s_j), M_ls [m, 3, 3] (d M_ij / d log_scale_j = M_ij), cov3d [m, 6, 3, 3], cam_mean [3, 3],
    screen [m, 2, 3], cov2d_cov3d [m, 4, 6], cov2d_cam [m, 4, 3], conic [m, 3, 4], sigmoid [m]."""
    c = camera_of(cam)
    V, F = _t(c["V"], f64), _t(c["F"], f64)
    m = len(fw["nrm"])
    jac = {}
    n, nrm = fw["n"], fw["nrm"]
    eye = torch.eye(4, dtype=f64)
    floor = (nrm <= NRM_FLOOR)[:, None, None]
    jac["normalise"] = torch.where(floor, eye / NRM_FLOOR, (eye - n[:, :, None] * n[:, None, :]) / nrm[:, None, None])
    w, x, y, z = n.unbind(1)
    zero = torch.zeros_like(w)
    rows = [[zero, zero, -4 * y, -4 * z], [-2 * z, 2 * y, 2 * x, -2 * w], [2 * y, 2 * z, 2 * w, 2 * x],
            [2 * z, 2 * y, 2 * x, 2 * w], [zero, -4 * x, zero, -4 * z], [-2 * x, -2 * w, 2 * z, 2 * y],
            [-2 * y, 2 * z, -2 * w, 2 * x], [2 * x, 2 * w, 2 * z, 2 * y], [zero, -4 * x, -4 * y, zero]]
    jac["R"] = torch.stack([torch.stack(r, 1) for r in rows], 1)
    jac["M_R"], jac["M_ls"] = fw["s"], fw["M"]
    M = fw["M"]
    d4 = torch.zeros((m, 6, 3, 3), dtype=f64)  # d C_ij / d M_ab = delta_ia M_jb + delta_ja M_ib
    for k, (i, j) in enumerate(UPPER):
        d4[:, k, i, :] += M[:, j, :]
        d4[:, k, j, :] += M[:, i, :]
    jac["cov3d"] = d4
    jac["cam_mean"] = V[:3, :3].T.clone()  # d cm_j / d p_i = V[i][j]: [j, i]
    p_w, clip = fw["p_w"], fw["clip"]
    size = _t([c["W"], c["H"]], f64)
    jac["screen"] = 0.5 * size[None, :, None] * (F[:3, :2].T[None] * p_w[:, None, None]
                                                 - (clip[:, :2] * (p_w * p_w)[:, None])[:, :, None] * F[:3, 3][None, None, :])
    T, vrk = fw["T"], fw["vrk"]
    out_rc = ((0, 0), (0, 1), (1, 0), (1, 1))
    d7 = torch.zeros((m, 4, 6), dtype=f64)
    for o, (r, cc) in enumerate(out_rc):
        for k, (i, j) in enumerate(UPPER):
            d7[:, o, k] = T[:, r, i] * T[:, cc, j] + (T[:, r, j] * T[:, cc, i] if i != j else 0.0)
    jac["cov2d_cov3d"] = d7
    cm = fw["cam_means"]
    tz = cm[:, 2]
    lim = _t([c["limx"], c["limy"]], f64)
    inside = (fw["ratio"] > -lim) & (fw["ratio"] < lim)
    foc = _t([c["fx"], c["fy"]], f64)
    dJ = torch.zeros((m, 2, 3, 3), dtype=f64)  # d J[r][k] / d cm_j
    for r in range(2):
        dJ[:, r, r, 2] = -foc[r] / (tz * tz)
        dJ[:, r, 2, r] = torch.where(inside[:, r], -foc[r] / (tz * tz), zero)
        dJ[:, r, 2, 2] = torch.where(inside[:, r], 2.0 * foc[r] * cm[:, r] / tz ** 3, foc[r] * fw["u"][:, r] / (tz * tz))
    dT = torch.einsum("mrkj,lk->mrlj", dJ, V[:3, :3])  # d T[r][l] / d cm_j, T[r][l] = sum_k J[r][k] V[l][k]
    TV = T @ vrk
    d7c = torch.zeros((m, 4, 3), dtype=f64)
    for o, (r, cc) in enumerate(out_rc):
        d7c[:, o] = torch.einsum("mlj,ml->mj", dT[:, r], TV[:, cc]) + torch.einsum("ml,mlj->mj", TV[:, r], dT[:, cc])
    jac["cov2d_cam"] = d7c
    a, b01, b10, cc = fw["cov2d"].unbind(1)
    di2 = 1.0 / (fw["det"] * fw["det"])
    bb = b10 * b01  # every entry in the form without a difference: d s0 / d c = 1 / det - a c / det^2 = -b10 b01 / det^2
    jac["conic"] = di2[:, None, None] * torch.stack([
        torch.stack([-cc * cc, cc * b10, cc * b01, -bb], 1),
        torch.stack([-bb, a * b10, a * b01, -a * a], 1),
        torch.stack([b01 * cc, -a * cc, -b01 * b01, b01 * a], 1)], 1)
    jac["sigmoid"] = fw["opacity"] * torch.sigmoid(-_t(fw["logit"], f64))
    return jac


def _chain(jac, rows, absolute):
    """The transposed stage Jacobians applied last to first to rows [m, >= 6]; absolute: |J| and |g| throughout."""
    g = _t(rows, f64)[:, :6]
    if absolute:
        g = g.abs()
        jac = {k: v.abs() for k, v in jac.items()}
    g_cov2d = torch.einsum("mos,mo->ms", jac["conic"], g[:, 3:6])                                                # 8
    g_cov3d = torch.einsum("mok,mo->mk", jac["cov2d_cov3d"], g_cov2d)                                            # 7
    g_cam = torch.einsum("moj,mo->mj", jac["cov2d_cam"], g_cov2d)
    g_mean = torch.einsum("ji,mj->mi", jac["cam_mean"], g_cam) + torch.einsum("moi,mo->mi", jac["screen"], g[:, 1:3])  # 5, 6
    g_M = torch.einsum("mkab,mk->mab", jac["cov3d"], g_cov3d)                                                    # 4
    g_ls = (g_M * jac["M_ls"]).sum(1)                                                                            # 3
    g_R = (g_M * jac["M_R"][:, None, :]).reshape(-1, 9)
    g_n = torch.einsum("mkq,mk->mq", jac["R"], g_R)                                                              # 2
    g_q = torch.einsum("mab,ma->mb", jac["normalise"], g_n)                                                      # 1
    return dict(means=g_mean, log_scales=g_ls, quats=g_q, opacity_logit=jac["sigmoid"] * g[:, 0])                # 9


def _masked(out, keep):
    return {k: torch.where(keep.reshape((-1,) + (1,) * (v.dim() - 1)), v, torch.zeros_like(v)).numpy() for k, v in out.items()}


def _forward(theta, cam, dtype=f64):
    fw = project64(theta, cam, dtype)
    fw["logit"] = _t(theta["opacity_logit"], dtype)
    return fw


@_one_thread
def vjp64(theta, cam, rows, compat=True):
    """dict(means [m, 3], log_scales [m, 3], quats [m, 4], opacity_logit [m]) float64: the stage-by-stage vector-Jacobian
    product of rows [m, >= 6]; zero for the gaussians that contribute nothing."""
    fw = _forward(theta, cam)
    return _masked(_chain(stage_jacobians(fw, cam), rows, False), contributes(fw, compat))


@_one_thread
def bound64(theta, cam, rows, compat=True):
    """The same chain with every stage's Jacobian replaced by its absolute value and the upstream by |rows|: B, per element."""
    fw = _forward(theta, cam)
    return _masked(_chain(stage_jacobians(fw, cam), rows, True), contributes(fw, compat))


# ---- (d) the kernel's arrangement of the chain ------------------------------------------------------------------------------------------
MUTANTS = ("fx_for_fy", "w2c20_dropped", "limx_for_limy")


def fused_upstream(fw, cam, rows, dtype=torch.float32, mutant=None):
    """The upstream quantities of the kernels' fused chain at the forward `fw`, in `dtype` (csrc/splat_chain.h forms them, for
    project_backward.hip on the way to the mean and camera_backward.hip on the way to the camera, as tools/camera_reference.py reads
    them here): P = g + g^T of the
    2x2, gT [m, 2, 3] = P (T cov3d), gJ [m, 2, 3] = gT A, gcm [m, 3], gpt [m, 4] (column 2 zero), inside [m, 2] (the ray clamp is
    not active), with V, F, A = w2c[:3, :3] (the mutant's, if any), g_op and a zero column."""
    assert mutant is None or mutant in MUTANTS
    c = camera_of(cam)
    V, F = _t(c["V"], dtype), _t(c["F"], dtype)
    g = _t(rows, dtype)[:, :6]
    g_op, g_mx, g_my, g0, g1, g2 = g.unbind(1)
    a, b01, b10, cc = fw["cov2d"].unbind(1)
    di = 1.0 / fw["det"]
    di2, bb = di * di, b10 * b01
    ga = di2 * ((-(cc * cc) * g0 - bb * g1) + (b01 * cc) * g2)
    gc = di2 * ((-bb * g0 - (a * a) * g1) + (b01 * a) * g2)
    gb01 = di2 * (((cc * b10) * g0 + (a * b10) * g1) - (a * cc) * g2)
    gb10 = di2 * (((cc * b01) * g0 + (a * b01) * g1) - (b01 * b01) * g2)
    P = torch.stack([2 * ga, gb01 + gb10, gb01 + gb10, 2 * gc], 1).reshape(-1, 2, 2)
    gT = P @ (fw["T"] @ fw["vrk"])
    A = V[:3, :3]                              # T[r][k] = sum_m J[r][m] A[k][m]
    if mutant == "w2c20_dropped":
        A = A.clone()
        A[2, 0] = 0.0
    gJ = gT @ A                                # gJ[r][m] = sum_k gT[r][k] A[k][m]
    cm = fw["cam_means"]
    tz = cm[:, 2]
    itz = 1.0 / tz
    lim = _t([c["limx"], c["limx" if mutant == "limx_for_limy" else "limy"]], dtype)
    inside = (fw["ratio"] > -lim) & (fw["ratio"] < lim)
    J = fw["J"]
    zero = torch.zeros_like(tz)
    gcm0 = torch.where(inside[:, 0], -(gJ[:, 0, 2] * J[:, 0, 0]) * itz, zero)
    J11 = J[:, 0, 0] if mutant == "fx_for_fy" else J[:, 1, 1]
    gcm1 = torch.where(inside[:, 1], -(gJ[:, 1, 2] * J11) * itz, zero)
    kx, ky = 1.0 + inside[:, 0].to(dtype), 1.0 + inside[:, 1].to(dtype)
    gcm2 = -(((gJ[:, 0, 0] * J[:, 0, 0] + gJ[:, 1, 1] * J[:, 1, 1]) + kx * (gJ[:, 0, 2] * J[:, 0, 2])) + ky * (gJ[:, 1, 2] * J[:, 1, 2])) * itz
    gcm = torch.stack([gcm0, gcm1, gcm2], 1)
    clip, p_w = fw["clip"], fw["p_w"]
    gnx, gny = g_mx * (0.5 * c["W"]), g_my * (0.5 * c["H"])
    gpt = torch.stack([gnx * p_w, gny * p_w, zero, -((gnx * clip[:, 0] + gny * clip[:, 1]) * p_w) * p_w], 1)
    return dict(V=V, F=F, A=A, P=P, gT=gT, gJ=gJ, gcm=gcm, gpt=gpt, inside=inside, g_op=g_op, zero=zero)


@_one_thread
def fused_vjp(theta, cam, rows, dtype=torch.float32, compat=True, mutant=None):
    """The chain as project_backward.hip forms it — P = g + g^T of the 2x2, S = T^T P T, S M, the closed quaternion sums, no stored
    Jacobian — in `dtype`.  float32: the emulation (torch's exp and its order inside a matrix product are not the device's);
    float64: a second statement of vjp64.

    mutant (tests/test_camera_variants.py only; nothing that faces the kernel passes it): one of MUTANTS, a one-token slip of the
    hand-indexed backward — d cm_y takes J00 (fx) for J11 (fy); the backward's copy of w2c has its [2][0] entry (V[8]) at zero; the
    y clamp is decided against lim_x.  The forward it is taken at stays the true one."""
    fw = _forward(theta, cam, dtype)
    up = fused_upstream(fw, cam, rows, dtype, mutant)
    F, A, P, gcm, gpt, g_op, zero = up["F"], up["A"], up["P"], up["gcm"], up["gpt"], up["g_op"], up["zero"]
    T, M, s = fw["T"], fw["M"], fw["s"]
    g_mean = gcm @ A.T + gpt @ F[:3].T
    S = T.transpose(1, 2) @ (P @ T)
    gM = S @ M
    g_ls = (gM * M).sum(1)
    gR = gM * s[:, None, :]
    w, x, y, z = fw["n"].unbind(1)
    r = lambda i, j: gR[:, i, j]
    gw = 2 * ((z * (r(1, 0) - r(0, 1)) + y * (r(0, 2) - r(2, 0))) + x * (r(2, 1) - r(1, 2)))
    gx = 2 * (((y * (r(0, 1) + r(1, 0)) + z * (r(0, 2) + r(2, 0))) + w * (r(2, 1) - r(1, 2))) - 2 * x * (r(1, 1) + r(2, 2)))
    gy = 2 * (((x * (r(0, 1) + r(1, 0)) + z * (r(1, 2) + r(2, 1))) + w * (r(0, 2) - r(2, 0))) - 2 * y * (r(0, 0) + r(2, 2)))
    gz = 2 * (((x * (r(0, 2) + r(2, 0)) + y * (r(1, 2) + r(2, 1))) + w * (r(1, 0) - r(0, 1))) - 2 * z * (r(0, 0) + r(1, 1)))
    gn = torch.stack([gw, gx, gy, gz], 1)
    dot = torch.where(fw["nrm"] <= NRM_FLOOR, zero, (gn * fw["n"]).sum(1))
    g_q = (gn - fw["n"] * dot[:, None]) / fw["nrm"][:, None]
    xl = fw["logit"]
    g_logit = g_op * ((1.0 / (1.0 + torch.exp(-xl))) * (1.0 / (1.0 + torch.exp(xl))))
    out = dict(means=g_mean, log_scales=g_ls, quats=g_q, opacity_logit=g_logit)
    return {k: v.astype(np.float64) for k, v in _masked(out, contributes(fw, compat)).items()}


def emulate_fp32(theta, cam, rows, compat=True):
    return fused_vjp(theta, cam, rows, torch.float32, compat)


# ---- (e) checks ---------------------------------------------------------------------------------------------------------------------------
def unit_rows(seed, n, idx):
    """[n, 8] float32: seeded unit-normal rows on the gaussians `idx`, zero elsewhere."""
    rows = np.zeros((n, 8), np.float32)
    rows[idx] = np.random.default_rng(4000 + seed).standard_normal((len(idx), 8)).astype(np.float32)
    return rows


def worst_ratios(got, want, bound, rel=REL):
    """Per output array: max over its elements of |got - want| / (rel bound); 0 / 0 counts as 0."""
    fig = {}
    for k in FIELDS:
        err = np.abs(np.asarray(got[k], np.float64) - want[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / (rel * bound[k]))
        fig[k] = float(r.max(initial=0.0))
    return fig


def check_geometry(tag, got, want, bound, rel=REL):
    """|got - want| <= rel bound per element of the four arrays.  Prints the worst ratio per array first ("project ..." lines)."""
    fig = worst_ratios(got, want, bound, rel)
    print(f"\nproject {tag}: worst |err| / ({rel:g} B) " + " ".join(f"{k}={v:.3g}" for k, v in fig.items()), end="")
    for k, v in fig.items():
        assert v <= 1.0, f"{tag}: {k} exceeds {rel:g} B by a factor of {v:.3g}"
    return fig


def sum_bounds(*bounds):
    return {k: sum(b[k] for b in bounds) for k in FIELDS}


def as_dict(g):
    """A GeometryGradient (device tensors) as a dict of float64 numpy arrays."""
    return {k: getattr(g, k).detach().cpu().numpy().astype(np.float64) for k in FIELDS}
