"""A float64 reference of the camera backward — the splat gradient of a view (d L / d opacity, 2-D mean, inverse 2-D covariance per
gaussian) summed over the gaussians into the gradient with respect to the CAMERA: w2c, full_proj, the two focal lengths, and,
from the view-direction rows the SH colour backward leaves, cam_center — an fp32 emulation of the kernel's arrangement
(csrc/camera_backward.hip), the bound that holds either of them to the reference, and the chain from those raw partials to a twist
and a log-focal step (renderer.pose_gradient).

The stages are projection_reference's (5 cam mean, 6 screen mean, 7 cov2d, 8 conic); this file states their Jacobians with respect
to what the CAMERA puts into them and nothing else — the forward, the conic's Jacobian, the cam-mean Jacobian of stage 7, the
contributes() rule and the kernels' upstream quantities are read from projection_reference, the view-direction rows from
sh_reference:
  5  cm_j = sum_k p_k V[k][j] + V[3][j]                      d / d V[k][j] = p_k, d / d V[3][j] = 1
  6  clip_j = sum_k p_k F[k][j] + F[3][j], j in (0, 1, 3)    d screen / d clip as projection_reference's stage 6, times p_k or 1
  7  T[r][l] = sum_m J[r][m] V[l][m], cov2d = T cov3d T^T    d PC[r][c] / d V[l][m] = J[r][m] TV[c][l] + J[c][m] TV[r][l]
     J[0] = (fx / z, 0, -fx t_x / z^2), J[1] likewise         d J[0] / d fx = (1 / z, 0, -t_x / z^2): linear, lim_x held fixed
The layout of a result is the kernel's (include/gsr.h): [3 k + j] w2c, [12 + 3 k + jj] full_proj columns (0, 1, 3), [24, 25]
focal, [26 .. 28] cam_center; SLOTS = 29 of them are sums.  The depth order, lim_x / lim_y and what project_backward holds fixed
are held fixed.  numpy in and out; torch inside.  Needs nothing from tests/.
"""
import numpy as np
import torch

import projection_reference as pr
import sh_reference as shr

SLOTS = 29
FCOLS = (0, 1, 3)     # the columns of full_proj the forward reads
REL = pr.REL
f64 = torch.float64


def slot_names():
    return ([f"w2c[{k}][{j}]" for k in range(4) for j in range(3)] + [f"full_proj[{k}][{j}]" for k in range(4) for j in FCOLS]
            + ["focal_x", "focal_y"] + [f"cam_center[{k}]" for k in range(3)])


# ---- the stage Jacobians with respect to the camera, and their chain ---------------------------------------------------------------
def camera_jacobians(fw, cam):
    """cam_mean_V [m, 3(j), 12] (d cm_j / d slot 3 k + j), screen_F [m, 2, 12] (d screen / d slot 12 + ..), cov2d_V [m, 4, 12]
    (stage 7 through T, J and cm held), cov2d_f [m, 4, 2] (d cov2d / d fx, fy), float64."""
    c = pr.camera_of(cam)
    m = len(fw["det"])
    p = torch.cat([fw["p"], torch.ones((m, 1), dtype=f64)], 1)  # [m, 4]: p_k, and 1 for the translation row
    jac = {}
    d5 = torch.zeros((m, 3, 4, 3), dtype=f64)
    for j in range(3):
        d5[:, j, :, j] = p
    jac["cam_mean_V"] = d5.reshape(m, 3, 12)
    p_w, clip = fw["p_w"], fw["clip"]
    size = pr._t([c["W"], c["H"]], f64)
    d_clip = torch.zeros((m, 2, 3), dtype=f64)  # d screen_a / d clip_(0, 1, 3)
    for a in range(2):
        d_clip[:, a, a] = 0.5 * size[a] * p_w
        d_clip[:, a, 2] = -0.5 * size[a] * clip[:, a] * p_w * p_w
    jac["screen_F"] = torch.einsum("maj,mk->makj", d_clip, p).reshape(m, 2, 12)
    J, TV = fw["J"], fw["T"] @ fw["vrk"]
    out_rc = ((0, 0), (0, 1), (1, 0), (1, 1))
    d7 = torch.zeros((m, 4, 4, 3), dtype=f64)  # [o, l, mm]; row 3 of w2c does not enter T
    for o, (r, cc) in enumerate(out_rc):
        d7[:, o, :3, :] = TV[:, cc, :, None] * J[:, r, None, :] + TV[:, r, :, None] * J[:, cc, None, :]
    jac["cov2d_V"] = d7.reshape(m, 4, 12)
    tz = fw["cam_means"][:, 2]
    t = fw["u"] * tz[:, None]
    V = pr._t(c["V"], f64)
    d7f = torch.zeros((m, 4, 2), dtype=f64)
    for a in range(2):
        dJ = torch.zeros((m, 2, 3), dtype=f64)
        dJ[:, a, a], dJ[:, a, 2] = 1.0 / tz, -t[:, a] / (tz * tz)
        dT = dJ @ V[:3, :3].T
        for o, (r, cc) in enumerate(out_rc):
            d7f[:, o, a] = (dT[:, r] * TV[:, cc]).sum(1) + (TV[:, r] * dT[:, cc]).sum(1)
    jac["cov2d_f"] = d7f
    return jac


def _forward(theta, cam):
    fw = pr._forward(theta, cam)
    fw["p"] = pr._t(theta["means"], f64)
    return fw


def _chain(fw, cam, rows, absolute):
    g = pr._t(rows, f64)[:, :6]
    stage, mine = pr.stage_jacobians(fw, cam), camera_jacobians(fw, cam)
    if absolute:
        g = g.abs()
        stage, mine = {k: v.abs() for k, v in stage.items()}, {k: v.abs() for k, v in mine.items()}
    g_cov2d = torch.einsum("mos,mo->ms", stage["conic"], g[:, 3:6])          # 8
    g_cam = torch.einsum("moj,mo->mj", stage["cov2d_cam"], g_cov2d)          # 7, through J <- cam mean
    out = torch.zeros((len(g), SLOTS), dtype=f64)
    out[:, 0:12] = torch.einsum("mos,mo->ms", mine["cov2d_V"], g_cov2d) + torch.einsum("mjs,mj->ms", mine["cam_mean_V"], g_cam)  # 7, 5
    out[:, 12:24] = torch.einsum("mas,ma->ms", mine["screen_F"], g[:, 1:3])  # 6
    out[:, 24:26] = torch.einsum("moa,mo->ma", mine["cov2d_f"], g_cov2d)     # 7
    return out


def _view_part(view_rows, m, absolute):
    part = np.zeros((m, SLOTS))
    if view_rows is not None:
        v = np.asarray(view_rows, np.float64)
        part[:, 26:29] = np.abs(v) if absolute else -v  # d = mean - cam_center
    return part


def _contributions(theta, cam, rows, view_rows, compat, absolute):
    m = len(theta["means"])
    per = np.zeros((m, SLOTS))
    if rows is not None and m:
        fw = _forward(theta, cam)
        keep = pr.contributes(fw, compat)
        per = torch.where(keep[:, None], _chain(fw, cam, rows, absolute), torch.zeros((), dtype=f64)).numpy()
    return per + _view_part(view_rows, m, absolute)


@pr._one_thread
def vjp64(theta, cam, rows, view_rows=None, compat=True):
    """(per [m, 29], total [29]) float64: every gaussian's contribution by the explicit stage Jacobians — zero where it contributes
    nothing (projection_reference.contributes) — plus the negated view-direction rows [m, 3], and their sum.  rows [m, >= 6] or None."""
    per = _contributions(theta, cam, rows, view_rows, compat, False)
    return per, per.sum(0)


@pr._one_thread
def bound64(theta, cam, rows, view_rows=None, compat=True):
    """(per [m, 29], B [29]): the same chain with every Jacobian entry and the upstream in absolute value, summed over gaussians."""
    per = _contributions(theta, cam, rows, view_rows, compat, True)
    return per, per.sum(0)


def contributing(theta, cam, rows, compat=True):
    """Slot 29: how many gaussians have a nonzero row (columns 0-5) and pass every exclusion."""
    if not len(theta["means"]):
        return 0
    touched = torch.as_tensor(np.asarray(rows)[:, :6] != 0).any(1)
    return int((touched & pr.contributes(pr._forward(theta, cam), compat)).sum())


@pr._one_thread
def emulate_fp32(theta, cam, rows, view_rows=None, compat=True, dtype=torch.float32):
    """(per [m, 29], total [29]): the kernel's arrangement (camera_backward.hip) per gaussian in torch `dtype` — one term per slot
    from projection_reference.fused_upstream's gT, gJ, gcm, gpt — and the sums in float64."""
    m = len(theta["means"])
    per = np.zeros((m, SLOTS))
    if rows is not None and m:
        c = pr.camera_of(cam)
        fw = pr._forward(theta, cam, dtype)
        up = pr.fused_upstream(fw, cam, rows, dtype)
        p, gT, gJ, gcm, gpt, J = pr._t(theta["means"], dtype), up["gT"], up["gJ"], up["gcm"], up["gpt"], fw["J"]
        out = torch.zeros((m, SLOTS), dtype=dtype)
        for k in range(3):
            out[:, 3 * k + 0] = p[:, k] * gcm[:, 0] + gT[:, 0, k] * J[:, 0, 0]
            out[:, 3 * k + 1] = p[:, k] * gcm[:, 1] + gT[:, 1, k] * J[:, 1, 1]
            out[:, 3 * k + 2] = p[:, k] * gcm[:, 2] + (gT[:, 0, k] * J[:, 0, 2] + gT[:, 1, k] * J[:, 1, 2])
        for jj, j in enumerate(FCOLS):
            for k in range(3):
                out[:, 12 + 3 * k + jj] = p[:, k] * gpt[:, j]
            out[:, 21 + jj] = gpt[:, j]
        out[:, 9:12] = gcm
        tz = fw["cam_means"][:, 2]
        itz, itz2 = 1.0 / tz, 1.0 / (tz * tz)
        t = fw["u"] * tz[:, None]
        out[:, 24] = gJ[:, 0, 0] * itz + gJ[:, 0, 2] * (-t[:, 0] * itz2)
        out[:, 25] = gJ[:, 1, 1] * itz + gJ[:, 1, 2] * (-t[:, 1] * itz2)
        keep = pr.contributes(fw, compat)
        per = torch.where(keep[:, None], out, torch.zeros((), dtype=dtype)).numpy().astype(np.float64)
    per = per + _view_part(None if view_rows is None else np.asarray(view_rows, np.float32 if dtype == torch.float32 else np.float64), m, False)
    return per, per.sum(0)


# ---- raw partials -> twist and log-focal ------------------------------------------------------------------------------------------
def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def rotation_of(w):
    """exp([w]x) by Rodrigues' formula, float64."""
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    K = skew(w)
    if th < 1e-12:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / (th * th) * K @ K


def camera_at(cam, twist=np.zeros(6), log_focal=np.zeros(2)):
    """The camera moved rigidly in its own frame by the twist (omega, v) — x_cam' = exp([omega]x) x_cam + v — and its focal lengths
    scaled by exp(log_focal), as the dict projection_reference.camera_of makes plus cc (the camera centre), in float64 from the
    struct's own values: w2c' = w2c E, full_proj' = w2c' (w2c^-1 full_proj) with columns 0 / 1 scaled, cam_center' =
    inverse(w2c')[3, :3].  lim_x / lim_y stay."""
    c = dict(pr.camera_of(cam))
    cc0 = shr.centre_of(cam["cc"] if isinstance(cam, dict) else cam)
    twist, log_focal = np.asarray(twist, np.float64), np.asarray(log_focal, np.float64)
    E = np.eye(4)
    E[:3, :3], E[3, :3] = rotation_of(twist[:3]).T, twist[3:]
    V0, F0 = np.asarray(c["V"], np.float64), np.asarray(c["F"], np.float64)
    V = V0 @ E
    F = V @ (np.linalg.inv(V0) @ F0)
    s = np.exp(log_focal)
    F[:, 0], F[:, 1] = F[:, 0] * s[0], F[:, 1] * s[1]
    # (the struct's centre is inverse(w2c)[3, :3] rounded to fp32: the motion is applied to the struct's own value)
    c.update(V=V, F=F, fx=c["fx"] * s[0], fy=c["fy"] * s[1], cc=cc0 + (np.linalg.inv(V)[3, :3] - np.linalg.inv(V0)[3, :3]))
    return c


def unpack(total):
    """The 29 (or 32) numbers as (dV [4, 4], dF [4, 4], dfocal [2], dcc [3]); the entries the forward never reads are 0."""
    t = np.asarray(total, np.float64)
    dV, dF = np.zeros((4, 4)), np.zeros((4, 4))
    dV[:, :3] = t[0:12].reshape(4, 3)
    dF[:, FCOLS] = t[12:24].reshape(4, 3)
    return dV, dF, t[24:26].copy(), t[26:29].copy()


def twist_chain64(cam, total, absolute=False):
    """(twist [6] = (omega, v), log_focal [2]) float64: the raw partials chained to a rigid motion of the camera in its own frame
    and to the logs of the focal lengths, at zero motion (camera_at's parameterisation).  absolute: every factor and every partial
    in absolute value — the bound of the chain's result when `total` is the bound of the partials."""
    c = pr.camera_of(cam)
    V, F = np.asarray(c["V"], np.float64), np.asarray(c["F"], np.float64)
    dV, dF, dfoc, dcc = unpack(total)
    Vinv = np.linalg.inv(V)
    Pm = Vinv @ F
    ab = np.abs if absolute else (lambda x: x)
    # d L / d E at E = I: V' = V E, F' = V E Pm, cc' = (E^-1 V^-1)[3, :3] -> d cc = -(dE V^-1)[3, :3]
    GE = ab(V).T @ ab(dV) + ab(V).T @ ab(dF) @ ab(Pm).T
    g_v = GE[3, :3] + (ab(Vinv[:3, :3]) @ ab(dcc) if absolute else -(Vinv[:3, :3] @ dcc))
    g_w = np.zeros(3)
    for k in range(3):
        dE = -skew(np.eye(3)[k])  # E[:3, :3] = exp([omega]x)^T
        g_w[k] = (GE[:3, :3] * ab(dE)).sum()
    g_f = np.array([ab(c["fx"]) * ab(dfoc[0]) + (ab(F[:, 0]) * ab(dF[:, 0])).sum(), ab(c["fy"]) * ab(dfoc[1]) + (ab(F[:, 1]) * ab(dF[:, 1])).sum()])
    return np.concatenate([g_w, g_v]), g_f


# ---- checks -----------------------------------------------------------------------------------------------------------------------------
def worst_ratio(got, want, bound, rel=REL):
    """max over the 29 entries of |got - want| / (rel bound); 0 / 0 counts as 0."""
    err = np.abs(np.asarray(got, np.float64)[:SLOTS] - np.asarray(want)[:SLOTS])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / (rel * np.asarray(bound)[:SLOTS]))
    return float(r.max(initial=0.0)), int(np.argmax(r))


def check_camera(tag, got, want, bound, rel=REL):
    """|got - want| <= rel bound per entry.  Prints the worst ratio first ("camera ..." lines)."""
    worst, at = worst_ratio(got, want, bound, rel)
    print(f"\ncamera {tag}: worst |err| / ({rel:g} B) {worst:.3g} at {slot_names()[at]}", end="")
    assert worst <= 1.0, f"{tag}: {slot_names()[at]} exceeds {rel:g} B by a factor of {worst:.3g}"
    return worst
