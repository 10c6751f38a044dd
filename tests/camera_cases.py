"""What the tests of the camera backward share (test_camera_reference.py on CPU, test_gpu_camera_backward.py on the GPU): the pinned
fuzz cases of backward_cases.py — imported, not restated — with the view-direction rows and the camera's own reference
(tools/camera_reference.py), and the bodies of the checks.  A plain module next to the tests, like backward_cases.py.

Every function takes the `G` of gpu_cases.modules() / namespace() and caches in G.cases under a key that starts with "camera".
"""
import ctypes as C
import os
import re

import numpy as np
import torch

import abi_checks as abi
from backward_cases import (PINNED, ORDERS, _reference_at_project64, dev, fm, pr, project_case, project_rows, projection_inputs, sh_e2e_case, sh_inputs, sh_masked,
                            shr, sr)
from gpu_cases import _tool

cr = _tool("camera_reference")
CAMERAS = [None] + list(fm.CAMERAS)
FD_ROWS = 8


def kernel_constants():
    """(CB_THREADS, CB_MAX_GROUPS) as csrc/camera_backward.hip documents them."""
    src = open(os.path.join(abi.CSRC, "camera_backward.hip")).read()
    return tuple(int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) for name in ("CB_THREADS", "CB_MAX_GROUPS"))


def view_rows_of(seed, n):
    """[n, 3] float32: seeded unit-normal view-direction rows."""
    return np.random.default_rng(7000 + seed).standard_normal((n, 3)).astype(np.float32)


# ---- the float64 reference (CPU) -----------------------------------------------------------------------------------------------------
def camera_inputs(G, seed, order, camera=None):
    """projection_inputs' case (the drawn gaussians in draw order, their unit-normal rows, the oracle's camera) plus unit-normal
    view rows on them; built once and only read."""
    key = ("camera", seed, order, camera)
    if key not in G.cases:
        c = projection_inputs(G, seed, order, camera)
        G.cases[key] = dict(c, view=view_rows_of(seed, len(c["k"])))
    return G.cases[key]


def assert_no_gaussian_on_the_clamp_band(c):
    if len(c["k"]):
        assert not pr.clamp_state(c["drawn"], c["cam"])[1].any(), c["tag"]


def _loss(theta, camd, rows):
    o = pr.project64(theta, camd)
    r = torch.as_tensor(rows, dtype=torch.float64)
    return torch.cat([r[:, :1] * o["opacity"][:, None], r[:, 1:3] * o["screen_means"], r[:, 3:6] * o["sigmas"]], 1)  # [m, 6] terms


def _pack(dV, dF, dfx, dfy):
    return np.concatenate([np.asarray(dV)[:, :3].reshape(-1), np.asarray(dF)[:, cr.FCOLS].reshape(-1), [float(dfx), float(dfy)]])


def check_vjp64_against_autograd(c):
    """Autograd of the monolithic project64 with V, F, fx, fy requiring a gradient: |diff| <= 1e-10 |value| on the 26 sums."""
    if not len(c["k"]):
        return
    per, total = cr.vjp64(c["drawn"], c["cam"], c["rows"])
    _, B = cr.bound64(c["drawn"], c["cam"], c["rows"])
    base = pr.camera_of(c["cam"])
    t = {k: torch.tensor(np.asarray(base[k], np.float64), dtype=torch.float64, requires_grad=True) for k in ("V", "F", "fx", "fy")}
    _loss(c["drawn"], dict(base, **t), c["rows"]).sum().backward()
    auto = _pack(t["V"].grad.numpy(), t["F"].grad.numpy(), t["fx"].grad, t["fy"].grad)
    assert not t["V"].grad[:, 3].any() and not t["F"].grad[:, 2].any()  # the columns the forward never reads
    err = np.abs(auto - total[:26])
    worst = float((err / np.maximum(np.abs(total[:26]), 1e-300)).max())
    print(f"\ncamera autograd {c['tag']}: worst |diff| / |value| {worst:.2e}", end="")
    assert (err <= pr.AUTOGRAD_REL * np.abs(total[:26])).all(), (c["tag"], err, total)
    assert (B[:26] >= np.abs(total[:26]) * (1 - 1e-12)).all() and total[:26].any() and not total[26:].any()
    assert np.array_equal(per.sum(0), total)


def check_vjp64_against_finite_differences(c, own_rounding=False):
    """Central differences of each of eight drawn gaussians' own loss in all 26 camera entries, step FD_STEP max(1, |value|):
    |fd - g| <= FD_REL max over the gaussians of |g| in that entry (splat_reference's rule, the entries as columns).
    own_rounding: plus the differences' own rounding, 2^-53 (|L+| + |L-|) / 2 h — for the one-gaussian pin alone, whose column
    "maximum" is its only entry and itself a sum that cancels (as backward_cases._fd_against allows it there)."""
    if not len(c["k"]):
        return
    per, _ = cr.vjp64(c["drawn"], c["cam"], c["rows"])
    at = sr.fd_rows(c["ref"], np.ones(len(c["k"]), bool))
    base = pr.camera_of(c["cam"])
    theta, rows = pr.rows_of(c["drawn"], at), c["rows"][at]
    entries = [("V", k, j) for k in range(4) for j in range(3)] + [("F", k, j) for k in range(4) for j in cr.FCOLS] + [("fx",), ("fy",)]
    fd, own = np.zeros((len(at), 26)), np.zeros((len(at), 26))
    for s, e in enumerate(entries):
        value = float(base[e[0]][e[1], e[2]]) if len(e) == 3 else float(base[e[0]])
        h = sr.FD_STEP * max(1.0, abs(value))
        side = []
        for sign in (1.0, -1.0):
            d = dict(base, V=np.array(base["V"], np.float64), F=np.array(base["F"], np.float64))
            if len(e) == 3:
                d[e[0]][e[1], e[2]] += sign * h
            else:
                d[e[0]] = value + sign * h
            side.append(_loss(theta, d, rows).numpy())
        fd[:, s] = (side[0] - side[1]).sum(1) / (2.0 * h)  # (the terms are differenced before they are summed)
        own[:, s] = 2.0 ** -53 * (np.abs(side[0]) + np.abs(side[1])).sum(1) / (2.0 * h) if own_rounding else 0.0
    scale = np.abs(per[:, :26]).max(0)
    worst = float((np.abs(fd - per[at, :26]) / np.maximum(scale, 1e-300)).max())
    print(f"\ncamera fd {c['tag']}: rows {len(at)}, worst |fd - g| / max |g column| {worst:.2e}", end="")
    assert (np.abs(fd - per[at, :26]) <= sr.FD_REL * scale + own).all(), (c["tag"], worst)


def check_fp32_emulation_within_the_bound(c):
    """|emulation - vjp64| <= 1e-5 B per entry, from the scene's float32 arrays, view rows included."""
    if not len(c["k"]):
        return None
    _, want = cr.vjp64(c["drawn"], c["cam"], c["rows"], c["view"])
    _, B = cr.bound64(c["drawn"], c["cam"], c["rows"], c["view"])
    _, emu = cr.emulate_fp32(c["drawn"], c["cam"], c["rows"], c["view"])
    _, emu64 = cr.emulate_fp32(c["drawn"], c["cam"], c["rows"], c["view"], dtype=torch.float64)  # a second statement of vjp64
    assert cr.worst_ratio(emu64, want, B, pr.AUTOGRAD_REL)[0] <= 1.0, c["tag"]
    return cr.check_camera(f"emulation {c['tag']}", emu, want, B)


class StructCamera:
    """The GsrCamera fields pose_gradient reads, from any camera that has them (the oracle's is one)."""

    def __init__(self, cam):
        self.w2c, self.full_proj, self.cam_center = list(cam.w2c), list(cam.full_proj), list(cam.cam_center)
        self.focal_x, self.focal_y = float(cam.focal_x), float(cam.focal_y)


def gradient_of(G, total):
    """A CameraGradient of CPU tensors from 29 (or 32) numbers."""
    buf = torch.zeros(32, dtype=torch.float64)
    buf[:len(total)] = torch.as_tensor(np.asarray(total, np.float64))
    return G.renderer._camera_gradient_of(buf)


def check_pose_gradient_against_finite_differences(G, c, s):
    """L(xi, log f) = <rows, project64(theta, camera_at(xi, log f))> + <g, sh_to_rgb at cam_center(xi)>, the camera fields rebuilt in
    float64, differenced centrally in the 6 + 2 parameters (step FD_STEP) against renderer.pose_gradient of vjp64's sums and against
    twist_chain64: |fd - g| <= FD_REL x the chain in absolute values of B."""
    if not len(c["k"]):
        return
    view = shr.vjp64(s["theta"], s["cam"], 3, s["g"])["means"]
    _, total = cr.vjp64(c["drawn"], c["cam"], c["rows"])
    _, B = cr.bound64(c["drawn"], c["cam"], c["rows"])
    total, B = total.copy(), B.copy()
    total[26:29], B[26:29] = -view.sum(0), shr.bound64(s["theta"], s["cam"], 3, s["g"])["means"].sum(0)
    cam = StructCamera(c["cam"])
    twist, logf = G.renderer.pose_gradient(cam, gradient_of(G, total))
    got = np.concatenate([twist.numpy(), logf.numpy()])
    ref = np.concatenate(cr.twist_chain64(c["cam"], total))
    scale = np.concatenate(cr.twist_chain64(c["cam"], B, absolute=True))
    assert (np.abs(got - ref) <= pr.AUTOGRAD_REL * scale).all(), (c["tag"], got, ref)
    p, sh, g = (torch.as_tensor(a, dtype=torch.float64) for a in (s["theta"]["means"], s["theta"]["sh"], s["g"]))

    def value(x):
        d = cr.camera_at(c["cam"], x[:6], x[6:])
        colour = (g * shr.sh_to_rgb_torch(p, sh, torch.as_tensor(d["cc"]), 3)).sum(1).numpy()
        return np.concatenate([_loss(c["drawn"], d, c["rows"]).numpy().reshape(-1), colour])

    fd = np.zeros(8)
    for j in range(8):
        x = np.zeros(8)
        x[j] = sr.FD_STEP
        fd[j] = (value(x) - value(-x)).sum() / (2.0 * sr.FD_STEP)
    worst = float((np.abs(fd - got) / np.maximum(scale, 1e-300)).max())
    print(f"\ncamera pose fd {c['tag']}: worst |fd - g| / chain(B) {worst:.2e}", end="")
    assert (np.abs(fd - got) <= sr.FD_REL * scale).all(), (c["tag"], fd, got, scale)
    assert got.all()


def check_end_to_end_against_finite_differences(G, c, seed):
    """The colour frame's loss with the support frozen, as backward_cases.check_end_to_end_against_finite_differences does it:
    L(xi, log f) = sum_p splat_reference.loss_pixels(ref, project64(theta, camera_at(xi, log f)), F(xi), G, gT) with F(xi) the SH
    colours (degree 3) at cam_center(xi), differenced centrally in the 6 + 2 parameters (the per-pixel losses before they are
    summed) against renderer.pose_gradient of vjp64 of the closed form's rows plus the negated SH view-mean sums:
    |fd - g| <= FD_REL x the chain in absolute values of B, B from |g| + A + B_splat and |g_rgb| + sum_p w |G|.
    -> whether anything was differenced."""
    cam = c["cam"]
    ref = _reference_at_project64(c)
    if not len(ref["kept"]):
        return False
    cc0, n = c["c"], ref["n"]
    theta = shr.theta_of(cc0["packed"])  # file order: what ref["kept"] indexes
    assert shr.keep_mask(theta, cam, 3)[2] == 0  # the SH band leaves out nothing
    Gz, gTz = sr.masked_inputs(ref, fm.upstream_of(seed, cc0["H"], cc0["W"])[0][..., :3], sr.gT_of(seed, cc0["H"], cc0["W"]))
    cf = sr.closed_form(ref, shr.sh64(theta, cam, 3)["rgb"], Gz, gTz)
    if not cf["reached"].any():
        return False
    rows, rowsB = cf["g"][ref["kept"]], (np.abs(cf["g"]) + cf["A"] + cf["B"])[ref["kept"]]  # draw order, as c["drawn"]
    g_rgb = fm.gradient(ref, Gz, n)
    own = fm.gradient(dict(ref, w=np.abs(ref["w"])), np.abs(Gz), n)
    total = cr.vjp64(c["drawn"], cam, rows)[1]
    B = cr.bound64(c["drawn"], cam, rowsB)[1]
    total[26:29] = -shr.vjp64(theta, cam, 3, g_rgb)["means"].sum(0)
    B[26:29] = shr.bound64(theta, cam, 3, np.abs(g_rgb) + own)["means"].sum(0)
    twist, logf = G.renderer.pose_gradient(StructCamera(cam), gradient_of(G, total))
    got = np.concatenate([twist.numpy(), logf.numpy()])
    scale = np.concatenate(cr.twist_chain64(cam, B, absolute=True))
    base = sr.params_of(ref)
    p, sh = (torch.as_tensor(theta[k], dtype=torch.float64) for k in ("means", "sh"))

    def value(x):
        d = cr.camera_at(cam, x[:6], x[6:])
        o = pr.project64(c["drawn"], d)
        F = shr.sh_to_rgb_torch(p, sh, torch.as_tensor(d["cc"]), 3).numpy()
        return sr.loss_pixels(ref, (o["screen_means"].numpy(), o["sigmas"].numpy(), o["opacity"].numpy()), F, Gz, gTz)

    at = sr.loss_pixels(ref, base, shr.sh64(theta, cam, 3)["rgb"], Gz, gTz)
    assert np.allclose(value(np.zeros(8)), at, rtol=1e-9, atol=1e-9 * np.abs(at).max())  # the same point (w2c (w2c^-1 full_proj) rounds)
    fd = np.zeros(8)
    for j in range(8):
        x = np.zeros(8)
        x[j] = sr.FD_STEP
        fd[j] = (value(x) - value(-x)).sum() / (2.0 * sr.FD_STEP)
    worst = float((np.abs(fd - got) / np.maximum(scale, 1e-300)).max())
    print(f"\ncamera end to end fd {c['tag']}: worst |fd - g| / chain(B) {worst:.2e}", end="")
    assert (np.abs(fd - got) <= sr.FD_REL * scale).all(), (c["tag"], fd, got, scale)
    return True


# ---- the kernel (GPU) ------------------------------------------------------------------------------------------------------------------
def raw_camera_backward(G, scene, cam, rows=None, view=None, opts=None):
    """gsr_camera_backward itself -> its [32] doubles as numpy (rows, view: device tensors or None)."""
    lib, r = G.renderer.lib, G.renderer
    ws = torch.empty(int(lib.gsr_camera_backward_bytes(scene.n)), dtype=torch.uint8, device="cuda")
    out = torch.full((32,), float("nan"), dtype=torch.float64, device="cuda")  # WRITTEN, not added into
    sc, o = scene.c_struct(), opts or r.make_options()
    r.check(lib.gsr_camera_backward(C.byref(sc), C.byref(cam), C.byref(o), rows.data_ptr() if rows is not None else None,
                                    view.data_ptr() if view is not None else None, out.data_ptr(), ws.data_ptr(), ws.numel(), None))
    return out.cpu().numpy()


def packed_gradient(cg):
    """A CameraGradient as the kernel's 30 numbers (numpy float64); asserts the never-read columns are zero."""
    w, f = cg.w2c.cpu().numpy(), cg.full_proj.cpu().numpy()
    assert not w[:, 3].any() and not f[:, 2].any()
    return np.concatenate([w[:, :3].reshape(-1), f[:, cr.FCOLS].reshape(-1), cg.focal.cpu().numpy(), cg.cam_center.cpu().numpy(),
                           [float(cg.contributing)]])


def check_operator_parity(G, c):
    """gsr_camera_backward on unit-normal rows (the drawn gaussians) and unit-normal view rows (every gaussian) against vjp64:
    |err| <= 1e-5 B per entry, slot 29 exact, slots 30-31 zero; renderer.camera_backward is the same 30 numbers."""
    rows, view = project_rows(c), view_rows_of(c["seed"], c["n"])
    got = raw_camera_backward(G, c["scene"], c["cam"], dev(rows), dev(view))
    _, want = cr.vjp64(c["theta"], c["ocam"], rows, view)
    _, B = cr.bound64(c["theta"], c["ocam"], rows, view)
    worst = cr.check_camera(f"{c['tag']} kind=operator", got, want, B)
    assert got[29] == cr.contributing(c["theta"], c["ocam"], rows) == len(c["ref"]["kept_in"]) and not got[30:].any()
    hosted = packed_gradient(G.renderer.camera_backward(c["scene"], c["cam"], dev(rows), dev(view)))
    assert np.array_equal(hosted, got[:30])
    return worst
