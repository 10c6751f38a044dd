// splat_chain.h — the chain from a row of a view's splat gradient (d L / d opacity, 2-D mean, inverse 2-D covariance, as
// blend_splat_backward.hip leaves them) up to the projection's inputs, stated ONCE for both kernels that walk it: project_backward.hip
// carries it on to the gaussian (mean, log-scales, quaternion), camera_backward.hip to the camera (w2c, full_proj, focal).
// The forward is recomputed by the functions the preprocess itself calls (gauss_math.h), so that the backward linearises the values
// the forward actually used and takes the forward's own decisions (cull, ray clamp, det == 0); the intermediates the chain needs
// (s, the normalised quaternion, M; x / z, y / z, J, T, T cov3d) come out of cov3d_of and ewa_cov2d through their keep-structs.
// Held fixed, as the splat gradient already holds them: the tile rect, the footprint, pthr and the cull.
// Both including files are built with -ffp-contract=off and without fast-math: an expression tree written here gives the same bits
// in either kernel, whatever the scheduler does with it.  The parenthesisation of every expression is part of the contract.
#pragma once
#include <cmath>
#include "gsr_internal.h"
#include "gauss_math.h"

namespace gsr {

// ---- the row.  Columns 6 and 7 are not looked at; returns "touched": a row of six zeros is skipped ----------------------------------
struct SplatRow { float g_op, g_mx, g_my, g_s0, g_s1, g_s2; };

__device__ __forceinline__ bool splat_row(const float4 r0, const float4 r1, SplatRow &g)
{
    g.g_op = r0.x, g.g_mx = r0.y, g.g_my = r0.z, g.g_s0 = r0.w, g.g_s1 = r1.x, g.g_s2 = r1.y;
    return g.g_op != 0.0f || g.g_mx != 0.0f || g.g_my != 0.0f || g.g_s0 != 0.0f || g.g_s1 != 0.0f || g.g_s2 != 0.0f;
}

// ---- the forward, by the functions geometry_one / geometry_view call (gauss_math.h).  Returns "contributes" -------------------------
struct SplatForward {
    float p[3], cm[3], a, b01, b10, c, det_inv;  // the mean, in world and camera space; cov2d incl. the low-pass; 1 / det
    Cov3dKeep k3;                                // (a caller that reads none of it pays for none)
    EwaKeep k2;                                  // (rows 0 and 1 of T and T cov3d are read)
};

__device__ __forceinline__ bool splat_forward(const GsrScene &sc, const Cam &cam, int compat, int64_t i, SplatForward &f)
{
    f.p[0] = sc.means[3 * i], f.p[1] = sc.means[3 * i + 1], f.p[2] = sc.means[3 * i + 2];
    cam_mean(cam.V, f.p, f.cm);
    if (f.cm[2] < GSR_CULL_Z) return false;  // culled: contributes nothing (after its 12-B mean, as in the preprocess)

    const float ls[3] = {sc.log_scales[3 * i], sc.log_scales[3 * i + 1], sc.log_scales[3 * i + 2]};
    const float4 q = reinterpret_cast<const float4 *>(sc.quats)[i];
    float C3[3][3], c2[4];
    cov3d_of(ls, q, C3, &f.k3);
    ewa_cov2d(cam.V, C3, f.cm, cam.fx, cam.fy, cam.limx, cam.limy, c2, &f.k2);
    f.a = c2[0], f.b01 = c2[1], f.b10 = c2[2], f.c = c2[3];
    const float det = cov2d_det(f.a, f.b01, f.b10, f.c);
    if (det == 0.0f) return false;  // (geometry_view goes on with 0 for 1 / det and draws nothing)
    float sx, sy, sxy;
    f.det_inv = conic_of(det, f.a, f.b01, f.c, &sx, &sy, &sxy);
    if (!(fabsf(sx) < INFINITY) || !(fabsf(sy) < INFINITY) || !(fabsf(sxy) < INFINITY)) return false;
    return !(compat && (sx == 0.0f || sy == 0.0f || sxy == 0.0f));  // Q2: the reference's loop never draws it
}

// ---- sigmas <- cov2d: s0 = c / det, s1 = a / det, s2 = -b01 / det, det = a c - b10 b01, the four entries separate inputs.  Every
// entry of the Jacobian in the form without a difference (d s0 / d c = 1 / det - a c / det^2 = -b10 b01 / det^2, ...).
// cov2d = T cov3d T^T + 0.3 I (the low-pass is a constant); cov3d symmetric, so both off-diagonal entries are one function of
// (T, cov3d) and only P = g + g^T enters: d / d cov3d = T^T P T (with its transpose), d / d T = P (T cov3d)
struct CovGrad { float P00, P01, P11; };

__device__ __forceinline__ CovGrad cov2d_grad(const SplatRow &g, const SplatForward &f)
{
    const float a = f.a, b01 = f.b01, b10 = f.b10, c = f.c;
    const float di2 = f.det_inv * f.det_inv, bb = b10 * b01;
    const float ga = di2 * ((-(c * c) * g.g_s0 - bb * g.g_s1) + (b01 * c) * g.g_s2);
    const float gc = di2 * ((-bb * g.g_s0 - (a * a) * g.g_s1) + (b01 * a) * g.g_s2);
    const float gb01 = di2 * (((c * b10) * g.g_s0 + (a * b10) * g.g_s1) - (a * c) * g.g_s2);
    const float gb10 = di2 * (((c * b01) * g.g_s0 + (a * b01) * g.g_s1) - (b01 * b01) * g.g_s2);
    return {2.0f * ga, gb01 + gb10, 2.0f * gc};
}

// ---- the mean-side upstream: d / d T (rows 0 and 1), d / d J's four entries, 1 / z_cam, d / d cam_mean, d / d clip point (its
// columns 0, 1, 3) ---------------------------------------------------------------------------------------------------------------------
struct MeanGrad { float gT[2][3], gJ00, gJ02, gJ11, gJ12, itz, gcm[3], gpt[3]; };

__device__ __forceinline__ void mean_grad(const Cam &cam, const SplatRow &g, const SplatForward &f, const CovGrad &P, MeanGrad &m)
{
    const float *V = cam.V;
    const float (&TV)[3][3] = f.k2.TV;
    const float tz = f.cm[2], J00 = f.k2.J[0][0], J02 = f.k2.J[0][2], J11 = f.k2.J[1][1], J12 = f.k2.J[1][2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        m.gT[0][k] = P.P00 * TV[0][k] + P.P01 * TV[1][k];
        m.gT[1][k] = P.P01 * TV[0][k] + P.P11 * TV[1][k];
    }
    // T = J A^T (A = w2c[:3,:3], row-vector convention: A^T[m][c] = V[4 c + m])
    m.gJ00 = (m.gT[0][0] * V[0] + m.gT[0][1] * V[4]) + m.gT[0][2] * V[8];
    m.gJ02 = (m.gT[0][0] * V[2] + m.gT[0][1] * V[6]) + m.gT[0][2] * V[10];
    m.gJ11 = (m.gT[1][0] * V[1] + m.gT[1][1] * V[5]) + m.gT[1][2] * V[9];
    m.gJ12 = (m.gT[1][0] * V[2] + m.gT[1][1] * V[6]) + m.gT[1][2] * V[10];
    // J <- cam_mean.  J00 = fx / z; J02 = -fx u / z with u = clamp(x / z): inside the clamp u = x / z (d/dx = -fx / z^2,
    // d/dz = -2 J02 / z); where it is active u is the constant +-lim, the derivative in x / z is 0 and tx = +-lim z still gives
    // d/dz = -J02 / z
    const bool in_x = f.k2.txtz > -cam.limx && f.k2.txtz < cam.limx, in_y = f.k2.tytz > -cam.limy && f.k2.tytz < cam.limy;
    m.itz = 1.0f / tz;
    m.gcm[0] = in_x ? -(m.gJ02 * J00) * m.itz : 0.0f;
    m.gcm[1] = in_y ? -(m.gJ12 * J11) * m.itz : 0.0f;
    m.gcm[2] = -(((m.gJ00 * J00 + m.gJ11 * J11) + (in_x ? 2.0f : 1.0f) * (m.gJ02 * J02)) + (in_y ? 2.0f : 1.0f) * (m.gJ12 * J12)) * m.itz;
    // screen_mean <- mean, through full_proj and 1 / (w + 1e-7): mx = ((x_clip p_w + 1) W - 1) / 2
    float pt[4], mx, my;
    clip_point(cam.F, f.p, pt);
    const float p_w = pixel_mean(pt, (float)cam.W, (float)cam.H, &mx, &my), pt0 = pt[0], pt1 = pt[1];
    const float gnx = g.g_mx * (0.5f * (float)cam.W), gny = g.g_my * (0.5f * (float)cam.H);
    m.gpt[0] = gnx * p_w, m.gpt[1] = gny * p_w, m.gpt[2] = -((gnx * pt0 + gny * pt1) * p_w) * p_w;
}

}  // namespace gsr
