// project_backward.hip — the transpose of stage 1's geometry: the splat gradient of a view (row i of grad_splat: d L / d opacity,
// 2-D mean, inverse 2-D covariance, as blend_splat_backward.hip leaves them) chained to what the scene stores — mean, log-scales,
// quaternion, opacity logit.  project_backward_kernel: one thread per gaussian, no LDS, no atomics (a gaussian belongs to one thread).
//
// Built with -ffp-contract=off, like preprocess.hip: the forward is recomputed here by the functions the preprocess itself calls
// (gauss_math.h: cam_mean, cov3d_of, ewa_cov2d, cov2d_det, conic_of, clip_point, pixel_mean), so that the backward linearises the
// values the forward actually used and takes the forward's own decisions (cull, ray clamp, det == 0); the intermediates the chain
// needs (s, the normalised quaternion, M; x / z, y / z, J, T, T cov3d) come out of cov3d_of and ewa_cov2d through their keep-structs.
// This file holds the load, the cull compare, those calls and the chain: no forward arithmetic of its own.
// Held fixed, as the splat gradient already holds them: the tile rect, the footprint, pthr and the cull.
//
// Roofline: HBM.  32 B per gaussian for its row of grad_splat; a wave whose 64 rows are all zero leaves on that (most waves of a
// Morton-ordered scene under one camera); a touched gaussian costs 44 B read (mean 12, log-scales 12, quaternion 16, logit 4) and
// 44 B read-modify-written.
#include <cmath>
#include "gsr_internal.h"
#include "gauss_math.h"

namespace gsr {

constexpr int PB_THREADS = 256;

// 5 waves per SIMD: 82 VGPRs, no scratch.  Asked for 6 it takes 80 and measures the same; asked for 8 it spills
__global__ __launch_bounds__(PB_THREADS, 5) void project_backward_kernel(GsrScene sc, Cam cam, int compat, const float4 *__restrict__ grad_splat,
                                                                      float *__restrict__ grad_means, float *__restrict__ grad_log_scales,
                                                                      float *__restrict__ grad_quats, float *__restrict__ grad_opacity_logit)
{
    const int64_t i = (int64_t)blockIdx.x * PB_THREADS + threadIdx.x;  // the constant, not blockDim.x (as in preprocess_kernel)
    float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0;
    if (i < sc.n) { r0 = grad_splat[2 * i]; r1 = grad_splat[2 * i + 1]; }
    const float g_op = r0.x, g_mx = r0.y, g_my = r0.z, g_s0 = r0.w, g_s1 = r1.x, g_s2 = r1.y;  // columns 6 and 7 are not looked at
    const bool touched = g_op != 0.0f || g_mx != 0.0f || g_my != 0.0f || g_s0 != 0.0f || g_s1 != 0.0f || g_s2 != 0.0f;
    if (__ballot(touched) == 0ull) return;  // wave-uniform: 32 B per gaussian and nothing else
    if (!touched) return;

    // ---- the forward, by the functions geometry_one / geometry_view call (gauss_math.h) ------------------------------------------------
    const float *V = cam.V, *F = cam.F;
    const float p[3] = {sc.means[3 * i], sc.means[3 * i + 1], sc.means[3 * i + 2]};
    float cm[3];
    cam_mean(V, p, cm);
    if (cm[2] < GSR_CULL_Z) return;  // culled: contributes nothing (after its 12-B mean, as in the preprocess)

    const float ls[3] = {sc.log_scales[3 * i], sc.log_scales[3 * i + 1], sc.log_scales[3 * i + 2]};
    const float4 q = reinterpret_cast<const float4 *>(sc.quats)[i];
    float C3[3][3], c2[4];
    Cov3dKeep k3;
    EwaKeep k2;
    cov3d_of(ls, q, C3, &k3);
    ewa_cov2d(V, C3, cm, cam.fx, cam.fy, cam.limx, cam.limy, c2, &k2);
    const float a = c2[0], b01 = c2[1], b10 = c2[2], c = c2[3];
    const float det = cov2d_det(a, b01, b10, c);
    if (det == 0.0f) return;  // (geometry_view goes on with 0 for 1 / det and draws nothing)
    float sx, sy, sxy;
    const float det_inv = conic_of(det, a, b01, c, &sx, &sy, &sxy);
    if (!(fabsf(sx) < INFINITY) || !(fabsf(sy) < INFINITY) || !(fabsf(sxy) < INFINITY)) return;
    if (compat && (sx == 0.0f || sy == 0.0f || sxy == 0.0f)) return;  // Q2: the reference's loop never draws it
    const float (&s)[3] = k3.s, (&M)[3][3] = k3.M, (&T)[3][3] = k2.T, (&TV)[3][3] = k2.TV;  // (rows 0 and 1 of T and T cov3d are read)
    const float nrm = k3.nrm, qw = k3.q[0], qx = k3.q[1], qy = k3.q[2], qz = k3.q[3];
    const float tz = cm[2], J00 = k2.J[0][0], J02 = k2.J[0][2], J11 = k2.J[1][1], J12 = k2.J[1][2];

    // ---- the chain ----------------------------------------------------------------------------------------------------------------------
    // sigmas <- cov2d: s0 = c / det, s1 = a / det, s2 = -b01 / det, det = a c - b10 b01, the four entries separate inputs.  Every
    // entry of the Jacobian in the form without a difference (d s0 / d c = 1 / det - a c / det^2 = -b10 b01 / det^2, ...).
    const float di2 = det_inv * det_inv, bb = b10 * b01;
    const float ga = di2 * ((-(c * c) * g_s0 - bb * g_s1) + (b01 * c) * g_s2);
    const float gc = di2 * ((-bb * g_s0 - (a * a) * g_s1) + (b01 * a) * g_s2);
    const float gb01 = di2 * (((c * b10) * g_s0 + (a * b10) * g_s1) - (a * c) * g_s2);
    const float gb10 = di2 * (((c * b01) * g_s0 + (a * b01) * g_s1) - (b01 * b01) * g_s2);
    // cov2d = T cov3d T^T + 0.3 I (the low-pass is a constant); cov3d symmetric, so both off-diagonal entries are one function of
    // (T, cov3d) and only P = g + g^T enters: d / d cov3d = T^T P T (with its transpose), d / d T = P (T cov3d)
    const float P00 = 2.0f * ga, P01 = gb01 + gb10, P11 = 2.0f * gc;

    float gp[3] = {0.0f, 0.0f, 0.0f};
    if (grad_means != nullptr) {
        float gT[2][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            gT[0][k] = P00 * TV[0][k] + P01 * TV[1][k];
            gT[1][k] = P01 * TV[0][k] + P11 * TV[1][k];
        }
        // T = J A^T (A = w2c[:3,:3], row-vector convention: A^T[m][c] = V[4 c + m])
        const float gJ00 = (gT[0][0] * V[0] + gT[0][1] * V[4]) + gT[0][2] * V[8];
        const float gJ02 = (gT[0][0] * V[2] + gT[0][1] * V[6]) + gT[0][2] * V[10];
        const float gJ11 = (gT[1][0] * V[1] + gT[1][1] * V[5]) + gT[1][2] * V[9];
        const float gJ12 = (gT[1][0] * V[2] + gT[1][1] * V[6]) + gT[1][2] * V[10];
        // J <- cam_mean.  J00 = fx / z; J02 = -fx u / z with u = clamp(x / z): inside the clamp u = x / z (d/dx = -fx / z^2,
        // d/dz = -2 J02 / z); where it is active u is the constant +-lim, the derivative in x / z is 0 and tx = +-lim z still gives
        // d/dz = -J02 / z
        const bool in_x = k2.txtz > -cam.limx && k2.txtz < cam.limx, in_y = k2.tytz > -cam.limy && k2.tytz < cam.limy;
        const float itz = 1.0f / tz;
        float gcm[3];
        gcm[0] = in_x ? -(gJ02 * J00) * itz : 0.0f;
        gcm[1] = in_y ? -(gJ12 * J11) * itz : 0.0f;
        gcm[2] = -(((gJ00 * J00 + gJ11 * J11) + (in_x ? 2.0f : 1.0f) * (gJ02 * J02)) + (in_y ? 2.0f : 1.0f) * (gJ12 * J12)) * itz;
        // screen_mean <- mean, through full_proj and 1 / (w + 1e-7): mx = ((x_clip p_w + 1) W - 1) / 2
        float pt[4], mx, my;
        clip_point(F, p, pt);
        const float p_w = pixel_mean(pt, (float)cam.W, (float)cam.H, &mx, &my), pt0 = pt[0], pt1 = pt[1];
        const float gnx = g_mx * (0.5f * (float)cam.W), gny = g_my * (0.5f * (float)cam.H);
        const float gpt0 = gnx * p_w, gpt1 = gny * p_w, gpt3 = -((gnx * pt0 + gny * pt1) * p_w) * p_w;
        // cam_mean <- mean and the clip point <- mean
#pragma unroll
        for (int k = 0; k < 3; ++k)
            gp[k] = ((gcm[0] * V[4 * k] + gcm[1] * V[4 * k + 1]) + gcm[2] * V[4 * k + 2]) +
                    ((gpt0 * F[4 * k] + gpt1 * F[4 * k + 1]) + gpt3 * F[4 * k + 3]);
    }

    float gls[3] = {0.0f, 0.0f, 0.0f}, gq[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (grad_log_scales != nullptr || grad_quats != nullptr) {
        // d / d cov3d, symmetrised: S = T^T P T
        float U[2][3], S[3][3], gM[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            U[0][k] = P00 * T[0][k] + P01 * T[1][k];
            U[1][k] = P01 * T[0][k] + P11 * T[1][k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int l = 0; l < 3; ++l) S[k][l] = T[0][k] * U[0][l] + T[1][k] * U[1][l];
        // cov3d = M M^T: d / d M = S M
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int l = 0; l < 3; ++l) gM[k][l] = (S[k][0] * M[0][l] + S[k][1] * M[1][l]) + S[k][2] * M[2][l];
        // M = R diag(s), s = exp(log_scale): d / d log_scale_j = sum_k gM[k][j] M[k][j]
#pragma unroll
        for (int j = 0; j < 3; ++j) gls[j] = (gM[0][j] * M[0][j] + gM[1][j] * M[1][j]) + gM[2][j] * M[2][j];
        if (grad_quats != nullptr) {
            float gR[3][3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int l = 0; l < 3; ++l) gR[k][l] = gM[k][l] * s[l];
            // R <- the normalised quaternion: the transpose of quat_to_rot(w, x, y, z, R), which cov3d_of calls
            const float gw = 2.0f * (((qz * (gR[1][0] - gR[0][1]) + qy * (gR[0][2] - gR[2][0])) + qx * (gR[2][1] - gR[1][2])));
            const float gx = 2.0f * ((((qy * (gR[0][1] + gR[1][0]) + qz * (gR[0][2] + gR[2][0])) + qw * (gR[2][1] - gR[1][2])) -
                                      2.0f * qx * (gR[1][1] + gR[2][2])));
            const float gy = 2.0f * ((((qx * (gR[0][1] + gR[1][0]) + qz * (gR[1][2] + gR[2][1])) + qw * (gR[0][2] - gR[2][0])) -
                                      2.0f * qy * (gR[0][0] + gR[2][2])));
            const float gz = 2.0f * ((((qx * (gR[0][2] + gR[2][0]) + qy * (gR[1][2] + gR[2][1])) + qw * (gR[1][0] - gR[0][1])) -
                                      2.0f * qz * (gR[0][0] + gR[1][1])));
            // normalised <- stored: n = q / max(|q|, 1e-12); at the floor the divisor is a constant
            const float dot = k3.nrm_floor ? 0.0f : ((qw * gw + qx * gx) + qy * gy) + qz * gz;
            gq[0] = (gw - qw * dot) / nrm;
            gq[1] = (gx - qx * dot) / nrm;
            gq[2] = (gy - qy * dot) / nrm;
            gq[3] = (gz - qz * dot) / nrm;
        }
    }

    if (grad_means != nullptr) {
        grad_means[3 * i] += gp[0]; grad_means[3 * i + 1] += gp[1]; grad_means[3 * i + 2] += gp[2];
    }
    if (grad_log_scales != nullptr) {
        grad_log_scales[3 * i] += gls[0]; grad_log_scales[3 * i + 1] += gls[1]; grad_log_scales[3 * i + 2] += gls[2];
    }
    if (grad_quats != nullptr) {
        float4 *dst = reinterpret_cast<float4 *>(grad_quats) + i;
        float4 v = *dst;
        v.x += gq[0]; v.y += gq[1]; v.z += gq[2]; v.w += gq[3];
        *dst = v;
    }
    if (grad_opacity_logit != nullptr) {
        // opacity = sigmoid(x): sigmoid(x) sigmoid(-x), not o (1 - o) (at logit 12, 1 - o has lost its digits)
        const float x = sc.opacity_logit[i];
        grad_opacity_logit[i] += g_op * ((1.0f / (1.0f + expf(-x))) * (1.0f / (1.0f + expf(x))));
    }
}

int launch_project_backward(const GsrScene &scene, const GsrCamera &cam, const GsrOptions &opts, const float *grad_splat, float *grad_means,
                            float *grad_log_scales, float *grad_quats, float *grad_opacity_logit, hipStream_t s)
{
    if (scene.n <= 0) return GSR_OK;
    const unsigned grid = (unsigned)((scene.n + PB_THREADS - 1) / PB_THREADS);
    hipLaunchKernelGGL(project_backward_kernel, dim3(grid), dim3(PB_THREADS), 0, s, scene, make_cam(cam), opts.reference_compat ? 1 : 0,
                       reinterpret_cast<const float4 *>(grad_splat), grad_means, grad_log_scales, grad_quats, grad_opacity_logit);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

}  // namespace gsr
