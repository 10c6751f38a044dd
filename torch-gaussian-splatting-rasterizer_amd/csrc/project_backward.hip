// project_backward.hip — the transpose of stage 1's geometry: the splat gradient of a view (row i of grad_splat: d L / d opacity,
// 2-D mean, inverse 2-D covariance, as blend_splat_backward.hip leaves them) chained to what the scene stores — mean, log-scales,
// quaternion, opacity logit.  project_backward_kernel: one thread per gaussian, no LDS, no atomics (a gaussian belongs to one thread).
//
// The chain down to P, gcm and gpt is splat_chain.h's, shared with camera_backward.hip (what it recomputes, decides and holds fixed:
// there); here are the load, the wave-uniform exit, the tails, the combination into d / d mean and the stores.  -ffp-contract=off.
//
// Roofline: HBM.  32 B per gaussian for its row of grad_splat; a wave whose 64 rows are all zero leaves on that (most waves of a
// Morton-ordered scene under one camera); a touched gaussian costs 44 B read (mean 12, log-scales 12, quaternion 16, logit 4) and
// 44 B read-modify-written.
#include "splat_chain.h"

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
    SplatRow g;
    const bool touched = splat_row(r0, r1, g);
    if (__ballot(touched) == 0ull) return;  // wave-uniform: 32 B per gaussian and nothing else
    if (!touched) return;

    SplatForward f;
    if (!splat_forward(sc, cam, compat, i, f)) return;
    const float *V = cam.V, *F = cam.F;
    const float (&s)[3] = f.k3.s, (&M)[3][3] = f.k3.M, (&T)[3][3] = f.k2.T;  // (rows 0 and 1 of T are read)
    const float nrm = f.k3.nrm, qw = f.k3.q[0], qx = f.k3.q[1], qy = f.k3.q[2], qz = f.k3.q[3];
    const CovGrad P = cov2d_grad(g, f);

    float gp[3] = {0.0f, 0.0f, 0.0f};
    if (grad_means != nullptr) {
        MeanGrad m;
        mean_grad(cam, g, f, P, m);
        // cam_mean <- mean and the clip point <- mean
#pragma unroll
        for (int k = 0; k < 3; ++k)
            gp[k] = ((m.gcm[0] * V[4 * k] + m.gcm[1] * V[4 * k + 1]) + m.gcm[2] * V[4 * k + 2]) +
                    ((m.gpt[0] * F[4 * k] + m.gpt[1] * F[4 * k + 1]) + m.gpt[2] * F[4 * k + 3]);
    }

    float gls[3] = {0.0f, 0.0f, 0.0f}, gq[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (grad_log_scales != nullptr || grad_quats != nullptr) {
        // d / d cov3d, symmetrised: S = T^T P T
        float U[2][3], S[3][3], gM[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            U[0][k] = P.P00 * T[0][k] + P.P01 * T[1][k];
            U[1][k] = P.P01 * T[0][k] + P.P11 * T[1][k];
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
            const float dot = f.k3.nrm_floor ? 0.0f : ((qw * gw + qx * gx) + qy * gy) + qz * gz;
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
        grad_opacity_logit[i] += g.g_op * ((1.0f / (1.0f + expf(-x))) * (1.0f / (1.0f + expf(x))));
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
