// sh_backward.hip — the transpose of sh_to_rgb (gauss_math.h's sh_eval_with) for one view: row i of grad_rgb (d L / d colour of
// gaussian i) carried to its SH coefficients (grad_sh [n,16,3]) and, through the view direction u = (mean - cam_center) / r, to its
// mean (grad_means [n,3]).  sh_backward_kernel: one thread per gaussian, no atomics (a gaussian belongs to one thread).
//
// Built with -ffp-contract=off, like preprocess.hip: the value before the clamp is recomputed by the forward's own function
// (sh_eval_with<false>) on the same coefficients, so that the clamp mask m_c = [0 <= v_c <= 1] is the forward's decision bit for bit; the
// view direction and the basis values come from the functions that one calls (sh_dir, sh_band1 .. 3, with their constants).  Only
// the derivatives of the basis, which the forward has no expression for, are written here.
//
// Roofline: HBM.  12 B per gaussian for its row of grad_rgb; a wave whose 64 rows are all zero leaves on that.  A touched gaussian
// moves 12 (mean) + 192 (SH row; 96 as fp16) + 384 (its row of grad_sh read and written) + 24 (grad_means) B.  One thread per row
// at a 192-B lane stride uses an eighth of every line per wave-instruction, so a DENSE wave (a full wave with at least
// GSR_SHB_DENSE_MIN touched lanes) moves its 64 SH rows and its 64 rows of grad_sh — 12 KB of consecutive addresses each — as whole
// lines, consecutive lanes taking consecutive 16 B, transposed through LDS in two rounds of 32 rows.  An LDS row is 13 float4 apart
// (52 dwords): the eight lanes of a ds_write_b128 group then sit on banks 0, 20, 8, 28, 16, 4, 24, 12 (mod 32) and the sixteen
// of a ds_read_b128 group on sixteen different 16-B slots (mod 64), where rows 12 float4 apart would be 4-way on both.  The sum
// old + delta is formed once per element in either form: the two give the same bits.
#include <cmath>
#include "gsr_internal.h"
#include "gauss_math.h"

#ifndef GSR_SHB_DENSE_MIN
#define GSR_SHB_DENSE_MIN 32  // touched lanes from which a full wave takes the LDS path (65 = never; measured: DESIGN.md §5.29)
#endif

namespace gsr {

constexpr int SHB_THREADS = 256;
constexpr int SHB_LDS_ROW = 13;               // float4 per staged row: 12 + 1 of padding
constexpr int SHB_LDS_WAVE = 32 * SHB_LDS_ROW;  // a wave stages 32 rows at a time

// 64 consecutive fp32 SH rows (those of gaussians i0 .. i0 + 63, all in range) into each lane's registers: float4 `col` of every
// row for col < nq, the rest zero.  Whole-line loads, then a lane reads its own row.  A wave's LDS operations execute in order.
__device__ __forceinline__ void load_rows_dense(const float *sh, int64_t i0, int lane, int nq, float4 *lds, float out[48])
{
    const float4 *base = reinterpret_cast<const float4 *>(sh + 48 * i0);
#pragma unroll
    for (int e = 0; e < 48; ++e) out[e] = 0.0f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int idx = k * 64 + lane, row = idx / 12, col = idx - 12 * row;
            if (col < nq) lds[row * SHB_LDS_ROW + col] = base[h * 384 + idx];
        }
        __builtin_amdgcn_wave_barrier();
        if ((lane >> 5) == h) {
            const float4 *row = lds + (lane & 31) * SHB_LDS_ROW;
#pragma unroll
            for (int j = 0; j < 12; ++j)
                if (j < nq) {
                    const float4 v = row[j];
                    out[4 * j] = v.x; out[4 * j + 1] = v.y; out[4 * j + 2] = v.z; out[4 * j + 3] = v.w;
                }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

__device__ __forceinline__ void load_row(const float *sh, int64_t i, int nq, float out[48])
{
    const float4 *p = reinterpret_cast<const float4 *>(sh + 48 * i);
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (j < nq) v = p[j];
        out[4 * j] = v.x; out[4 * j + 1] = v.y; out[4 * j + 2] = v.z; out[4 * j + 3] = v.w;
    }
}

// 4 waves per SIMD asked for; registers and LDS: DESIGN.md §5.29
template <bool SH16>
__global__ __launch_bounds__(SHB_THREADS, 4) void sh_backward_kernel(GsrScene sc, float ccx, float ccy, float ccz,
                                                                     const float *__restrict__ grad_rgb, int64_t grad_stride,
                                                                     float *__restrict__ grad_sh, float *__restrict__ grad_means)
{
#pragma clang fp contract(off)
    __shared__ float4 s_rows[(SHB_THREADS / 64) * SHB_LDS_WAVE];
    const int64_t i = (int64_t)blockIdx.x * SHB_THREADS + threadIdx.x;  // the constant, not blockDim.x (as in preprocess_kernel)
    float g[3] = {0.0f, 0.0f, 0.0f};
    if (i < sc.n) {
        const float *row = grad_rgb + i * grad_stride;
        g[0] = row[0]; g[1] = row[1]; g[2] = row[2];
    }
    const bool touched = g[0] != 0.0f || g[1] != 0.0f || g[2] != 0.0f;
    const unsigned long long touched_mask = __ballot(touched);
    if (touched_mask == 0ull) return;  // wave-uniform: 12 B per gaussian and nothing else

    const int degree = sc.sh_degree;
    const int ne = 3 * (degree + 1) * (degree + 1);  // the floats of a row this degree reads: 3, 12, 27, 48
    const int nq = (ne + 3) >> 2;                      // ... in float4: 1, 3, 7, 12
    const int lane = threadIdx.x & 63;
    const int64_t i0 = i - lane;
    float4 *lds = s_rows + (threadIdx.x >> 6) * SHB_LDS_WAVE;
    // wave-uniform: a full wave (the last one of the grid may not be) most of whose rows are touched
    const bool dense = i0 + 64 <= sc.n && (int)__popcll(touched_mask) >= GSR_SHB_DENSE_MIN;

    // ---- the forward: the value before the clamp, by the forward's own function -------------------------------------------------
    float sh[48];
    if (SH16) {
        if (touched) load_sh48_f16(sc.sh, i, sh);
    } else if (dense) {
        load_rows_dense(reinterpret_cast<const float *>(sc.sh), i0, lane, nq, lds, sh);
    } else if (touched) {
        load_row(reinterpret_cast<const float *>(sc.sh), i, nq, sh);
    }
    bool active = false;
    float mg[3] = {0.0f, 0.0f, 0.0f};  // m_c g_c
    float B[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) B[k] = 0.0f;
    if (touched) {
        const float p[3] = {sc.means[3 * i], sc.means[3 * i + 1], sc.means[3 * i + 2]};
        const float cc[3] = {ccx, ccy, ccz};
        float val[3];
        sh_eval_with<false>(p, [&sh](int e) { return sh[e]; }, cc, degree, val);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const bool pass = val[c] >= 0.0f && val[c] <= 1.0f;  // the edges pass; a NaN (a mean on the camera centre) does not
            mg[c] = pass ? g[c] : 0.0f;
            active = active || (pass && g[c] != 0.0f);
        }
        if (active) {
            // the direction and the basis, by the functions sh_eval_with calls; B[3] with the sign the forward applies where it subtracts
            float x, y, z;
            const float n = sh_dir(p, cc, &x, &y, &z);
            const float xx = x * x, yy = y * y;  // (for the derivatives)
            B[0] = SH_C0;
            if (degree > 0) {
                sh_band1(x, y, z, B + 1);
                B[3] = -B[3];
                if (degree > 1) {
                    sh_band2(x, y, z, B + 4);
                    if (degree > 2) sh_band3(x, y, z, B + 9);
                }
            }
            // ---- d / d mean: sum_k grad_u b_k(u) w_k with w_k = sum_c m_c g_c sh[k][c], then (I - u u^T) / r.  Zero at degree 0.
            if (grad_means != nullptr && degree > 0) {
                float w[16];
#pragma unroll
                for (int k = 1; k < 16; ++k) w[k] = (mg[0] * sh[3 * k] + mg[1] * sh[3 * k + 1]) + mg[2] * sh[3 * k + 2];
                float gx = -(SH_C1 * w[3]), gy = SH_NC1 * w[1], gz = SH_C1 * w[2];
                if (degree > 1) {
                    const float zz = z * z;
                    gx = gx + ((((SH_K20 * y) * w[4] - ((2.0f * SH_K22) * x) * w[6]) + (SH_K23 * z) * w[7]) + ((2.0f * SH_K24) * x) * w[8]);
                    gy = gy + ((((SH_K20 * x) * w[4] + (SH_K21 * z) * w[5]) - ((2.0f * SH_K22) * y) * w[6]) - ((2.0f * SH_K24) * y) * w[8]);
                    gz = gz + (((SH_K21 * y) * w[5] + ((4.0f * SH_K22) * z) * w[6]) + (SH_K23 * x) * w[7]);
                    if (degree > 2) {
                        const float xy = x * y, q4 = (4.0f * zz - xx) - yy;
                        gx = gx + (((((((6.0f * SH_K30) * xy) * w[9] + ((SH_K31 * y) * z) * w[10]) - ((2.0f * SH_K32) * xy) * w[11]) -
                                     (((6.0f * SH_K33) * z) * x) * w[12]) + (SH_K34 * (q4 - 2.0f * xx)) * w[13]) +
                                   (((2.0f * SH_K35) * z) * x) * w[14]) + ((3.0f * SH_K36) * (xx - yy)) * w[15];
                        gy = gy + (((((((3.0f * SH_K30) * (xx - yy)) * w[9] + ((SH_K31 * x) * z) * w[10]) + (SH_K32 * (q4 - 2.0f * yy)) * w[11]) -
                                     (((6.0f * SH_K33) * z) * y) * w[12]) - ((2.0f * SH_K34) * xy) * w[13]) -
                                   (((2.0f * SH_K35) * z) * y) * w[14]) - ((6.0f * SH_K36) * xy) * w[15];
                        gz = gz + ((((((SH_K31 * xy) * w[10] + (((8.0f * SH_K32) * y) * z) * w[11]) +
                                      (SH_K33 * ((6.0f * zz - 3.0f * xx) - 3.0f * yy)) * w[12]) + (((8.0f * SH_K34) * x) * z) * w[13]) +
                                    (SH_K35 * (xx - yy)) * w[14]));
                    }
                }
                const float dot = (gx * x + gy * y) + gz * z;
                grad_means[3 * i] += (gx - x * dot) / n;
                grad_means[3 * i + 1] += (gy - y * dot) / n;
                grad_means[3 * i + 2] += (gz - z * dot) / n;
            }
        }
    }
    if (grad_sh == nullptr) return;

    // ---- d / d sh: grad_sh[i][k][c] += b_k m_c g_c for the ne floats of the degree; a row that is not active is not touched -------
    float4 *out = reinterpret_cast<float4 *>(grad_sh);
    if (dense) {
        const unsigned long long active_mask = __ballot(active);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if ((lane >> 5) == h && active) {
                float4 *row = lds + (lane & 31) * SHB_LDS_ROW;
#pragma unroll
                for (int j = 0; j < 12; ++j)
                    if (j < nq)
                        row[j] = make_float4(B[(4 * j) / 3] * mg[(4 * j) % 3], B[(4 * j + 1) / 3] * mg[(4 * j + 1) % 3],
                                             B[(4 * j + 2) / 3] * mg[(4 * j + 2) % 3], B[(4 * j + 3) / 3] * mg[(4 * j + 3) % 3]);
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const int idx = k * 64 + lane, row = idx / 12, col = idx - 12 * row;
                if (col < nq && ((active_mask >> (32 * h + row)) & 1ull)) {
                    float4 *dst = out + 12 * i0 + h * 384 + idx;
                    const float4 d = lds[row * SHB_LDS_ROW + col];
                    float4 v = *dst;
                    const int e = 4 * col;
                    v.x += d.x;  // (e < ne: col < nq)
                    if (e + 1 < ne) v.y += d.y;
                    if (e + 2 < ne) v.z += d.z;
                    if (e + 3 < ne) v.w += d.w;
                    *dst = v;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    } else if (active) {
        float4 *row = out + 12 * i;
#pragma unroll
        for (int j = 0; j < 12; ++j)
            if (j < nq) {
                float4 v = row[j];
                v.x += B[(4 * j) / 3] * mg[(4 * j) % 3];
                if (4 * j + 1 < ne) v.y += B[(4 * j + 1) / 3] * mg[(4 * j + 1) % 3];
                if (4 * j + 2 < ne) v.z += B[(4 * j + 2) / 3] * mg[(4 * j + 2) % 3];
                if (4 * j + 3 < ne) v.w += B[(4 * j + 3) / 3] * mg[(4 * j + 3) % 3];
                row[j] = v;
            }
    }
}

int launch_sh_backward(const GsrScene &scene, const GsrCamera &cam, const float *grad_rgb, int64_t grad_stride, float *grad_sh,
                       float *grad_means, hipStream_t s)
{
    if (scene.n <= 0) return GSR_OK;
    const unsigned grid = (unsigned)((scene.n + SHB_THREADS - 1) / SHB_THREADS);
    if (scene.sh_dtype == 1)
        hipLaunchKernelGGL(sh_backward_kernel<true>, dim3(grid), dim3(SHB_THREADS), 0, s, scene, cam.cam_center[0], cam.cam_center[1],
                           cam.cam_center[2], grad_rgb, grad_stride, grad_sh, grad_means);
    else
        hipLaunchKernelGGL(sh_backward_kernel<false>, dim3(grid), dim3(SHB_THREADS), 0, s, scene, cam.cam_center[0], cam.cam_center[1],
                           cam.cam_center[2], grad_rgb, grad_stride, grad_sh, grad_means);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

}  // namespace gsr
