// gauss_math.h — the per-gaussian forward, each step stated ONCE: the fused preprocess kernels, the stand-alone helpers, the blend's
// deferred colours and both backward kernels (project_backward.hip, sh_backward.hip) call these functions, so a backward linearises
// the very expressions the forward evaluates.  What a backward needs beyond a step's result, the step hands out
// through an optional keep-struct (Cov3dKeep, EwaKeep: the function fills its own and copies it out on request, which folds away after inlining).
// Every function keeps the reference's fp32 operation order (file:line cited); translation units that include this header are built
// with -ffp-contract=off (blend.hip, which is not, uses the SH functions only: each carries its own pragma).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include "../../include/gsr.h"

namespace gsr {

// Coordinate j of [p 1] A for a 4x4 A in the row-vector convention (16 floats): with A = w2c the camera-space mean
// (project_to_camera_space, rasterize.py:80-86; its z is what the cull, :377, looks at), with A = full_proj the clip point (:374).
__device__ __forceinline__ float point_through(const float *A, const float p[3], int j) { return ((p[0] * A[0 + j] + p[1] * A[4 + j]) + p[2] * A[8 + j]) + A[12 + j]; }
__device__ __forceinline__ float cam_z(const float *V, const float p[3]) { return point_through(V, p, 2); }
__device__ __forceinline__ void cam_mean(const float *V, const float p[3], float cm[3])
{
#pragma unroll
    for (int j = 0; j < 3; ++j) cm[j] = point_through(V, p, j);
}
__device__ __forceinline__ void clip_point(const float *F, const float p[3], float pt[4])
{
#pragma unroll
    for (int j = 0; j < 4; ++j) pt[j] = point_through(F, p, j);
}

// perspective divide, rasterize.py:381-382, and NDC -> pixel, :391.  Returns p_w = 1 / (w + 1e-7).
__device__ __forceinline__ float pixel_mean(const float pt[4], float Wf, float Hf, float *mx, float *my)
{
    const float p_w = 1.0f / (pt[3] + 0.0000001f);
    const float ndc_x = pt[0] * p_w, ndc_y = pt[1] * p_w;
    *mx = ((ndc_x + 1.0f) * Wf - 1.0f) / 2.0f, *my = ((ndc_y + 1.0f) * Hf - 1.0f) / 2.0f;
    return p_w;
}

// rasterize.py:41-56 on fp32 inputs
__device__ __forceinline__ void quat_to_rot(float w, float x, float y, float z, float R[3][3])
{
    R[0][0] = 1.0f - 2.0f * (y * y) - 2.0f * (z * z); R[0][1] = 2.0f * x * y - 2.0f * z * w;           R[0][2] = 2.0f * x * z + 2.0f * y * w;
    R[1][0] = 2.0f * x * y + 2.0f * z * w;           R[1][1] = 1.0f - 2.0f * (x * x) - 2.0f * (z * z); R[1][2] = 2.0f * y * z - 2.0f * x * w;
    R[2][0] = 2.0f * x * z - 2.0f * y * w;           R[2][1] = 2.0f * y * z + 2.0f * x * w;           R[2][2] = 1.0f - 2.0f * (x * x) - 2.0f * (y * y);
}

// What cov3d_of computes on its way, for the backward: exp(log-scale); |q| floored, and whether the floor was active; the normalised
// quaternion (w, x, y, z); M = R diag(s)
struct Cov3dKeep {
    float s[3], nrm, q[4], M[3][3];
    bool nrm_floor;
};

// get_covariance_matrix_from_mesh, rasterize.py:89-120
__device__ __forceinline__ void cov3d_of(const float ls[3], const float4 q, float cov[3][3], Cov3dKeep *keep = nullptr)
{
    Cov3dKeep k;
    k.s[0] = expf(ls[0]); k.s[1] = expf(ls[1]); k.s[2] = expf(ls[2]);
    const float nrm = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    k.nrm_floor = nrm < 1e-12f;
    k.nrm = k.nrm_floor ? 1e-12f : nrm;  // F.normalize eps, :112
    k.q[0] = q.x / k.nrm; k.q[1] = q.y / k.nrm; k.q[2] = q.z / k.nrm; k.q[3] = q.w / k.nrm;
    float R[3][3];
    quat_to_rot(k.q[0], k.q[1], k.q[2], k.q[3], R);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) k.M[i][j] = R[i][j] * k.s[j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) cov[i][j] = k.M[i][0] * k.M[j][0] + k.M[i][1] * k.M[j][1] + k.M[i][2] * k.M[j][2];
    if (keep != nullptr) *keep = k;
}

// The SH basis of spherical_harmonics.py:27-65, one function per band, each value written exactly as the reference writes it; the
// constants by name, for the colour backward's derivatives of the same polynomials.  Each function switches contraction off itself.
constexpr float SH_C0 = 0.28209479177387814f, SH_C1 = 0.4886025119029199f, SH_NC1 = -0.4886025119029199f;
constexpr float SH_K20 = 1.0925484305920792f, SH_K21 = -1.0925484305920792f, SH_K22 = 0.31539156525252005f,
                SH_K23 = -1.0925484305920792f, SH_K24 = 0.5462742152960396f;
constexpr float SH_K30 = -0.5900435899266435f, SH_K31 = 2.890611442640554f, SH_K32 = -0.4570457994644658f,
                SH_K33 = 0.3731763325901154f, SH_K34 = -0.4570457994644658f, SH_K35 = 1.445305721320277f,
                SH_K36 = -0.5900435899266435f;

// view direction u = (mean - cam_center) / r, :37-40; returns r
__device__ __forceinline__ float sh_dir(const float p[3], const float cc[3], float *x, float *y, float *z)
{
#pragma clang fp contract(off)
    const float d0 = p[0] - cc[0], d1 = p[1] - cc[1], d2 = p[2] - cc[2];
    const float n = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
    *x = d0 / n; *y = d1 / n; *z = d2 / n;
    return n;
}

// band 1, :45-46: b[0], b[1] multiply sh1, sh2; b[2] = c1 x is SUBTRACTED with sh3 (basis_3 = -b[2], the same IEEE value either way)
__device__ __forceinline__ void sh_band1(float x, float y, float z, float *b)
{
#pragma clang fp contract(off)
    b[0] = SH_NC1 * y; b[1] = SH_C1 * z; b[2] = SH_C1 * x;
}

// band 2, :48-55: basis 4..8
__device__ __forceinline__ void sh_band2(float x, float y, float z, float *b)
{
#pragma clang fp contract(off)
    const float xx = x * x, yy = y * y;
    b[0] = (SH_K20 * x) * y; b[1] = (SH_K21 * y) * z; b[2] = SH_K22 * (((2.0f * z) * z - xx) - yy); b[3] = (SH_K23 * x) * z;
    b[4] = SH_K24 * (xx - yy);
}

// band 3, :56-65: basis 9..15
__device__ __forceinline__ void sh_band3(float x, float y, float z, float *b)
{
#pragma clang fp contract(off)
    const float xx = x * x, yy = y * y;
    b[0] = (SH_K30 * y) * ((3.0f * x) * x - yy); b[1] = ((SH_K31 * x) * y) * z;
    b[2] = (SH_K32 * y) * (((4.0f * z) * z - xx) - yy);
    b[3] = (SH_K33 * z) * (((2.0f * z) * z - (3.0f * x) * x) - (3.0f * y) * y);
    b[4] = (SH_K34 * x) * (((4.0f * z) * z - xx) - yy); b[5] = (SH_K35 * z) * (xx - yy);
    b[6] = (SH_K36 * x) * (xx - (3.0f * y) * y);
}

// sh_to_rgb, spherical_harmonics.py:27-73, for one gaussian.  `get(e)` returns element e = 3 k + c of its [16][3] coefficient row.
// The evaluation walks the row in MEMORY order (coefficient-major), each element consumed once into its channel's running sums, so a
// caller that loads the row 16 B at a time needs only a few of its 48 values in registers at once (the blend evaluates deferred
// colours inside a 64-VGPR kernel: a band's basis values are computed where its `degree >` branch consumes them); per channel the
// operations and their association are the reference's:
//   col = sh0 c0;  col += ((-c1 y) sh1 + (c1 z) sh2) - (c1 x) sh3;  col += (((t4 + t5) + t6) + t7) + t8;  col += ((...(t9 + t10) ... ) + t15)
// with t_k = basis_k sh_k; + 0.5, clamp to [0, 1] (:69-71, Q7).
// CLAMP = false leaves the value BEFORE the clamp in rgb: what the colour backward (sh_backward.hip) decides its clamp mask on, so
// that the decision is the forward's own.
template <bool CLAMP = true, typename Get>
__device__ __forceinline__ void sh_eval_with(const float p[3], Get get, const float cc[3], int degree, float rgb[3])
{
#pragma clang fp contract(off)  // also where the including file is built with contraction on (blend.hip evaluates deferred colours)
    float x, y, z;
    sh_dir(p, cc, &x, &y, &z);
    float col[3], part[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) col[c] = get(c) * SH_C0;
    if (degree > 0) {
        float b[3];
        sh_band1(x, y, z, b);
#pragma unroll
        for (int c = 0; c < 3; ++c) part[c] = b[0] * get(3 + c);
#pragma unroll
        for (int c = 0; c < 3; ++c) part[c] = part[c] + b[1] * get(6 + c);
#pragma unroll
        for (int c = 0; c < 3; ++c) col[c] = col[c] + (part[c] - b[2] * get(9 + c));
        if (degree > 1) {
            float b[5];
            sh_band2(x, y, z, b);
#pragma unroll
            for (int c = 0; c < 3; ++c) part[c] = b[0] * get(12 + c);
#pragma unroll
            for (int c = 0; c < 3; ++c) part[c] = part[c] + b[1] * get(15 + c);
#pragma unroll
            for (int c = 0; c < 3; ++c) part[c] = part[c] + b[2] * get(18 + c);
#pragma unroll
            for (int c = 0; c < 3; ++c) part[c] = part[c] + b[3] * get(21 + c);
#pragma unroll
            for (int c = 0; c < 3; ++c) col[c] = col[c] + (part[c] + b[4] * get(24 + c));
            if (degree > 2) {
                float b[7];
                sh_band3(x, y, z, b);
#pragma unroll
                for (int c = 0; c < 3; ++c) part[c] = b[0] * get(27 + c);
#pragma unroll
                for (int c = 0; c < 3; ++c) part[c] = part[c] + b[1] * get(30 + c);
#pragma unroll
                for (int c = 0; c < 3; ++c) part[c] = part[c] + b[2] * get(33 + c);
#pragma unroll
                for (int c = 0; c < 3; ++c) part[c] = part[c] + b[3] * get(36 + c);
#pragma unroll
                for (int c = 0; c < 3; ++c) part[c] = part[c] + b[4] * get(39 + c);
#pragma unroll
                for (int c = 0; c < 3; ++c) part[c] = part[c] + b[5] * get(42 + c);
#pragma unroll
                for (int c = 0; c < 3; ++c) col[c] = col[c] + (part[c] + b[6] * get(45 + c));
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = col[c] + 0.5f;                        // :69
        rgb[c] = !CLAMP ? v : v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);  // :71 (Q7)
    }
}

// sh = 48 floats [16][3] of one gaussian, already in registers
__device__ __forceinline__ void sh_eval(const float p[3], const float *sh, const float cc[3], int degree, float rgb[3])
{
    sh_eval_with(p, [sh](int e) { return sh[e]; }, cc, degree, rgb);
}

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// fp16 storage: 96-B rows, six 16-B loads, widened to fp32 before evaluation
__device__ __forceinline__ void load_sh48_f16(const void *sh, int64_t i, float out[48])
{
    const uint4 *p = reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(sh) + 96 * i);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint4 v = p[k];
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            out[8 * k + 2 * j] = __half2float(__ushort_as_half((unsigned short)(w[j] & 0xFFFFu)));
            out[8 * k + 2 * j + 1] = __half2float(__ushort_as_half((unsigned short)(w[j] >> 16)));
        }
    }
}

__device__ __forceinline__ void load_sh48(const float *sh, int64_t i, float out[48])
{
    const float4 *p = reinterpret_cast<const float4 *>(sh + 48 * i);  // 192-B rows are 16-B aligned
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const float4 v = p[k];
        out[4 * k] = v.x; out[4 * k + 1] = v.y; out[4 * k + 2] = v.z; out[4 * k + 3] = v.w;
    }
}


// What ewa_cov2d computes on its way, for the backward: x / z and y / z before the ray clamp; J; T = J W and T cov3d (row 2 of J is
// zero and cov2d reads rows 0 and 1 only: a caller that reads no row 2 pays for none)
struct EwaKeep {
    float txtz, tytz, J[3][3], T[3][3], TV[3][3];
};

// compute_2d_covariance, rasterize.py:201-252, one gaussian.  V = w2c (row-vector convention, 16 floats),
// C3 = 3x3 covariance, cm = camera-space mean.  Returns the 2x2 block {a, b01, b10, c} incl. the 0.3 low-pass.
__device__ __forceinline__ void ewa_cov2d(const float *V, const float C3[3][3], const float cm[3], float fx, float fy, float limx,
                                          float limy, float out[4], EwaKeep *keep = nullptr)
{
    EwaKeep k = {};  // (the zeros of J, :224-228)
    const float tz = cm[2];
    k.txtz = cm[0] / tz, k.tytz = cm[1] / tz;
    const float tx = fminf(limx, fmaxf(-limx, k.txtz)) * tz;  // :218-221
    const float ty = fminf(limy, fmaxf(-limy, k.tytz)) * tz;
    k.J[0][0] = fx / tz;
    k.J[0][2] = -(fx * tx) / (tz * tz);
    k.J[1][1] = fy / tz;
    k.J[1][2] = -(fy * ty) / (tz * tz);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) k.T[r][c] = (V[4 * c + 0] * k.J[r][0] + V[4 * c + 1] * k.J[r][1]) + V[4 * c + 2] * k.J[r][2];  // :230-232
    const float vrk[3][3] = {{C3[0][0], C3[0][1], C3[0][2]}, {C3[0][1], C3[1][1], C3[1][2]}, {C3[0][2], C3[1][2], C3[2][2]}};  // :234-243
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) k.TV[r][c] = (k.T[r][0] * vrk[0][c] + k.T[r][1] * vrk[1][c]) + k.T[r][2] * vrk[2][c];
    float PC[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) PC[r][c] = (k.TV[r][0] * k.T[c][0] + k.TV[r][1] * k.T[c][1]) + k.TV[r][2] * k.T[c][2];  // :245
    out[0] = PC[0][0] + GSR_LOWPASS;  // :249
    out[1] = PC[0][1];
    out[2] = PC[1][0];
    out[3] = PC[1][1] + GSR_LOWPASS;  // :250
    if (keep != nullptr) *keep = k;
}

// determinant of the 2x2 block (compute_covering_bbox, rasterize.py:163) and the conic from it, :395-411: (sx, sy, sxy) = (c, a, -b01) / det,
// with 0 for 1 / det at det == 0 (a degenerate or culled gaussian; nobody draws it)
__device__ __forceinline__ float cov2d_det(float a, float b01, float b10, float c) { return a * c - b10 * b01; }

__device__ __forceinline__ float conic_of(float det, float a, float b01, float c, float *sx, float *sy, float *sxy)
{
    const float det_inv = det == 0.0f ? 0.0f : 1.0f / det;
    *sx = c * det_inv; *sy = a * det_inv; *sxy = (-b01) * det_inv;
    return det_inv;
}

// compute_covering_bbox, rasterize.py:154-198, one gaussian: tile-unit bbox as floats (already floored).
__device__ __forceinline__ void covering_bbox(float mx, float my, float a, float b01, float b10, float c, float Wf, float Hf,
                                              float tb[4], float *det_out, float *spread_out)
{
    const float det = cov2d_det(a, b01, b10, c);
    const float trace = a + c;
    const float disc = sqrtf(fmaxf((trace * trace) / 4.0f - det, GSR_EIG_FLOOR));
    const float l1 = trace / 2.0f + disc, l2 = trace / 2.0f - disc;
    const float spread = ceilf(GSR_GAUSSIAN_SPREAD * sqrtf(fmaxf(l1, l2)));
    tb[0] = floorf(clampf((mx - spread) / 16.0f, 0.0f, Wf - 1.0f));
    tb[1] = floorf(clampf((my - spread) / 16.0f, 0.0f, Hf - 1.0f));
    tb[2] = floorf(clampf((mx + (spread + 16.0f - 1.0f)) / 16.0f, 0.0f, Wf - 1.0f));
    tb[3] = floorf(clampf((my + (spread + 16.0f - 1.0f)) / 16.0f, 0.0f, Hf - 1.0f));
    *det_out = det;
    *spread_out = spread;
}

}  // namespace gsr
