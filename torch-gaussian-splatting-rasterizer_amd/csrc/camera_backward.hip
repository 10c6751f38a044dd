// camera_backward.hip — the splat gradient of a view chained to the CAMERA: d L / d w2c, full_proj, focal_x, focal_y and cam_center,
// the raw partials in the GsrCamera fields as the kernels read them, 32 doubles (layout: include/gsr.h, gsr_camera_backward).
// camera_backward_kernel walks the chain of splat_chain.h by the very functions project_backward_kernel calls and,
// where that kernel carries gT, gJ.., gcm and gpt on to the gaussian's mean, multiplies them by what the camera contributed.  The view
// direction's term (cam_center) is the negated column sum of grad_view_means, which gsr_sh_backward computed: no SH row is read here.
//
// A reduction of n gaussians into 30 numbers, deterministic and in double: the per-gaussian terms are fp32, as in the chain they
// extend; every sum ACROSS gaussians is a double sum in a fixed order — within a thread over its trips, across a wave (shuffles),
// across the workgroup's four waves (LDS, wave order), across workgroups (camera_reduce_kernel, row order).  No atomics.
//   - G <= CB_MAX_GROUPS workgroups (3 per CU of a 256-CU part), G = ceil(B / ceil(B / CB_MAX_GROUPS)) for B = ceil(n / 256) blocks
//     of 256 gaussians; workgroup g owns blocks g, g + G, g + 2 G, ...: the assignment depends on n alone.  Interleaved, not
//     contiguous runs: the touched gaussians of a Morton-ordered scene lie in stretches, a run is then nearly all early exits or
//     nearly all work, and the kernel ends with its slowest workgroup (0.231 ms against 0.150 ms);
//   - a thread keeps its 29 sums and its count in registers; a trip in which no lane of the wave is touched costs its 32 B (+ 12 B)
//     per gaussian and nothing else (the wave-uniform early exit of project_backward_kernel);
//   - each workgroup writes one row of 32 doubles into the workspace, unconditionally: nothing has to be cleared;
//   - camera_reduce_kernel, one workgroup: eight contiguous runs of rows summed in row order, the eight sums in run order.
//
// Built with -ffp-contract=off, like preprocess.hip and project_backward.hip.  Roofline: HBM, the reads of project_backward_kernel.
#include "splat_chain.h"

namespace gsr {

constexpr int CB_THREADS = 256;
constexpr int CB_MAX_GROUPS = 768;   // 3 per CU x 256 CUs: what 150 VGPRs (3 waves per SIMD) keep resident at once, so no second round
constexpr int CB_SLOTS = 32;         // doubles per row: 29 sums, the count, two zeros
constexpr int CB_PARTS = 8;          // camera_reduce_kernel: contiguous runs of rows summed side by side

static int64_t camera_backward_groups(int64_t n)
{
    const int64_t blocks = n > 0 ? (n + CB_THREADS - 1) / CB_THREADS : 0;
    const int64_t per = blocks > 0 ? (blocks + CB_MAX_GROUPS - 1) / CB_MAX_GROUPS : 1;
    return blocks > 0 ? (blocks + per - 1) / per : 0;  // <= CB_MAX_GROUPS; every workgroup makes per or per - 1 trips, at least one
}

size_t camera_backward_bytes(int64_t n)
{
    const int64_t g = camera_backward_groups(n);
    return (size_t)(g > 0 ? g : 1) * CB_SLOTS * sizeof(double);  // 256 B per row
}

// sum over the wave's 64 lanes in a fixed tree; lane 0 holds it
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__global__ __launch_bounds__(CB_THREADS) void camera_backward_kernel(GsrScene sc, Cam cam, int compat,
                                                                   const float4 *__restrict__ grad_splat,
                                                                   const float *__restrict__ grad_view_means, double *__restrict__ rows)
{
    __shared__ double part[CB_THREADS / 64][CB_SLOTS];
    double acc[29];
#pragma unroll
    for (int k = 0; k < 29; ++k) acc[k] = 0.0;
    uint32_t count = 0;  // < 2^32: a thread makes at most 2^31 / 2^8 / G + 1 trips

    // this workgroup's blocks: blockIdx.x, blockIdx.x + gridDim.x, ... — interleaved, so that the touched stretches of a spatially
    // ordered scene spread over all workgroups; the rows of the next trip are asked for before this trip's work
    const int64_t blocks = (sc.n + CB_THREADS - 1) / CB_THREADS;
    const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 n0 = zero4, n1 = zero4;
    {
        const int64_t i = (int64_t)blockIdx.x * CB_THREADS + threadIdx.x;  // the constant, not blockDim.x (as in project_backward_kernel)
        if (grad_splat != nullptr && i < sc.n) { n0 = grad_splat[2 * i]; n1 = grad_splat[2 * i + 1]; }
    }
    for (int64_t b = blockIdx.x; b < blocks; b += gridDim.x) {  // workgroup-uniform
        const int64_t i = b * CB_THREADS + threadIdx.x;
        const float4 r0 = n0, r1 = n1;
        n0 = zero4; n1 = zero4;
        {
            const int64_t in = i + (int64_t)gridDim.x * CB_THREADS;
            if (grad_splat != nullptr && in < sc.n) { n0 = grad_splat[2 * in]; n1 = grad_splat[2 * in + 1]; }
        }
        if (grad_view_means != nullptr && i < sc.n) {
            // cam_center: d = mean - cam_center, so the row enters negated; no cull and no skip (gsr_sh_backward has none)
            acc[26] -= (double)grad_view_means[3 * i]; acc[27] -= (double)grad_view_means[3 * i + 1]; acc[28] -= (double)grad_view_means[3 * i + 2];
        }
        SplatRow g;
        const bool touched = splat_row(r0, r1, g);
        if (__ballot(touched) == 0ull) continue;  // wave-uniform: the rows and nothing else
        if (!touched) continue;

        SplatForward f;
        if (!splat_forward(sc, cam, compat, i, f)) continue;
        ++count;
        MeanGrad m;
        mean_grad(cam, g, f, cov2d_grad(g, f), m);
        const float (&p)[3] = f.p, (&gT)[2][3] = m.gT, (&gcm)[3] = m.gcm, (&gpt)[3] = m.gpt;
        const float tz = f.cm[2], J00 = f.k2.J[0][0], J02 = f.k2.J[0][2], J11 = f.k2.J[1][1], J12 = f.k2.J[1][2];
        const float txtz = f.k2.txtz, tytz = f.k2.tytz, itz = m.itz, gJ00 = m.gJ00, gJ02 = m.gJ02, gJ11 = m.gJ11, gJ12 = m.gJ12;

        // ---- what the camera contributed: one fp32 term per entry, added in double ----------------------------------------------------------
        // w2c rows 0..2: cm[j] = sum_k p[k] V[4 k + j] + V[12 + j], and T[r][c] = sum_m V[4 c + m] J[r][m] with J's four entries
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            acc[3 * k + 0] += (double)(p[k] * gcm[0] + gT[0][k] * J00);
            acc[3 * k + 1] += (double)(p[k] * gcm[1] + gT[1][k] * J11);
            acc[3 * k + 2] += (double)(p[k] * gcm[2] + (gT[0][k] * J02 + gT[1][k] * J12));
        }
        // w2c row 3 (the translation), full_proj columns 0, 1, 3
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            acc[9 + j] += (double)gcm[j];
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[12 + 3 * k + j] += (double)(p[k] * gpt[j]);
            acc[21 + j] += (double)gpt[j];
        }
        // focal: J00 = fx / z and J02 = -fx t_x / z^2 are linear in fx (t_x = clamp(x / z) z, the forward's: lim_x is held fixed)
        const float tx = fminf(cam.limx, fmaxf(-cam.limx, txtz)) * tz, ty = fminf(cam.limy, fmaxf(-cam.limy, tytz)) * tz;
        const float itz2 = 1.0f / (tz * tz);
        acc[24] += (double)(gJ00 * itz + gJ02 * (-tx * itz2));
        acc[25] += (double)(gJ11 * itz + gJ12 * (-ty * itz2));
    }

    // ---- wave, then workgroup: fixed order ---------------------------------------------------------------------------------------------
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 29; ++k) {
        const double s = wave_sum(acc[k]);
        if (lane == 0) part[wave][k] = s;
    }
    {
        const double s = wave_sum((double)count);
        if (lane == 0) { part[wave][29] = s; part[wave][30] = 0.0; part[wave][31] = 0.0; }
    }
    __syncthreads();
    if (threadIdx.x < CB_SLOTS) {
        double s = part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < CB_THREADS / 64; ++w) s += part[w][threadIdx.x];
        rows[(int64_t)blockIdx.x * CB_SLOTS + threadIdx.x] = s;
    }
}

// rows [groups][32] -> out [32]: thread (run r, slot) sums run r's rows in row order; then the eight runs in run order
__global__ __launch_bounds__(CB_THREADS) void camera_reduce_kernel(const double *__restrict__ rows, int groups, double *__restrict__ out)
{
    __shared__ double part[CB_PARTS][CB_SLOTS];
    const int slot = threadIdx.x & (CB_SLOTS - 1), run = threadIdx.x / CB_SLOTS;
    const int len = (groups + CB_PARTS - 1) / CB_PARTS;
    const int lo = run * len, hi = lo + len < groups ? lo + len : groups;
    double s = 0.0;
    for (int g = lo; g < hi; ++g) s += rows[(int64_t)g * CB_SLOTS + slot];
    part[run][slot] = s;
    __syncthreads();
    if (threadIdx.x < CB_SLOTS) {
        double t = part[0][slot];
#pragma unroll
        for (int r = 1; r < CB_PARTS; ++r) t += part[r][slot];
        out[slot] = t;
    }
}

int launch_camera_backward(const GsrScene &scene, const GsrCamera &cam, const GsrOptions &opts, const float *grad_splat,
                           const float *grad_view_means, double *grad_camera, void *workspace, hipStream_t s)
{
    const int64_t groups = camera_backward_groups(scene.n);
    if (groups == 0) {
        GSR_HIP(hipMemsetAsync(grad_camera, 0, CB_SLOTS * sizeof(double), s));
        return GSR_OK;
    }
    double *rows = static_cast<double *>(workspace);
    hipLaunchKernelGGL(camera_backward_kernel, dim3((unsigned)groups), dim3(CB_THREADS), 0, s, scene, make_cam(cam), opts.reference_compat ? 1 : 0,
                       reinterpret_cast<const float4 *>(grad_splat), grad_view_means, rows);
    GSR_HIP(hipGetLastError());
    hipLaunchKernelGGL(camera_reduce_kernel, dim3(1), dim3(CB_THREADS), 0, s, rows, (int)groups, grad_camera);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

}  // namespace gsr
