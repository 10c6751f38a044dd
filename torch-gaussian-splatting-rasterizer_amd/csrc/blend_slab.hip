// blend_slab.hip — stage 3 for caller-supplied channels between two per-pixel depth limits: pixel p composites the gaussians with
// near[p] <= z_i < far[p] only, out[p][c] = sum_i w_i(p) f_i[c] with T starting at 1 at the near limit (a gaussian in front of it is
// skipped, not blended), and out_final_T[p] the product of (1 - alpha_i) over the same gaussians.  z_i is the gaussian's camera-space
// depth, the float the depth sort orders the lists by.
//
// The kernel is blend_channels_kernel (blend_channels.hip) with one more staged word: the same workgroup (256 threads per 16x16 tile,
// wave = 8x8 quadrant, lane = pixel), the same lists (tile_list_of / tile_list_next), the same staging of the records and the rows,
// the same footprint test by wave ballot, the same launch order, and per channel its arithmetic in its order — w = alpha T,
// C_c = fma(w, f_c, C_c), T = fma(-T, alpha, T).  With open limits every bit of the map and of T is that kernel's, and so are
// wave_entries / fetched_entries.
//
// What is added:
//   - staging: the staging thread loads its gaussian's mean (12 B) and computes z = ((x V2 + y V6) + z V10) + V14 — the preprocess'
//     operations in the preprocess' order (preprocess.hip, geometry_view; that file is built without contraction, here every product
//     passes through an empty asm statement before it is added, so no build flag can fuse it) — into a fifth LDS plane, sZ[256];
//   - prologue: a lane reads its pixel's two limits; the quadrant's far_q = max far and near_q = min near over the pixels that can
//     draw anything (not NaN, near < far) are reduced across the wave once;
//   - ballot: the lane that tests entry e also requires near_q <= z_e < far_q: an entry outside the quadrant's range is never walked
//     and not counted in wave_entries;
//   - walk: a survivor's `valid` gains (z >= near) & (z < far) for the lane's own limits — unless the whole chunk of 64 entries lies
//     inside every pixel's range (near_hi <= z_first, z_last < far_lo; the list is ascending), when the walk is the channel blend's
//     as it stands (the bypass; GSR_SLAB_NO_BYPASS builds the kernel without it for the A/B in tools/slab_ab.py);
//   - stop: a quadrant has finished once every pixel has T <= early_out_T (pixels that can draw nothing do not count), or once a
//     staged entry has z_e >= far_q.  The second rule is exact: the list is ascending in the key bits, the key of a visible gaussian
//     (z >= 0.2) is the bit pattern of z, so every later entry has z >= z_e >= far_q >= far[p] and fails every pixel's test.
// Undrawn lanes (outside the frame, or the last column / row of reference_compat) take the limits of the nearest pixel inside the
// frame and walk along like the channel blend's undrawn lanes do; nothing of theirs is stored.
//
// LDS per workgroup: blend_channels_kernel's + 1 KB (sZ): 9216 + 1024 * CH + 5156 B.
#include <type_traits>
#include "gsr_internal.h"
#include "blend_args.h"
#include "blend_common.h"
#include "blend_channels.h"

namespace gsr {

struct SlabArgs {
    const float *near, *far;  // [H,W] planes in the frame's layout; nullptr: no limit on that side
    const float *means;       // the scene's means; nullptr: the pointer gsr_preprocess left in the control block
    float v2, v6, v10, v14;   // column 2 of the camera's w2c: z_cam = ((x v2 + y v6) + z v10) + v14
};

// A product that no later addition can be fused with.
__device__ __forceinline__ float opaque_mul(float a, float b)
{
    float p = a * b;
    asm volatile("" : "+v"(p));
    return p;
}

// The depth the sort orders by, bit for bit (preprocess.hip: cm[2]).
__device__ __forceinline__ float slab_depth(const SlabArgs &s, float x, float y, float z)
{
    float t = opaque_mul(x, s.v2) + opaque_mul(y, s.v6);
    t = t + opaque_mul(z, s.v10);
    return t + s.v14;
}

// blend_channels_one, and with TEST the lane's own limits in `valid`.
template <int CH, bool TEST>
__device__ __forceinline__ void blend_slab_one(const float2 g, const float4 c, const float L, const float z, const float4 (&f)[CH / 4],
                                               float fpx, float fpy, float near, float far, float &T, float (&acc)[CH])
{
    const float dx = g.x - fpx, dy = g.y - fpy;
    const float p = fmaf(dx, fmaf(c.y, dy, c.x * dx), fmaf(c.z * dy, dy, L));  // log2 domain, opacity folded in
    float alpha = fminf(__builtin_amdgcn_exp2f(p), GSR_MAX_ALPHA);
    bool valid = (alpha > GSR_MIN_ALPHA) & (p <= L);
    if (TEST) valid = valid & (z >= near) & (z < far);  // (a NaN limit fails both)
    alpha = valid ? alpha : 0.0f;
    const float w = alpha * T;
#pragma unroll
    for (int q = 0; q < CH / 4; ++q) {
        acc[4 * q + 0] = fmaf(w, f[q].x, acc[4 * q + 0]);
        acc[4 * q + 1] = fmaf(w, f[q].y, acc[4 * q + 1]);
        acc[4 * q + 2] = fmaf(w, f[q].z, acc[4 * q + 2]);
        acc[4 * q + 3] = fmaf(w, f[q].w, acc[4 * q + 3]);
    }
    T = fmaf(-T, alpha, T);  // what the channel blend's T - w compiles to
}

// waves per SIMD the register allocator aims at: what the LDS lets a CU hold
// The chunk-level bypass: kept at CH = 4 and 8 (DESIGN.md 5.17 has the A/B); at CH = 16 the second copy of the walk costs the kernel
// 16 B of scratch per lane inside the 96 VGPRs its five waves per SIMD leave, and under a bound of four waves it fits (106 VGPRs)
// but measured slower than the compares at five, so that width always compares.
#ifdef GSR_SLAB_NO_BYPASS
template <int CH> struct SlabBypass { static constexpr bool value = false; };
#else
template <int CH> struct SlabBypass { static constexpr bool value = CH <= 8; };
#endif

template <int CH> struct SlabWaves { static constexpr int value = CH <= 4 ? 8 : CH <= 8 ? 7 : 5; };

template <int CH>
__global__ __launch_bounds__(256, SlabWaves<CH>::value) void blend_slab_kernel(BlendArgs args, const ChannelArgs ch, const SlabArgs sl)
{
    static_assert(CH % 4 == 0, "rows of the feature plane are 16-byte words");
    constexpr int Q = CH / 4;
    constexpr bool BYPASS = SlabBypass<CH>::value;
    const BlendArgs a = blend_args_of_view(args);
    __shared__ float4 srec[2][256];
    __shared__ float4 sF[Q][256];
    __shared__ float sL[256], sZ[256];
    __shared__ int s_done;
    __shared__ uint32_t s_ring[TileList<256>::RING], s_wc[2 * TileList<256>::WAVES];
    const BlendLds lds = {srec[0], srec[1], nullptr, s_ring, s_wc, &s_done, nullptr};
    const float4 *const s0 = srec[0], *const s1 = srec[1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    TilePixel t = tile_of_slot(a);
    if (t.tile < 0) return empty_slot(t, tid);  // uniform
    tile_coords<1>(a, lane, wave, t);
    const float fpx = (float)t.px, fpy = (float)t.py;
    const float qx0 = (float)t.qx, qx1 = (float)(t.qx + 7), qy0 = (float)t.qy, qy1 = (float)(t.qy + 7);

    // the lane's limits: its pixel's, or for a lane outside the frame those of the nearest pixel inside (the tile's first pixel is)
    const float INF = __builtin_huge_valf();
    const size_t lpix = frame_pixel(a, t.ty, min(t.px, a.W - 1), min(t.py, a.H - 1));
    const float near = sl.near ? ldg(sl.near, lpix) : -INF, far = sl.far ? ldg(sl.far, lpix) : INF;
    const bool draws = near < far;  // false with a NaN on either side
    // the quadrant's range, over the lanes that can draw anything: [near_q, far_q) holds every entry some lane admits, and an entry
    // in [near_hi, far_lo) is admitted by every lane (empty as soon as one lane draws nothing)
    float near_q = draws ? near : INF, far_q = draws ? far : -INF, near_hi = draws ? near : INF, far_lo = draws ? far : -INF;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        near_q = fminf(near_q, __shfl_xor(near_q, d, 64));
        far_q = fmaxf(far_q, __shfl_xor(far_q, d, 64));
        near_hi = fmaxf(near_hi, __shfl_xor(near_hi, d, 64));
        far_lo = fminf(far_lo, __shfl_xor(far_lo, d, 64));
    }
    auto uniform = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };  // into a scalar register
    near_q = uniform(near_q); far_q = uniform(far_q); near_hi = uniform(near_hi); far_lo = uniform(far_lo);
    const float *const means = sl.means ? sl.means : a.ctrl->col_means;

    float T = 1.0f;
    float acc[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c] = 0.0f;
    uint32_t evaluated = 0;  // wave-uniform
    bool wave_done = false;
    uint32_t fetched = 0;  // workgroup-uniform
    const int nch = ch.nch;
    TileList<256> list = batches_begin<256, false>(a, t, tid, lds);
    for (;;) {
        // next_batch (blend_common.h) with this kernel's planes
        __syncthreads();  // previous batch fully consumed (and s_done initialised); a refilled ring published
        if (s_done == 4) break;  // uniform: every wave has finished
        uint32_t id = 0;
        const int nb = tile_list_next<256>(a, list, s_ring, s_wc, &id);
        if (nb < 0) continue;
        if (nb == 0) break;
        fetched += (uint32_t)nb;
        if (tid < nb) {
            const GaussRec *r = a.rec + id;
            const float *row = ch.features + (size_t)id * (size_t)ch.stride;
            const float *m = means + 3 * (size_t)id;
            srec[0][tid] = r->q0;
            srec[1][tid] = r->q1;
            sL[tid] = ldg(&r->q2.x, 0);
            sZ[tid] = slab_depth(sl, ldg(m, 0), ldg(m, 1), ldg(m, 2));
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // absent channels: not loaded
                if (ch.vec_in && 4 * q + 4 <= nch) {
                    v = ldg4(row, q);
                } else {
                    if (4 * q + 0 < nch) v.x = ldg(row, 4 * q + 0);
                    if (4 * q + 1 < nch) v.y = ldg(row, 4 * q + 1);
                    if (4 * q + 2 < nch) v.z = ldg(row, 4 * q + 2);
                    if (4 * q + 3 < nch) v.w = ldg(row, 4 * q + 3);
                }
                sF[q][tid] = v;
            }
        }
        __syncthreads();
        if (wave_done) continue;
        for (int chunk = 0; chunk < nb; chunk += 64) {
            const int e = chunk + lane;
            const float ze = e < nb ? sZ[e] : -INF;
            const bool hit = e < nb && footprint_hits_rect(s0[e], s1[e], qx0, qx1, qy0, qy1) && near_q <= ze && ze < far_q;
            const bool past = __any(ze >= far_q);  // this entry and every later one lie behind every pixel's far limit
            unsigned long long m = __ballot(hit);
            evaluated += (uint32_t)__popcll(m);
            // the survivors, two per trip so that the second one's LDS reads overlap the first one's arithmetic, an odd one out last
            // (blend_channels_kernel's walk); test_c: the lanes compare the entry's depth with their own limits
            auto walk = [&](auto test_c) __attribute__((always_inline)) {
                constexpr bool TEST = decltype(test_c)::value;
                while (m & (m - 1)) {
                    const int k0 = chunk + (__ffsll((long long)m) - 1);
                    m &= m - 1;
                    const int k1 = chunk + (__ffsll((long long)m) - 1);
                    m &= m - 1;
                    const float2 ga = *reinterpret_cast<const float2 *>(&s0[k0]);  // wave-uniform address: LDS broadcast
                    const float4 ca = s1[k0];
                    const float La = sL[k0];
                    const float za = TEST ? sZ[k0] : 0.0f;
                    float4 fa[Q];
#pragma unroll
                    for (int q = 0; q < Q; ++q) fa[q] = sF[q][k0];
                    asm volatile("" ::"v"(ca.w));  // keep the read a ds_read_b128 (4 LDS cycles); a b96 costs 8
                    const float2 gb = *reinterpret_cast<const float2 *>(&s0[k1]);
                    const float4 cb = s1[k1];
                    const float Lb = sL[k1];
                    const float zb = TEST ? sZ[k1] : 0.0f;
                    float4 fb[Q];
#pragma unroll
                    for (int q = 0; q < Q; ++q) fb[q] = sF[q][k1];
                    asm volatile("" ::"v"(cb.w));
                    blend_slab_one<CH, TEST>(ga, ca, La, za, fa, fpx, fpy, near, far, T, acc);
                    blend_slab_one<CH, TEST>(gb, cb, Lb, zb, fb, fpx, fpy, near, far, T, acc);
                }
                if (m) {
                    const int k0 = chunk + (__ffsll((long long)m) - 1);
                    const float2 ga = *reinterpret_cast<const float2 *>(&s0[k0]);
                    const float4 ca = s1[k0];
                    const float La = sL[k0];
                    const float za = TEST ? sZ[k0] : 0.0f;
                    float4 fa[Q];
#pragma unroll
                    for (int q = 0; q < Q; ++q) fa[q] = sF[q][k0];
                    asm volatile("" ::"v"(ca.w));
                    blend_slab_one<CH, TEST>(ga, ca, La, za, fa, fpx, fpy, near, far, T, acc);
                }
            };
            // every pixel of the quadrant admits every entry of the chunk: the first is the nearest, the last the farthest
            if (BYPASS && near_hi <= sZ[chunk] && sZ[min(chunk + 63, nb - 1)] < far_lo) walk(std::false_type{});  // uniform
            else walk(std::true_type{});
            if (past || __all((T <= a.early_T) | !draws)) {  // T: FeatureBlend's rule (a negative threshold never fires)
                wave_done = true;
                wave_finished(lds, lane);
                break;
            }
        }
    }

    blend_stats_out<256, false>(a, t, tid, lane, wave, lds, evaluated, fetched, 0u);
    if (t.px < a.W && t.py < a.H) {
        const bool drawn = t.px < a.xlim && t.py < a.ylim;  // Q1: last column / row stay zero, T stays 1
        const size_t pix = frame_pixel(a, t.ty, t.px, t.py);
        float *o = static_cast<float *>(a.out) + pix * (size_t)ch.channels + ch.c0;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const float4 v = make_float4(drawn ? acc[4 * q] : 0.0f, drawn ? acc[4 * q + 1] : 0.0f, drawn ? acc[4 * q + 2] : 0.0f,
                                         drawn ? acc[4 * q + 3] : 0.0f);
            if (ch.vec_out && 4 * q + 4 <= nch) {
                reinterpret_cast<float4 *>(o)[q] = v;
            } else {
                if (4 * q + 0 < nch) o[4 * q + 0] = v.x;
                if (4 * q + 1 < nch) o[4 * q + 1] = v.y;
                if (4 * q + 2 < nch) o[4 * q + 2] = v.z;
                if (4 * q + 3 < nch) o[4 * q + 3] = v.w;
            }
        }
        if (a.out_T) a.out_T[pix] = drawn ? T : 1.0f;
    }
}

template <int CH>
static void launch_width(int slots, const BlendArgs &a, const ChannelArgs &ch, const SlabArgs &sl, hipStream_t s)
{
    hipLaunchKernelGGL(blend_slab_kernel<CH>, dim3((unsigned)slots), dim3(256), 0, s, a, ch, sl);
}

// The instantiated widths: a map of up to 4 channels takes one walk of 4, up to 8 one of 8, a wider one walks of 16 with the rest
// in the narrowest width that holds it (launch_blend_channels' rule with one more width below it).
int launch_blend_slab(const GsrCamera &cam, const GsrOptions &opts, const Workspace &ws, const FramePlan &plan, const float *means,
                      const float *features, int channels, int64_t stride, const float *depth_near, const float *depth_far,
                      float *out_map, float *out_T, hipStream_t s)
{
    if (ws.views > 1) { set_error("feature maps: single views only"); return GSR_ERR_BAD_ARG; }
    BlendArgs a = blend_args_common(cam, opts, ws, plan, out_map, out_T);  // tile_work stays null: never written here
    if (a.rows <= 0 || a.tiles_x <= 0) return GSR_OK;
    const SlabArgs sl = {depth_near, depth_far, means, cam.w2c[2], cam.w2c[6], cam.w2c[10], cam.w2c[14]};
    // heaviest tiles first, by what the last colour blend on this workspace staged where that is known (a schedule only)
    const int slots = launch_tile_order(ws, plan, true, s);
    for (int c0 = 0; c0 < channels;) {
        const int rest = channels - c0;
        const int width = rest > 8 ? 16 : rest > 4 ? 8 : 4;
        ChannelArgs ch;
        ch.features = features + c0;
        ch.stride = stride;
        ch.channels = channels;
        ch.c0 = c0;
        ch.nch = rest < width ? rest : width;
        // 16-byte accesses where every row / pixel of this group starts on a 16-byte boundary
        ch.vec_in = reinterpret_cast<uintptr_t>(ch.features) % 16 == 0 && stride % 4 == 0;
        ch.vec_out = reinterpret_cast<uintptr_t>(out_map + c0) % 16 == 0 && channels % 4 == 0;
        if (width == 16) launch_width<16>(slots, a, ch, sl, s);
        else if (width == 8) launch_width<8>(slots, a, ch, sl, s);
        else launch_width<4>(slots, a, ch, sl, s);
        GSR_HIP(hipGetLastError());
        a.out_T = nullptr;  // every group ends with the same T: the first one's store is enough
        c0 += ch.nch;
    }
    return GSR_OK;
}

}  // namespace gsr
