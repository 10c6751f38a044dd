// blend_slab.hip — stage 3 for caller-supplied channels between two per-pixel depth limits: pixel p composites the gaussians with
// near[p] <= z_i < far[p] only, out[p][c] = sum_i w_i(p) f_i[c] with T starting at 1 at the near limit (a gaussian in front of it is
// skipped, not blended), and out_final_T[p] the product of (1 - alpha_i) over the same gaussians.  z_i is the gaussian's camera-space
// depth, the float the depth sort orders the lists by.
//
// The kernel is blend_channels_kernel (blend_channels.hip) with one more staged word, built from the same pieces
// (blend_weight_walk.h): workgroup, batch loop, staging of the rows, survivor walk, weight and channel update.  With open limits
// every bit of the map and of T is that kernel's, and so are wave_entries / fetched_entries.
//
// What is added:
//   - staging: the staging thread loads its gaussian's mean (12 B) and computes z = ((x V2 + y V6) + z V10) + V14 — the preprocess'
//     operations in the preprocess' order (gauss_math.h, cam_z; preprocess.hip is built without contraction, here every product
//     passes through an empty asm statement before it is added, so no build flag can fuse it) — into a fifth LDS plane, sZ[256];
//   - prologue: a lane reads its pixel's two limits; the quadrant's far_q = max far and near_q = min near over the pixels that can
//     draw anything (not NaN, near < far) are reduced across the wave once;
//   - ballot: the lane that tests entry e also requires near_q <= z_e < far_q: an entry outside the quadrant's range is never walked
//     and not counted in wave_entries;
//   - walk: a survivor's `valid` gains (z >= near) & (z < far) for the lane's own limits (blend_weight's `admit`) — unless the whole
//     chunk of 64 entries lies inside every pixel's range (near_hi <= z_first, z_last < far_lo; the list is ascending), when the
//     walk is the channel blend's as it stands (the bypass; GSR_SLAB_NO_BYPASS builds the kernel without it for the A/B in
//     tools/slab_ab.py);
//   - stop: a quadrant has finished once every pixel has T <= early_out_T (pixels that can draw nothing do not count), or once a
//     staged entry has z_e >= far_q.  The second rule is exact: the list is ascending in the key bits, the key of a visible gaussian
//     (z >= 0.2) is the bit pattern of z, so every later entry has z >= z_e >= far_q >= far[p] and fails every pixel's test.
// Undrawn lanes (outside the frame, or the last column / row of reference_compat) take the limits of the nearest pixel inside the
// frame and walk along like the channel blend's undrawn lanes do; nothing of theirs is stored.
//
// LDS per workgroup: blend_channels_kernel's + 1 KB (sZ): 9216 + 1024 * CH + 5156 B.
#include <type_traits>
#include "blend_weight_walk.h"

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
    struct Entry { float2 g; float4 c; float L, z; float4 f[Q]; };
    auto stage = [&](uint32_t id, const GaussRec *r) __attribute__((always_inline)) {
        const float *m = means + 3 * (size_t)id;
        sL[tid] = ldg(&r->q2.x, 0);
        sZ[tid] = slab_depth(sl, ldg(m, 0), ldg(m, 1), ldg(m, 2));
        const ChannelRow<Q> row = load_channel_row<Q>(ch.features + (size_t)id * (size_t)ch.stride, nch, ch.vec_in);
#pragma unroll
        for (int q = 0; q < Q; ++q) sF[q][tid] = row.v[q];
    };
    while (const int nb = next_batch_planes<256>(a, list, tid, lds, fetched, stage)) {
        if (wave_done) continue;
        for (int chunk = 0; chunk < nb; chunk += 64) {
            const int e = chunk + lane;
            const float ze = e < nb ? sZ[e] : -INF;
            const bool hit = e < nb && footprint_hits_rect(s0[e], s1[e], qx0, qx1, qy0, qy1) && near_q <= ze && ze < far_q;
            const bool past = __any(ze >= far_q);  // this entry and every later one lie behind every pixel's far limit
            const unsigned long long m = __ballot(hit);
            evaluated += (uint32_t)__popcll(m);
            // the channel blend's walk; test_c: the lanes compare the entry's depth with their own limits (a NaN limit fails both)
            auto walk = [&](auto test_c) __attribute__((always_inline)) {
                constexpr bool TEST = decltype(test_c)::value;
                walk_survivors(m, chunk,
                    [&](int k) __attribute__((always_inline)) {
                        Entry en;
                        en.g = *reinterpret_cast<const float2 *>(&s0[k]);
                        en.c = s1[k];
                        en.L = sL[k];
                        en.z = TEST ? sZ[k] : 0.0f;
#pragma unroll
                        for (int q = 0; q < Q; ++q) en.f[q] = sF[q][k];
                        keep_b128(en.c);
                        return en;
                    },
                    [&](const Entry &en) __attribute__((always_inline)) {
                        const bool admit = !TEST || ((en.z >= near) & (en.z < far));
                        blend_channels_add<Q>(blend_weight(en.g, en.c, en.L, fpx, fpy, T, admit), en.f, acc);
                    });
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
        store_channel_pixel<Q>(static_cast<float *>(a.out) + pix * (size_t)ch.channels + ch.c0, acc, nch, ch.vec_out, drawn);
        if (a.out_T) a.out_T[pix] = drawn ? T : 1.0f;
    }
}

template <int CH>
static void launch_width(int slots, const BlendArgs &a, const ChannelArgs &ch, const SlabArgs &sl, hipStream_t s)
{
    hipLaunchKernelGGL(blend_slab_kernel<CH>, dim3((unsigned)slots), dim3(256), 0, s, a, ch, sl);
}

// The instantiated widths: for_channel_groups' with 4 as the narrowest — a map of up to 4 channels takes one walk of 4.
int launch_blend_slab(const GsrCamera &cam, const GsrOptions &opts, const Workspace &ws, const FramePlan &plan, const float *means,
                      const float *features, int channels, int64_t stride, const float *depth_near, const float *depth_far,
                      float *out_map, float *out_T, hipStream_t s)
{
    BlendArgs a;
    int slots;
    const int rc = weight_walk_begin("feature maps", cam, opts, ws, plan, out_map, out_T, s, &a, &slots);
    if (rc || !slots) return rc;
    const SlabArgs sl = {depth_near, depth_far, means, cam.w2c[2], cam.w2c[6], cam.w2c[10], cam.w2c[14]};
    return for_channel_groups(features, stride, out_map, channels, 4, [&](const ChannelArgs &ch, int width) -> int {
        if (width == 16) launch_width<16>(slots, a, ch, sl, s);
        else if (width == 8) launch_width<8>(slots, a, ch, sl, s);
        else launch_width<4>(slots, a, ch, sl, s);
        GSR_HIP(hipGetLastError());
        a.out_T = nullptr;  // every group ends with the same T: the first one's store is enough
        return GSR_OK;
    });
}

}  // namespace gsr
