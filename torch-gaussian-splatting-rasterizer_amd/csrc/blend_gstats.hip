// blend_gstats.hip — per-gaussian statistics of one view, over the pixels p the caller counts:
//   weight_sum[i] += sum_p w_i(p)      weight_max[i] = max(weight_max[i], max_p w_i(p))      pixels[i] += #{p : w_i(p) > 0}
// with the forward's weights w_i = alpha_i T_i.  The sum is what blend_channels_backward.hip gives for a one-channel map of ones;
// the maximum and the count are no sum_p w G[p] and need this kernel.
//
// The workgroup, the batch loop, the survivor walk (one per trip) and the weight are blend_weight_walk.h's, with
// blend_channels_backward_kernel's staging, stop rule and flush after a batch: w and T are the forward's bit for bit.
//
// What differs:
//   per lane      no gradient registers: one predicate `counted` — false outside the frame, in Q1's undrawn last column / row (where
//                 the forward stores 0) and where the caller's pixel mask holds 0.  w' = counted ? w : 0; T moves with the unmasked
//                 alpha for every pixel, so the stop rule fires where the forward's does;
//   per survivor  b = ballot(w' != 0); nothing more if b == 0.  pixels: popcount(b), scalar.  sum and max: w' over the wave's 64
//                 lanes by six DPP steps each (row_shr 1 / 2 / 4 / 8, row_bcast 15 / 31), v_add_f32 for the one and v_max_u32 on
//                 the bit patterns for the other (non-negative floats order like their bits), the two chains interleaved.
//                 bound_ctrl's 0 is the identity of both: w' >= +0.  Lane 63 folds the three into the entry's row of the LDS plane
//                 sS with ds_add_f32, ds_max_u32 and ds_add_u32, and marks the row (a plain store of 1 into its fourth word: every
//                 writer writes the same);
//   per batch     after the barrier that ends the batch's consumption thread e < nb takes entry e: a marked row goes to the caller's
//                 arrays with global_atomic_add_f32, global_atomic_umax and global_atomic_add (one dword per row and array: the shape
//                 of the gradient kernel's one-channel flush) and back to zero.  Unmarked rows cost no atomic;
//   outputs       WANT (template parameter, bit 0 sum, 1 max, 2 pixels) removes an absent output's chain, LDS atomic and global
//                 atomic at compile time: seven instantiations (each once more with HITS, below);
//   masked waves  a wave none of whose 64 pixels is counted has finished before its first batch (exact: every w' is 0), and a tile
//                 whose four waves have stages nothing: a small region of interest costs what it covers.
//
// LDS per workgroup, 256 staged entries:
//   s0, s1 [256] float4, sL [256] float   as in blend_channels_backward.hip
//   sId [256] uint32                       the staged gaussian ids
//   sS  [256] uint4                        {sum, max (float bits), pixels, mark}: three words padded to four, so that a row is one
//                                          16-byte read in the flush and its index a shift
//   ring [1024] + wc [8] + done: tile_list_next's
// = 8192 + 1024 + 1024 + 4096 + 4132 B = 18.0 KB: LDS allows 8 workgroups per CU, and so do the registers (launch bound 8).
// Max and pixels do not depend on the order the atomics arrive in: two runs give the same bits.  The float sums may differ in
// their last bits.
//
// Several views per launch (gridDim.y, gsr_blend_gaussian_stats_views): view blockIdx.y walks its slice of the workspace
// (blend_args_of_view) and reads its own mask plane; all views flush into the same three arrays with the same atomics.  view_hits[i]
// += the views that reach gaussian i with w > 0 in a counted pixel: in the flush a marked row also does atomicOr(view_bits + i,
// 1 << blockIdx.y) and, if the bit was clear in the value that came back, atomicAdd(view_hits + i, 1) — exactly one flush per
// (gaussian, view) finds it clear, whatever the order.  view_bits is the caller's scratch, cleared by the host before the launch.
// An absent view_hits is a template bit, HITS, like WANT: without it the flush is the single-view kernel's, instruction for
// instruction, and so are the registers.
// Fifteen instantiations: WANT 1 .. 7 with and without HITS, and WANT = 0 with it — view_hits alone.  With gridDim.y == 1 every
// view offset is zero.
#include "blend_weight_walk.h"

namespace gsr {

struct GaussStatsArgs {
    const uint8_t *mask;   // one byte per pixel in the frame's layout, non-zero = counted; null: every drawn pixel
    float *weight_sum;     // [n], null unless WANT & 1
    uint32_t *weight_max;  // [n] float bits, null unless WANT & 2
    uint32_t *pixels;      // [n], null unless WANT & 4
    // several views per launch (gridDim.y): view blockIdx.y reads its own mask plane and all views add into the outputs above
    int64_t mask_view_stride;  // bytes between the views' mask planes
    uint32_t *view_hits;   // [n] += the views of this launch that reach the gaussian with w > 0 in a counted pixel; may be null
    uint32_t *view_bits;   // [n] scratch, cleared by the host before the launch: bit v = view v has been counted in view_hits
};

constexpr int WANT_SUM = 1, WANT_MAX = 2, WANT_PIXELS = 4;

// dpp_add's counterpart for the maximum; lanes without a source lane take 0 (bound_ctrl), the identity of both for x >= +0
// (the maximum of the BIT PATTERNS, v_max_u32: for floats >= +0 that is the float maximum, and fmaxf would first quiet each operand
// with a v_max_f32 x, x of its own — three issues a step instead of one)
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_max(uint32_t x)
{
    const uint32_t y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true);
    return x > y ? x : y;
}

// The wave's sum of s and maximum of m, left in lane 63 (blend_channels_backward.hip's wave_sum4, two chains instead of four)
template <int WANT>
__device__ __forceinline__ void wave_sum_max(float &s, uint32_t &m)
{
#define GSR_STEP(CTRL)                            \
    if (WANT & WANT_SUM) s = dpp_add<CTRL>(s);    \
    if (WANT & WANT_MAX) m = dpp_max<CTRL>(m);
    GSR_STEP(0x111) GSR_STEP(0x112) GSR_STEP(0x114) GSR_STEP(0x118) GSR_STEP(0x142) GSR_STEP(0x143)
#undef GSR_STEP
}

// One survivor's weights w: the wave's three statistics into the entry's row.
template <int WANT>
__device__ __forceinline__ void gstats_add(float w, bool counted, int lane, uint32_t *row)
{
    const float wc = counted ? w : 0.0f;
    const unsigned long long b = __ballot(wc != 0.0f);
    if (b == 0) return;  // uniform: nothing to record for any pixel of the quadrant
    float s = wc;
    uint32_t m = __float_as_uint(wc);
    wave_sum_max<WANT>(s, m);
    if (lane == 63) {  // (row is a per-lane value to the compiler: see the call)
        if (WANT & WANT_SUM) atomicAdd(reinterpret_cast<float *>(row), s);
        if (WANT & WANT_MAX) atomicMax(row + 1, m);
        if (WANT & WANT_PIXELS) atomicAdd(row + 2, (uint32_t)__popcll(b));
        row[3] = 1u;
    }
}

template <int WANT, bool HITS>
__global__ __launch_bounds__(256, 8) void blend_gstats_kernel(BlendArgs args, const GaussStatsArgs gs)
{
    static_assert(WANT >= 0 && WANT <= 7 && (WANT != 0 || HITS), "at least one output; WANT 0: view_hits alone");
    const BlendArgs a = blend_args_of_view(args);
    __shared__ float4 srec[2][256];
    __shared__ uint4 sS[256];
    __shared__ float sL[256];
    __shared__ uint32_t sId[256];
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

    // does this pixel count?  Not where the forward stores 0 (Q1's last column / row) or nothing (outside the frame), nor where the
    // caller's mask says so
    bool counted = t.px < a.W && t.py < a.H && t.px < a.xlim && t.py < a.ylim;
    if (counted && gs.mask) counted = ldg(gs.mask, (size_t)blockIdx.y * (size_t)gs.mask_view_stride + frame_pixel(a, t.ty, t.px, t.py)) != 0;
    sS[tid] = make_uint4(0u, 0u, 0u, 0u);  // published by the barrier below

    float T = 1.0f;
    uint32_t evaluated = 0;  // wave-uniform
    bool wave_done = false;
    uint32_t fetched = 0;  // workgroup-uniform
    TileList<256> list = batches_begin<256, false>(a, t, tid, lds);
    __syncthreads();  // s_done is initialised: a wave with nothing to count may say so at once
    if (!__any(counted)) {
        wave_done = true;
        wave_finished(lds, lane);
    }
    struct Entry { float2 g; float4 c; float L; int k; };
    auto stage = [&](uint32_t id, const GaussRec *r) __attribute__((always_inline)) {
        sL[tid] = ldg(&r->q2.x, 0);
        sId[tid] = id;
    };
    auto read = [&](int k) __attribute__((always_inline)) {
        const Entry en = {*reinterpret_cast<const float2 *>(&s0[k]), s1[k], sL[k], k};
        keep_b128(en.c);
        return en;
    };
    auto eval = [&](const Entry &en) __attribute__((always_inline)) {
        // the row's index goes through a vector register the compiler cannot see through: for an address it knows to be
        // wave-uniform it wraps every LDS atomic into a loop that first reduces the values of the active lanes
        int at = en.k;
        asm volatile("" : "+v"(at));
        const float w = blend_weight(en.g, en.c, en.L, fpx, fpy, T);
        gstats_add<WANT>(w, counted, lane, reinterpret_cast<uint32_t *>(&sS[at]));
    };
    // (the loop's top barrier: previous batch consumed AND flushed; the finished waves' count published)
    while (const int nb = next_batch_planes<256>(a, list, tid, lds, fetched, stage)) {
        if (!wave_done) {
            for (int chunk = 0; chunk < nb; chunk += 64) {
                const int e = chunk + lane;
                const bool hit = e < nb && footprint_hits_rect(s0[e], s1[e], qx0, qx1, qy0, qy1);
                const unsigned long long m = __ballot(hit);
                evaluated += (uint32_t)__popcll(m);
                walk_survivors_single(m, chunk, read, eval);
                if (__all(T <= a.early_T)) {  // the forward's stop rule, where the forward evaluates it
                    wave_done = true;
                    wave_finished(lds, lane);
                    break;
                }
            }
        }
        __syncthreads();  // every wave is through with the batch: sS is final
        // flush: thread e takes entry e; a marked row goes to the caller's arrays and back to zero
        if (tid < nb) {
            const uint4 r = sS[tid];
            if (r.w) {
                const size_t i = sId[tid];
                if (WANT & WANT_SUM) unsafeAtomicAdd(gs.weight_sum + i, __uint_as_float(r.x));
                if (WANT & WANT_MAX) atomicMax(gs.weight_max + i, r.y);
                if (WANT & WANT_PIXELS) atomicAdd(gs.pixels + i, r.z);
                if (HITS) {  // the first flush of this view that reaches gaussian i finds the view's bit clear
                    const uint32_t bit = 1u << blockIdx.y;
                    if (!(atomicOr(gs.view_bits + i, bit) & bit)) atomicAdd(gs.view_hits + i, 1u);
                }
                sS[tid] = make_uint4(0u, 0u, 0u, 0u);
            }
        }
    }

    blend_stats_out<256, false>(a, t, tid, lane, wave, lds, evaluated, fetched, 0u);
}

template <int WANT, bool HITS>
static void launch_one(int slots, int views, const BlendArgs &a, const GaussStatsArgs &gs, hipStream_t s)
{
    hipLaunchKernelGGL((blend_gstats_kernel<WANT, HITS>), dim3((unsigned)slots, (unsigned)views), dim3(256), 0, s, a, gs);
}

template <int WANT>
static void launch_want(int slots, int views, const BlendArgs &a, const GaussStatsArgs &gs, hipStream_t s)
{
    if (gs.view_hits) launch_one<WANT, true>(slots, views, a, gs, s);
    else launch_one<WANT, false>(slots, views, a, gs, s);
}

int launch_blend_gstats(const GsrCamera &cam, const GsrOptions &opts, const Workspace &ws, const FramePlan &plan, const uint8_t *pixel_mask,
                        float *weight_sum, float *weight_max, uint32_t *pixels, hipStream_t s, int64_t mask_view_stride,
                        uint32_t *view_hits, uint32_t *view_bits)
{
    BlendArgs a;  // no map is written
    int slots;
    const int rc = weight_walk_begin("gaussian statistics", cam, opts, ws, plan, nullptr, nullptr, s, &a, &slots, WalkViews::Several);
    if (rc || !slots) return rc;
    const GaussStatsArgs gs = {pixel_mask, weight_sum, reinterpret_cast<uint32_t *>(weight_max), pixels, mask_view_stride, view_hits, view_bits};
    const int views = ws.views;
    switch ((weight_sum ? WANT_SUM : 0) | (weight_max ? WANT_MAX : 0) | (pixels ? WANT_PIXELS : 0)) {
    case 1: launch_want<1>(slots, views, a, gs, s); break;
    case 2: launch_want<2>(slots, views, a, gs, s); break;
    case 3: launch_want<3>(slots, views, a, gs, s); break;
    case 4: launch_want<4>(slots, views, a, gs, s); break;
    case 5: launch_want<5>(slots, views, a, gs, s); break;
    case 6: launch_want<6>(slots, views, a, gs, s); break;
    case 7: launch_want<7>(slots, views, a, gs, s); break;
    default:
        if (!view_hits) { set_error("null statistics outputs: all three"); return GSR_ERR_BAD_ARG; }
        launch_one<0, true>(slots, views, a, gs, s);
    }
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

}  // namespace gsr
