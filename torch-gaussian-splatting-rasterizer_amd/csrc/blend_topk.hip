// blend_topk.hip — stage 3 for per-pixel contributor LISTS: of a pixel's depth-ordered list, with the weights w_i = alpha_i T_i of the
// colour frame,
//   - HEAVIEST: the k gaussians of largest weight, heaviest first (only w > 0 enters; at exactly equal weights the earlier one in
//     draw order comes first, so a later one that ties the k-th does not displace it: best_id's strict compare, generalised);
//   - NEAREST:  the first k gaussians in draw order with w > 0, nearest first;
// ids and weights, k <= GSR_MAX_TOPK, unused slots -1 / 0.  A per-pixel gather like the pick maps: no atomics, nothing per gaussian
// is written.
//
// The workgroup, the survivor walk and the weight w = alpha T with its T are blend_weight_walk.h's, the staging
// ({q0, q1, {log2 opacity, id}}) blend_pick_kernel's: w and T are the feature blend's, bit for bit.
// In the place of the argmax each lane keeps K weights and K ids in registers; K is instantiated at 4, 8 and 16, a request for k runs
// the smallest K >= k and stores k slots.
//
// HEAVIEST — branch-free sorted insertion.  The list is sorted descending, so g_j = (w > wk[j]) is monotone in j (false ... true),
// and with the OLD values, walking j from K - 1 down to 0,   wk[j] = g_j ? (g_{j-1} ? wk[j-1] : w) : wk[j]   (g_{-1} = false):
// slots behind the insertion point take their left neighbour, the first slot w beats takes w, the ones before stay.  The ids move
// under the same masks.  That is a compare and four selects per slot, ~5K vector instructions per survivor on top of the ~14 that
// give w; once the lists have filled most survivors insert nothing, so the insertion sits behind a wave-uniform
// `if (__any(w > wk[K-1]))` (GSR_TOPK_NO_GUARD builds the unguarded form for the measurement in DESIGN.md §5.16).
// A request for k < K uses the LAST k slots: slots 0 .. K-k-1 start at +inf, which no weight beats (g_j false, so the slot right of
// them takes w itself), and slots K-k .. K-1 are a sorted list of length k whose last slot — the k-th weight, which the guard and the
// stop rule look at — is wk[K-1] for every k.  Looking at slot k - 1 of a left-aligned list instead needs a select chain over the
// slots on every insertion, and the compiler folds every form of that chain tried here (`k - 1 == j`, the bits of 1 << (k - 1))
// back into one load at a runtime index: the lists then leave the registers for LDS or scratch.  Before the store the lists move
// K - k slots to the left, in up to three uniform power-of-two steps (K - k <= 7: a k that needs more runs the next smaller K).
// NEAREST — append: a `filled` counter per lane and, per slot j, `take & (filled == j)` selects w and the id into it; no slot is
// addressed by a runtime index (that would put the lists into scratch).  Behind `if (__any(take & (filled < k)))`.
//
// When has the walk of a quadrant stopped mattering?
//   - with out_final_T: when T <= early_T for its 64 pixels, the feature blend's rule where blend_kernel evaluates it, because T
//     itself is an output.  wave_entries / fetched_entries are the feature blend's.
//   - without: by that rule, or when every one of its pixels has a list that cannot change:
//       HEAVIEST  T <= wk[K-1], the k-th weight.  A later entry's w' = fl(alpha' T') <= T' (alpha <= 0.99 < 1, rounding is
//                 monotone and T' is a float), and T never grows (T' = fl(T - alpha T) <= T), so w' <= T' <= T <= wk[K-1]: the
//                 strict `w' > wk[K-1]` fails for this entry and, T only shrinking and wk[K-1] only growing, for every later one
//                 (the pick kernel's argument for best_w).  T == 0 is the special case wk[K-1] >= 0.
//       NEAREST   the k-th slot is filled, or T == 0 (no later w is > 0).  A pixel HEAVIEST has finished has k weights > 0 or T == 0,
//                 so NEAREST never walks further than HEAVIEST.
//       pixels whose lists are never stored (outside the frame, the undrawn last column / row of reference_compat): from the start.
//     The two conditions are tested per quadrant, not mixed per pixel: a pixel below early_T whose list could still change keeps
//     being fed for as long as the feature blend would feed it, so at early_T > 0 the lists are the top k of exactly the weights
//     the feature blend composites at that early_T — with or without out_final_T.
// Everything is exact at early_T = 0; early_T > 0 is the feature blend's approximation (entries behind T <= early_T are not seen).
//
// LDS per workgroup is blend_pick_kernel's 14.4 KB.  Registers: the lists are 2K VGPRs, so the launch bound is per K — 8 waves per
// SIMD (64 VGPRs) at K = 4, 6 (80) at K = 8, 4 (128) at K = 16; no instantiation uses scratch (tools/kernel_resources.sh
// blend_topk.hip; the table is in DESIGN.md §5.16).
// The record's colour words are neither read nor written and tile_work is only read, as in blend_pick.hip.
#include "blend_weight_walk.h"

namespace gsr {

struct TopkArgs {
    int32_t *ids;      // [.., k] in the frame's layout; one of ids / weights may be null
    float *weights;    // [.., k]
    float *final_T;    // [..] or null: null lets a quadrant stop once its lists cannot change
    int k;             // 1 .. K slots are stored
    int vec;           // k % 4 == 0 and both planes 16-byte aligned: 16-byte stores
};

// Both lists S slots to the left (S a power of two; what comes in at the far end is never stored)
template <int K, int S>
__device__ __forceinline__ void topk_shift(float (&wk)[K], int (&ik)[K])
{
#pragma unroll
    for (int j = 0; j + S < K; ++j) { wk[j] = wk[j + S]; ik[j] = ik[j + S]; }
}

template <int K>
__device__ __forceinline__ void topk_insert(float (&wk)[K], int (&ik)[K], float w, int id)
{
#pragma unroll
    for (int j = K - 1; j >= 1; --j) {
        const bool g = w > wk[j], gl = w > wk[j - 1];  // strict: on equal weights the earlier one in draw order stays in front
        wk[j] = g ? (gl ? wk[j - 1] : w) : wk[j];
        ik[j] = g ? (gl ? ik[j - 1] : id) : ik[j];
    }
    const bool g0 = w > wk[0];
    wk[0] = g0 ? w : wk[0];
    ik[0] = g0 ? id : ik[0];
}

template <int K>
__device__ __forceinline__ void topk_append(float (&wk)[K], int (&ik)[K], int &filled, float w, int id)
{
    const bool take = w > 0.0f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const bool here = take & (filled == j);
        wk[j] = here ? w : wk[j];
        ik[j] = here ? id : ik[j];
    }
    filled += take ? 1 : 0;  // (past K nothing matches any more)
}

// one survivor's weight into the lists
template <int K, bool NEAREST>
__device__ __forceinline__ void topk_take(float (&wk)[K], int (&ik)[K], int &filled, int k, float w, int id)
{
    if (NEAREST) {
#ifndef GSR_TOPK_NO_GUARD
        if (__any((w > 0.0f) & (filled < k)))
#endif
            topk_append<K>(wk, ik, filled, w, id);
    } else {
#ifndef GSR_TOPK_NO_GUARD
        if (__any(w > wk[K - 1]))
#endif
            topk_insert<K>(wk, ik, w, id);
    }
}

constexpr int topk_min_waves(int K) { return K <= 4 ? 8 : K <= 8 ? 6 : 4; }

template <int K, bool NEAREST>
__global__ __launch_bounds__(256, topk_min_waves(K)) void blend_topk_kernel(BlendArgs args, const TopkArgs tk)
{
    const BlendArgs a = blend_args_of_view(args);
    __shared__ float4 srec[2][256];
    __shared__ float2 sP[256];
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
    const int k = tk.k;
    const bool lists_only = tk.final_T == nullptr;  // uniform

    float T = 1.0f;
    float wk[K];
    int ik[K], filled = 0;
    const int pad = NEAREST ? 0 : K - k;  // HEAVIEST: the k slots in use are the LAST k (see the comment at the top)
#pragma unroll
    for (int j = 0; j < K; ++j) { wk[j] = j < pad ? __builtin_inff() : 0.0f; ik[j] = -1; }
    const bool drawn = t.px < a.xlim && t.py < a.ylim;  // Q1: the last column / row are never drawn (xlim <= W, ylim <= H)
    uint32_t evaluated = 0;  // wave-uniform
    bool wave_done = false;
    uint32_t fetched = 0;  // workgroup-uniform
    TileList<256> list = batches_begin<256, false>(a, t, tid, lds);
    struct Entry { float2 g; float4 c; float2 o; };
    auto read = [&](int k) __attribute__((always_inline)) {
        const Entry en = {*reinterpret_cast<const float2 *>(&s0[k]), s1[k], sP[k]};
        keep_b128(en.c);
        return en;
    };
    auto eval = [&](const Entry &en) __attribute__((always_inline)) {
        const float w = blend_weight(en.g, en.c, en.o.x, fpx, fpy, T);
        topk_take<K, NEAREST>(wk, ik, filled, k, w, __float_as_int(en.o.y));
    };
    // a trip's two: both weights (and T) first, in draw order, then the two go to the lists in that order
    auto eval2 = [&](const Entry &ea, const Entry &eb) __attribute__((always_inline)) {
        const float wa = blend_weight(ea.g, ea.c, ea.o.x, fpx, fpy, T);
        const float wb = blend_weight(eb.g, eb.c, eb.o.x, fpx, fpy, T);
        topk_take<K, NEAREST>(wk, ik, filled, k, wa, __float_as_int(ea.o.y));
        topk_take<K, NEAREST>(wk, ik, filled, k, wb, __float_as_int(eb.o.y));
    };
    for (;;) {
        // next_batch_planes (blend_weight_walk.h), spelled out: through the shared function the loop keeps more lane masks in
        // scalar registers, the K = 4 kernels run out of the 80 their eight waves per SIMD leave them and park six of them in a
        // vector register of their own, 43 VGPRs against 42
        __syncthreads();  // previous batch fully consumed (and s_done initialised); a refilled ring published
        if (s_done == 4) break;  // uniform: every wave has finished
        uint32_t id = 0;
        const int nb = tile_list_next<256>(a, list, s_ring, s_wc, &id);
        if (nb < 0) continue;
        if (nb == 0) break;
        fetched += (uint32_t)nb;
        if (tid < nb) {
            const GaussRec *r = a.rec + id;
            srec[0][tid] = r->q0;
            srec[1][tid] = r->q1;
            sP[tid] = make_float2(ldg(&r->q2.x, 0), __uint_as_float(id));  // the id: the index into the scene arrays
        }
        __syncthreads();
        if (wave_done) continue;
        for (int chunk = 0; chunk < nb; chunk += 64) {
            const int e = chunk + lane;
            const bool hit = e < nb && footprint_hits_rect(s0[e], s1[e], qx0, qx1, qy0, qy1);
            const unsigned long long m = __ballot(hit);
            evaluated += (uint32_t)__popcll(m);
            walk_survivors(m, chunk, read, eval, eval2);
            // the rules of the comment at the top (a negative early_T never fires: "blend every entry")
            const bool settled = !drawn | (NEAREST ? (filled >= k) | (T <= 0.0f) : T <= wk[K - 1]);
            if (__all(T <= a.early_T) || (lists_only && __all(settled))) {
                wave_done = true;
                wave_finished(lds, lane);
                break;
            }
        }
    }

    blend_stats_out<256, false>(a, t, tid, lane, wave, lds, evaluated, fetched, 0u);
    if (t.px < a.W && t.py < a.H) {
        const size_t pix = frame_pixel(a, t.ty, t.px, t.py);
        if (tk.final_T) tk.final_T[pix] = drawn ? T : 1.0f;
        if (pad & 1) topk_shift<K, 1>(wk, ik);  // uniform: slot pad comes to slot 0
        if (pad & 2) topk_shift<K, 2>(wk, ik);
        if (pad & 4) topk_shift<K, 4>(wk, ik);
#pragma unroll
        for (int j = 0; j < K; ++j) {  // what the undrawn pixels' lanes gathered is not theirs to show
            wk[j] = drawn ? wk[j] : 0.0f;
            ik[j] = drawn ? ik[j] : -1;
        }
        const size_t base = pix * (size_t)k;
        if (tk.vec) {  // uniform
#pragma unroll
            for (int j = 0; j < K; j += 4) {
                if (j < k) {
                    if (tk.ids) *reinterpret_cast<int4 *>(tk.ids + base + j) = make_int4(ik[j], ik[j + 1], ik[j + 2], ik[j + 3]);
                    if (tk.weights) *reinterpret_cast<float4 *>(tk.weights + base + j) = make_float4(wk[j], wk[j + 1], wk[j + 2], wk[j + 3]);
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < K; ++j) {
                if (j < k) {
                    if (tk.ids) tk.ids[base + j] = ik[j];
                    if (tk.weights) tk.weights[base + j] = wk[j];
                }
            }
        }
    }
}

template <int K>
static void launch_topk_k(bool nearest, int slots, const BlendArgs &a, const TopkArgs &tk, hipStream_t s)
{
    if (nearest) hipLaunchKernelGGL((blend_topk_kernel<K, true>), dim3((unsigned)slots), dim3(256), 0, s, a, tk);
    else hipLaunchKernelGGL((blend_topk_kernel<K, false>), dim3((unsigned)slots), dim3(256), 0, s, a, tk);
}

int launch_blend_topk(const GsrCamera &cam, const GsrOptions &opts, const Workspace &ws, const FramePlan &plan, int k, int select,
                      int32_t *out_ids, float *out_weights, float *out_final_T, hipStream_t s)
{
    BlendArgs a;
    int slots;
    const int rc = weight_walk_begin("top-k lists", cam, opts, ws, plan, nullptr, nullptr, s, &a, &slots);
    if (rc || !slots) return rc;
    const bool aligned = ((reinterpret_cast<uintptr_t>(out_ids) | reinterpret_cast<uintptr_t>(out_weights)) & 15u) == 0;
    const TopkArgs tk = {out_ids, out_weights, out_final_T, k, (k % 4 == 0 && aligned) ? 1 : 0};
    const bool nearest = select == GSR_TOPK_NEAREST;
    if (k <= 4) launch_topk_k<4>(nearest, slots, a, tk, s);
    else if (k <= 8) launch_topk_k<8>(nearest, slots, a, tk, s);
    else launch_topk_k<16>(nearest, slots, a, tk, s);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

}  // namespace gsr
