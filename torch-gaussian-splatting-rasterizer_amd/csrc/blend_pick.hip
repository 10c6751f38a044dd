// blend_pick.hip — stage 3 for what no blended channel can hold: per pixel, WHICH gaussian of its depth-ordered list
//   - dominates it:      best_id = argmax_i w_i(p), best_w = max_i w_i(p), with the weights w_i = alpha_i T_i of the colour frame;
//   - is its surface:    median_id = the first gaussian in draw order AFTER which T < median_T (0.5: the median depth of 2DGS and
//                        gsplat; 1.0: the first gaussian with w > 0);
//   - and how many contributed: count = #{i : w_i(p) > 0}   (COUNT instantiation only).
// A per-pixel gather: no atomics, nothing per gaussian is written.
//
// The workgroup, the batch loop, the survivor walk and the weight w = alpha T with its T are blend_weight_walk.h's: w and T are the
// feature blend's, bit for bit.
// In the place of the colour sums a survivor costs one compare and two selects for the maximum, one compare-and-select for the
// median and (COUNT) one compare-and-add.
//
// When has a pixel stopped changing?
//   - COUNT:  T <= early_T, FeatureBlend's rule where blend_kernel evaluates it.  With 0 that is T == 0.0f, after which every
//     w = alpha * 0 is 0: no maximum (strict >), no crossing (T stays 0, and a median not found by then never is: median_T > 0 means
//     T = 0 < median_T was seen by the entry that took T there), no count.  wave_entries / fetched_entries are the feature blend's.
//   - !COUNT: T <= early_T, or the median has been found and T <= best_w.  Exact at early_T = 0: alpha <= 0.99 < 1, so a later
//     entry's w' = fl(alpha' T') <= T' (rounding is monotone and T' is a float), and T never grows (T' = fl(T - alpha T) <= T), so
//     w' <= T' <= T <= best_w: the strict `w' > best_w` fails for this entry and, T only shrinking and best_w not moving, for every
//     later one — the earlier gaussian keeps an exact tie, as it would at the end of the list.  median_id is written once.  Neither
//     id nor best_w can change again; count is not an output of this instantiation.
//     Pixels whose values are never stored (outside the frame, the undrawn last column / row of reference_compat) are finished from
//     the start here.  (COUNT keeps walking them like the feature blend does — its counters are that kernel's — and stores the same
//     constants.)
// With early_T > 0 the result is the approximation the feature blend's is: entries past T <= early_T are not seen.
//
// LDS per workgroup, 256 staged entries:
//   s0 [256] float4   q0 = {mean_x, mean_y, -B/2C, -B/2A}      } the footprint test reads both per lane; a survivor's mean is a
//   s1 [256] float4   q1 = {A, B, C, pthr}                     } b64 broadcast, its conic a b128 broadcast
//   sP [256] float2   {log2 opacity (the record's q2.x), the entry's gaussian id as bits}: one b64 broadcast per survivor
//   ring [1024] + wc [8] + done: tile_list_next's
// = 8192 + 2048 + 4132 B = 14.4 KB: LDS allows 11 workgroups per CU, the 8 waves per SIMD of 64 VGPRs allow 8.
// The record's colour words are neither read nor written and tile_work is only read, as in blend_features.hip.
#include "blend_weight_walk.h"

namespace gsr {

struct PickArgs {
    int32_t *best_id;    // [H,W] in the frame's layout; any of the four may be null
    float *best_w;
    int32_t *median_id;
    int32_t *count;      // COUNT only
    float median_T;      // in (0, 1]
};

template <bool COUNT>
__global__ __launch_bounds__(256, 8) void blend_pick_kernel(BlendArgs args, const PickArgs pk)
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
    const float median_T = pk.median_T;

    float T = 1.0f, best_w = 0.0f;
    int best_id = -1, med_id = -1, count = 0;
    const bool drawn = t.px < a.xlim && t.py < a.ylim;  // Q1: the last column / row are never drawn (xlim <= W, ylim <= H)
    uint32_t evaluated = 0;  // wave-uniform
    bool wave_done = false;
    uint32_t fetched = 0;  // workgroup-uniform
    TileList<256> list = batches_begin<256, false>(a, t, tid, lds);
    struct Entry { float2 g; float4 c; float2 o; };
    auto stage = [&](uint32_t id, const GaussRec *r) __attribute__((always_inline)) {
        sP[tid] = make_float2(ldg(&r->q2.x, 0), __uint_as_float(id));  // the id: the index into the scene arrays
    };
    auto read = [&](int k) __attribute__((always_inline)) {
        const Entry en = {*reinterpret_cast<const float2 *>(&s0[k]), s1[k], sP[k]};
        keep_b128(en.c);
        return en;
    };
    // the pick accumulators in the place of blend_one's colour sums
    auto eval = [&](const Entry &en) __attribute__((always_inline)) {
        const int id = __float_as_int(en.o.y);
        const float w = blend_weight(en.g, en.c, en.o.x, fpx, fpy, T);
        const bool better = w > best_w;  // strict: on equal weights the earlier one in draw order stays (and w == 0 never wins)
        best_w = better ? w : best_w;
        best_id = better ? id : best_id;
        med_id = ((med_id < 0) & (T < median_T)) ? id : med_id;  // the first entry AFTER which T < median_T
        if (COUNT) count += w > 0.0f ? 1 : 0;
    };
    while (const int nb = next_batch_planes<256>(a, list, tid, lds, fetched, stage)) {
        if (wave_done) continue;
        for (int chunk = 0; chunk < nb; chunk += 64) {
            const int e = chunk + lane;
            const bool hit = e < nb && footprint_hits_rect(s0[e], s1[e], qx0, qx1, qy0, qy1);
            const unsigned long long m = __ballot(hit);
            evaluated += (uint32_t)__popcll(m);
            walk_survivors(m, chunk, read, eval);
            // the rules of the comment at the top (a negative early_T never fires: "blend every entry")
            const bool finished = COUNT ? T <= a.early_T : !drawn | (T <= a.early_T) | ((med_id >= 0) & (T <= best_w));
            if (__all(finished)) {
                wave_done = true;
                wave_finished(lds, lane);
                break;
            }
        }
    }

    blend_stats_out<256, false>(a, t, tid, lane, wave, lds, evaluated, fetched, 0u);
    if (t.px < a.W && t.py < a.H) {
        const size_t pix = frame_pixel(a, t.ty, t.px, t.py);
        if (pk.best_id) pk.best_id[pix] = drawn ? best_id : -1;
        if (pk.best_w) pk.best_w[pix] = drawn ? best_w : 0.0f;
        if (pk.median_id) pk.median_id[pix] = drawn ? med_id : -1;
        if (COUNT) pk.count[pix] = drawn ? count : 0;
    }
}

int launch_blend_pick(const GsrCamera &cam, const GsrOptions &opts, const Workspace &ws, const FramePlan &plan, float median_T,
                      int32_t *out_best_id, float *out_best_w, int32_t *out_median_id, int32_t *out_count, hipStream_t s)
{
    BlendArgs a;
    int slots;
    const int rc = weight_walk_begin("pick maps", cam, opts, ws, plan, nullptr, nullptr, s, &a, &slots);
    if (rc || !slots) return rc;
    const PickArgs pk = {out_best_id, out_best_w, out_median_id, out_count, median_T};
    if (out_count) hipLaunchKernelGGL(blend_pick_kernel<true>, dim3((unsigned)slots), dim3(256), 0, s, a, pk);
    else hipLaunchKernelGGL(blend_pick_kernel<false>, dim3((unsigned)slots), dim3(256), 0, s, a, pk);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

}  // namespace gsr
