// blend_channels.hip — stage 3 for MANY caller-supplied channels in one walk of the tile lists: out[p][c] = sum_i w_i(p) f_i[c] with the
// weights w_i = alpha_i T_i of the colour frame, CH channels per walk instead of blend_features.hip's three.
//
// The geometry of a (pixel, survivor) evaluation — 14 of blend_one's 17 vector-ALU issues, the footprint ballots, the filtering of
// the cell lists, the staging of the records — does not depend on the channels; a walk that carries CH accumulators pays for it once
// per CH channels: ceil(C / CH) * (14 + CH) issues per survivor against ceil(C / 3) * 17.
//
// The workgroup, the batch loop, the survivor walk and the weight w = alpha T with its T = fma(-T, alpha, T) are blend_weight_walk.h's;
// per channel C_c = fma(w, f_c, C_c), blend_one's colour update, with FeatureBlend's stop rule evaluated where blend_kernel evaluates
// it: every channel of the map is the three-channel kernel's, bit for bit, at any early_out_T, and wave_entries / fetched_entries
// are that kernel's.
//
// LDS per workgroup, 256 staged entries:
//   s0 [256] float4   q0 = {mean_x, mean_y, -B/2C, -B/2A}      } the footprint test reads both per lane; a survivor's mean is a
//   s1 [256] float4   q1 = {A, B, C, pthr}                     } b64 broadcast, its conic a b128 broadcast
//   sL [256] float    log2 opacity (the record's q2.x)           one b32 broadcast per survivor
//   sF [CH/4][256] float4   channels 4q .. 4q+3 of entry e at sF[q][e]: staging writes consecutive 16-B words (no bank conflict),
//                     a survivor's channels are CH/4 ds_read_b128 broadcasts
//   ring [1024] + wc [8] + done: tile_list_next's
// = 9216 + 1024 * CH + 4132 B: 21.5 KB at CH = 8 (7 workgroups per CU), 29.7 KB at CH = 16 (5).
// The record's colour words are neither read nor written and tile_work is only read, as in blend_features.hip.
// Several views per launch (gridDim.y, gsr_blend_channels_views): view blockIdx.y walks its slice of the workspace and writes its own
// map (blend_args_of_view: out_view_stride) and its own final-T plane (ChannelArgs.T_view_stride); all views read one features array.
#include "blend_weight_walk.h"

namespace gsr {

// waves per SIMD the register allocator aims at: what the LDS above lets a CU hold
template <int CH> struct ChannelWaves { static constexpr int value = CH <= 4 ? 8 : CH <= 8 ? 7 : CH <= 16 ? 5 : 3; };

template <int CH>
__global__ __launch_bounds__(256, ChannelWaves<CH>::value) void blend_channels_kernel(BlendArgs args, const ChannelArgs ch)
{
    static_assert(CH % 4 == 0, "rows of the feature plane are 16-byte words");
    constexpr int Q = CH / 4;
    const BlendArgs a = blend_args_of_view(args);
    __shared__ float4 srec[2][256];
    __shared__ float4 sF[Q][256];
    __shared__ float sL[256];
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

    float T = 1.0f;
    float acc[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c] = 0.0f;
    uint32_t evaluated = 0;  // wave-uniform
    bool wave_done = false;
    uint32_t fetched = 0;  // workgroup-uniform
    const int nch = ch.nch;
    TileList<256> list = batches_begin<256, false>(a, t, tid, lds);
    struct Entry { float2 g; float4 c; float L; float4 f[Q]; };
    auto stage = [&](uint32_t id, const GaussRec *r) __attribute__((always_inline)) {
        sL[tid] = ldg(&r->q2.x, 0);
        const ChannelRow<Q> row = load_channel_row<Q>(ch.features + (size_t)id * (size_t)ch.stride, nch, ch.vec_in);
#pragma unroll
        for (int q = 0; q < Q; ++q) sF[q][tid] = row.v[q];
    };
    auto read = [&](int k) __attribute__((always_inline)) {
        Entry en;
        en.g = *reinterpret_cast<const float2 *>(&s0[k]);
        en.c = s1[k];
        en.L = sL[k];
#pragma unroll
        for (int q = 0; q < Q; ++q) en.f[q] = sF[q][k];
        keep_b128(en.c);
        return en;
    };
    auto eval = [&](const Entry &en) __attribute__((always_inline)) {
        blend_channels_add<Q>(blend_weight(en.g, en.c, en.L, fpx, fpy, T), en.f, acc);
    };
    while (const int nb = next_batch_planes<256>(a, list, tid, lds, fetched, stage)) {
        if (wave_done) continue;
        for (int chunk = 0; chunk < nb; chunk += 64) {
            const int e = chunk + lane;
            const bool hit = e < nb && footprint_hits_rect(s0[e], s1[e], qx0, qx1, qy0, qy1);
            const unsigned long long m = __ballot(hit);
            evaluated += (uint32_t)__popcll(m);
            walk_survivors(m, chunk, read, eval);
            if (__all(T <= a.early_T)) {  // FeatureBlend's rule (a negative threshold never fires: "blend every entry")
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
        // (view blockIdx.y's plane: the map's offset is blend_args_of_view's, through out_view_stride)
        if (a.out_T) a.out_T[(size_t)blockIdx.y * (size_t)ch.T_view_stride + pix] = drawn ? T : 1.0f;
    }
}

template <int CH>
static void launch_width(int slots, int views, const BlendArgs &a, const ChannelArgs &ch, hipStream_t s)
{
    hipLaunchKernelGGL(blend_channels_kernel<CH>, dim3((unsigned)slots, (unsigned)views), dim3(256), 0, s, a, ch);
}

int launch_blend_channels(const GsrCamera &cam, const GsrOptions &opts, const Workspace &ws, const FramePlan &plan, const float *features,
                          int channels, int64_t stride, float *out_map, float *out_T, hipStream_t s, int64_t map_view_stride,
                          int64_t T_view_stride)
{
    BlendArgs a;
    int slots;
    const int rc = weight_walk_begin("feature maps", cam, opts, ws, plan, out_map, out_T, s, &a, &slots, WalkViews::Several,
                                     (size_t)map_view_stride * sizeof(float));
    if (rc || !slots) return rc;
    return for_channel_groups(features, stride, out_map, channels, 8, [&](const ChannelArgs &group, int width) -> int {
        ChannelArgs ch = group;
        ch.T_view_stride = T_view_stride;
        if (ws.views > 1 && map_view_stride % 4 != 0) ch.vec_out = 0;  // a later view's pixels need not start on 16 bytes
        if (width == 16) launch_width<16>(slots, ws.views, a, ch, s);
        else launch_width<8>(slots, ws.views, a, ch, s);
        GSR_HIP(hipGetLastError());
        a.out_T = nullptr;  // every group ends with the same T: the first one's store is enough
        return GSR_OK;
    });
}

}  // namespace gsr
