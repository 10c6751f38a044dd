// blend_channels_backward.hip — the transpose of blend_channels.hip in the per-gaussian channels:
// grad_features[i][c] += sum_p w_i(p) grad_map[p][c], with the forward's weights w_i = alpha_i T_i.
//
// out[p][c] = sum_i w_i(p) f_i[c] is linear in f, so its gradient needs the weights and nothing else: they are produced front to back,
// by the forward's walk of the forward's lists, with the forward's stop rule.  No per-pixel state is kept from the forward, nothing
// flows through alpha or T, and no map is written.  The workgroup, the survivor walk (one per trip) and the weight are
// blend_weight_walk.h's, the forward's: the weights are the forward's bit for bit.  (The batch head is spelled out: see the loop.)
//
// What differs:
//   per lane      CH registers with the pixel's upstream gradient, loaded once (zero outside the frame and in Q1's undrawn last
//                 column / row: the forward writes 0 there whatever f is);
//   per survivor  v_c = w * g_c summed over the wave's 64 lanes by six DPP adds per channel (row_shr 1 / 2 / 4 / 8, row_bcast 15 / 31:
//                 full-rate VALU, no LDS traffic), four channels' chains interleaved so that no DPP read waits for its operand;
//                 lane 63 then adds the sums into the LDS plane sG[entry][CH] with ds_add_f32 (the tile's four waves may meet in
//                 one entry) and marks the entry.  A survivor whose weight is 0 in all 64 pixels costs the 14 issues and a ballot;
//   per batch     after the barrier that ends the batch's consumption the workgroup adds the marked rows of sG to the caller's
//                 array with global_atomic_add_f32 and zeroes them: thread t of step k takes entry (k * 256 + t) / pad, channel
//                 % pad (pad = nch rounded up to a power of two), so a wave-instruction covers 64 / pad rows in segments of
//                 4 * pad bytes — four 64-byte segments at 16 channels — never one lane per row.  Unmarked rows and absent channels
//                 cost no atomic.
//
// LDS per workgroup, 256 staged entries:
//   s0, s1 [256] float4, sL [256] float   as in blend_channels.hip
//   sG  [256][CH] float   the batch's gradient rows (takes the place of the forward's sF, same size)
//   sId [256] uint32      the staged gaussian ids; bit 31 = some wave added into the entry's row in this batch
//   ring [1024] + wc [8] + done: tile_list_next's
// = 10240 + 1024 * CH + 4132 B: 22.0 KB at CH = 8 (7 workgroups per CU), 30.0 KB at CH = 16 (5).
// Float atomic sums depend on the order the adds arrive in: two runs of the same input may differ in the last bits.
// Several views per launch (gridDim.y, gsr_blend_channels_backward_views): view blockIdx.y walks its slice of the workspace and reads
// its own gradient map (ChannelGradArgs.map_view_stride); all views add into the one grad_features with the same atomics.
#include "blend_weight_walk.h"

namespace gsr {

struct ChannelGradArgs {
    const float *grad_map;  // channel c0 of pixel 0: a pixel's values lie `channels` floats apart
    float *grad_features;   // channel c0 of gaussian 0: row i at grad_features + i * stride
    int64_t stride;         // floats between rows
    int channels;           // of the whole map
    int nch;                // this walk handles channels c0 .. c0 + nch - 1, 1 <= nch <= CH
    int pad_shift;          // log2 of nch rounded up to a power of two: the flush's lanes per row
    int vec_map;            // 16-byte loads of the pixels are aligned (decided on the host)
    int64_t map_view_stride;  // several views per launch: floats between the views' gradient maps (all add into grad_features)
};

constexpr uint32_t ENTRY_TOUCHED = 1u << 31;  // ids are below 2^28 (LIST_ID_MASK)

// The sums of four values over the wave's 64 lanes, left in lane 63 (the other lanes hold partial sums nobody reads): row_shr
// 1 / 2 / 4 / 8 leave each row's sum in its lane 15, row_bcast:15 adds it into the next row — lane 31 = rows 0 + 1, lane 63 = rows
// 2 + 3 — and row_bcast:31 adds lane 31 into rows 2 and 3.  With the full row mask each step is one instruction.
__device__ __forceinline__ void wave_sum4(float (&v)[4])
{
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = dpp_add<0x111>(v[c]);
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = dpp_add<0x112>(v[c]);
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = dpp_add<0x114>(v[c]);
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = dpp_add<0x118>(v[c]);
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = dpp_add<0x142>(v[c]);
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = dpp_add<0x143>(v[c]);
}

// One survivor's weights w: the wave's sums of w * g_c into row k of sG.
template <int CH>
__device__ __forceinline__ void blend_channels_backward_add(float w, const float (&g)[CH], int nch, int lane, float *row, uint32_t *touched)
{
    if (__ballot(w != 0.0f) == 0) return;  // uniform: nothing to add for any pixel of the quadrant
#pragma unroll
    for (int q = 0; q < CH / 4; ++q) {
        if (4 * q < nch) {  // uniform
            float v[4] = {w * g[4 * q], w * g[4 * q + 1], w * g[4 * q + 2], w * g[4 * q + 3]};
            wave_sum4(v);
            if (lane == 63) {  // (row is a per-lane value to the compiler: see the call)
                atomicAdd(row + 4 * q, v[0]);
                if (4 * q + 1 < nch) atomicAdd(row + 4 * q + 1, v[1]);
                if (4 * q + 2 < nch) atomicAdd(row + 4 * q + 2, v[2]);
                if (4 * q + 3 < nch) atomicAdd(row + 4 * q + 3, v[3]);
            }
        }
    }
    if (lane == 63) atomicOr(touched, ENTRY_TOUCHED);
}

template <int CH> struct ChannelGradWaves { static constexpr int value = CH <= 8 ? 7 : 5; };  // blend_channels.hip's ChannelWaves

template <int CH>
__global__ __launch_bounds__(256, ChannelGradWaves<CH>::value) void blend_channels_backward_kernel(BlendArgs args, const ChannelGradArgs ch)
{
    static_assert(CH % 4 == 0, "channels are reduced four at a time");
    constexpr int Q = CH / 4;
    const BlendArgs a = blend_args_of_view(args);
    __shared__ float4 srec[2][256];
    __shared__ float sG[256 * CH];
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
    const int nch = ch.nch;

    // the pixel's upstream gradient; zero where the forward stores 0 (Q1's last column / row) or nothing (outside the frame)
    float g[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) g[c] = 0.0f;
    if (t.px < a.W && t.py < a.H && t.px < a.xlim && t.py < a.ylim) {
        const float *gp = ch.grad_map + (size_t)blockIdx.y * (size_t)ch.map_view_stride + frame_pixel(a, t.ty, t.px, t.py) * (size_t)ch.channels;
        const ChannelRow<Q> row = load_channel_row<Q>(gp, nch, ch.vec_map);
#pragma unroll
        for (int q = 0; q < Q; ++q) { g[4 * q] = row.v[q].x; g[4 * q + 1] = row.v[q].y; g[4 * q + 2] = row.v[q].z; g[4 * q + 3] = row.v[q].w; }
    }
#pragma unroll
    for (int j = 0; j < CH; ++j) sG[j * 256 + tid] = 0.0f;  // published by the loop's top barrier

    float T = 1.0f;
    uint32_t evaluated = 0;  // wave-uniform
    bool wave_done = false;
    uint32_t fetched = 0;  // workgroup-uniform
    TileList<256> list = batches_begin<256, false>(a, t, tid, lds);
    struct Entry { float2 g; float4 c; float L; int k; };
    auto read = [&](int k) __attribute__((always_inline)) {
        const Entry en = {*reinterpret_cast<const float2 *>(&s0[k]), s1[k], sL[k], k};
        keep_b128(en.c);
        return en;
    };
    auto eval = [&](const Entry &en) __attribute__((always_inline)) {
        // the row's index goes through a vector register the compiler cannot see through: for an address it knows to be
        // wave-uniform it wraps every LDS add into a loop that first sums the values of the active lanes
        int at = en.k * CH;
        asm volatile("" : "+v"(at));
        const float w = blend_weight(en.g, en.c, en.L, fpx, fpy, T);
        blend_channels_backward_add<CH>(w, g, nch, lane, &sG[at], &sId[en.k]);
    };
    for (;;) {
        // next_batch_planes (blend_weight_walk.h), spelled out: through the shared function the 16-channel kernel's median on the
        // bench frame came out 0.03 % above the parent's slowest run of five (the function's extra lane-mask bookkeeping per batch,
        // 23 scalar instructions); with its own head the kernel lies inside the parent's range at 8, 16 and 32 channels
        // 
        __syncthreads();  // previous batch consumed AND flushed (and s_done initialised); a refilled ring published
        if (s_done == 4) break;  // uniform: every wave saturated
        uint32_t id = 0;
        const int nb = tile_list_next<256>(a, list, s_ring, s_wc, &id);
        if (nb < 0) continue;
        if (nb == 0) break;
        fetched += (uint32_t)nb;
        if (tid < nb) {
            const GaussRec *r = a.rec + id;
            srec[0][tid] = r->q0;
            srec[1][tid] = r->q1;
            sL[tid] = ldg(&r->q2.x, 0);
            sId[tid] = id;  // ENTRY_TOUCHED clear
        }
        __syncthreads();
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
        __syncthreads();  // every wave is through with the batch: sG and the marks are final
        // flush: the marked rows into the caller's array, 64 / pad rows per wave-instruction, and back to zero
        const int total = nb << ch.pad_shift, cmask = (1 << ch.pad_shift) - 1;
        for (int i = tid; i < total; i += 256) {
            const int e = i >> ch.pad_shift, c = i & cmask;
            const uint32_t w = sId[e];
            if ((w & ENTRY_TOUCHED) && c < nch) {
                float *const cell = &sG[e * CH + c];
                float *dst = ch.grad_features + (size_t)(w & LIST_ID_MASK) * (size_t)ch.stride + c;
                unsafeAtomicAdd(dst, *cell);
                *cell = 0.0f;
            }
        }
    }

    blend_stats_out<256, false>(a, t, tid, lane, wave, lds, evaluated, fetched, 0u);
}

template <int CH>
static void launch_width(int slots, int views, const BlendArgs &a, const ChannelGradArgs &ch, hipStream_t s)
{
    hipLaunchKernelGGL(blend_channels_backward_kernel<CH>, dim3((unsigned)slots, (unsigned)views), dim3(256), 0, s, a, ch);
}

// for_channel_groups with the gradient map in the place of the forward's map (vec_map is the forward's vec_out)
int launch_blend_channels_backward(const GsrCamera &cam, const GsrOptions &opts, const Workspace &ws, const FramePlan &plan,
                                   const float *grad_map, int channels, float *grad_features, int64_t stride, hipStream_t s,
                                   int64_t map_view_stride)
{
    BlendArgs a;  // no map is written
    int slots;
    const int rc = weight_walk_begin("feature gradients", cam, opts, ws, plan, nullptr, nullptr, s, &a, &slots, WalkViews::Several);
    if (rc || !slots) return rc;
    return for_channel_groups(grad_features, stride, grad_map, channels, 8, [&](const ChannelArgs &g, int width) -> int {
        ChannelGradArgs ch;
        ch.grad_map = grad_map + g.c0;
        ch.grad_features = grad_features + g.c0;
        ch.stride = stride;
        ch.channels = channels;
        ch.nch = g.nch;
        ch.pad_shift = 0;
        while ((1 << ch.pad_shift) < ch.nch) ++ch.pad_shift;
        ch.vec_map = g.vec_out && (ws.views == 1 || map_view_stride % 4 == 0);  // a later view's pixels need not start on 16 bytes
        ch.map_view_stride = map_view_stride;
        if (width == 16) launch_width<16>(slots, ws.views, a, ch, s);
        else launch_width<8>(slots, ws.views, a, ch, s);
        GSR_HIP(hipGetLastError());
        return GSR_OK;
    });
}

}  // namespace gsr
