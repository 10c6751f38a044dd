// blend_channels.hip — stage 3 for MANY caller-supplied channels in one walk of the tile lists: out[p][c] = sum_i w_i(p) f_i[c] with the
// weights w_i = alpha_i T_i of the colour frame, CH channels per walk instead of blend_features.hip's three.
//
// The geometry of a (pixel, survivor) evaluation — 14 of blend_one's 17 vector-ALU issues, the footprint ballots, the filtering of
// the cell lists, the staging of the records — does not depend on the channels; a walk that carries CH accumulators pays for it once
// per CH channels: ceil(C / CH) * (14 + CH) issues per survivor against ceil(C / 3) * 17.
//
// The workgroup is blend_kernel's (blend_common.h): 256 threads per 16x16 tile, wave = 8x8 quadrant, lane = pixel, the same lists
// (tile_list_of / tile_list_next), the same footprint test by wave ballot, the same launch order, and per channel blend_one's
// arithmetic in blend_one's order — w = alpha T, C_c = fma(w, f_c, C_c), T = fma(-T, alpha, T) — with FeatureBlend's stop rule
// evaluated where blend_kernel evaluates it: every channel of the map is the three-channel kernel's, bit for bit, at any early_out_T,
// and wave_entries / fetched_entries are that kernel's.
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
#include "gsr_internal.h"
#include "blend_args.h"
#include "blend_common.h"
#include "blend_channels.h"

namespace gsr {

// blend_one with CH channels: the same 14 issues up to w, then one fma per channel, then T.
template <int CH>
__device__ __forceinline__ void blend_channels_one(const float2 g, const float4 c, const float L, const float4 (&f)[CH / 4], float fpx,
                                                   float fpy, float &T, float (&acc)[CH])
{
    const float dx = g.x - fpx, dy = g.y - fpy;
    const float p = fmaf(dx, fmaf(c.y, dy, c.x * dx), fmaf(c.z * dy, dy, L));  // log2 domain, opacity folded in
    float alpha = fminf(__builtin_amdgcn_exp2f(p), GSR_MAX_ALPHA);
    const bool valid = (alpha > GSR_MIN_ALPHA) & (p <= L);
    alpha = valid ? alpha : 0.0f;
    const float w = alpha * T;
#pragma unroll
    for (int q = 0; q < CH / 4; ++q) {
        acc[4 * q + 0] = fmaf(w, f[q].x, acc[4 * q + 0]);
        acc[4 * q + 1] = fmaf(w, f[q].y, acc[4 * q + 1]);
        acc[4 * q + 2] = fmaf(w, f[q].z, acc[4 * q + 2]);
        acc[4 * q + 3] = fmaf(w, f[q].w, acc[4 * q + 3]);
    }
    T = T - w;
}

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
    for (;;) {
        // next_batch (blend_common.h) with this kernel's planes
        __syncthreads();  // previous batch fully consumed (and s_done initialised); a refilled ring published
        if (s_done == 4) break;  // uniform: every wave saturated
        uint32_t id = 0;
        const int nb = tile_list_next<256>(a, list, s_ring, s_wc, &id);
        if (nb < 0) continue;
        if (nb == 0) break;
        fetched += (uint32_t)nb;
        if (tid < nb) {
            const GaussRec *r = a.rec + id;
            const float *row = ch.features + (size_t)id * (size_t)ch.stride;
            srec[0][tid] = r->q0;
            srec[1][tid] = r->q1;
            sL[tid] = ldg(&r->q2.x, 0);
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
            const bool hit = e < nb && footprint_hits_rect(s0[e], s1[e], qx0, qx1, qy0, qy1);
            unsigned long long m = __ballot(hit);
            evaluated += (uint32_t)__popcll(m);
            // two survivors per trip so that the second one's LDS reads overlap the first one's arithmetic; an odd one out comes
            // last, after the loop — as a second arm inside it (blend_kernel's form) the CH accumulators of the two arms meet in
            // CH register copies per trip
            while (m & (m - 1)) {
                const int k0 = chunk + (__ffsll((long long)m) - 1);
                m &= m - 1;
                const int k1 = chunk + (__ffsll((long long)m) - 1);
                m &= m - 1;
                const float2 ga = *reinterpret_cast<const float2 *>(&s0[k0]);  // wave-uniform address: LDS broadcast
                const float4 ca = s1[k0];
                const float La = sL[k0];
                float4 fa[Q];
#pragma unroll
                for (int q = 0; q < Q; ++q) fa[q] = sF[q][k0];
                asm volatile("" ::"v"(ca.w));  // keep the read a ds_read_b128 (4 LDS cycles); a b96 costs 8
                const float2 gb = *reinterpret_cast<const float2 *>(&s0[k1]);
                const float4 cb = s1[k1];
                const float Lb = sL[k1];
                float4 fb[Q];
#pragma unroll
                for (int q = 0; q < Q; ++q) fb[q] = sF[q][k1];
                asm volatile("" ::"v"(cb.w));
                blend_channels_one<CH>(ga, ca, La, fa, fpx, fpy, T, acc);
                blend_channels_one<CH>(gb, cb, Lb, fb, fpx, fpy, T, acc);
            }
            if (m) {
                const int k0 = chunk + (__ffsll((long long)m) - 1);
                const float2 ga = *reinterpret_cast<const float2 *>(&s0[k0]);
                const float4 ca = s1[k0];
                const float La = sL[k0];
                float4 fa[Q];
#pragma unroll
                for (int q = 0; q < Q; ++q) fa[q] = sF[q][k0];
                asm volatile("" ::"v"(ca.w));
                blend_channels_one<CH>(ga, ca, La, fa, fpx, fpy, T, acc);
            }
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
static void launch_width(int slots, const BlendArgs &a, const ChannelArgs &ch, hipStream_t s)
{
    hipLaunchKernelGGL(blend_channels_kernel<CH>, dim3((unsigned)slots), dim3(256), 0, s, a, ch);
}

// The instantiated widths.  A walk of CH channels costs 14 + CH issues per survivor whatever nch is, so the rest of a map goes to the
// narrowest width that holds it: C = 24 is 16 + 8, C = 9 one walk of 16 (two of 8 would pay the geometry twice).
constexpr int CH_NARROW = 8, CH_WIDE = 16;

int launch_blend_channels(const GsrCamera &cam, const GsrOptions &opts, const Workspace &ws, const FramePlan &plan, const float *features,
                          int channels, int64_t stride, float *out_map, float *out_T, hipStream_t s)
{
    if (ws.views > 1) { set_error("feature maps: single views only"); return GSR_ERR_BAD_ARG; }
    BlendArgs a = blend_args_common(cam, opts, ws, plan, out_map, out_T);  // tile_work stays null: never written here
    if (a.rows <= 0 || a.tiles_x <= 0) return GSR_OK;
    // heaviest tiles first, by what the last colour blend on this workspace staged where that is known (a schedule only)
    const int slots = launch_tile_order(ws, plan, true, s);
    for (int c0 = 0; c0 < channels;) {
        const int rest = channels - c0;
        const int width = rest > CH_NARROW ? CH_WIDE : CH_NARROW;
        ChannelArgs ch;
        ch.features = features + c0;
        ch.stride = stride;
        ch.channels = channels;
        ch.c0 = c0;
        ch.nch = rest < width ? rest : width;
        // 16-byte accesses where every row / pixel of this group starts on a 16-byte boundary
        ch.vec_in = reinterpret_cast<uintptr_t>(ch.features) % 16 == 0 && stride % 4 == 0;
        ch.vec_out = reinterpret_cast<uintptr_t>(out_map + c0) % 16 == 0 && channels % 4 == 0;
        if (width == CH_WIDE) launch_width<CH_WIDE>(slots, a, ch, s);
        else launch_width<CH_NARROW>(slots, a, ch, s);
        GSR_HIP(hipGetLastError());
        a.out_T = nullptr;  // every group ends with the same T: the first one's store is enough
        c0 += ch.nch;
    }
    return GSR_OK;
}

}  // namespace gsr
