// blend_splat_backward.hip — the gradient of a feature map with respect to the 2-D splat: per gaussian, the derivative of
//   L = sum_p G[p] . map[p] + sum_p gT[p] T_final[p]
// in the opacity o, the 2-D mean and the inverse 2-D covariance (s0, s1, s2), over the forward's lists with the forward's weights.
//
// Per pair (pixel p, drawn gaussian i), with dx = mean_x - x, dy = mean_y - y, power = -1/2 (s0 dx^2 + s1 dy^2) - s2 dx dy,
// u = o exp(power), alpha = min(0.99, u) kept where alpha > 1/255 and power <= 0, w = alpha T, s_i = G[p] . f_i:
//   R_i        = sum_{j > i} w_j s_j + gT[p] T_final[p]          what lies behind i
//   dL/dalpha  = T_i s_i - R_i / (1 - alpha_i)
//   e_i        = dL/dalpha alpha_i = w_i s_i - R_i alpha_i / (1 - alpha_i);  0 where the pair is not kept, where the cap is
//                active (u >= 0.99: the cap's derivative is 0) and where T_i < min_T
// and the row of gaussian i collects, over p,
//   [0] e / o   [1] e (-s0 dx - s2 dy)   [2] e (-s1 dy - s2 dx)   [3] e (-dx^2 / 2)   [4] e (-dy^2 / 2)   [5] e (-dx dy)
//   [6] |term 1|   [7] |term 2|   (ABS only).
// The support (footprint, 1/255, power <= 0) is held fixed.
//
// R_i is formed front to back as S' - P_i: P_i = sum_{j <= i} w_j s_j, one register, and S' = P_last + gT T_final.  The lists,
// the ring reader and the stop rule are forward-only, so S' comes from a first pass of this kernel over the same list:
//   pass 1   the forward in dot space: blend_channels.hip's staging (q0, q1, L, the feature rows in sF), per survivor blend_weight,
//            a CH-wide dot and P = fma(w, s, P);
//   pass 2   batches_begin again behind a barrier; the same bits again (weight_and_alpha below is blend_weight's 14 issues in
//            blend_weight's order, and the dot and the fma are pass 1's), so P ends where pass 1's ended and the last drawn
//            entry's R is gT T_final; then e, the products, two DPP wave sums (blend_channels_backward.hip's), lane 63's
//            ds_add_f32 into sG[entry][8], and after the batch the flush of the marked rows with global_atomic_add_f32, eight
//            lanes per row in 32-byte segments.  A survivor with e = 0 in all 64 pixels costs the walk and a ballot.
// The record holds the conic in the log2 domain (A, B, C = -s0/2, -s2, -s1/2 times log2 e) and L = log2 o: the mean terms are
// summed as e (2 A dx + B dy), e (2 C dy + B dx) and scaled by ln 2 in the flush, column 0 is scaled by 1 / o = 2^-L there.
// S' - P_i carries an absolute error of about 2^-24 |S'| alpha / (1 - alpha) per pixel: a gaussian seen only through T <~ 1e-6
// gets a gradient that is tiny but relatively meaningless; min_T (and the forward's early_out_T) cut those pairs off.
//
// LDS per workgroup, 256 staged entries:
//   s0, s1 [256] float4, sL [256] float   as in blend_channels.hip
//   sF [CH/4][256] float4                  the feature rows, as in blend_channels.hip
//   sG [256][8] float                      the batch's gradient rows
//   sId [256] uint32                       the staged ids; bit 31 = some wave added into the entry's row in this batch
//   ring [1024] + wc [8] + done: tile_list_next's
// = 18432 + 1024 * CH + 4132 B: 26.0 KB at CH = 4, 30.0 KB at CH = 8, 38.0 KB at CH = 16 (4 workgroups per CU).
// No per-pixel state is taken from the caller and no map is written.  Single views.
#include "blend_weight_walk.h"

namespace gsr {

struct SplatGradArgs {
    const float *features;  // channel c0 of gaussian 0: row i at features + i * stride
    int64_t stride;         // floats between rows
    const float *grad_map;  // channel c0 of pixel 0: a pixel's values lie `channels` floats apart
    const float *grad_T;    // [pixels] or null: the upstream gradient of the final T (the first group's walk only)
    float *grad_splat;      // [n][8], added into
    int channels;           // of the whole map
    int nch;                // this walk handles channels c0 .. c0 + nch - 1, 1 <= nch <= CH
    int vec_in, vec_map;    // 16-byte loads of the rows / the pixels are aligned (decided on the host)
    float min_T;            // pairs with T_i < min_T contribute e = 0 (0: off)
};

constexpr uint32_t SPLAT_ENTRY_TOUCHED = 1u << 31;  // ids are below 2^28 (LIST_ID_MASK)
constexpr int SPLAT_ROW = 8;

// blend_channels_backward.hip's wave_sum4 for N values: their sums over the wave's 64 lanes, left in lane 63.
template <int N>
__device__ __forceinline__ void splat_wave_sum(float (&v)[N])
{
#pragma unroll
    for (int c = 0; c < N; ++c) v[c] = dpp_add<0x111>(v[c]);
#pragma unroll
    for (int c = 0; c < N; ++c) v[c] = dpp_add<0x112>(v[c]);
#pragma unroll
    for (int c = 0; c < N; ++c) v[c] = dpp_add<0x114>(v[c]);
#pragma unroll
    for (int c = 0; c < N; ++c) v[c] = dpp_add<0x118>(v[c]);
#pragma unroll
    for (int c = 0; c < N; ++c) v[c] = dpp_add<0x142>(v[c]);
#pragma unroll
    for (int c = 0; c < N; ++c) v[c] = dpp_add<0x143>(v[c]);
}

// blend_weight (blend_weight_walk.h), the same 14 issues in the same order — w and T are the feature blend's bit for bit — that
// also hands out what the gradient needs: dx, dy, alpha, and whether alpha moves with u (kept and below the cap).
struct SplatPair { float w, alpha, dx, dy; bool moves; };
__device__ __forceinline__ SplatPair weight_and_alpha(const float2 g, const float4 c, const float L, float fpx, float fpy, float &T)
{
    SplatPair r;
    r.dx = g.x - fpx; r.dy = g.y - fpy;
    const float p = fmaf(r.dx, fmaf(c.y, r.dy, c.x * r.dx), fmaf(c.z * r.dy, r.dy, L));  // log2 domain, opacity folded in
    const float u = __builtin_amdgcn_exp2f(p);
    float alpha = fminf(u, GSR_MAX_ALPHA);
    const bool valid = (alpha > GSR_MIN_ALPHA) & (p <= L);
    alpha = valid ? alpha : 0.0f;
    r.moves = valid & (u < GSR_MAX_ALPHA);
    r.alpha = alpha;
    r.w = alpha * T;
    T = fmaf(-T, alpha, T);
    return r;
}

// s = G[p] . f over the walk's channels: one product and CH - 1 fmas, the same in both passes.
template <int Q>
__device__ __forceinline__ float splat_dot(const float4 (&f)[Q], const float (&g)[4 * Q])
{
    float s = f[0].x * g[0];
    s = fmaf(f[0].y, g[1], s);
    s = fmaf(f[0].z, g[2], s);
    s = fmaf(f[0].w, g[3], s);
#pragma unroll
    for (int q = 1; q < Q; ++q) {
        s = fmaf(f[q].x, g[4 * q + 0], s);
        s = fmaf(f[q].y, g[4 * q + 1], s);
        s = fmaf(f[q].z, g[4 * q + 2], s);
        s = fmaf(f[q].w, g[4 * q + 3], s);
    }
    return s;
}

// waves per SIMD the register allocator aims at: what the LDS above lets a CU hold
template <int CH> struct SplatWaves { static constexpr int value = CH <= 4 ? 6 : CH <= 8 ? 5 : 4; };

template <int CH, bool ABS>
__global__ __launch_bounds__(256, SplatWaves<CH>::value) void blend_splat_backward_kernel(BlendArgs args, const SplatGradArgs ch)
{
    static_assert(CH % 4 == 0, "rows of the feature plane are 16-byte words");
    constexpr int Q = CH / 4;
    constexpr int NB = ABS ? 4 : 2;  // the second chain: columns 4, 5 and, ABS, 6, 7
    const BlendArgs a = blend_args_of_view(args);
    __shared__ float4 srec[2][256];
    __shared__ float4 sF[Q][256];
    __shared__ float sG[256 * SPLAT_ROW];
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

    // the pixel's upstream gradients; zero where the forward stores 0 / 1 (Q1's last column / row) or nothing (outside the frame)
    float g[CH], gT = 0.0f;
#pragma unroll
    for (int c = 0; c < CH; ++c) g[c] = 0.0f;
    if (t.px < a.W && t.py < a.H && t.px < a.xlim && t.py < a.ylim) {
        const size_t pix = frame_pixel(a, t.ty, t.px, t.py);
        const ChannelRow<Q> row = load_channel_row<Q>(ch.grad_map + pix * (size_t)ch.channels, nch, ch.vec_map);
#pragma unroll
        for (int q = 0; q < Q; ++q) { g[4 * q] = row.v[q].x; g[4 * q + 1] = row.v[q].y; g[4 * q + 2] = row.v[q].z; g[4 * q + 3] = row.v[q].w; }
        if (ch.grad_T) gT = ldg(ch.grad_T, pix);
    }
#pragma unroll
    for (int j = 0; j < SPLAT_ROW; ++j) sG[j * 256 + tid] = 0.0f;  // published by the loops' top barriers

    struct Entry { float2 g; float4 c; float L; float4 f[Q]; int k; };
    auto read = [&](int k) __attribute__((always_inline)) {
        Entry en;
        en.g = *reinterpret_cast<const float2 *>(&s0[k]);
        en.c = s1[k];
        en.L = sL[k];
#pragma unroll
        for (int q = 0; q < Q; ++q) en.f[q] = sF[q][k];
        en.k = k;
        keep_b128(en.c);
        return en;
    };
    auto stage = [&](uint32_t id, const GaussRec *r) __attribute__((always_inline)) {
        sL[tid] = ldg(&r->q2.x, 0);
        const ChannelRow<Q> row = load_channel_row<Q>(ch.features + (size_t)id * (size_t)ch.stride, nch, ch.vec_in);
#pragma unroll
        for (int q = 0; q < Q; ++q) sF[q][tid] = row.v[q];
        sId[tid] = id;  // SPLAT_ENTRY_TOUCHED clear
    };

    // ---- pass 1: S' = sum_i w_i s_i + gT T_final ----
    float Sp;
    {
        float T = 1.0f, P = 0.0f;
        bool wave_done = false;
        uint32_t fetched = 0;
        TileList<256> list = batches_begin<256, false>(a, t, tid, lds);
        auto eval = [&](const Entry &en) __attribute__((always_inline)) {
            const float w = blend_weight(en.g, en.c, en.L, fpx, fpy, T);
            P = fmaf(w, splat_dot<Q>(en.f, g), P);
        };
        while (const int nb = next_batch_planes<256>(a, list, tid, lds, fetched, stage)) {
            if (wave_done) continue;
            for (int chunk = 0; chunk < nb; chunk += 64) {
                const int e = chunk + lane;
                const bool hit = e < nb && footprint_hits_rect(s0[e], s1[e], qx0, qx1, qy0, qy1);
                const unsigned long long m = __ballot(hit);
                walk_survivors(m, chunk, read, eval);
                if (__all(T <= a.early_T)) {  // the forward's stop rule, where the forward evaluates it
                    wave_done = true;
                    wave_finished(lds, lane);
                    break;
                }
            }
        }
        Sp = fmaf(gT, T, P);
    }

    // ---- pass 2: the same walk again, now with S' ----
    __syncthreads();  // nobody still reads pass 1's s_done or its planes
    float T = 1.0f, P = 0.0f;
    uint32_t evaluated = 0;  // wave-uniform
    bool wave_done = false;
    uint32_t fetched = 0;  // workgroup-uniform
    TileList<256> list = batches_begin<256, false>(a, t, tid, lds);
    const float min_T = ch.min_T;
    auto eval = [&](const Entry &en) __attribute__((always_inline)) {
        // (the row's index through a vector register the compiler cannot see through: blend_channels_backward.hip says why)
        int at = en.k * SPLAT_ROW;
        asm volatile("" : "+v"(at));
        const float T_in = T;
        const SplatPair pr = weight_and_alpha(en.g, en.c, en.L, fpx, fpy, T);
        const float s = splat_dot<Q>(en.f, g);
        const float ws = pr.w * s;
        P = fmaf(pr.w, s, P);
        const float R = Sp - P;
        // 1 - alpha >= 0.01: the hardware reciprocal is fine
        const float ratio = pr.alpha * __builtin_amdgcn_rcpf(1.0f - pr.alpha);
        float e = fmaf(-R, ratio, ws);
        e = (pr.moves & (T_in >= min_T)) ? e : 0.0f;
        if (__ballot(e != 0.0f) == 0) return;  // uniform: nothing to add for any pixel of the quadrant
        const float mx = fmaf(2.0f * en.c.x, pr.dx, en.c.y * pr.dy), my = fmaf(2.0f * en.c.z, pr.dy, en.c.y * pr.dx);
        float va[4] = {e, e * mx, e * my, e * (-0.5f * pr.dx * pr.dx)};
        float vb[NB];
        vb[0] = e * (-0.5f * pr.dy * pr.dy);
        vb[1] = e * (-(pr.dx * pr.dy));
        if constexpr (ABS) { vb[2] = fabsf(va[1]); vb[3] = fabsf(va[2]); }
        splat_wave_sum<4>(va);
        splat_wave_sum<NB>(vb);
        if (lane == 63) {
            float *row = &sG[at];
#pragma unroll
            for (int c = 0; c < 4; ++c) atomicAdd(row + c, va[c]);
#pragma unroll
            for (int c = 0; c < NB; ++c) atomicAdd(row + 4 + c, vb[c]);
            atomicOr(&sId[en.k], SPLAT_ENTRY_TOUCHED);
        }
    };
    while (const int nb = next_batch_planes<256>(a, list, tid, lds, fetched, stage)) {
        if (!wave_done) {
            for (int chunk = 0; chunk < nb; chunk += 64) {
                const int e = chunk + lane;
                const bool hit = e < nb && footprint_hits_rect(s0[e], s1[e], qx0, qx1, qy0, qy1);
                const unsigned long long m = __ballot(hit);
                evaluated += (uint32_t)__popcll(m);
                walk_survivors_single(m, chunk, read, eval);
                if (__all(T <= a.early_T)) {
                    wave_done = true;
                    wave_finished(lds, lane);
                    break;
                }
            }
        }
        __syncthreads();  // every wave is through with the batch: sG and the marks are final
        // flush: the marked rows into the caller's array, eight lanes per row, and back to zero (next_batch_planes' top barrier
        // then also says "flushed")
        for (int i = tid; i < nb * SPLAT_ROW; i += 256) {
            const int e = i >> 3, c = i & 7;
            const uint32_t w = sId[e];
            if ((w & SPLAT_ENTRY_TOUCHED) && (ABS || c < 6)) {
                float *const cell = &sG[e * SPLAT_ROW + c];
                const float scale = c == 0 ? __builtin_amdgcn_exp2f(-sL[e]) : (c < 3 || c > 5) ? 0.6931471805599453f : 1.0f;
                unsafeAtomicAdd(ch.grad_splat + (size_t)(w & LIST_ID_MASK) * SPLAT_ROW + c, *cell * scale);
                *cell = 0.0f;
            }
        }
    }

    blend_stats_out<256, false>(a, t, tid, lane, wave, lds, evaluated, fetched, 0u);
}

template <int CH, bool ABS>
static void launch_width(int slots, const BlendArgs &a, const SplatGradArgs &ch, hipStream_t s)
{
    hipLaunchKernelGGL((blend_splat_backward_kernel<CH, ABS>), dim3((unsigned)slots), dim3(256), 0, s, a, ch);
}

// for_channel_groups over the map's channels: the six gradients are linear in s = G . f, so the groups add; gT enters with the
// first group only.  The two absolute sums are not linear in s: want_abs is one group (the caller checked channels <= 16).
int launch_blend_splat_backward(const GsrCamera &cam, const GsrOptions &opts, const Workspace &ws, const FramePlan &plan,
                                const float *features, int64_t stride, int channels, const float *grad_map, const float *grad_T,
                                float min_T, bool want_abs, float *grad_splat, hipStream_t s)
{
    BlendArgs a;  // no map is written
    int slots;
    const int rc = weight_walk_begin("splat gradients", cam, opts, ws, plan, nullptr, nullptr, s, &a, &slots);
    if (rc || !slots) return rc;
    return for_channel_groups(features, stride, grad_map, channels, 4, [&](const ChannelArgs &g, int width) -> int {
        SplatGradArgs ch;
        ch.features = g.features;
        ch.stride = stride;
        ch.grad_map = grad_map + g.c0;
        ch.grad_T = grad_T;
        ch.grad_splat = grad_splat;
        ch.channels = channels;
        ch.nch = g.nch;
        ch.vec_in = g.vec_in;
        ch.vec_map = g.vec_out;
        ch.min_T = min_T;
        if (want_abs) {
            if (width == 16) launch_width<16, true>(slots, a, ch, s);
            else if (width == 8) launch_width<8, true>(slots, a, ch, s);
            else launch_width<4, true>(slots, a, ch, s);
        } else {
            if (width == 16) launch_width<16, false>(slots, a, ch, s);
            else if (width == 8) launch_width<8, false>(slots, a, ch, s);
            else launch_width<4, false>(slots, a, ch, s);
        }
        GSR_HIP(hipGetLastError());
        grad_T = nullptr;  // T_final is every group's: its gradient enters once
        return GSR_OK;
    });
}

}  // namespace gsr
