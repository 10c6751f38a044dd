// blend_weight_walk.h — what the kernels share that walk the colour frame's tile lists for the WEIGHTS w_i = alpha_i T_i and differ
// only in what they do with a weight: blend_channels.hip (many channels per walk), blend_slab.hip (between two depth limits),
// blend_channels_backward.hip (the transpose), blend_pick.hip (ids), blend_topk.hip (contributor lists), blend_gstats.hip
// (per-gaussian statistics).  One statement each of
//   - blend_weight:       the arithmetic of a (pixel, survivor), blend_one's (blend_common.h) up to w and its T;
//   - next_batch_planes:  next_batch with the kernel's own third planes;
//   - walk_survivors / walk_survivors_single and keep_b128: a chunk's survivors in draw order;
//   - ChannelArgs, load_channel_row, store_channel_pixel, blend_channels_add, dpp_add: rows of channels;
//   - host: weight_walk_begin (the launch prelude; WalkViews: whether the launcher's kernel takes several views per launch),
//     for_channel_groups (a map's channels in walks of 16 / 8 / 4).
// The workgroup is blend_kernel's (blend_common.h): 256 threads per 16x16 tile, wave = 8x8 quadrant, lane = pixel, the same lists,
// footprint ballots, launch order and stat words.  blend_kernel itself, blend_one and next_batch stay as they are: the colour
// frame's asm walks are pinned to them bit for bit.  The callables are always_inline lambdas that capture the
// kernel's accumulators by reference; DESIGN.md 5.20 has the registers of every instantiation before and after.
#pragma once
#include "gsr_internal.h"
#include "blend_args.h"
#include "blend_common.h"

namespace gsr {

// The weight of one (pixel, survivor) and the pixel's T behind it: g = {mean_x, mean_y}, c = {A, B, C, -}, L = log2(opacity) —
// blend_one's 14 issues in blend_one's order, so w and T are the colour frame's and the feature blend's bit for bit.  `admit`: what
// else the caller asks of the entry (the slab kernel: its depth within the lane's limits); the default costs nothing.
// T: blend_one writes T - w and every kernel built from it compiles that into this fma.  Here a branch of the caller's (top-k's
// guarded insertion, the gradient's `no lane has a weight`) can stand between the product and the difference; the compiler then
// contracted some of them and not others, twice, and T was no longer the feature blend's: spelled out.
__device__ __forceinline__ float blend_weight(const float2 g, const float4 c, const float L, float fpx, float fpy, float &T,
                                              const bool admit = true)
{
    const float dx = g.x - fpx, dy = g.y - fpy;
    const float p = fmaf(dx, fmaf(c.y, dy, c.x * dx), fmaf(c.z * dy, dy, L));  // log2 domain, opacity folded in
    float alpha = fminf(__builtin_amdgcn_exp2f(p), GSR_MAX_ALPHA);
    const bool valid = (alpha > GSR_MIN_ALPHA) & (p <= L) & admit;
    alpha = valid ? alpha : 0.0f;
    const float w = alpha * T;
    T = fmaf(-T, alpha, T);
    return w;
}

// next_batch (blend_common.h) for kernels with planes of their own: q0 and q1 of the batch's tid-th gaussian go to lds.s0 / lds.s1,
// stage(id, rec) fills the rest (sL, sP, sF, sZ, sId).  Returns the batch's size, or 0 once the list has ended or every wave has
// called wave_finished; `fetched` (workgroup-uniform) counts the staged entries.  A kernel that flushes after a batch does so at the
// end of its loop body, behind a barrier of its own: the top barrier here then also says "flushed".
template <int THREADS, class Stage>
__device__ __forceinline__ int next_batch_planes(const BlendArgs &a, TileList<THREADS> &list, int tid, const BlendLds &lds, uint32_t &fetched,
                                                 Stage stage)
{
    for (;;) {
        __syncthreads();  // previous batch fully consumed (and *lds.done initialised); a refilled ring published
        if (*lds.done == THREADS / 64) return 0;  // uniform: every wave has finished
        uint32_t id = 0;
        const int nb = tile_list_next<THREADS>(a, list, lds.ring, lds.wc, &id);
        if (nb < 0) continue;
        if (nb == 0) return 0;
        fetched += (uint32_t)nb;
        if (tid < nb) {
            const GaussRec *r = a.rec + id;
            lds.s0[tid] = r->q0;
            lds.s1[tid] = r->q1;
            stage(id, r);
        }
        __syncthreads();
        return nb;
    }
}

// The end of every read(k): the conic's four words stay ONE ds_read_b128 (4 LDS cycles) though the walk uses three; a b96 costs 8.
// Last, behind the entry's other reads: the statement waits for the conic, and no LDS read moves across it.
__device__ __forceinline__ void keep_b128(const float4 &c)
{
    asm volatile("" ::"v"(c.w));
}

// The survivors `m` of a chunk of 64 staged entries, in draw order: read(k) does the broadcasts of entry k at its wave-uniform
// address — the mean a b64, the conic (keep_b128), the kernel's planes — and eval(entry) consumes them.  Two per trip, both read
// before either is evaluated, so that the second one's LDS reads overlap the first one's arithmetic; an odd one out comes last,
// after the loop — as a second arm inside it (blend_kernel's form) the accumulators of the two arms meet in register copies every
// trip.  eval2(a, b), where given, takes a trip's two entries at once (top-k: both weights first, then both insertions).
template <class Read, class Eval, class Eval2>
__device__ __forceinline__ void walk_survivors(unsigned long long m, int chunk, Read read, Eval eval, Eval2 eval2)
{
    while (m & (m - 1)) {
        const int k0 = chunk + (__ffsll((long long)m) - 1);
        m &= m - 1;
        const int k1 = chunk + (__ffsll((long long)m) - 1);
        m &= m - 1;
        const auto ea = read(k0);
        const auto eb = read(k1);
        eval2(ea, eb);
    }
    if (m) eval(read(chunk + (__ffsll((long long)m) - 1)));
}

template <class Read, class Eval>
__device__ __forceinline__ void walk_survivors(unsigned long long m, int chunk, Read read, Eval eval)
{
    walk_survivors(m, chunk, read, eval, [&](const auto &ea, const auto &eb) __attribute__((always_inline)) { eval(ea); eval(eb); });
}

// One per trip: for the kernels whose eval ends in LDS atomics (nothing of the next entry can overlap those).
template <class Read, class Eval>
__device__ __forceinline__ void walk_survivors_single(unsigned long long m, int chunk, Read read, Eval eval)
{
    while (m) {
        const int k = chunk + (__ffsll((long long)m) - 1);
        m &= m - 1;
        eval(read(k));
    }
}

// ---- rows of channels ----------------------------------------------------------------------------------------------------------
// Where a walk of up to CH = 4 Q channels finds its rows and its pixels.
struct ChannelArgs {
    const float *features;  // channel c0 of gaussian 0: row i at features + i * stride
    int64_t stride;         // floats between rows
    int channels;           // of the whole map: a pixel's values lie channels floats apart
    int c0, nch;            // this walk composites channels c0 .. c0 + nch - 1, 1 <= nch <= CH
    int vec_in, vec_out;    // 16-byte loads of the rows / stores of the pixels are aligned (decided on the host)
    int64_t T_view_stride;  // several views per launch (blend_channels_kernel): floats between the views' final-T planes
};

template <int Q> struct ChannelRow { float4 v[Q]; };

// Four consecutive floats of a row in one 16-byte global load (the address is 16-byte aligned).
__device__ __forceinline__ float4 ldg4(const float *p, int q)
{
    typedef float V4 __attribute__((ext_vector_type(4)));
    const V4 v = ((const __attribute__((address_space(1))) V4 *)p)[q];
    return make_float4(v.x, v.y, v.z, v.w);
}

// Channels 0 .. nch - 1 of a row (a gaussian's features, a pixel's upstream gradient); absent channels are 0 and not loaded.
template <int Q>
__device__ __forceinline__ ChannelRow<Q> load_channel_row(const float *row, int nch, int vec)
{
    ChannelRow<Q> r;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (vec && 4 * q + 4 <= nch) {
            v = ldg4(row, q);
        } else {
            if (4 * q + 0 < nch) v.x = ldg(row, 4 * q + 0);
            if (4 * q + 1 < nch) v.y = ldg(row, 4 * q + 1);
            if (4 * q + 2 < nch) v.z = ldg(row, 4 * q + 2);
            if (4 * q + 3 < nch) v.w = ldg(row, 4 * q + 3);
        }
        r.v[q] = v;
    }
    return r;
}

// A pixel's channels 0 .. nch - 1 to o; an undrawn pixel (Q1's last column / row) stores zeros.
template <int Q>
__device__ __forceinline__ void store_channel_pixel(float *o, const float (&acc)[4 * Q], int nch, int vec, bool drawn)
{
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const float4 v = make_float4(drawn ? acc[4 * q] : 0.0f, drawn ? acc[4 * q + 1] : 0.0f, drawn ? acc[4 * q + 2] : 0.0f,
                                     drawn ? acc[4 * q + 3] : 0.0f);
        if (vec && 4 * q + 4 <= nch) {
            reinterpret_cast<float4 *>(o)[q] = v;
        } else {
            if (4 * q + 0 < nch) o[4 * q + 0] = v.x;
            if (4 * q + 1 < nch) o[4 * q + 1] = v.y;
            if (4 * q + 2 < nch) o[4 * q + 2] = v.z;
            if (4 * q + 3 < nch) o[4 * q + 3] = v.w;
        }
    }
}

// blend_one's colour update for 4 Q channels: C_c = fma(w, f_c, C_c).
template <int Q>
__device__ __forceinline__ void blend_channels_add(float w, const float4 (&f)[Q], float (&acc)[4 * Q])
{
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        acc[4 * q + 0] = fmaf(w, f[q].x, acc[4 * q + 0]);
        acc[4 * q + 1] = fmaf(w, f[q].y, acc[4 * q + 1]);
        acc[4 * q + 2] = fmaf(w, f[q].z, acc[4 * q + 2]);
        acc[4 * q + 3] = fmaf(w, f[q].w, acc[4 * q + 3]);
    }
}

// x + (x moved across lanes by the DPP control CTRL); lanes without a source lane add 0 (bound_ctrl): one v_add_f32_dpp.
// (No contraction: fused with the product that made x, the add would need the moved value in a register of its own.)
template <int CTRL>
__device__ __forceinline__ float dpp_add(float x)
{
#pragma clang fp contract(off)
    return x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// The prelude of every launcher: the single-view refusal under the caller's noun (unless it takes several), the arguments, the launch order — heaviest tiles
// first, by what the last colour blend on this workspace staged where that is known (a schedule only).  tile_work stays null: these
// kernels never write it.  *slots == 0: an empty frame, nothing to launch.
// views: what the launcher's kernel takes.  Several — it is launched with dim3(*slots, ws.views), view blockIdx.y walks slice
// blockIdx.y of the workspace (blend_args_of_view) and writes out + blockIdx.y * out_view_stride BYTES; whatever else it keeps per
// view it finds through strides in its own argument struct.  Single (pick, top-k, slab): a workspace of several views is refused.
enum class WalkViews { Single, Several };
inline int weight_walk_begin(const char *noun, const GsrCamera &cam, const GsrOptions &opts, const Workspace &ws, const FramePlan &plan,
                             void *out, float *out_T, hipStream_t s, BlendArgs *a, int *slots, WalkViews views = WalkViews::Single,
                             size_t out_view_stride = 0)
{
    *slots = 0;
    if (ws.views > 1 && views == WalkViews::Single) { set_error("%s: single views only", noun); return GSR_ERR_BAD_ARG; }
    *a = blend_args_common(cam, opts, ws, plan, out, out_T);
    a->view_stride = ws.view_stride;  // (0 for a single view: every offset is zero)
    a->out_view_stride = out_view_stride;
    if (a->rows > 0 && a->tiles_x > 0) *slots = launch_tile_order(ws, plan, true, s);
    return GSR_OK;
}

// A map's channels in walks: launch(ch, width) once per group, width = the instantiated CH that takes it.  A walk of CH channels
// costs 14 + CH issues per survivor whatever nch is, so a wide map goes in walks of 16 and its rest to the narrowest width >=
// min_width that holds it: C = 24 is 16 + 8, C = 9 one walk of 16 (two of 8 would pay the geometry twice).
template <class Launch>
inline int for_channel_groups(const float *features, int64_t stride, const float *map, int channels, int min_width, Launch launch)
{
    for (int c0 = 0; c0 < channels;) {
        const int rest = channels - c0;
        const int width = rest > 8 ? 16 : rest > 4 || min_width > 4 ? 8 : 4;
        ChannelArgs ch;
        ch.features = features + c0;
        ch.stride = stride;
        ch.channels = channels;
        ch.c0 = c0;
        ch.nch = rest < width ? rest : width;
        // 16-byte accesses where every row / pixel of this group starts on a 16-byte boundary
        ch.vec_in = reinterpret_cast<uintptr_t>(ch.features) % 16 == 0 && stride % 4 == 0;
        ch.vec_out = reinterpret_cast<uintptr_t>(map + c0) % 16 == 0 && channels % 4 == 0;
        ch.T_view_stride = 0;
        const int rc = launch(ch, width);
        if (rc) return rc;
        c0 += ch.nch;
    }
    return GSR_OK;
}

}  // namespace gsr
