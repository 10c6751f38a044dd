// blend_common.h — what every blend kernel shares (blend.hip: the colour frame; blend_features.hip: caller-supplied channels):
// the per-(pixel, entry) arithmetic, the staging of a tile's depth-ordered list, and the skeleton of a tile's workgroup — prologue
// (tile_of_slot, empty_slot, tile_coords), batch loop (batches_begin, next_batch), stat words (blend_stats_out); the pixel store is blend_args.h's store_pixel.
// blend_kernel, at the end, is the plain-C blend built from them, one instantiation per policy: the colour frame's
// (blend.hip, ColourBlend) and the feature maps' (blend_features.hip, FeatureBlend).  blend.hip's blend_walk_kernel, the product,
// takes prologue, stat words and pixel store from here and spells the batch loop out around its hand-scheduled walk (its comment
// says why).
#pragma once
#include "gsr_internal.h"
#include "blend_args.h"
#include "footprint.h"

namespace gsr {

// A load through a pointer that came out of memory: say that it points to global memory, or the access is a flat_load.
template <typename T>
__device__ __forceinline__ T ldg(const T *p, size_t i)
{
    return ((const __attribute__((address_space(1))) T *)p)[i];
}

// one (pixel, entry) evaluation; g = {mean_x, mean_y}, c = {A, B, C, -}, o = {log2(opacity), r, g, b}.
// 17 VALU issues (tools/valu_microbench.hip prices them):
//   - log2(opacity) rides in the quadratic's constant term: alpha = 2^p with p = power + L, and the reference's
//     `power <= 0` becomes p <= L;
//   - T*(1-alpha) is evaluated as T - alpha*T, reusing the product the colour update needs.
__device__ __forceinline__ void blend_one(const float2 g, const float4 c, const float4 o, float fpx, float fpy, float &T,
                                          float &Cr, float &Cg, float &Cb)
{
    const float dx = g.x - fpx, dy = g.y - fpy;
    const float p = fmaf(dx, fmaf(c.y, dy, c.x * dx), fmaf(c.z * dy, dy, o.x));  // log2 domain, opacity folded in
    float alpha = fminf(__builtin_amdgcn_exp2f(p), GSR_MAX_ALPHA);
    const bool valid = (alpha > GSR_MIN_ALPHA) & (p <= o.x);
    alpha = valid ? alpha : 0.0f;
    const float w = alpha * T;
    Cr = fmaf(w, o.y, Cr);
    Cg = fmaf(w, o.z, Cg);
    Cb = fmaf(w, o.w, Cb);
    T = T - w;
}

// ---- staging -----------------------------------------------------------------------------------------------------------------
// A tile's depth-ordered list is either a range of per-tile entries (fine binning) or, with coarse binning, the list of its 32x32
// cell filtered by the tile's bit of the mask each entry carries in its top four bits (binning.hip): the workgroup reads the
// cell list 2 * THREADS entries at a time, keeps — in order, by ballot + wave counts — the ids with its bit in a small ring in
// LDS, and stages THREADS of them per batch.  (Round 2 expanded the cell lists into tile lists in a kernel of its own: 34 us, a
// write and a read of 61 MB per frame, 16 B of workspace per pair slot.)
constexpr uint32_t LIST_ID_MASK = (1u << 28) - 1u;

template <int THREADS>
struct TileList {
    static constexpr int WAVES = THREADS / 64, RING = 4 * THREADS;  // ring: < THREADS left over + 2 * THREADS read
    uint32_t pos, end;    // cursor into the list / its end               } workgroup-uniform
    uint32_t head, qlen;  // ring: first unread slot, entries in it       }
    int bit;              // cell lists: 28 + the tile's index in its cell; -1: plain per-tile list
};

template <int THREADS>
__device__ __forceinline__ TileList<THREADS> tile_list_of(const BlendArgs &a, int tile, int tx, int ty)
{
    TileList<THREADS> t;
    uint2 r;
    if (a.cell_lists) {
        r = a.cranges[(ty >> 1) * a.ctiles_x + (tx >> 1)];
        t.bit = 28 + (ty & 1) * 2 + (tx & 1);
    } else {
        r = a.ranges[tile];
        t.bit = -1;
    }
    t.pos = r.x; t.end = r.y; t.head = 0; t.qlen = 0;
    return t;
}

// One step of the staging loop, called by every thread after the loop's top barrier.  Returns -1: the ring was refilled, go round
// again (the top barrier publishes it); 0: the list is exhausted; nb > 0: thread tid < nb takes the batch's tid-th gaussian, *id.
template <int THREADS>
__device__ __forceinline__ int tile_list_next(const BlendArgs &a, TileList<THREADS> &t, uint32_t *s_ring, uint32_t *s_wc, uint32_t *id)
{
    constexpr int WAVES = THREADS / 64, RING = TileList<THREADS>::RING;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (t.bit < 0) {
        if (t.pos >= t.end) return 0;
        const int nb = (int)min((uint32_t)THREADS, t.end - t.pos);
        if (tid < nb) *id = a.pval[t.pos + tid];
        t.pos += nb;
        return nb;
    }
    if (t.qlen < (uint32_t)THREADS && t.pos < t.end) {  // refill: the next 2 * THREADS entries of the cell list, filtered in order
        const uint32_t i0 = t.pos + tid, i1 = i0 + THREADS;
        const uint32_t v0 = i0 < t.end ? a.pval[i0] : 0u, v1 = i1 < t.end ? a.pval[i1] : 0u;  // mask 0: nobody's
        const bool f0 = (v0 >> t.bit) & 1u, f1 = (v1 >> t.bit) & 1u;
        const unsigned long long b0 = __ballot(f0), b1 = __ballot(f1);
        if (lane == 0) { s_wc[wave] = (uint32_t)__popcll(b0); s_wc[WAVES + wave] = (uint32_t)__popcll(b1); }
        __syncthreads();
        uint32_t o0 = 0, tot0 = 0, o1 = 0, tot1 = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const uint32_t c0 = s_wc[w], c1 = s_wc[WAVES + w];
            if (w < wave) { o0 += c0; o1 += c1; }
            tot0 += c0; tot1 += c1;
        }
        // set bits below this lane (v_mbcnt: no lane mask to keep in registers across the walks)
        auto below = [](unsigned long long b) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u)); };
        const uint32_t tail = t.head + t.qlen;
        if (f0) s_ring[(tail + o0 + below(b0)) & (RING - 1)] = v0 & LIST_ID_MASK;
        if (f1) s_ring[(tail + tot0 + o1 + below(b1)) & (RING - 1)] = v1 & LIST_ID_MASK;
        t.qlen += tot0 + tot1;
        t.pos += 2 * THREADS;
        return -1;
    }
    if (t.qlen == 0) return 0;
    const int nb = (int)min((uint32_t)THREADS, t.qlen);
    if (tid < nb) *id = s_ring[(t.head + tid) & (RING - 1)];
    t.head += nb;
    t.qlen -= nb;
    return nb;
}

// ---- the skeleton of a tile's workgroup ------------------------------------------------------------------------------------------
// Every blend kernel: THREADS = 256 / QPW threads per 16x16 tile, a wave QPW of its 8x8 quadrants, a lane one pixel of each.
// The kernels pass their own tid / lane / wave in: re-deriving them here from threadIdx.x (unsigned) compiles to other code.
// The workgroup's LDS: each kernel declares the arrays as __shared__ variables of its own and hands their addresses over.
struct BlendLds {
    float4 *s0, *s1, *s2;   // staged records, one plane of THREADS entries per 16-B part: q0, q1, q2 (or what stands in for it)
    uint32_t *ring, *wc;    // TileList<THREADS>::RING and 2 * WAVES words (tile_list_next)
    int *done;              // waves that have finished (next_batch / wave_finished; nullptr in blend_walk_kernel, whose live word stands in for it)
    uint32_t *col;          // the workgroup's deferred-colour evaluations (COLOUR kernels only)
};

// What the colour kernels add to a staged batch (lazy colours, blend.hip staged_q2): one class word per entry — bit q = the entry can
// touch quadrant q of the tile (q = 2 * lower half + right half), bit 4 + q = it may take the walk's unguarded path there
// (footprint_classify) — and the workgroup's word of quadrants that are still live.  The staging thread classifies its entry once,
// for all four quadrants; the waves take their masks from the class words, and a pending colour is evaluated only for an entry
// with a hit in a live quadrant.
struct BlendClassLds {
    uint32_t *cls;   // THREADS class words
    uint32_t *live;  // bit q: quadrant q has not finished (read after the batch's top barrier: workgroup-uniform)
};

// The pixel-centre bounds of the four quadrants of the tile whose first pixel is (x0, y0): quadrant q spans x[2 * (q & 1)] ..
// x[2 * (q & 1) + 1], y[2 * (q >> 1)] .. y[2 * (q >> 1) + 1].  Called where a batch is staged, with x0 and y0 made opaque there: left
// to itself the compiler computes the eight floats once, ahead of the batch loop, as eight vector registers that it then spills around
// the walks; this way they cost eight conversions per batch and no register.
struct QuadBounds {
    float x[4], y[4];
};
__device__ __forceinline__ QuadBounds quad_bounds(int x0, int y0)
{
    asm volatile("" : "+s"(x0), "+s"(y0));  // (workgroup-uniform: scalar registers)
    QuadBounds b;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        b.x[k] = (float)(x0 + 8 * (k >> 1) + 7 * (k & 1));
        b.y[k] = (float)(y0 + 8 * (k >> 1) + 7 * (k & 1));
    }
    return b;
}

// An entry's class word on the tile with the quadrants `b`.  FAST = false: hit bits only (footprint_hits_rect: the same value as
// footprint_classify's hit), for the plain kernel, which has no unguarded path.
template <bool FAST>
__device__ __forceinline__ uint32_t footprint_class4(const float4 q0, const float4 q1, float L, const QuadBounds &b)
{
    uint32_t c = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float fx0 = b.x[2 * (q & 1)], fx1 = b.x[2 * (q & 1) + 1], fy0 = b.y[2 * (q >> 1)], fy1 = b.y[2 * (q >> 1) + 1];
        if (FAST) {
            const FootprintClass f = footprint_classify(q0, q1, L, fx0, fx1, fy0, fy1);
            c |= (f.hit ? 1u : 0u) << q | (f.fast ? 16u : 0u) << q;
        } else {
            c |= (footprint_hits_rect(q0, q1, fx0, fx1, fy0, fy1) ? 1u : 0u) << q;
        }
    }
    return c;
}

struct TilePixel {
    int tile, tx, ty;
    int qx, qy;      // first pixel of the wave's quadrant (QPW = 2: of the left one)
    int px, py;      // the lane's pixel (QPW = 2: and (px + 8, py))
    uint32_t *stat;  // the launch slot's BLEND_STAT_WORDS counters
};

// Prologue: t = tile_of_slot(a); if (t.tile < 0) return empty_slot(t, tid); tile_coords<QPW>(a, lane, wave, t).  The branch stays
// in the kernel: as a helper's return value it compiles to a flag that is tested again, and the product kernels spill.
__device__ __forceinline__ TilePixel tile_of_slot(const BlendArgs &a)
{
    TilePixel t;
    t.tile = a.order[blockIdx.x];
    t.stat = a.stats + (size_t)blockIdx.x * BLEND_STAT_WORDS;
    return t;
}

__device__ __forceinline__ void empty_slot(const TilePixel &t, int tid)
{
    if (tid < BLEND_STAT_WORDS) t.stat[tid] = 0;
}

template <int QPW>
__device__ __forceinline__ void tile_coords(const BlendArgs &a, int lane, int wave, TilePixel &t)
{
    t.ty = t.tile / a.tiles_x; t.tx = t.tile - t.ty * a.tiles_x;
    t.qx = t.tx * 16 + (QPW == 1 ? (wave & 1) * 8 : 0); t.qy = t.ty * 16 + (QPW == 1 ? wave >> 1 : wave) * 8;
    t.px = t.qx + (lane & 7); t.py = t.qy + (lane >> 3);
}

// The batch loop: list = batches_begin(...); while (const int nb = next_batch(..., fetched, stage)) { consume nb staged entries }.
// next_batch stages the tile's list THREADS entries at a time — q0 and q1 of entry `id` from its record, the third plane from
// stage(id, need) — counts them in `fetched` (workgroup-uniform) and returns the batch's size, or 0 once the list has ended or every
// wave has called wave_finished.  COLOUR: the staging thread also leaves the entry's class word (hit bits) in cl.cls, and `need` says
// whether one of the quadrants it hits is still live (*cl.live as the batch's top barrier published it); the other policies stage
// with need = true and have no class plane.  The consuming side stays in the kernel's body: as a callable that captures the accumulators, the
// compiler sinks blend_one's `T - w` below the survivor loop's two arms, away from the multiply it contracts with into
// fma(-T, alpha, T), and the plain kernel's frames are no longer the asm walks' bit for bit.
template <int THREADS, bool COLOUR>
__device__ __forceinline__ TileList<THREADS> batches_begin(const BlendArgs &a, const TilePixel &t, int tid, const BlendLds &lds,
                                                           const BlendClassLds &cl = {})
{
    if (tid == 0) { *lds.done = 0; if (COLOUR) { *lds.col = 0; *cl.live = 0xFu; } }
    return tile_list_of<THREADS>(a, t.tile, t.tx, t.ty);
}

template <int THREADS, bool COLOUR, class Stage>
__device__ __forceinline__ int next_batch(const BlendArgs &a, TileList<THREADS> &list, const TilePixel &t, int tid, const BlendLds &lds,
                                          const BlendClassLds &cl, uint32_t &fetched, Stage stage)
{
    for (;;) {
        __syncthreads();  // previous batch fully consumed (and *lds.done initialised); a refilled ring published
        if (*lds.done == THREADS / 64) return 0;  // uniform: every wave saturated
        uint32_t live = 0;
        if constexpr (COLOUR) live = *cl.live;
        uint32_t id = 0;
        const int nb = tile_list_next<THREADS>(a, list, lds.ring, lds.wc, &id);
        if (nb < 0) continue;
        if (nb == 0) return 0;
        fetched += (uint32_t)nb;
        if (tid < nb) {
            const GaussRec *r = a.rec + id;
            if constexpr (COLOUR) {
                const float4 q0 = r->q0, q1 = r->q1;
                const uint32_t c = footprint_class4<false>(q0, q1, 0.0f, quad_bounds(t.tx * 16, t.ty * 16));
                lds.s0[tid] = q0;
                lds.s1[tid] = q1;
                cl.cls[tid] = c;
                lds.s2[tid] = stage(id, (c & live) != 0u);
            } else {
                lds.s0[tid] = r->q0;
                lds.s1[tid] = r->q1;
                lds.s2[tid] = stage(id, true);
            }
        }
        __syncthreads();
        return nb;
    }
}

// A wave that has finished says so, once.
__device__ __forceinline__ void wave_finished(const BlendLds &lds, int lane)
{
    if (lane == 0) atomicAdd(lds.done, 1);
}

// Quadrants that have finished leave the live word, once; they never come back.
__device__ __forceinline__ void quadrants_finished(const BlendClassLds &cl, int lane, uint32_t bits)
{
    if (lane == 0) {
        asm volatile("" : "+v"(bits));  // (the operand is formed here, not kept in a register across the walks)
        atomicAnd(cl.live, ~bits);
    }
}

// Epilogue, every thread: the counters gsr_read_stats totals.  COLOUR, the colour frame's kernels: stat[5] = the workgroup's
// deferred-colour evaluations (wave totals into LDS, one store), and tile_work = next frame's launch-order hint.  The feature
// blend evaluates no colour and leaves tile_work what the last colour blend left.
// ADD (slice B of a front-slice frame, blend.hip): the counters and the hint are added to what slice A's blend left — in the slot,
// which was another tile's there: only the totals over all slots are ever read.
template <int THREADS, bool COLOUR, bool ADD = false>
__device__ __forceinline__ void blend_stats_out(const BlendArgs &a, const TilePixel &t, int tid, int lane, int wave, const BlendLds &lds,
                                                uint32_t evaluated, uint32_t fetched, uint32_t col_evals)
{
    if (lane == 0) {
        t.stat[wave] = (ADD ? t.stat[wave] : 0u) + evaluated;
        if (THREADS == 128 && !ADD) t.stat[2 + wave] = 0;
    }
    if (COLOUR) {
        if (tid == 0) { t.stat[4] = (ADD ? t.stat[4] : 0u) + fetched; a.tile_work[t.tile] = (ADD ? a.tile_work[t.tile] : 1u) + fetched; }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) col_evals += (uint32_t)__shfl_xor((int)col_evals, d, 64);
        if (lane == 0 && col_evals) atomicAdd(lds.col, col_evals);
        __syncthreads();
        if (tid == 0) t.stat[5] = (ADD ? t.stat[5] : 0u) + *lds.col;
    } else if (tid == 0) {
        t.stat[4] = fetched; t.stat[5] = 0;
    }
}

// The plain-C statement of the blend: one 256-thread workgroup per tile, wave = 8x8 quadrant, lane = pixel.  The policy P says
//   - stage(a, id, evals): the third LDS plane of gaussian `id`, {log2 opacity, c0, c1, c2}; COLOUR: stage(a, id, need, evals),
//     need = false: no walk will read c0..c2 of this entry;
//   - acc_round(T, C0, C1, C2): what happens to the accumulators after every entry;
//   - finished(a, T, C0, C1, C2, undrawn): has this pixel stopped changing?
//   - COLOUR (blend_stats_out), MIN_WAVES (per SIMD, for the register allocator).
template <class P>
__global__ __launch_bounds__(256, P::MIN_WAVES) void blend_kernel(BlendArgs args, const P policy)
{
    const BlendArgs a = blend_args_of_view(args);
    __shared__ float4 srec[3][256];
    __shared__ int s_done;
    __shared__ uint32_t s_col;
    __shared__ uint32_t s_ring[TileList<256>::RING], s_wc[2 * TileList<256>::WAVES];
    __shared__ uint32_t s_cls[P::COLOUR ? 256 : 1], s_live;
    const BlendLds lds = {srec[0], srec[1], srec[2], s_ring, s_wc, &s_done, &s_col};
    const BlendClassLds cl = {s_cls, &s_live};  // COLOUR only.  s_done stays the loop's stop word for every policy (next_batch is shared); s_live == 0 says the same
    const float4 *const s0 = srec[0], *const s1 = srec[1], *const s2 = srec[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    TilePixel t = tile_of_slot(a);
    if (t.tile < 0) return empty_slot(t, tid);  // uniform
    tile_coords<1>(a, lane, wave, t);
    const float fpx = (float)t.px, fpy = (float)t.py;
    const float qx0 = (float)t.qx, qx1 = (float)(t.qx + 7), qy0 = (float)t.qy, qy1 = (float)(t.qy + 7);

    float T = 1.0f, C0 = 0.0f, C1 = 0.0f, C2 = 0.0f;
    const bool undrawn = a.sat_scale != 0.0f && !(t.px < a.xlim && t.py < a.ylim);  // never stored: finished from the start
    uint32_t evaluated = 0;  // wave-uniform
    uint32_t col_evals = 0;  // per thread: deferred colours this thread evaluated while staging

    auto stage = [&](uint32_t id, bool need) __attribute__((always_inline)) {
        if constexpr (P::COLOUR) return policy.stage(a, id, need, col_evals);
        else return policy.stage(a, id, col_evals);
    };
    bool wave_done = false;
    uint32_t fetched = 0;  // workgroup-uniform
    TileList<256> list = batches_begin<256, P::COLOUR>(a, t, tid, lds, cl);
    while (const int nb = next_batch<256, P::COLOUR>(a, list, t, tid, lds, cl, fetched, stage)) {
        if (wave_done) continue;
        for (int chunk = 0; chunk < nb; chunk += 64) {
            const int e = chunk + lane;
            bool hit;  // COLOUR: the bit the staging thread computed (quadrant = wave) — what decided whether the colour was evaluated
            if constexpr (P::COLOUR) hit = e < nb && (s_cls[e] >> wave & 1u);
            else hit = e < nb && footprint_hits_rect(s0[e], s1[e], qx0, qx1, qy0, qy1);
            unsigned long long m = __ballot(hit);
            evaluated += (uint32_t)__popcll(m);
            // two survivors per trip so that the second one's LDS reads overlap the first one's arithmetic
            while (m) {
                const int k0 = chunk + (__ffsll((long long)m) - 1);
                m &= m - 1;
                const float2 ga = *reinterpret_cast<const float2 *>(&s0[k0]);  // wave-uniform address: LDS broadcast
                const float4 ca = s1[k0];
                const float4 oa = s2[k0];
                asm volatile("" ::"v"(ca.w));  // keep the read a ds_read_b128 (4 LDS cycles); a b96 costs 8
                if (m) {
                    const int k1 = chunk + (__ffsll((long long)m) - 1);
                    m &= m - 1;
                    const float2 gb = *reinterpret_cast<const float2 *>(&s0[k1]);
                    const float4 cb = s1[k1];
                    const float4 ob = s2[k1];
                    asm volatile("" ::"v"(cb.w));
                    blend_one(ga, ca, oa, fpx, fpy, T, C0, C1, C2);
                    policy.acc_round(T, C0, C1, C2);
                    blend_one(gb, cb, ob, fpx, fpy, T, C0, C1, C2);
                    policy.acc_round(T, C0, C1, C2);
                } else {
                    blend_one(ga, ca, oa, fpx, fpy, T, C0, C1, C2);
                    policy.acc_round(T, C0, C1, C2);
                }
            }
            if (__all(policy.finished(a, T, C0, C1, C2, undrawn))) {
                wave_done = true;
                wave_finished(lds, lane);
                if constexpr (P::COLOUR) quadrants_finished(cl, lane, 1u << wave);
                break;
            }
        }
    }

    blend_stats_out<256, P::COLOUR>(a, t, tid, lane, wave, lds, evaluated, fetched, col_evals);
    store_pixel(a, t.ty, t.px, t.py, T, C0, C1, C2);
}

}  // namespace gsr
