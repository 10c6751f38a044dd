// blend_common.h — what every blend kernel shares (blend.hip: the colour frame; blend_features.hip: caller-supplied channels):
// the per-(pixel, entry) arithmetic and the staging of a tile's depth-ordered list.
#pragma once
#include "gsr_internal.h"
#include "blend_args.h"

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
        const unsigned long long lt = (1ull << lane) - 1ull;
        const uint32_t tail = t.head + t.qlen;
        if (f0) s_ring[(tail + o0 + (uint32_t)__popcll(b0 & lt)) & (RING - 1)] = v0 & LIST_ID_MASK;
        if (f1) s_ring[(tail + tot0 + o1 + (uint32_t)__popcll(b1 & lt)) & (RING - 1)] = v1 & LIST_ID_MASK;
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

}  // namespace gsr
