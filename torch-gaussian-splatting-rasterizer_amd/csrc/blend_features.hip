// blend_features.hip — stage 3 for caller-supplied channels: out[p] = sum_i w_i(p) f_i over the tile's depth-ordered list, with the
// weights w_i = alpha_i T_i of the colour frame (blend.hip) and three fp32 values f_i per gaussian from the caller's array instead of
// the record's colour.  Depth is f = z_cam, accumulated alpha f = 1; precomputed colours, normals, feature vectors, ids the same.
//
// The structure is blend_kernel's (blend.hip, the plain-C statement of the blend): one 256-thread workgroup per 16x16 tile, wave =
// 8x8 quadrant, lane = pixel; the same lists (blend_common.h: per-tile ranges or the 32x32-cell lists filtered by tile bit), the
// same footprint test by wave ballot, the same blend_one per survivor — so with f = the gaussians' colours the map IS the colour
// frame, bit for bit.  What differs:
//   - the third LDS plane is {log2 opacity, f0, f1, f2}: ONE 4-byte load of the record's q2.x and three of the caller's array.  The
//     record's colour words are neither read nor written: with GsrOptions.colour_stage = 0 they may still be the "unevaluated"
//     negatives and stay so, and tile_work (the colour frames' launch-order hint) is only read.  A gsr_blend on the same workspace,
//     before or after, renders the bits it renders alone.
//   - the stop rule is T alone: a quadrant stops once T <= early_out_T for its 64 pixels; with 0 that is T == 0.0f, which is exact
//     for finite f (w = alpha T = 0 and fma(0, f, C) = C).  The colour frame's T <= 2^-25 min C rests on 0 <= c <= 1 and does not
//     carry over to signed or unbounded channels.
// 52 B per staged entry (32 of the record's q0 / q1, 4 of q2, 12 of the features, 4 of the list) from three lines instead of 48 from
// one and the list's.  No deferred colour evaluation lives in this kernel, which is why it fits 64 VGPRs = 8 waves per SIMD where
// blend_kernel needs 93 (DESIGN.md has the measured time against it).
#include "gsr_internal.h"
#include "blend_args.h"
#include "blend_common.h"
#include "footprint.h"

namespace gsr {

__global__ __launch_bounds__(256, 8) void blend_features_kernel(BlendArgs a, const float *__restrict__ features)
{
    __shared__ float4 srec[3][256];  // staged entries, one plane per 16-B part: q0, q1, {log2 opacity, f0, f1, f2}
    float4 *const s0 = srec[0], *const s1 = srec[1], *const s2 = srec[2];
    __shared__ int s_done;
    __shared__ uint32_t s_ring[TileList<256>::RING], s_wc[2 * TileList<256>::WAVES];

    const int tile = a.order[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t *stat = a.stats + (size_t)blockIdx.x * BLEND_STAT_WORDS;
    if (tile < 0) {  // uniform: empty launch slot
        if (tid < BLEND_STAT_WORDS) stat[tid] = 0;
        return;
    }
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;

    const int qx = tx * 16 + (wave & 1) * 8, qy = ty * 16 + (wave >> 1) * 8;
    const int px = qx + (lane & 7), py = qy + (lane >> 3);
    const float fpx = (float)px, fpy = (float)py;
    const float qx0 = (float)qx, qx1 = (float)(qx + 7), qy0 = (float)qy, qy1 = (float)(qy + 7);

    TileList<256> list = tile_list_of<256>(a, tile, tx, ty);
    float T = 1.0f, C0 = 0.0f, C1 = 0.0f, C2 = 0.0f;
    bool wave_done = false;
    uint32_t evaluated = 0;  // wave-uniform
    uint32_t fetched = 0;    // workgroup-uniform
    if (tid == 0) s_done = 0;

    for (;;) {
        __syncthreads();  // previous batch fully consumed (and s_done initialised); a refilled ring published
        if (s_done == 4) break;  // uniform: every wave saturated
        uint32_t id = 0;
        const int nb = tile_list_next<256>(a, list, s_ring, s_wc, &id);
        if (nb < 0) continue;
        if (nb == 0) break;
        fetched += (uint32_t)nb;
        if (tid < nb) {
            const GaussRec *r = a.rec + id;
            const float *f = features + 3 * (size_t)id;
            s0[tid] = r->q0;
            s1[tid] = r->q1;
            s2[tid] = make_float4(ldg(&r->q2.x, 0), ldg(f, 0), ldg(f, 1), ldg(f, 2));
        }
        __syncthreads();
        if (wave_done) continue;
        for (int chunk = 0; chunk < nb; chunk += 64) {
            const int e = chunk + lane;
            const bool hit = e < nb && footprint_hits_rect(s0[e], s1[e], qx0, qx1, qy0, qy1);
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
                    blend_one(gb, cb, ob, fpx, fpy, T, C0, C1, C2);
                } else {
                    blend_one(ga, ca, oa, fpx, fpy, T, C0, C1, C2);
                }
            }
            if (__all(T <= a.early_T)) {  // (a negative threshold never fires: "blend every entry")
                wave_done = true;
                if (lane == 0) atomicAdd(&s_done, 1);
                break;
            }
        }
    }

    // the counters gsr_read_stats totals; tile_work stays what the last colour blend left
    if (lane == 0) stat[wave] = evaluated;
    if (tid == 0) { stat[4] = fetched; stat[5] = 0; }
    if (px < a.W && py < a.H) {
        const bool drawn = px < a.xlim && py < a.ylim;  // Q1: last column / row stay 0, T stays 1
        const size_t pix = a.layout == 0 ? (size_t)py * a.W + px                                           // [H,W,3]
                         : a.layout == 1 ? (size_t)px * a.H + py                                           // [W,H,3]
                                         : (size_t)(a.rs.index_of(ty) * 16 + (py - ty * 16)) * a.W + px;  // strip
        float *p = static_cast<float *>(a.out) + pix * 3;
        p[0] = drawn ? C0 : 0.0f; p[1] = drawn ? C1 : 0.0f; p[2] = drawn ? C2 : 0.0f;
        if (a.out_T) a.out_T[pix] = drawn ? T : 1.0f;
    }
}

int launch_blend_features(const GsrCamera &cam, const GsrOptions &opts, const Workspace &ws, const FramePlan &plan, const float *features,
                          float *out_map, float *out_T, hipStream_t s)
{
    if (ws.views > 1) { set_error("feature maps: single views only"); return GSR_ERR_BAD_ARG; }
    BlendArgs a = {};
    a.ranges = ws.ranges;
    a.cranges = ws.cranges;
    a.ctiles_x = ws.ctiles_x;
    a.cell_lists = plan.cell_lists ? 1 : 0;
    a.pval = ws.pval[plan.lists_buf];
    a.rec = ws.rec;
    a.ctrl = ws.ctrl;
    a.out = out_map;
    a.out_T = out_T;
    a.stats = ws.blend_stats;
    a.tile_work = nullptr;  // never written here
    a.order = ws.tile_order;
    a.W = cam.width; a.H = cam.height;
    a.xlim = opts.reference_compat ? cam.width - 1 : cam.width;
    a.ylim = opts.reference_compat ? cam.height - 1 : cam.height;
    a.tiles_x = ws.tiles_x;
    a.rs = plan.rs;
    a.rows = plan.rows;
    a.layout = opts.output_layout;
    a.early_T = opts.early_out_T;
    if (a.rows <= 0 || a.tiles_x <= 0) return GSR_OK;
    // heaviest tiles first, by what the last colour blend on this workspace staged where that is known (a schedule only)
    const int slots = launch_tile_order(ws, plan, true, s);
    hipLaunchKernelGGL(blend_features_kernel, dim3((unsigned)slots), dim3(256), 0, s, a, features);
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

}  // namespace gsr
