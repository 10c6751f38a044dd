// blend_features.hip — stage 3 for caller-supplied channels: out[p] = sum_i w_i(p) f_i over the tile's depth-ordered list, with the
// weights w_i = alpha_i T_i of the colour frame (blend.hip) and three fp32 values f_i per gaussian from the caller's array instead of
// the record's colour.  Depth is f = z_cam, accumulated alpha f = 1; precomputed colours, normals, feature vectors, ids the same.
//
// The kernel is the plain-C colour kernel's (blend_common.h, blend_kernel: one 256-thread workgroup per 16x16 tile, wave = 8x8
// quadrant, lane = pixel) under another policy: the same lists (per-tile ranges or the 32x32-cell lists filtered by tile bit), the
// same footprint test by wave ballot, the same blend_one per survivor — so with f = the gaussians' colours the map IS the colour
// frame, bit for bit.  What the policy changes:
//   - the third LDS plane is {log2 opacity, f0, f1, f2}: ONE 4-byte load of the record's q2.x and three of the caller's array.  The
//     record's colour words are neither read nor written: with GsrOptions.colour_stage = 0 they may still be the "unevaluated"
//     negatives and stay so, and tile_work (the colour frames' launch-order hint) is only read.  A gsr_blend on the same workspace,
//     before or after, renders the bits it renders alone.
//   - the stop rule is T alone: a quadrant stops once T <= early_out_T for its 64 pixels; with 0 that is T == 0.0f, which is exact
//     for finite f (w = alpha T = 0 and fma(0, f, C) = C).  The colour frame's T <= 2^-25 min C rests on 0 <= c <= 1 and does not
//     carry over to signed or unbounded channels.
// 52 B per staged entry (32 of the record's q0 / q1, 4 of q2, 12 of the features, 4 of the list) from three lines instead of 48 from
// one and the list's.  No deferred colour evaluation lives in this kernel, which is why it fits 64 VGPRs = 8 waves per SIMD where
// the colour policy needs 93 (DESIGN.md has the measured time against it).
#include "gsr_internal.h"
#include "blend_args.h"
#include "blend_common.h"

namespace gsr {

// blend_common.h's blend_kernel with this policy is the kernel.
struct FeatureBlend {
    static constexpr bool COLOUR = false;  // stat[5] = 0, tile_work untouched
    static constexpr int MIN_WAVES = 8;
    const float *__restrict__ features;  // [n][3]
    __device__ float4 stage(const BlendArgs &a, uint32_t id, uint32_t &) const
    {
        const float *f = features + 3 * (size_t)id;
        return make_float4(ldg(&a.rec[id].q2.x, 0), ldg(f, 0), ldg(f, 1), ldg(f, 2));
    }
    __device__ void acc_round(float &, float &, float &, float &) const {}
    __device__ bool finished(const BlendArgs &a, float T, float, float, float, bool) const
    {
        return T <= a.early_T;  // (a negative threshold never fires: "blend every entry")
    }
};

int launch_blend_features(const GsrCamera &cam, const GsrOptions &opts, const Workspace &ws, const FramePlan &plan, const float *features,
                          float *out_map, float *out_T, hipStream_t s)
{
    if (ws.views > 1) { set_error("feature maps: single views only"); return GSR_ERR_BAD_ARG; }
    const BlendArgs a = blend_args_common(cam, opts, ws, plan, out_map, out_T);  // tile_work stays null: never written here
    if (a.rows <= 0 || a.tiles_x <= 0) return GSR_OK;
    // heaviest tiles first, by what the last colour blend on this workspace staged where that is known (a schedule only)
    const int slots = launch_tile_order(ws, plan, true, s);
    hipLaunchKernelGGL(blend_kernel<FeatureBlend>, dim3((unsigned)slots), dim3(256), 0, s, a, FeatureBlend{features});
    GSR_HIP(hipGetLastError());
    return GSR_OK;
}

}  // namespace gsr
