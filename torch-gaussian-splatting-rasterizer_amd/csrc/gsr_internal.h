// gsr_internal.h — shared declarations of libgsr.so (not part of the public ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <stdlib.h>
#include <type_traits>

#include "../../include/gsr.h"

namespace gsr {

// ---------------------------------------------------------------------------------------------
// Device control block at the head of the workspace.  Zeroed at the start of every frame.
// The first 48 bytes are GsrStats verbatim.
// ---------------------------------------------------------------------------------------------
struct FrameCtrl {
    uint32_t n_visible;     // V  (written by the first depth-sort scatter pass)
    uint32_t n_pairs_bbox;  // D  (total of the tile-count scan, before clamping)
    uint32_t n_pairs;       // E  (pairs that survive footprint culling; written by tile-sort pass 0)
    uint32_t overflow;
    uint32_t max_list_len;
    uint32_t sort_passes;   // depth-sort plan of this frame (sort.hip): passes it needs (1..4) — the sorted ids end up in pay[sort_buf] / val[sort_buf]
    unsigned long long wave_entries;  // (quadrant, entry) pairs evaluated by the blend   } totals of blend_stats[], filled in
    unsigned long long fetched_entries;  // list entries staged by the blend              } by gsr_read_stats
    unsigned long long colour_evals;     // deferred colours evaluated by the blend       }
    uint32_t digit_tot[512]; // per-digit totals of the radix pass in flight
    uint32_t stats_off;      // byte offset of blend_stats[] from this struct, and the number of launch slots the last
    uint32_t stats_slots;    // blend filled (tile_order_kernel writes both; 0 = no blend since the frame was reset)
    uint32_t n_slots;        // min(D, max_pairs): pair slots written by the emit kernel
    uint32_t sort_key_bits;  // rest of the depth-sort plan: significant bits of key - bits(0.2f); digit width of the passes
    uint32_t sort_bits_rest; //   after the first.  Written by the pass-0 rowscan (with sort_passes).
    uint32_t n_cpairs;       // coarse binning: 32x32-cell pairs that survive the sort's drop (count of the coarse ranges pass)
    uint32_t n_records;      // multi-GPU shard: records entering the depth sort (= this rank's visible gaussians; preprocess.hip)
    uint32_t ent_off;        // coarse binning without expansion: byte offset (from this struct) of the emit workgroups' partial counts
                             // of tile-list entries; gsr_read_stats totals them into n_pairs.  0: n_pairs is already final.
    // deferred colour (GsrOptions.colour_stage = 0): what the blend needs to evaluate sh_to_rgb for a gaussian it stages — written by
    // the preprocess kernel's workgroup 0 after the clear, so that gsr_blend (which is handed no scene) finds it in the workspace
    const float *col_means;  // GsrScene.means
    const void *col_sh;      // GsrScene.sh
    float col_cc[3];         // GsrCamera.cam_center
    int32_t col_degree;      // GsrScene.sh_degree
    int32_t col_sh16;        // GsrScene.sh_dtype
    uint32_t sort_buf;       // which of pay[] (val[] when the rect does not ride along) the last depth-sort pass that RAN wrote: min(sort_passes, passes enqueued) & 1.
                             // A frame short of passes (flagged, to be re-rendered) still hands binning a buffer this frame's sort filled
    uint32_t depth_key_max;  // maximum of the frame's valid depth keys (pass-0 histogram).  Cleared with the frame AND by the pass-0
                             // rowscan once consumed (gsr_bin_sort may be repeated on one gsr_preprocess).
    // the front slice (FramePlan.front_slice; binning.hip has the sequence): what slice A leaves for the frame's totals.  0 on every
    // other path (cleared with the frame)
    uint32_t front_bbox;     // pair slots of slice A's rects (the first part of D)
    uint32_t front_entries;  // tile-list entries slice A emitted (the first part of E): open_cells_kernel totals A's partial counts
    uint32_t ent_first;      // first emit block whose partial count at ent_off is slice B's (those before it are totalled in front_entries)
    uint32_t _pad0;
    // ---- everything below survives the per-frame clear of a frame rendered with GsrOptions.keep_flags (and of the later views
    // ---- of a batch): the record of what went wrong in ANY frame since the last full clear
    uint32_t batch_overflow;     // bit 0 pair overflow, bit 1 depth sort short of passes
    uint32_t batch_need;         // largest D seen
    uint32_t batch_sort_passes;  // most radix passes any frame's depth sort has needed
    uint32_t _pad1;
};
constexpr int BLEND_STAT_WORDS = 8;  // per launch slot: [0..3] evaluated entries of waves 0..3, [4] staged entries, [5] deferred colours evaluated

// Per-gaussian record consumed by pair emission and the blend (48 B, three 16-B loads):
//   q0 = {mean_x, mean_y, -B/(2C), -B/(2A)}   the two ratios locate the edge maxima in footprint.h
//   q1 = {A, B, C, pthr}    power2(dx,dy) = A dx^2 + B dx dy + C dy^2 (log2 domain); pthr: see footprint.h
//   q2 = {log2(opacity), red, green, blue}     alpha = 2^(power2 + log2(opacity))
struct alignas(16) GaussRec {
    float4 q0, q1, q2;
};

constexpr int DEPTH_SORT_THREADS = 512;  // depth sort: 9-bit digits on 8192-key tiles (radix.h)
constexpr int PAIR_SORT_THREADS = 256;   // pair sort: <= 8-bit digits on 4096-pair tiles
constexpr int DEPTH_SORT_ITEMS = 16;     // keys per thread per pass (2048-key tiles measured slower: fixed per-workgroup costs dominate)
#ifndef GSR_DS_SHARD_ITEMS
#define GSR_DS_SHARD_ITEMS 8
#endif
constexpr int DEPTH_SORT_ITEMS_SHARD = GSR_DS_SHARD_ITEMS;  // (the macro: tools/ A/B builds; 2048-key tiles measured on a rank of 8 with rows in pairs: 0.138 against 0.126 ms per frame)  // a multi-GPU rank's compact records (~0.8 M at G = 8): 4096-key tiles, twice the workgroups, half the serial chain each
constexpr int PAIR_SORT_ITEMS = 16;
constexpr int EMIT_THREADS = 256;                     // threads per workgroup in the binning kernels
constexpr uint32_t KEY_INVALID = 0xFFFFFFFFu;

struct Workspace {
    FrameCtrl *ctrl;
    GaussRec *rec;        // [n]
    ushort4 *rect;        // [n]   tile rect {tx0, ty0, tx1, ty1} (exclusive upper), after footprint refinement.  Written and read only when
                          //       the rect does not travel packed (FramePlan.packed_rect false); on the packed path nobody touches it, and a
                          //       front-slice frame keeps its planes there (front_acc[0], tile_open, cell_open, open_sum)
    uint32_t *rect8[2];   // [n]   the same rect packed x0 | y0<<8 | (x1-1)<<16 | (y1-1)<<24, written per gaussian into rect8[0] when the
                          //       tile grid fits 8 bits (frames up to 4096 px); depth-sort pass 0 moves it into the payload (pay[])
                          //       ([1]: a shard rank's run scratch)
    uint32_t *key[2];     // [n]   depth keys (ping-pong); key[1] also: a shard rank's run scratch (preprocess.hip).  CONTRACT: dead between
                          //       the last pass of launch_depth_sort and the next preprocess — nothing after the sort reads a key — and key[1]
                          //       follows key[0] at align_up(4 n, 256) (carve_workspace checks it): a front-slice frame, which is never
                          //       a shard's, keeps front_acc[1] and blk_full over the two.  A new reader of keys behind the sort, or a
                          //       new array carved between them, must take the overlay out of carve_workspace first
    uint32_t *val[2];     // [n]   gaussian ids (ping-pong) — the depth sort's payload when the rect does not ride along; val[0] also: a
                          //       shard rank's compacted ids entering pass 0
    uint2 *pay[2];        // [n]   {gaussian id, rect8}: the depth sort's payload from pass 0's output on when the rect rides along
                          //       (ping-pong).  No bytes of its own: pay[b] lies over val[b] and rect8[b], which are side by side
    uint32_t *pair_off;   // [n]   exclusive pair offsets in depth order
    uint32_t *blk_sum;    // [ceil(n/EMIT_THREADS)+1]
    uint32_t *hist;       // [512 * hist_blocks] digit-major: hist[digit][block]
    uint32_t *pkey[2];    // [max_pairs] tile ids
    uint32_t *pval[2];    // [max_pairs] gaussian ids
    uint2 *ranges;        // [tiles]
    uint2 *cranges;       // [ctiles]  coarse binning: [begin, end) of every 32x32 cell's list in the sorted pair array
    int *tile_order;      // [8 * ceil(tiles_y/8) * tiles_x] blend launch order
    unsigned char *blk_dead; // [ceil(n / GSR_BOUNDS_BLOCK)] block-level culling: 1 = the preprocess skips the block (preprocess.hip, block_flags_kernel)
    uint32_t *tile_work;  // [tiles] 1 + entries the tile's blend staged in the LAST frame rendered on this workspace (0 / garbage: unknown):
                          // the launch-order hint of the next frame (blend.hip, tile_order_kernel); never cleared, never trusted
    uint32_t *blend_stats; // [tile_order slots][BLEND_STAT_WORDS] per-workgroup counters: plain stores, no atomics (40 k
                          // same-address atomics per frame put a 0.45 ms floor under the blend kernel)
    // the front slice (FramePlan.front_slice): no bytes of their own — they lie over rect[] and key[] (carve_workspace), dead on the
    // coarse path once the depth sort has run.  front_fits: there is room for them
    bool front_fits;
    float4 *front_acc[2]; // [tiles][128] each: {T, Cr, Cg, Cb} of the first / second pixel of every thread of a tile slice A left open, as its blend's registers held them
    unsigned char *tile_open;  // [tiles] 1: slice A's list ended with a quadrant of the tile still live
    unsigned char *cell_open;  // [ctiles] bit q: tile q of the 32x32 cell is open
    uint32_t *open_sum;   // [(ctiles_y + 1) * (ctiles_x + 1)] open_sum[y][x] = open cells in rows < y and columns < x
    uint32_t *blk_full;   // [like blk_sum] slice B: pair slots of each emit block's rects before the open-cell test (for D)
    int64_t n;
    int64_t max_pairs;
    int tiles_x, tiles_y;
    int ctiles_x, ctiles_y;  // 32x32 cells = 2x2 tiles
    int hist_blocks;      // row stride of `hist`
    size_t bytes;
    // Several views through ONE launch sequence (gsr_render_batch): every kernel of the render path is launched with gridDim.y = views
    // and view v works on the v-th slice of the caller's workspace.  The pointers above are view 0's; slice v lies v * view_stride
    // bytes further (a slice is a complete one-view workspace: gsr_read_stats reads any of them).
    int views = 1;
    size_t view_stride = 0;
};
constexpr int MAX_VIEWS = 8;  // views per launch sequence (the cameras travel in the preprocess kernel's argument block)

// p + off bytes, as pointer arithmetic (a round trip through an integer would hide from the compiler that the result still points into the
// kernel argument's global buffer: flat loads instead of global / scalar ones).
template <typename T>
__device__ __forceinline__ T *view_at(T *p, size_t off)
{
    using Byte = std::conditional_t<std::is_const<T>::value, const char, char>;
    return reinterpret_cast<T *>(reinterpret_cast<Byte *>(p) + off);
}
__device__ __forceinline__ void *view_at(void *p, size_t off) { return static_cast<char *>(p) + off; }
// The v-th view's instance of a workspace pointer (v = blockIdx.y; the host passes view 0's).  nullptr stays nullptr.
template <typename T>
__device__ __forceinline__ T *view_slice(T *p, size_t view_stride)
{
    return p == nullptr ? nullptr : view_at(p, (size_t)blockIdx.y * view_stride);
}

// Carves `base` (may be nullptr to only size).  Returns total bytes.
size_t carve_workspace(void *base, int64_t n, int width, int height, int64_t max_pairs, Workspace *ws);

void set_error(const char *fmt, ...);
int hip_fail(hipError_t e, const char *what);

#define GSR_HIP(call)                                      \
    do {                                                   \
        hipError_t e__ = (call);                           \
        if (e__ != hipSuccess) return gsr::hip_fail(e__, #call); \
    } while (0)

// Which tile rows a rank owns (multi-GPU sharding, GsrOptions.tile_row_begin / _step / _block): blocks of 2^bshift consecutive tile
// rows, block b is the rank's when b % step == begin.  bshift 0: the rows begin, begin + step, ...; bshift 1: pairs of rows = the
// tile rows of one 32x32 cell row.  The rank's rows in ascending order are its STRIP rows (output_layout = 2): index k <-> row_at(k).
struct RowShard {
    int begin, step, bshift;
    // how many of the rank's rows lie below tile row t (t >= 0) = strip index of its first row >= t
    __host__ __device__ __forceinline__ int rows_before(int t) const
    {
        if (step <= 1) return t;
        const int b = t >> bshift, q = b / step, r = b - q * step;
        int k = (q + (begin < r ? 1 : 0)) << bshift;         // whole blocks of the rank below block b
        if (r == begin) k += t & ((1 << bshift) - 1);        // t lies inside one of its blocks: that block's rows below t
        return k;
    }
    __host__ __device__ __forceinline__ int row_at(int k) const
    {
        if (bshift == 0) return k * step + begin;
        return ((((k >> bshift) * step) + begin) << bshift) | (k & ((1 << bshift) - 1));
    }
    __host__ __device__ __forceinline__ bool owns(int t) const { return step <= 1 || (t >> bshift) % step == begin; }
    // strip index of a row the rank owns
    __host__ __device__ __forceinline__ int index_of(int t) const { return (((t >> bshift) / step) << bshift) | (t & ((1 << bshift) - 1)); }
    // any of the rank's rows in [t0, t1)?
    __host__ __device__ __forceinline__ bool any_in(int t0, int t1) const { return t1 > t0 && (step <= 1 || rows_before(t1) > rows_before(t0)); }
};
inline RowShard row_shard_of(const GsrOptions &o)
{
    return RowShard{o.tile_row_begin, o.tile_row_step < 1 ? 1 : o.tile_row_step, o.tile_row_block == 2 ? 1 : 0};
}

// ---- the frame's plan -----------------------------------------------------------------------------
// Every host-side choice a frame makes: which kernel variants run and which buffer each stage leaves its result in.  Decided once per
// entry point by plan_frame (api.hip), where the reasons stand; the launchers below read their choices from it and derive none.
enum class BlendKernel {
    Tile,       // blend_kernel<ColourBlend<false>>: one workgroup per tile, fp32 accumulators (GsrOptions.blend_impl = 1)
    TileBf16,   // blend_kernel<ColourBlend<true>>: the same with bf16 accumulators (GsrOptions.accum_dtype = 1)
    Walk2,      // blend_walk_kernel<2, false>: two quadrants per wave
    Walk1,      // blend_walk_kernel<1, false>: one quadrant per wave
    Walk1Pipe,  // blend_walk_kernel<1, true>: one quadrant per wave, pipelined
};
constexpr int COARSE_ID_BITS = 28;  // coarse pairs: value = gaussian id | (mask of the cell's tiles the gaussian reaches) << 28
struct FramePlan {
    // stage 1 (preprocess.hip)
    bool packed_rect;      // the tile rect is written packed into rect8[0] and rides through the depth sort beside the id (one uint2, pay[]); else ushort4 in rect[], gathered by id
    bool compact_input;    // the three-phase shard kernel hands the depth sort compact (key, id, rect) records; else the whole-frame kernel (its K-view form when ws.views > 1) one key per gaussian
    RowShard rs;           // the rank's tile rows
    RowShard cull_rs;      // the rows block-level culling tests a block against
    // depth sort (sort.hip)
    int depth_passes;      // radix passes enqueued (1..4)
    int depth_items;       // keys per thread: DEPTH_SORT_ITEMS or DEPTH_SORT_ITEMS_SHARD
    // binning and pair sort (binning.hip, sort.hip).  Pair keys: (grid row << bits_x) | grid column; culled pairs carry the row
    // grid_y and are dropped from drop_from on
    bool coarse;           // pairs are generated and sorted per 32x32 cell (grid = cells); else per tile
    int grid_x, grid_y, bits_x, bits_y;
    uint32_t drop_from;
    RowShard csh;          // the cell rows the rank's tile rows fall into
    bool key16;            // pair keys are uint16_t in memory (the first half of each pkey buffer)
    int pair_passes, pair_bits_pp;  // radix passes of the pair sort, and key bits each takes (the last: what is left)
    int lists_buf;         // pval[lists_buf] holds the lists (gaussian ids [| tile mask << COARSE_ID_BITS]) that ranges[] / cranges[] index after launch_binning
    // blend (blend.hip)
    bool cell_lists;       // the blend filters the 32x32-cell lists by tile bit itself
    int rows;              // tile rows the rank blends
    BlendKernel blend;
    // the front slice: the nearest 1 / FRONT_SLICE_FRACTION of the draw order is binned and blended first, the rest is binned only where a
    // tile is still open after it (binning.hip has the sequence and why the frame is the single pass's bit for bit)
    bool front_slice;
};
#ifndef GSR_FRONT_SLICE_FRACTION
#define GSR_FRONT_SLICE_FRACTION 8
#endif
constexpr uint32_t FRONT_SLICE_FRACTION = GSR_FRONT_SLICE_FRACTION;  // (the macro: the sweep builds of csrc/Makefile, libgsr_fsfrac%.so)
// ws: after check_frame, with ws.views set.  colour_frame: the fused colour-frame entries without a final-T output (render_views) — the
// only callers that may be handed a front slice
FramePlan plan_frame(const Workspace &ws, const GsrOptions &opts, bool colour_frame = false);

// A view's camera as the per-gaussian kernels hold it (preprocess.hip, project_backward.hip): a kernel argument
struct Cam {
    float V[16];
    float F[16];
    float cc[3];
    float fx, fy, limx, limy;
    float w_sigma2;  // largest eigenvalue of A^T A, A = w2c[:3,:3] (1 for a unit qvec), padded: bounds |J A| in the shard kernel's phase 1
    int W, H;
};
Cam make_cam(const GsrCamera &c);  // preprocess.hip

// ---- kernels' host launchers (each returns GSR_OK / GSR_ERR_HIP) --------------------------------
// cams: ws.views cameras (one frame size); ctrl_reset_words: how much of each view's control block the frame clears
int launch_preprocess(const GsrScene &scene, const GsrCamera *cams, const GsrOptions &opts, const Workspace &ws, const FramePlan &plan,
                      const GsrDebugOut *dbg, int ctrl_reset_words, hipStream_t s);
int launch_block_visibility(const GsrScene &scene, const GsrCamera &cam, const FramePlan &plan, unsigned char *dead, hipStream_t s);
int launch_scene_bounds(int64_t n, const float *means, const float *log_scales, float *bounds, hipStream_t s);
int launch_sh_to_rgb(int64_t n, const float *means, const float *sh, const float cc[3], int degree, float *rgb, hipStream_t s);
int launch_cov3d(int64_t n, const float *log_scales, const float *quats, float *out, hipStream_t s);
int launch_project(int64_t n, const float *means, const float w2c[16], float *out, hipStream_t s);
int launch_cov2d(int64_t n, const float *cov3d, const float *cam_means, const float w2c[16], float fx, float fy, float limx, float limy,
                 float *out, hipStream_t s);
int launch_bbox(int64_t n, const float *screen_means, const float *cov2d, float W, float H, int64_t *out, hipStream_t s);
int launch_rasterize_gaussian(int64_t g, const int64_t *bboxes, float *screen, const float *screen_means, const float *sigmas,
                              const float *rgb, float *opacity_buffer, const float *opacity, int W, int H, hipStream_t s);

// Depth order (sort.hip): stable LSD radix sort of the depth keys; leaves V in FrameCtrl.n_visible and the sorted ids (+ packed
// rects) in pay[p] — val[p] without the rects —, p = FrameCtrl.sort_buf (decided on the device from the frame's key range).
int launch_depth_sort(const Workspace &ws, const FramePlan &plan, hipStream_t s);
// gsr_scene_order (sort.hip): Morton-curve permutation of the gaussians, built with the radix passes of the pair sort
size_t scene_order_bytes(int64_t n);
int launch_scene_order(int64_t n, const float *means, uint32_t *perm_out, void *workspace, hipStream_t s);
// Stable radix sort of the pair arrays in pkey[0] / pval[0] by the plan's keys (sort.hip); needs max_pairs > 0
int launch_pair_sort(const Workspace &ws, const FramePlan &plan, const uint32_t *n_dev, uint32_t *n_out, int *result_buf, hipStream_t s);
// Stage 2b: pairs of the depth-sorted gaussians -> per-tile depth-ordered lists + ranges[] (count, scan, emit, sort, ranges,
// and with coarse binning the expansion).
// slice (plan.front_slice only): 0 = the whole draw order; 1 = slice A, its first 1 / FRONT_SLICE_FRACTION; 2 = slice B, the rest, where open
int launch_binning(const GsrOptions &opts, const Workspace &ws, const FramePlan &plan, hipStream_t s, int slice = 0);
// Between the slices: cell_open[], open_sum[] from slice A's tile_open[], and A's share of E into the control block
int launch_open_cells(const Workspace &ws, hipStream_t s);
// out_image: view 0's frame, view v's lies v * out_view_stride BYTES further (out_T: single views only).  scene: where deferred
// colours are evaluated from (single views only); nullptr = what the preprocess left in the workspace's control block
int launch_blend(const GsrCamera &cam, const GsrOptions &opts, const Workspace &ws, const FramePlan &plan, void *out_image,
                 size_t out_view_stride, float *out_T, const GsrScene *scene, hipStream_t s, int slice = 0);
// The blend's launch order (blend.hip, tile_order_kernel): returns the launch slots per view; use_hint: by what each tile staged last frame
int launch_tile_order(const Workspace &ws, const FramePlan &plan, bool use_hint, hipStream_t s, int slice = 0);
// Stage 3 for caller-supplied channels (blend_features.hip): out_map[p] = sum_i w_i(p) features[i], single views only
int launch_blend_features(const GsrCamera &cam, const GsrOptions &opts, const Workspace &ws, const FramePlan &plan, const float *features,
                          float *out_map, float *out_T, hipStream_t s);
// The same for `channels` channels, rows `stride` floats apart, up to 16 channels per walk (blend_channels.hip): one launch per group.
// ws.views views per launch: view v writes out_map + v * map_view_stride and out_T + v * T_view_stride (floats); all read `features`
int launch_blend_channels(const GsrCamera &cam, const GsrOptions &opts, const Workspace &ws, const FramePlan &plan, const float *features,
                          int channels, int64_t stride, float *out_map, float *out_T, hipStream_t s, int64_t map_view_stride = 0,
                          int64_t T_view_stride = 0);
// The transpose of launch_blend_channels in the channels (blend_channels_backward.hip): grad_features[i] += sum_p w_i(p) grad_map[p].
// ws.views views per launch: view v reads grad_map + v * map_view_stride (floats); all add into the one grad_features
int launch_blend_channels_backward(const GsrCamera &cam, const GsrOptions &opts, const Workspace &ws, const FramePlan &plan,
                                   const float *grad_map, int channels, float *grad_features, int64_t stride, hipStream_t s,
                                   int64_t map_view_stride = 0);
// Stage 3 for ids (blend_pick.hip): per pixel the gaussian of largest weight (+ that weight), the first one after which T < median_T,
// and (out_count != nullptr: the COUNT kernel) how many had w > 0.  Any output may be null; single views only
int launch_blend_pick(const GsrCamera &cam, const GsrOptions &opts, const Workspace &ws, const FramePlan &plan, float median_T,
                      int32_t *out_best_id, float *out_best_w, int32_t *out_median_id, int32_t *out_count, hipStream_t s);
// Stage 3 for contributor lists (blend_topk.hip): per pixel the k heaviest (select 0) or nearest (1) gaussians with w > 0, ids and
// weights [.., k]; one of the two may be null, out_final_T may be (and then the walk stops once no list can change); single views only
int launch_blend_topk(const GsrCamera &cam, const GsrOptions &opts, const Workspace &ws, const FramePlan &plan, int k, int select,
                      int32_t *out_ids, float *out_weights, float *out_final_T, hipStream_t s);
// Stage 3 for channels between two per-pixel depth limits (blend_slab.hip): launch_blend_channels restricted, per pixel, to the
// gaussians with near <= z_cam < far; either plane may be null (no limit); means null: the pointer the preprocess left in the
// control block; single views only
int launch_blend_slab(const GsrCamera &cam, const GsrOptions &opts, const Workspace &ws, const FramePlan &plan, const float *means,
                      const float *features, int channels, int64_t stride, const float *depth_near, const float *depth_far,
                      float *out_map, float *out_T, hipStream_t s);
// Per-gaussian statistics of the view's weights over the counted pixels (blend_gstats.hip): weight_sum[i] += sum_p w_i(p),
// weight_max[i] = max(old, max_p w_i(p)), pixels[i] += #{p : w_i(p) > 0}; any of the three may be null, not all; pixel_mask null: every
// drawn pixel counts.  ws.views views per launch: view v reads pixel_mask + v * mask_view_stride bytes and all accumulate into the
// three arrays; view_hits[i] (may be null, may be the only output) += the views that reach gaussian i with w > 0 in a counted pixel,
// through view_bits [n], a scratch the caller has cleared on the stream
int launch_blend_gstats(const GsrCamera &cam, const GsrOptions &opts, const Workspace &ws, const FramePlan &plan, const uint8_t *pixel_mask,
                        float *weight_sum, float *weight_max, uint32_t *pixels, hipStream_t s, int64_t mask_view_stride = 0,
                        uint32_t *view_hits = nullptr, uint32_t *view_bits = nullptr);
// The gradient of a feature map (and of the final T) with respect to the 2-D splat (blend_splat_backward.hip): row i of grad_splat
// [n][8] += {d/d opacity, d/d mean x, y, d/d sigma 0, 1, 2, and with want_abs the per-pixel absolute mean terms}; grad_T may be
// null; want_abs: channels <= 16; single views only
int launch_blend_splat_backward(const GsrCamera &cam, const GsrOptions &opts, const Workspace &ws, const FramePlan &plan,
                                const float *features, int64_t stride, int channels, const float *grad_map, const float *grad_T,
                                float min_T, bool want_abs, float *grad_splat, hipStream_t s);
// The transpose of stage 1's geometry (project_backward.hip): row i of grad_splat [n][8] (columns 0-5) chained to gaussian i's mean,
// log-scales, quaternion and opacity logit, ADDED into the four arrays that are not null; no workspace, no lists
int launch_project_backward(const GsrScene &scene, const GsrCamera &cam, const GsrOptions &opts, const float *grad_splat, float *grad_means,
                            float *grad_log_scales, float *grad_quats, float *grad_opacity_logit, hipStream_t s);
// The transpose of sh_to_rgb (sh_backward.hip): row i of grad_rgb (columns 0-2, rows grad_stride floats apart) carried to gaussian
// i's SH coefficients and, through the view direction, to its mean; ADDED into the two arrays that are not null; no workspace
int launch_sh_backward(const GsrScene &scene, const GsrCamera &cam, const float *grad_rgb, int64_t grad_stride, float *grad_sh,
                       float *grad_means, hipStream_t s);
// The splat gradient of a view chained to the camera (camera_backward.hip): 32 doubles WRITTEN to grad_camera, the partial sums in
// `workspace` (camera_backward_bytes(n), a function of n alone); either input may be null, not both; no atomics, fixed order
size_t camera_backward_bytes(int64_t n);
int launch_camera_backward(const GsrScene &scene, const GsrCamera &cam, const GsrOptions &opts, const float *grad_splat,
                           const float *grad_view_means, double *grad_camera, void *workspace, hipStream_t s);
int launch_blend_stats(FrameCtrl *ctrl, size_t workspace_bytes, hipStream_t s);

// ---- small device helpers -----------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// Exclusive scan across a workgroup of THREADS = 64 * WAVES threads.  `scratch` = 2 * WAVES uint32 of LDS.  Returns the
// exclusive prefix of `v`; *total receives the workgroup sum.  Contains two __syncthreads().
template <int THREADS>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *scratch, uint32_t *total)
{
    constexpr int WAVES = THREADS / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = wave_incl_scan(v);
    if (lane == 63) scratch[wave] = incl;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const uint32_t s = scratch[w];
        if (w < wave) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + incl - v;
}

}  // namespace gsr
