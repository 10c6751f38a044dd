// api.hip — the extern "C" surface of libgsr.so (include/gsr.h) and its host-side logic.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstddef>
#include <cstring>

#include "gsr_internal.h"

namespace gsr {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

int hip_fail(hipError_t e, const char *what)
{
    set_error("HIP error %d (%s) in %s", (int)e, hipGetErrorString(e), what);
    return GSR_ERR_HIP;
}

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

size_t carve_workspace(void *base, int64_t n, int width, int height, int64_t max_pairs, Workspace *ws)
{
    char *p = static_cast<char *>(base);
    size_t off = 0;
    auto take = [&](size_t bytes) -> void * {
        void *r = p ? p + off : nullptr;
        off = align_up(off + bytes, 256);
        return r;
    };
    const size_t nn = (size_t)std::max<int64_t>(n, 1), np = (size_t)std::max<int64_t>(max_pairs, 1);
    ws->n = n;
    ws->max_pairs = max_pairs;
    ws->tiles_x = (width + GSR_TILE - 1) / GSR_TILE;
    ws->tiles_y = (height + GSR_TILE - 1) / GSR_TILE;
    ws->ctiles_x = (ws->tiles_x + 1) / 2;
    ws->ctiles_y = (ws->tiles_y + 1) / 2;
    // row stride of the histogram table: tiles of the depth sort, tiles of the pair sort
    ws->hist_blocks = (int)std::max((nn + DEPTH_SORT_THREADS * DEPTH_SORT_ITEMS_SHARD - 1) / (DEPTH_SORT_THREADS * DEPTH_SORT_ITEMS_SHARD),
                                    (np + PAIR_SORT_THREADS * PAIR_SORT_ITEMS - 1) / (PAIR_SORT_THREADS * PAIR_SORT_ITEMS));
    ws->ctrl = static_cast<FrameCtrl *>(take(sizeof(FrameCtrl)));
    ws->rec = static_cast<GaussRec *>(take(sizeof(GaussRec) * nn));
    ws->rect = static_cast<ushort4 *>(take(sizeof(ushort4) * nn));
    for (int b = 0; b < 2; ++b) ws->key[b] = static_cast<uint32_t *>(take(4 * nn));
    // val[b] and rect8[b] side by side: together they are pay[b], the depth sort's 8-byte {id, rect8} payload (sort.hip).  Pass 0 reads
    // val[0] / rect8[0] (what the preprocess wrote) and writes pay[1]; pay[0] is first written by pass 1
    for (int b = 0; b < 2; ++b) {
        ws->val[b] = static_cast<uint32_t *>(take(4 * nn));
        ws->rect8[b] = static_cast<uint32_t *>(take(4 * nn));
        ws->pay[b] = reinterpret_cast<uint2 *>(ws->val[b]);
    }
    ws->blk_dead = static_cast<unsigned char *>(take((nn + GSR_BOUNDS_BLOCK - 1) / GSR_BOUNDS_BLOCK));  // (with the per-gaussian arrays: stage 1 carves with max_pairs = 0)
    ws->blk_sum = static_cast<uint32_t *>(
        take(4 * ((std::max(nn, (size_t)ws->tiles_x * ws->tiles_y) + EMIT_THREADS - 1) / EMIT_THREADS + 1)));
    ws->hist = static_cast<uint32_t *>(take(4 * 512 * (size_t)ws->hist_blocks));
    for (int b = 0; b < 2; ++b) ws->pkey[b] = static_cast<uint32_t *>(take(4 * np));
    for (int b = 0; b < 2; ++b) ws->pval[b] = static_cast<uint32_t *>(take(4 * np));
    ws->ranges = static_cast<uint2 *>(take(sizeof(uint2) * (size_t)ws->tiles_x * ws->tiles_y));
    ws->cranges = static_cast<uint2 *>(take(sizeof(uint2) * (size_t)ws->ctiles_x * ws->ctiles_y));
    const size_t order_slots = 8 * (size_t)((ws->tiles_y + 7) / 8) * ws->tiles_x;
    ws->tile_order = static_cast<int *>(take(sizeof(int) * order_slots));
    ws->blend_stats = static_cast<uint32_t *>(take(sizeof(uint32_t) * BLEND_STAT_WORDS * order_slots));
    ws->tile_work = static_cast<uint32_t *>(take(sizeof(uint32_t) * (size_t)ws->tiles_x * ws->tiles_y));
    // The front slice (plan_frame) takes no bytes of its own: its planes and tables lie over per-gaussian arrays that nobody reads
    // between the depth sort and the next preprocess on the coarse path — rect[] (the rect travels packed, in rect8[]) and the
    // depth keys key[0], key[1] (the sort has consumed them).  16 B per pixel of the frame, in two halves: a scene of fewer than
    // ~257 gaussians per tile has no room for them, and front_fits says so.
    {
        const size_t tiles = (size_t)ws->tiles_x * ws->tiles_y, cells = (size_t)ws->ctiles_x * ws->ctiles_y;
        const size_t half = align_up(sizeof(float4) * 128 * tiles, 256);
        char *r1 = reinterpret_cast<char *>(ws->rect), *r2 = reinterpret_cast<char *>(ws->key[0]);
        const size_t r1_bytes = sizeof(ushort4) * nn, r2_bytes = align_up(4 * nn, 256) + 4 * nn;  // (key[1] follows key[0])
        const bool adjacent = !p || reinterpret_cast<char *>(ws->key[1]) == r2 + align_up(4 * nn, 256);  // gsr_internal.h, the contract at key[]
        size_t o1 = 0, o2 = 0;
        auto over = [](char *r, size_t &o, size_t bytes) { char *q = r ? r + o : nullptr; o = (o + bytes + 255) / 256 * 256; return q; };
        ws->front_acc[0] = reinterpret_cast<float4 *>(over(r1, o1, half));
        ws->front_acc[1] = reinterpret_cast<float4 *>(over(r2, o2, half));
        ws->tile_open = reinterpret_cast<unsigned char *>(over(r1, o1, tiles));
        ws->cell_open = reinterpret_cast<unsigned char *>(over(r1, o1, cells));
        ws->open_sum = reinterpret_cast<uint32_t *>(over(r1, o1, 4 * (size_t)(ws->ctiles_x + 1) * (ws->ctiles_y + 1)));
        ws->blk_full = reinterpret_cast<uint32_t *>(over(r2, o2, 4 * ((nn + EMIT_THREADS - 1) / EMIT_THREADS + 4)));
        ws->front_fits = adjacent && ws->tiles_x <= 256 && ws->tiles_y <= 256 && o1 <= r1_bytes && o2 <= r2_bytes;
    }

    ws->pair_off = nullptr;
    ws->bytes = off;
    return off;
}

// The size limits of include/gsr.h, shared by gsr_workspace_bytes and every render entry point: a workspace can only be sized for
// a frame that can be rendered.
static int check_sizes(int64_t n, int32_t width, int32_t height, int64_t max_pairs)
{
    if (n < 0 || n > GSR_MAX_GAUSSIANS) { set_error("n = %lld out of range [0, %lld]", (long long)n, (long long)GSR_MAX_GAUSSIANS); return GSR_ERR_BAD_ARG; }
    // tile rects are ushort4 with an exclusive upper bound: at most 65535 tiles per side
    if (width <= 0 || height <= 0 || width > GSR_MAX_FRAME_SIDE || height > GSR_MAX_FRAME_SIDE) {
        set_error("bad frame size %dx%d (1 .. %d px per side)", width, height, GSR_MAX_FRAME_SIDE); return GSR_ERR_BAD_ARG;
    }
    // the sort kernels index pairs with 32-bit arithmetic, one 4096-pair tile past the last pair at most
    if (max_pairs < 0 || max_pairs > GSR_MAX_PAIRS) { set_error("max_pairs = %lld out of range [0, %lld]", (long long)max_pairs, (long long)GSR_MAX_PAIRS); return GSR_ERR_BAD_ARG; }
    return GSR_OK;
}

static int check_frame(int64_t n, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                       size_t workspace_bytes, Workspace *ws)
{
    if (!cam || !opts || !workspace) { set_error("null camera/options/workspace"); return GSR_ERR_BAD_ARG; }
    const int rc = check_sizes(n, cam->width, cam->height, max_pairs);
    if (rc) return rc;
    if (opts->tile_row_step < 0 || opts->tile_row_begin < 0 || opts->tile_row_begin >= std::max(opts->tile_row_step, 1)) {
        set_error("bad tile-row shard %d/%d", opts->tile_row_begin, opts->tile_row_step); return GSR_ERR_BAD_ARG;
    }
    if (opts->tile_row_block < 0 || opts->tile_row_block > 2) { set_error("bad tile_row_block %d (0 / 1: single rows, 2: pairs)", opts->tile_row_block); return GSR_ERR_BAD_ARG; }
    if (opts->draw_limit < 0) { set_error("bad draw_limit %d", opts->draw_limit); return GSR_ERR_BAD_ARG; }
    if (opts->output_dtype != 0 && opts->output_dtype != 1) { set_error("bad output_dtype %d", opts->output_dtype); return GSR_ERR_BAD_ARG; }
    if (opts->blend_impl < 0 || opts->blend_impl > 1) { set_error("bad blend_impl %d", opts->blend_impl); return GSR_ERR_BAD_ARG; }
    if (opts->output_layout < 0 || opts->output_layout > 2) { set_error("bad output_layout %d", opts->output_layout); return GSR_ERR_BAD_ARG; }
    if (opts->depth_sort_passes < 0 || opts->depth_sort_passes > 4) { set_error("bad depth_sort_passes %d", opts->depth_sort_passes); return GSR_ERR_BAD_ARG; }
    if (opts->accum_dtype != 0 && opts->accum_dtype != 1) { set_error("bad accum_dtype %d", opts->accum_dtype); return GSR_ERR_BAD_ARG; }
    if (opts->keep_flags != 0 && opts->keep_flags != 1) { set_error("bad keep_flags %d", opts->keep_flags); return GSR_ERR_BAD_ARG; }
    if (opts->saturation_rule != 0 && opts->saturation_rule != 1 && opts->saturation_rule != 3 && opts->saturation_rule != 4) { set_error("bad saturation_rule %d", opts->saturation_rule); return GSR_ERR_BAD_ARG; }
    if (opts->fine_binning != 0 && opts->fine_binning != 1) { set_error("bad fine_binning %d", opts->fine_binning); return GSR_ERR_BAD_ARG; }
    if (opts->shard_preprocess < 0 || opts->shard_preprocess > 2) { set_error("bad shard_preprocess %d", opts->shard_preprocess); return GSR_ERR_BAD_ARG; }
    if (opts->blend_pipe_tiles < -1) { set_error("bad blend_pipe_tiles %d", opts->blend_pipe_tiles); return GSR_ERR_BAD_ARG; }
    if (opts->no_order_hint != 0 && opts->no_order_hint != 1) { set_error("bad no_order_hint %d", opts->no_order_hint); return GSR_ERR_BAD_ARG; }
    if (opts->colour_stage != 0 && opts->colour_stage != 1) { set_error("bad colour_stage %d", opts->colour_stage); return GSR_ERR_BAD_ARG; }
    if (opts->sh_dense_min < 0 || opts->sh_dense_min > 65) { set_error("bad sh_dense_min %d", opts->sh_dense_min); return GSR_ERR_BAD_ARG; }
    if (opts->batch_views < 0 || opts->batch_views > MAX_VIEWS) { set_error("bad batch_views %d (0 .. %d)", opts->batch_views, MAX_VIEWS); return GSR_ERR_BAD_ARG; }
    if (reinterpret_cast<uintptr_t>(workspace) % 256 != 0) { set_error("workspace must be 256-byte aligned"); return GSR_ERR_BAD_ARG; }
    const size_t need = carve_workspace(workspace, n, cam->width, cam->height, max_pairs, ws);
    if (workspace_bytes < need) {
        set_error("workspace too small: %zu bytes given, %zu needed", workspace_bytes, need);
        return GSR_ERR_WORKSPACE;
    }
    return GSR_OK;
}

static int ceil_log2(int v)
{
    int bits = 0;
    while ((1 << bits) < v) ++bits;
    return bits;
}

// two quadrants per wave from this many tiles per launch on (measured: 4080 tiles better with two, 2040 with one); below, one quadrant per wave (see blend_walk_kernel)
#ifndef GSR_BLEND_HALF_MIN_TILES
#define GSR_BLEND_HALF_MIN_TILES 3000
#endif
constexpr int BLEND_HALF_MIN_TILES = GSR_BLEND_HALF_MIN_TILES;  // (the macro: tools/ A/B builds)
// the pipelined one-quadrant walk (96 VGPRs: 5 waves per SIMD = 1280 four-wave workgroups resident) up to this many tiles per launch;
// GsrOptions.blend_pipe_tiles overrides it (experiments and tests: -1 switches the variant off)
constexpr int BLEND_PIPE_MAX_TILES = 1280;
// The front slice (FramePlan.front_slice) by plan: from this many gaussians and this many views per launch sequence on.  Both from the
// sweep of profiles/front_slice_sweeps.txt (1080p, forced on against off, one stream): the second round of 13 dispatches is paid
// per launch sequence and the spared pair work per view and per gaussian the first slice hides — at 6 views 2^21 gaussians are 22 %
// slower sliced, 5.0 M 2.5 % slower, 6.13 M 0.8 % faster (+3.9 % in bench.py's three batches in flight); at 4 views and at 1 every size
// up to 6.13 M is slower.  So: only what was measured to win
constexpr int FRONT_SLICE_MIN_VIEWS = 6;
constexpr int64_t FRONT_SLICE_MIN_N = 6000000;

FramePlan plan_frame(const Workspace &ws, const GsrOptions &opts, bool colour_frame)
{
    FramePlan p;
    // ---- stage 1.  The tile rect packs into 32 bits when the tile grid fits 8 bits per coordinate (frames up to 4096 px): the
    // preprocess writes that form, the depth sort carries it as a second payload and binning reads it in depth order
    p.packed_rect = ws.tiles_x <= 256 && ws.tiles_y <= 256;
    p.rs = row_shard_of(opts);
    // A multi-GPU shard's preprocess (preprocess.hip) hands the depth sort a compact list of (key, id, rect) records of the rank's
    // visible gaussians instead of one key per gaussian.  Progressive frames (draw_limit) rank ALL gaussians the reference
    // draws, so they take the whole-frame path.
    if (opts.tile_row_step <= 1 || opts.draw_limit != 0) p.compact_input = false;
    else if (opts.shard_preprocess != 0) p.compact_input = opts.shard_preprocess == 2;  // A/B: 1 = whole-frame kernel, 2 = three-phase kernel
    else p.compact_input = opts.tile_row_step >= 5;  // measured: 2 and 4 shards are as fast or faster through the whole-frame kernel
    // progressive frames rank every gaussian the reference draws, whatever rows it touches: no row test then
    p.cull_rs = opts.draw_limit > 0 ? RowShard{0, 1, 0} : p.rs;
    // ---- depth sort: four passes cover any depth range; a shard's compact records are few (its visible gaussians): smaller
    // tiles, more workgroups, shorter serial chains
    p.depth_passes = opts.depth_sort_passes >= 1 && opts.depth_sort_passes <= 4 ? opts.depth_sort_passes : 4;
    p.depth_items = p.compact_input ? DEPTH_SORT_ITEMS_SHARD : DEPTH_SORT_ITEMS;
    // ---- binning.  Coarse (per 32x32 cell) when the packed rect exists and the gaussian ids leave four bits of the pair value for
    // the tile mask.  GsrOptions.fine_binning = 1 forces the fine path (A/B timing, and the test that both build the same frame).
    p.coarse = p.packed_rect && ws.n <= ((int64_t)1 << COARSE_ID_BITS) && opts.fine_binning == 0;
    p.grid_x = p.coarse ? ws.ctiles_x : ws.tiles_x;
    p.grid_y = p.coarse ? ws.ctiles_y : ws.tiles_y;
    p.bits_x = std::max(1, ceil_log2(p.grid_x));
    p.bits_y = std::max(1, ceil_log2(p.grid_y + 1));  // one spare row value marks culled pairs
    p.drop_from = (uint32_t)p.grid_y << p.bits_x;
    // cells of a shard: pairs of rows (tile_row_block = 2) ARE cell rows — the rank owns cell rows begin + k step whole; with single rows
    // and an even step the rank's tile rows begin + k step fall into the cell rows (begin >> 1) + k (step >> 1), each holding exactly one
    // of them; with an odd step (or none) every cell row can hold one.  The expansion keeps only this rank's tiles either way.
    p.csh = p.rs.step <= 1 ? RowShard{0, 1, 0}
          : p.rs.bshift == 1 ? RowShard{p.rs.begin, p.rs.step, 0}
          : p.rs.step % 2 == 0 ? RowShard{p.rs.begin >> 1, p.rs.step >> 1, 0} : RowShard{0, 1, 0};
    // ---- pair sort.  Keys are uint16_t in memory when every key (the culled row included) fits: 6 B per pair instead of 8
    // through emit, the sort passes and the range scan, all of them bound by HBM.  8 bits or fewer per pass, the bits split evenly
    // (13 tile-id bits sort as 7 + 6, not 8 + 5: with 128 digit values a workgroup's runs in the first, far-scattering pass are 32
    // entries = one full 128-B line per array instead of half a line).  Every pass moves the pairs to the other buffer, from 0.
    const int key_bits = p.bits_x + p.bits_y;
    p.key16 = key_bits <= 16;
    p.pair_passes = (key_bits + 7) / 8;
    p.pair_bits_pp = (key_bits + p.pair_passes - 1) / p.pair_passes;
    p.lists_buf = ws.n <= 0 || ws.max_pairs <= 0 ? 0 : p.pair_passes & 1;  // (nothing emitted or sorted: launch_binning)
    // ---- blend.  Coarse binning hands it the sorted CELL lists (values = gaussian id | tile mask << 28) and cranges[]; the blend of
    // a tile keeps the entries with its bit while it stages (blend.hip).  Round 2 expanded them into per-tile lists first
    // (pair_expand_kernel: 34 us, 122 MB of traffic, 16 B of workspace per pair slot); A/B in one process on the bench frame: bin +
    // sort 0.375 -> 0.341 ms, blend 0.553 -> 0.565 ms, frames and counters identical.
    p.cell_lists = p.coarse;
    p.rows = p.rs.rows_before(ws.tiles_y);
    // which walk: by the tiles of the whole launch (all views: what fills the machine)
    const int launch_tiles = p.rows * ws.tiles_x * ws.views;
    const int pipe_max_tiles = opts.blend_pipe_tiles == 0 ? BLEND_PIPE_MAX_TILES : opts.blend_pipe_tiles;
    p.blend = opts.accum_dtype == 1 ? BlendKernel::TileBf16
            : opts.blend_impl == 1 ? BlendKernel::Tile
            : launch_tiles >= BLEND_HALF_MIN_TILES ? BlendKernel::Walk2
            : launch_tiles <= pipe_max_tiles ? BlendKernel::Walk1Pipe : BlendKernel::Walk1;
    // ---- the front slice.  A whole colour frame under the exact colour-saturation rule, binned by cells and blended by the product
    // walk: the nearest eighth of the draw order finishes most tiles (bench frame: 61 % of the cells), and the rest of the order is
    // then binned and sorted only where a tile is still open.  It pays where binning the whole order costs more than a second round
    // of launches: frames of Walk2 size over scenes of FRONT_SLICE_MIN_N gaussians.  saturation_rule 3 forces it on whatever the two
    // sizes say, 4 switches it off (tests, A/B).  A sliced frame is blended by the two-quadrant walk, the one kernel that knows how.
    const bool sliceable = colour_frame && p.coarse && opts.tile_row_step <= 1 && opts.draw_limit == 0 && opts.early_out_T == 0.0f &&
                           opts.accum_dtype == 0 && opts.blend_impl == 0 && (opts.saturation_rule == 0 || opts.saturation_rule == 3);
    // (forced where its planes have no room — carve_workspace, front_fits — the frame is refused by render_views, not quietly built whole)
    // (the two measured thresholds: above, at their definitions)
    p.front_slice = sliceable && (opts.saturation_rule == 3 || (ws.front_fits && ws.views >= FRONT_SLICE_MIN_VIEWS &&
                                                                p.rows * ws.tiles_x >= BLEND_HALF_MIN_TILES && ws.n >= FRONT_SLICE_MIN_N));
    if (p.front_slice) p.blend = BlendKernel::Walk2;
    return p;
}

}  // namespace gsr

using namespace gsr;

extern "C" {

int gsr_version(void) { return GSR_VERSION; }

const char *gsr_last_error(void) { return g_err; }

void gsr_default_options(GsrOptions *o)
{
    if (!o) return;
    memset(o, 0, sizeof *o);
    o->reference_compat = 1;
    o->early_out_T = 0.0f;
    o->tile_row_begin = 0;
    o->tile_row_step = 1;
    o->output_layout = 0;
}

int gsr_camera_setup(const double qvec[4], const double tvec[3], double fx_full, double fy_full, int64_t cam_width,
                     int64_t cam_height, int32_t width, int32_t height, GsrCamera *cam)
{
    if (!qvec || !tvec || !cam) { set_error("null argument"); return GSR_ERR_BAD_ARG; }
    if (!(fx_full > 0.0) || !(fy_full > 0.0) || cam_width <= 0 || cam_height <= 0 || width <= 0 || height <= 0) {
        set_error("bad intrinsics"); return GSR_ERR_BAD_ARG;
    }
    const double Z_FAR = 100.0, Z_NEAR = 0.01;  // rasterize.py:29-30
    // world -> camera: the quaternion formula of rasterize.py:41-56 evaluated in float64 on the COLMAP qvec
    // (un-normalised, Q8), cast to fp32 (:56), +tvec in the last column (:75), then transposed (:361).
    const double w = qvec[0], x = qvec[1], y = qvec[2], z = qvec[3];
    const double R[3][3] = {
        {1 - 2 * (y * y) - 2 * (z * z), 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w},
        {2 * x * y + 2 * z * w, 1 - 2 * (x * x) - 2 * (z * z), 2 * y * z - 2 * x * w},
        {2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w, 1 - 2 * (x * x) - 2 * (y * y)}};
    float M[4][4] = {{0}};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) M[i][j] = (float)R[i][j];
        M[i][3] = (float)tvec[i];
    }
    M[3][3] = 1.0f;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) cam->w2c[4 * i + j] = M[j][i];
    // field of view from the full-resolution camera, rasterize.py:342-345
    const double fov_x = 2.0 * std::atan((double)cam_width / (2.0 * fx_full));
    const double fov_y = 2.0 * std::atan((double)cam_height / (2.0 * fy_full));
    cam->tan_fov_x = (float)std::tan(fov_x * 0.5);
    cam->tan_fov_y = (float)std::tan(fov_y * 0.5);
    cam->lim_x = (float)(1.3 * std::tan(fov_x * 0.5));  // :210
    cam->lim_y = (float)(1.3 * std::tan(fov_y * 0.5));  // :211
    cam->focal_x = (float)(fx_full / 2.0);              // :216 (Q3: always full-res / 2)
    cam->focal_y = (float)(fy_full / 2.0);
    // perspective matrix, rasterize.py:123-151 (float64 python arithmetic stored into an fp32 tensor)
    const double thx = std::tan(fov_x / 2), thy = std::tan(fov_y / 2);
    const double top = thy * Z_NEAR, bottom = -top, right = thx * Z_NEAR, left = -right;
    float P[4][4] = {{0}};
    P[0][0] = (float)(2.0 * Z_NEAR / (right - left));
    P[1][1] = (float)(2.0 * Z_NEAR / (top - bottom));
    P[0][2] = (float)((right + left) / (right - left));
    P[1][2] = (float)((top + bottom) / (top - bottom));
    P[3][2] = 1.0f;
    P[2][2] = (float)(Z_FAR / (Z_FAR - Z_NEAR));
    P[2][3] = (float)(-(Z_FAR * Z_NEAR) / (Z_FAR - Z_NEAR));
    for (int i = 0; i < 4; ++i)  // full = w2c @ P^T in fp32, :364
        for (int j = 0; j < 4; ++j) {
            float acc = 0.0f;
            for (int k = 0; k < 4; ++k) acc = acc + cam->w2c[4 * i + k] * P[j][k];
            cam->full_proj[4 * i + j] = acc;
        }
    // camera centre = inverse(w2c)[3,:3] (spherical_harmonics.py:35) = -t A^-1, A = w2c[:3,:3]; float64, one cast
    double A[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) A[i][j] = (double)cam->w2c[4 * i + j];
    const double c00 = A[1][1] * A[2][2] - A[1][2] * A[2][1], c01 = A[1][2] * A[2][0] - A[1][0] * A[2][2],
                 c02 = A[1][0] * A[2][1] - A[1][1] * A[2][0];
    const double det = A[0][0] * c00 + A[0][1] * c01 + A[0][2] * c02;
    if (det == 0.0 || !std::isfinite(det)) { set_error("singular world-to-camera rotation"); return GSR_ERR_BAD_ARG; }
    const double inv[3][3] = {
        {c00 / det, (A[0][2] * A[2][1] - A[0][1] * A[2][2]) / det, (A[0][1] * A[1][2] - A[0][2] * A[1][1]) / det},
        {c01 / det, (A[0][0] * A[2][2] - A[0][2] * A[2][0]) / det, (A[0][2] * A[1][0] - A[0][0] * A[1][2]) / det},
        {c02 / det, (A[0][1] * A[2][0] - A[0][0] * A[2][1]) / det, (A[0][0] * A[1][1] - A[0][1] * A[1][0]) / det}};
    for (int j = 0; j < 3; ++j) {
        double c = 0.0;
        for (int k = 0; k < 3; ++k) c -= (double)cam->w2c[12 + k] * inv[k][j];
        cam->cam_center[j] = (float)c;
    }
    cam->width = width;
    cam->height = height;
    return GSR_OK;
}

int gsr_workspace_bytes(int64_t n, int32_t width, int32_t height, int64_t max_pairs, size_t *bytes)
{
    if (!bytes) { set_error("null bytes"); return GSR_ERR_BAD_ARG; }
    const int rc = check_sizes(n, width, height, max_pairs);
    if (rc) return rc;
    Workspace ws;
    *bytes = carve_workspace(nullptr, n, width, height, max_pairs, &ws);
    return GSR_OK;
}

static int check_scene(const GsrScene *sc)
{
    if (!sc) { set_error("null scene"); return GSR_ERR_BAD_ARG; }
    if (sc->n > 0 && (!sc->means || !sc->log_scales || !sc->quats || !sc->opacity_logit || !sc->sh)) {
        set_error("null scene array"); return GSR_ERR_BAD_ARG;
    }
    if (sc->sh_degree < 0 || sc->sh_degree > 3) { set_error("sh_degree %d not in 0..3", sc->sh_degree); return GSR_ERR_BAD_ARG; }
    if (sc->sh_dtype != 0 && sc->sh_dtype != 1) { set_error("sh_dtype %d: 0 (float32) or 1 (float16)", sc->sh_dtype); return GSR_ERR_BAD_ARG; }
    if (reinterpret_cast<uintptr_t>(sc->sh) % 16 != 0 || reinterpret_cast<uintptr_t>(sc->quats) % 16 != 0 ||
        reinterpret_cast<uintptr_t>(sc->block_bounds) % 16 != 0) {
        set_error("sh, quats and block_bounds must be 16-byte aligned"); return GSR_ERR_BAD_ARG;
    }
    return GSR_OK;
}

// how much of a view's control block its frame clears: a fresh workspace may hold anything, so the default clears the whole block
// (a 0xFF-filled one renders correctly); keep_flags / the later views of a batch keep the sticky record at its tail
static int reset_words_of(const GsrOptions *opts, bool keep_batch_words)
{
    static_assert(sizeof(FrameCtrl) % 4 == 0 && offsetof(FrameCtrl, batch_overflow) % 4 == 0, "FrameCtrl is cleared by words");
    return (int)((keep_batch_words || opts->keep_flags ? offsetof(FrameCtrl, batch_overflow) : sizeof(FrameCtrl)) / 4);
}

int gsr_preprocess(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, void *workspace,
                   size_t workspace_bytes, const GsrDebugOut *debug, void *stream)
{
    int rc = check_scene(scene);
    if (rc) return rc;
    Workspace ws;
    // stage 1 does not touch the pair buffers: any max_pairs >= 0 gives the same per-gaussian layout,
    // so size-check against the smallest one.
    rc = check_frame(scene->n, cam, opts, 0, workspace, workspace_bytes, &ws);
    if (rc) return rc;
    return launch_preprocess(*scene, cam, *opts, ws, plan_frame(ws, *opts), debug, reset_words_of(opts, false), static_cast<hipStream_t>(stream));
}

// depth order: pass 0 drops culled gaussians and leaves V in ctrl; 3 passes on ordinary scenes (sort.hip); then pairs in depth
// order, stably sorted by tile -> per-tile lists and their ranges; E in ctrl
static int bin_sort_impl(const GsrOptions *opts, const Workspace &ws, const FramePlan &plan, hipStream_t s)
{
    const int rc = launch_depth_sort(ws, plan, s);
    if (rc) return rc;
    return launch_binning(*opts, ws, plan, s);
}

int gsr_bin_sort(int64_t n, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                 size_t workspace_bytes, void *stream)
{
    Workspace ws;
    int rc = check_frame(n, cam, opts, max_pairs, workspace, workspace_bytes, &ws);
    if (rc) return rc;
    return bin_sort_impl(opts, ws, plan_frame(ws, *opts), static_cast<hipStream_t>(stream));
}

// A scene named beside lists of n gaussians (gsr_blend, gsr_blend_slab): check_scene's refusals, and the lists must be its own
static int check_scene_of_lists(const GsrScene *scene, int64_t n)
{
    const int rc = check_scene(scene);
    if (rc) return rc;
    if (scene->n != n) { set_error("scene->n = %lld but n = %lld", (long long)scene->n, (long long)n); return GSR_ERR_BAD_ARG; }
    return GSR_OK;
}

int gsr_blend(const GsrScene *scene, int64_t n, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
              size_t workspace_bytes, void *out_image, float *out_final_T, void *stream)
{
    if (!out_image) { set_error("null output image"); return GSR_ERR_BAD_ARG; }
    int rc = scene ? check_scene_of_lists(scene, n) : GSR_OK;
    if (rc) return rc;
    Workspace ws;
    rc = check_frame(n, cam, opts, max_pairs, workspace, workspace_bytes, &ws);
    if (rc) return rc;
    return launch_blend(*cam, *opts, ws, plan_frame(ws, *opts), out_image, 0, out_final_T, scene, static_cast<hipStream_t>(stream));
}

// ---- what the entries that take several cameras say about them, once each ----------------------------------------------------
// Every camera has the first one's frame size, or `wording` is the refusal (the frame batches and the view entries word it
// differently).  refuse_empty: a camera without pixels is refused as the loop comes to it (the frame batches)
static int check_one_frame_size(const GsrCamera *cams, int32_t n_cams, const char *wording, bool refuse_empty = false)
{
    for (int32_t i = 0; i < n_cams; ++i) {
        if (refuse_empty && (cams[i].width <= 0 || cams[i].height <= 0)) { set_error("bad frame size %dx%d", cams[i].width, cams[i].height); return GSR_ERR_BAD_ARG; }
        if (cams[i].width != cams[0].width || cams[i].height != cams[0].height) { set_error("%s", wording); return GSR_ERR_BAD_ARG; }
    }
    return GSR_OK;
}

// Pixels of one view's plane: the frame, or (output_layout = 2) the strip of the shard's tile rows.  0 for sizes check_frame
// refuses; a shard check_frame refuses counts as the whole frame
static int64_t view_plane_pixels(const GsrCamera &cam, const GsrOptions &opts)
{
    if (cam.width <= 0 || cam.height <= 0) return 0;
    int64_t rows_px = cam.height;
    if (opts.output_layout == 2 && opts.tile_row_step >= 0 && opts.tile_row_begin >= 0) {
        const int tiles_y = (cam.height + GSR_TILE - 1) / GSR_TILE;
        rows_px = (int64_t)row_shard_of(opts).rows_before(tiles_y) * GSR_TILE;
    }
    return (int64_t)cam.width * rows_px;
}

// The frame's checks for n_views views in slices 0 .. n_views - 1 of the workspace; *ws describes them (check_frame's, with the views)
static int check_view_slices(int64_t n, const GsrCamera *cams, int32_t n_views, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                             size_t workspace_bytes, Workspace *ws)
{
    const int rc = check_frame(n, &cams[0], opts, max_pairs, workspace, workspace_bytes, ws);
    if (rc) return rc;
    if (workspace_bytes / ws->bytes < (size_t)n_views) {
        set_error("workspace too small for %d views per launch: %zu bytes given, %zu needed", (int)n_views, workspace_bytes, ws->bytes * (size_t)n_views);
        return GSR_ERR_WORKSPACE;
    }
    if (n_views > 1) {
        ws->views = n_views;
        ws->view_stride = ws->bytes;
    }
    return GSR_OK;
}

// How many views go through one launch sequence: as many slices as the workspace holds, at most MAX_VIEWS, GsrOptions.batch_views
// (when set) and the views there are.  0: the workspace does not hold one view.
static int views_per_launch(const GsrScene *scene, const GsrCamera *cam0, const GsrOptions *opts, int64_t max_pairs, size_t workspace_bytes, int32_t n_cams)
{
    Workspace ws;
    const size_t per = carve_workspace(nullptr, scene->n, cam0->width, cam0->height, max_pairs, &ws);
    size_t k = workspace_bytes / per;
    k = std::min<size_t>(k, (size_t)MAX_VIEWS);
    if (opts->batch_views > 0) k = std::min<size_t>(k, (size_t)opts->batch_views);
    return (int)std::min<size_t>(k, (size_t)std::max<int32_t>(n_cams, 1));
}

// The cameras of a batch, K per launch sequence: group(first camera, how many, the group's number) until one fails.  K = 0: the
// workspace does not hold one view — groups of one, and the first group's own checks report it.  Whose control blocks a group finds
// used is the caller's to say from the group's number: a slice's first view clears its whole block, the views that follow in later
// groups keep the batch-sticky overflow words (reset_words_of)
extern "C++" {
template <class Group>
static int for_view_groups(int32_t n_cams, int K, Group group)
{
    int32_t g = 0;
    for (int32_t i = 0; i < n_cams; i += std::max(K, 1), ++g) {
        const int rc = group(i, std::max(1, std::min<int32_t>(K, n_cams - i)), g);
        if (rc) return rc;
    }
    return GSR_OK;
}
}  // extern "C++"

// Stages 1-3 for `views` cameras through ONE launch sequence: view v works in slice v of the workspace (slices of
// gsr_workspace_bytes() bytes) and renders into out_images + v * out_view_stride bytes.
static int render_views(const GsrScene *scene, const GsrCamera *cams, int views, const GsrOptions *opts, int64_t max_pairs,
                        void *workspace, size_t workspace_bytes, void *out_images, size_t out_view_stride, float *out_final_T,
                        void *stream, bool keep_batch_words)
{
    int rc = check_scene(scene);
    if (rc) return rc;
    if (!out_images) { set_error("null output image"); return GSR_ERR_BAD_ARG; }
    if (!cams || views < 1 || views > MAX_VIEWS || (views > 1 && out_final_T)) { set_error("bad view count %d", views); return GSR_ERR_BAD_ARG; }
    Workspace ws;
    rc = check_view_slices(scene->n, cams, views, opts, max_pairs, workspace, workspace_bytes, &ws);
    if (rc) return rc;
    const FramePlan plan = plan_frame(ws, *opts, out_final_T == nullptr);
    if (plan.front_slice && !ws.front_fits) {
        set_error("saturation_rule 3: no room for the front slice's planes (%lld gaussians, %d tiles: 257 gaussians per tile hold them)",
                  (long long)ws.n, ws.tiles_x * ws.tiles_y);
        return GSR_ERR_BAD_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    rc = launch_preprocess(*scene, cams, *opts, ws, plan, nullptr, reset_words_of(opts, keep_batch_words), s);
    if (rc) return rc;
    // (the blend finds the scene through what the preprocess above left in each view's control block: same call, same arrays)
    if (!plan.front_slice) {
        rc = bin_sort_impl(opts, ws, plan, s);
        if (rc) return rc;
        return launch_blend(cams[0], *opts, ws, plan, out_images, out_view_stride, out_final_T, nullptr, s);
    }
    // the front slice (binning.hip): one depth sort; bin and blend the nearest ranks; bin the rest where a tile is still open, blend on
    rc = launch_depth_sort(ws, plan, s);
    for (int slice = 1; slice <= 2 && !rc; ++slice) {
        if (slice == 2) rc = launch_open_cells(ws, s);
        if (!rc) rc = launch_binning(*opts, ws, plan, s, slice);
        if (!rc) rc = launch_blend(cams[0], *opts, ws, plan, out_images, out_view_stride, nullptr, nullptr, s, slice);
    }
    return rc;
}

int gsr_render_forward(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs,
                       void *workspace, size_t workspace_bytes, void *out_image, float *out_final_T, void *stream)
{
    if (!cam || !opts) { set_error("null camera/options"); return GSR_ERR_BAD_ARG; }
    return render_views(scene, cam, 1, opts, max_pairs, workspace, workspace_bytes, out_image, 0, out_final_T, stream, false);
}

static int check_batch(const GsrScene *scene, const GsrCamera *cams, int32_t n_cams, const GsrOptions *opts, int64_t max_pairs, const void *out_images,
                       int64_t frame_stride)
{
    if (!scene || !cams || n_cams < 0 || !out_images || !opts) { set_error("bad argument"); return GSR_ERR_BAD_ARG; }
    if (scene->n < 0 || scene->n > 0x7FFFFFFF || max_pairs < 0) { set_error("bad argument"); return GSR_ERR_BAD_ARG; }
    const int rc = check_one_frame_size(cams, n_cams, "views of a batch must share one frame size", true);
    if (rc) return rc;
    // what one view writes: the frame, or (output_layout = 2) the strip of its shard's tile rows
    if (n_cams > 0 && frame_stride < view_plane_pixels(cams[0], *opts) * 3) { set_error("frame_stride smaller than a frame"); return GSR_ERR_BAD_ARG; }
    return GSR_OK;
}

// The frames of a checked batch, group g in slot g % n_slots (its workspace, its stream): the slot's first group finds its slices
// unused, whatever g its later ones have
static int render_groups(const GsrScene *scene, const GsrCamera *cams, int32_t n_cams, const GsrOptions *opts, int64_t max_pairs,
                         void *const *workspaces, size_t workspace_bytes, void *const *streams, int32_t n_slots, void *out_images, int64_t frame_stride)
{
    const size_t fbytes = (size_t)frame_stride * (opts->output_dtype == 1 ? 2 : 4);
    return for_view_groups(n_cams, views_per_launch(scene, &cams[0], opts, max_pairs, workspace_bytes, n_cams), [&](int32_t first, int count, int32_t g) {
        return render_views(scene, &cams[first], count, opts, max_pairs, workspaces[g % n_slots], workspace_bytes,
                            static_cast<char *>(out_images) + (size_t)first * fbytes, fbytes, nullptr, streams[g % n_slots], g >= n_slots);
    });
}

int gsr_render_batch(const GsrScene *scene, const GsrCamera *cams, int32_t n_cams, const GsrOptions *opts, int64_t max_pairs,
                     void *workspace, size_t workspace_bytes, void *out_images, int64_t frame_stride, void *stream)
{
    const int rc = check_batch(scene, cams, n_cams, opts, max_pairs, out_images, frame_stride);
    if (rc || n_cams == 0) return rc;
    return render_groups(scene, cams, n_cams, opts, max_pairs, &workspace, workspace_bytes, &stream, 1, out_images, frame_stride);
}

int gsr_render_batch_slots(const GsrScene *scene, const GsrCamera *cams, int32_t n_cams, const GsrOptions *opts, int64_t max_pairs,
                           void *const *workspaces, size_t workspace_bytes, void *const *streams, int32_t n_slots, void *out_images,
                           int64_t frame_stride)
{
    if (!workspaces || !streams || n_slots < 1) { set_error("bad argument"); return GSR_ERR_BAD_ARG; }
    const int rc = check_batch(scene, cams, n_cams, opts, max_pairs, out_images, frame_stride);
    if (rc) return rc;
    for (int32_t k = 0; k < n_slots; ++k) {
        if (!workspaces[k]) { set_error("null workspace in slot %d", (int)k); return GSR_ERR_BAD_ARG; }
        for (int32_t j = 0; j < k; ++j)
            if (workspaces[j] == workspaces[k]) { set_error("slots %d and %d share a workspace", (int)j, (int)k); return GSR_ERR_BAD_ARG; }
    }
    if (n_cams == 0) return GSR_OK;
    return render_groups(scene, cams, n_cams, opts, max_pairs, workspaces, workspace_bytes, streams, n_slots, out_images, frame_stride);
}

// ---- list consumers: blends that walk the colour frame's tile lists and do something of their own with the weights ------------
// One struct per kind holds the call's own arguments in the order its entries take them (a view stride is 0 where one view is all
// there is) and says
//   check(cam, opts)                    what the kind refuses before anything else, and before any HIP call, in this order;
//   launch(lists)                       its blend over them;
//   check_view_strides(plane, n_views)  where the kind takes several views per launch sequence: its strides against a view's plane.
// The entries below are one call each of the runners behind the structs.  DESIGN.md section 5.26 says what a new kind writes.
extern "C++" {  // (templates cannot have C linkage)
struct Lists {  // what a consumer walks: the (first) view, the options the lists were made with, where they lie, the frame's plan, the stream
    const GsrCamera &cam; const GsrOptions &opts; const Workspace &ws; const FramePlan &plan; hipStream_t s;
};

static int check_camera_options(const GsrCamera *cam, const GsrOptions *opts)
{
    if (!cam) { set_error("null camera"); return GSR_ERR_BAD_ARG; }
    if (!opts) { set_error("null options"); return GSR_ERR_BAD_ARG; }
    return GSR_OK;
}

// `channels` values per row, rows `stride` floats apart (`name`: what the entry calls the stride)
static int check_channel_rows(int32_t channels, const char *name, int64_t stride)
{
    if (channels < 1 || channels > GSR_MAX_FEATURE_CHANNELS) {
        set_error("bad channels %d (1 .. %d)", channels, GSR_MAX_FEATURE_CHANNELS); return GSR_ERR_BAD_ARG;
    }
    if (stride < channels) { set_error("bad %s %lld: rows of %d channels overlap", name, (long long)stride, channels); return GSR_ERR_BAD_ARG; }
    return GSR_OK;
}

// No consumer stores or accumulates bfloat16: "<outputs_are>: output_dtype = 1 ..." and "<sums_are> accumulated in float32: ..."
static int refuse_bf16(const GsrOptions *opts, const char *outputs_are, const char *sums_are)
{
    if (opts->output_dtype == 1) { set_error("%s: output_dtype = 1 (bfloat16) is not supported", outputs_are); return GSR_ERR_BAD_ARG; }
    if (opts->accum_dtype == 1) { set_error("%s accumulated in float32: accum_dtype = 1 (bfloat16) is not supported", sums_are); return GSR_ERR_BAD_ARG; }
    return GSR_OK;
}

static int check_view_stride(const char *name, int64_t stride, int64_t need, int32_t n_views, const char *what)
{
    if (n_views > 1 && stride < need) { set_error("bad %s %lld: smaller than %s (%lld)", name, (long long)stride, what, (long long)need); return GSR_ERR_BAD_ARG; }
    return GSR_OK;
}

struct Features {  // three channels
    const float *features; float *out_map, *out_final_T;
    int check(const GsrCamera *cam, const GsrOptions *opts) const
    {
        if (!cam || !opts) { set_error("null camera/options"); return GSR_ERR_BAD_ARG; }
        if (!features) { set_error("null features"); return GSR_ERR_BAD_ARG; }
        if (!out_map) { set_error("null output map"); return GSR_ERR_BAD_ARG; }
        return refuse_bf16(opts, "feature maps are float32", "feature maps are");
    }
    int launch(const Lists &l) const { return launch_blend_features(l.cam, l.opts, l.ws, l.plan, features, out_map, out_final_T, l.s); }
};

struct Channels {  // any number of channels; view v writes out_map + v * map_stride and out_final_T + v * T_stride
    const float *features; int32_t channels; int64_t feature_stride;
    float *out_map, *out_final_T; int64_t map_stride, T_stride;
    int check(const GsrCamera *cam, const GsrOptions *opts) const
    {
        int rc = check_camera_options(cam, opts);
        if (rc) return rc;
        if (!features) { set_error("null features"); return GSR_ERR_BAD_ARG; }
        if (!out_map) { set_error("null output map"); return GSR_ERR_BAD_ARG; }
        rc = check_channel_rows(channels, "feature_stride", feature_stride);
        return rc ? rc : refuse_bf16(opts, "feature maps are float32", "feature maps are");
    }
    int check_view_strides(int64_t plane, int32_t n_views) const
    {
        const int rc = check_view_stride("map_stride", map_stride, plane * channels, n_views, "a view's map");
        if (rc) return rc;
        return out_final_T ? check_view_stride("T_stride", T_stride, plane, n_views, "a view's final-T plane") : GSR_OK;
    }
    Channels from_view(int32_t v) const  // the same call for the views from v on
    {
        Channels c = *this;
        c.out_map += (size_t)v * (size_t)map_stride;
        if (out_final_T) c.out_final_T += (size_t)v * (size_t)T_stride;
        return c;
    }
    int launch(const Lists &l) const
    {
        return launch_blend_channels(l.cam, l.opts, l.ws, l.plan, features, channels, feature_stride, out_map, out_final_T, l.s, map_stride, T_stride);
    }
};

struct Slab {  // Channels between two depth planes, either of which may be null; scene: whose means give the depths (null: the preprocess's)
    Channels maps; const GsrScene *scene; const float *depth_near, *depth_far;
    int check(const GsrCamera *cam, const GsrOptions *opts) const { return maps.check(cam, opts); }
    int launch(const Lists &l) const
    {
        return launch_blend_slab(l.cam, l.opts, l.ws, l.plan, scene ? scene->means : nullptr, maps.features, maps.channels, maps.feature_stride,
                                 depth_near, depth_far, maps.out_map, maps.out_final_T, l.s);
    }
};

struct ChannelsBackward {  // view v reads grad_map + v * map_stride; all add into the one grad_features
    const float *grad_map; int32_t channels; float *grad_features; int64_t grad_stride, map_stride;
    int check(const GsrCamera *cam, const GsrOptions *opts) const
    {
        int rc = check_camera_options(cam, opts);
        if (rc) return rc;
        if (!grad_map) { set_error("null gradient map"); return GSR_ERR_BAD_ARG; }
        if (!grad_features) { set_error("null feature gradient"); return GSR_ERR_BAD_ARG; }
        rc = check_channel_rows(channels, "grad_stride", grad_stride);
        return rc ? rc : refuse_bf16(opts, "gradient maps are float32", "feature gradients are");
    }
    int check_view_strides(int64_t plane, int32_t n_views) const
    {
        return check_view_stride("map_stride", map_stride, plane * channels, n_views, "a view's gradient map");
    }
    int launch(const Lists &l) const { return launch_blend_channels_backward(l.cam, l.opts, l.ws, l.plan, grad_map, channels, grad_features, grad_stride, l.s, map_stride); }
};

struct SplatBackward {
    const float *features; int64_t feature_stride; int32_t channels;
    const float *grad_map, *grad_T; float min_T; int32_t want_abs; float *grad_splat;
    int check(const GsrCamera *cam, const GsrOptions *opts) const
    {
        int rc = check_camera_options(cam, opts);
        if (rc) return rc;
        if (!features) { set_error("null features"); return GSR_ERR_BAD_ARG; }
        if (!grad_map) { set_error("null gradient map"); return GSR_ERR_BAD_ARG; }
        if (!grad_splat) { set_error("null splat gradient"); return GSR_ERR_BAD_ARG; }
        rc = check_channel_rows(channels, "feature_stride", feature_stride);
        if (rc) return rc;
        if (!(min_T >= 0.0f) || min_T > 3.4028234e38f) { set_error("bad min_T %g: a finite value >= 0", (double)min_T); return GSR_ERR_BAD_ARG; }
        if (want_abs && channels > 16) {
            set_error("want_abs with %d channels: the absolute sums are not linear in the channels, one walk of at most 16", channels);
            return GSR_ERR_BAD_ARG;
        }
        return refuse_bf16(opts, "gradient maps are float32", "splat gradients are");
    }
    int launch(const Lists &l) const
    {
        return launch_blend_splat_backward(l.cam, l.opts, l.ws, l.plan, features, feature_stride, channels, grad_map, grad_T, min_T, want_abs != 0, grad_splat, l.s);
    }
};

struct GaussianStats {  // view v reads pixel_mask + v * mask_stride; view_hits / view_bits: the form for several views alone (several)
    const uint8_t *pixel_mask; float *weight_sum, *weight_max; uint32_t *pixels;
    int64_t mask_stride; uint32_t *view_hits, *view_bits; bool several;
    int check(const GsrCamera *cam, const GsrOptions *opts) const
    {
        const int rc = check_camera_options(cam, opts);
        if (rc) return rc;
        if (!weight_sum && !weight_max && !pixels && !view_hits) {
            set_error("null statistics outputs: all %s", several ? "four" : "three"); return GSR_ERR_BAD_ARG;
        }
        if (view_hits && !view_bits) { set_error("view_hits needs the view_bits scratch"); return GSR_ERR_BAD_ARG; }
        if (!view_hits && view_bits) { set_error("a view_bits scratch without view_hits"); return GSR_ERR_BAD_ARG; }
        return refuse_bf16(opts, "gaussian statistics are float32 / uint32", "the weights are");
    }
    int check_view_strides(int64_t plane, int32_t n_views) const
    {
        return pixel_mask ? check_view_stride("mask_stride", mask_stride, plane, n_views, "a view's mask plane") : GSR_OK;
    }
    int launch(const Lists &l) const
    {
        // the scratch is this launch sequence's: bit v = view v has counted the gaussian
        if (view_hits && l.ws.n > 0) GSR_HIP(hipMemsetAsync(view_bits, 0, sizeof(uint32_t) * (size_t)l.ws.n, l.s));
        return launch_blend_gstats(l.cam, l.opts, l.ws, l.plan, pixel_mask, weight_sum, weight_max, pixels, l.s, mask_stride, view_hits, view_bits);
    }
};

struct Pick {
    float median_T; int32_t *out_best_id; float *out_best_w; int32_t *out_median_id, *out_count;
    int check(const GsrCamera *cam, const GsrOptions *opts) const
    {
        const int rc = check_camera_options(cam, opts);
        if (rc) return rc;
        if (!out_best_id && !out_best_w && !out_median_id && !out_count) { set_error("null pick outputs: all four"); return GSR_ERR_BAD_ARG; }
        if (!(median_T > 0.0f && median_T <= 1.0f)) {  // (a NaN fails both compares)
            set_error("bad median_T %g (0 < median_T <= 1)", (double)median_T); return GSR_ERR_BAD_ARG;
        }
        return refuse_bf16(opts, "pick maps are int32 / float32", "pick weights are");
    }
    int launch(const Lists &l) const { return launch_blend_pick(l.cam, l.opts, l.ws, l.plan, median_T, out_best_id, out_best_w, out_median_id, out_count, l.s); }
};

struct TopK {
    int32_t k, select, *out_ids; float *out_weights, *out_final_T;
    int check(const GsrCamera *cam, const GsrOptions *opts) const
    {
        const int rc = check_camera_options(cam, opts);
        if (rc) return rc;
        if (!out_ids && !out_weights) { set_error("null top-k outputs: both ids and weights"); return GSR_ERR_BAD_ARG; }
        if (k < 1 || k > GSR_MAX_TOPK) { set_error("bad k %d (1 .. %d)", k, GSR_MAX_TOPK); return GSR_ERR_BAD_ARG; }
        if (select != GSR_TOPK_HEAVIEST && select != GSR_TOPK_NEAREST) {
            set_error("bad select %d (GSR_TOPK_HEAVIEST = 0, GSR_TOPK_NEAREST = 1)", select); return GSR_ERR_BAD_ARG;
        }
        return refuse_bf16(opts, "top-k lists are int32 / float32", "top-k weights are");
    }
    int launch(const Lists &l) const { return launch_blend_topk(l.cam, l.opts, l.ws, l.plan, k, select, out_ids, out_weights, out_final_T, l.s); }
};

// What every gsr_blend_X / gsr_render_X pair does behind the consumer's own checks: check_scene (when a scene is given), the frame's
// checks, the plan, and the consumer's launch on the lists — those already in the workspace (scene == nullptr: n gaussians), or
// the ones made here from the scene: stages 1 and 2 with colour_stage = 0 (nobody here needs a colour: the preprocess reads no SH
// row, the records keep their "unevaluated" marks).
template <class Consumer>
static int on_lists(const GsrScene *scene, int64_t n, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                    size_t workspace_bytes, void *stream, const Consumer &c)
{
    int rc = scene ? check_scene(scene) : GSR_OK;
    if (rc) return rc;
    Workspace ws;
    rc = check_frame(scene ? scene->n : n, cam, opts, max_pairs, workspace, workspace_bytes, &ws);
    if (rc) return rc;
    GsrOptions o = *opts;
    if (scene) o.colour_stage = 0;
    const FramePlan plan = plan_frame(ws, o);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (scene) {
        rc = launch_preprocess(*scene, cam, o, ws, plan, nullptr, reset_words_of(&o, false), s);
        if (rc) return rc;
        rc = bin_sort_impl(&o, ws, plan, s);
        if (rc) return rc;
    }
    return c.launch(Lists{*cam, o, ws, plan, s});
}

// gsr_blend_X: the consumer's checks, then its blend over the lists of n gaussians in the workspace
template <class Consumer>
static int run_on_lists(int64_t n, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace, size_t workspace_bytes,
                        void *stream, const Consumer &c)
{
    const int rc = c.check(cam, opts);
    return rc ? rc : on_lists(nullptr, n, cam, opts, max_pairs, workspace, workspace_bytes, stream, c);
}

// gsr_render_X: the consumer's checks, then stages 1-2 and its blend; the scene is not optional ("null scene" is check_scene's to say)
template <class Consumer>
static int render_on_lists(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                           size_t workspace_bytes, void *stream, const Consumer &c)
{
    const int rc = c.check(cam, opts);
    if (rc) return rc;
    if (!scene) return check_scene(scene);
    return on_lists(scene, 0, cam, opts, max_pairs, workspace, workspace_bytes, stream, c);
}
}  // extern "C++"

int gsr_blend_features(int64_t n, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace, size_t workspace_bytes,
                       const float *features, float *out_map, float *out_final_T, void *stream)
{
    return run_on_lists(n, cam, opts, max_pairs, workspace, workspace_bytes, stream, Features{features, out_map, out_final_T});
}

int gsr_render_features(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                        size_t workspace_bytes, const float *features, float *out_map, float *out_final_T, void *stream)
{
    return render_on_lists(scene, cam, opts, max_pairs, workspace, workspace_bytes, stream, Features{features, out_map, out_final_T});
}

int gsr_blend_channels(int64_t n, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace, size_t workspace_bytes,
                       const float *features, int32_t channels, int64_t feature_stride, float *out_map, float *out_final_T, void *stream)
{
    return run_on_lists(n, cam, opts, max_pairs, workspace, workspace_bytes, stream,
                        Channels{features, channels, feature_stride, out_map, out_final_T, 0, 0});
}

int gsr_render_channels(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                        size_t workspace_bytes, const float *features, int32_t channels, int64_t feature_stride, float *out_map,
                        float *out_final_T, void *stream)
{
    return render_on_lists(scene, cam, opts, max_pairs, workspace, workspace_bytes, stream,
                           Channels{features, channels, feature_stride, out_map, out_final_T, 0, 0});
}

// gsr_blend_slab may name the scene whose means it reads, which must then be the lists' own; it preprocesses nothing
int gsr_blend_slab(const GsrScene *scene, int64_t n, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                   size_t workspace_bytes, const float *features, int32_t channels, int64_t feature_stride, const float *depth_near,
                   const float *depth_far, float *out_map, float *out_final_T, void *stream)
{
    const Slab c{{features, channels, feature_stride, out_map, out_final_T, 0, 0}, scene, depth_near, depth_far};
    int rc = c.check(cam, opts);
    if (!rc && scene) rc = check_scene_of_lists(scene, n);
    return rc ? rc : on_lists(nullptr, n, cam, opts, max_pairs, workspace, workspace_bytes, stream, c);
}

int gsr_render_slab(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                    size_t workspace_bytes, const float *features, int32_t channels, int64_t feature_stride, const float *depth_near,
                    const float *depth_far, float *out_map, float *out_final_T, void *stream)
{
    return render_on_lists(scene, cam, opts, max_pairs, workspace, workspace_bytes, stream,
                           Slab{{features, channels, feature_stride, out_map, out_final_T, 0, 0}, scene, depth_near, depth_far});
}

int gsr_blend_channels_backward(int64_t n, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                                size_t workspace_bytes, const float *grad_map, int32_t channels, float *grad_features, int64_t grad_stride,
                                void *stream)
{
    return run_on_lists(n, cam, opts, max_pairs, workspace, workspace_bytes, stream,
                        ChannelsBackward{grad_map, channels, grad_features, grad_stride, 0});
}

int gsr_render_channels_backward(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                                 size_t workspace_bytes, const float *grad_map, int32_t channels, float *grad_features,
                                 int64_t grad_stride, void *stream)
{
    return render_on_lists(scene, cam, opts, max_pairs, workspace, workspace_bytes, stream,
                           ChannelsBackward{grad_map, channels, grad_features, grad_stride, 0});
}

int gsr_blend_splat_backward(int64_t n, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                             size_t workspace_bytes, const float *features, int64_t feature_stride, int32_t channels,
                             const float *grad_map, const float *grad_T, float min_T, int32_t want_abs, float *grad_splat, void *stream)
{
    return run_on_lists(n, cam, opts, max_pairs, workspace, workspace_bytes, stream,
                        SplatBackward{features, feature_stride, channels, grad_map, grad_T, min_T, want_abs, grad_splat});
}

int gsr_render_splat_backward(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                              size_t workspace_bytes, const float *features, int64_t feature_stride, int32_t channels,
                              const float *grad_map, const float *grad_T, float min_T, int32_t want_abs, float *grad_splat, void *stream)
{
    return render_on_lists(scene, cam, opts, max_pairs, workspace, workspace_bytes, stream,
                           SplatBackward{features, feature_stride, channels, grad_map, grad_T, min_T, want_abs, grad_splat});
}

// The splat gradient of a view chained to the scene's parameters: no workspace, no lists — the scene, the camera and reference_compat
int gsr_project_backward(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, const float *grad_splat, float *grad_means,
                         float *grad_log_scales, float *grad_quats, float *grad_opacity_logit, void *stream)
{
    if (!scene) { set_error("null scene"); return GSR_ERR_BAD_ARG; }
    int rc = check_camera_options(cam, opts);
    if (rc) return rc;
    if (!grad_splat) { set_error("null splat gradient"); return GSR_ERR_BAD_ARG; }
    if (!grad_means && !grad_log_scales && !grad_quats && !grad_opacity_logit) { set_error("null geometry gradients: all four"); return GSR_ERR_BAD_ARG; }
    const size_t rows = scene->n > 0 ? (size_t)scene->n : 0;
    const uintptr_t gs = reinterpret_cast<uintptr_t>(grad_splat);
    const struct { const float *p; size_t floats; const char *name; } outs[4] = {
        {grad_means, 3, "grad_means"}, {grad_log_scales, 3, "grad_log_scales"}, {grad_quats, 4, "grad_quats"}, {grad_opacity_logit, 1, "grad_opacity_logit"}};
    for (const auto &o : outs) {
        const uintptr_t b = reinterpret_cast<uintptr_t>(o.p);
        if (b && (b == gs || (b < gs + 32 * rows && gs < b + 4 * o.floats * rows))) {
            set_error("%s aliases grad_splat", o.name); return GSR_ERR_BAD_ARG;
        }
    }
    if (reinterpret_cast<uintptr_t>(grad_splat) % 16 != 0) { set_error("grad_splat must be 16-byte aligned"); return GSR_ERR_BAD_ARG; }
    if (reinterpret_cast<uintptr_t>(grad_quats) % 16 != 0) { set_error("grad_quats must be 16-byte aligned"); return GSR_ERR_BAD_ARG; }
    rc = check_scene(scene);
    if (rc) return rc;
    rc = refuse_bf16(opts, "geometry gradients are float32", "geometry gradients are");
    if (rc) return rc;
    return launch_project_backward(*scene, *cam, *opts, grad_splat, grad_means, grad_log_scales, grad_quats, grad_opacity_logit,
                                   static_cast<hipStream_t>(stream));
}

size_t gsr_camera_backward_bytes(int64_t n) { return camera_backward_bytes(n); }

// The splat gradient of a view (and the view-direction term gsr_sh_backward left) chained to the camera: 32 doubles, no lists
int gsr_camera_backward(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, const float *grad_splat,
                        const float *grad_view_means, double *grad_camera, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!scene) { set_error("null scene"); return GSR_ERR_BAD_ARG; }
    int rc = check_camera_options(cam, opts);
    if (rc) return rc;
    if (!grad_camera) { set_error("null camera gradient"); return GSR_ERR_BAD_ARG; }
    if (!workspace) { set_error("null workspace"); return GSR_ERR_BAD_ARG; }
    if (!grad_splat && !grad_view_means) { set_error("null inputs: both grad_splat and grad_view_means"); return GSR_ERR_BAD_ARG; }
    const size_t need = camera_backward_bytes(scene->n);
    if (workspace_bytes < need) { set_error("camera workspace too small: %zu bytes given, %zu needed", workspace_bytes, need); return GSR_ERR_BAD_ARG; }
    if (reinterpret_cast<uintptr_t>(grad_splat) % 16 != 0) { set_error("grad_splat must be 16-byte aligned"); return GSR_ERR_BAD_ARG; }
    if (reinterpret_cast<uintptr_t>(grad_camera) % 8 != 0) { set_error("grad_camera must be 8-byte aligned"); return GSR_ERR_BAD_ARG; }
    if (reinterpret_cast<uintptr_t>(workspace) % 8 != 0) { set_error("the camera workspace must be 8-byte aligned"); return GSR_ERR_BAD_ARG; }
    const size_t rows = scene->n > 0 ? (size_t)scene->n : 0;
    const struct { const void *p; size_t bytes; const char *name; } ins[2] = {{grad_splat, 32 * rows, "grad_splat"},
                                                                               {grad_view_means, 12 * rows, "grad_view_means"}},
                                                                     outs[2] = {{grad_camera, 32 * sizeof(double), "grad_camera"},
                                                                                {workspace, need, "the workspace"}};
    for (const auto &o : outs) {
        const uintptr_t b = reinterpret_cast<uintptr_t>(o.p);
        for (const auto &in : ins) {
            const uintptr_t a = reinterpret_cast<uintptr_t>(in.p);
            if (a && (a == b || (b < a + in.bytes && a < b + o.bytes))) { set_error("%s overlaps %s", o.name, in.name); return GSR_ERR_BAD_ARG; }
        }
    }
    {
        const uintptr_t g = reinterpret_cast<uintptr_t>(grad_camera), w = reinterpret_cast<uintptr_t>(workspace);
        if (g < w + need && w < g + 32 * sizeof(double)) { set_error("grad_camera overlaps the workspace"); return GSR_ERR_BAD_ARG; }
    }
    rc = check_scene(scene);
    if (rc) return rc;
    if (opts->output_dtype == 1) { set_error("camera gradients are float64: output_dtype = 1 (bfloat16) is not supported"); return GSR_ERR_BAD_ARG; }
    if (opts->accum_dtype == 1) { set_error("camera gradients are summed in float64: accum_dtype = 1 (bfloat16) is not supported"); return GSR_ERR_BAD_ARG; }
    return launch_camera_backward(*scene, *cam, *opts, grad_splat, grad_view_means, grad_camera, workspace, static_cast<hipStream_t>(stream));
}

// The colour gradient of a view chained to the scene's SH coefficients and means: no workspace, no lists, no options
int gsr_sh_backward(const GsrScene *scene, const GsrCamera *cam, const float *grad_rgb, int64_t grad_rgb_stride, float *grad_sh,
                    float *grad_means, void *stream)
{
    if (!scene) { set_error("null scene"); return GSR_ERR_BAD_ARG; }
    if (!cam) { set_error("null camera"); return GSR_ERR_BAD_ARG; }
    if (!grad_rgb) { set_error("null colour gradient"); return GSR_ERR_BAD_ARG; }
    if (!grad_sh && !grad_means) { set_error("null outputs: both grad_sh and grad_means"); return GSR_ERR_BAD_ARG; }
    if (grad_rgb_stride < 3) { set_error("bad grad_rgb_stride %lld: rows of 3 channels overlap", (long long)grad_rgb_stride); return GSR_ERR_BAD_ARG; }
    const size_t rows = scene->n > 0 ? (size_t)scene->n : 0;
    const uintptr_t gr = reinterpret_cast<uintptr_t>(grad_rgb);
    const size_t gr_bytes = rows ? 4 * ((rows - 1) * (size_t)grad_rgb_stride + 3) : 0;
    const struct { const float *p; size_t floats; const char *name; } outs[2] = {{grad_sh, 48, "grad_sh"}, {grad_means, 3, "grad_means"}};
    for (const auto &o : outs) {
        const uintptr_t b = reinterpret_cast<uintptr_t>(o.p);
        if (b && (b == gr || (b < gr + gr_bytes && gr < b + 4 * o.floats * rows))) {
            set_error("%s aliases grad_rgb", o.name); return GSR_ERR_BAD_ARG;
        }
    }
    if (reinterpret_cast<uintptr_t>(grad_sh) % 16 != 0) { set_error("grad_sh must be 16-byte aligned"); return GSR_ERR_BAD_ARG; }
    const int rc = check_scene(scene);
    if (rc) return rc;
    return launch_sh_backward(*scene, *cam, grad_rgb, grad_rgb_stride, grad_sh, grad_means, static_cast<hipStream_t>(stream));
}

int gsr_blend_gaussian_stats(int64_t n, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                             size_t workspace_bytes, const uint8_t *pixel_mask, float *weight_sum, float *weight_max, uint32_t *pixels,
                             void *stream)
{
    return run_on_lists(n, cam, opts, max_pairs, workspace, workspace_bytes, stream,
                        GaussianStats{pixel_mask, weight_sum, weight_max, pixels, 0, nullptr, nullptr, false});
}

int gsr_render_gaussian_stats(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                              size_t workspace_bytes, const uint8_t *pixel_mask, float *weight_sum, float *weight_max, uint32_t *pixels,
                              void *stream)
{
    return render_on_lists(scene, cam, opts, max_pairs, workspace, workspace_bytes, stream,
                           GaussianStats{pixel_mask, weight_sum, weight_max, pixels, 0, nullptr, nullptr, false});
}

int gsr_blend_pick(int64_t n, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace, size_t workspace_bytes,
                   float median_T, int32_t *out_best_id, float *out_best_w, int32_t *out_median_id, int32_t *out_count, void *stream)
{
    return run_on_lists(n, cam, opts, max_pairs, workspace, workspace_bytes, stream, Pick{median_T, out_best_id, out_best_w, out_median_id, out_count});
}

int gsr_render_pick(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                    size_t workspace_bytes, float median_T, int32_t *out_best_id, float *out_best_w, int32_t *out_median_id,
                    int32_t *out_count, void *stream)
{
    return render_on_lists(scene, cam, opts, max_pairs, workspace, workspace_bytes, stream,
                           Pick{median_T, out_best_id, out_best_w, out_median_id, out_count});
}

int gsr_blend_topk(int64_t n, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace, size_t workspace_bytes,
                   int32_t k, int32_t select, int32_t *out_ids, float *out_weights, float *out_final_T, void *stream)
{
    return run_on_lists(n, cam, opts, max_pairs, workspace, workspace_bytes, stream, TopK{k, select, out_ids, out_weights, out_final_T});
}

int gsr_render_topk(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                    size_t workspace_bytes, int32_t k, int32_t select, int32_t *out_ids, float *out_weights, float *out_final_T,
                    void *stream)
{
    return render_on_lists(scene, cam, opts, max_pairs, workspace, workspace_bytes, stream, TopK{k, select, out_ids, out_weights, out_final_T});
}

// ---- feature maps, their gradient and view statistics for several views per launch sequence ---------------------------------------
static const char VIEWS_OF_TWO_SIZES[] = "views of a launch sequence must share one frame size";

// What the gsr_*_views entries refuse about their views before anything else (and before any HIP call): view v works in slice v
static int check_views(const GsrCamera *cams, int32_t n_views, const GsrOptions *opts)
{
    if (!cams) { set_error("null cameras"); return GSR_ERR_BAD_ARG; }
    if (!opts) { set_error("null options"); return GSR_ERR_BAD_ARG; }
    if (n_views < 1 || n_views > MAX_VIEWS) { set_error("bad view count %d (1 .. %d)", (int)n_views, MAX_VIEWS); return GSR_ERR_BAD_ARG; }
    const int rc = check_one_frame_size(cams, n_views, VIEWS_OF_TWO_SIZES);
    if (rc) return rc;
    if (opts->output_layout == 1) { set_error("views of a launch sequence are [H,W] maps or shard strips: output_layout = 1 is not supported"); return GSR_ERR_BAD_ARG; }
    return GSR_OK;
}

// Stages 1-2 of gsr_lists_views; keep_batch_words: a later group of gsr_render_channels_batch
static int lists_views(const GsrScene *scene, const GsrCamera *cams, int32_t n_views, const GsrOptions *opts, int64_t max_pairs,
                       void *workspace, size_t workspace_bytes, void *stream, bool keep_batch_words)
{
    Workspace ws;
    int rc = check_view_slices(scene->n, cams, n_views, opts, max_pairs, workspace, workspace_bytes, &ws);
    if (rc) return rc;
    GsrOptions o = *opts;
    o.colour_stage = 0;
    const FramePlan plan = plan_frame(ws, o);
    hipStream_t s = static_cast<hipStream_t>(stream);
    rc = launch_preprocess(*scene, cams, o, ws, plan, nullptr, reset_words_of(&o, keep_batch_words), s);
    if (rc) return rc;
    return bin_sort_impl(&o, ws, plan, s);
}

int gsr_lists_views(const GsrScene *scene, const GsrCamera *cams, int32_t n_views, const GsrOptions *opts, int64_t max_pairs,
                    void *workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_scene(scene);
    if (rc) return rc;
    rc = check_views(cams, n_views, opts);
    if (rc) return rc;
    return lists_views(scene, cams, n_views, opts, max_pairs, workspace, workspace_bytes, stream, false);
}

extern "C++" {
// What a gsr_blend_X_views entry refuses before it looks at the workspace: the views, the consumer's own, its strides
template <class Consumer>
static int check_on_views(const GsrCamera *cams, int32_t n_views, const GsrOptions *opts, const Consumer &c)
{
    int rc = check_views(cams, n_views, opts);
    if (!rc) rc = c.check(&cams[0], opts);
    return rc ? rc : c.check_view_strides(view_plane_pixels(cams[0], *opts), n_views);
}

// behind them: the frame's checks for the slices, the plan, and the consumer's launch on the lists of n gaussians in every slice
template <class Consumer>
static int on_view_lists(int64_t n, const GsrCamera *cams, int32_t n_views, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                         size_t workspace_bytes, void *stream, const Consumer &c)
{
    Workspace ws;
    const int rc = check_view_slices(n, cams, n_views, opts, max_pairs, workspace, workspace_bytes, &ws);
    if (rc) return rc;
    const FramePlan plan = plan_frame(ws, *opts);
    return c.launch(Lists{cams[0], *opts, ws, plan, static_cast<hipStream_t>(stream)});
}

template <class Consumer>
static int run_on_view_lists(int64_t n, const GsrCamera *cams, int32_t n_views, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                             size_t workspace_bytes, void *stream, const Consumer &c)
{
    const int rc = check_on_views(cams, n_views, opts, c);
    return rc ? rc : on_view_lists(n, cams, n_views, opts, max_pairs, workspace, workspace_bytes, stream, c);
}
}  // extern "C++"

int gsr_blend_channels_views(int64_t n, const GsrCamera *cams, int32_t n_views, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                             size_t workspace_bytes, const float *features, int32_t channels, int64_t feature_stride, float *out_maps,
                             int64_t map_stride, float *out_final_T, int64_t T_stride, void *stream)
{
    return run_on_view_lists(n, cams, n_views, opts, max_pairs, workspace, workspace_bytes, stream,
                             Channels{features, channels, feature_stride, out_maps, out_final_T, map_stride, T_stride});
}

int gsr_blend_channels_backward_views(int64_t n, const GsrCamera *cams, int32_t n_views, const GsrOptions *opts, int64_t max_pairs,
                                      void *workspace, size_t workspace_bytes, const float *grad_maps, int64_t map_stride, int32_t channels,
                                      float *grad_features, int64_t grad_stride, void *stream)
{
    return run_on_view_lists(n, cams, n_views, opts, max_pairs, workspace, workspace_bytes, stream,
                             ChannelsBackward{grad_maps, channels, grad_features, grad_stride, map_stride});
}

int gsr_blend_gaussian_stats_views(int64_t n, const GsrCamera *cams, int32_t n_views, const GsrOptions *opts, int64_t max_pairs,
                                   void *workspace, size_t workspace_bytes, const uint8_t *pixel_masks, int64_t mask_stride,
                                   float *weight_sum, float *weight_max, uint32_t *pixels, uint32_t *view_hits, uint32_t *view_bits,
                                   void *stream)
{
    return run_on_view_lists(n, cams, n_views, opts, max_pairs, workspace, workspace_bytes, stream,
                             GaussianStats{pixel_masks, weight_sum, weight_max, pixels, mask_stride, view_hits, view_bits, true});
}

int gsr_render_channels_batch(const GsrScene *scene, const GsrCamera *cams, int32_t n_cams, const GsrOptions *opts, int64_t max_pairs,
                              void *workspace, size_t workspace_bytes, const float *features, int32_t channels, int64_t feature_stride,
                              float *out_maps, int64_t map_stride, float *out_final_T, int64_t T_stride, void *stream)
{
    int rc = check_scene(scene);
    if (rc) return rc;
    if (!cams) { set_error("null cameras"); return GSR_ERR_BAD_ARG; }
    if (!opts) { set_error("null options"); return GSR_ERR_BAD_ARG; }
    if (n_cams < 0) { set_error("bad camera count %d", (int)n_cams); return GSR_ERR_BAD_ARG; }
    if (n_cams == 0) return GSR_OK;
    rc = check_one_frame_size(cams, n_cams, VIEWS_OF_TWO_SIZES);  // every camera against the first, whatever the group it falls into
    if (rc) return rc;
    // (a group's own checks, on a group as large as any: the strides are asked for whenever there is a second camera)
    const Channels c{features, channels, feature_stride, out_maps, out_final_T, map_stride, T_stride};
    rc = check_on_views(cams, std::min<int32_t>(n_cams, 2), opts, c);
    if (rc) return rc;
    rc = check_sizes(scene->n, cams[0].width, cams[0].height, max_pairs);
    if (rc) return rc;
    GsrOptions o = *opts;
    o.colour_stage = 0;
    return for_view_groups(n_cams, views_per_launch(scene, &cams[0], opts, max_pairs, workspace_bytes, n_cams), [&](int32_t first, int count, int32_t g) {
        const int lists_rc = lists_views(scene, &cams[first], count, opts, max_pairs, workspace, workspace_bytes, stream, g > 0);
        return lists_rc ? lists_rc : on_view_lists(scene->n, &cams[first], count, &o, max_pairs, workspace, workspace_bytes, stream, c.from_view(first));
    });
}

int gsr_read_stats(void *workspace, size_t workspace_bytes, GsrStats *out, void *stream)
{
    if (!workspace || !out || workspace_bytes < sizeof(FrameCtrl)) { set_error("bad argument"); return GSR_ERR_BAD_ARG; }
    static_assert(sizeof(GsrStats) == 48 && offsetof(FrameCtrl, digit_tot) == sizeof(GsrStats), "GsrStats is the head of FrameCtrl");
    hipStream_t s = static_cast<hipStream_t>(stream);
    {  // total the blend's per-workgroup counters; the kernel finds them through the offsets kept in FrameCtrl
        const int rc = launch_blend_stats(static_cast<FrameCtrl *>(workspace), workspace_bytes, s);
        if (rc != GSR_OK) return rc;
    }
    // the whole control block (2 KB): GsrStats is its head, the sticky record of earlier frames its tail
    FrameCtrl host;
    GSR_HIP(hipMemcpyAsync(&host, workspace, sizeof(FrameCtrl), hipMemcpyDeviceToHost, s));
    GSR_HIP(hipStreamSynchronize(s));
    memcpy(out, &host, sizeof(GsrStats));
    if (out->overflow & 1u) {
        set_error("pair overflow: the frame needs %u (gaussian,tile) pairs", out->n_pairs_bbox);
        return GSR_ERR_PAIR_OVERFLOW;
    }
    if (out->overflow & 2u) {
        // the flag is sticky over a batch / a run of keep_flags frames while sort_passes describes the LAST frame: report what
        // the worst frame needed, or a caller that re-renders with "GsrStats.sort_passes" could be handed its own bound back
        out->sort_passes = std::max(out->sort_passes, host.batch_sort_passes);
        set_error("the depth sort needs %u passes, more than depth_sort_passes allowed", out->sort_passes);
        return GSR_ERR_SORT_PASSES;
    }
    return GSR_OK;
}

int gsr_scene_order_bytes(int64_t n, size_t *bytes)
{
    if (!bytes || n < 0 || n > 0x7FFFFFFF) { set_error("bad argument"); return GSR_ERR_BAD_ARG; }
    *bytes = scene_order_bytes(n);
    return GSR_OK;
}

int gsr_scene_order(int64_t n, const float *means, uint32_t *perm_out, void *workspace, size_t workspace_bytes, void *stream)
{
    if (n < 0 || n > 0x7FFFFFFF || (n > 0 && (!means || !perm_out || !workspace))) { set_error("bad argument"); return GSR_ERR_BAD_ARG; }
    if (n > 0 && reinterpret_cast<uintptr_t>(workspace) % 256 != 0) { set_error("workspace must be 256-byte aligned"); return GSR_ERR_BAD_ARG; }
    if (workspace_bytes < scene_order_bytes(n)) {
        set_error("workspace too small: %zu bytes given, %zu needed", workspace_bytes, scene_order_bytes(n));
        return GSR_ERR_WORKSPACE;
    }
    return launch_scene_order(n, means, perm_out, workspace, static_cast<hipStream_t>(stream));
}

int gsr_scene_bounds(int64_t n, const float *means, const float *log_scales, float *bounds_out, void *stream)
{
    if (n < 0 || n > 0x7FFFFFFF || (n > 0 && (!means || !log_scales || !bounds_out))) { set_error("bad argument"); return GSR_ERR_BAD_ARG; }
    if (reinterpret_cast<uintptr_t>(bounds_out) % 16 != 0) { set_error("bounds_out must be 16-byte aligned"); return GSR_ERR_BAD_ARG; }
    return launch_scene_bounds(n, means, log_scales, bounds_out, static_cast<hipStream_t>(stream));
}

int gsr_block_visibility(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, uint8_t *dead_out, void *stream)
{
    int rc = check_scene(scene);
    if (rc) return rc;
    if (!cam || !opts || !scene->block_bounds || (scene->n > 0 && !dead_out)) { set_error("null camera / options / block_bounds / output"); return GSR_ERR_BAD_ARG; }
    if (cam->width <= 0 || cam->height <= 0) { set_error("bad frame size %dx%d", cam->width, cam->height); return GSR_ERR_BAD_ARG; }
    Workspace ws;  // nothing to carve: the plan reads the frame's tile grid from it
    carve_workspace(nullptr, scene->n, cam->width, cam->height, 0, &ws);
    return launch_block_visibility(*scene, *cam, plan_frame(ws, *opts), dead_out, static_cast<hipStream_t>(stream));
}

int gsr_sh_to_rgb(int64_t n, const float *means, const float *sh, const float cam_center[3], int32_t degree, float *rgb_out,
                  void *stream)
{
    if (n < 0 || (n > 0 && (!means || !sh || !rgb_out)) || !cam_center || degree < 0 || degree > 3) {
        set_error("bad argument"); return GSR_ERR_BAD_ARG;
    }
    if (reinterpret_cast<uintptr_t>(sh) % 16 != 0) { set_error("sh must be 16-byte aligned"); return GSR_ERR_BAD_ARG; }
    return launch_sh_to_rgb(n, means, sh, cam_center, degree, rgb_out, static_cast<hipStream_t>(stream));
}

int gsr_cov3d(int64_t n, const float *log_scales, const float *quats, float *cov3d_out, void *stream)
{
    if (n < 0 || (n > 0 && (!log_scales || !quats || !cov3d_out))) { set_error("bad argument"); return GSR_ERR_BAD_ARG; }
    if (reinterpret_cast<uintptr_t>(quats) % 16 != 0) { set_error("quats must be 16-byte aligned"); return GSR_ERR_BAD_ARG; }
    return launch_cov3d(n, log_scales, quats, cov3d_out, static_cast<hipStream_t>(stream));
}

int gsr_project_to_camera_space(int64_t n, const float *means, const float w2c[16], float *out, void *stream)
{
    if (n < 0 || !w2c || (n > 0 && (!means || !out))) { set_error("bad argument"); return GSR_ERR_BAD_ARG; }
    return launch_project(n, means, w2c, out, static_cast<hipStream_t>(stream));
}

int gsr_compute_2d_covariance(int64_t n, const float *cov3d, const float *cam_means, double tan_fov_x, double tan_fov_y,
                              double focal_x, double focal_y, const float w2c[16], float *cov2d_out, void *stream)
{
    if (n < 0 || !w2c || (n > 0 && (!cov3d || !cam_means || !cov2d_out))) { set_error("bad argument"); return GSR_ERR_BAD_ARG; }
    if (reinterpret_cast<uintptr_t>(cov2d_out) % 16 != 0) { set_error("cov2d_out must be 16-byte aligned"); return GSR_ERR_BAD_ARG; }
    // focals / 2 (rasterize.py:216) and 1.3 * tan_fov (rasterize.py:210-211), formed in float64 like the reference
    return launch_cov2d(n, cov3d, cam_means, w2c, (float)(focal_x / 2.0), (float)(focal_y / 2.0), (float)(1.3 * tan_fov_x),
                        (float)(1.3 * tan_fov_y), cov2d_out, static_cast<hipStream_t>(stream));
}

int gsr_compute_covering_bbox(int64_t n, const float *screen_means, const float *cov2d, double width, double height,
                              int64_t *tile_bboxes_out, void *stream)
{
    if (n < 0 || (n > 0 && (!screen_means || !cov2d || !tile_bboxes_out))) { set_error("bad argument"); return GSR_ERR_BAD_ARG; }
    if (reinterpret_cast<uintptr_t>(cov2d) % 16 != 0) { set_error("cov2d must be 16-byte aligned"); return GSR_ERR_BAD_ARG; }
    return launch_bbox(n, screen_means, cov2d, (float)width, (float)height, tile_bboxes_out, static_cast<hipStream_t>(stream));
}

int gsr_rasterize_gaussian(int64_t gaussian_index, int64_t n, const int64_t *bboxes, float *screen, const float *screen_means,
                           const float *sigmas, const float *rgb, float *opacity_buffer, const float *opacity, int32_t width,
                           int32_t height, void *stream)
{
    if (!bboxes || !screen || !screen_means || !sigmas || !rgb || !opacity_buffer || !opacity || width <= 0 || height <= 0) {
        set_error("bad argument"); return GSR_ERR_BAD_ARG;
    }
    if (gaussian_index < 0 || gaussian_index >= n) { set_error("gaussian_index %lld out of range", (long long)gaussian_index); return GSR_ERR_BAD_ARG; }
    return launch_rasterize_gaussian(gaussian_index, bboxes, screen, screen_means, sigmas, rgb, opacity_buffer, opacity, width, height,
                                     static_cast<hipStream_t>(stream));
}

}  // extern "C"
