/*
 * gsr.h — C ABI of libgsr.so, the MI355X (gfx950) forward rasterizer for 3D Gaussian Splatting.
 *
 * Boundary: the reference (arnaudstiegler/torch-gaussian-splatting-rasterizer)
 * has no FFI of its own — its "render call" is the body of rasterize.py:315-478.  This header is what a
 * binding for that path binds: every entry point names the reference lines it replaces.  Rules:
 *   - extern "C", POD structs, plain pointers and sizes; no C++/torch types; no exceptions cross.
 *   - every call returns int: GSR_OK or a negative GsrStatus; gsr_last_error() gives thread-local text.
 *     (gsr_camera_backward_bytes returns a size: it cannot fail.)
 *   - the CALLER owns all device memory (inputs, outputs, one scratch workspace sized by
 *     gsr_workspace_bytes); the library never allocates on the hot path and holds no global state,
 *     so calls with distinct workspaces/streams may run concurrently.
 *   - all device work is enqueued on the caller's hipStream_t (passed as void*); nothing synchronises
 *     except gsr_read_stats.
 *   - fp32 throughout (the reference's arithmetic type); device pointers unless marked [host].
 *     (gsr_camera_backward sums its fp32 per-gaussian terms over the scene in double and writes doubles.)
 *   - no environment variable is read anywhere: the A/B switches of rounds 1-3 are GsrOptions fields since 0.5.0
 *     (fine_binning, shard_preprocess, blend_pipe_tiles, sh_dense_min) — same frames whatever they say.
 */
#ifndef GSR_H
#define GSR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_VERSION 600 /* 0.6.0 (additions since, no existing entry point or struct changed: gsr_blend_features / gsr_render_features —
                            depth, alpha and caller-supplied channels composited with the colour frame's weights; gsr_blend_channels /
                            gsr_render_channels + GSR_MAX_FEATURE_CHANNELS — any number of channels, rows at a caller's stride, many channels per walk of the lists; gsr_blend_channels_backward /
                            gsr_render_channels_backward — the transpose of gsr_blend_channels in the channels: the gradient of a map with respect to the per-gaussian rows; gsr_blend_pick /
                            gsr_render_pick — per-pixel ids: the gaussian of largest weight, the one at which T crosses a threshold, the contributor count; gsr_blend_topk /
                            gsr_render_topk + GSR_MAX_TOPK — per-pixel contributor lists: the k heaviest or the k nearest gaussians of a pixel with their weights; gsr_blend_slab /
                            gsr_render_slab — gsr_blend_channels between two per-pixel depth limits: a depth test against a z-buffer, section planes, depth layers; gsr_blend_gaussian_stats /
                            gsr_render_gaussian_stats — per-gaussian statistics of a view: the sum and the maximum of a gaussian's weights and the number of pixels it reaches, optionally under a pixel mask; gsr_lists_views /
                            gsr_blend_channels_views / gsr_blend_channels_backward_views / gsr_blend_gaussian_stats_views / gsr_render_channels_batch — feature maps, their gradient and the
                            statistics for several views per launch sequence, with view_hits, the exact number of views that reach a gaussian; gsr_blend_splat_backward /
                            gsr_render_splat_backward — the gradient of a feature map and of the final T with respect to the 2-D splat: opacity, 2-D mean, inverse 2-D covariance, and the
                            per-pixel absolute mean gradients; gsr_project_backward — that gradient chained through the projection to the scene's means, log-scales,
                            quaternions and opacity logits; gsr_sh_backward — the transpose of gsr_sh_to_rgb: a view's colour gradient carried to the SH coefficients
                            and, through the view direction, to the means; gsr_camera_backward / gsr_camera_backward_bytes — the splat gradient of a view
                            summed into the gradient with respect to the camera: w2c, full_proj, the focal lengths and cam_center, 32 doubles): several views per launch sequence — gsr_render_batch / gsr_render_batch_slots put as many views through ONE
                            preprocess / sort / blend launch sequence as the workspace holds slices of gsr_workspace_bytes() (GsrOptions.batch_views
                            caps it); gsr_blend takes the scene again (NULL = what gsr_preprocess left in the workspace); GsrScene.block_bounds + gsr_scene_bounds /
                            gsr_block_visibility (block-level culling); GsrOptions.tile_row_block (tile-row shards in pairs of rows).  0.5.0: GsrOptions.saturation_rule (the exact colour-saturation early-out), the four environment switches became GsrOptions
                            fields (the library reads no environment and holds no function statics), GsrOptions.colour_stage / no_order_hint,
                            GsrStats.colour_evals, + gsr_scene_order.  0.4.0: GsrOptions.keep_flags, GsrOptions.accum_dtype; GsrStats.sort_passes reports the worst frame when the bound was exceeded; blend_impl 2
                            (matrix-pipe experiment) removed; the frame clear covers every word of the control block.  0.3.0: GsrOptions.depth_sort_passes, GsrStats.sort_passes, GSR_ERR_SORT_PASSES.  0.2.1: + gsr_render_batch_slots.
                            0.2.0: gsr_preprocess_geometry/_color removed (measured slower), gsr_read_stats takes a non-const workspace */

typedef enum GsrStatus {
    GSR_OK = 0,
    GSR_ERR_BAD_ARG = -1,       /* null pointer, non-positive size, unsupported option */
    GSR_ERR_WORKSPACE = -2,     /* workspace smaller than gsr_workspace_bytes() says */
    GSR_ERR_PAIR_OVERFLOW = -3, /* (gaussian,tile) pairs exceeded max_pairs: frame is incomplete, re-render with more */
    GSR_ERR_HIP = -4,           /* a HIP runtime call failed; see gsr_last_error() */
    GSR_ERR_SORT_PASSES = -5    /* the frame's depth keys span more bits than GsrOptions.depth_sort_passes passes cover: the frame is
                                   wrong, re-render with GsrStats.sort_passes (or 0) */
} GsrStatus;

/* Constants of rasterize.py:29-38 and the literals buried in the reference's glue. */
#define GSR_TILE 16                  /* BLOCK_SIZE, rasterize.py:34 */
#define GSR_GAUSSIAN_SPREAD 3.0f     /* rasterize.py:32 */
#define GSR_MAX_ALPHA 0.99f          /* MAX_GAUSSIAN_DENSITY, rasterize.py:36 */
#define GSR_MIN_ALPHA (1.0f / 255.0f)/* rasterize.py:38 */
#define GSR_CULL_Z 0.2f              /* rasterize.py:377 */
#define GSR_LOWPASS 0.3f             /* rasterize.py:249-250 */
#define GSR_EIG_FLOOR 0.1f           /* rasterize.py:172,175 */
#define GSR_MAX_PAIRS 0xFFFFE000ll   /* largest max_pairs: pairs are indexed in 32 bits, one 4096-pair sort tile of headroom */
#define GSR_MAX_BATCH_VIEWS 8        /* most views gsr_render_batch puts through one launch sequence */
#define GSR_BOUNDS_BLOCK 64          /* consecutive gaussians per entry of GsrScene.block_bounds */

/* Camera-independent trained gaussians, exactly the values stored in the INRIA .ply
 * (rasterize.py:98-106,354-358; utils.py:10-31).  Row-major dense arrays.
 * The ORDER of the arrays is the caller's; it decides one thing: gaussians at EXACTLY equal depth (fp32 z_cam) are drawn in array-
 * index order (the reference's torch.sort, rasterize.py:425, leaves their order undefined; in practice torch's CPU sort keeps file
 * order).  Arrays in .ply file order therefore reproduce the reference's practical frame bit for bit in its tie order as well; arrays
 * reordered for speed (gsr_scene_order: what the Python loaders do by default, `spatial_order=False` / `--scene-order file` turn it
 * off) render the same frame except where two tied gaussians overlap — measured up to ~1e-2 per pixel on scenes with many exact
 * ties (tools/fuzz_parity.py: 0.0086), ~1e5 tie pairs among the 3.4 M visible gaussians of a 6 M-gaussian scene. */
typedef struct GsrScene {
    int64_t n;                  /* number of gaussians */
    const float *means;         /* [n,3]  x,y,z */
    const float *log_scales;    /* [n,3]  scale_0..2, BEFORE exp (rasterize.py:97) */
    const float *quats;         /* [n,4]  rot_0..3 = (w,x,y,z), un-normalised (rasterize.py:99-112) */
    const float *opacity_logit; /* [n]    BEFORE sigmoid (rasterize.py:358) */
    const void *sh;             /* [n,16,3] sh[i][k][c], k=0 is f_dc (utils.py:21-31); fp32, or IEEE fp16 if sh_dtype = 1 */
    int32_t sh_degree;          /* 0..3; the reference always evaluates 3 (rasterize.py:368) */
    int32_t sh_dtype;           /* 0 = float32 (the reference's type), 1 = float16 storage (evaluated in fp32; halves the
                                   192-B/gaussian stream that dominates stage 1; ~91 dB vs fp32 coefficients) */
    const float *block_bounds;  /* optional (NULL = none): [ceil(n / GSR_BOUNDS_BLOCK)][8] from gsr_scene_bounds — per block of
                                   GSR_BOUNDS_BLOCK consecutive gaussians the box of their means and their largest log-scale.  The
                                   first kernel of a frame tests every block against the view (cull plane rasterize.py:377, frame, this
                                   rank's tile rows) and the preprocess skips, BEFORE touching their gaussians' 44 B each, the blocks none
                                   of whose gaussians can be drawn: a conservative bound, frames are bit-identical with and without.
                                   Worth having when the arrays are in a spatial order (gsr_scene_order).  16-byte aligned. */
} GsrScene;

/* One view.  Filled by gsr_camera_setup() or by hand.  All matrices are in the reference's
 * row-vector convention (transposed at rasterize.py:361-362): x_cam = x_w @ w2c[:3,:3] + w2c[3,:3]. */
typedef struct GsrCamera {
    float w2c[16];        /* get_world_to_camera_matrix(...).T, rasterize.py:59-77,:361 */
    float full_proj[16];  /* w2c @ get_projection_matrix(...).T, rasterize.py:123-151,:362-364 */
    float cam_center[3];  /* inverse(w2c)[3,:3], spherical_harmonics.py:35 */
    float focal_x, focal_y;     /* focal of the EWA Jacobian = full-res fx,fy / 2 (rasterize.py:216; quirk Q3) */
    float lim_x, lim_y;         /* fp32(1.3*tan(fov/2)), rasterize.py:210-211 */
    float tan_fov_x, tan_fov_y; /* rasterize.py:344-345 */
    int32_t width, height;      /* output size in pixels, rasterize.py:338 */
} GsrCamera;

typedef struct GsrOptions {
    int32_t reference_compat; /* 1 (default): reproduce Q1 (column W-1 / row H-1 never drawn, rasterize.py:271-272,
                                 :415-418) and Q2 (skip if ANY conic entry == 0, :441).  0: draw every pixel. */
    float early_out_T;        /* a wave of 64 pixels stops once all their transmittances are <= this.  0 (default) is
                                 exact — identical bits to blending every gaussian like the reference (Q5); see
                                 saturation_rule for what "exact" stops on.  >0 is a bounded approximation (INRIA
                                 uses 1e-4). */
    int32_t tile_row_begin;   /* multi-GPU sharding: this call bins+blends tile rows begin, begin+step, ... (blocks of rows: tile_row_block) */
    int32_t tile_row_step;    /* default 0 / 1 = all rows */
    int32_t output_layout;    /* 0 (default): image [H,W,3] (= screen.transpose(1,0), rasterize.py:471);
                                 1: reference `screen` layout [W,H,3] (rasterize.py:437);
                                 2: compact strip [rows_of_this_shard*16, W, 3] for the framebuffer gather */
    int32_t no_footprint_cull;/* 0 (default): tile rects / quadrant tests are tightened to the AABB of the region where
                                 alpha > 1/255 can hold (exact: skipped work contributes nothing).  1: bin the
                                 reference's full 3-sigma tile rect — only to prove that property in tests. */
    int32_t blend_impl;       /* 0 (default): the blend kernel with its inner walk hand-scheduled (EXEC-masked update, csrc/blend.hip).
                                 1: the same kernel with the walk in plain C — the readable statement of the arithmetic and the A/B
                                 reference; frames are bit-identical to 0. */
    int32_t draw_limit;       /* 0 (default): blend everything.  k > 0: blend only the first k gaussians of the reference's
                                 draw order (depth order restricted to those its skip guard rasterize.py:441 lets through) —
                                 the progressive frames of --generate_video (rasterize.py:448-450). */
    int32_t output_dtype;     /* 0 (default): the frame is float32.  1: the frame is stored as bfloat16 (round to nearest even),
                                 6 B per pixel (BASELINE configs[2]); T and the colour sums are ALWAYS accumulated in fp32
                                 registers — bf16 accumulators measure 41 dB, below the 50 dB bar.
                                 out_final_T stays float32. */
    int32_t depth_sort_passes;/* 0 (default): enqueue the four radix passes any depth range can need; those a frame does not need
                                 return at once, but still cost their launches (3 per pass, ~4.6 us each).  1..4: the caller's bound on
                                 what the frames need — GsrStats.sort_passes of an earlier frame of the scene (3 whenever the depths stay
                                 within 0.2 .. 13 000): only that many are enqueued.  Verified on the device like max_pairs: a frame
                                 that needs more is flagged and gsr_read_stats returns GSR_ERR_SORT_PASSES. */
    int32_t accum_dtype;      /* 0 (default): T and the colour sums are accumulated in fp32 registers.  1: they are rounded to bfloat16 after
                                 every gaussian — BASELINE configs[2] as literally worded ("bf16 blend accumulator").  A measurement
                                 option, not a fast path (it runs the plain-C blend kernel, whatever blend_impl says): 8 mantissa bits
                                 cannot carry a transmittance through hundreds of layers, the frame lands far below the fp32 one
                                 (tests/test_gpu_configs.py prints the PSNR; SURVEY.md §7.3 probed 41 dB on the CPU). */
    int32_t keep_flags;       /* 0 (default): the frame starts from a cleared control block (a fresh workspace needs no initialisation).
                                 1: the frame keeps the overflow record of the frames rendered before it on this workspace (bits of
                                 GsrStats.overflow, the largest D, the most depth-sort passes), so ONE gsr_read_stats after a run of
                                 unchecked frames — first frame 0, the rest 1 — reports whether ANY of them exceeded max_pairs or
                                 depth_sort_passes.  The views of gsr_render_batch are chained this way internally. */
    int32_t saturation_rule;  /* when may a quadrant of 64 pixels stop EXACTLY (early_out_T = 0)?
                                 0 (default): once no later gaussian can change a bit of its COLOUR: every pixel has
                                 T <= 2^-25 * min(Cr, Cg, Cb).  The update is C = fma(w, c, C) with w = fl(alpha T) <= T and c <= 1 (Q7),
                                 so w c <= T < ulp(C) / 2 for each channel and the fma returns C unchanged, now and ever after (T only
                                 shrinks).  Pixels the reference never draws (Q1) count as finished.  Frames are bit-identical to rule 1;
                                 ~4x fewer evaluated entries on the bench frame.  When out_final_T is requested rule 1 applies (T itself
                                 is then an output and keeps shrinking).
                                 1: once T has underflowed to 0.0f for all 64 pixels (rounds 1-3) — the A/B reference of rule 0.
                                 3, 4: rule 0 with the FRONT SLICE forced on / switched off (tests, A/B timing; 2 is refused).  The front
                                 slice is how gsr_render_forward / gsr_render_batch / gsr_render_batch_slots build a whole colour frame
                                 of a large scene under rule 0 (coarse binning, no shard, draw_limit = 0, early_out_T = 0, fp32
                                 accumulators, blend_impl = 0, no out_final_T; by plan: from 3000 tiles, 6 000 000 gaussians and SIX views per launch
                                 sequence on — one view alone is faster in one pass, so gsr_render_forward slices only when forced): the
                                 nearest eighth of the draw order is binned and blended first, the rest is binned and sorted only
                                 where a tile is still open after it, and blended on from the stored fp32 T and colour sums.  Same
                                 bits as the single pass (csrc/binning.hip has the argument).  Its planes (16 B per pixel) lie over the
                                 workspace's depth keys and unpacked rects, which need ~257 gaussians per tile: rule 0 builds a scene
                                 below that in one pass, rule 3 refuses it (GSR_ERR_BAD_ARG).  After such a frame the depth keys are
                                 gone and the lists in the workspace are the second slice's remainder, not the frame's: a gsr_bin_sort
                                 there needs a gsr_preprocess first, and a stage-3 entry over the workspace's lists needs both (see
                                 gsr_render_forward).
                                 1 never slices; the staged calls and every list consumer never do either: their lists are complete. */
    int32_t fine_binning;     /* 0 (default): (gaussian, 32x32 cell) pairs whenever the frame allows (<= 4096 px, n <= 2^28), the blend filters
                                 the cell lists by tile.  1: (gaussian, 16x16 tile) pairs — the path wider frames always take; A/B timing and
                                 the test that both build the same frame (csrc/binning.hip).  Was GSR_FINE_BINNING. */
    int32_t shard_preprocess; /* tile-row shards only: 0 (default) = the three-phase shard preprocess from tile_row_step 5 on, 1 = always the
                                 whole-frame kernel, 2 = always the three-phase kernel (csrc/preprocess.hip).  Was GSR_SHARD_PREPROCESS. */
    int32_t blend_pipe_tiles; /* tile count up to which the blend runs its pipelined one-quadrant walk: 0 (default) = 1280, -1 = never
                                 (csrc/blend.hip).  Was GSR_BLEND_PIPE_TILES. */
    int32_t no_order_hint;    /* 0 (default): tiles are launched heaviest first by what each tile's blend STAGED in the last frame rendered on
                                 this workspace (consecutive frames of a camera path look alike; a tile saturates long before the end of
                                 its list), falling back to the list length where that record is missing or impossible.  1: by list length
                                 alone (rounds 1-3).  A schedule only: every order renders the same bits. */
    int32_t colour_stage;     /* where is sh_to_rgb (spherical_harmonics.py:27-73) evaluated?
                                 0 (default): in the blend, when a tile first STAGES a gaussian (its 192-B SH row is read and its colour
                                 evaluated then, and remembered in the gaussian's record for the tiles that stage it later): gaussians
                                 that no tile reaches before it is saturated — most of a dense scene — never read their SH row.  The
                                 preprocess then reads 44 B per gaussian instead of up to 236.  Same arithmetic in the same order on the
                                 same inputs: frames are bit-identical to 1.
                                 1: in gsr_preprocess, for every visible gaussian (rounds 1-3) — the A/B reference of 0.
                                 (gsr_preprocess with a GsrDebugOut always evaluates there: `rgb` is one of its outputs.)  Only
                                 gsr_preprocess reads this field; gsr_blend finds out from the records. */
    int32_t sh_dense_min;     /* visible gaussians per wave from which the preprocess fetches the wave's 64 SH rows whole through LDS:
                                 0 (default) = 48, 65 = never (csrc/preprocess.hip).  Was GSR_SH_DENSE. */
    int32_t batch_views;      /* gsr_render_batch / gsr_render_batch_slots: at most this many views per launch sequence; 0 (default) = as many
                                 as the workspace holds slices for, up to GSR_MAX_BATCH_VIEWS.  1 = one view at a time (rounds 1-4).  Same
                                 frames whatever it says. */
    int32_t tile_row_block;   /* multi-GPU sharding: how many consecutive tile rows form one unit of the interleave.  0 / 1 (default): single
                                 rows — this call owns tile rows begin, begin + step, ...  2: PAIRS of rows, i.e. the two tile rows of one
                                 32x32 binning cell — block b = rows 2b, 2b + 1 is owned when b % step == begin.  A rank then bins and sorts
                                 only the cells it owns (with single rows and an even step every cell row is shared by two ranks, and each
                                 of them emits and sorts all its pairs); the strip (output_layout = 2) holds the owned rows in ascending
                                 order either way.  Same pixels; only the partition differs. */
} GsrOptions;

/* Counters of one frame (device -> host with gsr_read_stats). */
typedef struct GsrStats {
    uint32_t n_visible;     /* V: gaussians that survive cull and have a non-empty footprint */
    uint32_t n_pairs_bbox;  /* D: pair slots this frame needs, i.e. what max_pairs must cover: (gaussian, 32x32 cell) pairs of the
                               visible gaussians' rects (frames wider than 4096 px: (gaussian, 16x16 tile) pairs of this shard) */
    uint32_t n_pairs;       /* E: entries of the per-tile lists the blend consumes (this shard; after footprint culling).  A front-slice
                               frame (GsrOptions.saturation_rule): the entries actually EMITTED — those of tiles already finished when
                               the second slice is binned are not; D above stays what the whole draw order needs */
    uint32_t overflow;      /* bit 0: D exceeded max_pairs (frame incomplete); bit 1: the depth sort needed more passes than
                               depth_sort_passes allowed (frame wrong) */
    uint32_t max_list_len;  /* longest list a blend workgroup walks: per 32x32 cell (frames wider than 4096 px: per 16x16 tile; a
                               front-slice frame: per cell and slice) */
    uint32_t sort_passes;   /* radix passes the depth sort of this frame needs (1..4): the bound to pass as depth_sort_passes.  When
                               overflow bit 1 is set: the most any frame since the last cleared one (keep_flags, batches) needed */
    uint64_t wave_entries;  /* (8x8 quadrant, entry) pairs the blend actually evaluated: 64 pixel evaluations each */
    uint64_t fetched_entries; /* list entries the blend staged (<= n_pairs: a saturated tile stops fetching) */
    uint64_t colour_evals;  /* sh_to_rgb evaluations (192-B SH rows read) by the blend: colour_stage = 0 evaluates a gaussian when a tile
                               first stages an entry of it that NEEDS the colour — one whose exact footprint hits an 8x8 quadrant of the
                               tile that has not finished; an entry over finished quadrants only, or over none, leaves the record
                               pending for the next tile.  Tiles racing for the same gaussian may each evaluate it (same result), so this
                               is an UPPER-BOUND estimate of the gaussians coloured and varies by a few per cent from run to run.  0 when the
                               preprocess evaluated the colours (colour_stage = 1: n_visible evaluations there). */
} GsrStats;

/* Optional intermediates of gsr_preprocess, one entry per gaussian, any pointer may be NULL.
 * They are the tensors the reference's helpers return (used by the drop-in helper functions and parity tests). */
typedef struct GsrDebugOut {
    float *cov3d;         /* [n,9]  get_covariance_matrix_from_mesh, rasterize.py:89-120 */
    float *cam_means;     /* [n,3]  project_to_camera_space, rasterize.py:80-86 */
    float *cov2d;         /* [n,4]  compute_2d_covariance, rasterize.py:201-252 (before the cull zeroing of :388) */
    float *screen_means;  /* [n,2]  rasterize.py:391 */
    int64_t *tile_bboxes; /* [n,4]  compute_covering_bbox, rasterize.py:154-198 */
    float *sigmas;        /* [n,3]  conic (sigma_x, sigma_y, sigma_xy), rasterize.py:404-411 */
    int64_t *pixel_bboxes;/* [n,4]  rasterize.py:415-419 */
    float *rgb;           /* [n,3]  sh_to_rgb, spherical_harmonics.py:27-73 */
    float *opacity;       /* [n]    sigmoid(opacity_logit), rasterize.py:358 */
} GsrDebugOut;

int gsr_version(void);
const char *gsr_last_error(void);
void gsr_default_options(GsrOptions *opts /* [host] */);

/* [host] Camera set-up from COLMAP extrinsics/intrinsics: replaces rasterize.py:336-345 (fov, focals),
 * :59-77 + :361 (world->camera), :123-151 + :362-364 (projection, full transform) and
 * spherical_harmonics.py:35 (camera centre).  fx_full/fy_full/cam_width/cam_height are the FULL-RES camera
 * of cameras.bin (cam_info[1]); width/height the size of the images_{K} frame (rasterize.py:338). */
int gsr_camera_setup(const double qvec[4], const double tvec[3], double fx_full, double fy_full, int64_t cam_width,
                     int64_t cam_height, int32_t width, int32_t height, GsrCamera *out /* [host] */);

/* Bytes of scratch one frame needs for n gaussians, a width x height target and room for max_pairs
 * pairs.  max_pairs is the caller's bound on D = the (gaussian, 32x32 cell) pairs of a frame (frames wider than 4096 px:
 * (gaussian, 16x16 tile) pairs); GsrStats.n_pairs_bbox reports what a frame needed; exceeding it is reported, never UB. */
/* The limits it and every render entry point apply (GSR_ERR_BAD_ARG past them): n in [0, GSR_MAX_GAUSSIANS], width and height in
 * [1, GSR_MAX_FRAME_SIDE] (tile rects are ushort4: 65535 tiles per side), max_pairs in [0, GSR_MAX_PAIRS]. */
#define GSR_MAX_GAUSSIANS 0x7FFFFFFFll
#define GSR_MAX_FRAME_SIDE (65535 * GSR_TILE)
int gsr_workspace_bytes(int64_t n, int32_t width, int32_t height, int64_t max_pairs, size_t *bytes /* [host] */);

/* Stage 1 — per-gaussian preprocessing, fused: rasterize.py:354-420 (means, cov3D, opacity, SH colour,
 * camera/clip projection, z<0.2 cull, EWA 2D covariance, NDC->pixel, radius + tile rect, conic, pixel rect). */
int gsr_preprocess(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, void *workspace,
                   size_t workspace_bytes, const GsrDebugOut *debug /* [host], may be NULL */, void *stream);

/* Stage 2 — depth order (rasterize.py:424-425, ties broken by gaussian index) and 16x16 tile binning:
 * radix sort of the visible gaussians by depth, pair emission in depth order, stable radix sort by tile,
 * per-tile [begin,end) ranges.  Needs gsr_preprocess on the same workspace first. */
int gsr_bin_sort(int64_t n, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                 size_t workspace_bytes, void *stream);

/* Stage 3 — front-to-back compositing of every tile list: rasterize.py:436-446 (driver loop + skip guard)
 * and :255-305 (rasterize_gaussian).  out_image layout per opts->output_layout; out_final_T [H,W] may be NULL.
 * n and max_pairs must be the values given to the earlier stages (the library keeps no state; they fix the
 * workspace layout).  With GsrOptions.colour_stage = 0 (default) this stage evaluates sh_to_rgb (spherical_harmonics.py:27-73) for
 * the gaussians its tiles stage, from `scene`'s means / sh arrays and cam->cam_center: pass the scene gsr_preprocess was given
 * (the same values: the arrays may have MOVED since, they may not have changed).  scene = NULL: the pointers gsr_preprocess left
 * in the workspace are used instead — then those arrays must still be alive where they were, which no argument check can see
 * (a binding should always pass the scene). */
int gsr_blend(const GsrScene *scene /* may be NULL */, int64_t n, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs,
              void *workspace, size_t workspace_bytes, void *out_image /* float32 or bfloat16, opts->output_dtype */,
              float *out_final_T, void *stream);

/* Stages 1-3 back to back: the whole render call of rasterize.py:354-446.
 * WHAT IT LEAVES IN THE WORKSPACE.  This entry, gsr_render_batch and gsr_render_batch_slots owe the caller the frame and the counters,
 * NOT the frame's lists: when the plan takes the front slice (GsrOptions.saturation_rule; by default gsr_render_batch of six or more
 * views of a whole 1080p-class frame of a scene of 6 000 000 gaussians or more) the lists left behind are the second slice's remainder — the far seven eighths of the draw order,
 * without the gaussians and tile bits of tiles that had finished — and the depth keys are overwritten.  A stage-3 entry that walks the
 * workspace's lists (a second gsr_blend, gsr_blend_features / _channels / _pick / _topk / _slab / _gaussian_stats, the backward
 * blends) must therefore follow gsr_preprocess + gsr_bin_sort (or a gsr_render_X / gsr_lists_views of its own kind), never one of the
 * three fused colour-frame entries: nothing on the host can see the difference, and the maps would be built from partial lists without
 * an error.  saturation_rule = 4 restores the old behaviour (complete lists after the fused entries) at the single pass's speed. */
int gsr_render_forward(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs,
                       void *workspace, size_t workspace_bytes, void *out_image, float *out_final_T, void *stream);

/* Stage 3 for the caller's own per-gaussian values (no reference counterpart: rasterize.py composites the SH colour and nothing else):
 * out_map[p][c] = sum_i w_i(p) features[i][c], c = 0..2, over the same depth-ordered lists and with the same weights w_i = alpha_i T_i
 * as the colour frame — the arithmetic of gsr_blend with features[i] in the place of the colour, unclamped: with the gaussians' colours
 * as features the map is gsr_blend's frame bit for bit.  Depth map: features[i] = z_cam; accumulated alpha: features[i] = 1 (then
 * out = 1 - final T up to rounding).  features [n,3] float32 in the order of the scene arrays; finite values for every gaussian that
 * can be drawn.  An alternative stage 3: needs gsr_preprocess and gsr_bin_sort on the workspace first, may be called any number of
 * times (more than three channels: three at a time), and mixes freely with gsr_blend — it reads the records' geometry and opacity
 * only, never their colour words, and leaves the launch-order hint of the colour frames alone, so a gsr_blend before or after it
 * renders the bits it renders alone.  out_map: layout per opts->output_layout with 3 channels, float32; out_final_T may be NULL.
 * Honoured options: reference_compat, tile_row_begin / _step / _block, output_layout, no_footprint_cull, draw_limit, fine_binning,
 * depth_sort_passes, keep_flags, early_out_T.  A quadrant of 64 pixels stops once T <= early_out_T for all of them: with 0 (default) that
 * is T == 0.0f, which is exact for finite features; the colour-saturation rule of gsr_blend rests on colours in [0, 1] and does not
 * apply, so saturation_rule, blend_impl, blend_pipe_tiles, no_order_hint and colour_stage are ignored.  GSR_ERR_BAD_ARG for
 * output_dtype = 1 and accum_dtype = 1 (the maps are float32).  Single views.  gsr_read_stats afterwards describes this blend
 * (wave_entries, fetched_entries; colour_evals = 0). */
int gsr_blend_features(int64_t n, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                       size_t workspace_bytes, const float *features /* [n,3] */, float *out_map, float *out_final_T, void *stream);

/* Stages 1-3 back to back with the feature blend as stage 3.  The preprocess runs as with colour_stage = 0 whatever opts says: no SH
 * row is read (scene->sh must still be a valid array: a later gsr_blend on this workspace evaluates colours from it). */
int gsr_render_features(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                        size_t workspace_bytes, const float *features /* [n,3] */, float *out_map, float *out_final_T, void *stream);

/* gsr_blend_features for 1 <= channels <= GSR_MAX_FEATURE_CHANNELS channels, read where the caller keeps them:
 * out_map[p][c] = sum_i w_i(p) features[i * feature_stride + c], c = 0 .. channels - 1.  One walk of the tile lists composites up to 16
 * channels (the geometry of a (pixel, gaussian) evaluation is paid once per walk, not once per three channels); more channels are
 * further walks inside this one call, on the caller's stream.  Every channel is, bit for bit and at any early_out_T, the channel
 * gsr_blend_features composites from the same values, and gsr_read_stats afterwards describes one walk (every walk stages and
 * evaluates the same entries: wave_entries and fetched_entries are gsr_blend_features').  features: float32, any 4-byte-aligned
 * address, rows feature_stride >= channels floats apart (a column window of a wider array needs no copy; rows on 16-byte boundaries
 * are read with 16-byte loads); finite values for every gaussian that can be drawn.  out_map: layout per opts->output_layout with
 * `channels` channels, float32, contiguous; out_final_T may be NULL.  Semantics, honoured and ignored options, and what it leaves alone
 * on the workspace (the records' colour words, the launch-order hint) are gsr_blend_features'.  GSR_ERR_BAD_ARG, before any HIP call
 * or look at the workspace, for a null camera, options, features or output map, channels < 1 or > GSR_MAX_FEATURE_CHANNELS,
 * feature_stride < channels, output_dtype = 1, accum_dtype = 1.  Single views. */
#define GSR_MAX_FEATURE_CHANNELS 1024
int gsr_blend_channels(int64_t n, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                       size_t workspace_bytes, const float *features /* row i at features + i * feature_stride */,
                       int32_t channels, int64_t feature_stride, float *out_map /* [.., channels] */, float *out_final_T,
                       void *stream);

/* Stages 1-3 back to back with gsr_blend_channels as stage 3; the preprocess runs as with colour_stage = 0, like gsr_render_features'. */
int gsr_render_channels(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                        size_t workspace_bytes, const float *features /* row i at features + i * feature_stride */,
                        int32_t channels, int64_t feature_stride, float *out_map /* [.., channels] */, float *out_final_T,
                        void *stream);

/* The transpose of gsr_blend_channels under the same camera and options:
 * grad_features[i * grad_stride + c] += sum_p w_i(p) grad_map[p][c], c = 0 .. channels - 1, with the weights w_i = alpha_i T_i the
 * forward composites with, bit for bit, over the forward's lists and with its stop rule.  out_map is linear in the features, so this
 * is its exact gradient with respect to them; nothing flows through the geometry or the opacities.  It ADDS into grad_features (the
 * caller zeroes it, or keeps summing over views); rows of gaussians no pixel draws are not touched.  grad_map: float32, contiguous,
 * layout per opts->output_layout with `channels` channels (what gsr_blend_channels writes); pixels the forward leaves 0 (the undrawn
 * last column / row of reference_compat) contribute nothing.  grad_features: float32, rows grad_stride >= channels floats apart.
 * Honoured and ignored options, and what it leaves alone on the workspace, are gsr_blend_channels'; gsr_read_stats afterwards
 * describes the walk (wave_entries / fetched_entries are the forward's).  Nothing else is written: no map, no final T.
 *   - The sums are float atomic adds: their value depends on the order the adds arrive in, so two calls with the same input can
 *     differ in the last bits.
 *   - grad_map must be finite.
 *   - grad_features must not alias grad_map.
 * GSR_ERR_BAD_ARG, before any HIP call or look at the workspace, for a null camera, options, grad_map or grad_features, channels < 1
 * or > GSR_MAX_FEATURE_CHANNELS, grad_stride < channels, output_dtype = 1, accum_dtype = 1.  Single views. */
int gsr_blend_channels_backward(int64_t n, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                                size_t workspace_bytes, const float *grad_map /* [.., channels], layout per opts->output_layout */,
                                int32_t channels, float *grad_features /* row i at + i * grad_stride */, int64_t grad_stride,
                                void *stream);

/* gsr_preprocess (as with colour_stage = 0) + gsr_bin_sort + gsr_blend_channels_backward */
int gsr_render_channels_backward(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                                 size_t workspace_bytes, const float *grad_map /* [.., channels], layout per opts->output_layout */,
                                 int32_t channels, float *grad_features /* row i at + i * grad_stride */, int64_t grad_stride,
                                 void *stream);

/* The gradient of a feature map with respect to the 2-D SPLAT, under the camera and options of the forward.  With the map
 * out_map[p] = sum_i w_i(p) f_i of gsr_blend_channels, its final transmittance T_final[p], and
 *   L = sum_p grad_map[p] . out_map[p] + sum_p grad_T[p] T_final[p],
 * row i of grad_splat ([n][8] float32, 32 bytes a row) receives the derivative of L in what gsr_preprocess computes for gaussian i
 * (GsrDebugOut: opacity, screen_means, sigmas = the inverse 2-D covariance s0, s1, s2):
 *   [0] dL/d opacity   [1] dL/d mean_x   [2] dL/d mean_y   [3] dL/d s0   [4] dL/d s1   [5] dL/d s2
 *   [6] sum_p |dL/d mean_x restricted to pixel p|   [7] the same for mean_y   (want_abs only; else columns 6 and 7 are not touched).
 * Means are in pixels.  Per pair: dx = mean_x - x, dy = mean_y - y, power = -(s0 dx^2 + s1 dy^2) / 2 - s2 dx dy, u = opacity
 * exp(power), alpha = min(0.99, u), kept where alpha > 1/255 and power <= 0.  The support (footprint, threshold, power <= 0) is held
 * fixed, and the cap has derivative 0: a pair with u >= 0.99 contributes nothing (the reference implementation of 3DGS lets the
 * gradient pass through its cap; this does not).  The weights, the lists and the stop rule are gsr_blend_channels', bit for bit; the
 * walk runs twice inside the one launch (first for S' = sum_i w_i s_i + grad_T T_final with s_i = grad_map[p] . f_i, then for the
 * gradients, with what lies behind gaussian i formed as S' minus the running sum), no per-pixel state is taken from the caller and
 * no map is written.  More than 16 channels are further launches inside this call; grad_T enters once.
 * It ADDS into grad_splat (the caller zeroes it, or keeps summing over views); rows of gaussians no pixel draws are not touched.
 * features: as gsr_blend_channels reads them, rows feature_stride >= channels floats apart.  grad_map: float32, contiguous, layout
 * per opts->output_layout with `channels` channels (what gsr_blend_channels writes); grad_T: NULL or one float per pixel in the
 * layout of out_final_T; pixels the forward leaves 0 / 1 (the undrawn last column / row of reference_compat) contribute nothing.
 * min_T >= 0: a pair whose incoming transmittance T_i is below min_T contributes nothing of its own (it still counts in what lies
 * in front of the others); 0 switches it off.  Honoured and ignored options, and what it leaves alone on the workspace, are
 * gsr_blend_channels'; gsr_read_stats afterwards describes the second walk (wave_entries / fetched_entries are the forward's).
 *   - The sums are float atomic adds: their value depends on the order the adds arrive in, so two calls with the same input can
 *     differ in the last bits.
 *   - Accuracy: S' minus the running sum carries an absolute error of about 2^-24 |S'| alpha / (1 - alpha) per pixel, so a gaussian
 *     seen only through T <~ 1e-6 gets a gradient that is tiny but relatively meaningless; min_T and early_out_T cut such pairs off.
 *   - features, grad_map and grad_T must be finite.
 *   - grad_splat must not alias features, grad_map or grad_T.
 * GSR_ERR_BAD_ARG, before any HIP call or look at the workspace, for a null camera, options, features, grad_map or grad_splat,
 * channels < 1 or > GSR_MAX_FEATURE_CHANNELS, feature_stride < channels, min_T negative or not finite, want_abs with channels > 16
 * (the absolute sums are not linear in the channels: one walk), output_dtype = 1, accum_dtype = 1.  Single views. */
int gsr_blend_splat_backward(int64_t n, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                             size_t workspace_bytes, const float *features /* row i at features + i * feature_stride */,
                             int64_t feature_stride, int32_t channels, const float *grad_map /* [.., channels] */,
                             const float *grad_T /* may be NULL */, float min_T, int32_t want_abs, float *grad_splat /* [n][8], ADDS */,
                             void *stream);

/* gsr_preprocess (as with colour_stage = 0) + gsr_bin_sort + gsr_blend_splat_backward */
int gsr_render_splat_backward(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                              size_t workspace_bytes, const float *features /* row i at features + i * feature_stride */,
                              int64_t feature_stride, int32_t channels, const float *grad_map /* [.., channels] */,
                              const float *grad_T /* may be NULL */, float min_T, int32_t want_abs, float *grad_splat /* [n][8], ADDS */,
                              void *stream);

/* The projection backward: the splat gradient of a view chained to what the SCENE stores.  Row i of grad_splat ([n][8] float32, as
 * gsr_blend_splat_backward writes it; columns 0-5 = d L / d opacity, mean_x, mean_y, s0, s1, s2 are read, columns 6 and 7 are
 * ignored) is carried through the transpose of gsr_preprocess' geometry for gaussian i under this camera, and the result is ADDED
 * into four arrays laid out like the scene's: grad_means [n,3], grad_log_scales [n,3], grad_quats [n,4] (w, x, y, z as stored, not
 * normalised), grad_opacity_logit [n].  Any of the four may be NULL (not all): a NULL output and the work feeding only it are
 * skipped, and each output is bit for bit what it is in a call with all four.  One thread per gaussian, no atomics: two calls with
 * the same input give the same bits, and adding a row twice doubles it exactly.
 * The forward is recomputed in fp32 from the expressions of gsr_preprocess, in their operation order, so the chain linearises the
 * values the forward used.  Stage by stage, last to first:
 *   sigmas <- cov2d        s0 = c / det, s1 = a / det, s2 = -b01 / det, det = a c - b10 b01, with a, b01, b10, c four separate inputs;
 *   cov2d <- (T, cov3d)    cov2d = T cov3d T^T + 0.3 I with T = J A^T (A = w2c[:3,:3]); the low-pass is a constant;
 *   J <- cam_mean          J = [[fx / z, 0, -fx u / z], [0, fy / z, -fy v / z]], u = clamp(x / z, +-lim_x), v likewise;
 *   cam_mean <- mean       through w2c;
 *   screen_mean <- mean    through full_proj, the divide 1 / (w + 1e-7) and the NDC -> pixel map (means are in pixels);
 *   cov3d <- M             cov3d = M M^T, M = R diag(exp(log_scales));
 *   R <- quaternion        through the normalisation q / max(|q|, 1e-12) (at the floor the divisor is a constant);
 *   opacity <- logit       sigmoid(x) sigmoid(-x), which keeps its digits where 1 - sigmoid(x) has lost them.
 * Clamp rule: where the ray clamp is active the derivative in x / z is 0, and t_x = +-lim_x z still depends on z (likewise y).
 * Held fixed: the tile rect, the footprint, the 1/255 threshold and the cull — the support gsr_blend_splat_backward already holds
 * fixed.  No colour term HERE: nothing flows through the SH evaluation; the view direction's part of d / d mean is what
 * gsr_sh_backward adds into the same grad_means.
 * Skip rule: a gaussian whose six values are all zero is not touched — its rows of the outputs are neither read nor written, and
 * a wave of 64 consecutive such gaussians reads nothing but their rows of grad_splat.  A gaussian contributes nothing either when
 * the forward culls it (z_cam < GSR_CULL_Z), when its det is 0, when a conic entry is not finite, or, with reference_compat,
 * when a conic entry is 0 (the reference never draws it): whatever its row holds.
 * Needs no workspace and no lists; depends on the scene, the camera and opts->reference_compat only.  The scene's arrays are read,
 * never written: a caller that updates a resident scene in place must rebuild what was derived from it (block_bounds, the order).
 *   - grad_splat must be finite where it is not zero.
 *   - No output may alias grad_splat (refused), another output or an array of the scene (not checked: the caller's to keep);
 *     grad_splat and grad_quats must be 16-byte aligned.
 * GSR_ERR_BAD_ARG, before any HIP call, for a null scene, camera, options or grad_splat, all four outputs NULL, an output that
 * aliases grad_splat, a misaligned grad_splat or grad_quats, a scene gsr_preprocess refuses (sh_dtype), output_dtype = 1,
 * accum_dtype = 1.  Single views: sum over cameras by calling it once per view into the same outputs. */
int gsr_project_backward(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts,
                         const float *grad_splat /* [n][8], columns 0-5 read */,
                         float *grad_means /* [n,3] ADDS, may be NULL */, float *grad_log_scales /* [n,3] */,
                         float *grad_quats /* [n,4] */, float *grad_opacity_logit /* [n] */, void *stream);

/* The SH colour backward: the exact transpose of gsr_sh_to_rgb at scene->sh_degree and cam->cam_center.  Row i of grad_rgb
 * (d L / d colour of gaussian i; columns 0-2 of rows grad_rgb_stride floats apart are read, so a column window of a wider array is
 * read where it lies) is carried to the gaussian's SH coefficients and, through the view direction, to its mean.  No cull: the
 * operator has none because gsr_sh_to_rgb has none.  Per gaussian, with d = mean - cam_center, r = |d|, u = d / r and
 * v_c = sum_k b_k(u) sh[k][c] + 0.5 the value before the clamp:
 *   Clamp mask   m_c = 1 where 0 <= v_c <= 1, else 0: the edges pass, as the forward's v < 0 ? 0 : (v > 1 ? 1 : v) passes them.
 *                v_c is recomputed by the forward's own function on the same fp32 values: the decision is the forward's, bit for bit.
 *   grad_sh      [n,16,3] float32: grad_sh[i][k][c] += b_k(u) m_c g_c for k < (degree + 1)^2; coefficients k >= (degree + 1)^2 are
 *                neither read nor written.  With sh_dtype = 1 (fp16 storage) it is the gradient in the widened values, still float32.
 *   grad_means   [n,3]: grad_means[i] += (I - u u^T) / r  sum_k grad_u b_k(u) (sum_c m_c g_c sh[k][c]).  Zero at degree 0: it is
 *                then neither computed nor written.
 *   r == 0       (a mean on the camera centre) makes the forward NaN above degree 0; the gaussian then contributes nothing.
 * Both outputs are ADDED into; either may be NULL (not both), and the other is bit for bit what it is in a call with both.  One
 * thread per gaussian, no atomics: two calls with the same input give the same bits, and adding a row twice doubles it exactly.
 * Skip rule: a gaussian whose three values are all zero is not touched — its rows of the outputs, its mean and its SH row are
 * neither read nor written — and a wave of 64 consecutive such gaussians reads nothing but their 12 B of grad_rgb each; a gaussian
 * all of whose channels with a nonzero value are clamped writes nothing either.
 * Needs no workspace, no lists and no options; the scene's arrays are read, never written.
 *   - grad_rgb must be finite where it is not zero.
 *   - No output may alias grad_rgb (refused), the other output or an array of the scene (not checked: the caller's to keep);
 *     grad_sh must be 16-byte aligned.
 * GSR_ERR_BAD_ARG, before any HIP call, for a null scene, camera or grad_rgb, both outputs NULL, grad_rgb_stride < 3, an output that
 * aliases grad_rgb, a misaligned grad_sh, a scene gsr_preprocess refuses (sh_dtype, sh_degree).  n = 0 is GSR_OK.  Single views: sum
 * over cameras by calling it once per view into the same outputs. */
int gsr_sh_backward(const GsrScene *scene, const GsrCamera *cam,
                    const float *grad_rgb /* [n] rows, columns 0-2 read */, int64_t grad_rgb_stride /* floats, >= 3 */,
                    float *grad_sh /* [n,16,3] fp32, ADDS, may be NULL */, float *grad_means /* [n,3] ADDS, may be NULL */,
                    void *stream);

/* The camera backward: the splat gradient of a view chained to the CAMERA.  grad_splat is the array gsr_project_backward reads
 * ([n][8] float32, columns 0-5 read, columns 6 and 7 ignored); per gaussian the forward is recomputed and the upstream quantities
 * are formed exactly as gsr_project_backward does it — the same rules, bit for bit, by the same functions: the same Skip rule (a
 * row of six zeros is not touched, a wave of 64 such rows reads nothing else), the same exclusions (z_cam < GSR_CULL_Z, det is 0, a
 * conic entry not finite or, with reference_compat, 0), the same Clamp rule (where the ray clamp is active the derivative in x / z is
 * 0, and t_x = +-lim_x z still depends on z), the same quantities Held fixed (the tile rect, the footprint, the 1/255 threshold and
 * the cull) and, new here, the depth order and lim_x / lim_y.  Where gsr_project_backward carries gcm, gT, gJ.. and gpt.. on to the
 * gaussian's mean, this entry multiplies them by what the camera contributed and sums over the gaussians:
 *   w2c through the camera-space mean   cm[j] = sum_k p[k] V[4 k + j] + V[12 + j]: dV[4 k + j] += p[k] gcm[j], dV[12 + j] += gcm[j];
 *   w2c through T = J A^T               T[r][c] = sum_m V[4 c + m] J[r][m]: dV[4 c + m] += sum_{r = 0, 1} gT[r][c] J[r][m];
 *   full_proj                           dF[4 k + j] += p[k] gpt_j, dF[12 + j] += gpt_j for j in {0, 1, 3};
 *   focal lengths                       J00 = fx / z and J02 = -fx t_x / z^2 are linear in fx: dfx += gJ00 / z - gJ02 t_x / z^2
 *                                       (no division by fx); fy likewise;
 *   cam_center                          grad_view_means [n][3] is the view-direction term of d L / d mean — what gsr_sh_backward
 *                                       leaves in a zeroed [n,3] array when called with grad_sh = NULL; the SH colours depend on
 *                                       mean - cam_center, so dcc[k] -= grad_view_means[i][k], for EVERY row (no cull: gsr_sh_backward
 *                                       has none).  No SH row is read here.
 * Either input may be NULL (not both), and the entries the other feeds are bit for bit what they are in a call with both.
 * Result layout: grad_camera is 32 doubles on the device, WRITTEN (not added into) — raw partials in the struct fields as the kernels
 * read them, so a hand-filled GsrCamera has a gradient too:
 *   [3 k + j]        k = 0..3, j = 0..2    d L / d w2c[4 k + j]       (column 3 of w2c is never read by the forward: derivative 0)
 *   [12 + 3 k + jj]  k = 0..3, jj = 0..2   d L / d full_proj[4 k + (0, 1, 3)[jj]]   (column 2 of full_proj is never read)
 *   [24], [25]       d L / d focal_x, focal_y
 *   [26 .. 28]       d L / d cam_center
 *   [29]             the number of gaussians that contributed a grad_splat term: touched and passing every exclusion.  Exact.
 *   [30], [31]       0
 * Reduction: the per-gaussian terms are float32, as in the chain they extend; every sum across gaussians is done in double — within
 * a thread, across a wave, across a workgroup and across workgroups.  No atomics; which thread takes which gaussian and the order of
 * every sum depend on n alone: two calls with the same input give the same bits, and doubling the inputs doubles the result exactly.
 * Workspace: gsr_camera_backward_bytes(n) = 256 * max(1, ceil(B / ceil(B / 768))) bytes with B = ceil(n / 256) — one row of 32 doubles
 * per workgroup, at most 768 of them (a 256-byte multiple); every row is written before it is read, so nothing has to be cleared.
 * 8-byte aligned.  No lists; depends on the scene, the camera and opts->reference_compat only.  The scene's arrays are read, never written.
 *   - grad_splat and grad_view_means must be finite.
 * GSR_ERR_BAD_ARG, before any HIP call, for a null scene, camera, options, grad_camera or workspace, both inputs NULL, a workspace
 * that is too small, a misaligned grad_splat (16 bytes), grad_camera or workspace (8 bytes), grad_camera or the workspace overlapping
 * an input or each other, a scene gsr_preprocess refuses (sh_dtype), output_dtype = 1, accum_dtype = 1.  n = 0 writes 32 zeros and is
 * GSR_OK.  Single views: sum over cameras on the caller's side. */
size_t gsr_camera_backward_bytes(int64_t n);
int gsr_camera_backward(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts,
                        const float *grad_splat /* [n][8], columns 0-5 read, may be NULL */,
                        const float *grad_view_means /* [n][3], may be NULL (not both) */,
                        double *grad_camera /* [32] device, WRITTEN */,
                        void *workspace, size_t workspace_bytes, void *stream);

/* Stage 3 for what no blended channel can hold — per pixel p, over the same depth-ordered lists and with the same weights
 * w_i = alpha_i T_i (and the same T, bit for bit) as gsr_blend_features (no reference counterpart):
 *   out_best_id[p]   = the gaussian of largest w_i(p), -1 where no gaussian has w > 0;   out_best_w[p] = that weight (0 with -1);
 *   out_median_id[p] = the first gaussian in draw order AFTER which the transmittance T is < median_T, -1 if T never gets there:
 *                      median_T = 0.5 is the "median depth" gaussian of 2DGS / gsplat, which ignores floaters that pull
 *                      sum w z forward; median_T = 1 the first gaussian with w > 0;
 *   out_count[p]     = how many gaussians have w_i(p) > 0.
 * Ids are indices into the caller's scene arrays (the order gsr_preprocess was given them in).  At EXACTLY equal weights the earlier
 * gaussian in draw order wins; at exactly equal depth the draw order is array-index order, as elsewhere (GsrScene).  Pixels the
 * frame never draws (the last column / row of reference_compat) hold -1, 0, -1, 0.  Each output is one [H,W] plane of 4-byte values
 * in opts->output_layout (image [H,W], screen [W,H] or strip [rows * 16, W]); any of the four may be NULL, not all.  out_count == NULL
 * selects a walk that stops earlier: once a pixel's median is found and T <= best_w no later gaussian can change either id
 * (w' = fl(alpha' T') <= T' <= T <= best_w and the maximum is strict) — exact, like every stop at early_out_T = 0; with out_count the
 * walk is gsr_blend_features' (T == 0.0f) and so are wave_entries / fetched_entries.  early_out_T > 0: gaussians behind T <= early_out_T
 * are not seen — an approximation, as in the feature blend.
 * An alternative stage 3 like gsr_blend_features: needs gsr_preprocess and gsr_bin_sort on the workspace first, may be called any
 * number of times and mixes freely with gsr_blend and the feature blends (it reads the records' geometry and opacity only, never
 * their colour words, and leaves the launch-order hint alone).  Honoured and ignored options are gsr_blend_features'.
 * GSR_ERR_BAD_ARG, before any HIP call or look at the workspace, for a null camera or options, all four outputs NULL, median_T NaN or
 * outside (0, 1], output_dtype = 1, accum_dtype = 1.  Single views.  gsr_read_stats afterwards describes this walk (wave_entries,
 * fetched_entries; colour_evals = 0). */
int gsr_blend_pick(int64_t n, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace, size_t workspace_bytes,
                   float median_T, int32_t *out_best_id, float *out_best_w, int32_t *out_median_id, int32_t *out_count, void *stream);

/* Stages 1-3 back to back with gsr_blend_pick as stage 3; the preprocess runs as with colour_stage = 0, like gsr_render_features'. */
int gsr_render_pick(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                    size_t workspace_bytes, float median_T, int32_t *out_best_id, float *out_best_w, int32_t *out_median_id,
                    int32_t *out_count, void *stream);

/* Stage 3 for per-pixel contributor LISTS — of every pixel p the k gaussians that make it, ids and weights (no reference
 * counterpart).  k is 1 .. GSR_MAX_TOPK, `select` one of GSR_TOPK_HEAVIEST / GSR_TOPK_NEAREST.
 * Lists, weights and T.  The lists are the depth-ordered lists of gsr_blend_features, the weights are w_i = alpha_i T_i, bit for bit
 * that kernel's, and so is T.  out_ids[p * k + j] and out_weights[p * k + j] hold slot j = 0 .. k-1 of pixel p, p laid out per
 * opts->output_layout: [H,W,k], [W,H,k] or the strip [rows * 16, W, k]; the k values of a pixel are contiguous and the stride is
 * exactly k.
 *   GSR_TOPK_HEAVIEST: the slots are sorted by weight, descending; only w > 0 enters.  At EXACTLY equal weights the earlier gaussian
 *     in draw order comes first — so if the k-th and a later one tie, the earlier keeps the slot (gsr_blend_pick's strict compare
 *     for best_id, generalised: k = 1 is best_id / best_w).
 *   GSR_TOPK_NEAREST: the slots are in draw order: the first k gaussians with w > 0 (k = 1 is gsr_blend_pick's median_id at
 *     median_T = 1).
 * Unused slots hold id -1 and weight 0; pixels the frame never draws (the last column / row of reference_compat) hold -1 / 0 in
 * every slot.  Ids are indices into the caller's scene arrays (the order gsr_preprocess was given them in); at exactly equal depth
 * the draw order is array-index order, as elsewhere (GsrScene).
 * out_ids or out_weights may be NULL, not both.  out_final_T: [H,W] float32 in the same layout (1 where the frame never draws), or
 * NULL.
 * Stop rule.  With out_final_T the walk is gsr_blend_features': a quadrant stops once T <= early_out_T for its pixels, because T
 * itself is an output, and wave_entries / fetched_entries are that kernel's.  Without it a quadrant also stops once none of its lists
 * can change: HEAVIEST — T <= the weight in slot k-1 (a later w' = fl(alpha' T') <= T' <= T <= w_k, so the strict `>` fails, and fails
 * forever because T only shrinks); NEAREST — slot k-1 is filled (or T == 0); undrawn pixels from the start.  All exact at
 * early_out_T = 0.  early_out_T > 0 is the feature blend's approximation: gaussians behind T <= early_out_T are not seen, and the
 * lists are the top k of the weights gsr_blend_features composites at that early_out_T, with or without out_final_T.
 * An alternative stage 3 like gsr_blend_features: needs gsr_preprocess and gsr_bin_sort on the workspace first, may be called any
 * number of times and mixes freely with gsr_blend, the feature blends and gsr_blend_pick (it reads the records' geometry and opacity
 * only, never their colour words, and only reads the launch-order hint).  Honoured and ignored options are gsr_blend_features'.
 * GSR_ERR_BAD_ARG, before any HIP call or look at the workspace, for a null camera or options, out_ids and out_weights both NULL,
 * k < 1 or > GSR_MAX_TOPK, select not 0 or 1, output_dtype = 1, accum_dtype = 1.  Single views.  gsr_read_stats afterwards describes
 * this walk (wave_entries, fetched_entries; colour_evals = 0). */
#define GSR_MAX_TOPK 16
#define GSR_TOPK_HEAVIEST 0   /* the k largest weights, heaviest first */
#define GSR_TOPK_NEAREST  1   /* the first k gaussians in draw order with w > 0, nearest first */
int gsr_blend_topk(int64_t n, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace, size_t workspace_bytes,
                   int32_t k, int32_t select, int32_t *out_ids, float *out_weights, float *out_final_T, void *stream);

/* Stages 1-3 back to back with gsr_blend_topk as stage 3; the preprocess runs as with colour_stage = 0, like gsr_render_features'. */
int gsr_render_topk(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                    size_t workspace_bytes, int32_t k, int32_t select, int32_t *out_ids, float *out_weights, float *out_final_T,
                    void *stream);

/* Stage 3 for caller-supplied channels BETWEEN TWO PER-PIXEL DEPTH LIMITS (no reference counterpart): gsr_blend_channels restricted,
 * pixel by pixel, to a part of the depth range — the splats in front of a mesh z-buffer, behind a section plane, behind the median
 * surface, one layer of a layered depth image.
 * Semantics.  depth_near and depth_far are [H,W] float32 planes [device], laid out per opts->output_layout exactly like out_final_T;
 * either may be NULL: no limit on that side.  Pixel p composites the gaussians with
 *     depth_near[p] <= z_i   and   z_i < depth_far[p]
 * (>= on the near side, < on the far side: consecutive slabs [a,b), [b,c) partition the range) and no others:
 *     out_map[p][c] = sum_i w_i(p) f_i[c],   out_final_T[p] = prod_i (1 - alpha_i(p))   over those gaussians, in draw order,
 * with T starting at 1 at the near limit: a gaussian in front of it is SKIPPED, not blended — it neither adds to the map nor dims
 * what lies behind it.  The arithmetic per gaussian is gsr_blend_channels'; with both planes NULL (or -inf / +inf everywhere) the map
 * and T are that function's bit for bit, and so are wave_entries / fetched_entries.
 * z_i is CAMERA-SPACE LINEAR DEPTH, the unit of the depth maps (f = z_cam through the feature blends), not NDC / z-buffer depth: the
 * float the depth sort orders the gaussians by, ((x * w2c[2] + y * w2c[6]) + z * w2c[10]) + w2c[14] evaluated in fp32 in exactly this
 * order without fused multiply-adds — the same bits as GsrDebugOut.cam_means[3 * i + 2].  A caller with an OpenGL-style depth buffer
 * linearises it first.
 * If either limit of a pixel is NaN, or depth_far[p] <= depth_near[p], the pixel draws nothing: its map is 0 and its T is 1.  Pixels
 * the frame never draws (the last column / row of reference_compat) hold 0 / 1 whatever the limits say.
 * Stop rule.  The lists are in ascending z (ties in array-index order), so a far limit keeps a prefix: a quadrant stops once every
 * pixel of it has T <= early_out_T, as in gsr_blend_channels, or — exactly — once the list has reached the largest far limit of its
 * pixels; the tile stops fetching when its four quadrants have.  Entries in front of the smallest near limit of a quadrant are
 * staged but never evaluated, and are not counted in wave_entries.
 * features / channels / feature_stride / out_map / out_final_T: gsr_blend_channels'.  scene may be NULL, as for gsr_blend: the means
 * are then read through the pointer the last gsr_preprocess on this workspace was given (which must still be valid); a non-NULL
 * scene must have scene->n == n.  An alternative stage 3 like gsr_blend_channels: needs gsr_preprocess and gsr_bin_sort on the
 * workspace first, may be called any number of times (one call per layer of a layered depth image) and mixes freely with the other
 * blends.  Honoured and ignored options are gsr_blend_channels' (draw_limit, early_out_T, the layouts and tile-row shards included).
 * GSR_ERR_BAD_ARG, before any HIP call or look at the workspace, for gsr_blend_channels' cases: a null camera, null options, null
 * features, a null out_map, channels < 1 or > GSR_MAX_FEATURE_CHANNELS, feature_stride < channels, output_dtype = 1, accum_dtype = 1.
 * Single views.  No backward.  gsr_read_stats afterwards describes this walk (wave_entries, fetched_entries; colour_evals = 0). */
int gsr_blend_slab(const GsrScene *scene /* may be NULL */, int64_t n, const GsrCamera *cam, const GsrOptions *opts,
                   int64_t max_pairs, void *workspace, size_t workspace_bytes, const float *features, int32_t channels,
                   int64_t feature_stride, const float *depth_near, const float *depth_far, float *out_map,
                   float *out_final_T, void *stream);

/* Stages 1-3 back to back with gsr_blend_slab as stage 3; the preprocess runs as with colour_stage = 0, like gsr_render_features'. */
int gsr_render_slab(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                    size_t workspace_bytes, const float *features, int32_t channels, int64_t feature_stride,
                    const float *depth_near, const float *depth_far, float *out_map, float *out_final_T, void *stream);

/* Stage 3 turned round: per GAUSSIAN i, over the pixels p of this view that count, with the weights w_i(p) = alpha_i T_i the feature
 * blends composite with — bit for bit, over their lists and with their stop rule (no reference counterpart):
 *   weight_sum[i] += sum_p w_i(p)                  the summed weight: gsr_blend_channels_backward of a one-channel map of ones;
 *   weight_max[i]  = max(weight_max[i], max_p w_i(p))   the largest weight the gaussian reaches in any pixel: the score of max-based pruning;
 *   pixels[i]     += #{p : w_i(p) > 0}             how many pixels it reaches (gsr_blend_pick's out_count rule, transposed): pixels[i] > 0
 *                                                  over a zeroed array is the EXACT visible set of the view.
 * Each array has n entries in the order of the caller's scene arrays (the order gsr_preprocess was given them in); any of the three
 * may be NULL, not all three, and an absent output costs nothing.  All three ACCUMULATE (the caller zeroes them, or keeps going over
 * views: sum of sums, max of maxima, sum of counts); entries of gaussians that no counted pixel draws are not touched.
 *   - weight_max and pixels are exact and reproducible to the bit: the maximum is taken over the floats' bit patterns as unsigned
 *     integers (for non-negative floats that is the float maximum) and neither depends on the order the atomics arrive in.
 *     weight_max must therefore hold NON-NEGATIVE FINITE floats on entry (zeros, or the result of an earlier call).
 *   - weight_sum is a float atomic sum: its value depends on the order the adds arrive in, so two calls with the same input can
 *     differ in the last bits.
 * pixel_mask: one byte per pixel [device], laid out per opts->output_layout like out_final_T ([H,W], [W,H] or the strip
 * [rows * 16, W]); non-zero = the pixel counts.  NULL: every drawn pixel counts.  Pixels the forward leaves 0 (the undrawn last
 * column / row of reference_compat) never count.  The mask selects what is COUNTED, not what is blended: T evolves as in the
 * unmasked view.  A quadrant of 64 pixels none of which counts is skipped, and a tile of four such quadrants stages nothing.
 * Honoured and ignored options, the stop rule (a quadrant stops once T <= early_out_T for all its pixels; exact at 0) and what it
 * leaves alone on the workspace are gsr_blend_channels_backward's: it reads the records' geometry and opacity only, no colour word,
 * and leaves the launch-order hint alone.  gsr_read_stats afterwards describes this walk (wave_entries, fetched_entries;
 * colour_evals = 0).
 * GSR_ERR_BAD_ARG, before any HIP call or look at the workspace, for a null camera or options, all three outputs NULL,
 * output_dtype = 1, accum_dtype = 1.  Single views. */
int gsr_blend_gaussian_stats(int64_t n, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                             size_t workspace_bytes, const uint8_t *pixel_mask /* may be NULL */, float *weight_sum,
                             float *weight_max, uint32_t *pixels, void *stream);

/* gsr_preprocess (as with colour_stage = 0) + gsr_bin_sort + gsr_blend_gaussian_stats */
int gsr_render_gaussian_stats(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, int64_t max_pairs, void *workspace,
                              size_t workspace_bytes, const uint8_t *pixel_mask /* may be NULL */, float *weight_sum,
                              float *weight_max, uint32_t *pixels, void *stream);

/* Several views of ONE resident scene (the reference renders one view per process, rasterize.py:315-329; BASELINE configs[3] is a
 * camera set).  cams[n_cams] [host] must share width/height; frame i goes to out_images + i * frame_stride (in elements of the
 * output dtype).
 * Views per launch sequence.  With S = gsr_workspace_bytes(n, width, height, max_pairs), a workspace of K * S bytes is K slices,
 * and K = min(workspace_bytes / S, GSR_MAX_BATCH_VIEWS, opts->batch_views if set, n_cams) views at a time go through ONE sequence
 * of launches — one preprocess that reads every gaussian's 44 B once for the K cameras, one set of depth-sort and cell-sort launches
 * over K x the keys, one blend over K x the tiles: ~22 dispatches per K frames instead of per frame, each K times better filled.
 * View i works in slice i % K (workspace + (i % K) * S) and its frame is bit for bit the frame gsr_render_forward renders.
 * Counters: gsr_read_stats on slice j (pointer workspace + j * S, size S) describes the LAST view rendered there (views j, j + K, ...);
 * an overflow in any of them is sticky in it, and n_pairs_bbox / sort_passes then report what the WORST of them needed (the values
 * to re-render with).  A caller that checks a batch reads slices 0 .. min(K, n_cams) - 1. */
int gsr_render_batch(const GsrScene *scene, const GsrCamera *cams /* [host] */, int32_t n_cams, const GsrOptions *opts,
                     int64_t max_pairs, void *workspace, size_t workspace_bytes, void *out_images, int64_t frame_stride,
                     void *stream);

/* The same with n_slots batches in flight: with K = the views per launch sequence as above (every workspace of workspace_bytes = K
 * slices), group g = views g K .. g K + K - 1 is enqueued with workspaces[g % n_slots] on streams[g % n_slots], so that the ramps
 * and tails of one group's kernels overlap another's (the library keeps no state; each slot is one more (workspace, stream) pair).
 * Frames are bit-identical to gsr_render_batch.  Each slice's counters afterwards describe the LAST view rendered there; an overflow
 * in any of them is sticky.  The caller orders the streams against whatever produced the scene and whatever consumes the frames. */
int gsr_render_batch_slots(const GsrScene *scene, const GsrCamera *cams /* [host] */, int32_t n_cams, const GsrOptions *opts,
                           int64_t max_pairs, void *const *workspaces /* [host] n_slots device pointers */, size_t workspace_bytes,
                           void *const *streams /* [host] n_slots streams */, int32_t n_slots, void *out_images, int64_t frame_stride);

/* Feature maps, their gradient and the per-gaussian statistics for SEVERAL VIEWS PER LAUNCH SEQUENCE (no reference counterpart):
 * what gsr_render_batch does for the colour frame, for gsr_blend_channels, gsr_blend_channels_backward and gsr_blend_gaussian_stats.
 * "Views" are n_views <= GSR_MAX_BATCH_VIEWS cameras cams[n_views] [host] of one frame size; view v works in slice v of the workspace
 * (workspace + v * S, S = gsr_workspace_bytes(n, width, height, max_pairs)), exactly as in gsr_render_batch, and every kernel of the
 * sequence is launched once for all of them.  Every view's map, final T, weights and per-slice GsrStats (gsr_read_stats on slice v)
 * are those of the single-view entry point under the same options, bit for bit.  Honoured and ignored options are
 * gsr_blend_channels'; tile-row shards with output_layout = 2 are honoured (a view's plane is then its strip), output_layout = 1 is
 * refused.
 *
 * gsr_lists_views: stages 1-2 (gsr_preprocess as with colour_stage = 0, then gsr_bin_sort) for the n_views cameras in ONE launch
 * sequence: the tile lists the three gsr_blend_*_views calls below walk.  opts->keep_flags is honoured for every slice.
 * GSR_ERR_WORKSPACE if the workspace holds fewer than n_views slices.
 *
 * The three blends run over the lists in slices 0 .. n_views - 1, as made by ONE gsr_lists_views call with the same cameras, options
 * and max_pairs (any number of blends per such call).  Strides between the views' planes are in ELEMENTS (floats; bytes for the
 * masks), at least a plane, and only read when n_views > 1:
 *   gsr_blend_channels_views           view v writes out_maps + v * map_stride ([.., channels], as gsr_blend_channels lays it out) and,
 *                                      if out_final_T is not NULL, out_final_T + v * T_stride; all views read the one `features`.
 *   gsr_blend_channels_backward_views  view v reads grad_maps + v * map_stride; ALL views add into the one grad_features:
 *                                      grad_features[i][c] += sum_v sum_p w_v,i(p) grad_maps[v][p][c].  Float atomic adds: the value
 *                                      depends on the order the adds arrive in, as for a single view.
 *   gsr_blend_gaussian_stats_views     view v reads pixel_masks + v * mask_stride (NULL: every drawn pixel of every view counts); all
 *                                      views accumulate into weight_sum / weight_max / pixels as gsr_blend_gaussian_stats does (sum of
 *                                      sums, max of maxima, sum of counts: weight_max and pixels stay exact and reproducible to the bit,
 *                                      weight_sum depends on the order the adds arrive in), and
 *                                        view_hits[i] += #{views v of this call : gaussian i has w > 0 in a counted pixel of v}
 *                                      — the number of views whose exact visible set holds the gaussian.  It is exact and does not
 *                                      depend on the order anything arrives in: the first flush of view v that reaches gaussian i
 *                                      sets bit v of view_bits[i] with an atomic OR and adds 1 only if the bit was clear.  view_bits is
 *                                      an [n] uint32 scratch of the caller's, required exactly when view_hits is given; the library
 *                                      clears it on the caller's stream before the blend, so its contents are ignored on entry and
 *                                      undefined on return.  Any of the four outputs may be NULL, not all four; an absent view_hits
 *                                      costs nothing.
 * gsr_render_channels_batch: any number n_cams of cameras, in groups of K = min(slices the workspace holds, GSR_MAX_BATCH_VIEWS,
 * opts->batch_views if set, n_cams) views as gsr_render_batch loops: per group gsr_lists_views + gsr_blend_channels_views, view i in
 * slice i % K, its map at out_maps + i * map_stride and its final T at out_final_T + i * T_stride; the slices' counters are
 * gsr_render_batch's (the LAST view rendered there, overflows sticky).  The accumulating calls have no such one-shot form: a caller
 * that adds into its buffers checks the lists first (gsr_read_stats on every slice, re-run gsr_lists_views until complete) and only
 * then blends, so that an incomplete walk never reaches them.
 * GSR_ERR_BAD_ARG, before any HIP call or look at the workspace and each with its own words: null cams, null options, n_views < 1 or
 * > GSR_MAX_BATCH_VIEWS (n_cams < 0), cameras of different frame sizes, output_layout = 1, every refusal of the single-view function,
 * a stride smaller than a view's map or plane (n_views > 1), all four statistics outputs NULL, view_hits without view_bits or
 * view_bits without view_hits. */
int gsr_lists_views(const GsrScene *scene, const GsrCamera *cams /* [host] */, int32_t n_views, const GsrOptions *opts,
                    int64_t max_pairs, void *workspace, size_t workspace_bytes, void *stream);
int gsr_blend_channels_views(int64_t n, const GsrCamera *cams /* [host] */, int32_t n_views, const GsrOptions *opts, int64_t max_pairs,
                             void *workspace, size_t workspace_bytes, const float *features, int32_t channels,
                             int64_t feature_stride, float *out_maps, int64_t map_stride, float *out_final_T /* may be NULL */,
                             int64_t T_stride, void *stream);
int gsr_blend_channels_backward_views(int64_t n, const GsrCamera *cams /* [host] */, int32_t n_views, const GsrOptions *opts,
                                      int64_t max_pairs, void *workspace, size_t workspace_bytes, const float *grad_maps,
                                      int64_t map_stride, int32_t channels, float *grad_features, int64_t grad_stride, void *stream);
int gsr_blend_gaussian_stats_views(int64_t n, const GsrCamera *cams /* [host] */, int32_t n_views, const GsrOptions *opts,
                                   int64_t max_pairs, void *workspace, size_t workspace_bytes,
                                   const uint8_t *pixel_masks /* may be NULL */, int64_t mask_stride, float *weight_sum,
                                   float *weight_max, uint32_t *pixels, uint32_t *view_hits, uint32_t *view_bits, void *stream);
int gsr_render_channels_batch(const GsrScene *scene, const GsrCamera *cams /* [host] */, int32_t n_cams, const GsrOptions *opts,
                              int64_t max_pairs, void *workspace, size_t workspace_bytes, const float *features, int32_t channels,
                              int64_t feature_stride, float *out_maps, int64_t map_stride, float *out_final_T /* may be NULL */,
                              int64_t T_stride, void *stream);

/* Totals the blend's per-workgroup counters (one small kernel on `stream`: wave_entries / fetched_entries describe the
 * LAST gsr_blend of the frame, 0 if none ran; the two totals are written into the workspace's counter block, no frame
 * data changes), copies the frame counters to host memory and waits for the stream.
 * Returns GSR_ERR_PAIR_OVERFLOW if the frame overflowed max_pairs, GSR_ERR_SORT_PASSES if depth_sort_passes was too small. */
int gsr_read_stats(void *workspace, size_t workspace_bytes, GsrStats *out /* [host] */, void *stream);

/* Scene order (no reference counterpart: the reference reads the .ply in file order, rasterize.py:353-358, and its result does not
 * depend on the storage order except for gaussians at exactly equal depth, which its unstable torch.sort leaves undefined and this
 * library draws in array-index order).  perm_out[i] = index, in the caller's arrays, of the gaussian that should be stored i-th: the
 * gaussians along a Morton curve of their means (every axis rank-quantised to 10 bits, bits interleaved, stable).  Gathering all five
 * scene arrays with it before rendering makes the same frames ~10 % faster on MI355X (culled waves, L2 hits).  Once per scene:
 * sixteen radix passes; at 6.13 M gaussians the permutation plus the caller's gather of the five arrays take 3.8 ms in a warm process
 * (the first call of a process also loads this library's code objects: 19 - 71 ms seen).  workspace: gsr_scene_order_bytes(n) bytes,
 * 256-B aligned, free afterwards. */
int gsr_scene_order_bytes(int64_t n, size_t *bytes /* [host] */);
int gsr_scene_order(int64_t n, const float *means /* [n,3] */, uint32_t *perm_out /* [n] */, void *workspace, size_t workspace_bytes,
                    void *stream);

/* Camera-independent block bounds for GsrScene.block_bounds (no reference counterpart; once per scene, after any reordering):
 * bounds_out [ceil(n / GSR_BOUNDS_BLOCK)][8] = {min x, min y, min z, max x, max y, max z, max log-scale, 0} over each block of
 * GSR_BOUNDS_BLOCK consecutive gaussians (a block with a non-finite value gets an unbounded box: never skipped). */
int gsr_scene_bounds(int64_t n, const float *means /* [n,3] */, const float *log_scales /* [n,3] */, float *bounds_out, void *stream);

/* Which blocks of scene->block_bounds does the preprocess skip for this view (and, with a tile-row shard in opts, this rank)?
 * dead_out [ceil(n / GSR_BOUNDS_BLOCK)] = 1 where no gaussian of the block can be drawn.  The test the kernels apply, exposed for
 * tests (every gaussian of a skipped block must fail the reference's own skip guard, rasterize.py:441) and for tooling. */
int gsr_block_visibility(const GsrScene *scene, const GsrCamera *cam, const GsrOptions *opts, uint8_t *dead_out, void *stream);

/* Stand-alone helpers behind the reference's helper functions (same maths as inside gsr_preprocess). */
/* sh_to_rgb, spherical_harmonics.py:27-73 */
int gsr_sh_to_rgb(int64_t n, const float *means, const float *sh, const float cam_center[3] /* [host] */, int32_t degree,
                  float *rgb_out, void *stream);
/* get_covariance_matrix_from_mesh, rasterize.py:89-120: out [n,9] */
int gsr_cov3d(int64_t n, const float *log_scales, const float *quats, float *cov3d_out, void *stream);

/* project_to_camera_space, rasterize.py:80-86: out[n,3] = means @ w2c[:3,:3] + w2c[3,:3]; w2c [host] row-major 4x4 */
int gsr_project_to_camera_space(int64_t n, const float *means, const float w2c[16] /* [host] */, float *out, void *stream);
/* compute_2d_covariance, rasterize.py:201-252: cov3d [n,9], cam_means [n,3] -> cov2d_out [n,4] (2x2 row-major).
 * tan_fov_*, focal_* are the reference's arguments as given (focals are halved inside, rasterize.py:216). */
int gsr_compute_2d_covariance(int64_t n, const float *cov3d, const float *cam_means, double tan_fov_x, double tan_fov_y,
                              double focal_x, double focal_y, const float w2c[16] /* [host] */, float *cov2d_out, void *stream);
/* compute_covering_bbox, rasterize.py:154-198: screen_means [n,2], cov2d [n,4] -> tile-unit bboxes int64 [n,4] */
int gsr_compute_covering_bbox(int64_t n, const float *screen_means, const float *cov2d, double width, double height,
                              int64_t *tile_bboxes_out, void *stream);
/* rasterize_gaussian, rasterize.py:255-305: blend ONE gaussian in place into screen [W,H,3] / opacity_buffer [W,H]
 * (the reference's x-major layout).  n = number of gaussians in the per-gaussian arrays (bounds check). */
int gsr_rasterize_gaussian(int64_t gaussian_index, int64_t n, const int64_t *bboxes, float *screen, const float *screen_means,
                           const float *sigmas, const float *rgb, float *opacity_buffer, const float *opacity, int32_t width,
                           int32_t height, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSR_H */
