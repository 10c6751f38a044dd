"""Host side of the render call: device-resident scene, camera block, workspace, frame launch.

This is the function the reference never had — its render call is the body of
`run_rasterization` (reference rasterize.py:347-446) and returns nothing; `Rasterizer.render`
returns the frame.  PyTorch only provides device memory and the stream; all per-gaussian and
per-pixel work happens in libgsr.so through the C ABI (include/gsr.h).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Mapping, NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import GsrCamera, GsrDebugOut, GsrOptions, GsrScene, GsrStats, check, lib
from .utils import pack_gaussians

TILE = 16
MAX_RETRIES = 6  # re-renders of one frame / batch after an exceeded bound (pair buffer, depth-sort passes) before giving up


def _require_cuda(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU: libgsr has no CPU path")


def _stream_ptr(device) -> int:
    return int(torch.cuda.current_stream(device).cuda_stream)


def morton_order(means: np.ndarray) -> np.ndarray:
    """Permutation that lays gaussians out along a Morton (Z-order) curve of their means: every axis rank-quantised to 10 bits (so
    the curve is balanced whatever the scene's extent), bits interleaved, stable.  A trained .ply is in no spatial order, and what
    a camera sees is a spatial region: in curve order the gaussians of a wave are neighbours, so waves are culled whole, the 192-B
    SH rows of the visible ones are contiguous (no partly used lines) and the blend's record gathers hit L2 more often."""
    n = len(means)
    if n == 0:
        return np.zeros(0, np.int64)

    def spread(v):  # 10 bits -> every third bit
        v = v.astype(np.uint64) & 0x3FF
        v = (v | (v << 16)) & 0x30000FF
        v = (v | (v << 8)) & 0x300F00F
        v = (v | (v << 4)) & 0x30C30C3
        v = (v | (v << 2)) & 0x9249249
        return v

    q = [np.argsort(np.argsort(means[:, a], kind="stable"), kind="stable") * 1024 // n for a in range(3)]
    code = spread(q[0]) | (spread(q[1]) << 1) | (spread(q[2]) << 2)
    return np.argsort(code, kind="stable")


def scene_order(means: torch.Tensor) -> torch.Tensor:
    """morton_order through the C ABI (gsr_scene_order: libgsr's own radix passes, ~2 ms at 6 M gaussians, no first-use kernel
    loading): int64 permutation on the device of `means`, element for element the numpy statement's."""
    _require_cuda(means, "means")
    n = int(means.shape[0])
    if n == 0:
        return torch.zeros(0, dtype=torch.int64, device=means.device)
    m = means.contiguous().float()
    need = C.c_size_t(0)
    check(lib.gsr_scene_order_bytes(n, C.byref(need)))
    with torch.cuda.device(means.device):
        ws = torch.empty(int(need.value), dtype=torch.uint8, device=means.device)
        perm = torch.empty(n, dtype=torch.int32, device=means.device)  # uint32 on the wire; n < 2^31
        check(lib.gsr_scene_order(n, m.data_ptr(), perm.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr(means.device)))
        return perm.to(torch.int64)


def morton_order_device(means: torch.Tensor) -> torch.Tensor:
    """morton_order with torch ops, on whatever device the means live on (CPU in the tests): the same permutation, element for
    element — per axis a stable argsort and its inverse give the ranks, the quantised ranks are interleaved into 30-bit codes, one
    more stable argsort orders them.  On the GPU the loaders use `scene_order` (the C ABI) instead: the first torch sort of a
    process costs 0.1-0.4 s of rocPRIM kernel loading."""
    n = int(means.shape[0])
    if n == 0:
        return torch.zeros(0, dtype=torch.int64, device=means.device)

    def spread(v):  # 10 bits -> every third bit
        v = v & 0x3FF
        v = (v | (v << 16)) & 0x30000FF
        v = (v | (v << 8)) & 0x300F00F
        v = (v | (v << 4)) & 0x30C30C3
        v = (v | (v << 2)) & 0x9249249
        return v

    ar = torch.arange(n, dtype=torch.int64, device=means.device)
    code = torch.zeros(n, dtype=torch.int64, device=means.device)
    for a in range(3):
        idx = torch.argsort(means[:, a].float(), stable=True)
        rank = torch.empty_like(idx)
        rank[idx] = ar
        code |= spread(rank * 1024 // n) << a
    return torch.argsort(code, stable=True)


class GaussianScene:
    """Camera-independent trained gaussians, resident in HBM in the layout of GsrScene.

    The loaders below upload the arrays along a Morton curve of the means (`spatial_order=True`, their default since round 4;
    `order` holds the permutation: scene index -> file index, None in file order).  A trained .ply is in no spatial order while a
    camera sees a spatial region: in curve order the preprocess culls whole waves, the SH rows of the visible gaussians are
    contiguous and the blend's record gathers hit L2 more often — ~10 % of the frame (bench.py's `file_order` leg).
    The frame is the same: the reference's depth sort orders the draw, not the storage order — except for gaussians at EXACTLY
    equal depth, whose mutual order the reference leaves undefined (torch.sort, rasterize.py:425, is unstable) and this library
    resolves by scene index.  Per-gaussian outputs (`Rasterizer.preprocess_debug`) come back in FILE order either way.
    The constructor takes device arrays as they are (no reordering): that is the C ABI's view."""

    FIELDS = ("means", "log_scales", "quats", "opacity_logit", "sh")

    def __init__(self, arrays: Mapping[str, torch.Tensor], sh_degree: int = 3, sh_half: bool = False):
        self.t: Dict[str, torch.Tensor] = {}
        self.bounds: Optional[torch.Tensor] = None   # GsrScene.block_bounds (build_bounds): [ceil(n / GSR_BOUNDS_BLOCK), 8] or None
        self.order_t: Optional[torch.Tensor] = None  # device, int64: scene index -> file index (None: file order)
        self._order_np: Optional[np.ndarray] = None
        self.order_ms = 0.0                          # what building the order and gathering the arrays cost at upload
        self.sh_half = bool(sh_half)
        for k in self.FIELDS:
            v = arrays[k]
            _require_cuda(v, k)
            self.t[k] = v.contiguous().half() if (k == "sh" and sh_half) else v.contiguous().float()
        self.n = int(self.t["means"].shape[0])
        self.device = self.t["means"].device
        self.sh_degree = int(sh_degree)
        shapes = {"means": (self.n, 3), "log_scales": (self.n, 3), "quats": (self.n, 4), "opacity_logit": (self.n,),
                  "sh": (self.n, 16, 3)}
        for k, shp in shapes.items():
            if tuple(self.t[k].shape) != shp:
                raise ValueError(f"{k}: expected shape {shp}, got {tuple(self.t[k].shape)}")

    @property
    def order(self) -> Optional[np.ndarray]:
        """scene index -> file index as a numpy array (None: the scene is in file order)."""
        if self.order_t is None:
            return None
        if self._order_np is None:
            self._order_np = self.order_t.cpu().numpy()
        return self._order_np

    def sort_spatially(self) -> "GaussianScene":
        """Reorder the resident arrays along the Morton curve of the means (on the device; a scene already ordered is left alone)."""
        if self.order_t is not None or self.n == 0:
            return self
        with torch.cuda.device(self.device):  # the events (and the sorts' temporaries) belong to the scene's device, whichever is current
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            order = scene_order(self.t["means"])
            for k in self.FIELDS:
                self.t[k] = self.t[k].index_select(0, order).contiguous()
            t1.record()
            t1.synchronize()
        self.order_t, self._order_np, self.order_ms = order, None, float(t0.elapsed_time(t1))
        if self.bounds is not None:  # they described the old order
            self.build_bounds()
        return self

    def blocks_skipped(self, cam: GsrCamera, opts: Optional[GsrOptions] = None) -> torch.Tensor:
        """uint8 [blocks]: 1 where the preprocess skips the block for this view (gsr_block_visibility; needs build_bounds)."""
        if self.bounds is None:
            raise ValueError("the scene has no block bounds (build_bounds)")
        opts = opts or make_options()
        sc = self.c_struct()
        with torch.cuda.device(self.device):
            dead = torch.zeros(self.bounds.shape[0], dtype=torch.uint8, device=self.device)
            check(lib.gsr_block_visibility(C.byref(sc), C.byref(cam), C.byref(opts), dead.data_ptr(), _stream_ptr(self.device)))
        return dead

    def build_bounds(self) -> "GaussianScene":
        """Camera-independent block bounds of the arrays AS THEY LIE NOW (gsr_scene_bounds: per GSR_BOUNDS_BLOCK = 64 consecutive
        gaussians the box of their means and their largest log-scale, 32 B per block): the preprocess then skips, unread, every block none
        of whose gaussians can be drawn in a view — bit-identical frames.  Pays off in spatial order (31 % of the bench frame's blocks,
        DESIGN.md §5.0); harmless in file order."""
        if self.n == 0:
            return self
        with torch.cuda.device(self.device):
            nblk = (self.n + _lib.GSR_BOUNDS_BLOCK - 1) // _lib.GSR_BOUNDS_BLOCK
            b = torch.empty((nblk, 8), dtype=torch.float32, device=self.device)
            check(lib.gsr_scene_bounds(self.n, self.t["means"].data_ptr(), self.t["log_scales"].data_ptr(), b.data_ptr(), _stream_ptr(self.device)))
        self.bounds = b
        return self

    @classmethod
    def from_columns(cls, columns, device="cuda", sh_degree: int = 3, sh_half: bool = False, spatial_order: bool = True) -> "GaussianScene":
        """`columns`: ply element / dict of float32 columns named as in the INRIA .ply."""
        return cls.from_packed(pack_gaussians(columns), device, sh_degree, sh_half, spatial_order)

    @classmethod
    def from_packed(cls, packed: Mapping[str, np.ndarray], device="cuda", sh_degree: int = 3, sh_half: bool = False,
                    spatial_order: bool = True) -> "GaussianScene":
        scene = cls({k: torch.from_numpy(np.ascontiguousarray(np.asarray(packed[k], np.float32))).to(device) for k in cls.FIELDS},
                    sh_degree, sh_half)
        # block bounds pay in spatial order (31 % of the bench frame's blocks are skipped unread); in file order no box is tight enough
        # to rule a block out and the flags kernel would run for nothing
        return scene.sort_spatially().build_bounds() if spatial_order else scene

    @classmethod
    def from_ply(cls, path: str, device="cuda", sh_degree: int = 3, sh_half: bool = False, spatial_order: bool = True) -> "GaussianScene":
        from .ply import PlyData

        return cls.from_columns(PlyData.read(path), device, sh_degree, sh_half, spatial_order)

    def c_struct(self) -> GsrScene:
        s = GsrScene()
        s.n = self.n
        for k in self.FIELDS:
            setattr(s, k, self.t[k].data_ptr())
        s.sh_degree = self.sh_degree
        s.sh_dtype = 1 if self.sh_half else 0
        s.block_bounds = self.bounds.data_ptr() if self.bounds is not None else None
        return s


def make_camera(qvec, tvec, fx_full: float, fy_full: float, cam_width: int, cam_height: int, width: int, height: int) -> GsrCamera:
    """COLMAP pose + full-res intrinsics + frame size -> GsrCamera (reference rasterize.py:336-345,:361-364)."""
    return _lib.camera_setup(qvec, tvec, fx_full, fy_full, cam_width, cam_height, width, height)


def make_options(reference_compat: bool = True, early_out_T: float = 0.0, tile_row_begin: int = 0, tile_row_step: int = 1,
                 output_layout: int = 0, no_footprint_cull: bool = False, blend_impl: int = 0, draw_limit: int = 0,
                 output_bf16: bool = False, depth_sort_passes: int = 0, keep_flags: bool = False, accum_bf16: bool = False,
                 saturation_rule: int = 0, fine_binning: bool = False, shard_preprocess: int = 0, blend_pipe_tiles: int = 0,
                 sh_dense_min: int = 0, colour_stage: int = 0, no_order_hint: bool = False, batch_views: int = 0,
                 tile_row_block: int = 0) -> GsrOptions:
    o = _lib.default_options()
    o.reference_compat = 1 if reference_compat else 0
    o.early_out_T = float(early_out_T)
    o.tile_row_begin = int(tile_row_begin)
    o.tile_row_step = int(tile_row_step)
    o.output_layout = int(output_layout)
    o.no_footprint_cull = 1 if no_footprint_cull else 0
    o.blend_impl = int(blend_impl)
    o.draw_limit = int(draw_limit)
    o.output_dtype = 1 if output_bf16 else 0  # frame stored as bfloat16; accumulation stays fp32
    o.depth_sort_passes = int(depth_sort_passes)  # 0: no bound (Rasterizer.render / render_batch fill in what the frames' counters have taught them)
    o.accum_dtype = 1 if accum_bf16 else 0        # configs[2] as worded: bf16 accumulators (measurement option, plain-C kernel)
    o.keep_flags = 1 if keep_flags else 0         # Rasterizer.enqueue sets it itself for the frames after the first since the last stats()
    o.saturation_rule = int(saturation_rule)      # 0: a quadrant stops once its colour cannot change (exact); 1: once T == 0.0f (the A/B reference)
    o.fine_binning = 1 if fine_binning else 0     # A/B switches (same frames): per-tile pairs; 1/2 = whole-frame / three-phase shard
    o.shard_preprocess = int(shard_preprocess)    # preprocess; tile bound of the pipelined blend walk (-1 = never); dense-wave SH threshold
    o.blend_pipe_tiles = int(blend_pipe_tiles)
    o.sh_dense_min = int(sh_dense_min)
    o.no_order_hint = 1 if no_order_hint else 0   # blend launch order by list length alone (default: by what each tile staged last frame)
    o.colour_stage = int(colour_stage)            # 0: sh_to_rgb when a tile first stages the gaussian (blend); 1: for every visible gaussian (preprocess)
    o.batch_views = int(batch_views)              # render_batch: at most this many views per launch sequence (0: as many as the workspace has slices)
    o.tile_row_block = int(tile_row_block)        # tile-row shards: 0 / 1 = single rows interleave, 2 = pairs of rows (whole 32x32 cell rows)
    return o


def shard_row_list(height: int, begin: int, step: int, block: int = 1):
    """The tile rows a tile-row shard owns, ascending = its strip rows (GsrOptions.tile_row_begin / _step / _block: blocks of `block`
    consecutive tile rows, block b is the shard's when b % step == begin)."""
    tiles_y = (height + TILE - 1) // TILE
    block = 2 if block == 2 else 1
    return [t for t in range(tiles_y) if (t // block) % max(step, 1) == (begin if step > 1 else 0)]


def shard_rows(height: int, begin: int, step: int, block: int = 1) -> int:
    return len(shard_row_list(height, begin, step, block))


class UncheckedFrames:
    """Which slices of a Rasterizer's workspace hold frames that no stats() has read yet.  A call renders into slices 0 .. k-1
    (enqueue: slice 0; enqueue_batch: one per view of a launch sequence), so these are always the first `slices`.  libgsr keeps an
    overflow record per slice: a slice's first frame since the last stats() starts a new one, later frames add to it (keep_flags)."""

    def __init__(self):
        self.slices = 0      # slices 0 .. slices - 1 hold unchecked frames
        self.empty = False   # the last enqueue was a shard without tile rows: no kernel ran, its counters are all zero

    def to_reset(self, k: int) -> range:
        """Slices a call into 0 .. k-1 resets first: when slice 0 holds unchecked frames the call keeps every slice's record, so
        those of its slices that hold none start from an empty one (stats() leaves the record it read in the slice)."""
        return range(self.slices, k) if self.slices else range(0)

    def wrote(self, k: int) -> None:
        """A call rendered into slices 0 .. k-1 (k = 0: an empty shard)."""
        self.slices, self.empty = max(self.slices, k), k == 0

    def read(self) -> int:
        """stats() reads slices 0 .. read() - 1: the unchecked ones, else slice 0 once more (none after an empty shard); the record starts over."""
        n = self.slices if self.empty else max(self.slices, 1)
        self.slices = 0
        return n


def _render_checked(rasterizers, streams, opts: GsrOptions, attempt, slack_div: int, what: str):
    """The retry loop of Rasterizer.render / render_batch and FramesInFlight.render_batch: `attempt(o)` enqueues the frames with
    options `o`, then each rasterizer with anything to report runs stats() on its stream (None: the current one).  They share their
    bounds: a frame over the pair bound grows all pair buffers to the worst need (+ 1 / slack_div); one short of depth-sort passes
    re-runs with the learned bound, or with every pass once the need reported is no higher than what was enqueued.  The caller's own
    depth_sort_passes is re-raised; after MAX_RETRIES re-renders so is the last attempt's status (pair overflow before sort passes)."""
    r0, unbounded = rasterizers[0], False
    for _ in range(MAX_RETRIES + 1):
        for r in rasterizers:  # a depth-sort bound one of them has learned holds for all
            r.sort_passes = max(q.sort_passes for q in rasterizers)
        o = opts if unbounded else r0.bounded(opts)
        frames = attempt(o)
        failed = []
        for r, s in zip(rasterizers, streams):
            if r.unchecked.slices or r.unchecked.empty:
                with torch.cuda.stream(s):
                    try:
                        r.stats()
                    except (_lib.GsrPairOverflow, _lib.GsrSortPasses) as e:
                        failed.append((e, r.last_stats))
        if not failed:
            return frames
        short = [e for e, _ in failed if isinstance(e, _lib.GsrSortPasses)]
        if short and opts.depth_sort_passes != 0:
            raise short[0]  # the caller's own bound
        need = max([st["n_pairs_bbox"] for e, st in failed if isinstance(e, _lib.GsrPairOverflow)], default=0)
        if need >= _lib.GSR_MAX_PAIRS:
            raise _lib.GsrError(_lib.GSR_ERR_PAIR_OVERFLOW, f"a frame needs {need} pairs, more than libgsr can index")
        if need:
            grown = int(min(_lib.GSR_MAX_PAIRS, need + need // slack_div + 1024))
            if grown <= r0.max_pairs:
                raise _lib.GsrError(_lib.GSR_ERR_PAIR_OVERFLOW, f"pair overflow persists at max_pairs = {r0.max_pairs} (need {need})")
            for r in rasterizers:
                r.max_pairs = grown
        if short:  # stats() has raised the learned bound to the need
            unbounded = o.depth_sort_passes >= max(r.sort_passes for r in rasterizers)
    e, st = max(failed, key=lambda f: isinstance(f[0], _lib.GsrPairOverflow))
    raise type(e)(e.code, f"{what} still incomplete after {MAX_RETRIES} re-renders: {st}")


def _check_tensor(name: str, t, shape, dtype=None, device=None, layout: str = "contiguous", note: str = "") -> None:
    """The one check of a caller's tensor argument: `name` must be a [contiguous] `dtype` tensor of shape `shape` on `device` (the
    scene's).  shape: per dimension an int, or (lo, hi) for lo <= size <= hi (hi None: no upper limit).  dtype: one, a tuple of
    them, or None (any: the call converts).  layout: "contiguous"; "rows" — rows (of a batch: frames) contiguous in themselves and
    at least their own length apart, which libgsr takes with a stride; "any" — the call copies if it has to.  ValueError naming
    the argument, what was expected and what came."""
    dtypes = () if dtype is None else dtype if isinstance(dtype, tuple) else (dtype,)

    def refusal(got: str) -> ValueError:  # (worded only when something is refused: the calls are on every frame's path)
        kind = ("contiguous " if layout == "contiguous" else "") + " or ".join(str(d)[6:] for d in dtypes) + (" " if dtypes else "")
        dims = ", ".join(str(s) if isinstance(s, int) else f"{s[0]}..{'' if s[1] is None else s[1]}" for s in shape)
        rows = ", its rows contiguous and at least their length apart" if layout == "rows" else ""
        return ValueError(f"{name} must be a {kind}tensor of shape [{dims}]{note}{rows}, got {got}")

    if not isinstance(t, torch.Tensor):
        raise refusal(type(t).__name__)
    fits = t.dim() == len(shape) and all(z == s if isinstance(s, int) else s[0] <= z and (s[1] is None or z <= s[1])
                                         for z, s in zip(t.shape, shape))
    if not fits or (dtypes and t.dtype not in dtypes):
        raise refusal(f"{t.dtype} {tuple(t.shape)}")
    if device is not None and t.device != device:
        raise ValueError(f"{name} must live on the scene's device ({device}), got {t.device}")
    if layout == "rows" and t.numel():  # (a single row is any distance from the next)
        laid_out = t.stride(-1) == 1 and t[0].is_contiguous() and (t.shape[0] == 1 or t.stride(0) >= t[0].numel())
    else:
        laid_out = layout == "any" or t.is_contiguous()
    if not laid_out:
        raise refusal(f"strides {tuple(t.stride())}")


def file_order_gradient(buf: torch.Tensor, order_t: Optional[torch.Tensor]) -> torch.Tensor:
    """A per-gaussian gradient in the scene's order -> in the order of the file the scene was loaded from: the transpose of the
    gather `rows = features.index_select(0, order_t)` (row j of the scene is row order_t[j] of the file).  order_t=None: the scene
    kept the file's order and `buf` itself is returned.  Works on CPU and GPU tensors."""
    if order_t is None:
        return buf
    return torch.empty_like(buf).index_copy_(0, order_t, buf)


def file_order_ids(ids: torch.Tensor, order_t: Optional[torch.Tensor]) -> torch.Tensor:
    """A map of gaussian ids in the scene's order (indices into its resident arrays, -1 = none) -> the same map with ids of the
    file the scene was loaded from: id j becomes order_t[j], -1 stays -1.  order_t=None: the scene kept the file's order and `ids`
    itself is returned.  Works on CPU and GPU tensors."""
    if order_t is None:
        return ids
    file_ids = order_t.to(ids.dtype)[ids.clamp(min=0).long()]
    return torch.where(ids < 0, ids, file_ids)


class _PerGaussianOut:
    """The result side of a call that sums per-gaussian values over a view's pixels.  fields: per buffer (name
    of the caller's tensor for it, shape behind [n], dtype, wanted).  `out` — the caller's tensors, one per field, in the SCENE's
    order — is checked first, before any buffer is made; a field that is not wanted is not looked at and stays None.  With `out`
    the call adds into the caller's tensors and answers with them; else into buffers of its own, which come back in the file's
    order unless scene_order.  zeroed: nothing else clears own buffers (False: _accumulate_view does, on every attempt)."""

    def __init__(self, scene: "GaussianScene", fields, out, scene_order: bool, zeroed: bool, layout: str = "contiguous"):
        n, dev = scene.n, scene.device
        if isinstance(out, torch.Tensor):  # a call with one field takes the tensor itself
            out = (out,)
        if out is not None:
            if len(out) != len(fields):
                raise ValueError(f"out must hold a tensor (or None) for each of {', '.join(f[0] for f in fields)}, got {len(out)}")
            for (name, shape, dtype, wanted), t in zip(fields, out):
                if wanted:
                    _check_tensor(name, t, (n,) + tuple(shape), dtype, dev, layout)
            self.bufs = [t if f[3] else None for f, t in zip(fields, out)]
        else:
            new = torch.zeros if zeroed else torch.empty
            self.bufs = [new((n,) + tuple(shape), dtype=dtype, device=dev) if wanted else None for _, shape, dtype, wanted in fields]
        self.ptrs = [b.data_ptr() if b is not None else None for b in self.bufs]    # None for a field that is not wanted
        self.own = None if out is not None else [b for b in self.bufs if b is not None]  # what _accumulate_view clears
        self._order_t = None if out is not None or scene_order else scene.order_t

    def result(self) -> list:
        """The tensors to return, one per field: the caller's own objects, or this call's in the order that was asked for."""
        return [None if b is None else file_order_gradient(b, self._order_t) for b in self.bufs]


def _wanted(want, names) -> tuple:
    """`want`, a sequence of names out of `names`, as one flag per name."""
    if isinstance(want, str) or not all(isinstance(w, str) for w in want):
        raise ValueError(f"want must be a sequence of names from {names}, got {want!r}")
    if not len(want) or any(w not in names for w in want):
        raise ValueError(f"want must name at least one of {names} and nothing else, got {tuple(want)!r}")
    return tuple(name in want for name in names)


class PickMaps(NamedTuple):
    """Rasterizer.render_pick: per pixel the gaussian of largest blend weight and that weight, the gaussian after which T first
    falls below median_T, and (count=True) how many gaussians contributed.  Ids are int32, -1 = none."""
    best_id: torch.Tensor
    best_w: torch.Tensor
    median_id: torch.Tensor
    count: Optional[torch.Tensor]


class TopK(NamedTuple):
    """Rasterizer.render_topk: per pixel the k heaviest (or nearest) gaussians and their blend weights.  ids: int32 [H, W, k], -1 =
    unused slot; weights: float32 [H, W, k], 0 with -1; final_T: float32 [H, W], or None when it was not asked for."""
    ids: torch.Tensor
    weights: torch.Tensor
    final_T: Optional[torch.Tensor]


class ViewStats(NamedTuple):
    """Rasterizer.view_stats: per gaussian, over the counted pixels of a view (or of several), the sum of its blend weights
    (float32), the largest weight it reaches in any pixel (float32) and the number of pixels it reaches with w > 0 (int32).  [n]
    tensors; a field that was not asked for is None."""
    weight_sum: Optional[torch.Tensor]
    weight_max: Optional[torch.Tensor]
    pixels: Optional[torch.Tensor]


VIEW_STATS = ("sum", "max", "pixels")  # the names `want` takes, in ViewStats' field order
# ... and what view_stats / view_stats_batch add them up in: ViewStats' fields, then the batch's view count (_PerGaussianOut's fields)
_STATS_FIELDS = (("out.weight_sum", (), torch.float32), ("out.weight_max", (), torch.float32), ("out.pixels", (), torch.int32),
                 ("out's views", (), torch.int32))


class SplatGradient(NamedTuple):
    """Rasterizer.splat_gradient: per gaussian, the gradient of L = <grad_map, map> + <grad_T, final T> with respect to what the
    preprocess computes for it (preprocess_debug's names).  mean2d [n, 2]: d L / d screen_means, in 1 / pixel (multiply by W / 2,
    H / 2 for the NDC norm 3DGS densifies by); sigmas [n, 3]: d L / d (s0, s1, s2), the inverse 2-D covariance; opacity [n]:
    d L / d opacity (opacity_logit_gradient chains it to the logit); abs_mean2d [n, 2]: the per-pixel absolute values of the two
    mean terms, summed (the AbsGS densification statistic), or None when it was not asked for.  All float32."""
    mean2d: torch.Tensor
    sigmas: torch.Tensor
    opacity: torch.Tensor
    abs_mean2d: Optional[torch.Tensor]


def opacity_logit_gradient(scene: "GaussianScene", g: SplatGradient, scene_order: bool = False) -> torch.Tensor:
    """[n]: d L / d opacity_logit = g.opacity * o (1 - o) with o = sigmoid(opacity_logit), the chain through the activation the
    preprocess applies.  `g` in the file's order (scene_order=True: in the order of the scene's resident arrays, as it was asked
    for)."""
    x = scene.t["opacity_logit"]
    chain = torch.sigmoid(x) * torch.sigmoid(-x)  # o (1 - o) without the cancellation of 1 - o (at logit 12, 1 - o = 6e-6)
    if not scene_order:
        chain = file_order_gradient(chain, scene.order_t)
    return g.opacity * chain


class GeometryGradient(NamedTuple):
    """project_backward / Rasterizer.geometry_gradient: per gaussian, the gradient with respect to what the scene stores, laid out
    like its arrays — means [n, 3], log_scales [n, 3], quats [n, 4] (w, x, y, z as stored, not normalised), opacity_logit [n].
    All float32; a field that was left out of `out` is None."""
    means: Optional[torch.Tensor]
    log_scales: Optional[torch.Tensor]
    quats: Optional[torch.Tensor]
    opacity_logit: Optional[torch.Tensor]


def _geometry_out(scene: "GaussianScene", out: Optional[GeometryGradient], scene_order: bool) -> _PerGaussianOut:
    """The four tensors a projection backward adds into: new zeroed ones (no entry clears them), or those of `out` that are not
    None, once they are what it takes."""
    if out is not None and (len(out) != 4 or all(b is None for b in out)):
        raise ValueError("out must be a GeometryGradient with at least one tensor")
    fields = [(f"out.{name}", shape, torch.float32, out is None or out[k] is not None)
              for k, (name, shape) in enumerate(zip(GeometryGradient._fields, ((3,), (3,), (4,), ())))]
    return _PerGaussianOut(scene, fields, out, scene_order, zeroed=True)


def _project_backward_into(scene: "GaussianScene", cam: GsrCamera, opts: GsrOptions, splat_rows: torch.Tensor, ptrs) -> None:
    """One gsr_project_backward on the scene's stream: added into the four outputs that are not None."""
    sc = scene.c_struct()
    with torch.cuda.device(scene.device):
        check(lib.gsr_project_backward(C.byref(sc), C.byref(cam), C.byref(opts), splat_rows.data_ptr(), *ptrs, _stream_ptr(scene.device)))


def project_backward(scene: "GaussianScene", cam: GsrCamera, splat_rows: torch.Tensor, opts: Optional[GsrOptions] = None,
                     out: Optional[GeometryGradient] = None, scene_order: bool = False) -> GeometryGradient:
    """The splat gradient of a view chained through the preprocess' projection to the scene's own parameters
    (gsr_project_backward): one pass, one thread per gaussian, the forward recomputed in fp32 from the preprocess' expressions.
    splat_rows: [n, 8] float32 contiguous on the scene's device, in the SCENE's order, columns (opacity, mean x, y, s0, s1, s2, -,
    -) as splat_gradient(out=) fills them; columns 6 and 7 are ignored.  A row of six zeros is skipped: the gaussian's gradients are
    not touched.  Gaussians the view culls (z_cam < 0.2), or whose 2-D covariance is singular, contribute nothing whatever their row
    holds.  Held fixed: the tile rect, the footprint, the 1/255 threshold and the cull; where the ray clamp is active the derivative
    in x / z is 0.  No colour term in this call: the SH view direction's part of d / d mean is sh_backward's, which adds it into the
    same `means` (Rasterizer.colour_gradient runs both).
    Returns a GeometryGradient in the order of the file the scene was loaded from (scene_order=True: of the scene's resident
    arrays).  With `out` — a GeometryGradient of float32 contiguous tensors on the scene's device, in the SCENE's order; a field that
    is None is not computed — the gradient is ACCUMULATED into its tensors and `out` is returned: summing over a camera set needs
    no temporary.  No atomics: two calls give the same bits.
    The scene's arrays are read, never written.  A caller that steps a resident scene's tensors in place must rebuild what was
    derived from them: the block bounds (GaussianScene.build_bounds()), and the Morton order goes stale as the means move."""
    _require_cuda(splat_rows, "splat_rows")
    _check_tensor("splat_rows", splat_rows, (scene.n, 8), torch.float32, scene.device)
    res = _geometry_out(scene, out, scene_order)
    if scene.n:
        _project_backward_into(scene, cam, opts or make_options(), splat_rows, res.ptrs)
    return out if out is not None else GeometryGradient(*res.result())


class ColourGradient(NamedTuple):
    """sh_backward: per gaussian, the gradient with respect to its SH coefficients, sh [n, 16, 3] (float32 also where the scene
    stores them as float16: the gradient in the widened values), and the part of the gradient with respect to its mean that comes
    through the view direction, means [n, 3].  A field that was left out of `out` is None."""
    sh: Optional[torch.Tensor]
    means: Optional[torch.Tensor]


class SceneGradient(NamedTuple):
    """Rasterizer.colour_gradient: per gaussian, the gradient with respect to every array the scene stores, each laid out like
    that array — means [n, 3], log_scales [n, 3], quats [n, 4] (w, x, y, z as stored), opacity_logit [n], sh [n, 16, 3].  All
    float32; a field that was left out of `out` is None."""
    means: Optional[torch.Tensor]
    log_scales: Optional[torch.Tensor]
    quats: Optional[torch.Tensor]
    opacity_logit: Optional[torch.Tensor]
    sh: Optional[torch.Tensor]


_SCENE_SHAPES = {"means": (3,), "log_scales": (3,), "quats": (4,), "opacity_logit": (), "sh": (16, 3)}


def _gradient_out(scene: "GaussianScene", kind, out, scene_order: bool) -> _PerGaussianOut:
    """The tensors a ColourGradient or a SceneGradient (`kind`) is added into: new zeroed ones (no entry clears them), or those of
    `out` that are not None, once they are what it takes."""
    if out is not None and (len(out) != len(kind._fields) or all(b is None for b in out)):
        raise ValueError(f"out must be a {kind.__name__} with at least one tensor")
    fields = [(f"out.{name}", _SCENE_SHAPES[name], torch.float32, out is None or out[k] is not None)
              for k, name in enumerate(kind._fields)]
    return _PerGaussianOut(scene, fields, out, scene_order, zeroed=True)


def _sh_backward_into(scene: "GaussianScene", cam: GsrCamera, grad_rgb: torch.Tensor, sh_ptr, means_ptr) -> None:
    """One gsr_sh_backward on the scene's stream: grad_rgb's rows where they lie, into the outputs that are not None."""
    sc = scene.c_struct()
    stride = int(grad_rgb.stride(0)) if grad_rgb.shape[0] > 1 else int(grad_rgb.shape[1])  # (a single row is any distance from the next)
    with torch.cuda.device(scene.device):
        check(lib.gsr_sh_backward(C.byref(sc), C.byref(cam), grad_rgb.data_ptr(), stride, sh_ptr, means_ptr, _stream_ptr(scene.device)))


def sh_backward(scene: "GaussianScene", cam: GsrCamera, grad_rgb: torch.Tensor, out: Optional[ColourGradient] = None,
                scene_order: bool = False) -> ColourGradient:
    """The gradient of a view's per-gaussian colours carried to the SH coefficients and, through the view direction, to the means
    (gsr_sh_backward): the exact transpose of sh_to_rgb at the scene's degree and this camera's centre, one pass, one thread per
    gaussian, no cull (sh_to_rgb has none).  grad_rgb: [n, C >= 3] float32 on the scene's device, in the SCENE's order, unit element
    stride, rows at least C apart; columns 0-2 are read where they lie (a column window of a wider tensor included).  The clamp of
    the colour to [0, 1] has derivative 0 where it is active and 1 on its edges; the decision is the forward's own.  A row of three
    zeros is skipped: the gaussian's gradients are not touched.  Coefficients beyond the scene's degree get nothing, and at degree 0
    the means get nothing.
    Returns a ColourGradient in the order of the file the scene was loaded from (scene_order=True: of the scene's resident arrays).
    With `out` — a ColourGradient of float32 contiguous tensors on the scene's device, in the SCENE's order; a field that is None is
    not computed — the gradient is ACCUMULATED into its tensors and `out` is returned.  No atomics: two calls give the same bits."""
    _require_cuda(grad_rgb, "grad_rgb")
    _check_tensor("grad_rgb", grad_rgb, (scene.n, (3, None)), torch.float32, scene.device, "rows")
    res = _gradient_out(scene, ColourGradient, out, scene_order)
    if scene.n:
        _sh_backward_into(scene, cam, grad_rgb, *res.ptrs)
    return out if out is not None else ColourGradient(*res.result())


class CameraGradient(NamedTuple):
    """camera_backward / Rasterizer.camera_gradient: the gradient with respect to the GsrCamera fields as the kernels read them —
    w2c [4, 4], full_proj [4, 4], focal [2] = (focal_x, focal_y), cam_center [3] — and `contributing` (0-d), the exact number of
    gaussians that contributed a splat term.  float64 tensors on the scene's device, all views of ONE buffer (nothing has
    synchronised); the entries the forward never reads (column 3 of w2c, column 2 of full_proj) are 0.  pose_gradient chains them to
    a twist and a log-focal step."""
    w2c: torch.Tensor
    full_proj: torch.Tensor
    focal: torch.Tensor
    cam_center: torch.Tensor
    contributing: torch.Tensor


def _camera_gradient_of(buf: torch.Tensor) -> CameraGradient:
    """The [32] doubles gsr_camera_backward wrote, laid out as the struct's fields: slot 3 k + j is w2c[k][j] (j < 3), slot
    12 + 3 k + jj is full_proj[k][(0, 1, 3)[jj]]; the columns the forward never reads are zeros.  Slice copies on the device into
    ONE buffer, of which the five fields are views: no index tensor, no sync."""
    out = torch.zeros(38, dtype=torch.float64, device=buf.device)
    w2c, proj, src = out[0:16].view(4, 4), out[16:32].view(4, 4), buf[12:24].view(4, 3)
    w2c[:, :3] = buf[0:12].view(4, 3)
    proj[:, 0:2] = src[:, 0:2]
    proj[:, 3] = src[:, 2]
    out[32:38] = buf[24:30]
    return CameraGradient(w2c, proj, out[32:34], out[34:37], out[37])


def _camera_workspace(scene: "GaussianScene", keep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The partial sums' workspace of gsr_camera_backward for this scene (`keep` itself when it already is one)."""
    nbytes = int(lib.gsr_camera_backward_bytes(scene.n))
    if keep is not None and keep.numel() == nbytes and keep.device == scene.device:
        return keep
    return torch.empty(nbytes, dtype=torch.uint8, device=scene.device)


def _camera_backward_into(scene: "GaussianScene", cam: GsrCamera, opts: GsrOptions, splat_ptr, view_ptr, ws: torch.Tensor) -> CameraGradient:
    """One gsr_camera_backward on the scene's stream into a new [32] float64 buffer."""
    buf = torch.empty(32, dtype=torch.float64, device=scene.device)
    sc = scene.c_struct()
    with torch.cuda.device(scene.device):
        check(lib.gsr_camera_backward(C.byref(sc), C.byref(cam), C.byref(opts), splat_ptr, view_ptr, buf.data_ptr(), ws.data_ptr(), ws.numel(),
                                      _stream_ptr(scene.device)))
    return _camera_gradient_of(buf)


def camera_backward(scene: "GaussianScene", cam: GsrCamera, splat_rows: Optional[torch.Tensor] = None,
                    view_mean_rows: Optional[torch.Tensor] = None, opts: Optional[GsrOptions] = None) -> CameraGradient:
    """The splat gradient of a view summed into the gradient with respect to the CAMERA (gsr_camera_backward): the bare operator
    on arrays in the SCENE's order.  splat_rows: [n, 8] float32 contiguous on the scene's device, columns (opacity, mean x, y, s0,
    s1, s2, -, -) as splat_gradient(out=) fills them — the array project_backward reads, under its rules: a row of six zeros is
    skipped, gaussians the view culls or whose 2-D covariance is singular contribute nothing, the derivative in x / z is 0 where the
    ray clamp is active; held fixed are the tile rect, the footprint, the 1/255 threshold, the cull, the depth order and lim_x /
    lim_y.  view_mean_rows: [n, 3] float32 contiguous, the view-direction term of d L / d mean that sh_backward leaves in `means`
    when it is called alone; its negated column sum is d L / d cam_center.  Either may be None, not both.
    Returns a CameraGradient of float64 tensors on the device.  The per-gaussian terms are float32, every sum across gaussians is a
    double sum in a fixed order: no atomics, two calls give the same bits."""
    if splat_rows is None and view_mean_rows is None:
        raise ValueError("camera_backward needs splat_rows, view_mean_rows or both")
    for name, t, cols in (("splat_rows", splat_rows, 8), ("view_mean_rows", view_mean_rows, 3)):
        if t is not None:
            _require_cuda(t, name)
            _check_tensor(name, t, (scene.n, cols), torch.float32, scene.device)
    if scene.n == 0:  # nothing to sum (an empty tensor has no address to hand to the library)
        return _camera_gradient_of(torch.zeros(32, dtype=torch.float64, device=scene.device))
    return _camera_backward_into(scene, cam, opts or make_options(), splat_rows.data_ptr() if splat_rows is not None else None,
                                 view_mean_rows.data_ptr() if view_mean_rows is not None else None, _camera_workspace(scene))


def pose_gradient(cam: GsrCamera, cg: CameraGradient):
    """(twist [6], log_focal [2]), float64 CPU tensors: a CameraGradient's raw partials chained to the six parameters of a rigid
    motion of the camera in its own frame and to the logs of the two focal lengths — what a pose or focal optimiser steps in.  The
    twist xi = (omega, v) moves the camera by x_cam' = x_cam + omega x x_cam + v + O(|xi|^2): w2c' = w2c E(xi) in the row-vector
    convention (E[:3, :3] = exp([omega]x)^T, E[3, :3] = v), full_proj' = w2c' (w2c^-1 full_proj) with the projection matrix
    unchanged, cam_center' = inverse(w2c')[3, :3].  log_focal[0] = focal_x cg.focal[0] + sum_k full_proj[4 k] cg.full_proj[k][0]:
    column 0 of full_proj is proportional to fx; lim_x is held fixed; y likewise with column 1.  Chained in float64 from the
    struct's own values.  This is the one place that synchronises (it reads cg)."""
    f64 = torch.float64
    V = torch.tensor(list(cam.w2c), dtype=f64).view(4, 4)
    F = torch.tensor(list(cam.full_proj), dtype=f64).view(4, 4)
    dV, dF, dfoc, dcc = (t.detach().to("cpu", f64) for t in (cg.w2c, cg.full_proj, cg.focal, cg.cam_center))
    Vinv = torch.linalg.inv(V)
    GE = V.T @ dV + V.T @ dF @ (Vinv @ F).T  # d L / d E at E = I
    A = GE[:3, :3]
    # d E[:3, :3] / d omega_k = -[e_k]x: <A, -[e_k]x>
    omega = torch.stack([A[1, 2] - A[2, 1], A[2, 0] - A[0, 2], A[0, 1] - A[1, 0]])
    v = GE[3, :3] - Vinv[:3, :3] @ dcc  # d cam_center = -(dE V^-1)[3, :3]
    log_focal = torch.stack([cam.focal_x * dfoc[0] + (F[:, 0] * dF[:, 0]).sum(), cam.focal_y * dfoc[1] + (F[:, 1] * dF[:, 1]).sum()])
    return torch.cat([omega, v]), log_focal


TOPK_SELECT = {"heaviest": _lib.GSR_TOPK_HEAVIEST, "nearest": _lib.GSR_TOPK_NEAREST}


def topk_composite(topk: TopK, features: torch.Tensor) -> torch.Tensor:
    """[H, W, C] = sum_j weights[..., j] * features[ids[..., j]], slots with id -1 contributing 0: the sparse approximation of
    render_features(cam, features) from a pixel's k listed gaussians, for any C.  `features`: [n, C] on the lists' device, rows in
    the order the ids index (the file's, unless the lists were rendered with scene_order=True).  Plain torch: differentiable in
    `features` through autograd; not a kernel, and not bit for bit any blend's sum.  Memory: one [H, W, C] gather per slot (autograd
    keeps the k index maps and weight planes, not the gathers)."""
    ids, weights = topk.ids, topk.weights
    if features.dim() != 2:
        raise ValueError(f"features must be [n, C], got {tuple(features.shape)}")
    out = None
    for j in range(ids.shape[-1]):  # slot by slot: the largest temporary is [H, W, C], not [H, W, k, C]
        idj = ids[..., j]
        wj = torch.where(idj >= 0, weights[..., j], torch.zeros_like(weights[..., j])).to(features.dtype)
        term = wj.unsqueeze(-1) * features[idj.clamp(min=0).long()]
        out = term if out is None else out + term
    return out


def composite_over(map: torch.Tensor, T: torch.Tensor, background: torch.Tensor) -> torch.Tensor:
    """map + T[..., None] * background: what a blend leaves of whatever lies behind it.  `map` is [H, W, C] with its final
    transmittance `T` [H, W] (render(..., return_T=True), render_features, render_slab); `background` is [C] (one colour) or
    [H, W, C] (a frame: the mesh render behind the splats, the next depth layer).  Plain torch, one multiply-add per element in the
    map's dtype; differentiable in all three; works on CPU and GPU tensors."""
    if map.dim() != 3 or tuple(T.shape) != tuple(map.shape[:2]):
        raise ValueError(f"map must be [H, W, C] and T [H, W], got {tuple(map.shape)} and {tuple(T.shape)}")
    background = torch.as_tensor(background, dtype=map.dtype, device=map.device)
    if tuple(background.shape) not in ((map.shape[2],), tuple(map.shape)):
        raise ValueError(f"background must be [{map.shape[2]}] or {tuple(map.shape)}, got {tuple(background.shape)}")
    return map + T.to(map.dtype).unsqueeze(-1) * background


class _RenderFeatures(torch.autograd.Function):
    """render_features as a differentiable function of the features alone: the map is linear in them, so the backward is the
    transpose under the same camera and options (Rasterizer.feature_gradient); nothing flows to the geometry or the opacities."""

    @staticmethod
    def forward(ctx, features, rasterizer, cam, opts, return_T, scene_order):
        ctx.rasterizer, ctx.scene_order = rasterizer, scene_order
        ctx.cam = GsrCamera.from_buffer_copy(cam)
        ctx.opts = GsrOptions.from_buffer_copy(opts or make_options())
        res = rasterizer._render_features(cam, features.detach(), opts, return_T, scene_order)
        if return_T:
            ctx.mark_non_differentiable(res[1])
        return res

    @staticmethod
    def backward(ctx, grad_out, *_):
        g = ctx.rasterizer.feature_gradient(ctx.cam, grad_out, ctx.opts, scene_order=ctx.scene_order)
        return g, None, None, None, None, None


class _RenderFeaturesBatch(torch.autograd.Function):
    """render_features_batch as a differentiable function of the features alone: ONE node for all views, whose backward is
    Rasterizer.feature_gradient_batch under the same cameras and options (the views' gradients summed by the kernel)."""

    @staticmethod
    def forward(ctx, features, rasterizer, cams, opts, return_T, scene_order):
        ctx.rasterizer, ctx.scene_order = rasterizer, scene_order
        ctx.cams = [GsrCamera.from_buffer_copy(c) for c in cams]
        ctx.opts = GsrOptions.from_buffer_copy(opts or make_options())
        res = rasterizer._render_features_batch(cams, features.detach(), opts, return_T, scene_order)
        if return_T:
            ctx.mark_non_differentiable(res[1])
        return res

    @staticmethod
    def backward(ctx, grad_out, *_):
        g = ctx.rasterizer.feature_gradient_batch(ctx.cams, grad_out, ctx.opts, scene_order=ctx.scene_order)
        return g, None, None, None, None, None


VIEW_STATS_BATCH = VIEW_STATS + ("views",)  # the names view_stats_batch's `want` takes: ViewStats' fields, then the view count


# render_features: maps of more channels than this go through gsr_render_channels (many channels per walk of the tile lists), the
# others through the three-channel blend.  DESIGN.md §5.11 has the measurement the rule rests on.
WIDE_BLEND_ABOVE = 3


class Rasterizer:
    """Owns the scratch workspace for one scene and renders frames of it.

    `views` > 1 makes the workspace that many slices (each a complete one-view workspace, gsr_workspace_bytes): render_batch /
    enqueue_batch then put `views` cameras at a time through ONE launch sequence of libgsr (gsr_render_batch: one preprocess that
    reads the scene once for all of them, one set of sorts, one blend — a quarter of the dispatches per frame at views = 4, each four
    times better filled).  Frames are bit-identical to single-view renders.  Single frames (render / enqueue) use slice 0."""

    def __init__(self, scene: GaussianScene, max_pairs: Optional[int] = None, views: int = 1):
        self.scene = scene
        self.views = max(1, min(int(views), _lib.GSR_MAX_BATCH_VIEWS))
        self.max_pairs = min(_lib.GSR_MAX_PAIRS, int(max_pairs) if max_pairs else max(1 << 20, 8 * scene.n))
        # radix passes the depth sort of this scene's frames has needed so far (GsrStats.sort_passes, learned whenever the counters
        # are read): passed as GsrOptions.depth_sort_passes so that the passes a frame does not need are not even enqueued
        self.sort_passes = 0
        self._ws: Optional[torch.Tensor] = None
        self._ws_key = None
        self._slice = 0            # bytes per slice of the workspace
        self.unchecked = UncheckedFrames()
        self.last_stats: Optional[Dict[str, int]] = None
        self.last_slice_stats: list = []   # stats() per slice: the last view each slice rendered
        self._splat_rows: Optional[torch.Tensor] = None  # geometry_gradient's [n, 8] scratch, zeroed on every call
        self._colour_rows: Optional[torch.Tensor] = None  # colour_gradient's [n, 4] scratch (d L / d colour), zeroed on every call
        self._view_mean_rows: Optional[torch.Tensor] = None  # camera_gradient's [n, 3] scratch (the view direction's d L / d mean)
        self._camera_ws: Optional[torch.Tensor] = None  # camera_gradient's workspace of partial sums (gsr_camera_backward_bytes)

    # -- workspace ------------------------------------------------------------------------------
    def _workspace(self, width: int, height: int) -> torch.Tensor:
        key = (self.scene.n, width, height, self.max_pairs, self.views)
        if self._ws is None or self._ws_key != key:
            nbytes = _lib.workspace_bytes(self.scene.n, width, height, self.max_pairs)
            self._ws = None  # free the old one first
            self._ws = torch.empty(nbytes * self.views, dtype=torch.uint8, device=self.scene.device)
            assert self._ws.data_ptr() % 256 == 0 and nbytes % 256 == 0
            self._ws_key, self._slice = key, nbytes
            self.unchecked = UncheckedFrames()
            self._reset_slices(range(self.views))
        return self._ws

    def _reset_slices(self, slices: range) -> None:
        """Zero the head of these slices (libgsr needs no initialisation): an empty overflow record for a frame rendered with keep_flags,
        and zeros for a gsr_read_stats before any frame has run there rather than whatever the allocator left."""
        for v in slices:
            self._ws[v * self._slice: v * self._slice + min(4096, self._slice)].zero_()

    def _views_per_launch(self, opts: GsrOptions, n_cams: int) -> int:
        """Views per launch sequence of gsr_render_batch, view j in slice j: api.hip views_per_launch for this workspace."""
        k = min(self.views, opts.batch_views) if opts.batch_views > 0 else self.views
        return min(k, max(n_cams, 1))

    def _out_shape(self, cam: GsrCamera, opts: GsrOptions):
        if opts.output_layout == 0:
            return (cam.height, cam.width, 3), (cam.height, cam.width)
        if opts.output_layout == 1:
            return (cam.width, cam.height, 3), (cam.width, cam.height)
        rows = shard_rows(cam.height, opts.tile_row_begin, opts.tile_row_step, opts.tile_row_block) * TILE
        return (rows, cam.width, 3), (rows, cam.width)

    def bounded(self, opts: Optional[GsrOptions] = None) -> GsrOptions:
        """opts with the learned depth-sort bound filled in (a copy), unless the caller set one.  render() / render_batch()
        apply it themselves (they check every frame and re-render); for enqueue() / FramesInFlight.submit() the caller opts
        in with this — the frames are then unchecked until the next stats(), which reports ANY of them that exceeded it."""
        opts = opts or make_options()
        if opts.depth_sort_passes != 0 or self.sort_passes == 0:
            return opts
        o = GsrOptions.from_buffer_copy(opts)
        o.depth_sort_passes = self.sort_passes
        return o

    # -- the host skeleton of every single-view call ---------------------------
    def _new(self, opts: GsrOptions, shape, dtype=torch.float32, fill=None) -> torch.Tensor:
        """An output of a single-view call.  fill=None: a map the blend stores whole, except that strips (output_layout == 2) may
        hold rows below the frame's last pixel row, which are kept defined (0).  Else the value that reads "nothing drawn" (0; -1 for
        an id; 1 for T), everywhere."""
        if fill is None:
            return (torch.zeros if opts.output_layout == 2 else torch.empty)(shape, dtype=dtype, device=self.scene.device)
        return torch.full(shape, fill, dtype=dtype, device=self.scene.device)

    def _chained(self, opts: GsrOptions) -> GsrOptions:
        """Slice 0 holds unchecked frames: a single view adds to their record (keep_flags; a copy, the caller's struct is never
        written).  Batches have a rule of their own (_enqueue_group), FramesInFlight.render_batch clears the flag on purpose."""
        if not self.unchecked.slices or opts.keep_flags:
            return opts
        o = GsrOptions.from_buffer_copy(opts)
        o.keep_flags = 1
        return o

    def _enqueue_view(self, cam: GsrCamera, opts: GsrOptions, entry, result: Optional[torch.Tensor], *args) -> Optional[GsrOptions]:
        """One gsr_render_* entry (all share the prefix scene, cam, opts, max_pairs, workspace; `args` lie between it and the stream)
        into slice 0 on the current stream, unchecked like enqueue().  The workspace comes first: one of a new size resets
        `unchecked`.  A `result` without elements is a shard that owns no tile row (more ranks than tile rows): nothing is called
        and None returned; else the options the entry ran with."""
        ws = self._workspace(cam.width, cam.height)
        if result is not None and result.numel() == 0:
            self.unchecked.wrote(0)
            return None
        opts, sc = self._chained(opts), self.scene.c_struct()
        check(entry(C.byref(sc), C.byref(cam), C.byref(opts), self.max_pairs, ws.data_ptr(), ws.numel(), *args, _stream_ptr(self.scene.device)))
        self.unchecked.wrote(1)
        return opts

    def _stages_1_2(self, sc, cam, opts, max_pairs, ws, ws_bytes, stream) -> int:
        """gsr_preprocess then gsr_bin_sort, with the parameters and the status of a gsr_render_* entry."""
        return lib.gsr_preprocess(sc, cam, opts, ws, ws_bytes, None, stream) or \
            lib.gsr_bin_sort(self.scene.n, cam, opts, max_pairs, ws, ws_bytes, stream)

    def _enqueue_lists(self, cam: GsrCamera, opts: GsrOptions, result: Optional[torch.Tensor] = None) -> Optional[GsrOptions]:
        """Stages 1-2 alone, as _enqueue_view enqueues a whole view: the tile lists the gsr_blend_* entries walk (_blend_lists) with
        the options returned here."""
        return self._enqueue_view(cam, opts, self._stages_1_2, result)

    def _blend_lists(self, cam: GsrCamera, opts: GsrOptions, entry, *args) -> None:
        """One gsr_blend_* entry (prefix n, cam, opts, max_pairs, workspace) over the lists in slice 0.  The workspace is asked for
        again: _render_checked may have grown max_pairs since the caller last saw it."""
        ws = self._workspace(cam.width, cam.height)
        check(entry(self.scene.n, C.byref(cam), C.byref(opts), self.max_pairs, ws.data_ptr(), ws.numel(), *args, _stream_ptr(self.scene.device)))

    def _checked_lists(self, cam: GsrCamera, opts: GsrOptions, what: str) -> GsrOptions:
        """The first phase of a call that ACCUMULATES into the caller's buffers.  An incomplete walk must never reach them — what it
        added could not be taken back — so stages 1-2 are enqueued, checked and re-run until they are complete (_render_checked), with
        colour_stage = 0 as the gsr_render_* entries of these blends set it; only then does the caller's gsr_blend_* add, once, with
        the options returned here."""
        def attempt(o):
            o = GsrOptions.from_buffer_copy(o)
            o.colour_stage = 0
            return self._enqueue_lists(cam, o)

        return _render_checked([self], [None], opts, attempt, 8, what)

    def _accumulate_view(self, cam: GsrCamera, opts: GsrOptions, what: str, own, render_entry, blend_entry, *args) -> None:
        """A single view's per-gaussian sums into the buffers whose addresses stand in `args`, the arguments both entries take
        between the workspace and the stream.  own = the buffers when they are this call's: zeroed on every attempt, then ONE
        gsr_render_X under _render_checked — an incomplete walk is thrown away with them.  own = None, the caller's buffers:
        _checked_lists first, then one gsr_blend_X that adds."""
        if own is None:
            o = self._checked_lists(cam, opts, what)
            self._blend_lists(cam, o, blend_entry, *args)
            return

        def attempt(o):  # a re-run after an overflow starts from zero again
            for b in own:
                b.zero_()
            self._enqueue_view(cam, o, render_entry, None, *args)

        _render_checked([self], [None], opts, attempt, 8, what)

    # -- one frame ------------------------------------------------------------------------------
    def enqueue(self, cam: GsrCamera, opts: Optional[GsrOptions] = None, out: Optional[torch.Tensor] = None,
                final_T: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Enqueue one frame on the current stream with `opts` as given; no host synchronisation and no check of the
        caller's bounds (max_pairs; opts.depth_sort_passes if set).  The frames enqueued since the last stats() are chained
        with GsrOptions.keep_flags, so the next stats() / render() reports a bound exceeded by ANY of them, not only the last."""
        opts = opts or make_options()
        shape, _ = self._out_shape(cam, opts)
        dtype = torch.bfloat16 if opts.output_dtype == 1 else torch.float32
        if out is None:
            out = self._new(opts, shape, dtype)
        else:
            _check_tensor("out", out, shape, dtype, self.scene.device)
        self._enqueue_view(cam, opts, lib.gsr_render_forward, out, out.data_ptr(), final_T.data_ptr() if final_T is not None else None)
        return out

    def stats(self) -> Dict[str, int]:
        """Counters of the last enqueued frame (synchronises the stream; zeros for a shard without tile rows).  Reads every slice
        that holds frames enqueued since the previous stats() and raises GsrPairOverflow / GsrSortPasses if one exceeded a bound:
        then, also after an empty shard, last_stats holds the worst slice's figures and last_slice_stats every slice read."""
        per, worst_rc = [], 0
        for v in range(self.unchecked.read() if self._ws is not None else 0):
            st = GsrStats()
            rc = lib.gsr_read_stats(self._ws.data_ptr() + v * self._slice, self._slice, C.byref(st), _stream_ptr(self.scene.device))
            per.append(st.as_dict())
            self.sort_passes = max(self.sort_passes, int(st.sort_passes))  # also when a frame was short of passes: the retry has them
            if rc == _lib.GSR_ERR_PAIR_OVERFLOW or (rc != 0 and worst_rc != _lib.GSR_ERR_PAIR_OVERFLOW):
                worst_rc = rc
        zeros = not per or (self.unchecked.empty and not worst_rc)  # nothing read, or an empty shard behind frames that were fine
        self.last_slice_stats = [{k: 0 for k, _ in GsrStats._fields_ if not k.startswith("_")}] if zeros else per
        self.last_stats = dict(self.last_slice_stats[0])
        if worst_rc:  # what a re-render needs: the worst slice's figures
            self.last_stats = dict(per[0], n_pairs_bbox=max(d["n_pairs_bbox"] for d in per), sort_passes=max(d["sort_passes"] for d in per))
            for d in per:
                self.last_stats["overflow"] |= d["overflow"]
        check(worst_rc)
        return self.last_stats

    def render(self, cam: GsrCamera, opts: Optional[GsrOptions] = None, out: Optional[torch.Tensor] = None,
               return_T: bool = False):
        """Render one frame and verify it is complete: grows the pair buffer / raises the learned depth-sort bound and
        re-renders when the frame exceeded one (_render_checked).  Frames enqueued before this one and not yet checked share
        its overflow record: if one of THEM exceeded a bound, this frame is re-rendered once with room for it."""
        def attempt(o):
            final_T = torch.ones(self._out_shape(cam, o)[1], dtype=torch.float32, device=self.scene.device) if return_T else None
            img = self.enqueue(cam, o, out, final_T)
            return (img, final_T) if return_T else img

        return _render_checked([self], [None], opts or make_options(), attempt, 8, "frame")

    # -- feature, depth and alpha maps -----------------------------------------------------------------
    def _check_features(self, features: torch.Tensor, max_channels: Optional[int] = None) -> None:
        _require_cuda(features, "features")
        _check_tensor("features", features, (self.scene.n, (1, None)), torch.float32, self.scene.device, "any")
        if max_channels is not None and features.shape[1] > max_channels:
            raise ValueError(f"at most {max_channels} channels per call, got {features.shape[1]}")

    def _feature_triple(self, features: torch.Tensor, scene_order: bool) -> torch.Tensor:
        """[n, C <= 3] caller values -> one contiguous [n, 3] float32 array in the scene's order, zero-padded: what the three-channel
        blend reads (wider maps go through _feature_rows and gsr_render_channels, WIDE_BLEND_ABOVE)."""
        self._check_features(features)
        n, n_ch = self.scene.n, int(features.shape[1])
        assert n_ch <= 3
        if n == 0:  # an empty tensor has no address; libgsr refuses a null array
            return torch.zeros((1, 3), dtype=torch.float32, device=self.scene.device)
        if not scene_order and self.scene.order_t is not None:
            features = features.index_select(0, self.scene.order_t)
        if n_ch < 3:
            features = torch.cat([features, torch.zeros((n, 3 - n_ch), dtype=torch.float32, device=self.scene.device)], 1)
        return features.contiguous()

    def _depth_features(self, cam: GsrCamera) -> torch.Tensor:
        """[n, 3] = (z_cam, 1, 0) in the scene's order; z_cam = column 2 of gsr_project_to_camera_space for the camera's w2c."""
        n, dev = self.scene.n, self.scene.device
        f = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        if n:
            pc = torch.empty((n, 3), dtype=torch.float32, device=dev)
            check(lib.gsr_project_to_camera_space(n, self.scene.t["means"].data_ptr(), cam.w2c, pc.data_ptr(), _stream_ptr(dev)))
            f[:, 0] = pc[:, 2]
            f[:, 1] = 1.0
        return f

    def _enqueue_maps(self, cam: GsrCamera, opts: GsrOptions, triple: torch.Tensor, want_T: bool):
        """One preprocess, one bin / sort and the three-channel feature blend (gsr_render_features) on the current stream, unchecked
        like enqueue().  Returns (map, T or None)."""
        shape, tshape = self._out_shape(cam, opts)
        out = self._new(opts, shape)
        T = self._new(opts, tshape, fill=1) if want_T else None
        self._enqueue_view(cam, opts, lib.gsr_render_features, out, triple.data_ptr(), out.data_ptr(), T.data_ptr() if want_T else None)
        return out, T

    def _enqueue_rgbd(self, cam: GsrCamera, opts: GsrOptions, triple: torch.Tensor):
        """One preprocess and one bin / sort, then the colour blend with the caller's options (the frame may be bf16) and one feature
        blend over the same lists, on the current stream, unchecked like enqueue().  Returns (image, map)."""
        shape, _ = self._out_shape(cam, opts)
        img = self._new(opts, shape, torch.bfloat16 if opts.output_dtype == 1 else torch.float32)
        out = self._new(opts, shape)
        opts = self._enqueue_lists(cam, opts, out)
        if opts is not None:
            sc = self.scene.c_struct()
            fo = GsrOptions.from_buffer_copy(opts)  # the map is float32 whatever the frame is stored as
            fo.output_dtype = 0
            self._blend_lists(cam, opts, lambda *a: lib.gsr_blend(C.byref(sc), *a), img.data_ptr(), None)
            self._blend_lists(cam, fo, lib.gsr_blend_features, triple.data_ptr(), out.data_ptr(), None)
        return img, out

    def _feature_rows(self, features: torch.Tensor, scene_order: bool) -> torch.Tensor:
        """[n, C] caller values -> a float32 tensor in the scene's order that gsr_render_channels reads where it lies: rows of unit
        element stride, stride(0) >= C apart.  The caller's own tensor (a column window of a wider one included) whenever it already
        is in the scene's order and laid out so; else ONE copy (the gather through scene.order_t, or .contiguous())."""
        self._check_features(features, _lib.GSR_MAX_FEATURE_CHANNELS)
        if self.scene.n == 0:  # an empty tensor has no address; libgsr refuses a null array
            return torch.zeros((1, features.shape[1]), dtype=torch.float32, device=self.scene.device)
        if not scene_order and self.scene.order_t is not None:
            return features.index_select(0, self.scene.order_t)
        if features.stride(1) == 1 and features.stride(0) >= features.shape[1]:
            return features
        return features.contiguous()

    def _enqueue_channels(self, cam: GsrCamera, opts: GsrOptions, rows: torch.Tensor, want_T: bool, limits=None):
        """One preprocess, one bin / sort and one gsr_blend_channels (gsr_render_channels) on the current stream, unchecked like
        enqueue(): the [.., C] map is written in place, no group copies.  With limits = (near, far), planes or None, gsr_blend_slab
        (gsr_render_slab) instead.  Returns (map, T or None)."""
        shape, tshape = self._out_shape(cam, opts)
        n_ch = int(rows.shape[1])
        out = self._new(opts, shape[:2] + (n_ch,))
        T = self._new(opts, tshape, fill=1) if want_T else None
        entry, planes = lib.gsr_render_channels, ()
        if limits is not None:
            entry, planes = lib.gsr_render_slab, tuple(p.data_ptr() if p is not None else None for p in limits)
        self._enqueue_view(cam, opts, entry, out, rows.data_ptr(), n_ch, int(rows.stride(0)), *planes, out.data_ptr(),
                           T.data_ptr() if want_T else None)
        return out, T

    def render_features(self, cam: GsrCamera, features: torch.Tensor, opts: Optional[GsrOptions] = None, return_T: bool = False,
                        scene_order: bool = False):
        """Composite the caller's per-gaussian values with the colour frame's weights: out[p] = sum_i w_i(p) features[i], w_i = alpha_i T_i
        over the same depth-ordered lists (gsr_render_features / gsr_blend_features).  features: [n, C] float32 on the scene's device,
        C >= 1, indexed like the file the scene was loaded from (scene_order=True: like the scene's resident arrays).  Returns
        [H, W, C] (layouts as render()), and the final transmittance [H, W] with return_T.  One preprocess and one bin / sort, then
        for C <= 3 one three-channel blend (gsr_render_features), for C > 3 gsr_render_channels: up to 16 channels per walk of the
        tile lists, read from the caller's tensor without a copy when scene_order=True and its rows have unit element stride
        (column windows of a wider tensor included), written straight into the [.., C] map.  Every channel is bit for bit what it is
        as a map of its own.  Checked and re-rendered on overflow like render().  Values are not clamped; they must be finite.
        Differentiable in `features`: when they require a gradient (and grad mode is on) the map carries a grad_fn whose backward
        is feature_gradient() under the same camera and options; the values are those of the detached tensor, bit for bit, and T
        is not differentiable.  No gradient flows to the scene."""
        if features.requires_grad and torch.is_grad_enabled():
            return _RenderFeatures.apply(features, self, cam, opts, return_T, scene_order)
        return self._render_features(cam, features, opts, return_T, scene_order)

    def _render_features(self, cam: GsrCamera, features: torch.Tensor, opts: Optional[GsrOptions], return_T: bool, scene_order: bool):
        if features.dim() == 2 and features.shape[1] > WIDE_BLEND_ABOVE:
            rows = self._feature_rows(features, scene_order)

            def attempt_wide(o):
                out, T = self._enqueue_channels(cam, o, rows, return_T)
                return (out, T) if return_T else out

            return _render_checked([self], [None], opts or make_options(), attempt_wide, 8, "feature map")
        triple = self._feature_triple(features, scene_order)
        n_ch = int(features.shape[1])

        def attempt(o):
            out, T = self._enqueue_maps(cam, o, triple, return_T)
            out = out if n_ch == 3 else out[..., :n_ch].contiguous()
            return (out, T) if return_T else out

        return _render_checked([self], [None], opts or make_options(), attempt, 8, "feature map")

    # -- the gradient of a feature map with respect to the features -------------------------------------------------------------
    def _gradient_request(self, cam: GsrCamera, opts: GsrOptions, grad_map: torch.Tensor, out, scene_order: bool, in_one_view: bool,
                          name: str = "grad_map", lead=()):
        """feature_gradient's argument checks (feature_gradient_batch's: name="grad_maps", lead=(B,), any of the cameras), before any
        workspace or buffer is made: (the map, contiguous float32 — None when there is nothing to draw; the [n, C] result, whose
        own buffer is zeros unless one view's _accumulate_view is going to clear it)."""
        _require_cuda(grad_map, name)
        want = tuple(lead) + tuple(self._out_shape(cam, opts)[0][:2])
        _check_tensor(name, grad_map, want + ((1, _lib.GSR_MAX_FEATURE_CHANNELS),), None, self.scene.device, "any")
        # nothing to draw, or a shard that owns no tile row: the gradient is zero.  Here and in view_stats no workspace is made for
        # that and the shard leaves no mark in `unchecked`, unlike the map calls (_enqueue_view).
        drawn = self.scene.n != 0 and grad_map.numel() != 0
        res = _PerGaussianOut(self.scene, [("out", (int(grad_map.shape[-1]),), torch.float32, True)], out, scene_order,
                              zeroed=not (drawn and in_one_view), layout="rows")
        return (grad_map.detach().to(torch.float32).contiguous() if drawn else None), res

    def feature_gradient(self, cam: GsrCamera, grad_map: torch.Tensor, opts: Optional[GsrOptions] = None,
                         out: Optional[torch.Tensor] = None, scene_order: bool = False) -> torch.Tensor:
        """The transpose of render_features under the same camera and options: [n, C] with row i = sum_p w_i(p) grad_map[p]
        (gsr_render_channels_backward; every C >= 1 goes through it).  grad_map: [H, W, C] as render_features lays the map out
        (made contiguous float32), finite.  Returned in the order of the file the scene was loaded from (scene_order=True: of the
        scene's resident arrays).  With `out` — [n, C] float32 on the scene's device, in the SCENE's order, unit element stride, rows
        at least C apart — the gradient is ACCUMULATED into `out` and `out` is returned: summing over a batch of views needs no
        temporary.  Stages 1-2 are re-run on every call and checked like any frame; float atomic sums may differ in the last bits
        between two calls."""
        opts = opts or make_options()
        gm, res = self._gradient_request(cam, opts, grad_map, out, scene_order, True)
        if gm is not None:
            buf = res.bufs[0]
            self._accumulate_view(cam, opts, "feature gradient", res.own, lib.gsr_render_channels_backward,
                                  lib.gsr_blend_channels_backward, gm.data_ptr(), int(buf.shape[1]), buf.data_ptr(), int(buf.stride(0)))
        return res.result()[0]

    # -- the gradient of a feature map with respect to opacity and the 2-D splat ----------------------------------------------------
    def _upstream(self, cam: GsrCamera, opts: GsrOptions, name: str, grad_map: torch.Tensor, channels: int, grad_T, min_T: float):
        """The upstream arguments of splat_gradient, colour_gradient and camera_gradient (each has looked at where the map lives),
        checked in this order — the map against the frame's shape with `channels`, grad_T, min_T — and handed back detached, float32
        and contiguous: (gm, gt or None); (None, None) when there is nothing to draw or the shard owns no tile row: no copy is made."""
        shape, tshape = self._out_shape(cam, opts)
        _check_tensor(name, grad_map, tuple(shape[:2]) + (channels,), None, self.scene.device, "any")
        if grad_T is not None:
            _check_tensor("grad_T", grad_T, tshape, None, self.scene.device, "any", " (the layout of the final T)")
        if not (float(min_T) >= 0.0 and float(min_T) < float("inf")):
            raise ValueError(f"min_T must be finite and >= 0, got {min_T}")
        if not (self.scene.n and grad_map.numel()):
            return None, None
        return (grad_map.detach().to(torch.float32).contiguous(),
                grad_T.detach().to(torch.float32).contiguous() if grad_T is not None else None)

    def splat_gradient(self, cam: GsrCamera, features: torch.Tensor, grad_map: torch.Tensor, grad_T: Optional[torch.Tensor] = None,
                       opts: Optional[GsrOptions] = None, min_T: float = 0.0, abs_mean: bool = False,
                       out: Optional[torch.Tensor] = None, scene_order: bool = False) -> SplatGradient:
        """The gradient of L = <grad_map, render_features(cam, features)> + <grad_T, final T> with respect to every gaussian's
        opacity, 2-D mean and inverse 2-D covariance — preprocess_debug's opacity, screen_means and sigmas — under the same camera
        and options (gsr_render_splat_backward).  The weights, lists and stop rule are the forward's; the support of a splat (its
        footprint, the 1/255 threshold) is held fixed and the alpha cap at 0.99 has derivative 0.  features: [n, C] as
        render_features takes them (scene_order applies to them and to the result); grad_map: [H, W, C] as render_features lays the
        map out; grad_T: [H, W] in the layout of the final T, or None.  All finite, float32.
        Units: means are in pixels, so mean2d is per pixel; multiply by W / 2, H / 2 for the NDC norm of 3DGS's densification.
        abs_mean=True also sums the per-pixel absolute values of the two mean terms (AbsGS); C <= 16 then (they are not linear in
        the channels).  min_T > 0: a pair whose incoming transmittance is below it contributes nothing of its own.
        Accuracy: what lies behind a gaussian in a pixel is formed as the pixel's total minus a running sum, which carries an
        absolute error of about 2^-24 |total| alpha / (1 - alpha) per pixel; a gaussian seen only through T <~ 1e-6 gets a gradient
        that is tiny but relatively meaningless.  min_T and opts.early_out_T are the remedies.
        Returns a SplatGradient in the order of the file the scene was loaded from (scene_order=True: of the scene's resident
        arrays).  With `out` — [n, 8] float32 contiguous on the scene's device, in the SCENE's order, columns (opacity, mean x, y,
        s0, s1, s2, |mean x|, |mean y|) — the gradient is ACCUMULATED into `out` (columns 6 and 7 only with abs_mean) and the
        SplatGradient returned holds views of it, in the scene's order: stages 1-2 are checked and re-run first and only then does
        the blend add.  Float atomic sums may differ in the last bits between two calls."""
        opts = opts or make_options()
        self._check_features(features, _lib.GSR_MAX_FEATURE_CHANNELS)
        n_ch = int(features.shape[1])
        _require_cuda(grad_map, "grad_map")
        gm, gt = self._upstream(cam, opts, "grad_map", grad_map, n_ch, grad_T, min_T)
        if abs_mean and n_ch > 16:
            raise ValueError(f"abs_mean takes at most 16 channels (the absolute sums are not linear in them), got {n_ch}")
        drawn = gm is not None  # else nothing to draw, or a shard that owns no tile row
        res = _PerGaussianOut(self.scene, [("out", (8,), torch.float32, True)], out, scene_order, zeroed=not drawn)
        if drawn:
            rows = self._feature_rows(features.detach(), scene_order)
            self._accumulate_view(cam, opts, "splat gradient", res.own, lib.gsr_render_splat_backward, lib.gsr_blend_splat_backward,
                                  rows.data_ptr(), int(rows.stride(0)), n_ch, gm.data_ptr(), gt.data_ptr() if gt is not None else None,
                                  float(min_T), int(bool(abs_mean)), *res.ptrs)
        g = res.result()[0]
        return SplatGradient(g[:, 1:3], g[:, 3:6], g[:, 0], g[:, 6:8] if abs_mean else None)

    # -- the gradient of a feature map with respect to the scene's geometry ---------------------------------------------------------
    def geometry_gradient(self, cam: GsrCamera, features: torch.Tensor, grad_map: torch.Tensor, grad_T: Optional[torch.Tensor] = None,
                          opts: Optional[GsrOptions] = None, min_T: float = 0.0, out: Optional[GeometryGradient] = None,
                          scene_order: bool = False) -> GeometryGradient:
        """The gradient of L = <grad_map, render_features(cam, features)> + <grad_T, final T> with respect to every gaussian's mean,
        log-scales, quaternion and opacity logit: splat_gradient (checked and re-run like any frame) into an [n, 8] scratch kept on
        this Rasterizer and zeroed on every call, then project_backward under the same camera and options.  Arguments as
        splat_gradient's (scene_order applies to the features and to the result); what is held fixed and the clamp rule are
        project_backward's.  The features are the caller's, so nothing flows through the SH evaluation here: colour_gradient is the
        call that differentiates the colour frame, SH term included.  Returns a GeometryGradient in the file's order (scene_order=True: the scene's).  With
        `out` (project_backward's: tensors in the SCENE's order, None = not computed) the view's gradient is ACCUMULATED into it, as
        feature_gradient(out=) does: a camera set is one call per view.  The splat gradient's float atomic sums may differ in the
        last bits between two calls; the projection adds nothing to that."""
        if out is not None:
            _geometry_out(self.scene, out, scene_order)  # refused before the splat gradient runs, not after
        rows = self._zeroed_scratch("_splat_rows", 8)
        self.splat_gradient(cam, features, grad_map, grad_T, opts, min_T, abs_mean=False, out=rows, scene_order=scene_order)
        return project_backward(self.scene, cam, rows, opts, out, scene_order)

    # -- the gradient of the colour frame with respect to everything the scene stores ---------------------------------------------------
    def _zeroed_scratch(self, name: str, cols: int) -> torch.Tensor:
        """An [n, cols] float32 scratch kept on this Rasterizer under `name`, zeroed."""
        buf = getattr(self, name, None)
        if buf is None or tuple(buf.shape) != (self.scene.n, cols):
            buf = torch.empty((self.scene.n, cols), dtype=torch.float32, device=self.scene.device)
            setattr(self, name, buf)
        return buf.zero_()

    def _gradient_rows(self, cam: GsrCamera, opts: GsrOptions, what: str, feats: torch.Tensor, gm: torch.Tensor, gt, min_T: float, colour: bool):
        """A view's gradient rows over ONE pair of stages 1-2, checked and re-run like any frame: with `colour` the feature gradient of
        the three-channel map (gsr_blend_channels_backward) into the zeroed [n, 4] scratch `_colour_rows`, then the splat gradient
        under the features `feats` (gsr_blend_splat_backward) into the zeroed [n, 8] scratch `_splat_rows`.  (colour rows or None,
        splat rows)."""
        g_rgb = self._zeroed_scratch("_colour_rows", 4) if colour else None
        rows = self._zeroed_scratch("_splat_rows", 8)
        o = self._checked_lists(cam, opts, what)
        if colour:
            self._blend_lists(cam, o, lib.gsr_blend_channels_backward, gm.data_ptr(), 3, g_rgb.data_ptr(), 4)
        self._blend_lists(cam, o, lib.gsr_blend_splat_backward, feats.data_ptr(), int(feats.stride(0)), int(feats.shape[1]), gm.data_ptr(),
                          gt.data_ptr() if gt is not None else None, float(min_T), 0, rows.data_ptr())
        return g_rgb, rows

    def colour_gradient(self, cam: GsrCamera, grad_image: torch.Tensor, grad_T: Optional[torch.Tensor] = None,
                        opts: Optional[GsrOptions] = None, min_T: float = 0.0, out: Optional[SceneGradient] = None,
                        scene_order: bool = False) -> SceneGradient:
        """The gradient of L = <grad_image, render(cam)> + <grad_T, final T> with respect to every array the scene stores: means,
        log-scales, quaternions, opacity logits and SH coefficients.  The view's colours (gsr_sh_to_rgb) are the features of the
        feature blend; ONE pair of stages 1-2, checked and re-run like any frame, then over those same lists the feature gradient
        (gsr_blend_channels_backward, d L / d colour) and the splat gradient (gsr_blend_splat_backward), each into a scratch kept on
        this Rasterizer ([n, 4] and [n, 8], zeroed on every call); then project_backward, then sh_backward, which adds the view
        direction's term into the same `means`.  grad_image: [H, W, 3] as render() lays the frame out (made contiguous float32);
        grad_T: [H, W] in the layout of the final T, or None; min_T as splat_gradient's.  All finite.
        Held fixed: what splat_gradient and project_backward hold fixed (the tile rect, the footprint, the 1/255 threshold, the cull;
        the alpha cap and the ray clamp have derivative 0 where they are active), and the colour clamp to [0, 1]: derivative 0 where
        it is active, 1 on its edges.
        Returns a SceneGradient in the file's order (scene_order=True: the scene's).  With `out` — a SceneGradient of float32
        contiguous tensors on the scene's device, in the SCENE's order; a field that is None is not computed — the view's gradient
        is ACCUMULATED into it, as geometry_gradient(out=) does: a camera set is one call per view.  The blends' float atomic sums
        may differ in the last bits between two calls; the projection and the SH transpose add nothing to that."""
        opts = opts or make_options()
        scene = self.scene
        _require_cuda(grad_image, "grad_image")
        gm, gt = self._upstream(cam, opts, "grad_image", grad_image, 3, grad_T, min_T)
        res = _gradient_out(scene, SceneGradient, out, scene_order)  # refused before anything runs, not after
        if gm is not None:  # else nothing to draw, or a shard that owns no tile row: the gradient is zero
            g_rgb, rows = self._gradient_rows(cam, opts, "colour gradient", self._view_colours(cam), gm, gt, min_T, colour=True)
            if any(p is not None for p in res.ptrs[:4]):
                _project_backward_into(scene, cam, opts, rows, res.ptrs[:4])
            if res.ptrs[4] is not None or (res.ptrs[0] is not None and scene.sh_degree > 0):
                _sh_backward_into(scene, cam, g_rgb, res.ptrs[4], res.ptrs[0])
        return out if out is not None else SceneGradient(*res.result())

    # -- the gradient of a frame or of a feature map with respect to the camera -----------------------------------------------------------
    def camera_gradient(self, cam: GsrCamera, grad_image: torch.Tensor, grad_T: Optional[torch.Tensor] = None,
                        opts: Optional[GsrOptions] = None, min_T: float = 0.0, features: Optional[torch.Tensor] = None,
                        scene_order: bool = False) -> CameraGradient:
        """The gradient of L = <grad_image, render(cam)> + <grad_T, final T> with respect to the CAMERA: w2c, full_proj, the focal
        lengths and cam_center, as a CameraGradient (pose_gradient chains it to a twist and a log-focal step).  colour_gradient's
        sequence: the view's colours as the features, ONE pair of stages 1-2, checked and re-run like any frame; over those lists
        gsr_blend_channels_backward ([n, 4] scratch) and gsr_blend_splat_backward ([n, 8] scratch); above degree 0 gsr_sh_backward
        with no grad_sh into a zeroed [n, 3] scratch — the view direction's term, whose negated sum is d L / d cam_center; then ONE
        gsr_camera_backward.  With `features` ([n, C] as render_features takes them; scene_order applies to them) grad_image is the
        [H, W, C] upstream of render_features(cam, features), as in geometry_gradient, and nothing flows through the SH evaluation:
        cam_center gets 0.  grad_T: [H, W] in the layout of the final T, or None; min_T as splat_gradient's.  All finite.
        Held fixed: what colour_gradient holds fixed, and the depth order and lim_x / lim_y.  The scratches and the partial sums'
        workspace are kept on this Rasterizer.  The blends' float atomic sums may differ in the last bits between two calls; the
        camera reduction adds nothing to that (double sums in a fixed order)."""
        opts = opts or make_options()
        scene = self.scene
        _require_cuda(grad_image, "grad_image")
        if features is not None:
            self._check_features(features, _lib.GSR_MAX_FEATURE_CHANNELS)
        gm, gt = self._upstream(cam, opts, "grad_image", grad_image, 3 if features is None else int(features.shape[1]), grad_T, min_T)
        self._camera_ws = _camera_workspace(scene, getattr(self, "_camera_ws", None))
        if gm is None:  # nothing to draw, or a shard that owns no tile row: the gradient is zero
            return _camera_gradient_of(torch.zeros(32, dtype=torch.float64, device=scene.device))
        feats = self._view_colours(cam) if features is None else self._feature_rows(features.detach(), scene_order)
        g_rgb, rows = self._gradient_rows(cam, opts, "camera gradient", feats, gm, gt, min_T, colour=features is None)
        view_rows = None
        if features is None and scene.sh_degree > 0:
            view_rows = self._zeroed_scratch("_view_mean_rows", 3)
            _sh_backward_into(scene, cam, g_rgb, None, view_rows.data_ptr())
        return _camera_backward_into(scene, cam, opts, rows.data_ptr(), view_rows.data_ptr() if view_rows is not None else None, self._camera_ws)

    def blend_weights(self, cam: GsrCamera, opts: Optional[GsrOptions] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[n]: every gaussian's blend weight summed over the drawn pixels of this view, sum_p w_i(p) — feature_gradient of a
        one-channel map of ones; the importance score pruning works with.  Returned in the file's order; with `out` ([n] float32,
        contiguous, in the SCENE's order) the weights are accumulated into it, e.g. over a camera set."""
        opts = opts or make_options()
        if out is not None:
            _check_tensor("out", out, (self.scene.n,), torch.float32, self.scene.device)
        shape, _ = self._out_shape(cam, opts)
        ones = torch.ones(shape[:2] + (1,), dtype=torch.float32, device=self.scene.device)
        if out is not None:
            self.feature_gradient(cam, ones, opts, out=out.unsqueeze(1))
            return out
        return self.feature_gradient(cam, ones, opts).squeeze(1)

    # -- per-gaussian statistics of a view ---------------------------------------------------------------------------------------
    def _count_mask(self, cam: GsrCamera, opts: GsrOptions, mask) -> Optional[torch.Tensor]:
        """A mask of view_stats as gsr_render_gaussian_stats reads it (None stays None): one byte per pixel, non-zero = counted."""
        if mask is None:
            return None
        _check_tensor("mask", mask, self._out_shape(cam, opts)[1], (torch.bool, torch.uint8), self.scene.device, "any",
                      " (the layout of the final T)")
        mask = mask.detach().contiguous()
        return mask.view(torch.uint8) if mask.dtype == torch.bool else mask

    def view_stats(self, cam: GsrCamera, opts: Optional[GsrOptions] = None, mask: Optional[torch.Tensor] = None,
                   out: Optional[ViewStats] = None, scene_order: bool = False, want=VIEW_STATS) -> ViewStats:
        """Per gaussian, over the counted pixels of this view and with the weights w_i = alpha_i T_i render_features composites with
        (gsr_render_gaussian_stats): weight_sum = sum_p w_i(p) (blend_weights' value), weight_max = max_p w_i(p) — the score of
        max-based pruning — and pixels = #{p : w_i(p) > 0}; pixels > 0 is the exact visible set of the view.  `want` names the
        fields to compute ("sum", "max", "pixels"); the others are None and cost nothing.  weight_max and pixels are exact and
        reproducible to the bit, weight_sum is a float atomic sum (last bits may differ between two calls).
        mask: [H, W] bool or uint8 on the scene's device in the layout render_features writes (layouts as render()); non-zero = the
        pixel counts.  It selects what is counted, not what is blended (a lasso or click region: the statistics of what shows
        there); quadrants and tiles with no counted pixel are skipped.
        Returned in the order of the file the scene was loaded from (scene_order=True: of the scene's resident arrays).  With `out`
        — a ViewStats of [n] tensors (float32, float32, int32) in the SCENE's order, only the wanted fields needed — the statistics
        are ACCUMULATED (sum +=, max = max(old, .), pixels +=; weight_max must hold non-negative finite values) and out's tensors
        are returned: stages 1-2 are checked and re-run first and only then does the blend add, so that an incomplete walk never
        reaches `out`.  Checked and re-rendered on overflow like render(); sets last_stats."""
        opts = opts or make_options()
        flags = _wanted(want, VIEW_STATS)
        mask = self._count_mask(cam, opts, mask)
        drawn = self.scene.n != 0 and 0 not in self._out_shape(cam, opts)[1]  # else nothing to draw, or a shard that owns no tile row
        res = _PerGaussianOut(self.scene, [f + (w,) for f, w in zip(_STATS_FIELDS, flags)], out, scene_order, zeroed=not drawn)
        if drawn:
            self._accumulate_view(cam, opts, "view statistics", res.own, lib.gsr_render_gaussian_stats, lib.gsr_blend_gaussian_stats,
                                  mask.data_ptr() if mask is not None else None, *res.ptrs)
        return ViewStats(*res.result())

    def visible_ids(self, cam: GsrCamera, opts: Optional[GsrOptions] = None, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """int64 ids, ascending, in the order of the file the scene was loaded from, of the gaussians that reach at least one counted
        pixel with w > 0: the view's exact visible set (view_stats' pixels > 0).  The preprocess cull is a superset of it, and a
        saturated tile hides most of that."""
        return torch.nonzero(self.view_stats(cam, opts, mask, want=("pixels",)).pixels > 0)[:, 0]

    def render_depth(self, cam: GsrCamera, opts: Optional[GsrOptions] = None, normalize: bool = False):
        """(depth [H, W], alpha [H, W]): depth = sum_i w_i z_i with z = the gaussians' camera-space depth, alpha = sum_i w_i (= 1 - final T
        up to rounding).  normalize=True divides depth by alpha where alpha > 0 (the expected depth of what was hit), 0 elsewhere."""
        m = self.render_features(cam, self._depth_features(cam), opts, scene_order=True)
        depth, alpha = m[..., 0].contiguous(), m[..., 1].contiguous()
        if normalize:
            depth = torch.where(alpha > 0, depth / alpha, torch.zeros_like(depth))
        return depth, alpha

    def render_rgbd(self, cam: GsrCamera, opts: Optional[GsrOptions] = None):
        """(image, depth, alpha): render()'s frame, bit for bit, and render_depth()'s maps from ONE preprocess and ONE bin / sort — the
        colour blend and the feature blend run on the same lists."""
        triple = self._feature_triple(self._depth_features(cam), True)

        def attempt(o):
            img, m = self._enqueue_rgbd(cam, o, triple)
            return img, m[..., 0].contiguous(), m[..., 1].contiguous()

        return _render_checked([self], [None], opts or make_options(), attempt, 8, "frame")

    # -- feature maps between two per-pixel depth limits ----------------------------------------------------------------------------
    def _depth_limit(self, plane, name: str, shape) -> Optional[torch.Tensor]:
        """A limit plane of render_slab as gsr_render_slab reads it (None stays None): float32 `shape` on the scene's device."""
        if plane is None:
            return None
        _check_tensor(name, plane, shape, torch.float32, self.scene.device, "any", " (the layout of the final T)")
        return plane.detach().contiguous()

    def render_slab(self, cam: GsrCamera, features: torch.Tensor, near: Optional[torch.Tensor] = None, far: Optional[torch.Tensor] = None,
                    opts: Optional[GsrOptions] = None, return_T: bool = True, scene_order: bool = False):
        """render_features between two per-pixel depth limits (gsr_render_slab): pixel p composites only the gaussians with
        near[p] <= z_i < far[p], z_i = the gaussian's camera-space linear depth (the unit of render_depth, the bits of
        preprocess_debug(cam)["cam_means"][:, 2]); T starts at 1 at the near limit — what lies in front of it is skipped, not
        blended.  near / far: float32 [H, W] on the scene's device in the layout of the final T (layouts as render()), or None for
        no limit on that side; a pixel with a NaN limit or far <= near draws nothing (map 0, T 1).  features, scene_order and the
        result are render_features' — (map [H, W, C], T [H, W]), or the map alone with return_T=False; with both limits open the
        map and T are render_features' bit for bit.  Up to 4 channels take one walk of the lists, up to 8 one, wider maps walks of
        16.  One preprocess and one bin / sort per call; checked and re-rendered on overflow like render(); sets last_stats.
        This path has NO BACKWARD: features that require a gradient are refused (detach them, or mask the features and use
        render_features), and nothing is differentiable in the limits."""
        if isinstance(features, torch.Tensor) and features.requires_grad and torch.is_grad_enabled():
            raise ValueError("render_slab has no backward: features that require a gradient are refused (pass features.detach())")
        opts = opts or make_options()
        tshape = self._out_shape(cam, opts)[1]
        near, far = self._depth_limit(near, "near", tshape), self._depth_limit(far, "far", tshape)
        rows = self._feature_rows(features, scene_order)

        def attempt(o):
            out, T = self._enqueue_channels(cam, o, rows, return_T, (near, far))
            return (out, T) if return_T else out

        return _render_checked([self], [None], opts, attempt, 8, "slab map")

    def _view_colours(self, cam: GsrCamera) -> torch.Tensor:
        """[n, 3] float32 in the scene's order: every gaussian's colour seen from this camera (gsr_sh_to_rgb: the values the colour
        frame blends)."""
        n, dev = self.scene.n, self.scene.device
        rgb = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        if n:
            sh = self.scene.t["sh"] if not self.scene.sh_half else self.scene.t["sh"].float()
            check(lib.gsr_sh_to_rgb(n, self.scene.t["means"].data_ptr(), sh.data_ptr(), cam.cam_center, self.scene.sh_degree,
                                    rgb.data_ptr(), _stream_ptr(dev)))
        return rgb

    def render_occluded(self, cam: GsrCamera, depth: torch.Tensor, background: Optional[torch.Tensor] = None,
                        opts: Optional[GsrOptions] = None):
        """(image [H, W, 3], T [H, W]): the colour frame IN FRONT OF a depth buffer — render_slab with the scene's colours for this
        camera as features and far = depth, so that pixel p shows the gaussians with z_i < depth[p] (camera-space linear depth; +inf:
        no occluder, the whole frame) and T[p] is how much of what lies at depth[p] shows through.  With `background` ([3] or
        [H, W, 3]: the occluder's own render) the image is composite_over(image, T, background)."""
        img, T = self.render_slab(cam, self._view_colours(cam), far=depth, opts=opts, return_T=True, scene_order=True)
        if background is not None:
            img = composite_over(img, T, background)
        return img, T

    # -- per-pixel gaussian ids ---------------------------------------------------------------------------------------------------
    def _enqueue_pick(self, cam: GsrCamera, opts: GsrOptions, median_T: float, count: bool):
        """One preprocess, one bin / sort and one gsr_blend_pick (gsr_render_pick) on the current stream, unchecked like enqueue().
        Returns (best_id, best_w, median_id, count or None) with the ids as the kernel wrote them (the scene's order)."""
        _, shape = self._out_shape(cam, opts)
        best_id, best_w, median_id = self._new(opts, shape, torch.int32, -1), self._new(opts, shape, fill=0), self._new(opts, shape, torch.int32, -1)
        cnt = self._new(opts, shape, torch.int32, 0) if count else None
        self._enqueue_view(cam, opts, lib.gsr_render_pick, best_id, float(median_T), best_id.data_ptr(), best_w.data_ptr(),
                           median_id.data_ptr(), cnt.data_ptr() if count else None)
        return best_id, best_w, median_id, cnt

    def render_pick(self, cam: GsrCamera, opts: Optional[GsrOptions] = None, median_T: float = 0.5, count: bool = False,
                    scene_order: bool = False) -> PickMaps:
        """Per pixel, over the colour frame's depth-ordered lists and with its weights w_i = alpha_i T_i (gsr_render_pick):
        best_id = the gaussian of largest weight and best_w that weight (-1 / 0 where nothing was drawn; at exactly equal weights the
        earlier gaussian in draw order), median_id = the first gaussian in draw order after which T < median_T (0.5: the median-depth
        surface; 1.0: the first hit; -1 where T never gets there), and with count=True how many gaussians had w > 0 (the walk then
        runs to T == 0 like the feature blend; without it it stops as soon as neither id can change).  int32 / float32 [H, W] maps
        (layouts as render()).  Ids index the file the scene was loaded from (scene_order=True: the scene's resident arrays, as the
        kernel wrote them).  One preprocess and one bin / sort per call; checked and re-rendered on overflow like render()."""
        if not 0.0 < float(median_T) <= 1.0:
            raise ValueError(f"median_T must lie in (0, 1], got {median_T}")

        def attempt(o):
            return self._enqueue_pick(cam, o, median_T, count)

        best_id, best_w, median_id, cnt = _render_checked([self], [None], opts or make_options(), attempt, 8, "pick map")
        if not scene_order:
            best_id, median_id = file_order_ids(best_id, self.scene.order_t), file_order_ids(median_id, self.scene.order_t)
        return PickMaps(best_id, best_w, median_id, cnt)

    # -- per-pixel contributor lists --------------------------------------------------------------------------------------------
    def _enqueue_topk(self, cam: GsrCamera, opts: GsrOptions, k: int, select: int, return_T: bool):
        """One preprocess, one bin / sort and one gsr_blend_topk (gsr_render_topk) on the current stream, unchecked like enqueue().
        Returns (ids, weights, final_T or None) with the ids as the kernel wrote them (the scene's order)."""
        shape = tuple(self._out_shape(cam, opts)[1])
        ids, weights = self._new(opts, shape + (k,), torch.int32, -1), self._new(opts, shape + (k,), fill=0)
        final_T = self._new(opts, shape, fill=1) if return_T else None
        self._enqueue_view(cam, opts, lib.gsr_render_topk, ids, k, select, ids.data_ptr(), weights.data_ptr(),
                           final_T.data_ptr() if return_T else None)
        return ids, weights, final_T

    def render_topk(self, cam: GsrCamera, k: int, opts: Optional[GsrOptions] = None, select: str = "heaviest", return_T: bool = False,
                    scene_order: bool = False) -> TopK:
        """Per pixel, over the colour frame's depth-ordered lists and with its weights w_i = alpha_i T_i (gsr_render_topk), k of the
        gaussians that make it: select="heaviest" — the k largest weights, heaviest first (at exactly equal weights the earlier
        gaussian in draw order first); select="nearest" — the first k gaussians in draw order with w > 0.  ids int32 [H, W, k] and
        weights float32 [H, W, k] (layouts as render()), unused slots -1 / 0, 1 <= k <= 16.  return_T=True adds the final
        transmittance [H, W] and walks the lists like the feature blend; without it a quadrant stops as soon as none of its lists
        can change.  Ids index the file the scene was loaded from (scene_order=True: the scene's resident arrays, as the kernel
        wrote them).  One preprocess and one bin / sort per call; checked and re-rendered on overflow like render()."""
        if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= _lib.GSR_MAX_TOPK:
            raise ValueError(f"k must be an integer in 1 .. {_lib.GSR_MAX_TOPK}, got {k}")
        if select not in TOPK_SELECT:
            raise ValueError(f"select must be one of {sorted(TOPK_SELECT)}, got {select!r}")

        def attempt(o):
            return self._enqueue_topk(cam, o, int(k), TOPK_SELECT[select], return_T)

        ids, weights, final_T = _render_checked([self], [None], opts or make_options(), attempt, 8, "top-k lists")
        if not scene_order:
            ids = file_order_ids(ids, self.scene.order_t)
        return TopK(ids, weights, final_T)

    def render_median_depth(self, cam: GsrCamera, opts: Optional[GsrOptions] = None, median_T: float = 0.5) -> torch.Tensor:
        """[H, W] float32: the camera-space depth z_cam of render_pick's median_id — the depth at which the transmittance falls below
        median_T, which floaters in front of a surface do not pull forward the way they pull render_depth's sum_i w_i z_i — and 0
        where no gaussian takes T there."""
        ids = self.render_pick(cam, opts, median_T, scene_order=True).median_id
        z = self._depth_features(cam)[:, 0]
        if self.scene.n == 0:
            return torch.zeros(ids.shape, dtype=torch.float32, device=self.scene.device)
        return torch.where(ids >= 0, z[ids.clamp(min=0).long()], torch.zeros((), dtype=torch.float32, device=self.scene.device))

    def pick(self, cam: GsrCamera, x: int, y: int, opts: Optional[GsrOptions] = None):
        """(best_id, median_id) of pixel (x, y) as Python ints, in file order (-1: nothing there): click-to-select.  A convenience over
        render_pick (median_T = 0.5) for the whole-frame image layout."""
        opts = opts or make_options()
        if opts.output_layout != 0:
            raise ValueError("pick() addresses pixels of the image layout (output_layout = 0)")
        if not (0 <= int(x) < cam.width and 0 <= int(y) < cam.height):
            raise ValueError(f"pixel ({x}, {y}) lies outside the {cam.width}x{cam.height} frame")
        m = self.render_pick(cam, opts)
        return int(m.best_id[int(y), int(x)]), int(m.median_id[int(y), int(x)])

    # -- feature maps, their gradient and view statistics, `views` cameras per launch sequence -----------------
    def _view_list(self, cams, opts: GsrOptions):
        """The cameras of a *_batch call as a list, refused as libgsr refuses them: at least one, one frame size, no screen layout."""
        cams = list(cams)
        if not cams:
            raise ValueError("a batch needs at least one view")
        if opts.output_layout == 1:
            raise ValueError("batches hold [H,W] maps or shard strips: output_layout = 1 is not supported")
        if any((c.width, c.height) != (cams[0].width, cams[0].height) for c in cams):
            raise ValueError("the views of a batch must share one frame size")
        return cams

    def _view_groups(self, cams, opts: GsrOptions):
        """(index of its first camera, the group's cameras as a ctypes array) per launch sequence: `views` cameras at a time, fewer
        with opts.batch_views or in the last group."""
        k = self._views_per_launch(opts, len(cams))
        return [(i, (GsrCamera * len(cams[i:i + k]))(*cams[i:i + k])) for i in range(0, len(cams), k)]

    def _enqueue_group(self, arr, opts: GsrOptions, entry, *args) -> GsrOptions:
        """_enqueue_view for the cameras of `arr`: one entry that takes them through the slices, `views` per launch sequence and view j
        of a sequence in slice j (gsr_render_batch, gsr_render_channels_batch; gsr_lists_views for one group — all share the prefix
        scene, cameras, how many, opts, max_pairs, workspace; `args` lie between it and the stream), on the current stream and
        unchecked.  A slice's first view starts a new record (libgsr chains the later ones) unless slice 0 holds unchecked frames:
        then all keep theirs, and the slices that held none start from an empty one.  Returns the options the entry ran with."""
        ws = self._workspace(arr[0].width, arr[0].height)
        k = self._views_per_launch(opts, len(arr))
        self._reset_slices(self.unchecked.to_reset(k))
        o = GsrOptions.from_buffer_copy(opts)
        o.keep_flags = 1 if (self.unchecked.slices or opts.keep_flags) else 0
        sc = self.scene.c_struct()
        check(entry(C.byref(sc), arr, len(arr), C.byref(o), self.max_pairs, ws.data_ptr(), ws.numel(), *args, _stream_ptr(self.scene.device)))
        self.unchecked.wrote(k)
        return o

    def _checked_lists_views(self, arr, opts: GsrOptions, what: str) -> GsrOptions:
        """_checked_lists for one group of views: gsr_lists_views, stats() on every slice and a re-run until all are complete (the
        worst view decides); only then may the caller's gsr_blend_*_views add, with the options returned here."""
        def attempt(o):
            o = GsrOptions.from_buffer_copy(o)
            o.colour_stage = 0
            return self._enqueue_group(arr, o, lib.gsr_lists_views)

        return _render_checked([self], [None], opts, attempt, 8, what)

    def _blend_lists_views(self, arr, opts: GsrOptions, entry, *args) -> None:
        """One gsr_blend_*_views entry over the lists in slices 0 .. len(arr) - 1 (the workspace is asked for again, as in _blend_lists)."""
        ws = self._workspace(arr[0].width, arr[0].height)
        check(entry(self.scene.n, arr, len(arr), C.byref(opts), self.max_pairs, ws.data_ptr(), ws.numel(), *args, _stream_ptr(self.scene.device)))

    def render_features_batch(self, cams, features: torch.Tensor, opts: Optional[GsrOptions] = None, return_T: bool = False,
                              scene_order: bool = False):
        """render_features for several cameras of one frame size, `views` of them per launch sequence (gsr_render_channels_batch: one
        preprocess, one set of sorts and one blend per group): [B, H, W, C] (a tile-row shard: [B, rows*16, W, C]) and, with return_T,
        the final transmittances [B, H, W].  Every view's map and T are render_features' bit for bit; every C goes through the
        many-channel blend.  features, scene_order: render_features'.  Checked and re-rendered on overflow like render_batch(): the
        worst view decides.  Differentiable in `features` like render_features: one autograd node for all views, whose backward is
        feature_gradient_batch()."""
        if features.requires_grad and torch.is_grad_enabled():
            return _RenderFeaturesBatch.apply(features, self, list(cams), opts, return_T, scene_order)
        return self._render_features_batch(cams, features, opts, return_T, scene_order)

    def _render_features_batch(self, cams, features: torch.Tensor, opts: Optional[GsrOptions], return_T: bool, scene_order: bool):
        opts = opts or make_options()
        cams = self._view_list(cams, opts)
        rows = self._feature_rows(features, scene_order)
        n_ch, B = int(rows.shape[1]), len(cams)
        shape, tshape = self._out_shape(cams[0], opts)
        arr = (GsrCamera * B)(*cams)

        def attempt(o):
            out = self._new(o, (B,) + tuple(shape[:2]) + (n_ch,))
            T = self._new(o, (B,) + tuple(tshape), fill=1) if return_T else None
            if out.numel() == 0 or self.scene.n == 0:  # a shard that owns no tile row, or nothing to draw: zeros, T = 1
                out.zero_()
                self.unchecked.wrote(0)
                return (out, T) if return_T else out
            self._enqueue_group(arr, o, lib.gsr_render_channels_batch, rows.data_ptr(), n_ch, int(rows.stride(0)), out.data_ptr(),
                                out[0].numel(), T.data_ptr() if return_T else None, T[0].numel() if return_T else 0)
            return (out, T) if return_T else out

        return _render_checked([self], [None], opts, attempt, 4, "feature map batch")

    def feature_gradient_batch(self, cams, grad_maps: torch.Tensor, opts: Optional[GsrOptions] = None, out: Optional[torch.Tensor] = None,
                               scene_order: bool = False) -> torch.Tensor:
        """The transpose of render_features_batch: [n, C] with row i = sum_v sum_p w_v,i(p) grad_maps[v][p] — the sum of
        feature_gradient over the cameras, added up by the kernel (gsr_blend_channels_backward_views), `views` cameras per launch
        sequence.  grad_maps: [B, H, W, C] as render_features_batch lays the maps out (made contiguous float32), finite.  Order of the
        result, `out` and its accumulation: feature_gradient's.  Two phases per group, with or without `out`: gsr_lists_views, stats()
        and a re-run until every slice is complete, and only then the blend that adds — an incomplete walk never reaches the buffer.
        Float atomic sums may differ in the last bits between two calls."""
        opts = opts or make_options()
        cams = self._view_list(cams, opts)
        gm, res = self._gradient_request(cams[0], opts, grad_maps, out, scene_order, False, "grad_maps", (len(cams),))
        if gm is not None:  # (else no workspace: feature_gradient's rule)
            buf = res.bufs[0]
            for i, arr in self._view_groups(cams, opts):
                o = self._checked_lists_views(arr, opts, "feature gradient batch")
                self._blend_lists_views(arr, o, lib.gsr_blend_channels_backward_views, gm[i].data_ptr(), gm[0].numel(), int(buf.shape[1]),
                                        buf.data_ptr(), int(buf.stride(0)))
        return res.result()[0]

    def view_stats_batch(self, cams, opts: Optional[GsrOptions] = None, masks=None, out=None, scene_order: bool = False,
                         want=VIEW_STATS_BATCH):
        """view_stats over several cameras of one frame size into ONE set of buffers, `views` cameras per launch sequence
        (gsr_blend_gaussian_stats_views): (ViewStats, views) with weight_sum summed, weight_max the maximum and pixels summed over the
        cameras, and views [n] int32 = in how many of them the gaussian reaches a counted pixel with w > 0 — counted exactly, in the
        kernel.  `want` names what to compute ("sum", "max", "pixels", "views"); the rest is None and costs nothing.  weight_max,
        pixels and views are exact and reproducible to the bit, weight_sum is a float atomic sum.
        masks: None, or one mask (view_stats') or None per camera; they travel as one uint8 [B, H, W] tensor, ones for None.
        Order of the result: view_stats'.  out: (ViewStats, views) of [n] tensors in the SCENE's order (only the wanted ones needed) to
        ACCUMULATE into; they are returned.  Two phases per group, with or without `out`: gsr_lists_views, stats() and a re-run until
        every slice is complete, and only then the blend that adds.  Sets last_stats."""
        opts = opts or make_options()
        cams = self._view_list(cams, opts)
        flags = _wanted(want, VIEW_STATS_BATCH)
        masks = [None] * len(cams) if masks is None else list(masks)
        if len(masks) != len(cams):
            raise ValueError(f"masks must hold one entry per camera: {len(masks)} for {len(cams)} cameras")
        masks = [self._count_mask(cams[0], opts, m) for m in masks]
        if out is not None:
            if not isinstance(out, tuple) or len(out) != 2 or not isinstance(out[0], tuple):
                raise ValueError("out must be (ViewStats, views), as view_stats_batch returns them")
            out = tuple(out[0]) + (out[1],)
        dev, n = self.scene.device, self.scene.n
        tshape = tuple(self._out_shape(cams[0], opts)[1])
        res = _PerGaussianOut(self.scene, [f + (w,) for f, w in zip(_STATS_FIELDS, flags)], out, scene_order, zeroed=True)
        if n != 0 and 0 not in tshape:  # else nothing to draw, or a shard that owns no tile row: no workspace (view_stats' rule)
            stacked = None
            if any(m is not None for m in masks):
                stacked = torch.ones((len(cams),) + tshape, dtype=torch.uint8, device=dev)
                for j, m in enumerate(masks):
                    if m is not None:
                        stacked[j] = m
            bits = torch.empty(n, dtype=torch.int32, device=dev) if flags[3] else None  # libgsr's scratch: cleared by every call
            for i, arr in self._view_groups(cams, opts):
                o = self._checked_lists_views(arr, opts, "view statistics batch")
                self._blend_lists_views(arr, o, lib.gsr_blend_gaussian_stats_views, stacked[i].data_ptr() if stacked is not None else None,
                                        tshape[0] * tshape[1], *res.ptrs, bits.data_ptr() if bits is not None else None)
        back = res.result()
        return ViewStats(*back[:3]), back[3]

    def _batch_out(self, cams, opts: GsrOptions, out: Optional[torch.Tensor]):
        """(out, frame_stride in elements) of a batch: whole frames [B,H,W,3], or with a tile-row shard (output_layout = 2) the
        strips [B,rows*16,W,3]."""
        if opts.output_layout == 1:
            raise ValueError("batches render [H,W,3] frames or shard strips")
        shape, _ = self._out_shape(cams[0], opts)
        full = (len(cams),) + tuple(shape)
        dtype = torch.bfloat16 if opts.output_dtype == 1 else torch.float32
        frame = shape[0] * shape[1] * shape[2]
        if out is None:
            out = self._new(opts, full, dtype)
        else:  # (consecutive frames may lie further apart than a frame: the strips of a padded wire buffer, dist.FrameGather)
            _check_tensor("out", out, full, dtype, self.scene.device, "rows")
        return out, (out.stride(0) if len(cams) > 1 and frame else frame)

    def enqueue_batch(self, cams, opts: Optional[GsrOptions] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Enqueue several views on the current stream, `views` at a time through one launch sequence (gsr_render_batch), with `opts`
        as given: no host synchronisation, no check of the caller's bounds — like enqueue(), the next stats() speaks for all of them."""
        opts = opts or make_options()
        cams = list(cams)
        if not cams:
            raise ValueError("a batch needs at least one view")
        out, stride = self._batch_out(cams, opts, out)
        if out.numel() == 0:  # a shard that owns no tile row
            self.unchecked.wrote(0)
            return out
        self._enqueue_group((GsrCamera * len(cams))(*cams), opts, lib.gsr_render_batch, out.data_ptr(), stride)
        return out

    def render_batch(self, cams, opts: Optional[GsrOptions] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Several views of the resident scene in one call: [B,H,W,3] (a tile-row shard: [B,rows*16,W,3]), `views` of them per launch
        sequence.  Pair buffers and the depth-sort bound are sized on the fly: a view that exceeds one makes the batch re-run with
        room for the worst view (_render_checked)."""
        cams = list(cams)
        def attempt(o):
            nonlocal out
            out = self.enqueue_batch(cams, o, out)
            return out

        return _render_checked([self], [None], opts or make_options(), attempt, 4, "batch")

    def fit_pairs(self, cam: GsrCamera, opts: Optional[GsrOptions] = None, slack: float = 1.25) -> int:
        """Size the pair buffers to this view: one probing frame, then max_pairs = slack * D (+ margin).
        Sort grids and histogram tables scale with max_pairs, so a snug bound is also the fast one."""
        self.render(cam, opts)
        need = int(self.last_stats["n_pairs_bbox"])
        self.max_pairs = int(min(_lib.GSR_MAX_PAIRS, max(4096, slack * need + 4096)))
        return self.max_pairs

    # -- stage-by-stage (tests, helper functions) -------------------------------------------------
    def preprocess_debug(self, cam: GsrCamera, opts: Optional[GsrOptions] = None) -> Dict[str, torch.Tensor]:
        """Run stage 1 alone and return every per-gaussian intermediate the reference's helpers produce, indexed like the
        file the scene was loaded from (whatever order the scene is stored in)."""
        opts = opts or make_options()
        n, dev = self.scene.n, self.scene.device
        f32, i64 = torch.float32, torch.int64
        out = {
            "cov3d": torch.empty((n, 3, 3), dtype=f32, device=dev), "cam_means": torch.empty((n, 3), dtype=f32, device=dev),
            "cov2d": torch.empty((n, 2, 2), dtype=f32, device=dev), "screen_means": torch.empty((n, 2), dtype=f32, device=dev),
            "tile_bboxes": torch.empty((n, 4), dtype=i64, device=dev), "sigmas": torch.empty((n, 3), dtype=f32, device=dev),
            "pixel_bboxes": torch.empty((n, 4), dtype=i64, device=dev), "rgb": torch.empty((n, 3), dtype=f32, device=dev),
            "opacity": torch.empty((n,), dtype=f32, device=dev),
        }
        dbg = GsrDebugOut()
        for k, v in out.items():
            setattr(dbg, k, v.data_ptr())
        ws = self._workspace(cam.width, cam.height)
        sc = self.scene.c_struct()
        check(lib.gsr_preprocess(C.byref(sc), C.byref(cam), C.byref(opts), ws.data_ptr(), ws.numel(), C.byref(dbg),
                                 _stream_ptr(dev)))
        # the library works in scene order; callers (and the reference's helpers) index by file order
        return {k: file_order_gradient(v, self.scene.order_t) for k, v in out.items()}


def accumulate_view_stats(R: "Rasterizer", cams, opts: Optional[GsrOptions] = None, masks=None):
    """Rasterizer.view_stats over a camera set into one set of buffers: (ViewStats, views) in the order of the file the scene was
    loaded from — weight_sum summed, weight_max the maximum and pixels summed over the views, and `views` [n] int32 = in how many
    of the views the gaussian reached a counted pixel.  masks: None, or one mask (or None) per camera.  A Rasterizer with `views` > 1
    takes all cameras through ONE view_stats_batch call (`views` of them per launch sequence, the view count exact from the kernel);
    else one view_stats call per camera."""
    cams = list(cams)
    masks = [None] * len(cams) if masks is None else list(masks)
    if len(masks) != len(cams):
        raise ValueError(f"masks must hold one entry per camera: {len(masks)} for {len(cams)} cameras")
    if getattr(R, "views", 1) > 1 and cams:
        return R.view_stats_batch(cams, opts, masks)
    n, dev = R.scene.n, R.scene.device
    total = ViewStats(torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev),
                      torch.zeros(n, dtype=torch.int32, device=dev))
    views = torch.zeros(n, dtype=torch.int32, device=dev)
    seen = torch.zeros(n, dtype=torch.int32, device=dev)  # this view's pixel counts
    for cam, mask in zip(cams, masks):
        seen.zero_()
        R.view_stats(cam, opts, mask, out=ViewStats(total.weight_sum, total.weight_max, seen))
        total.pixels.add_(seen)
        views.add_((seen > 0).to(torch.int32))
    o_t = R.scene.order_t
    return ViewStats(*[file_order_gradient(b, o_t) for b in total]), file_order_gradient(views, o_t)


class FramesInFlight:
    """Throughput mode for independent frames (a camera path, a batch of views): `slots` frames in flight, each on its own
    HIP stream with its own workspace, so that one frame's HBM-bound stages (preprocess, sorts) overlap another's
    VALU-bound blend and the short launch-bound kernels of a multi-GPU shard overlap each other.  libgsr keeps no state and
    every call is stream-asynchronous, so this is plain use of the C ABI: one (workspace, stream) pair per slot.  Frames
    are bit-identical to single-stream rendering; only the time per frame changes (tools/stream_overlap.py).

    submit() returns the slot it used; the caller owns the ordering of its output buffers: wait(slot) makes the current
    stream wait for that slot's last frame."""

    def __init__(self, scene: GaussianScene, slots: int = 4, max_pairs: Optional[int] = None, views: int = 1):
        if slots < 1:
            raise ValueError("slots must be >= 1")
        self.scene = scene
        self.rasterizers = [Rasterizer(scene, max_pairs=max_pairs, views=views) for _ in range(slots)]
        self.streams = [torch.cuda.Stream(device=scene.device) for _ in range(slots)]
        cur = torch.cuda.current_stream(scene.device)
        for st in self.streams:  # the scene upload (and whatever else the caller enqueued) comes first
            st.wait_stream(cur)
        self._next = 0

    @property
    def slots(self) -> int:
        return len(self.rasterizers)

    def set_max_pairs(self, max_pairs: int) -> None:
        for r in self.rasterizers:
            r.max_pairs = int(max_pairs)

    def set_sort_passes(self, passes: int) -> None:
        """Share the depth-sort bound one slot has learned (Rasterizer.sort_passes) with all of them."""
        for r in self.rasterizers:
            r.sort_passes = max(r.sort_passes, int(passes))

    def _take_slot(self, slot: Optional[int]) -> int:
        """The slot a submit uses: the caller's, else the next one round robin."""
        if slot is not None:
            return int(slot)
        k = self._next
        self._next = (k + 1) % len(self.rasterizers)
        return k

    def submit(self, cam: GsrCamera, opts: Optional[GsrOptions] = None, out: Optional[torch.Tensor] = None,
               slot: Optional[int] = None) -> int:
        """Enqueue one frame on the next slot's stream (round robin) and return the slot.  Unchecked, with `opts` as given
        (Rasterizer.enqueue): stats(slot) afterwards speaks for every frame the slot has rendered since its last stats()."""
        k = self._take_slot(slot)
        with torch.cuda.stream(self.streams[k]):
            self.rasterizers[k].enqueue(cam, opts, out=out)
        return k

    def submit_batch(self, cams, opts: Optional[GsrOptions] = None, out: Optional[torch.Tensor] = None, slot: Optional[int] = None) -> int:
        """submit() for several views at once: Rasterizer.enqueue_batch on the next slot's stream (`views` of them per launch sequence)."""
        k = self._take_slot(slot)
        with torch.cuda.stream(self.streams[k]):
            self.rasterizers[k].enqueue_batch(cams, opts, out=out)
        return k

    def render_batch(self, cams, opts: Optional[GsrOptions] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Rasterizer.render_batch with the views spread round robin over the slots (gsr_render_batch_slots; with `views` > 1 each
        slot takes `views` consecutive cameras per launch sequence): [B,H,W,3], bit-identical to the single-stream batch.  The
        current stream waits for every slot before this returns; a view that exceeds a bound makes the batch re-run with room for
        it (_render_checked).  Frames submit()ted and not yet checked are checked first: their errors are raised."""
        opts = opts or make_options()
        if opts.output_layout != 0 or opts.tile_row_step > 1:
            raise ValueError("render_batch renders whole [H,W,3] frames")
        cams = list(cams)
        if not cams:
            raise ValueError("render_batch needs at least one view")
        arr = (GsrCamera * len(cams))(*cams)
        W, H = cams[0].width, cams[0].height
        dev = self.scene.device
        dtype = torch.bfloat16 if opts.output_dtype == 1 else torch.float32
        if out is None:
            out = torch.empty((len(cams), H, W, 3), dtype=dtype, device=dev)
        else:
            _check_tensor("out", out, (len(cams), H, W, 3), dtype, dev)
        sc = self.scene.c_struct()
        n = len(self.rasterizers)
        cur = torch.cuda.current_stream(dev)
        r0 = self.rasterizers[0]

        def attempt(o):
            wss = [r._workspace(W, H) for r in self.rasterizers]  # all of one size: the slots share max_pairs
            for k, r in enumerate(self.rasterizers):
                self.streams[k].wait_stream(cur)  # `out` (and the workspaces) may have been allocated / used on the current stream
                if r.unchecked.slices:  # frames submit()ted and not yet checked: read (and report) their record before the batch clears it
                    self.stats(k)
            o = GsrOptions.from_buffer_copy(o)
            o.keep_flags = 0  # a slot's first view clears its record, libgsr chains the slot's later views
            ws_arr = (C.c_void_p * n)(*[w.data_ptr() for w in wss])
            st_arr = (C.c_void_p * n)(*[int(st.cuda_stream) for st in self.streams])
            check(lib.gsr_render_batch_slots(C.byref(sc), arr, len(cams), C.byref(o), r0.max_pairs, ws_arr, wss[0].numel(), st_arr, n,
                                             out.data_ptr(), H * W * 3))
            k = r0._views_per_launch(o, len(cams))
            sizes = [min(k, len(cams) - i) for i in range(0, len(cams), k)]  # launch sequence g renders on slot g % n
            for s, r in enumerate(self.rasterizers[:len(sizes)]):
                r.unchecked.wrote(max(sizes[s::n]))  # the slices its launch sequences rendered into
            for s in range(n):
                self.wait(s)
            return out

        return _render_checked(self.rasterizers, self.streams, opts, attempt, 4, "batch")

    def wait(self, slot: int) -> None:
        torch.cuda.current_stream(self.scene.device).wait_stream(self.streams[slot])

    def synchronize(self) -> None:
        for st in self.streams:
            st.synchronize()

    def stats(self, slot: int = 0) -> Dict[str, int]:
        with torch.cuda.stream(self.streams[slot]):
            return self.rasterizers[slot].stats()
