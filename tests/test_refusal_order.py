"""CPU: the ORDER of every entry point's refusals.  The test_*_abi.py files state that each refusal exists and what it says; this
one states which comes first.  Every entry that takes a camera and a workspace is called with everything it checks wrong at once
and peeled: the call is refused (return code and the whole gsr_last_error() text are compared), exactly what that text names is
put right, the call is made again — until the last refusal, GSR_ERR_WORKSPACE.  No call gets further than that: the workspace is
an address nobody owns and its size stays 0 (for the entries that take several views in one workspace: one slice, for two views),
so nothing is ever launched and no GPU is needed.

Two fields can be wrong in two ways that different checks refuse.  output_dtype / accum_dtype = 1 (bfloat16) is what the list
consumers refuse and 2 what the frame's checks refuse; output_layout = 1 is what the view entries refuse and 3 what the frame's
checks refuse.  Putting the first right leaves the second wrong, so the peel also states which of the two checks comes first.
Likewise the cameras: first of two sizes, then of one size that is too large.  A text that names several arguments ("bad
argument", "null camera/options/workspace") has them put right one call at a time.

EXPECTED was read off the library as it stood before the entries were folded onto one description per list consumer.
"""
import ctypes as C
import re
import types

import pytest

P = 0x70000          # an address nobody owns: 256-byte aligned, never dereferenced
BIG_SIDE = 1 << 20   # > GSR_MAX_FRAME_SIDE
CONSUMERS = ("features", "channels", "slab", "channels_backward", "splat_backward", "gaussian_stats", "pick", "topk")
VIEW_BLENDS = ("gsr_blend_channels_views", "gsr_blend_channels_backward_views", "gsr_blend_gaussian_stats_views")
SLICED = ("gsr_lists_views",) + VIEW_BLENDS   # view v works in slice v of ONE workspace: a second refusal about its size
ENTRIES = (("gsr_preprocess", "gsr_bin_sort", "gsr_blend", "gsr_render_forward")
           + tuple(f"gsr_{stage}_{kind}" for kind in CONSUMERS for stage in ("blend", "render"))
           + SLICED + ("gsr_render_channels_batch", "gsr_render_batch", "gsr_render_batch_slots"))


def _wrong(entry):
    """Every argument `entry` checks, wrong."""
    from gsr_amd import _lib

    s = types.SimpleNamespace(entry=entry)
    s.scene, s.scene_null = _lib.GsrScene(), entry not in ("gsr_blend", "gsr_blend_slab")   # (these two may do without one: given)
    s.scene.n, s.scene.sh_degree, s.scene.sh_dtype, s.scene.block_bounds = _lib.GSR_MAX_GAUSSIANS + 1, 4, 2, P + 4
    s.n = -1
    s.cams, s.cams_null, s.opts_null = (_lib.GsrCamera * 2)(), True, True
    batch = entry in ("gsr_render_batch", "gsr_render_batch_slots")
    (s.cams[0].width, s.cams[0].height), (s.cams[1].width, s.cams[1].height) = (BIG_SIDE, 48), ((0, 32) if batch else (64, 32))
    s.n_views = -1 if "batch" in entry else 0
    o = s.opts = _lib.default_options()
    o.tile_row_begin, o.tile_row_step, o.tile_row_block, o.draw_limit, o.blend_impl, o.depth_sort_passes = -1, -1, 3, -1, 2, 5
    o.keep_flags, o.saturation_rule, o.fine_binning, o.shard_preprocess, o.blend_pipe_tiles, o.no_order_hint = 2, 2, 2, 3, -2, 2
    o.colour_stage, o.sh_dense_min, o.batch_views = 2, 66, 9
    consumer = any(kind in entry for kind in CONSUMERS)
    o.output_dtype = o.accum_dtype = 1 if consumer else 2
    o.output_layout = 1 if entry in SLICED or entry == "gsr_render_channels_batch" else 3
    s.max_pairs, s.workspace, s.workspace_bytes = _lib.GSR_MAX_PAIRS + 1, None, 0
    s.slots, s.slots_null, s.streams_null, s.n_slots = (C.c_void_p * 2)(), True, True, 0
    s.out, s.frame_stride = None, 0                                  # gsr_blend, gsr_render_forward and the frame batches
    s.features = s.out_map = s.grad_map = s.grad_features = s.grad_splat = None
    s.channels, s.feature_stride, s.grad_stride, s.min_T, s.want_abs = 0, 0, 0, float("nan"), 1
    s.stats, s.view_hits, s.view_bits = [None, None, None], None, None
    s.median_T, s.pick, s.k, s.select, s.topk = float("nan"), None, 0, 2, None
    s.map_stride = s.T_stride = s.mask_stride = 0
    return s


def _call(s):
    from gsr_amd import _lib

    entry = s.entry
    scene = None if s.scene_null else C.byref(s.scene)
    opts = None if s.opts_null else C.byref(s.opts)
    ws = (s.workspace, s.workspace_bytes)
    if "views" in entry or "batch" in entry:
        cams = (None if s.cams_null else s.cams, s.n_views, opts, s.max_pairs)
    else:
        cams = (None if s.cams_null else C.byref(s.cams[0]), opts, s.max_pairs)
    kind = next((k for k in CONSUMERS if entry in (f"gsr_blend_{k}", f"gsr_render_{k}")), None)
    tail = {
        None: (),
        "features": (s.features, s.out_map, None),
        "channels": (s.features, s.channels, s.feature_stride, s.out_map, None),
        "slab": (s.features, s.channels, s.feature_stride, None, None, s.out_map, None),
        "channels_backward": (s.grad_map, s.channels, s.grad_features, s.grad_stride),
        "splat_backward": (s.features, s.feature_stride, s.channels, s.grad_map, None, s.min_T, s.want_abs, s.grad_splat),
        "gaussian_stats": (None, *s.stats),
        "pick": (s.median_T, s.pick, None, None, None),
        "topk": (s.k, s.select, s.topk, None, None),
    }[kind]
    if entry in ("gsr_blend_channels_views", "gsr_render_channels_batch"):  # (with a final T and masks, so that their strides are read)
        tail = (s.features, s.channels, s.feature_stride, s.out_map, s.map_stride, P, s.T_stride)
    elif entry == "gsr_blend_channels_backward_views":
        tail = (s.grad_map, s.map_stride, s.channels, s.grad_features, s.grad_stride)
    elif entry == "gsr_blend_gaussian_stats_views":
        tail = (P, s.mask_stride, *s.stats, s.view_hits, s.view_bits)
    fn = getattr(_lib.lib, entry)
    if entry == "gsr_preprocess":
        return fn(scene, cams[0], opts, *ws, None, None)
    if entry == "gsr_bin_sort":
        return fn(s.n, *cams, *ws, None)
    if entry == "gsr_blend":
        return fn(scene, s.n, *cams, *ws, s.out, None, None)
    if entry == "gsr_render_forward":
        return fn(scene, *cams, *ws, s.out, None, None)
    if entry == "gsr_render_batch":
        return fn(scene, *cams, *ws, s.out, s.frame_stride, None)
    if entry == "gsr_render_batch_slots":
        return fn(scene, *cams, None if s.slots_null else s.slots, s.workspace_bytes, None if s.streams_null else (C.c_void_p * 2)(), s.n_slots,
                  s.out, s.frame_stride)
    if entry == "gsr_blend_slab":
        return fn(scene, s.n, *cams, *ws, *tail, None)
    head = scene if entry.startswith("gsr_render_") or entry == "gsr_lists_views" else s.n
    return fn(head, *cams, *ws, *tail, None)


def _first_null(s, names):
    """Put right the first of these that is still missing: one argument per call."""
    for name in names:
        if name in ("scene", "cams", "opts", "slots", "streams"):
            if getattr(s, name + "_null"):
                return setattr(s, name + "_null", False)
        elif name == "n_slots":
            if s.n_slots < 1:
                s.n_slots = 2
                return
        elif name == "n_views":
            if s.n_views < 0:
                s.n_views = 2
                return
        elif name == "workspace":
            if s.workspace is None:
                s.workspace = P + 8   # there, but not 256-byte aligned
                return
        elif name == "scene.n":
            if s.scene.n > 0x7FFFFFFF:
                s.scene.n = 0x7FFFFFFF   # what check_batch accepts; the frame's checks accept it too
                return
        elif getattr(s, name) is None:
            return setattr(s, name, P)
    raise AssertionError(f"{s.entry}: nothing left to put right among {names}")


def _set(**fields):
    def repair(s, m):
        for k, v in fields.items():
            if k.startswith("opts."):
                setattr(s.opts, k[5:], v)
            elif k.startswith("scene."):
                setattr(s.scene, k[6:], v)
            else:
                setattr(s, k, v)
    return repair


def _scene_arrays(s, m):
    for k in ("means", "log_scales", "opacity_logit"):
        setattr(s.scene, k, P)
    s.scene.quats = s.scene.sh = P + 4   # there, but not 16-byte aligned


def _one_size(s, m):
    s.cams[1].width, s.cams[1].height = s.cams[0].width, s.cams[0].height


def _all_sizes(s, m):
    for c in s.cams:
        c.width, c.height = 64, 48


def _bf16(field):
    return lambda s, m: setattr(s.opts, field, 2)   # no longer bfloat16, and still no dtype there is


def _slot(s, m):
    s.slots[int(m.group(1))] = P + 8   # (shared with the other slot, and misaligned)


BATCH_ARGS = ("scene", "cams", "n_views", "out", "opts", "scene.n")   # what the frame batches refuse in two words
SLOT_ARGS = ("slots", "streams", "n_slots")                            # gsr_render_batch_slots: and these, before them
# the text of a refusal -> what puts exactly that right
REPAIRS = [(re.compile(pattern), repair) for pattern, repair in (
    (r"null scene$", _set(scene_null=False)),
    (r"null scene array$", _scene_arrays),
    (r"sh_degree 4 not in 0\.\.3$", _set(**{"scene.sh_degree": 3})),
    (r"sh_dtype 2: ", _set(**{"scene.sh_dtype": 0})),
    (r"sh, quats and block_bounds must be 16-byte aligned$", _set(**{"scene.quats": P, "scene.sh": P, "scene.block_bounds": P})),
    (r"scene->n = (\d+) but n = -1$", lambda s, m: setattr(s, "n", int(m.group(1)))),
    (r"null camera/options/workspace$", lambda s, m: _first_null(s, ("cams", "opts", "workspace"))),
    (r"null camera/options$", lambda s, m: _first_null(s, ("cams", "opts"))),
    (r"null cameras?$", _set(cams_null=False)),
    (r"null options$", _set(opts_null=False)),
    (r"bad argument$", lambda s, m: _first_null(s, (SLOT_ARGS if "slots" in s.entry else ()) + BATCH_ARGS)),
    (r"null workspace in slot (\d)$", _slot),
    (r"slots 0 and 1 share a workspace$", lambda s, m: s.slots.__setitem__(1, 2 * P + 8)),
    (r"null output image$", _set(out=P)),
    (r"null features$", _set(features=P)),
    (r"null output map$", _set(out_map=P)),
    (r"null gradient map$", _set(grad_map=P)),
    (r"null feature gradient$", _set(grad_features=P)),
    (r"null splat gradient$", _set(grad_splat=P)),
    (r"null statistics outputs: all three$", lambda s, m: s.stats.__setitem__(0, P)),
    (r"null statistics outputs: all four$", _set(view_hits=P)),
    (r"view_hits needs the view_bits scratch$", _set(view_bits=P)),
    (r"null pick outputs: all four$", _set(pick=P)),
    (r"null top-k outputs: both ids and weights$", _set(topk=P)),
    (r"bad channels 0 ", _set(channels=17)),
    (r"bad feature_stride 0: rows of 17 channels overlap$", _set(feature_stride=32)),
    (r"bad grad_stride 0: rows of 17 channels overlap$", _set(grad_stride=32)),
    (r"bad min_T nan", _set(min_T=0.0)),
    (r"want_abs with 17 channels", _set(want_abs=0)),
    (r"bad median_T nan", _set(median_T=0.5)),
    (r"bad k 0 ", _set(k=4)),
    (r"bad select 2 ", _set(select=0)),
    (r".*: output_dtype = 1 \(bfloat16\) is not supported$", _bf16("output_dtype")),
    (r".*: accum_dtype = 1 \(bfloat16\) is not supported$", _bf16("accum_dtype")),
    (r"bad view count 0 ", _set(n_views=2)),
    (r"bad camera count -1$", _set(n_views=2)),
    (r"bad frame size 0x32$", lambda s, m: setattr(s.cams[1], "width", 64)),
    (r"views of a (batch|launch sequence) must share one frame size$", _one_size),
    (r"views of a launch sequence are .* output_layout = 1 is not supported$", _set(**{"opts.output_layout": 3})),
    (r"frame_stride smaller than a frame$", _set(frame_stride=1 << 40)),
    (r"bad (map|T|mask)_stride 0: smaller than a view's .* \((\d+)\)$", lambda s, m: setattr(s, m.group(1) + "_stride", int(m.group(2)))),
    (r"n = -?\d+ out of range ", _set(n=100, **{"scene.n": 100})),
    (r"bad frame size \d+x48 \(1 \.\. ", _all_sizes),
    (r"max_pairs = \d+ out of range ", _set(max_pairs=1000)),
    (r"bad tile-row shard -1/-1$", _set(**{"opts.tile_row_begin": 0, "opts.tile_row_step": 1})),
    (r"bad tile_row_block 3 ", _set(**{"opts.tile_row_block": 0})),
    (r"bad batch_views 9 ", _set(**{"opts.batch_views": 0})),
    (r"bad (\w+) -?\d+$", lambda s, m: setattr(s.opts, m.group(1), 0)),   # the frame's checks of one options field each
    (r"workspace must be 256-byte aligned$", lambda s, m: (_set(workspace=P)(s, m), s.slots.__setitem__(0, P), s.slots.__setitem__(1, 2 * P))),
)]


def _put_right(s, text):
    hits = [(p.match(text), repair) for p, repair in REPAIRS if p.match(text)]
    assert hits, f"{s.entry}: no argument is named by {text!r}"
    m, repair = hits[0]
    repair(s, m)


def peel(entry):
    """[(return code, text)] of the refusals of `entry`, from everything wrong to the workspace's size."""
    from gsr_amd import _lib

    s, seen = _wrong(entry), []
    for _ in range(80):
        rc = _call(s)
        assert rc != _lib.GSR_OK, f"{entry}: the call went through after {seen}"
        text = _lib.lib.gsr_last_error().decode()
        seen.append((rc, text))
        if rc == _lib.GSR_ERR_WORKSPACE:
            one = re.match(r"workspace too small: 0 bytes given, (\d+) needed$", text)
            if one and entry in SLICED and s.n_views == 2:   # one slice for two views: refused as well, and last
                s.workspace_bytes = int(one.group(1))
                continue
            return seen
        _put_right(s, text)
    raise AssertionError(f"{entry}: no end after {seen}")


# the frame's checks of the options, one field each, and of the workspace's address: the same run in every entry
OPTIONS = [
    (-1, 'bad tile-row shard -1/-1'),
    (-1, 'bad tile_row_block 3 (0 / 1: single rows, 2: pairs)'),
    (-1, 'bad draw_limit -1'),
    (-1, 'bad output_dtype 2'),
    (-1, 'bad blend_impl 2'),
    (-1, 'bad output_layout 3'),
    (-1, 'bad depth_sort_passes 5'),
    (-1, 'bad accum_dtype 2'),
    (-1, 'bad keep_flags 2'),
    (-1, 'bad saturation_rule 2'),
    (-1, 'bad fine_binning 2'),
    (-1, 'bad shard_preprocess 3'),
    (-1, 'bad blend_pipe_tiles -2'),
    (-1, 'bad no_order_hint 2'),
    (-1, 'bad colour_stage 2'),
    (-1, 'bad sh_dense_min 66'),
    (-1, 'bad batch_views 9 (0 .. 8)'),
    (-1, 'workspace must be 256-byte aligned'),
]
# a scene that is there: its arrays, its two enumerations, its alignment
SCENE = [
    (-1, 'null scene array'),
    (-1, 'sh_degree 4 not in 0..3'),
    (-1, 'sh_dtype 2: 0 (float32) or 1 (float16)'),
    (-1, 'sh, quats and block_bounds must be 16-byte aligned'),
]
SIZES = [
    (-1, 'bad frame size 1048576x48 (1 .. 1048560 px per side)'),
    (-1, 'max_pairs = 4294959105 out of range [0, 4294959104]'),
]
# the frame's checks from the workspace pointer on, behind an entry's own: with n = -1 (lists in the workspace), with the scene's n
FRAME_OF_LISTS = [(-1, 'null camera/options/workspace'), (-1, 'n = -1 out of range [0, 2147483647]'), *SIZES, *OPTIONS]
FRAME_OF_SCENE = [(-1, 'null camera/options/workspace'), (-1, 'n = 2147483648 out of range [0, 2147483647]'), *SIZES, *OPTIONS]
EXPECTED = {
    "gsr_preprocess": [
        (-1, 'null scene'),
        *SCENE,
        (-1, 'null camera/options/workspace'),
        (-1, 'null camera/options/workspace'),
        (-1, 'null camera/options/workspace'),
        (-1, 'n = 2147483648 out of range [0, 2147483647]'),
        (-1, 'bad frame size 1048576x48 (1 .. 1048560 px per side)'),
        *OPTIONS,
        (-2, 'workspace too small: 0 bytes given, 16896 needed'),
    ],
    "gsr_bin_sort": [
        (-1, 'null camera/options/workspace'),
        (-1, 'null camera/options/workspace'),
        *FRAME_OF_LISTS,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
    ],
    "gsr_blend": [
        (-1, 'null output image'),
        *SCENE,
        (-1, 'scene->n = 2147483648 but n = -1'),
        (-1, 'null camera/options/workspace'),
        (-1, 'null camera/options/workspace'),
        *FRAME_OF_SCENE,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
    ],
    "gsr_render_forward": [
        (-1, 'null camera/options'),
        (-1, 'null camera/options'),
        (-1, 'null scene'),
        *SCENE,
        (-1, 'null output image'),
        *FRAME_OF_SCENE,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
    ],
    "gsr_blend_features": [
        (-1, 'null camera/options'),
        (-1, 'null camera/options'),
        (-1, 'null features'),
        (-1, 'null output map'),
        (-1, 'feature maps are float32: output_dtype = 1 (bfloat16) is not supported'),
        (-1, 'feature maps are accumulated in float32: accum_dtype = 1 (bfloat16) is not supported'),
        *FRAME_OF_LISTS,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
    ],
    "gsr_render_features": [
        (-1, 'null camera/options'),
        (-1, 'null camera/options'),
        (-1, 'null features'),
        (-1, 'null output map'),
        (-1, 'feature maps are float32: output_dtype = 1 (bfloat16) is not supported'),
        (-1, 'feature maps are accumulated in float32: accum_dtype = 1 (bfloat16) is not supported'),
        (-1, 'null scene'),
        *SCENE,
        *FRAME_OF_SCENE,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
    ],
    "gsr_blend_channels": [
        (-1, 'null camera'),
        (-1, 'null options'),
        (-1, 'null features'),
        (-1, 'null output map'),
        (-1, 'bad channels 0 (1 .. 1024)'),
        (-1, 'bad feature_stride 0: rows of 17 channels overlap'),
        (-1, 'feature maps are float32: output_dtype = 1 (bfloat16) is not supported'),
        (-1, 'feature maps are accumulated in float32: accum_dtype = 1 (bfloat16) is not supported'),
        *FRAME_OF_LISTS,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
    ],
    "gsr_render_channels": [
        (-1, 'null camera'),
        (-1, 'null options'),
        (-1, 'null features'),
        (-1, 'null output map'),
        (-1, 'bad channels 0 (1 .. 1024)'),
        (-1, 'bad feature_stride 0: rows of 17 channels overlap'),
        (-1, 'feature maps are float32: output_dtype = 1 (bfloat16) is not supported'),
        (-1, 'feature maps are accumulated in float32: accum_dtype = 1 (bfloat16) is not supported'),
        (-1, 'null scene'),
        *SCENE,
        *FRAME_OF_SCENE,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
    ],
    "gsr_blend_slab": [
        (-1, 'null camera'),
        (-1, 'null options'),
        (-1, 'null features'),
        (-1, 'null output map'),
        (-1, 'bad channels 0 (1 .. 1024)'),
        (-1, 'bad feature_stride 0: rows of 17 channels overlap'),
        (-1, 'feature maps are float32: output_dtype = 1 (bfloat16) is not supported'),
        (-1, 'feature maps are accumulated in float32: accum_dtype = 1 (bfloat16) is not supported'),
        *SCENE,
        (-1, 'scene->n = 2147483648 but n = -1'),
        *FRAME_OF_SCENE,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
    ],
    "gsr_render_slab": [
        (-1, 'null camera'),
        (-1, 'null options'),
        (-1, 'null features'),
        (-1, 'null output map'),
        (-1, 'bad channels 0 (1 .. 1024)'),
        (-1, 'bad feature_stride 0: rows of 17 channels overlap'),
        (-1, 'feature maps are float32: output_dtype = 1 (bfloat16) is not supported'),
        (-1, 'feature maps are accumulated in float32: accum_dtype = 1 (bfloat16) is not supported'),
        (-1, 'null scene'),
        *SCENE,
        *FRAME_OF_SCENE,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
    ],
    "gsr_blend_channels_backward": [
        (-1, 'null camera'),
        (-1, 'null options'),
        (-1, 'null gradient map'),
        (-1, 'null feature gradient'),
        (-1, 'bad channels 0 (1 .. 1024)'),
        (-1, 'bad grad_stride 0: rows of 17 channels overlap'),
        (-1, 'gradient maps are float32: output_dtype = 1 (bfloat16) is not supported'),
        (-1, 'feature gradients are accumulated in float32: accum_dtype = 1 (bfloat16) is not supported'),
        *FRAME_OF_LISTS,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
    ],
    "gsr_render_channels_backward": [
        (-1, 'null camera'),
        (-1, 'null options'),
        (-1, 'null gradient map'),
        (-1, 'null feature gradient'),
        (-1, 'bad channels 0 (1 .. 1024)'),
        (-1, 'bad grad_stride 0: rows of 17 channels overlap'),
        (-1, 'gradient maps are float32: output_dtype = 1 (bfloat16) is not supported'),
        (-1, 'feature gradients are accumulated in float32: accum_dtype = 1 (bfloat16) is not supported'),
        (-1, 'null scene'),
        *SCENE,
        *FRAME_OF_SCENE,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
    ],
    "gsr_blend_splat_backward": [
        (-1, 'null camera'),
        (-1, 'null options'),
        (-1, 'null features'),
        (-1, 'null gradient map'),
        (-1, 'null splat gradient'),
        (-1, 'bad channels 0 (1 .. 1024)'),
        (-1, 'bad feature_stride 0: rows of 17 channels overlap'),
        (-1, 'bad min_T nan: a finite value >= 0'),
        (-1, 'want_abs with 17 channels: the absolute sums are not linear in the channels, one walk of at most 16'),
        (-1, 'gradient maps are float32: output_dtype = 1 (bfloat16) is not supported'),
        (-1, 'splat gradients are accumulated in float32: accum_dtype = 1 (bfloat16) is not supported'),
        *FRAME_OF_LISTS,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
    ],
    "gsr_render_splat_backward": [
        (-1, 'null camera'),
        (-1, 'null options'),
        (-1, 'null features'),
        (-1, 'null gradient map'),
        (-1, 'null splat gradient'),
        (-1, 'bad channels 0 (1 .. 1024)'),
        (-1, 'bad feature_stride 0: rows of 17 channels overlap'),
        (-1, 'bad min_T nan: a finite value >= 0'),
        (-1, 'want_abs with 17 channels: the absolute sums are not linear in the channels, one walk of at most 16'),
        (-1, 'gradient maps are float32: output_dtype = 1 (bfloat16) is not supported'),
        (-1, 'splat gradients are accumulated in float32: accum_dtype = 1 (bfloat16) is not supported'),
        (-1, 'null scene'),
        *SCENE,
        *FRAME_OF_SCENE,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
    ],
    "gsr_blend_gaussian_stats": [
        (-1, 'null camera'),
        (-1, 'null options'),
        (-1, 'null statistics outputs: all three'),
        (-1, 'gaussian statistics are float32 / uint32: output_dtype = 1 (bfloat16) is not supported'),
        (-1, 'the weights are accumulated in float32: accum_dtype = 1 (bfloat16) is not supported'),
        *FRAME_OF_LISTS,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
    ],
    "gsr_render_gaussian_stats": [
        (-1, 'null camera'),
        (-1, 'null options'),
        (-1, 'null statistics outputs: all three'),
        (-1, 'gaussian statistics are float32 / uint32: output_dtype = 1 (bfloat16) is not supported'),
        (-1, 'the weights are accumulated in float32: accum_dtype = 1 (bfloat16) is not supported'),
        (-1, 'null scene'),
        *SCENE,
        *FRAME_OF_SCENE,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
    ],
    "gsr_blend_pick": [
        (-1, 'null camera'),
        (-1, 'null options'),
        (-1, 'null pick outputs: all four'),
        (-1, 'bad median_T nan (0 < median_T <= 1)'),
        (-1, 'pick maps are int32 / float32: output_dtype = 1 (bfloat16) is not supported'),
        (-1, 'pick weights are accumulated in float32: accum_dtype = 1 (bfloat16) is not supported'),
        *FRAME_OF_LISTS,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
    ],
    "gsr_render_pick": [
        (-1, 'null camera'),
        (-1, 'null options'),
        (-1, 'null pick outputs: all four'),
        (-1, 'bad median_T nan (0 < median_T <= 1)'),
        (-1, 'pick maps are int32 / float32: output_dtype = 1 (bfloat16) is not supported'),
        (-1, 'pick weights are accumulated in float32: accum_dtype = 1 (bfloat16) is not supported'),
        (-1, 'null scene'),
        *SCENE,
        *FRAME_OF_SCENE,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
    ],
    "gsr_blend_topk": [
        (-1, 'null camera'),
        (-1, 'null options'),
        (-1, 'null top-k outputs: both ids and weights'),
        (-1, 'bad k 0 (1 .. 16)'),
        (-1, 'bad select 2 (GSR_TOPK_HEAVIEST = 0, GSR_TOPK_NEAREST = 1)'),
        (-1, 'top-k lists are int32 / float32: output_dtype = 1 (bfloat16) is not supported'),
        (-1, 'top-k weights are accumulated in float32: accum_dtype = 1 (bfloat16) is not supported'),
        *FRAME_OF_LISTS,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
    ],
    "gsr_render_topk": [
        (-1, 'null camera'),
        (-1, 'null options'),
        (-1, 'null top-k outputs: both ids and weights'),
        (-1, 'bad k 0 (1 .. 16)'),
        (-1, 'bad select 2 (GSR_TOPK_HEAVIEST = 0, GSR_TOPK_NEAREST = 1)'),
        (-1, 'top-k lists are int32 / float32: output_dtype = 1 (bfloat16) is not supported'),
        (-1, 'top-k weights are accumulated in float32: accum_dtype = 1 (bfloat16) is not supported'),
        (-1, 'null scene'),
        *SCENE,
        *FRAME_OF_SCENE,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
    ],
    "gsr_lists_views": [
        (-1, 'null scene'),
        *SCENE,
        (-1, 'null cameras'),
        (-1, 'null options'),
        (-1, 'bad view count 0 (1 .. 8)'),
        (-1, 'views of a launch sequence must share one frame size'),
        (-1, 'views of a launch sequence are [H,W] maps or shard strips: output_layout = 1 is not supported'),
        *FRAME_OF_SCENE,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
        (-2, 'workspace too small for 2 views per launch: 32256 bytes given, 64512 needed'),
    ],
    "gsr_blend_channels_views": [
        (-1, 'null cameras'),
        (-1, 'null options'),
        (-1, 'bad view count 0 (1 .. 8)'),
        (-1, 'views of a launch sequence must share one frame size'),
        (-1, 'views of a launch sequence are [H,W] maps or shard strips: output_layout = 1 is not supported'),
        (-1, 'null features'),
        (-1, 'null output map'),
        (-1, 'bad channels 0 (1 .. 1024)'),
        (-1, 'bad feature_stride 0: rows of 17 channels overlap'),
        (-1, 'feature maps are float32: output_dtype = 1 (bfloat16) is not supported'),
        (-1, 'feature maps are accumulated in float32: accum_dtype = 1 (bfloat16) is not supported'),
        (-1, "bad map_stride 0: smaller than a view's map (855638016)"),
        (-1, "bad T_stride 0: smaller than a view's final-T plane (50331648)"),
        *FRAME_OF_LISTS,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
        (-2, 'workspace too small for 2 views per launch: 32256 bytes given, 64512 needed'),
    ],
    "gsr_blend_channels_backward_views": [
        (-1, 'null cameras'),
        (-1, 'null options'),
        (-1, 'bad view count 0 (1 .. 8)'),
        (-1, 'views of a launch sequence must share one frame size'),
        (-1, 'views of a launch sequence are [H,W] maps or shard strips: output_layout = 1 is not supported'),
        (-1, 'null gradient map'),
        (-1, 'null feature gradient'),
        (-1, 'bad channels 0 (1 .. 1024)'),
        (-1, 'bad grad_stride 0: rows of 17 channels overlap'),
        (-1, 'gradient maps are float32: output_dtype = 1 (bfloat16) is not supported'),
        (-1, 'feature gradients are accumulated in float32: accum_dtype = 1 (bfloat16) is not supported'),
        (-1, "bad map_stride 0: smaller than a view's gradient map (855638016)"),
        *FRAME_OF_LISTS,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
        (-2, 'workspace too small for 2 views per launch: 32256 bytes given, 64512 needed'),
    ],
    "gsr_blend_gaussian_stats_views": [
        (-1, 'null cameras'),
        (-1, 'null options'),
        (-1, 'bad view count 0 (1 .. 8)'),
        (-1, 'views of a launch sequence must share one frame size'),
        (-1, 'views of a launch sequence are [H,W] maps or shard strips: output_layout = 1 is not supported'),
        (-1, 'null statistics outputs: all four'),
        (-1, 'view_hits needs the view_bits scratch'),
        (-1, 'gaussian statistics are float32 / uint32: output_dtype = 1 (bfloat16) is not supported'),
        (-1, 'the weights are accumulated in float32: accum_dtype = 1 (bfloat16) is not supported'),
        (-1, "bad mask_stride 0: smaller than a view's mask plane (50331648)"),
        *FRAME_OF_LISTS,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
        (-2, 'workspace too small for 2 views per launch: 32256 bytes given, 64512 needed'),
    ],
    "gsr_render_channels_batch": [
        (-1, 'null scene'),
        *SCENE,
        (-1, 'null cameras'),
        (-1, 'null options'),
        (-1, 'bad camera count -1'),
        (-1, 'views of a launch sequence must share one frame size'),
        (-1, 'views of a launch sequence are [H,W] maps or shard strips: output_layout = 1 is not supported'),
        (-1, 'null features'),
        (-1, 'null output map'),
        (-1, 'bad channels 0 (1 .. 1024)'),
        (-1, 'bad feature_stride 0: rows of 17 channels overlap'),
        (-1, 'feature maps are float32: output_dtype = 1 (bfloat16) is not supported'),
        (-1, 'feature maps are accumulated in float32: accum_dtype = 1 (bfloat16) is not supported'),
        (-1, "bad map_stride 0: smaller than a view's map (855638016)"),
        (-1, "bad T_stride 0: smaller than a view's final-T plane (50331648)"),
        (-1, 'n = 2147483648 out of range [0, 2147483647]'),
        (-1, 'bad frame size 1048576x48 (1 .. 1048560 px per side)'),
        (-1, 'max_pairs = 4294959105 out of range [0, 4294959104]'),
        (-1, 'null camera/options/workspace'),
        *OPTIONS,
        (-2, 'workspace too small: 0 bytes given, 32256 needed'),
    ],
    "gsr_render_batch": [
        (-1, 'bad argument'),
        (-1, 'bad argument'),
        (-1, 'bad argument'),
        (-1, 'bad argument'),
        (-1, 'bad argument'),
        (-1, 'bad argument'),
        (-1, 'bad frame size 0x32'),
        (-1, 'views of a batch must share one frame size'),
        (-1, 'frame_stride smaller than a frame'),
        *SCENE,
        (-1, 'null camera/options/workspace'),
        (-1, 'bad frame size 1048576x48 (1 .. 1048560 px per side)'),
        (-1, 'max_pairs = 4294959105 out of range [0, 4294959104]'),
        *OPTIONS,
        (-2, 'workspace too small: 0 bytes given, 172939563520 needed'),
    ],
    "gsr_render_batch_slots": [
        (-1, 'bad argument'),
        (-1, 'bad argument'),
        (-1, 'bad argument'),
        (-1, 'bad argument'),
        (-1, 'bad argument'),
        (-1, 'bad argument'),
        (-1, 'bad argument'),
        (-1, 'bad argument'),
        (-1, 'bad argument'),
        (-1, 'bad frame size 0x32'),
        (-1, 'views of a batch must share one frame size'),
        (-1, 'frame_stride smaller than a frame'),
        (-1, 'null workspace in slot 0'),
        (-1, 'null workspace in slot 1'),
        (-1, 'slots 0 and 1 share a workspace'),
        *SCENE,
        (-1, 'bad frame size 1048576x48 (1 .. 1048560 px per side)'),
        (-1, 'max_pairs = 4294959105 out of range [0, 4294959104]'),
        *OPTIONS,
        (-2, 'workspace too small: 0 bytes given, 172939563520 needed'),
    ],
}


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_refusals_come_in_this_order(entry):
    got = peel(entry)
    assert got == EXPECTED[entry], "\n".join(f"{rc} {text}" for rc, text in got)
    assert got[-1][0] == -2 and all(rc == -1 for rc, _ in got[:-1 - (entry in SLICED)])


def test_every_entry_with_a_camera_and_a_workspace_is_peeled():
    from gsr_amd import _lib

    taking = [name for name in _lib.EXPORTS if name not in ("gsr_version", "gsr_last_error", "gsr_default_options")
              and C.POINTER(_lib.GsrCamera) in (getattr(_lib.lib, name).argtypes or ()) and C.c_size_t in getattr(_lib.lib, name).argtypes]
    assert sorted(taking) == sorted(ENTRIES) and len(ENTRIES) == 27 and sorted(EXPECTED) == sorted(ENTRIES)
