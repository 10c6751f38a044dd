"""GPU: frames at and past the geometry limits where binning and the pair sort change kernels.

The binning / pair-sort stage picks its kernels from the frame's tile grid (api.hip plan_frame fills gsr_internal.h FramePlan;
launch_binning, launch_pair_sort and launch_blend read it):
  - the tile rect rides through the depth sort packed as 4 x u8 while tiles_x, tiles_y <= 256, and is gathered by id past that;
  - with the packed rect, pairs are (gaussian, 32x32 cell) pairs (coarse binning), otherwise (gaussian, 16x16 tile) pairs;
  - pair keys are (row << bits_x) | column with one spare row value for culled pairs: 2 bytes while bits_x + bits_y <= 16,
    4 bytes past that, and ceil(key_bits / 8) radix passes whose parity decides which ping-pong buffer holds the lists.
The bench-size frames reach only the 2-byte-key paths.  Every case below is held to the CPU oracle (frame and transmittance),
shows content past the limit it is aimed at, shows its binning path from outside (n_pairs_bbox of the default and of the
fine_binning = 1 frame), and carries bit-identity checks of the options that have kernels of their own on that path.
"""
import dataclasses
from typing import Tuple

import numpy as np
import pytest
import torch

from conftest import assert_frames_close, psnr
from gpu_cases import namespace

pytestmark = pytest.mark.gpu

TILE = 16
MAX_SIDE = 65535 * TILE  # include/gsr.h GSR_MAX_FRAME_SIDE: tile rects are ushort4


def _ceil_log2(v):
    bits = 0
    while (1 << bits) < v:
        bits += 1
    return bits


def _path(W, H, fine_binning=False):
    """The kernel choice of the binning and pair-sort stage for a W x H frame, restated from the C++ (ordinary scene sizes:
    n <= 2^28)."""
    tiles_x, tiles_y = -(-W // TILE), -(-H // TILE)
    packed = tiles_x <= 256 and tiles_y <= 256               # FramePlan.packed_rect
    coarse = packed and not fine_binning                     # FramePlan.coarse (+ n <= 2^28): opts.fine_binning == 0
    grid_x = (tiles_x + 1) // 2 if coarse else tiles_x       # FramePlan.grid_x / grid_y: 32x32 cells or 16x16 tiles
    grid_y = (tiles_y + 1) // 2 if coarse else tiles_y
    bits_x = max(1, _ceil_log2(grid_x))
    bits_y = max(1, _ceil_log2(grid_y + 1))                  # one spare row value marks culled pairs (drop_from = grid_y << bits_x)
    key_bits = bits_x + bits_y
    return dict(packed=packed, coarse=coarse, bits_x=bits_x, bits_y=bits_y, key_bits=key_bits,
                key16=key_bits <= 16,                        # FramePlan.key16
                pair_passes=(key_bits + 7) // 8,             # FramePlan.pair_passes: 8-bit digits; the lists end in pval[lists_buf = passes & 1]
                drop_from=grid_y << bits_x, tiles_x=tiles_x, tiles_y=tiles_y, n_tiles=tiles_x * tiles_y)


@dataclasses.dataclass(frozen=True)
class Case:
    W: int
    H: int
    fine: bool                         # GsrOptions.fine_binning of the frame held to the oracle
    expect: Tuple[bool, bool, int, int]  # (packed, coarse, key bits, pair passes) this case is aimed at
    n: int = 100_000
    shift: float = 1.0                 # added to every log-scale: footprints large enough to reach the frame's far tiles
    checks: Tuple[str, ...] = ()       # bit-identity checks on the same frame (see test_frame_past_a_geometry_limit)


CASES = {
    "A_4081x64": Case(4081, 64, False, (True, True, 9, 2), checks=("fine_equals_coarse",)),            # tile column 255 holds one pixel
    "A_4096x64": Case(4096, 64, False, (True, True, 9, 2), checks=("fine_equals_coarse", "blend_impl")),  # rect8 column field at 255
    "B_4097x64": Case(4097, 64, False, (False, False, 12, 2), checks=("blend_impl", "no_order_hint")),   # first column past the packed rect
    "C_64x4096": Case(64, 4096, False, (True, True, 9, 2), checks=("fine_equals_coarse", "layout")),     # rect8 row field at 255; bits_y = 8
    "D_64x4097": Case(64, 4097, False, (False, False, 11, 2),                                         # > 256 tile rows; 1028 tiles
                      checks=("saturation_rule", "bf16", "no_order_hint", "shards8x2", "batch3")),
    "E_4096x2032": Case(4096, 2032, True, (True, False, 15, 2), checks=("blend_impl",)),                # below the key-width edge
    "F_4096x2033": Case(4096, 2033, True, (True, False, 16, 2), checks=("saturation_rule", "layout")),  # 16 bits: 2-byte keys, drop row 32768
    "G_4096x4096_fine": Case(4096, 4096, True, (True, False, 17, 3),                                  # 4-byte keys with packed rects
                             checks=("fine_equals_coarse", "blend_impl", "no_order_hint", "draw_limit")),
    "G_4096x4096": Case(4096, 4096, False, (True, True, 15, 2)),
    "H_4200x2100": Case(4200, 2100, False, (False, False, 17, 3),                                     # wide + 4-byte keys
                        checks=("saturation_rule", "layout", "bf16", "shards3", "batch3", "draw_limit")),
    "I_2100x4200": Case(2100, 4200, False, (False, False, 17, 3),                                     # tall + 4-byte keys
                        checks=("blend_impl", "no_order_hint", "saturation_rule", "layout", "bf16", "shards8x2", "batch3")),
    "J_7680x4320": Case(7680, 4320, False, (False, False, 18, 3),                                     # 8K: 129 600 tiles
                        checks=("no_order_hint", "blend_impl", "bf16")),
    "K_1048560x16": Case(MAX_SIDE, 16, False, (False, False, 17, 3), n=60_000, shift=1.5,             # the ABI's widest frame
                         checks=("no_order_hint", "blend_impl")),
    "K_16x1048560": Case(16, MAX_SIDE, False, (False, False, 17, 3), n=60_000, shift=1.5,             # the ABI's tallest frame
                         checks=("saturation_rule",)),
}

# Every row of the path table must keep an oracle-parity case: if a threshold moves, a case must be re-aimed, not drift to another path.
ROWS = {
    "coarse (cells), 2-byte keys": lambda c, p: p["coarse"] and p["key16"],
    "packed rect, fine, 2-byte keys": lambda c, p: p["packed"] and not p["coarse"] and p["key16"],
    "gathered rect, fine, 2-byte keys": lambda c, p: not p["packed"] and p["key16"],
    "key bits == 16 (drop row at bit 15)": lambda c, p: p["key_bits"] == 16,
    "packed rect, fine, 4-byte keys, 3 passes": lambda c, p: p["packed"] and not p["key16"] and p["pair_passes"] == 3,
    "gathered rect, 4-byte keys, 3 passes": lambda c, p: not p["packed"] and not p["key16"] and p["pair_passes"] == 3,
    "rect8 column field at 255": lambda c, p: p["packed"] and p["tiles_x"] == 256,
    "rect8 row field at 255": lambda c, p: p["packed"] and p["tiles_y"] == 256,
    "> 256 tile rows": lambda c, p: p["tiles_y"] > 256,
    "> 65 536 tiles": lambda c, p: p["n_tiles"] > 65536,
    "widest frame": lambda c, p: c.W == MAX_SIDE,
    "tallest frame": lambda c, p: c.H == MAX_SIDE,
}
for _id, _c in CASES.items():
    _p = _path(_c.W, _c.H, _c.fine)
    assert (_p["packed"], _p["coarse"], _p["key_bits"], _p["pair_passes"]) == _c.expect, (_id, _p)
for _row, _hit in ROWS.items():
    assert any(_hit(_c, _path(_c.W, _c.H, _c.fine)) for _c in CASES.values()), f"no case on the path-table row {_row!r}"
# the 32-bit-key row and the > 256-tile-rows row each carry a shard and a batch check
for _row in ("gathered rect, 4-byte keys, 3 passes", "> 256 tile rows"):
    for _kind in ("shards", "batch"):
        assert any(_hit and any(k.startswith(_kind) for k in _c.checks)
                   for _c in CASES.values() for _hit in [ROWS[_row](_c, _path(_c.W, _c.H, _c.fine))]), (_row, _kind)
assert _path(4096, 2033, True)["drop_from"] == 32768


@pytest.fixture(scope="module")
def G():
    return namespace()


def _columns(c, seed=12):
    from gsr_amd import synthetic

    cols = synthetic.mip360_like(c.n, seed)
    for i in range(3):
        cols[f"scale_{i}"] = (cols[f"scale_{i}"] + np.float32(c.shift)).astype(np.float32)
    return cols


def _camera_args(c, eye=(0.0, -2.0, 0.1)):
    """Close to the foreground blob (the wide test's trick), 100 degrees across the frame's long side; a tall frame turns the camera on
    its side so that its long axis runs along the blob's long one."""
    from gsr_amd import synthetic

    p = synthetic.look_at_pose(eye, (0, 0, 0), 1, "g.png", world_up=(1.0, 0.0, 0.0) if c.H > c.W else (0.0, 0.0, 1.0))
    f = synthetic.pinhole_focal(max(c.W, c.H), 100.0)
    return (p.qvec, p.tvec, 2 * f, 2 * f, 2 * c.W, 2 * c.H, c.W, c.H)


def _reassembles(G, R, cam, opts, step, block):
    """Tile-row shards (output_layout = 2) put back where their rows belong == the whole frame."""
    mk = G.renderer.make_options
    full = R.render(cam, mk(**opts))
    out = torch.zeros_like(full)
    for r in range(step):
        strip = R.render(cam, mk(tile_row_begin=r, tile_row_step=step, output_layout=2, tile_row_block=block, **opts))
        for k, ty in enumerate(G.renderer.shard_row_list(cam.height, r, step, block)):
            h = min(TILE, cam.height - ty * TILE)
            out[ty * TILE: ty * TILE + h] = strip[k * TILE: k * TILE + h]
    return torch.equal(out, full) and bool(full.any())


@pytest.mark.parametrize("case_id", list(CASES))
def test_frame_past_a_geometry_limit(G, case_id):
    c = CASES[case_id]
    p = _path(c.W, c.H, c.fine)
    mk = G.renderer.make_options
    base = dict(fine_binning=c.fine)
    cols = _columns(c)
    args = _camera_args(c)
    cam, ocam = G.renderer.make_camera(*args), G.orc.camera(*args)
    packed = G.utils.pack_gaussians(cols)
    scene = G.renderer.GaussianScene.from_columns(cols)
    R = G.renderer.Rasterizer(scene)

    # oracle parity: frame and final transmittance.  T is held to the frame's bar, not to test_degenerate_inputs' 1e-5 everywhere: the
    # `alpha > 1/255` step (conftest.assert_frames_close) flips for the odd pixel of a frame of millions, and a flipped gaussian of
    # alpha ~ 1/255 moves T by T / 255.  Measured: at most 18 pixels of a frame off by more than 1e-5, by up to 7e-4 (J_7680x4320), and
    # the two binnings of G_4096x4096 (2- and 4-byte keys) leave the very same T
    img, T = R.render(cam, mk(**base), return_T=True)
    st = dict(R.last_stats)
    oimg, oT, _ = G.orc.render(packed, ocam, want_T=True)
    a, t = img.cpu().numpy(), T.cpu().numpy()
    assert_frames_close(a, oimg)
    assert_frames_close(t, oT)
    dT = np.abs(t.astype(np.float64) - oT)
    print(f"\n{case_id}: {c.W}x{c.H} {p} PSNR vs oracle {psnr(a, oimg):.1f} dB (T: {psnr(t, oT):.1f} dB, {int((dT > 1e-5).sum())} px "
          f"off by > 1e-5, max {dT.max():.2e}), stats {st}")

    # not vacuous: content in the last tile row and column, and past the 4096-px packed-rect limit where the frame reaches it.  The
    # reference never draws pixel column W-1 / row H-1 (GsrOptions.reference_compat), which is all that 4081, 4097 px leave in the
    # last tile: there the non-compat frame (the same frame plus that column and row) must show it
    assert st["n_pairs"] > 0 and st["overflow"] == 0
    b = R.render(cam, mk(reference_compat=False, **base))
    assert torch.equal(b[:-1, :-1], img[:-1, :-1])
    b = b.cpu().numpy()
    assert b[(p["tiles_y"] - 1) * TILE:].any() and b[:, (p["tiles_x"] - 1) * TILE:].any()
    if c.W > 4096:
        assert b[:, 4096:].any()
    if c.H > 4096:
        assert b[4096:].any()
    if c.W % TILE != 1:
        assert a[:, (p["tiles_x"] - 1) * TILE:].any()
    if c.H % TILE != 1:
        assert a[(p["tiles_y"] - 1) * TILE:].any()

    # the path seen from outside: D counts cell pairs where the frame bins coarsely by default, tile pairs otherwise
    R.render(cam)
    d_default = R.last_stats["n_pairs_bbox"]
    R.render(cam, mk(fine_binning=True))
    d_fine = R.last_stats["n_pairs_bbox"]
    if _path(c.W, c.H)["coarse"]:
        assert d_default != d_fine, (d_default, d_fine)
    else:
        assert d_default == d_fine, (d_default, d_fine)

    for check in c.checks:
        if check == "fine_equals_coarse":
            other, oT2 = R.render(cam, mk(fine_binning=not c.fine), return_T=True)
            assert torch.equal(other, img) and torch.equal(oT2, T), check
        elif check == "blend_impl":
            assert torch.equal(R.render(cam, mk(blend_impl=1, **base)), img), check
        elif check == "saturation_rule":
            assert torch.equal(R.render(cam, mk(saturation_rule=1, **base)), img), check
        elif check == "no_order_hint":
            assert torch.equal(R.render(cam, mk(no_order_hint=True, **base)), img), check
        elif check == "layout":
            assert torch.equal(R.render(cam, mk(output_layout=1, **base)).permute(1, 0, 2), img), check
        elif check == "bf16":
            got = R.render(cam, mk(output_bf16=True, **base))
            assert got.dtype == torch.bfloat16 and torch.equal(got, img.to(torch.bfloat16)), check
        elif check == "shards3":
            assert _reassembles(G, R, cam, base, 3, 1), check
        elif check == "shards8x2":  # ranks of 5+ shards: the three-phase shard preprocess, here with gathered rects
            assert _reassembles(G, R, cam, base, 8, 2), check
        elif check == "batch3":  # three poses through one launch sequence: view slices of the workspace
            cams = [G.renderer.make_camera(*_camera_args(c, eye)) for eye in ((0.0, -2.0, 0.1), (0.06, -2.0, 0.12), (-0.05, -2.05, 0.08))]
            singles = torch.stack([R.render(k, mk(**base)) for k in cams])
            batch = G.renderer.Rasterizer(scene, views=3).render_batch(cams, mk(**base))
            assert torch.equal(batch, singles) and not torch.equal(singles[0], singles[1]), check
        elif check == "draw_limit":  # a progressive prefix against the oracle's loop stopped after k drawn gaussians
            pre = G.orc.preprocess(packed, ocam)
            order = G.orc.depth_order(pre["cam_means"])
            k = st["n_visible"] // 3
            screen, _, drawn = G.orc.composite(order, pre, c.W, c.H, limit=k, threads=G.orc.max_threads())
            prog = R.render(cam, mk(draw_limit=k, **base)).cpu().numpy()
            assert drawn == k and prog.any() and not np.array_equal(prog, a)
            assert_frames_close(prog, screen.transpose(1, 0, 2))
        else:
            raise AssertionError(f"unknown check {check}")
