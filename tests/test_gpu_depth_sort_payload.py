"""GPU: the depth sort's 8-byte {id, rect8} payload (csrc/sort.hip, csrc/radix.h, csrc/binning.hip) and the hand-off between its
passes, held to the CPU oracle on order scenes (tests/order_scenes.py): any swapped neighbour, lost or doubled key moves a frame
beyond conftest.assert_frames_close.  The expected frame is always oracle.cpu_oracle.render on the same packed scene; GPU paths are
compared with one another bit for bit only.

What the cases aim at (the plan shapes and tile edges are those at which a narrower key format between the last two passes would
change hands — built with this payload, measured, not kept: profiles/pay8_narrow_keys_not_kept.txt — and they hold whichever pass
writes what):
  plan shapes     B = 9 (one pass: pass 0 writes the only payload buffer), 10 and 18 (two), 19 and 27 (three), 28 (9 + 7 + 7 + 5)
                  — each with the passes enqueued at the plan and above it (the surplus kernels return at once; binning finds the
                  buffer by the plan, not the bound), and one below (flagged, retried)
  tile edges      V survivors on, before and past the 8192-key tile of the passes that read the 8-byte payload
  two plans       a four-pass and a three-pass view through one launch sequence, each in its own workspace slice
  shard input     a rank's compacted (key, id, rect) records entering pass 0 (4096-key tiles: the payload staged in one round)
  wide frame      frames wider than 4096 px keep the 4-byte id payload (rects gathered by id)
"""
import numpy as np
import pytest
import torch

import order_scenes as osc
from conftest import assert_frames_close
from gpu_cases import namespace

pytestmark = pytest.mark.gpu

DEPTH_TILE = 512 * 16        # csrc/gsr_internal.h DEPTH_SORT_THREADS * DEPTH_SORT_ITEMS
TILE = 16
W, H = 640, 360              # 3600 stacks of six: 21 600 drawn gaussians, three depth-sort tiles
_ORACLE = {}                 # oracle frames per (scene, view), computed once and left unchanged


@pytest.fixture(scope="module")
def G():
    return namespace()


def _oracle(G, key, s, vi=0):
    k = (key, vi)
    if k not in _ORACLE:
        v = s.views[vi]
        img, drawn = G.orc.render(s.packed, G.orc.camera(*v.cam_args))
        assert drawn == v.n_drawn and np.isfinite(img).all(), (key, drawn, v.n_drawn)
        _ORACLE[k] = img
    return _ORACLE[k]


def _file_order(G, s, **kw):
    return G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(s.packed, spatial_order=False), **kw)


def _precondition(R, cam, s, v):
    z = R.preprocess_debug(cam)["cam_means"][:, 2].cpu().numpy()
    assert np.array_equal(z[v.drawn].view(np.uint32), s.z_cam[v.drawn].view(np.uint32)), \
        "the kernel's z_cam is not bit for bit the key the builder chose: the expected order is not defined on this device"


@pytest.mark.parametrize("B", [9, 10, 18, 19, 27, 28])
def test_plan_shapes_at_the_plan_above_it_and_one_below(G, B):
    s = osc.OrderScene(W, H, B, seed=300 + B)
    v = s.views[0]
    plan = osc.plan_passes(B)
    assert plan == {9: 1, 10: 2, 18: 2, 19: 3, 27: 3, 28: 4}[B]
    if B == 28:
        assert osc.plan_shifts(B) == [0, 9, 16, 23]                      # 9 + 7 + 7 + 5
    mk = G.renderer.make_options
    cam = G.renderer.make_camera(*v.cam_args)
    R = _file_order(G, s)
    _precondition(R, cam, s, v)
    oimg = _oracle(G, ("plan", B), s)
    img = None
    for k in range(plan, 5):                                             # at the plan, then above it
        got = R.render(cam, mk(depth_sort_passes=k)).clone()
        st = dict(R.last_stats)
        assert st["sort_passes"] == plan and st["n_visible"] == v.n_drawn and st["overflow"] == 0, (k, st)
        assert_frames_close(got.cpu().numpy(), oimg)
        assert img is None or torch.equal(got, img), k
        img = got
        assert torch.equal(R.render(cam, mk(depth_sort_passes=k, fine_binning=True)), img), k
        assert R.last_stats["sort_passes"] == plan
    assert torch.equal(R.render(cam), img)                               # the bound the class has learned
    assert R.last_stats["sort_passes"] == plan and torch.equal(R.render(cam, mk(fine_binning=True)), img)
    if plan > 1:                                                         # one below the plan: refused, and a clean frame on the retry
        with pytest.raises(G._lib.GsrSortPasses):
            R.render(cam, mk(depth_sort_passes=plan - 1))
        assert R.last_stats["sort_passes"] == plan and R.last_stats["overflow"] == 2
        assert torch.equal(R.render(cam), img) and R.last_stats["overflow"] == 0
        R2 = _file_order(G, s)                                           # a bound learned elsewhere: detected, raised inside, re-rendered
        R2.sort_passes = plan - 1
        got = R2.render(cam)
        assert R2.sort_passes == plan and R2.last_stats["sort_passes"] == plan and R2.last_stats["overflow"] == 0
        assert torch.equal(got, img)


@pytest.mark.parametrize("B", [19, 27])
@pytest.mark.parametrize("V", [5, DEPTH_TILE - 1, DEPTH_TILE, DEPTH_TILE + 1, 2 * DEPTH_TILE + 1])
def test_survivors_on_the_tile_edges_of_the_later_passes(G, V, B):
    s = osc.OrderScene(W, H, B, seed=1000 * B + V, n_drawn=V)
    v = s.views[0]
    assert v.n_drawn == V and s.n > V
    cam = G.renderer.make_camera(*v.cam_args)
    R = _file_order(G, s)
    _precondition(R, cam, s, v)
    img = R.render(cam).clone()
    assert R.last_stats["n_visible"] == V and R.last_stats["sort_passes"] == 3, R.last_stats
    assert_frames_close(img.cpu().numpy(), _oracle(G, ("V", V, B), s))
    assert torch.equal(R.render(cam, G.renderer.make_options(fine_binning=True)), img)


def test_a_four_pass_and_a_three_pass_view_in_one_launch_sequence(G):
    s = osc.OrderScene.two_sided(W, H, 28, 19, seed=11)
    scene = G.renderer.GaussianScene.from_packed(s.packed, spatial_order=False)
    cams = [G.renderer.make_camera(*v.cam_args) for v in s.views]
    R = G.renderer.Rasterizer(scene)
    singles = []
    for vi, v in enumerate(s.views):
        _precondition(R, cams[vi], s, v)
        img = R.render(cams[vi]).clone()
        assert R.last_stats["sort_passes"] == (4, 3)[vi] and R.last_stats["n_visible"] == v.n_drawn, (vi, R.last_stats)
        assert_frames_close(img.cpu().numpy(), _oracle(G, ("two", 28, 19), s, vi))
        assert torch.equal(R.render(cams[vi], G.renderer.make_options(fine_binning=True)), img), vi
        singles.append(img)
    Rb = G.renderer.Rasterizer(scene, views=2)
    for order in ((0, 1), (1, 0)):
        got = Rb.render_batch([cams[i] for i in order])
        assert [d["sort_passes"] for d in Rb.last_slice_stats] == [(4, 3)[i] for i in order]
        for k, i in enumerate(order):
            assert torch.equal(got[k], singles[i]), (order, k)


def test_rank_3_of_8_takes_its_compacted_records_through_the_sort(G):
    B, step, begin = 19, 8, 3
    W, H = 1920, 1080                                                    # one stack per tile: the rank sorts 5 760 records, two 4096-key tiles
    s = osc.OrderScene(W, H, B, seed=77, stacks_per=16)
    v = s.views[0]
    mk = G.renderer.make_options
    cam = G.renderer.make_camera(*v.cam_args)
    R = _file_order(G, s)
    _precondition(R, cam, s, v)
    img = R.render(cam).clone()
    assert R.last_stats["sort_passes"] == 3 and R.last_stats["n_visible"] == v.n_drawn
    assert_frames_close(img.cpu().numpy(), _oracle(G, ("shard", B), s))
    assert torch.equal(R.render(cam, mk(fine_binning=True)), img)
    rows = G.renderer.shard_row_list(H, begin, step, 1)
    sub = osc.order_in_rows(s, v, rows)
    assert len(rows) >= 2 and 512 * 8 < len(sub) < v.n_drawn
    for kw in (dict(), dict(fine_binning=True)):
        strip = R.render(cam, mk(tile_row_begin=begin, tile_row_step=step, output_layout=2, tile_row_block=1, shard_preprocess=2, **kw))
        assert R.last_stats["n_visible"] == len(sub) and R.last_stats["sort_passes"] == 3, R.last_stats   # explicit ids: the compact records
        for k, ty in enumerate(rows):
            h = min(TILE, H - ty * TILE)
            assert torch.equal(strip[k * TILE: k * TILE + h], img[ty * TILE: ty * TILE + h]), (kw, ty)


def test_a_frame_wider_than_4096_px_keeps_the_four_byte_payload(G):
    Ww, Hw, B = 4200, 48, 19
    s = osc.OrderScene(Ww, Hw, B, seed=5)
    v = s.views[0]
    assert v.n_drawn > DEPTH_TILE                                         # more than one tile through the id-only scatter
    cam = G.renderer.make_camera(*v.cam_args)
    R = _file_order(G, s)
    _precondition(R, cam, s, v)
    img = R.render(cam).clone()
    assert R.last_stats["sort_passes"] == 3 and R.last_stats["n_visible"] == v.n_drawn, R.last_stats
    assert_frames_close(img.cpu().numpy(), _oracle(G, ("wide", Ww, Hw, B), s))
    assert torch.equal(R.render(cam, G.renderer.make_options(fine_binning=True)), img)
