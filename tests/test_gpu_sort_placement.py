"""GPU: where the workgroups of the radix passes run must not show in the frame.

csrc/radix.h radix_tile_of: a workgroup of the hist / scatter grids takes tile (blockIdx.x & 7) * per + (blockIdx.x >> 3) with
per = ceil(live tiles / 8) taken from the count on the device, so that one XCD's workgroups own consecutive tiles; the grids are
sized by the host's bound (rounded up to a multiple of 8) and are larger than the live tiles.  What can go wrong is a tile nobody
takes or two workgroups take — when the live tiles are just under, on and just over a multiple of 8 (the last class short or
empty), or a single one — and the alignment of the classes across the views of one launch sequence.  The scenes are order scenes
(tests/order_scenes.py): any exchanged neighbours, and any lost or doubled tile, move the frame by more than
conftest.assert_frames_close allows; between GPU paths frames are compared bit for bit.
"""
import numpy as np
import pytest
import torch

import order_scenes as osc
from conftest import assert_frames_close
from gpu_cases import namespace

pytestmark = pytest.mark.gpu

DEPTH_TILE = 512 * 16         # csrc/gsr_internal.h DEPTH_SORT_THREADS * DEPTH_SORT_ITEMS: keys per workgroup of a depth-sort pass
PAIR_TILE = 256 * 16          # PAIR_SORT_THREADS * PAIR_SORT_ITEMS: the 256-thread kernels (pair sort, gsr_scene_order)
_ORACLE = {}


@pytest.fixture(scope="module")
def G():
    return namespace()


def _file_order(G, packed):
    return G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(packed, spatial_order=False))


def _z_cam_is_the_key(R, cam, z_cam, drawn):
    z = R.preprocess_debug(cam)["cam_means"][:, 2].cpu().numpy()
    assert np.array_equal(z[drawn].view(np.uint32), z_cam[drawn].view(np.uint32)), \
        "the kernel's z_cam is not bit for bit the key the builder chose: the expected order is not defined on this device"


@pytest.mark.parametrize("V", [7 * DEPTH_TILE + 1, 8 * DEPTH_TILE - 1, 8 * DEPTH_TILE, 8 * DEPTH_TILE + 1, 9 * DEPTH_TILE + 1, 5])
def test_live_depth_sort_tiles_around_a_multiple_of_eight(G, V):
    """8, 8, 8, 9, 10 and 1 live tiles in passes 1 and 2 (the V survivors of pass 0) under a grid sized by the scene's n > V.
    8 tiles: per = 1, every class holds one; 9 and 10: per = 2, classes 0-3 hold two tiles, class 4 one or two, the others none;
    1: class 0 alone.  Pass 0 itself runs over the ceil(n / 8192) tiles of the whole scene and drops the decoys' keys in each.
    B = 19 (9 + 5 + 5)."""
    W, H, B = 1920, 1080, 19
    s = osc.OrderScene(W, H, B, seed=V, n_drawn=V)
    v = s.views[0]
    assert v.n_drawn == V and s.n > V
    assert -(-V // DEPTH_TILE) == {7 * DEPTH_TILE + 1: 8, 8 * DEPTH_TILE - 1: 8, 8 * DEPTH_TILE: 8, 8 * DEPTH_TILE + 1: 9,
                                   9 * DEPTH_TILE + 1: 10, 5: 1}[V]
    cam = G.renderer.make_camera(*v.cam_args)
    R = _file_order(G, s.packed)
    _z_cam_is_the_key(R, cam, s.z_cam, v.drawn)
    img = R.render(cam)
    assert R.last_stats["n_visible"] == V and R.last_stats["sort_passes"] == 3, R.last_stats
    if ("V", V) not in _ORACLE:
        oimg, drawn = G.orc.render(s.packed, G.orc.camera(*v.cam_args))
        assert drawn == V
        _ORACLE[("V", V)] = oimg
    assert_frames_close(img.cpu().numpy(), _ORACLE[("V", V)])
    assert torch.equal(R.render(cam, G.renderer.make_options(fine_binning=True)), img)


def test_two_views_in_one_launch_sequence_keep_their_tiles(G):
    """Both cameras of a two-sided scene, 8 * 8192 + 1 drawn gaussians each (9 live tiles, per = 2), in one launch sequence
    (gridDim.y = 2): the grid's x extent is rounded up to a multiple of 8 so that view 1's workgroup classes start where view 0's
    do, and every view takes its own count.  Bit for bit the single-view frames, which are the oracle's."""
    W, H, V = 1920, 1080, 8 * DEPTH_TILE + 1
    s = osc.OrderScene.two_sided(W, H, 19, 19, seed=V, n_drawn=V)
    scene = G.renderer.GaussianScene.from_packed(s.packed, spatial_order=False)
    cams = [G.renderer.make_camera(*v.cam_args) for v in s.views]
    R = G.renderer.Rasterizer(scene)
    singles = []
    for vi, v in enumerate(s.views):
        assert v.n_drawn == V
        _z_cam_is_the_key(R, cams[vi], s.z_cam, v.drawn)
        img = R.render(cams[vi]).clone()
        assert R.last_stats["n_visible"] == V and R.last_stats["sort_passes"] == 3, (vi, R.last_stats)
        oimg, drawn = G.orc.render(s.packed, G.orc.camera(*v.cam_args))
        assert drawn == V
        assert_frames_close(img.cpu().numpy(), oimg)
        singles.append(img)
    assert not torch.equal(singles[0], singles[1])
    Rb = G.renderer.Rasterizer(scene, views=2)
    assert torch.equal(Rb.render_batch(cams), torch.stack(singles))
    assert [d["n_visible"] for d in Rb.last_slice_stats] == [V, V]
    assert torch.equal(Rb.render_batch(cams[::-1]), torch.stack(singles[::-1]))


@pytest.mark.parametrize("n", [1, 8 * PAIR_TILE - 1, 8 * PAIR_TILE, 8 * PAIR_TILE + 1, 9 * PAIR_TILE + 5])
def test_scene_order_on_tile_counts_around_a_multiple_of_eight(G, n):
    """gsr_scene_order: sixteen passes of the 256-thread kernels with the count on the HOST side (n_dev = nullptr: live tiles = the
    grid's bound, here 1, 8, 8, 9 and 10 tiles of 4096).  Means from a 7 x 5 x 3 grid: thousands of equal coordinates per axis and
    of equal Morton codes, so a pass that is not stable — or a tile written to another tile's place — changes the permutation."""
    rng = np.random.default_rng(n)
    means = np.stack([rng.integers(0, 7, n), rng.integers(0, 5, n), rng.integers(0, 3, n)], 1).astype(np.float32) * np.float32(0.25) - 1
    want = G.renderer.morton_order(means)
    got = G.renderer.scene_order(torch.from_numpy(means).cuda()).cpu().numpy()
    assert np.array_equal(got, want)
