"""CPU: the order scenes (tests/order_scenes.py) do what they claim — proved with the oracle alone, no kernel involved.

tests/test_gpu_draw_order.py compares GPU frames of these scenes with the oracle's through conftest.assert_frames_close, which lets
a sample sit 4.5e-3 off.  That pins the draw order only if every wrong order moves some sample by MORE than twice that (the GPU
frame may itself sit 4.5e-3 from the oracle): the sensitivity condition below, 9e-3, asserted for every adjacent transposition of
every stack.  The rest checks that the scene is what the builder says: depths bit for bit the chosen keys, the oracle's own order
equal to the builder's numpy order, every stack drawn, no decoy drawn, and the key populations covering every bit and every pass
boundary of the depth sort's plan.
"""
import numpy as np
import pytest

import order_scenes as osc
from conftest import assert_frames_close

W, H = 320, 192
BS = (1, 9, 10, 18, 19, 27, 28, 29)     # plans 9 | 9 | 9+1 | 9+9 | 9+5+5 | 9+9+9 | 9+7+7+5 | 9+7+7+6 (29: as far as fp32 covariances stay finite)
NEED = 2 * 4.5e-3                       # conftest.assert_frames_close: no sample off by more than 4.5e-3, on either side of the truth
THREADS = 8


def _check_view(orc, s, v, where):
    """Everything the issue asks of one (scene, camera); returns the smallest change any adjacent transposition makes."""
    Wd, Hd = s.W, s.H
    cam = orc.camera(*v.cam_args)
    pre = orc.preprocess(s.packed, cam)
    zc = pre["cam_means"][:, 2]
    assert np.array_equal(zc[v.drawn].view(np.uint32), s.z_cam[v.drawn].view(np.uint32)), f"{where}: z_cam is not the chosen key"
    # the rest (decoys, the other camera's half): +-z bit for bit as well
    other = ~v.drawn
    assert np.array_equal(np.abs(zc[other]).view(np.uint32), np.abs(s.packed["means"][other, 2]).view(np.uint32)), where
    oo = orc.depth_order(pre["cam_means"])
    assert np.array_equal(oo[v.drawn[oo]], v.expected_order), f"{where}: the oracle's depth order is not the builder's"
    screen, _, drawn = orc.composite(v.expected_order, pre, Wd, Hd, threads=THREADS)
    img, n_render = orc.render(s.packed, cam)
    assert drawn == n_render == v.n_drawn, (where, drawn, n_render, v.n_drawn)          # every member drawn, no decoy drawn
    assert np.isfinite(img).all(), where
    assert np.array_equal(img, screen.transpose(1, 0, 2)), f"{where}: render != composite(expected order)"
    worst = np.inf
    for j in range(s.L - 1):
        swapped, _, _ = orc.composite(osc.transposed(s, v, j), pre, Wd, Hd, threads=THREADS)
        stacks, change = osc.stack_change(s, v, screen, swapped, j)
        assert len(stacks) > 0, (where, j)
        low = stacks[change <= NEED]
        assert len(low) == 0, f"{where}: transposing ranks {j},{j + 1} is not visible enough in stacks {low[:10]} ({change.min():.4f})"
        worst = min(worst, float(change.min()))
    # every stack was part of that: each has all its members in this view's order
    ids, counts = np.unique(s.stack_of[v.expected_order], return_counts=True)
    assert np.array_equal(counts, s.stack_size[ids]) and (counts >= 2).all(), where
    return worst


def _coverage(s):
    """From the offsets alone: every bit below B is the ONLY differing bit of some adjacent pair of some stack whose array order is
    against its depth order (a sort that drops the bit leaves the pair in array order: wrong, and visible); every pass boundary of
    the plan lies inside a carry stack ((m << shift) - 1 and m << shift are neighbours in it); every population that fits B is there."""
    v = s.views[0]
    order = v.expected_order
    by_stack = {}
    for g in order:
        by_stack.setdefault(int(s.stack_of[g]), []).append(int(s.offset[g]))
    ids = {}
    for g in order:
        ids.setdefault(int(s.stack_of[g]), []).append(int(g))
    bits, against, boundaries = set(), set(), set()
    for st, offs in by_stack.items():
        assert offs == sorted(offs)
        for k, (a, b) in enumerate(zip(offs, offs[1:])):
            x = a ^ b
            if x and x & (x - 1) == 0:
                bits.add(x.bit_length() - 1)
                if ids[st][k] > ids[st][k + 1]:                     # drawn first, stored later: a sort that loses this bit shows
                    against.add(x.bit_length() - 1)
            if s.pop[st] == "carry" and b == a + 1:
                for sh in osc.plan_shifts(s.B)[1:]:
                    if b & ((1 << sh) - 1) == 0:
                        boundaries.add(sh)
    assert bits == set(range(s.B)), (s.B, sorted(set(range(s.B)) - bits))
    assert against == set(range(s.B)), (s.B, sorted(set(range(s.B)) - against))
    assert boundaries == set(osc.plan_shifts(s.B)[1:]), (s.B, boundaries)
    assert set(s.pop) == {p for p in osc.POPS if s.B >= osc.FITS_FROM[p]}, (s.B, set(s.pop))
    assert s.offset[v.drawn].max() == (1 << s.B) - 1 and s.offset[v.drawn].min() == 0          # the plan is fixed by construction
    assert set(np.unique(s.decoy_kind)) == {-1, 0, 1, 2}                                        # all three kinds of decoy


@pytest.mark.parametrize("B", BS)
def test_small_stacks_show_every_adjacent_swap(B):
    from oracle import cpu_oracle as orc

    s = osc.OrderScene(W, H, B, seed=3)
    assert s.n_stacks == (W // 8) * (H // 8) and s.n_drawn == 6 * s.n_stacks and s.n > s.n_drawn
    worst = _check_view(orc, s, s.views[0], f"B={B}")
    _coverage(s)
    print(f"\nsmall stacks {W}x{H} B={B}: {s.n_stacks} stacks, {s.n} gaussians ({s.n - s.n_drawn} decoys), plan {osc.plan_shifts(B)}, "
          f"minimum adjacent-swap change {worst:.4f} (needed > {NEED})")
    again = osc.OrderScene(W, H, B, seed=3)
    assert all(np.array_equal(again.packed[k], s.packed[k]) for k in s.packed) and np.array_equal(again.expected_order, s.expected_order)
    other = osc.OrderScene(W, H, B, seed=4)
    assert not np.array_equal(other.packed["means"], s.packed["means"])


@pytest.mark.parametrize("Wd,Hd,B", [(W, H, b) for b in BS] + [(640, 384, b) for b in (9, 19, 28)])
def test_wide_stacks_show_every_adjacent_swap(Wd, Hd, B):
    from oracle import cpu_oracle as orc

    s = osc.OrderScene(Wd, Hd, B, seed=3, wide=True)
    assert s.n_stacks == (Wd // 128) * (Hd // 128)
    worst = _check_view(orc, s, s.views[0], f"wide {Wd}x{Hd} B={B}")
    # every member covers several 32x32 cells both ways: the reference's rect is at least 4 tiles wide and high
    tb = orc.preprocess(s.packed, orc.camera(*s.cam_args))["tile_bboxes"][s.views[0].drawn]
    assert ((tb[:, 2] - tb[:, 0]) >= 4).all() and ((tb[:, 3] - tb[:, 1]) >= 4).all()
    print(f"\nwide stacks {Wd}x{Hd} B={B}: {s.n_stacks} stacks, minimum adjacent-swap change {worst:.4f} (needed > {NEED})")


@pytest.mark.parametrize("Bf,Bb", [(9, 28), (28, 9), (1, 19)])
def test_two_sided_scene_through_both_cameras(Bf, Bb):
    from oracle import cpu_oracle as orc

    s = osc.OrderScene.two_sided(W, H, Bf, Bb, seed=5)
    front, back = s.views
    assert (front.B, back.B) == (Bf, Bb) and not (front.drawn & back.drawn).any()
    assert front.n_drawn == back.n_drawn == 6 * (W // 8) * (H // 8)
    for name, v in (("front", front), ("back", back)):
        worst = _check_view(orc, s, v, f"two-sided ({Bf},{Bb}) {name}")
        print(f"\ntwo-sided ({Bf},{Bb}) {name} camera: minimum adjacent-swap change {worst:.4f} (needed > {NEED})")
    again = osc.OrderScene.two_sided(W, H, Bf, Bb, seed=5)
    assert all(np.array_equal(again.packed[k], s.packed[k]) for k in s.packed)


def test_one_transposition_in_one_stack_fails_assert_frames_close():
    """What makes the GPU tests bite, shown without a GPU: a frame composited in an order with ONE adjacent pair of ONE stack
    transposed is refused by the very function the GPU tests use, against the very frame they use."""
    from oracle import cpu_oracle as orc

    rng = np.random.default_rng(0)
    for B, wide in ((19, False), (28, False), (1, False), (19, True)):
        s = osc.OrderScene(W, H, B, seed=3, wide=wide)
        v = s.views[0]
        pre = orc.preprocess(s.packed, orc.camera(*v.cam_args))
        true, _, _ = orc.composite(v.expected_order, pre, W, H, threads=THREADS)
        assert_frames_close(true, true)
        for _ in range(12):
            p = int(rng.integers(0, len(v.expected_order)))
            g = v.expected_order[p]
            st, r = s.stack_of[g], s.rank[g]
            if r + 1 >= s.stack_size[st]:
                continue
            q = int(np.nonzero((s.stack_of[v.expected_order] == st) & (s.rank[v.expected_order] == r + 1))[0][0])
            wrong = v.expected_order.copy()
            wrong[p], wrong[q] = wrong[q], wrong[p]
            frame, _, _ = orc.composite(wrong, pre, W, H, threads=THREADS)
            with pytest.raises(AssertionError):
                assert_frames_close(frame, true)


def test_size_knobs():
    """The number drawn lands exactly where asked; tie stacks straddle the asked positions of the expected order; decoys fall into
    every 8192-key tile of the array (what pass 0 of the depth sort reads) at the sizes the GPU tests use."""
    for V in (1, 2, 63, 64, 65, 3 * 8192 - 1, 3 * 8192, 3 * 8192 + 1):
        s = osc.OrderScene(960, 540, 19, seed=V, n_drawn=V)
        assert s.n_drawn == V == len(s.expected_order) and s.n > V
        assert s.offset[s.views[0].drawn].max() == (1 << 19) - 1
        if V > 1:
            assert s.offset[s.views[0].drawn].min() == 0
    at = (4096, 8192, 3 * 4096, 2 * 8192)
    s = osc.OrderScene(960, 540, 28, seed=9, tie_at=at)
    o = s.expected_order
    for p in at:
        assert s.offset[o[p - 1]] == s.offset[o[p]] and s.stack_of[o[p - 1]] == s.stack_of[o[p]] and s.pop[s.stack_of[o[p]]] == "tie"
        assert o[p - 1] < o[p]                                     # ties in array order
    s = osc.OrderScene(1920, 1080, 19, seed=1)
    assert s.n_stacks == 240 * 135
    dec = s.stack_of < 0
    for t in range(0, s.n, 8192):
        assert dec[t:t + 8192].any() and not dec[t:t + 8192].all()
    # tile stacks: one per 16x16 tile
    s = osc.OrderScene(W, H, 19, seed=2, stacks_per=16)
    assert s.n_stacks == (W // 16) * (H // 16)


def _shard_rows(height, begin, step, block):
    """renderer.shard_row_list, restated (the GPU test asserts they agree): blocks of `block` tile rows, block b is shard b % step's."""
    return [t for t in range((height + 15) // 16) if (t // block) % step == begin]


SHARD_TILE = 512 * 8   # csrc/gsr_internal.h DEPTH_SORT_THREADS * DEPTH_SORT_ITEMS_SHARD: keys per workgroup of a shard's compact-record sort


@pytest.mark.parametrize("B,step,block,begin", [(28, 2, 1, 1), (19, 2, 2, 0), (28, 8, 2, 3)])
def test_tie_stacks_straddle_the_tiles_of_a_shards_own_sort(B, step, block, begin):
    """A tile-row shard sorts only the gaussians that touch its rows, so positions in ITS sorted order are what its sort tiles
    cut.  With one stack per 16x16 tile every stack lies in one tile row; the tie stacks' equal keys hold positions p - 1, p, p + 1
    of the expected order restricted to the shard's rows, for every multiple p of the shard sort's tile that the shard reaches."""
    Wd, Hd = 1920, 1080
    rows = _shard_rows(Hd, begin, step, block)
    n_strip = 6 * (Wd // 16) * len([t for t in rows if 16 * t + 8 <= Hd - 3])
    at = tuple(range(SHARD_TILE, n_strip - 6, SHARD_TILE))
    assert len(at) >= 1
    s = osc.OrderScene(Wd, Hd, B, seed=50 + step, stacks_per=16, tie_at=at, tie_rows=rows)
    v = s.views[0]
    sub = osc.order_in_rows(s, v, rows)
    assert len(sub) == n_strip and len(sub) < v.n_drawn
    for p in at:
        assert s.offset[sub[p - 1]] == s.offset[sub[p]] == s.offset[sub[p + 1]] and sub[p - 1] < sub[p] < sub[p + 1]
        assert s.stack_of[sub[p - 1]] == s.stack_of[sub[p]] and s.pop[s.stack_of[sub[p]]] == "tie"
        assert osc.stack_tile_row(s.centres)[s.stack_of[sub[p]]] in rows
    # and the oracle's screen means agree on which gaussians reach the shard's rows: REACH pixels around a mean (more than any
    # footprint) stay inside one tile row, in the shard's rows for the subsequence and outside them for every other stack
    from oracle import cpu_oracle as orc

    pre = orc.preprocess(s.packed, orc.camera(*v.cam_args))
    outside = v.drawn.copy()
    outside[sub] = False
    my = pre["screen_means"][:, 1]
    lo, hi = np.floor(my - osc.REACH).astype(int) >> 4, np.floor(my + osc.REACH).astype(int) >> 4
    assert not np.isin(lo[outside], rows).any() and not np.isin(hi[outside], rows).any()
    assert np.isin(lo[sub], rows).all() and np.array_equal(lo[sub], hi[sub])
