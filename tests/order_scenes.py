"""Deterministic scenes on which the draw ORDER is visible in the frame, bit by chosen bit (tests/test_order_scenes.py proves it on
the CPU, tests/test_gpu_draw_order.py holds the kernels to it).

Camera at the origin looking along +z (qvec = (1,0,0,0), tvec = 0): z_cam = z exactly, so the builder chooses every depth key:
z = the float32 whose bits are bits(0.2f) + offset.  The camera turned half round about y (qvec = (0,0,1,0)) gives z_cam = -z,
equally exact (`sign = -1`, and the two halves of OrderScene.two_sided).

A scene is made of STACKS: L = 6 small isotropic gaussians (sigma ~1.5 px, opacity 0.5, SH degree-0 term only) on one pixel, one
stack per block of the frame (8x8 quadrants by default), the members coloured pure red / green / blue BY THEIR RANK in the stack's
expected draw order.  Transposing two neighbours of a stack moves a pixel of its block by alpha^2 (1 - alpha)^k |c_a - c_b|: 0.0219
at worst (k = 4, the pixel where alpha ~ 1/3), against the 4.5e-3 conftest.assert_frames_close allows a sample.  What a passing
frame shows is therefore: no two NEIGHBOURS of any stack are exchanged.  It does not show more: the members of a stack differ only
in depth and colour and the colours repeat every three ranks, so a permutation that keeps a stack's colour sequence (ranks j and
j + 3 exchanged) leaves the frame as it is.

Every stack draws its six key offsets (in [0, 2^B - 1]) from one population, listed in ARRAY-INDEX order:
  ladder  six consecutive ulps, array order opposite to depth order
  bit     three pairs {v | 1 << b, v}: array order against depth order; b runs over every bit below B across the scene's bit stacks
  carry   (d << s) + (-2 .. +3); s runs over the pass shifts of the depth sort's plan for B, then every other bit position
  tie     v, v, v+1, v+1, v-1, v: exact ties (drawn in array order) with 1-ulp neighbours, index order against depth order
  random  uniform over the span
  zero    offsets 5 .. 0: z = 0.2f exactly (the cull plane keeps z >= 0.2) and the ulps above it
One drawn gaussian carries offset 2^B - 1 and one carries 0, so the frame's key range (and with it the sort's plan) is fixed by
construction.  DECOYS that must not be drawn — whole stacks at 0.2f - 1 ulp, at negative depth, and far outside the frustum, pure
white, on pixels that real stacks occupy — are scattered through the array, so that pass 0 of the depth sort drops keys inside
every one of its tiles.

`wide=True`: one stack per 128x128 block, sigma ~20 px: every member covers several 32x32 cells both ways and emits a dozen
pairs or more, so the pair sort's stability and the cell lists' tile masks carry the order.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np

BASE = 0x3E4CCCCD                 # bits(0.2f): csrc/radix.h DEPTH_KEY_BASE
DIGIT = 9                         # csrc/radix.h DEPTH_DIGIT_BITS
SH_C0 = 0.28209479177387814
POPS = ("ladder", "bit", "carry", "tie", "random", "zero")
FITS_FROM = {"ladder": 3, "bit": 1, "carry": 4, "tie": 2, "random": 1, "zero": 3}   # smallest B whose span holds the population
Q_FRONT, Q_BACK = (1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0)


def plan_shifts(B: int) -> List[int]:
    """Shift of every pass of the depth sort's plan for a frame whose largest key offset has B bits (sort.hip
    radix_rowscan_kernel, radix.h resolve_pass, restated): 9 bits first, the rest split evenly over as few passes as possible."""
    rest = max(B - DIGIT, 0)
    rest_passes = -(-rest // DIGIT)
    per = -(-rest // rest_passes) if rest_passes else 0
    return [0] + [DIGIT + i * per for i in range(rest_passes)]


def plan_passes(B: int) -> int:
    return len(plan_shifts(B))


def camera_args(W: int, H: int, q=Q_FRONT):
    f = W / (2.0 * math.tan(math.radians(30.0)))
    return (np.array(q, np.float64), np.zeros(3), 2.0 * f, 2.0 * f, 2 * W, 2 * H, W, H), f


class View:
    """One camera of a scene: its arguments, the sign of z_cam / z, the key bit length B of what it draws, the expected draw order
    (array indices, stable by key bits then index, drawn gaussians only) and the expected z_cam of every drawn gaussian."""

    def __init__(self, cam_args, sign, B, expected_order, drawn):
        self.cam_args, self.sign, self.B = cam_args, sign, B
        self.expected_order = expected_order
        self.drawn = drawn                       # bool per gaussian
        self.n_drawn = int(drawn.sum())


def _expected(z: np.ndarray, drawn: np.ndarray, sign: int) -> np.ndarray:
    idx = np.nonzero(drawn)[0]
    keys = (np.float32(sign) * z[idx]).view(np.uint32)
    return idx[np.argsort(keys, kind="stable")].astype(np.int64)


def _bit_pairs(rng, bits: Sequence[int], span: int) -> List[int]:
    """three pairs {v, v | 1 << b}, each listed larger key first (array order against depth order: a sort that loses bit b leaves
    the pair in array order, which is the wrong one), later pairs drawn clear of the earlier ones' intervals where the span allows
    it, so that each pair stays adjacent in the stack's order."""
    out, taken = [], []
    for b in sorted(bits, reverse=True):
        for attempt in range(200):
            v = int(rng.integers(0, span + 1)) & ~(1 << b)
            lo, hi = v, v | (1 << b)
            if all((hi < a or lo > c) and not (lo < a < hi) and not (lo < c < hi) for a, c in taken):
                break
        taken.append((lo, hi))
        out += [hi, lo]
    return out


def _stack_offsets(rng, pops: Sequence[str], B: int, L: int) -> np.ndarray:
    """[len(pops), L] key offsets, every stack's listed in array-index order (module docstring)."""
    span = (1 << B) - 1
    shifts = [s for s in plan_shifts(B) if s > 0]
    carry_s = shifts + [s for s in range(1, B) if s not in shifts]
    n_bit = n_carry = 0
    offs = np.zeros((len(pops), L), np.int64)
    for s, p in enumerate(pops):
        if p == "ladder":
            o = int(rng.integers(0, span - 4)) + np.arange(6)[::-1]
        elif p == "bit":
            o = _bit_pairs(rng, [(3 * n_bit + i) % B for i in range(3)], span)
            n_bit += 1
        elif p == "carry":
            sh = carry_s[n_carry % len(carry_s)]
            n_carry += 1
            lo = 1 if sh > 1 else 2                                          # (d << s) - 2 >= 0
            hi = (span - 3) >> sh
            d = int(rng.integers(lo, hi + 1)) if hi >= lo else lo
            o = (d << sh) + np.array([-2, -1, 0, 1, 2, 3])
        elif p == "tie":
            o = _tie_offsets(int(rng.integers(1, span)))
        elif p == "random":
            o = rng.integers(0, span + 1, 6)
        else:
            o = np.arange(6)[::-1]
        offs[s] = np.clip(np.asarray(o, np.int64)[:L], 0, span)
    return offs


def _tie_offsets(v: int) -> np.ndarray:
    return np.array([v, v, v + 1, v + 1, v - 1, v])


REACH = 6   # px: no footprint of a small stack reaches further from its pixel (alpha > 1/255 out to 4.97 px; the preprocess's
            # conservative bound on it, 2 % and 0.05 px wider, is 5.05 px), so a stack in a 16-px block touches ONE tile row


def stack_tile_row(centres: np.ndarray) -> np.ndarray:
    """The one 16-px tile row every stack touches (asserted: the scene needs stacks_per = 16 or a multiple): which tile-row
    shards sort its members is then a matter of geometry, not of the kernel's margins."""
    cy = centres[:, 1]
    assert np.array_equal((cy - REACH) >> 4, (cy + REACH) >> 4), "a stack straddles two tile rows: use stacks_per=16"
    return cy >> 4


class OrderScene:
    """Packed arrays (utils.pack_gaussians layout) + per gaussian: stack (-1: decoy), rank in the stack's expected order, key offset.

    stacks_per   side in pixels of the block that holds one stack (8: one per quadrant, 16: one per tile; wide: 128)
    max_stacks   use only this many blocks (chosen by the seed)
    n_drawn      make the number of drawn gaussians exactly this (members are removed at the end: the last stack is partial)
    tie_at       sorted positions p: a `tie` stack is added whose equal keys hold positions p - 1, p, p + 1 of the expected order
    tie_rows     tile rows of a tile-row shard (renderer.shard_row_list): tie_at then counts positions in the order of THAT SHARD's
                 depth sort — the expected order restricted to the stacks in those rows (order_in_rows) — and the tie stacks lie
                 in those rows.  Needs stacks that touch one tile row each (stacks_per = 16)
    sign         -1: the scene at -z for the camera turned half round (Q_BACK)
    neg_decoys   decoy stacks at negative depth (off in the halves of a two-sided scene: the other camera would draw them)
    """

    def __init__(self, W: int, H: int, B: int, seed: int, stacks_per: Optional[int] = None, wide: bool = False, L: int = 6,
                 max_stacks: Optional[int] = None, n_drawn: Optional[int] = None, tie_at: Sequence[int] = (),
                 tie_rows: Optional[Sequence[int]] = None, sign: int = 1, neg_decoys: bool = True):
        assert 1 <= B <= 31 and 1 <= L <= 6 and sign in (1, -1) and (L == 6 or not tie_at)
        self.W, self.H, self.B, self.seed, self.L, self.wide, self.sign = W, H, B, seed, L, wide, sign
        block = stacks_per or (128 if wide else 8)
        self.block = block
        self.sigma_px = 20.0 if wide else 1.5
        args, f = camera_args(W, H, Q_FRONT if sign > 0 else Q_BACK)
        self.f = f
        rng = np.random.default_rng(seed)
        span = (1 << B) - 1
        self.span = span

        # blocks that hold a stack: whole blocks only, the stack's pixel clear of the last row and column (Q1); the tie stacks
        # take the last places (in the shard's rows, if one is named)
        off = block // 2 + (3 if wide else 0)
        bx, by = np.meshgrid(np.arange(W // block), np.arange(H // block), indexing="ij")
        bx, by = bx.ravel(), by.ravel()
        ok = (bx * block + off <= W - 3) & (by * block + off <= H - 3)
        bx, by = bx[ok], by[ok]
        pick = rng.permutation(len(bx))
        n_tie = len(tie_at)
        S = len(bx) - n_tie if max_stacks is None else min(max_stacks, len(bx) - n_tie)
        if n_drawn is not None:
            S = -(-(n_drawn - n_tie * L) // L)
            assert 0 < S <= len(bx) - n_tie, (n_drawn, len(bx))
        assert S >= 1
        for_ties = pick if tie_rows is None else pick[np.isin((by[pick] * block + off) >> 4, tie_rows)]
        for_ties = for_ties[:n_tie]
        assert len(for_ties) == n_tie
        pick = np.concatenate([pick[~np.isin(pick, for_ties)][:S], for_ties])
        bx, by = bx[pick], by[pick]
        self.centres = np.stack([bx * block + off, by * block + off], 1)      # [S + n_tie, 2] pixel of every stack
        counted = np.ones(S + n_tie, bool) if tie_rows is None else np.isin(stack_tile_row(self.centres), tie_rows)
        members = np.full(S, L)
        if n_drawn is not None:
            members[-1] = n_drawn - n_tie * L - L * (S - 1)
            assert 1 <= members[-1] <= L

        # populations: the ones that fit this B, in turn
        pops = [p for p in POPS if B >= FITS_FROM[p]]
        self.pop = [pops[s % len(pops)] for s in range(S)] + ["tie"] * n_tie
        offs = _stack_offsets(rng, self.pop[:S], B, L)

        # main part of the array: the members and the decoys in one random order; member m of a stack takes the stack's m-th slot
        # in ascending array order, so that the populations' "listed in array-index order" holds
        n_dec_stacks = max(3, S // 8)
        dec_kinds = [k for k in range(3) if k != 1 or neg_decoys]
        n_dec = n_dec_stacks * L
        n_main = int(members.sum()) + n_dec
        owner = np.concatenate([np.repeat(np.arange(S), members), np.repeat(-1 - np.arange(n_dec_stacks), L)])
        owner = owner[rng.permutation(n_main)]                                   # which stack (or decoy stack) owns each array slot
        # per gaussian: stack (-1: decoy), key offset (-1: decoy), depth, pixel, sideways shift in half-frames, kind of decoy (-1: none)
        g = dict(stack_of=np.where(owner >= 0, owner, -1), offset=np.full(n_main, -1, np.int64), z=np.zeros(n_main, np.float32),
                 cxy=np.zeros((n_main, 2)), far=np.zeros((n_main, 2)), decoy_kind=np.full(n_main, -1))
        slots = np.argsort(owner, kind="stable")[n_dec:]                         # (decoy slots first), then every stack's slots, ascending
        g["offset"][slots] = offs[np.arange(L)[None, :] < members[:, None]]
        # the frame's key range: one drawn gaussian at each end
        first = np.nonzero(owner >= 0)[0]
        g["offset"][first[0]] = span
        if len(first) > 1:
            g["offset"][first[-1]] = 0
        m = owner >= 0
        g["z"][m] = (BASE + g["offset"][m]).astype(np.uint32).view(np.float32)
        g["cxy"][m] = self.centres[owner[m]]
        for d in range(n_dec_stacks):
            sl = np.nonzero(owner == -1 - d)[0]
            kind = dec_kinds[d % len(dec_kinds)]
            g["cxy"][sl] = self.centres[int(rng.integers(0, S))]                  # on a real stack's pixel: a leak is loud
            g["decoy_kind"][sl] = kind
            some = (BASE + rng.integers(0, span + 1, L)).astype(np.uint32).view(np.float32)
            if kind == 0:
                g["z"][sl] = np.uint32(BASE - 1).view(np.float32)                  # 0.2f - 1 ulp
            elif kind == 1:
                g["z"][sl] = -some                                                  # behind the camera
            else:
                g["z"][sl] = some                                                   # a valid key, 3 .. 6 half-frames off to one side
                g["far"][sl, d % 2] = rng.uniform(3.0, 6.0, L) * rng.choice([-1.0, 1.0], L)
        for t, p in enumerate(sorted(tie_at)):
            g = self._insert_tie_stack(g, p, S + t, counted)
        stack_of, offset, z = g["stack_of"], g["offset"], g["z"]
        n = len(z)
        self.n, self.n_stacks = n, S + n_tie
        self.stack_of, self.offset, self.decoy_kind = stack_of, offset, g["decoy_kind"]
        drawn = stack_of >= 0

        # geometry: the mean on its pixel's centre at depth |z| (float64, rounded once), isotropic scale sigma_px pixels there
        zz = np.abs(z.astype(np.float64))
        x = (g["cxy"][:, 0] + 0.5 - 0.5 * W) * zz / f + g["far"][:, 0] * W * zz / f
        y = (g["cxy"][:, 1] + 0.5 - 0.5 * H) * zz / f + g["far"][:, 1] * W * zz / f
        zw = (np.float32(sign) * z).astype(np.float32)                               # world z; z_cam = sign * zw = z
        xw = (sign * x).astype(np.float32)                                           # the half turn about y mirrors x as well
        sc = np.log(self.sigma_px * zz / f).astype(np.float32)
        sh = np.zeros((n, 16, 3), np.float32)
        self.packed = dict(means=np.ascontiguousarray(np.stack([xw, y.astype(np.float32), zw], 1)),
                           log_scales=np.ascontiguousarray(np.stack([sc, sc, sc], 1)),
                           quats=np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1)),
                           opacity_logit=np.zeros(n, np.float32), sh=sh)
        self.z_cam = z                                                               # expected camera depth of every gaussian, bit for bit
        order = _expected(z, drawn, 1)
        self.rank = np.full(n, -1, np.int64)
        seen = np.zeros(self.n_stacks, np.int64)
        for i in order:
            self.rank[i] = seen[stack_of[i]]
            seen[stack_of[i]] += 1
        self.stack_size = seen
        col = np.ones((n, 3), np.float32)                                            # decoys: white
        col[drawn] = np.eye(3, dtype=np.float32)[self.rank[drawn] % 3]
        sh[:, 0, :] = (col - 0.5) / SH_C0
        self.views = [View(args, sign, B, order, drawn)]
        sub = order if tie_rows is None else order_in_rows(self, self.views[0], tie_rows)
        for p in tie_at:                                                             # the straddle really happened
            assert offset[sub[p - 1]] == offset[sub[p]] and stack_of[sub[p - 1]] == stack_of[sub[p]] >= S, p

    def _insert_tie_stack(self, g, p: int, stack: int, counted: np.ndarray):
        """A tie stack whose three equal keys v take positions p - 1, p, p + 1 among the gaussians of the `counted` stacks in draw
        order: v = the key that holds position p - 2 there now; the six members go into the array side by side in front of that
        gaussian (equal keys are drawn in array order), v - 1 among them."""
        live = np.nonzero((g["stack_of"] >= 0) & counted[np.maximum(g["stack_of"], 0)])[0]
        live = live[np.argsort(g["offset"][live], kind="stable")]
        assert 2 <= p < len(live), (p, len(live))
        at = int(live[p - 2])
        v = int(g["offset"][at])
        assert 1 <= v < self.span, f"position {p} lies in the run of key {v}: no room for v - 1 and v + 1"
        o = _tie_offsets(v)
        rows = dict(stack_of=np.full(6, stack), offset=o, z=(BASE + o).astype(np.uint32).view(np.float32),
                    cxy=np.tile(self.centres[stack], (6, 1)), far=np.zeros((6, 2)), decoy_kind=np.full(6, -1))
        return {k: np.insert(a, at, rows[k], axis=0) for k, a in g.items()}

    # -- a single scene is its own (only) view
    @property
    def cam_args(self):
        return self.views[0].cam_args

    @property
    def expected_order(self):
        return self.views[0].expected_order

    @property
    def n_drawn(self):
        return self.views[0].n_drawn

    @classmethod
    def two_sided(cls, W: int, H: int, B_front: int, B_back: int, seed: int, **kw) -> "OrderScene":
        """One order scene at +z and another at -z in one set of arrays, views[0] = the front camera, views[1] = the camera turned
        half round: each culls the other's half.  The halves are interleaved at random, each keeping its own array order (ranks
        and colours were fixed by it: exact ties are drawn in array order)."""
        a = cls(W, H, B_front, seed, sign=1, neg_decoys=False, **kw)
        b = cls(W, H, B_back, seed + 1, sign=-1, neg_decoys=False, **kw)
        na, n = a.n, a.n + b.n
        is_a = np.random.default_rng(seed + 2).permutation(n) < na
        perm = np.empty(n, np.int64)                                                 # new index i holds concatenated index perm[i]
        perm[is_a], perm[~is_a] = np.arange(na), na + np.arange(b.n)
        cat = lambda u, v: np.concatenate([u, v])[perm]
        both = cls.__new__(cls)
        both.W, both.H, both.L, both.wide, both.block, both.seed = W, H, a.L, a.wide, a.block, seed
        both.n, both.n_stacks = n, a.n_stacks + b.n_stacks
        both.packed = {k: np.ascontiguousarray(cat(a.packed[k], b.packed[k])) for k in a.packed}
        both.stack_of = cat(a.stack_of, np.where(b.stack_of >= 0, b.stack_of + a.n_stacks, -1))
        both.rank, both.offset, both.decoy_kind = cat(a.rank, b.rank), cat(a.offset, b.offset), cat(a.decoy_kind, b.decoy_kind)
        both.z_cam = cat(a.z_cam, b.z_cam)                                           # as the gaussian's OWN camera sees it
        both.centres = np.concatenate([a.centres, b.centres])
        both.stack_size = np.concatenate([a.stack_size, b.stack_size])
        both.pop = a.pop + b.pop
        da = cat(a.views[0].drawn, np.zeros(b.n, bool))
        db = cat(np.zeros(na, bool), b.views[0].drawn)
        both.views = [View(a.cam_args, 1, B_front, _expected(both.z_cam, da, 1), da),
                      View(b.cam_args, -1, B_back, _expected(both.z_cam, db, 1), db)]
        return both


def transposed(scene: OrderScene, view: View, j: int) -> np.ndarray:
    """view.expected_order with the members ranked j and j + 1 of EVERY stack the view draws (that has both) transposed."""
    order = view.expected_order
    pos = np.full(scene.n, -1, np.int64)
    pos[order] = np.arange(len(order))
    member = np.full((scene.n_stacks, scene.L + 1), -1, np.int64)
    g = order
    member[scene.stack_of[g], scene.rank[g]] = g
    a, b = member[:, j], member[:, j + 1]
    both = (a >= 0) & (b >= 0)
    out = order.copy()
    out[pos[a[both]]], out[pos[b[both]]] = b[both], a[both]
    return out


def stack_change(scene: OrderScene, view: View, screen_a: np.ndarray, screen_b: np.ndarray, j: int):
    """Largest |a - b| over the samples of every stack's own pixel block ([W,H,3] screens, orc.composite's layout), for the stacks the
    view draws that have members ranked j and j + 1: (stack ids, change per stack)."""
    d = np.abs(screen_a.astype(np.float64) - screen_b.astype(np.float64)).max(axis=2)
    stacks = np.unique(scene.stack_of[view.expected_order])
    stacks = stacks[scene.stack_size[stacks] > j + 1]
    blk = scene.block
    x0, y0 = scene.centres[stacks, 0] // blk * blk, scene.centres[stacks, 1] // blk * blk
    return stacks, np.array([d[x:x + blk, y:y + blk].max() for x, y in zip(x0, y0)])


def order_in_rows(scene: OrderScene, view: View, rows: Sequence[int]) -> np.ndarray:
    """view.expected_order restricted to the stacks that lie in the given tile rows: the order a tile-row shard with those rows
    (renderer.shard_row_list) sorts and draws — a shard's depth sort holds only the gaussians that touch its rows."""
    order = view.expected_order
    return order[np.isin(stack_tile_row(scene.centres)[scene.stack_of[order]], rows)]
