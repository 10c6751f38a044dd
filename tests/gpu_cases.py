"""What two or more test files (or a test file and a tool) share: the module namespace the `G` fixtures return, the scenes, the
cached cases and the references built on them.  A plain module next to the tests, like order_scenes.py and margin_scenes.py:
test modules and tools import it by name.

Rules (tests/test_support_layout.py holds the first two): it imports no test_* module; it does not touch sys.path (the one thing
it takes from tools/, the fuzz campaign's scene builder, is loaded by path); torch, gsr_amd and the oracle are imported inside
the functions that need them, so importing it and building a scene work without a GPU.

Every function that takes `G` takes what `namespace()` returns; the scene builders read only its modules, so a caller without a
GPU passes `modules()`.  Cases live in `G.cases`, one dict per test module: no module sees another's Rasterizer.
"""
import importlib.util
import os
import sys

import numpy as np

from conftest import REPO, golden_columns, load_golden, psnr
from order_scenes import OrderScene, camera_args

MIN_DB = 100.0        # the project's standing bar for fp32 compositing: per channel PSNR, peak = max |reference channel|
N_CH = 17             # channels of the gradient case: a full wide walk plus a narrow walk of one
N_SAMPLE = 96
MEDIANS = (0.5, 0.9, 1.0)
NEVER = 1 << 30


# ---- the namespace ----------------------------------------------------------------------------------------------------------------
def modules(orc=None):
    """The package's modules, the oracle (or the stand-in `orc`) and an empty case cache under the names the tests use."""
    import gsr_amd  # noqa: F401
    from gsr_amd import _lib, rasterize, renderer, synthetic, utils

    if orc is None:
        from oracle import cpu_oracle as orc

    class NS:
        pass

    ns = NS()
    ns.renderer, ns.rasterize, ns.synthetic, ns.utils, ns.orc, ns.lib = renderer, rasterize, synthetic, utils, orc, _lib
    ns._lib = ns.lib
    ns.cases = {}
    return ns


def namespace(orc=None):
    """What a GPU test module's fixture `G` returns: modules() on a machine with the GPU.  One per module (scope="module")."""
    import torch

    ns = modules(orc)
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return ns


# ---- scenes (CPU only) ------------------------------------------------------------------------------------------------------------
def golden_args(g, prefix=""):
    """The camera arguments of a golden file `g` (make_camera's, orc.camera's and _lib.camera_setup's parameter list)."""
    return (g[prefix + "qvec"], g[prefix + "tvec"], float(g["fx_full"]), float(g["fy_full"]), int(g["cam_width"]),
            int(g["cam_height"]), int(g["width"]), int(g["height"]))


def golden_cameras(G, g, prefix=""):
    args = golden_args(g, prefix)
    return G.renderer.make_camera(*args), G.orc.camera(*args)


def golden(G, name, prefix=""):
    g = load_golden(name)
    return G.utils.pack_gaussians(golden_columns(g)), golden_args(g, prefix)


def medium_columns(G, n=200_000, seed=5, shift=1.2, W=640, H=360, pose=2):
    cols = G.synthetic.mip360_like(n, seed)
    for i in range(3):
        cols[f"scale_{i}"] = (cols[f"scale_{i}"] + np.float32(shift)).astype(np.float32)
    p = G.synthetic.ring_cameras(25)[pose]
    fx = G.synthetic.pinhole_focal(W)
    return cols, (p.qvec, p.tvec, 2 * fx, 2 * fx, 2 * W, 2 * H, W, H)


def medium(G, *a, **kw):
    """medium_columns as (packed arrays, camera arguments)."""
    cols, args = medium_columns(G, *a, **kw)
    return G.utils.pack_gaussians(cols), args


def medium_cameras(G, *a, **kw):
    """medium_columns as (columns, the library's camera, the oracle's camera)."""
    cols, args = medium_columns(G, *a, **kw)
    return cols, G.renderer.make_camera(*args), G.orc.camera(*args)


def _tool(name):
    """tools/<name>.py as the module `name`: the one a tool has imported under that name, else loaded by its path and
    entered under it (this module does not touch sys.path), so that a tool and the tests hold the same objects."""
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "tools", name + ".py"))
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
        sys.modules[name] = module
    return sys.modules[name]


# fuzz_case(case_seed, max_n=60000): the deterministic scene / frame / camera of one campaign case of tools/fuzz_parity.py.  The
# function is tools/fuzz_scene.build_case (fuzz_parity.build_case is the same object): the tools must work without this file.
fuzz_case = _tool("fuzz_scene").build_case


def f5_case():
    """(g, c): the golden file of fixture f5 — the reference's own frame of the deep-stack fuzz case — and the case rebuilt from
    the seed it records."""
    g = load_golden("f5_deep_stack.npz")
    return g, fuzz_case(int(g["case_seed"]), int(g["max_n"]))


def build(G, name):
    """(packed arrays, camera arguments) of the scene `name`: f1 f2 f3a f3b f5 medium 1080p wall."""
    if name == "f1":
        return golden(G, "f1_unit.npz")
    if name == "f2":
        return golden(G, "f2_small.npz")
    if name in ("f3a", "f3b"):
        return golden(G, "f3_edge.npz", name[2] + "_")
    if name == "f5":
        _, c = f5_case()
        return c["packed"], c["args"]
    if name == "medium":
        return medium(G)
    if name == "1080p":
        return medium(G, n=600_000, seed=360, shift=0.8, W=1920, H=1080, pose=0)
    if name == "wall":  # the "opaque wall" of test_gpu_parity._rule_cases: every opacity logit 6 (alpha capped at 0.99)
        packed, args = medium(G, n=300_000, shift=1.6)
        packed["opacity_logit"] = np.full_like(packed["opacity_logit"], 6.0)
        return packed, args
    raise KeyError(name)


def deep_tile_scene():
    """40x24 (3x2 tiles), 1000 gaussians at 1000 distinct depths, array order shuffled against depth order.  Nine in ten lie in the
    first quadrant of tile (0, 0): small (sigma 0.5 - 0.9 px before the low-pass) and faint (opacity 0.0042 - 0.0065: alpha just above
    1/255, on the few pixels next to the centre only), so a pixel keeps most of its transmittance through hundreds of list entries; five strong, wider ones lie late in depth
    (ranks 560, 700, 850, 990, 995) over the same quadrant; the rest are scattered over the frame."""
    W, H, n = 40, 24, 1000
    args, f = camera_args(W, H)
    rng = np.random.default_rng(17)
    rank = rng.permutation(n)
    z = 1.0 + 0.002 * rank
    strong = np.isin(rank, (560, 700, 850, 990, 995))
    away = (rank % 10 == 3) & ~strong
    cx, cy = rng.uniform(1.5, 6.5, n), rng.uniform(1.5, 6.5, n)
    sigma, opacity = rng.uniform(0.5, 0.9, n), rng.uniform(0.0042, 0.0065, n)
    cx[away], cy[away] = rng.uniform(0, W, away.sum()), rng.uniform(0, H, away.sum())
    sigma[away], opacity[away] = rng.uniform(1.5, 4.0, away.sum()), rng.uniform(0.05, 0.6, away.sum())
    cx[strong], cy[strong] = rng.uniform(2.0, 6.0, strong.sum()), rng.uniform(2.0, 6.0, strong.sum())
    sigma[strong], opacity[strong] = rng.uniform(3.0, 5.0, strong.sum()), rng.uniform(0.7, 0.95, strong.sum())
    x, y = (cx + 0.5 - 0.5 * W) * z / f, (cy + 0.5 - 0.5 * H) * z / f
    s = np.log(sigma * z / f)
    q = rng.normal(size=(n, 4))
    packed = dict(means=np.stack([x, y, z], 1).astype(np.float32),
                  log_scales=np.stack([s + rng.uniform(-0.2, 0.2, n), s, s + rng.uniform(-0.2, 0.2, n)], 1).astype(np.float32),
                  quats=(q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32),
                  opacity_logit=np.log(opacity / (1.0 - opacity)).astype(np.float32), sh=np.zeros((n, 16, 3), np.float32))
    return {k: np.ascontiguousarray(v) for k, v in packed.items()}, args


def wall_scene():
    """32x16 (two tiles), 300 gaussians at 300 distinct depths, array order shuffled against depth order.  The six nearest are wide
    (sigma 40 px, centred on the frame) and nearly opaque: behind them T is below every pixel's fourth weight.  The other 294 are small
    and faint and lie behind: they keep T above zero, so the feature blend walks every one of them."""
    W, H, n = 32, 16, 300
    args, f = camera_args(W, H)
    rng = np.random.default_rng(23)
    rank = rng.permutation(n)
    z = 1.0 + 0.002 * rank
    front = rank < 6
    cx, cy = rng.uniform(0, W, n), rng.uniform(0, H, n)
    sigma, opacity = rng.uniform(3.0, 6.0, n), rng.uniform(0.05, 0.3, n)
    cx[front], cy[front] = rng.uniform(14.0, 18.0, 6), rng.uniform(6.0, 10.0, 6)
    sigma[front], opacity[front] = 40.0, rng.uniform(0.90, 0.97, 6)
    x, y = (cx + 0.5 - 0.5 * W) * z / f, (cy + 0.5 - 0.5 * H) * z / f
    s = np.log(sigma * z / f)
    q = rng.normal(size=(n, 4))
    packed = dict(means=np.stack([x, y, z], 1).astype(np.float32), log_scales=np.stack([s, s, s], 1).astype(np.float32),
                  quats=(q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32),
                  opacity_logit=np.log(opacity / (1.0 - opacity)).astype(np.float32), sh=np.zeros((n, 16, 3), np.float32))
    return {k: np.ascontiguousarray(v) for k, v in packed.items()}, args, rank


# ---- cases: a scene with its cameras and its Rasterizer, cached in G.cases ----------------------------------------------------------
def z_cam(G, cam, means):
    """fp32 camera-space depth of every gaussian: column 2 of gsr_project_to_camera_space for the camera's w2c."""
    import torch

    w2c = torch.tensor(list(cam.w2c), dtype=torch.float32).view(4, 4)
    return G.rasterize.project_to_camera_space(torch.from_numpy(np.ascontiguousarray(means)).cuda(), w2c)[:, 2].cpu().numpy()


def custom_case(G, name, packed, args):
    if name not in G.cases:
        cam, ocam = G.renderer.make_camera(*args), G.orc.camera(*args)
        R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(packed))
        G.cases[name] = dict(packed=packed, cam=cam, ocam=ocam, R=R)
    return G.cases[name]


def feature_case(G, name):
    """packed scene (file order), cameras, a Rasterizer on the Morton-ordered scene and the test features
    (z_cam, 1, 1000 - 3.5 z_cam) in file order."""
    import torch

    if name not in G.cases:
        packed, args = build(G, name)
        cam, ocam = G.renderer.make_camera(*args), G.orc.camera(*args)
        R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(packed))
        z = z_cam(G, cam, packed["means"])
        F = np.stack([z, np.ones_like(z), np.float32(1000.0) - np.float32(3.5) * z], 1).astype(np.float32)
        F[~np.isfinite(F)] = 0.0  # (gaussians with such values are culled; the array must still be finite)
        G.cases[name] = dict(packed=packed, cam=cam, ocam=ocam, R=R, F=F, Ft=torch.from_numpy(F).cuda())
    return G.cases[name]


def gradient_case(G, name):
    """The scene, its Rasterizer, the oracle's preprocess and depth order, N_CH feature columns in file order and the upstream
    gradient Gm [H, W, N_CH]; computed once and only read."""
    import torch

    if name not in G.cases:
        packed, args = build(G, name)
        cam, ocam = G.renderer.make_camera(*args), G.orc.camera(*args)
        R = G.renderer.Rasterizer(G.renderer.GaussianScene.from_packed(packed))
        pre = G.orc.preprocess(packed, ocam)
        order = G.orc.depth_order(pre["cam_means"])
        gen = torch.Generator().manual_seed(23)
        Gm = torch.randn((cam.height, cam.width, N_CH), generator=gen)
        F = torch.randn((R.scene.n, 2 * N_CH - 1), generator=gen) * 50.0
        bb, sg = pre["pixel_bboxes"], pre["sigmas"]
        drawable = ((bb[:, 2] - bb[:, 0]) * (bb[:, 3] - bb[:, 1]) != 0) & (sg != 0).all(1)  # what the oracle's loop does not skip
        G.cases[name] = dict(packed=packed, cam=cam, ocam=ocam, R=R, pre=pre, order=order, Gm=Gm, Gt=Gm.cuda(), Ft=F.cuda(),
                             drawable=drawable, refs={})
    return G.cases[name]


def pick_case(G, name):
    if name == "deep":
        return custom_case(G, "pick_deep", *deep_tile_scene())
    if name == "stacks":
        s = OrderScene(64, 48, 12, seed=5)
        return custom_case(G, "pick_stacks", s.packed, s.cam_args)
    return feature_case(G, name)


# ---- comparisons against the oracle's camera and preprocess -------------------------------------------------------------------------
def assert_same_camera(cam, ocam):
    """gsr_camera_setup's struct against gsr_oracle_camera's, field for field and bit for bit (both run on the host)."""
    for f in ("w2c", "full_proj", "cam_center"):
        assert list(getattr(cam, f)) == list(getattr(ocam, f)), f
    for f in ("focal_x", "focal_y", "lim_x", "lim_y", "tan_fov_x", "tan_fov_y", "width", "height"):
        assert getattr(cam, f) == getattr(ocam, f), f


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max(initial=0.0) / max(np.abs(b).max(initial=0.0), 1e-30)


def assert_preprocess_matches(dbg, pre, rects_on=None):
    """Rasterizer.preprocess_debug (as numpy arrays) against orc.preprocess: the integer rects bit for bit — on every gaussian, or on
    those of the mask `rects_on` — the zero pattern of the conics, and each float array within its tolerance of the array's largest
    |value|; cov2d on the gaussians in front of the cull plane.  -> the worst share of a tolerance used."""
    on = slice(None) if rects_on is None else rects_on
    assert np.array_equal(dbg["tile_bboxes"][on], pre["tile_bboxes"][on])
    assert np.array_equal(dbg["pixel_bboxes"][on], pre["pixel_bboxes"][on])
    assert np.array_equal(dbg["sigmas"] == 0, pre["sigmas"] == 0)
    worst = 0.0
    for k, tol in (("cov3d", 1e-6), ("cam_means", 1e-6), ("rgb", 1e-6), ("opacity", 1e-6), ("screen_means", 1e-6),
                   ("sigmas", 1e-5)):
        assert _rel(dbg[k], pre[k]) < tol, k
        worst = max(worst, _rel(dbg[k], pre[k]) / tol)
    vis = pre["cam_means"][:, 2] >= 0.2
    assert _rel(dbg["cov2d"][vis], pre["cov2d"][vis]) < 1e-5
    return max(worst, _rel(dbg["cov2d"][vis], pre["cov2d"][vis]) / 1e-5)


# ---- references -------------------------------------------------------------------------------------------------------------------
def oracle_maps(G, c, feats, limit=-1):
    """The oracle's compositing loop over `feats` [n,3] in the place of the colours -> (map [H,W,3], T [H,W], drawn)."""
    if "pre" not in c:
        c["pre"] = G.orc.preprocess(c["packed"], c["ocam"])
        c["order"] = G.orc.depth_order(c["pre"]["cam_means"])
    pre = dict(c["pre"], rgb=np.ascontiguousarray(feats, np.float32))
    screen, trans, drawn = G.orc.composite(c["order"], pre, c["cam"].width, c["cam"].height, limit=limit, threads=G.orc.max_threads())
    return screen.transpose(1, 0, 2), trans.transpose(1, 0), drawn


def weight_maps(G, c, ids, restrict):
    """The oracle's weight maps [len(ids), H, W] of the gaussians `ids`, three per orc.composite.  restrict: over the depth order
    up to the last of the three, and of those gaussians only whose pixel bbox meets one of the three's — nobody else changes the
    transmittance the three are drawn with, and the one-hot columns give everybody else the colour 0."""
    cam, n, bb, order = c["cam"], len(c["drawable"]), c["pre"]["pixel_bboxes"], c["order"]
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    maps = np.zeros((len(ids), cam.height, cam.width), np.float32)
    by_depth = np.argsort(rank[ids])  # neighbours in depth share a composite: short restricted orders
    for k0 in range(0, len(ids), 3):
        at = by_depth[k0:k0 + 3]
        trio, sub = ids[at], order
        if restrict:
            sub = order[:rank[trio].max() + 1]
            near = np.zeros(n, bool)
            for i in trio:
                near |= (bb[:, 0] < bb[i, 2]) & (bb[:, 2] > bb[i, 0]) & (bb[:, 1] < bb[i, 3]) & (bb[:, 3] > bb[i, 1])
            sub = np.ascontiguousarray(sub[near[sub]])
        onehot = np.zeros((n, 3), np.float32)
        onehot[trio, np.arange(len(trio))] = 1.0
        screen, _, _ = G.orc.composite(sub, dict(c["pre"], rgb=onehot), cam.width, cam.height, limit=-1, threads=G.orc.max_threads())
        maps[at] = screen.transpose(2, 1, 0)[:len(trio)]
    return maps


def bar(tag, got, ref):
    """Per channel PSNR of the block `got` against the oracle block `ref`, peak = max |ref channel|; prints, then asserts."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    got, ref = got.reshape(len(ref), -1), ref.reshape(len(ref), -1)
    dbs = []
    for ch in range(ref.shape[1]):
        peak = float(np.abs(ref[:, ch]).max())
        dbs.append(psnr(got[:, ch], ref[:, ch], peak=peak) if peak > 0 else (float("inf") if not got[:, ch].any() else 0.0))
    print(f"\n{tag}: {min(dbs):.1f} .. {max(dbs):.1f} dB over {len(dbs)} channels", end="")
    assert min(dbs) >= MIN_DB, (tag, dbs)
    return dbs


def sample(c, name):
    """N_SAMPLE seeded gaussians among those the oracle's loop does not skip; "wall": among the first 5 % of their depth order, where
    the transmittance has not yet reached zero."""
    pool = c["order"][c["drawable"][c["order"]]]
    if name == "wall":
        pool = pool[:len(pool) // 20]
    rng = np.random.default_rng(7)
    return np.sort(rng.choice(pool, size=min(N_SAMPLE, len(pool)), replace=False))


def expected_of(Wk, appear, med, med_rank):
    """The expected maps after some prefix: Wk [H,W,n] its weights, appear [H,W,n] the prefix each gaussian first had w > 0 in."""
    import torch

    bw = Wk.max(-1).values
    is_max = (Wk == bw[..., None]) & (bw[..., None] > 0)
    first = torch.where(is_max, appear, torch.full_like(appear, NEVER))  # of several maximisers: the first in the prefix sweep
    bid = first.argmin(-1).to(torch.int32)
    bid = torch.where(bw > 0, bid, torch.full_like(bid, -1))
    brank = torch.where(bw > 0, first.min(-1).values, torch.zeros_like(bid))
    return dict(best_id=bid, best_w=bw.clone(), best_rank=brank, count=(Wk > 0).sum(-1).to(torch.int32),
                median_id={m: v.clone() for m, v in med.items()}, median_rank={m: v.clone() for m, v in med_rank.items()})


def exact(G, c, snapshots=()):
    """One sweep of the prefixes per scene, shared by the tests that need it: c["exact"] = the expected maps of the whole draw,
    c["exact_at"][k] those of draw_limit = k, c["W"] the full weight maps (file order, like the ids render_pick returns)."""
    import torch

    if "exact" in c:
        assert all(k in c["exact_at"] for k in snapshots)
        return c["exact"]
    R, cam, mk = c["R"], c["cam"], G.renderer.make_options
    n, dev = R.scene.n, R.scene.device
    eye = torch.eye(n, dtype=torch.float32, device=dev)
    W_full, T_full = R.render_features(cam, eye, return_T=True)
    shape = (cam.height, cam.width)
    appear = torch.zeros(shape + (n,), dtype=torch.int32, device=dev)
    med = {m: torch.full(shape, -1, dtype=torch.int32, device=dev) for m in MEDIANS}
    med_rank = {m: torch.zeros(shape, dtype=torch.int32, device=dev) for m in MEDIANS}
    prev, at = torch.zeros_like(W_full), {}
    for k in range(1, n + 1):  # (prefixes past the last drawn gaussian are the whole draw again)
        Wk, Tk = R.render_features(cam, eye, mk(draw_limit=k), return_T=True)
        new = (Wk > 0) & (prev == 0)
        appear = torch.where(new, torch.full_like(appear, k), appear)
        for m in MEDIANS:
            cross = (Tk < m) & (med_rank[m] == 0)  # r = min{k : T^(k) < median_T}
            if bool(cross.any()):
                rows = new[cross]
                assert bool((rows.sum(-1) == 1).all()), (k, m)  # the unique gaussian the prefix gained at these pixels
                med[m][cross] = rows.to(torch.int32).argmax(-1).to(torch.int32)
                med_rank[m][cross] = k
        if k in snapshots:
            at[k] = expected_of(Wk, appear, med, med_rank)
        prev = Wk
    assert torch.equal(prev, W_full) and torch.equal(Tk, T_full)  # the sweep ended on the frame's own weights
    c["W"], c["T"], c["appear"], c["exact_at"] = W_full, T_full, appear, at
    c["exact"] = expected_of(W_full, appear, med, med_rank)
    return c["exact"]
