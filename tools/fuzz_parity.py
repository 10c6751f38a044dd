#!/usr/bin/env python3
"""Randomised parity campaign on the GPU: random scenes / frame sizes / cameras / options, HIP path (through the C ABI)
against the C oracle, plus the bit-identity properties (sharding, culling off, bf16 store, repeat).  Not part of the test
suite (open-ended run time); run it on the GPU box after touching a kernel:  python tools/fuzz_parity.py --seconds 120
Checker only: imports oracle/.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


from fuzz_scene import build_case  # noqa: E402  (tools/fuzz_scene.py, next to this file; tests/gpu_cases.fuzz_case is the same function)


def maps_campaign(a):
    """--maps: the map kernels (feature / channel blend, its backward, pick, top-k, slab, view statistics, K views per launch)
    against the float64 reference of tools/fuzz_maps.py on fresh campaign cases small enough for it (H * W * drawn <= 2e7), in
    file and in Morton order, with the check functions the suite runs on its pinned seeds.  A case whose drawn neighbours lie
    closer than 16 ulps in depth gets the identities between the kernels only; one over an exclusion cap is counted and skipped.
    A gradient whose bar fails on a cancelling sum of one or two rows (fuzz_maps._gradient_bar) is tallied as ill-conditioned, not as
    a failure, while its error stays under 1e-5 of the terms' own magnitude.  Tallies go to --maps-out."""
    import fuzz_maps as fm
    import gsr_amd  # noqa: F401
    from gsr_amd import renderer
    from oracle import cpu_oracle as orc

    master = np.random.default_rng(a.seed)
    t_end = time.time() + a.seconds
    tally = dict(cases=0, checked=0, identities_only=0, too_large=0, over_a_cap=0, ill_conditioned_gradient=0, failures=0)
    worst, shares, failed = {}, {}, []
    while time.time() < t_end and not (a.case_seed is not None and tally["cases"]):
        case_seed = int(master.integers(0, 1 << 62)) if a.case_seed is None else a.case_seed
        c = build_case(case_seed, a.max_n)
        tally["cases"] += 1
        pre = orc.preprocess(c["packed"], orc.camera(*c["args"]))
        bb = pre["pixel_bboxes"]
        drawn = int((((bb[:, 2] - bb[:, 0]) * (bb[:, 3] - bb[:, 1]) != 0) & (pre["sigmas"] != 0).all(1)).sum())
        desc = f"case-seed={case_seed} n={c['n']} {c['W']}x{c['H']} gen={c['gen'].__name__} drawn={drawn}"
        if c["H"] * c["W"] * drawn > 2e7:
            tally["too_large"] += 1
            continue
        print(f"case {tally['cases']}: {desc}", flush=True)  # before it runs: a stall then points at its case
        for order in ("file", "morton"):
            try:
                scene = renderer.GaussianScene.from_packed(c["packed"], spatial_order=order == "morton")
                R = renderer.Rasterizer(scene)
                views = [(renderer.make_camera(*args), ref) for args, ref in fm.case_views(orc, c, scene.order)]
                cam, ref = views[0]
                F, Gm = fm.features_of(case_seed % 1000, c["n"]), fm.upstream_of(case_seed % 1000, c["H"], c["W"], 3)
                if any(fm.facts(r)["min_gap_ulps"] < 16 for _, r in views):
                    tally["identities_only"] += 1
                    figs = dict(identities=fm.run_identities(renderer, R, [v for v, _ in views], F, Gm[0]))
                else:
                    sh = fm.shares(ref)
                    for k, v in sh.items():
                        shares[k] = max(shares.get(k, 0.0), v)
                    if any(fm.shares(r)[k] > cap for _, r in views for k, cap in fm.CAPS.items()):
                        tally["over_a_cap"] += 1
                        continue
                    from gsr_amd import rasterize
                    w2c = torch.tensor(list(cam.w2c), dtype=torch.float32).view(4, 4)
                    z = rasterize.project_to_camera_space(torch.from_numpy(c["packed"]["means"]).cuda(), w2c)[:, 2].cpu().numpy()
                    figs = dict(forward=fm.run_forward(R, cam, ref, F), slab=fm.run_slab(R, cam, ref, F, z),
                                backward=fm.run_backward(R, cam, ref, Gm[0], lenient=True), stats=fm.run_stats(R, cam, ref),
                                pick=fm.run_pick(R, cam, ref), topk=fm.run_topk(R, cam, ref),
                                views=fm.run_views(renderer, R, views, F, Gm, lenient=True))
                    tally["checked"] += 1
                    tally["ill_conditioned_gradient"] += any("ill_conditioned_rel" in f for f in figs.values())
                for kind, fig in figs.items():
                    for k, v in fig.items():
                        key = f"{kind}.{k}"
                        worst[key] = (min if k.startswith("dB") else max)(worst.get(key, v), v)
            except Exception as e:  # noqa: BLE001
                tally["failures"] += 1
                failed.append(f"{desc} order={order}: {type(e).__name__}: {str(e)[:300]}")
                print("FAIL " + failed[-1], flush=True)
    lines = ["fuzz_parity.py --maps: " + ", ".join(f"{k} {v}" for k, v in tally.items()) + f" (seed {a.seed}, max_n {a.max_n})",
             "largest share left out, reference alone: " + ", ".join(f"{k} {100 * v:.2f} %" for k, v in sorted(shares.items())),
             "worst figure per kind (dB: the lowest; errors and shares: the largest):"]
    lines += [f"  {k} = {v:.3g}" for k, v in sorted(worst.items())] + ["FAIL " + f for f in failed]
    os.makedirs(os.path.dirname(os.path.abspath(a.maps_out)), exist_ok=True)
    with open(a.maps_out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    sys.exit(1 if tally["failures"] else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", action="store_true", help="check the map kernels against the float64 reference of tools/fuzz_maps.py "
                    "instead of the colour frame (cases with H * W * drawn <= 2e7); tallies go to --maps-out")
    ap.add_argument("--maps-out", default=os.path.join(REPO, "profiles", "fuzz_maps_summary.txt"))
    ap.add_argument("--seconds", type=float, default=120.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-n", type=int, default=60000)
    ap.add_argument("--case-seed", type=int, default=None, help="replay one case (printed by a failure) with diagnostics")
    ap.add_argument("--report-flips", action="store_true", help="print every case in which a pixel sits on the alpha > 1/255 step "
                    "(differs from the oracle by more than 1e-5): how often, and by how much, the tolerance is actually used")
    a = ap.parse_args()
    if a.maps:
        return maps_campaign(a)

    import gsr_amd  # noqa: F401
    from conftest import psnr
    from gsr_amd import renderer
    from oracle import cpu_oracle as orc

    def close(x, ref):
        """conftest.assert_frames_close for frames of any size: `alpha > 1/255` is a step function, so a pixel sitting on the
        threshold may flip (by at most MIN_ALPHA * T * c < 4.5e-3, in colour and in T); on a tiny frame one flip already
        exceeds a relative budget, so at least 3 flipped pixels are always allowed.  A pixel counts as flipped from 5e-5 on:
        below that sits the accumulated fp32 rounding of deep stacks (hundreds of semi-transparent layers: every alpha carries
        ~1e-6 relative from the log2-domain exponent, and T carries the product) — case-seed 2519059510838425248 (scales
        blown up e-fold on a 15-px-wide frame) has 37 pixels between 1e-5 and 2e-5 and none above."""
        d = np.abs(np.asarray(x, np.float64) - np.asarray(ref, np.float64))
        assert d.max() <= 4.5e-3, f"max {d.max()}"
        px = d.reshape(d.shape[0] * d.shape[1], -1).max(1)
        assert (px > 5e-5).sum() <= max(3, 1e-4 * px.size), f"{(px > 5e-5).sum()} of {px.size} pixels off"
        if d.size >= 300_000:
            assert psnr(x, ref) >= 100.0, f"psnr {psnr(x, ref)}"

    master = np.random.default_rng(a.seed)
    t_end = time.time() + a.seconds
    cases = fails = 0
    mk = renderer.make_options
    while time.time() < t_end and not (a.case_seed is not None and cases):
        case_seed = int(master.integers(0, 1 << 62)) if a.case_seed is None else a.case_seed
        c = build_case(case_seed, a.max_n)
        rng, n, W, H, gen, shift, degree, pose, args, packed = (c[k] for k in ("rng", "n", "W", "H", "gen", "shift", "degree", "pose", "args", "packed"))
        cam, ocam = renderer.make_camera(*args), orc.camera(*args)
        desc = f"case-seed={case_seed} n={n} {W}x{H} gen={gen.__name__} shift={shift} deg={degree} sf={c['sf']}"
        # the case names itself BEFORE it runs: a stall (the harness kills a silent run) then points at its case
        print(f"case {cases}: {desc}", flush=True)
        try:
            # file order: deliberate depth ties resolve by scene index, and the oracle's scene is the file
            scene = renderer.GaussianScene.from_packed(packed, sh_degree=degree, spatial_order=False)
            R = renderer.Rasterizer(scene, max_pairs=int(rng.choice([0, 1000])) or None)
            img, T = R.render(cam, return_T=True)
            oimg, oT, _ = orc.render(packed, ocam, sh_degree=degree, want_T=True)
            if a.case_seed is not None:
                d = np.abs(img.cpu().numpy().astype(np.float64) - oimg).max(2)
                dT = np.abs(T.cpu().numpy().astype(np.float64) - oT)
                print(desc)
                print(f"pixels off by > 1e-5: {(d > 1e-5).sum()} of {d.size}; > 4.5e-3: {(d > 4.5e-3).sum()}; worst colour {d.max():.6f}, worst T {dT.max():.6f}")
                for y, x in zip(*np.unravel_index(np.argsort(-d, axis=None)[:6], d.shape)):
                    print(f"   pixel ({x},{y}) colour diff {d[y, x]:.6f}  T diff {dT[y, x]:.6f}  T oracle {oT[y, x]:.6f}")
            if a.report_flips:
                dpx = np.abs(img.cpu().numpy().astype(np.float64) - oimg).max(2)
                if (dpx > 1e-5).any():
                    print(f"flip: {desc}: {(dpx > 1e-5).sum()} of {dpx.size} pixels off by > 1e-5, worst {dpx.max():.2e} "
                          f"(one step = MIN_ALPHA * T * c <= 3.9e-3); share of samples {(np.abs(img.cpu().numpy() - oimg) > 1e-5).mean():.2e}", flush=True)
            close(img.cpu().numpy(), oimg)
            close(T.cpu().numpy()[..., None], oT[..., None])
            assert torch.equal(R.render(cam), img), "not reproducible"
            assert torch.equal(R.render(cam, mk(no_footprint_cull=True)), img), "culling changes bits"
            assert torch.equal(R.render(cam, mk(blend_impl=1)), img), "asm walk differs from the plain blend kernel"
            assert torch.equal(R.render(cam, mk(fine_binning=True)), img), "coarse and fine binning differ"
            assert torch.equal(R.render(cam, mk(saturation_rule=1)), img), "colour-saturation rule differs from the T == 0 rule"
            assert torch.equal(R.render(cam, mk(saturation_rule=1, early_out_T=-1.0)), img), "early-out differs from blending everything"
            assert torch.equal(R.render(cam, mk(output_bf16=True)), img.to(torch.bfloat16)), "bf16 store"
            step = int(rng.choice([2, 3, 5, 8]))
            block = int(rng.choice([1, 2]))  # single tile rows, or pairs of rows = whole 32x32 cell rows (GsrOptions.tile_row_block)
            tiles_y = (H + 15) // 16
            full = torch.zeros((tiles_y * 16, W, 3), device=img.device)
            for r in range(step):
                strip = R.render(cam, mk(tile_row_begin=r, tile_row_step=step, output_layout=2, tile_row_block=block))
                rows = renderer.shard_row_list(H, r, step, block)
                if rows:
                    full.view(tiles_y, 16, W, 3)[torch.as_tensor(rows, device=img.device)] = strip.view(len(rows), 16, W, 3)
            assert torch.equal(full[:H], img), f"shards (step {step}, rows in blocks of {block}) differ"
            # -- the other modes, each against an exact property or the oracle ----------------------------------
            assert torch.equal(R.render(cam, mk(output_layout=1)), img.transpose(0, 1)), "layout 1 is not the transpose"
            nc = R.render(cam, mk(reference_compat=False))
            assert torch.equal(nc[: H - 1, : W - 1], img[: H - 1, : W - 1]), "non-compat differs inside the frame"
            eo = float(rng.choice([1e-4, 1e-2]))
            assert float((R.render(cam, mk(early_out_T=eo)) - img).abs().max()) <= eo * 1.01 + 1e-6, "early-out bound"
            cam2 = renderer.make_camera(pose.qvec, np.asarray(pose.tvec) + np.array([0.05, -0.02, 0.1]), *args[2:])
            b = R.render_batch([cam, cam2, cam])
            assert torch.equal(b[0], img) and torch.equal(b[2], img) and torch.equal(b[1], R.render(cam2)), "batch"
            # several views through ONE launch sequence (gsr_render_batch with K workspace slices): the same frames, also for a
            # tile-row shard, also with a pair buffer that is too small on entry
            K = int(rng.choice([2, 3, 4, 8]))
            img2 = R.render(cam2)
            views = [cam, cam2, cam, cam2, cam][: int(rng.integers(2, 6))]
            want = torch.stack([img if v is cam else img2 for v in views])
            RK = renderer.Rasterizer(scene, max_pairs=int(rng.choice([0, 1000])) or None, views=K)
            assert torch.equal(RK.render_batch(views), want), f"{K} views per launch sequence differ from single views"
            so = mk(tile_row_begin=int(rng.integers(0, step)), tile_row_step=step, output_layout=2, tile_row_block=block)
            assert torch.equal(RK.render_batch(views, so), torch.stack([R.render(v, so) for v in views])), f"{K} views per launch sequence, shard"
            # block-level culling (GsrScene.block_bounds): the same bits with the bounds, and no skipped block holds a gaussian the
            # reference would draw (its skip guard, rasterize.py:441, on the reference-parity intermediates)
            bounded = renderer.GaussianScene.from_packed(packed, sh_degree=degree, spatial_order=False).build_bounds()
            RB = renderer.Rasterizer(bounded, views=K)
            assert torch.equal(RB.render(cam), img), "block-level culling changes bits"
            assert torch.equal(RB.render(cam, so), R.render(cam, so)), "block-level culling changes a shard's bits"
            assert torch.equal(RB.render_batch(views), want), "block-level culling changes a batch's bits"
            if n <= 200_000:
                dbg = R.preprocess_debug(cam)
                pb, sg = dbg["pixel_bboxes"], dbg["sigmas"]
                drawn = (dbg["cam_means"][:, 2] >= 0.2) & ((pb[:, 2] - pb[:, 0]) > 0) & ((pb[:, 3] - pb[:, 1]) > 0) & (sg != 0).all(dim=1)
                dead = bounded.blocks_skipped(cam).bool()
                per_block = torch.nn.functional.pad(drawn, (0, (-n) % 64)).view(-1, 64)
                assert not (per_block & dead[:, None]).any(), "a skipped block holds a gaussian the reference draws"
            if degree == 3 and n <= 200_000:
                pre = orc.preprocess(packed, ocam)
                dbg = R.preprocess_debug(cam)
                for k in ("tile_bboxes", "pixel_bboxes"):
                    got = dbg[k].cpu().numpy()
                    bad = np.flatnonzero((got != pre[k]).any(1))
                    if a.case_seed is not None and len(bad):
                        for i in bad[:5]:
                            print(f"   {k}[{i}]: hip {got[i]} oracle {pre[k][i]}  cov2d hip {dbg['cov2d'][i].cpu().numpy().ravel()} oracle {pre['cov2d'][i].ravel()}"
                                  f"  mean hip {dbg['screen_means'][i].cpu().numpy()} oracle {pre['screen_means'][i]}  z {pre['cam_means'][i][2]}")
                    # the rects are floor/ceil of fp32 expressions: exp/sqrt may differ by an ulp between ocml and libm, which
                    # moves a rect edge by one tile for the rare gaussian sitting on the step
                    assert len(bad) <= max(1, 2e-5 * n), f"{k}: {len(bad)} of {n} differ from the oracle"
                    assert np.abs(got[bad] - pre[k][bad]).max(initial=0) <= (1 if k == "tile_bboxes" else 16), f"{k} off by more than one tile"
                order = orc.depth_order(pre["cam_means"])
                k = int(rng.integers(0, max(1, min(n, 2000))))
                screen, _, _ = orc.composite(order, pre, W, H, limit=k)
                if k > 0:
                    close(R.render(cam, mk(draw_limit=k)).cpu().numpy(), screen.transpose(1, 0, 2))
            # the loader's Morton order: the same frame, bit for bit unless two visible gaussians share a depth exactly
            Rm = renderer.Rasterizer(renderer.GaussianScene.from_packed(packed, sh_degree=degree, spatial_order=True))
            mimg = Rm.render(cam)
            bare = renderer.GaussianScene({k: Rm.scene.t[k] for k in Rm.scene.FIELDS}, sh_degree=degree)   # the same arrays without block bounds
            assert torch.equal(renderer.Rasterizer(bare).render(cam), mimg), "block-level culling changes bits (Morton order)"
            # gaussians at EXACTLY equal depth (the generator plants some) are drawn in scene-index order, which the reference
            # leaves undefined: with ties among the visible ones the oracle is fed the arrays in the scene's order (same gaussians, same
            # tie order) — case-seed 1149722072972822031: 20 ties among 40 412 visible, 0.0086 apart from the file-order frame
            zc = orc.preprocess(packed, ocam, sh_degree=degree)["cam_means"][:, 2]
            zv = zc[zc >= 0.2]
            if len(zv) != len(np.unique(zv)):
                mo = Rm.scene.order
                moimg, _, _ = orc.render({k: np.ascontiguousarray(v[mo]) for k, v in packed.items()}, ocam, sh_degree=degree, want_T=True)
                close(mimg.cpu().numpy(), moimg)
            else:
                close(mimg.cpu().numpy(), oimg)
            R.render(cam)
            assert Rm.last_stats["n_visible"] == R.last_stats["n_visible"] and Rm.last_stats["n_pairs"] == R.last_stats["n_pairs"], "spatial order changes the lists"
            half = renderer.Rasterizer(renderer.GaussianScene.from_packed(packed, sh_degree=degree, sh_half=True, spatial_order=False))
            h = half.render(cam)
            assert torch.equal(half.render(cam, mk(no_footprint_cull=True)), h), "fp16 SH: culling changes bits"
            if float(img.abs().max()) > 0:
                assert psnr(h.cpu().numpy(), img.cpu().numpy()) >= 60.0, "fp16 SH storage below 60 dB"
        except Exception as e:  # noqa: BLE001
            fails += 1
            print(f"FAIL {desc}: {type(e).__name__}: {str(e)[:300]}", flush=True)
        cases += 1
        if cases % 25 == 0:
            print(f"{cases} cases, {fails} failures", flush=True)
    print(f"done: {cases} cases, {fails} failures", flush=True)
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()
