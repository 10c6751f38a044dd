"""GPU: BASELINE.json's configurations at their FULL sizes, through the C ABI, against the CPU oracle.

  configs[1]  garden stand-in    5 834 784 gaussians, 1920x1080, fp32            frame >= 100 dB; integer rects counted vs the oracle
  configs[2]  bicycle stand-in   6 131 954 gaussians, 1920x1080                  fp32 frame >= 100 dB (the bench headline);
                                                                                 fp16-SH storage vs the oracle fed the fp16-rounded
                                                                                 coefficients >= 100 dB; + bf16 frame store >= 55 dB
  configs[4]  uniform_box        20 000 000 gaussians, 3840x2160                 frame >= 100 dB; footprint culling off and 8-shard
                                                                                 reassembly bit-identical at that size
  configs[3]  bicycle stand-in, the whole 25-camera set, 8 interleaved tile-row shards per frame on this GPU, assembled and compared
              bit for bit with the unsharded frames (+ 3 cameras vs the oracle); the gather: tools/dist_check.py under torchrun,
              nccl when the box has >= 2 GPUs, otherwise the same ranks over gloo sharing the one GPU.

The real MipNeRF-360 scenes are not available offline: these are the seeded stand-ins of SURVEY.md §8(d).
Tolerance stated by north_star: PSNR >= 50 dB vs the torch reference; held here: >= 100 dB (fp32), >= 55 dB (bf16 store).
The oracle takes ~10 s (1080p) / ~40 s (4K) on the box's host cores.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, assert_frames_close, psnr
from gpu_cases import namespace

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    return namespace()


def _ring_camera(G, W, H, pose=0):
    p = G.synthetic.ring_cameras(25)[pose]
    fx = G.synthetic.pinhole_focal(W)
    args = (p.qvec, p.tvec, 2 * fx, 2 * fx, 2 * W, 2 * H, W, H)
    return G.renderer.make_camera(*args), G.orc.camera(*args)


def _in_scene_order(packed, scene):
    """The packed arrays as `scene` stores them (the loaders' Morton order).  The reference leaves the mutual order of gaussians at
    EXACTLY equal depth undefined (torch.sort, rasterize.py:425); libgsr and the oracle both resolve such ties by array index, so the
    oracle is fed the arrays in the scene's order: same gaussians, same tie order — a pass never depends on which tied gaussians
    happen to overlap (a mip360_like scene of 6 M holds ~1e5 exact fp32 depth ties)."""
    return packed if scene.order is None else {k: np.ascontiguousarray(v[scene.order]) for k, v in packed.items()}


def _oracle_frame(G, packed, ocam):
    pre = G.orc.preprocess(packed, ocam)
    order = G.orc.depth_order(pre["cam_means"])
    screen, _, drawn = G.orc.composite(order, pre, ocam.width, ocam.height, threads=G.orc.max_threads())
    return screen.transpose(1, 0, 2), pre, drawn


def test_configs2_bicycle_full_size(G):
    """The bench headline (fp32) and configs[2]'s storage options on the bicycle stand-in at 1080p."""
    W, H = 1920, 1080
    packed = G.utils.pack_gaussians(G.synthetic.mip360_like(6_131_954, 361))
    cam, ocam = _ring_camera(G, W, H)
    mk = G.renderer.make_options

    scene = G.renderer.GaussianScene.from_packed(packed)
    oimg, _, drawn = _oracle_frame(G, _in_scene_order(packed, scene), ocam)
    R = G.renderer.Rasterizer(scene)
    img = R.render(cam).cpu().numpy()
    st = dict(R.last_stats)
    assert 0 < st["n_visible"] <= drawn and st["overflow"] == 0
    assert_frames_close(img, oimg)
    print(f"\nbicycle fp32: {psnr(img, oimg):.1f} dB vs oracle, stats {st}")
    del R, scene

    # fp16 SH storage == the fp16-rounded coefficients evaluated in fp32: compare with the oracle fed exactly those
    scene_h = G.renderer.GaussianScene.from_packed(packed, sh_half=True)
    rounded = _in_scene_order(packed, scene_h)
    rounded["sh"] = rounded["sh"].astype(np.float16).astype(np.float32)
    oimg16, _, _ = _oracle_frame(G, rounded, ocam)
    del rounded
    Rh = G.renderer.Rasterizer(scene_h)
    half = Rh.render(cam).cpu().numpy()
    assert_frames_close(half, oimg16)
    db_vs_fp32 = psnr(half, oimg)
    assert db_vs_fp32 >= 75.0, db_vs_fp32                        # fp16 storage alone vs the fp32-coefficient oracle

    # + bf16 frame store (accumulation fp32): 8 mantissa bits of storage; the bar is 50 dB
    both = Rh.render(cam, mk(output_bf16=True))
    assert both.dtype == torch.bfloat16
    assert torch.equal(both, torch.from_numpy(half).to(torch.bfloat16).to(both.device))   # store = RNE of the fp32 frame
    db = psnr(both.float().cpu().numpy(), oimg)
    assert db >= 55.0, db
    print(f"bicycle fp16 SH: {psnr(half, oimg16):.1f} dB vs oracle(fp16-rounded), {db_vs_fp32:.1f} dB vs oracle(fp32); + bf16 store {db:.1f} dB")

    # configs[2] AS WORDED: fp16 SH + bf16 blend ACCUMULATORS (T and the colour sums rounded to bf16 after every gaussian).
    # Measured here on the HIP path, full size; it is why the product keeps fp32 accumulators: the bar is 50 dB.
    acc = Rh.render(cam, mk(accum_bf16=True, output_bf16=True))
    db_acc = psnr(acc.float().cpu().numpy(), oimg)
    print(f"bicycle fp16 SH + bf16 ACCUMULATORS + bf16 store: {db_acc:.1f} dB vs oracle(fp32) -- below / above the 50 dB bar: {'below' if db_acc < 50 else 'above'}")
    assert 20.0 <= db_acc <= db + 1.0, db_acc                    # a real image, and no better than fp32 accumulation


def test_configs1_garden_full_size_and_rect_mismatch_count(G):
    """configs[1] at full size, plus the honest measure of 'integer outputs bit-exact': ocml's expf vs libm's under ceil/floor
    moves a rect by one tile for a gaussian in ~1e5.  Counted here at bench scale, bounded, printed."""
    W, H = 1920, 1080
    N = 5_834_784
    packed = G.utils.pack_gaussians(G.synthetic.mip360_like(N, 360))
    cam, ocam = _ring_camera(G, W, H)
    scene = G.renderer.GaussianScene.from_packed(packed)
    oimg, _, drawn = _oracle_frame(G, _in_scene_order(packed, scene), ocam)
    R = G.renderer.Rasterizer(scene)
    img = R.render(cam).cpu().numpy()
    assert R.last_stats["n_visible"] <= drawn
    assert_frames_close(img, oimg)
    pre = G.orc.preprocess(packed, ocam)   # per-gaussian outputs are compared in FILE order (preprocess_debug answers in file order)
    dbg = R.preprocess_debug(cam)
    tb, pb = dbg["tile_bboxes"].cpu().numpy(), dbg["pixel_bboxes"].cpu().numpy()
    del dbg
    for name, got, ref, step in (("tile_bboxes", tb, pre["tile_bboxes"], 1), ("pixel_bboxes", pb, pre["pixel_bboxes"], 16)):
        diff = np.abs(got - ref)
        bad = np.flatnonzero(diff.any(axis=1))
        print(f"\ngarden {name}: {len(bad)} of {N} gaussians differ from the oracle (max |diff| {int(diff.max())})")
        assert len(bad) <= 2e-5 * N, len(bad)
        assert diff.max() <= step                                  # never by more than one tile


@pytest.fixture(scope="module")
def box4k(G):
    n = int(os.environ.get("GSR_TEST_BOX_N", "20000000"))
    packed = G.utils.pack_gaussians(G.synthetic.uniform_box(n, 20))
    W, H = 3840, 2160
    p = G.synthetic.box_camera()
    fx = G.synthetic.pinhole_focal(W)
    args = (p.qvec, p.tvec, 2 * fx, 2 * fx, 2 * W, 2 * H, W, H)
    scene = G.renderer.GaussianScene.from_packed(packed)          # the loaders' default: along the Morton curve
    # The camera looks down +z from (0, 0, -14): depth = z + 14, and 20 M fp32 draws from U[-10, 10] repeat values — thousands of
    # EXACT depth ties, whose order the reference leaves undefined (torch.sort is unstable) and this library resolves by scene index.
    # The oracle resolves them by ITS index, so it is fed the arrays in the scene's order: same gaussians, same tie order.
    order = scene.order
    packed = {k: np.ascontiguousarray(v[order]) for k, v in packed.items()}
    return packed, scene, G.renderer.make_camera(*args), G.orc.camera(*args)


def test_configs4_box_4k_vs_oracle(G, box4k):
    packed, scene, cam, ocam = box4k
    R = G.renderer.Rasterizer(scene)
    img = R.render(cam).cpu().numpy()
    st = dict(R.last_stats)
    oimg, _, drawn = _oracle_frame(G, packed, ocam)
    assert 0 < st["n_visible"] <= drawn and st["overflow"] == 0
    assert_frames_close(img, oimg)
    print(f"\nbox4k: {psnr(img, oimg):.1f} dB vs oracle, stats {st}")


def test_configs4_box_4k_exactness_properties(G, box4k):
    """At configs[4]'s size: footprint culling changes no bit, and 8 interleaved tile-row shards (single rows here; pairs of rows: the
    configs[3] test) reassemble bit-exactly."""
    _, scene, cam, _ = box4k
    mk = G.renderer.make_options
    R = G.renderer.Rasterizer(scene)
    full, T = R.render(cam, return_T=True)
    culled_pairs = R.last_stats["n_pairs"]
    b, Tb = R.render(cam, mk(no_footprint_cull=True), return_T=True)
    assert torch.equal(full, b) and torch.equal(T, Tb)
    assert culled_pairs < R.last_stats["n_pairs"]
    del b, Tb
    tiles_y = (cam.height + 15) // 16
    out = torch.zeros_like(full)
    Rs = G.renderer.Rasterizer(scene, max_pairs=max(1 << 20, R.max_pairs // 4))
    del R
    for r in range(8):
        strip = Rs.render(cam, mk(tile_row_begin=r, tile_row_step=8, output_layout=2))
        k = len(range(r, tiles_y, 8))
        out.view(tiles_y, 16, cam.width, 3)[r::8] = strip[: k * 16].view(k, 16, cam.width, 3)
    assert torch.equal(out, full)


def test_configs3_bicycle_camera_set_in_8_tile_row_shards(G):
    """configs[3] at its own workload, on one GPU: the bicycle stand-in (6 131 954 gaussians) at 1920x1080 over the WHOLE
    25-camera set, every frame rendered as the 8 interleaved tile-row shards an 8-GPU node would render (TileRowPlan's default: a rank owns every
    8th PAIR of tile rows, rank 0 the ones no remainder falls to; the rank's loop is bench.py's: frames in flight on separate streams, strips into padded wire buffers,
    bounds learned on camera 0 and passed explicitly, ONE stats() per slot after the run) and put together by
    TileRowPlan.assemble (what rank 0 does after the RCCL gather).
      (i)   every camera's assembled frame is bit-identical to its unsharded frame;
      (ii)  three cameras spread over the ring are checked against the CPU oracle at full size (>= 100 dB);
      (iii) the pair-buffer / depth-sort bounds learned on camera 0 hold for the other cameras or are re-learned: a camera
            that exceeds one is reported by the slot's stats() (the frames are chained with GsrOptions.keep_flags) and the
            rank re-renders with room for it — never a silently incomplete frame.
    The gather itself (gloo here, RCCL on a multi-GPU box) is test_configs3_sharded_frame_over_*."""
    from gsr_amd import _lib
    from gsr_amd import dist as gdist

    W, H, NCAM, GPUS = 1920, 1080, 25, 8
    packed = G.utils.pack_gaussians(G.synthetic.mip360_like(6_131_954, 361))
    scene = G.renderer.GaussianScene.from_packed(packed)
    views = [_ring_camera(G, W, H, i) for i in range(NCAM)]
    cams = [v[0] for v in views]
    mk = G.renderer.make_options

    R = G.renderer.Rasterizer(scene)
    R.fit_pairs(cams[0])
    learned0 = (R.max_pairs, R.sort_passes)
    full = [R.render(c) for c in cams]            # render() verifies every frame and re-learns a bound that does not hold
    print(f"\nunsharded: bounds learned on camera 0 {learned0}, after the set {(R.max_pairs, R.sort_passes)}")
    del R

    plan = gdist.TileRowPlan(H, W, GPUS)
    relearned = []
    # every frame's wire buffer (strip padded to the longest rank's rows), allocated and zeroed BEFORE any slot stream writes
    # into it: FramesInFlight leaves the ordering of output buffers to the caller
    wire = torch.zeros((GPUS, NCAM) + tuple(plan.padded_shape()), device="cuda")
    torch.cuda.synchronize()
    for r in range(GPUS):
        so = plan.shard_options(r)
        rows = len(plan.rows[r]) * 16
        fif = G.renderer.FramesInFlight(scene, slots=2)
        r0 = fif.rasterizers[0]
        r0.fit_pairs(cams[0], mk(**so))
        fif.set_max_pairs(r0.max_pairs)
        fif.set_sort_passes(r0.sort_passes)
        for attempt in range(5):
            opts = r0.bounded(mk(**so))
            for i, c in enumerate(cams):
                fif.submit(c, opts, out=wire[r, i, :rows])
            need, passes = 0, 0
            for k in range(fif.slots):
                try:
                    fif.stats(k)
                except _lib.GsrPairOverflow:
                    need = max(need, fif.rasterizers[k].last_stats["n_pairs_bbox"])
                except _lib.GsrSortPasses:
                    passes = max(passes, fif.rasterizers[k].last_stats["sort_passes"])
            if not need and not passes:
                break
            relearned.append((r, attempt, need, passes))
            if need:
                fif.set_max_pairs(need + need // 8 + 1024)
            if passes:
                fif.set_sort_passes(passes)
        else:
            pytest.fail(f"rank {r}: bounds still exceeded after 5 runs: {relearned}")
        fif.synchronize()
        del fif, r0
    print(f"shard runs that re-learned a bound (rank, attempt, pairs needed, passes needed): {relearned}")
    for i in range(NCAM):
        frame = plan.assemble([wire[r][i] for r in range(GPUS)])
        assert torch.equal(frame, full[i]), f"camera {i}: the 8-shard frame differs from the unsharded one"
    del wire
    ordered = _in_scene_order(packed, scene)
    for i in (0, 8, 17):
        oimg, _, _ = _oracle_frame(G, ordered, views[i][1])
        img = full[i].cpu().numpy()
        assert_frames_close(img, oimg)
        print(f"camera {i}: {psnr(img, oimg):.1f} dB vs oracle")


def test_configs3_batches_of_sharded_frames_over_gloo_ranks_sharing_the_gpu(G):
    """The same with bench.py's default schedule since round 5: every rank renders its strips of `views` consecutive frames through
    ONE launch sequence (Rasterizer.enqueue_batch into the padded wire buffer's strided strips) and ONE gather moves the batch
    (dist.ShardedFrames(views = 2); 7 frames, so the last batch is partial).  Rank 0 compares every frame with its unsharded render."""
    p = _run_dist_check("gloo", 3, {"GSR_DIST_CHECK_VIEWS": "2", "GSR_DIST_CHECK_SLOTS": "2"})
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "DIST_CHECK_OK" in p.stdout


def _run_dist_check(backend, ranks, extra_env=None, timeout=600):
    env = dict(os.environ)
    env["GSR_BENCH_BACKEND"] = backend
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.update(extra_env or {})
    port = 29500 + (os.getpid() % 2000)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(REPO, "tools", "dist_check.py")]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)


def test_configs3_sharded_frame_over_gloo_ranks_sharing_the_gpu(G):
    """The N>1 path of bench.py (shard options, double-buffered gather, de-interleave) with real GPU strips: 3 ranks on this
    box's GPU, strips staged through the host for gloo.  Rank 0 compares the gathered frame with its own unsharded render."""
    p = _run_dist_check("gloo", 3)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "DIST_CHECK_OK" in p.stdout


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs >= 2 GPUs for RCCL")
def test_configs3_sharded_frame_over_rccl(G):
    """One rank per GPU, RCCL gather over xGMI: frames bit-identical to the single-GPU frame, for several frames in a row
    (pins the buffer-reuse ordering between gather_async on the communicator stream and the next frame's render)."""
    ranks = min(torch.cuda.device_count(), 4)  # + this pytest process: within the box's limit of 6 GPU processes
    p = _run_dist_check("nccl", ranks)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "DIST_CHECK_OK" in p.stdout


def _run_bench_multi(backend, ranks, extra=(), timeout=900):
    env = dict(os.environ)
    env["GSR_BENCH_BACKEND"] = backend
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    port = 31500 + (os.getpid() % 2000)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(REPO, "bench.py"), "--gpus", str(ranks), "--steps", "6", "--warmup", "2",
           "--gaussians", "400000", "--full", "--legs", "", "--no-psnr", "--no-cpu-baseline", *extra]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)


def _check_bench_line(p, ranks):
    import json

    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["n_gpus"] == ranks and r["scaling"] == "strong" and r["steps"] == 6 and r["warmup"] == 2
    assert r["value"] > 0 and abs(r["value"] * r["ms_per_step"] - 1e3) < 1e-3 * 1e3
    assert "tile rows interleaved" in r["config"]["sharding"] and str(ranks) in r["config"]["sharding"]
    assert r["config"]["gaussians"] == 400000 and r["metric"].startswith("frames/sec @1080p")
    assert r["roofline"]["frac"] > 0 and r["roofline"]["avg_kernel_ms"] > 0 and "rank 0's shard" in r["roofline"]["note"]
    assert r["stats_rank0_shard"]["overflow"] == 0 and r["stats"]["overflow"] == 0 and r["stats"]["n_visible"] > 0
    assert r["single_stream"]["frames_per_s"] > 0
    return r


def test_bench_py_with_two_ranks_over_gloo(G):
    """The driver's multi-GPU command line — `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...` — with N = 2
    ranks sharing this box's GPU over gloo (GSR_BENCH_BACKEND), a small scene, no legs: the whole N > 1 half of bench.py
    (sharded frames in flight, asynchronous gather, max-over-ranks timing, rank 0's roofline of its shard, every slot's counters
    read after the timed loop) must run to ONE well-formed JSON line.  The first 8-GPU lease must not be spent on a traceback."""
    r = _check_bench_line(_run_bench_multi("gloo", 2), 2)
    print(f"\nbench.py --gpus 2 over gloo (ranks share the GPU): {r['value']:.0f} frames/s, {r['ms_per_step']:.3f} ms per frame")


def test_bench_py_plain_run_is_lean_and_dumps_the_last_frame(G, tmp_path):
    """`bench.py --gpus 1` without --full: the headline alone (no single-stream leg, roofline, oracle, CPU baseline or other legs),
    exactly --steps timed frames, and --dump-outputs writes the last timed frame: camera 0 of the same seeded scene, bit-identical
    to a single-view render of it."""
    import json

    import bench

    steps, n = 7, 400_000
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
           "--gaussians", str(n), "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["n_gpus"] == 1 and r["steps"] == steps and r["warmup"] == 2 and r["config"]["gaussians"] == n
    assert r["unit"] == "frames/s" and r["higher_is_better"] is True and r["dtype"] == "f32" and r["metric"].startswith("frames/sec @1080p")
    assert r["value"] > 0 and abs(r["value"] * r["ms_per_step"] - 1e3) < 1e-3 * 1e3
    assert not {"single_stream", "roofline", "stage_ms", "psnr_vs_oracle_db", "cpu_baseline", "early_out", "configs2", "camera_set",
                "shards8", "file_order", "garden", "box4k"} & set(r)
    img = np.load(tmp_path / "frame.npy")
    assert img.dtype == np.float32 and img.shape == (1080, 1920, 3) and img.max() > 0.05

    gen, _, seed, W, H, _ = bench.WORKLOADS["bicycle"]
    packed = G.utils.pack_gaussians(getattr(G.synthetic, gen)(n, seed))
    scene = G.renderer.GaussianScene.from_packed(packed, device="cuda:0", spatial_order=True)
    cam, _ = _ring_camera(G, W, H, 0)
    ref = G.renderer.Rasterizer(scene).render(cam, G.renderer.make_options()).cpu().numpy()
    assert np.array_equal(img, ref)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs >= 2 GPUs for RCCL")
def test_bench_py_with_two_ranks_over_rccl(G):
    r = _check_bench_line(_run_bench_multi("nccl", 2), 2)
    print(f"\nbench.py --gpus 2 over RCCL: {r['value']:.0f} frames/s, {r['ms_per_step']:.3f} ms per frame")
