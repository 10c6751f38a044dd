"""The scene builder of the randomised parity campaign (tools/fuzz_parity.py), in a module of its own: the campaign, the golden
generator (tools/make_golden.py) and the tests (tests/gpu_cases.fuzz_case, which replays a case by its seed) all call this one
function.  It lives under tools/ and needs nothing from tests/, so the tools work with whatever tests/ directory stands next to
them; it imports numpy only, and gsr_amd when a case is built."""
import numpy as np


def build_case(case_seed, max_n=60000):
    """The deterministic scene / frame / camera of one campaign case (also used by tests/ to replay a case by its seed).
    Returns the rng too: the campaign keeps drawing its per-case options from it."""
    from gsr_amd import synthetic, utils

    rng = np.random.default_rng(case_seed)
    n = int(rng.choice([1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, int(rng.integers(1, max_n))]))
    W = int(rng.choice([1, 15, 16, 17, 31, 33, 160, 333, 640, int(rng.integers(1, 1300))]))
    H = int(rng.choice([1, 15, 16, 17, 96, 197, 360, int(rng.integers(1, 800))]))
    gen = synthetic.mip360_like if rng.random() < 0.7 else synthetic.uniform_box
    cols = gen(n, int(rng.integers(0, 1 << 30)))
    shift = float(rng.choice([0.0, 1.0, 2.0, 3.5]))
    for i in range(3):
        cols[f"scale_{i}"] = (cols[f"scale_{i}"] + np.float32(shift)).astype(np.float32)
    if rng.random() < 0.2:  # stacks of exactly equal depth
        k = int(rng.integers(1, 50))
        for c in "xyz":
            cols[c] = np.ascontiguousarray(cols[c][np.arange(n) % k])
    if rng.random() < 0.2:
        cols["opacity"] = np.full_like(cols["opacity"], float(rng.choice([-8.0, 6.0, 12.0])))
    if gen is synthetic.uniform_box:
        pose = synthetic.box_camera()
    else:
        th = rng.uniform(0, 2 * np.pi)
        rad = float(rng.choice([0.5, 2.0, 4.0, 30.0]))
        pose = synthetic.look_at_pose((rad * np.cos(th), rad * np.sin(th), rng.uniform(-1, 2)), (0, 0, 0), 1, "c.png")
    fx = synthetic.pinhole_focal(max(W, 2), float(rng.choice([30.0, 60.0, 100.0])))
    sf = int(rng.choice([1, 2, 4]))
    args = (pose.qvec, pose.tvec, sf * fx, sf * fx, sf * W, sf * H, W, H)
    degree = int(rng.choice([3, 3, 3, 0, 1, 2]))
    return dict(rng=rng, n=n, W=W, H=H, gen=gen, shift=shift, degree=degree, pose=pose, args=args, sf=sf, cols=cols,
                packed=utils.pack_gaussians(cols))
