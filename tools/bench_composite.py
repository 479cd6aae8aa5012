"""Times the per-ray compositing kernels alone at the ray and sample counts of iterations of one 800x800 frame
(render_image_test's schedule, N_samples = clamp(N_rays // N_alive, 1, 64)): an early iteration (a quarter of the 640 000
rays alive, 4 samples each) and a late one (10 000 rays, 64 samples each).  Three rays in four use their whole budget,
the others stop after a uniform 0 .. budget - 1 samples; everything comes from one seed."""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ced_nerf_amd import ops
dev = "cuda:0"
def timed(fn, reps=200):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3
def run(n_rays, budget):
    rng = np.random.default_rng(0)
    cnt = np.where(rng.random(n_rays) < 0.75, budget, rng.integers(0, budget, n_rays)).astype(np.int64)
    packed = np.stack([np.cumsum(cnt) - cnt, cnt], 1)
    S = int(cnt.sum())
    t0 = 2.0 + np.repeat(rng.random(n_rays), cnt) + (np.arange(S) - np.repeat(packed[:, 0], cnt)) * 5e-3
    T = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(dev)
    packed, t0, t1 = T(packed, np.int64), T(t0), T(t0 + 5e-3)
    sig, rgbs = T(rng.gamma(0.5, 20.0, S)), T(rng.random((S, 3)))
    rgb = torch.zeros((n_rays, 3), device=dev); op = torch.zeros((n_rays, 1), device=dev); dp = torch.zeros((n_rays, 1), device=dev)
    mask = torch.zeros(n_rays, dtype=torch.bool, device=dev); stats = torch.zeros(2, dtype=torch.int64, device=dev)
    d_color = T(rng.normal(size=(n_rays, 3))); d_op = T(rng.normal(size=n_rays)); d_dp = T(rng.normal(size=n_rays))
    cases = (("composite_prefix_", lambda: ops.composite_prefix_(packed, t0, t1, sig, rgbs, rgb, op, dp)),
             ("composite_step_", lambda: ops.composite_step_(packed, t0, t1, sig, rgbs, rgb, op, dp, 0.999, budget, mask, stats)),
             ("render_weights", lambda: ops.render_weights(packed, t0, t1, sig)),
             ("composite_backward", lambda: ops.composite_backward(packed, t0, t1, sig, rgbs, d_color, d_op, d_dp)))
    for nm, fn in cases:
        print(f"{nm:19s} {n_rays:7d} rays x {budget:2d} ({S:7d} samples): {timed(fn):8.1f} us")
run(160000, 4)
run(10000, 64)
