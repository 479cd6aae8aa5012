"""Timing of DyNeRF's importance-sampled batch on the DyNeRF shape (19 cameras x 300 frames of 338 x 253 RGB, 1.62 G cells,
so the pool path: 2 000 000 candidates), num_rays 65 536:
  (a) TrainViews.batch_importance (csrc/train_batch.hip);
  (b) the reference's formulation (dnerf_3d_video_IS.py:401-440 + its ray generation) in torch on the same device:
      randint + gather + multinomial + index arithmetic + pinhole rays and pixel gather;
  (c) the uniform TrainViews.batch;
and of the three weight-map kernels (csrc/importance.hip) with the fraction of the HBM peak they reach, counting the
bytes each must move once (its inputs read once, its output written once).
Device events around `--iters` back-to-back calls after `--warmup` calls, repeated `--repeats` times: median and range.
Usage: python tools/bench_importance_batch.py [--cameras 19 --frames 300 --width 338 --height 253] [--out FILE]"""
import argparse, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ced_nerf_amd import importance, synthetic as S
from ced_nerf_amd.trainset import TrainViews

ap = argparse.ArgumentParser()
ap.add_argument("--cameras", type=int, default=19)
ap.add_argument("--frames", type=int, default=300)
ap.add_argument("--width", type=int, default=338)
ap.add_argument("--height", type=int, default=253)
ap.add_argument("--num-rays", type=int, default=65536)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--hbm-tbps", type=float, default=8.0, help="HBM peak the fractions refer to (MI355X: 8 TB/s)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = "cuda:0"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, iters=None):
    """Milliseconds per call: (median, min, max) over the repeats."""
    iters = iters or args.iters
    for _ in range(args.warmup):
        fn()
    out = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return float(np.median(out)), min(out), max(out)


C_, T_, H, W = args.cameras, args.frames, args.height, args.width
V = C_ * T_
g = torch.Generator(device=dev).manual_seed(0)
# a static background per camera with noise and a moving bright region, made on the device frame by frame
images = torch.empty((V, H, W, 3), dtype=torch.uint8, device=dev)
for c in range(C_):
    base = torch.randint(40, 200, (H, W, 3), device=dev, generator=g)
    for t in range(T_):
        f = base + torch.randint(-3, 4, (H, W, 3), device=dev, generator=g)
        x0 = (7 * t + 13 * c) % (W - 40)
        f[H // 3: H // 3 + 40, x0: x0 + 40] += 60
        images[c * T_ + t] = f.clamp_(0, 255).to(torch.uint8)
focal = 0.5 * W / np.tan(0.45)
K = np.array([[focal, 0, W / 2.0], [0, focal, H / 2.0], [0, 0, 1]], np.float32)
c2w = np.stack([S.look_at_c2w(2.5, 10.0, 10.0 * (v // T_), False) for v in range(V)])
ts = np.tile(np.linspace(0.0, 1.0, T_, dtype=np.float32), C_)
views = TrainViews.pinhole(images, K, c2w, ts, opengl=False, device=dev, view_mode="one_per_step")
say(f"clip: {C_} cameras x {T_} frames of {W} x {H} RGB = {images.numel() / 1e9:.3f} GB, {V * H * W / 1e6:.1f} M cells; "
    f"{args.iters} calls per timing, {args.warmup} warm-up, {args.repeats} repeats (median [min, max])")

# -- weight kernels -----------------------------------------------------------------------------------------------------
n_px = V * H * W
med = importance.temporal_median(views, C_)
jobs = [("temporal_median", lambda: importance.temporal_median(views, C_), 3 * n_px + 3 * C_ * H * W),
        ("isg_weights", lambda: importance.isg_weights(views, C_, median=med), 3 * n_px + 4 * n_px),
        ("ist_weights(shift 25)", lambda: importance.ist_weights(views, C_), 3 * n_px + 4 * n_px)]
for name, fn, nbytes in jobs:
    ms, lo, hi = timed(fn, iters=3)
    tbps = nbytes / (ms * 1e-3) / 1e12
    say(f"{name:24s} {ms:9.3f} ms [{lo:.3f}, {hi:.3f}]  {nbytes / 1e9:6.2f} GB once -> {tbps:5.2f} TB/s = "
        f"{100.0 * tbps / args.hbm_tbps:4.1f} % of {args.hbm_tbps:g} TB/s")
isg = importance.isg_weights(views, C_, median=med).reshape(-1)
del med

# -- batches ------------------------------------------------------------------------------------------------------------
step = [0]


def ours():
    step[0] += 1
    return views.batch_importance(args.num_rays, step[0], isg, bkgd="random", seed=1)


def uniform():
    step[0] += 1
    return views.batch(args.num_rays, step[0], bkgd="random", seed=1)


Kt, c2wt = torch.from_numpy(K).to(dev), torch.from_numpy(c2w).to(dev)


def reference_torch(pool=2_000_000):
    """fetch_data (dnerf_3d_video_IS.py:401-466) in torch: pool, multinomial, cell -> pixel, pixels / 255, OpenCV rays."""
    subset = torch.randint(0, isg.numel(), (pool,), dtype=torch.int64, device=dev)
    samples = torch.multinomial(isg[subset], args.num_rays)
    index = subset[samples]
    image_id = torch.div(index, H * W, rounding_mode="floor")
    y = torch.remainder(index, H * W).div(W, rounding_mode="floor")
    x = torch.remainder(index, H * W).remainder(W)
    rgb = images[image_id, y, x] / 255.0
    cam = c2wt[image_id]
    dirs = torch.stack([(x - Kt[0, 2] + 0.5) / Kt[0, 0], (y - Kt[1, 2] + 0.5) / Kt[1, 1], torch.ones_like(x, dtype=torch.float32)], -1)
    d = (dirs[:, None, :] * cam[:, :3, :3]).sum(-1)
    origins = cam[:, :3, 3]
    viewdirs = d / torch.linalg.norm(d, dim=-1, keepdim=True)
    bk = torch.rand(3, device=dev)
    return origins, viewdirs, rgb, bk


res = {}
for name, fn in (("(a) batch_importance", ours), ("(b) torch formulation", reference_torch), ("(c) uniform batch", uniform)):
    ms, lo, hi = timed(fn)
    res[name] = ms
    say(f"{name:24s} {ms:9.3f} ms [{lo:.3f}, {hi:.3f}]  {args.num_rays} rays")
say(f"(a) / (b) = {res['(a) batch_importance'] / res['(b) torch formulation']:.2f}, "
    f"(a) / (c) = {res['(a) batch_importance'] / res['(c) uniform batch']:.1f}")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
