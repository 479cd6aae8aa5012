"""Timing of the evaluation metrics (csrc/metrics.hip) against a float32 torch restatement of the same algorithm on the GPU
(F.conv2d with groups, F.avg_pool2d: what pytorch_msssim runs), on
  a batch of 16 800x800x3 pairs and one 536x960x3 pair (MS-SSIM + MSE, device events, after warm-up), and
  metrics.evaluate_views on 8 synthetic 800x800 D-NeRF views, split into render and metric time.
Usage: python tools/bench_metrics.py [--iters 20] [--out FILE] [--batch-only]
Per-level kernel times: run it with --batch-only under `rocprofv3 --kernel-trace -d DIR -o kt --output-format csv -- ...`,
then `python tools/bench_metrics.py --levels-from DIR/.../kt_kernel_trace.csv` (no GPU needed) splits the ced_ssim launches
by pyramid level (the level follows from the grid: image size and tile count)."""
import argparse, os, sys, time
import numpy as np, torch, torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ced_nerf_amd import metrics as M, ops, synthetic as S
from ced_nerf_amd.model import DNGPradianceField
from ced_nerf_amd.nerfacc_api import OccGridEstimator
from ced_nerf_amd.utils import Rays, render_image_test

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--out", default=None)
ap.add_argument("--batch-only", action="store_true", help="only the two batch timings (for a kernel trace)")
ap.add_argument("--levels-from", default=None, metavar="CSV", help="split a rocprofv3 kernel trace by level and exit")
args = ap.parse_args()

SHAPES = ((16, 800, 800), (1, 536, 960))


def split_levels(path):
    """Kernel time of every ced_ssim launch of a trace, grouped by (shape, level) via the grid of each level's launch."""
    import collections, csv
    tiles = {}
    for n, h0, w0 in SHAPES:
        h, w = h0, w0
        for lv in range(5):
            tiles[((h - 10 + 15) // 16) * ((w - 10 + 31) // 32) * 256, 3, n] = f"{n} x {h0}x{w0} level {lv} ({h}x{w})"
            h, w = (h + 1) // 2, (w + 1) // 2
    acc = collections.defaultdict(list)
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"]
        if "ssim" not in name:
            continue
        grid = (int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]), int(r["Grid_Size_Z"]))
        short = name.split("(")[0].replace("void ", "")
        key = tiles.get(grid, f"{short} (grid {grid})") if "level" in name else f"{short} (grid {grid})"
        acc[key].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for key, v in sorted(acc.items()):
        print(f"{key:60s} {len(v):5d} launches  median {sorted(v)[len(v) // 2]:8.1f} us")


if args.levels_from:
    split_levels(args.levels_from)
    sys.exit(0)
dev = "cuda:0"
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def torch_ms_ssim(X, Y, data_range=1.0):
    """pytorch_msssim.ms_ssim's arithmetic in float32 torch (size_average=False)."""
    Ch = X.shape[1]
    g = torch.tensor(M.gaussian_window(), device=X.device)
    wh, ww = g.reshape(1, 1, -1, 1).repeat(Ch, 1, 1, 1), g.reshape(1, 1, 1, -1).repeat(Ch, 1, 1, 1)
    filt = lambda t: F.conv2d(F.conv2d(t, wh, groups=Ch), ww, groups=Ch)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    w = X.new_tensor(M.MS_SSIM_WEIGHTS)
    mcs = []
    for lv in range(5):
        mx, my = filt(X), filt(Y)
        sxx, syy, sxy = filt(X * X) - mx * mx, filt(Y * Y) - my * my, filt(X * Y) - mx * my
        cs_map = (2 * sxy + c2) / (sxx + syy + c2)
        ss = (((2 * mx * my + c1) / (mx * mx + my * my + c1)) * cs_map).flatten(2).mean(-1)
        if lv < 4:
            mcs.append(torch.relu(cs_map.flatten(2).mean(-1)))
            pad = [s % 2 for s in X.shape[2:]]
            X, Y = F.avg_pool2d(X, kernel_size=2, padding=pad), F.avg_pool2d(Y, kernel_size=2, padding=pad)
    v = torch.prod(torch.stack(mcs + [torch.relu(ss)]) ** w.view(-1, 1, 1), dim=0)
    return v.mean(1)


def hip(X, Y):
    return ops.ssim(X, Y, M.gaussian_window(), 5, weights=M.MS_SSIM_WEIGHTS, data_range=1.0, want_mean=False,
                    want_mse=True)[0]


def torch_path(X, Y):
    v = torch_ms_ssim(X, Y)
    return v, ((X - Y) ** 2).flatten(1).mean(1)


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3       # us per call


g = torch.Generator(device=dev).manual_seed(0)
say(f"device: {torch.cuda.get_device_name(0)}")
for n, h, w in SHAPES:
    X = torch.rand((n, h, w, 3), device=dev, generator=g)
    Y = (X + 0.05 * torch.randn((n, h, w, 3), device=dev, generator=g)).clamp(0, 1)
    Xp, Yp = X.permute(0, 3, 1, 2), Y.permute(0, 3, 1, 2)               # the renders' [H,W,3] layout, read in place
    Xc, Yc = Xp.contiguous(), Yp.contiguous()
    t_hip = timed(lambda: hip(Xp, Yp), args.iters)
    t_hip_c = timed(lambda: hip(Xc, Yc), args.iters)
    t_torch = timed(lambda: torch_path(Xc, Yc), max(3, args.iters // 4))
    d = float((hip(Xp, Yp) - torch_path(Xc, Yc)[0]).abs().max())
    say(f"{n} x {h}x{w}x3 pairs: HIP ms_ssim+mse {t_hip:9.1f} us ({t_hip / n:7.1f} us/pair; contiguous input "
        f"{t_hip_c / n:7.1f} us/pair)   torch f32 restatement {t_torch:9.1f} us ({t_torch / n:7.1f} us/pair)   "
        f"speed-up {t_torch / t_hip:5.1f}x   max |HIP - torch f32| {d:.1e}")

if args.batch_only:
    sys.exit(0)

# evaluate_views on 8 synthetic 800x800 D-NeRF views
sc = S.make_scene("dnerf", 800, 800, "trained")
cfg = sc["cfg"]
field = DNGPradianceField.from_params(sc["params"], dev).eval()
est = OccGridEstimator(cfg["aabb"], cfg["grid_resolution"], cfg["grid_levels"]).to(dev)
est.set_binaries(T(sc["binaries"]))
rk = dict(sc["render"]); bkgd = T(rk.pop("render_bkgd"))
views = []
for k in range(8):
    c2w = S.look_at_c2w(cfg["radius"], 30.0, 15.0 * k, cfg["opengl"])
    o, dd = S.make_camera_rays(800, 800, cfg["camera_angle_x"], c2w, cfg["opengl"])
    rays = Rays(T(o), T(dd))
    t = T(np.array([[0.1 * k]], np.float32))
    gt = render_image_test(1024, field, est, rays, render_bkgd=bkgd, timestamps=t + 0.05, **rk)[0].clone()
    views.append(dict(rays=rays, pixels=gt, timestamps=t, color_bkgd=bkgd))


def render_only():
    return [render_image_test(1024, field, est, v["rays"], render_bkgd=bkgd, timestamps=v["timestamps"], **rk)[0]
            for v in views]


frames = render_only()
pix = torch.stack([v["pixels"] for v in views])
rgbs = torch.stack(frames)
reps = 3
for fpc in (1, 4):
    M.evaluate_views(field, est, views, 1024, frames_per_call=fpc, **rk)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(reps):
    render_only()
torch.cuda.synchronize()
t_render = (time.perf_counter() - t0) / reps / 8 * 1e3
t_metric1 = timed(lambda: [M._view_metrics(rgbs[i:i + 1], pix[i:i + 1]) for i in range(8)], args.iters) / 8
t_metric8 = timed(lambda: M._view_metrics(rgbs, pix), args.iters) / 8
for fpc in (1, 4):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        res = M.evaluate_views(field, est, views, 1024, frames_per_call=fpc, **rk)
    t_eval = (time.perf_counter() - t0) / reps / 8 * 1e3
    say(f"evaluate_views 8 x 800x800 D-NeRF views, frames_per_call={fpc}: {t_eval:7.3f} ms/view "
        f"(psnr_avg {res['psnr_avg']:.3f} dB, ssim_avg {res['ssim_avg']:.5f}, {sum(res['n_samples']) / 8:.0f} samples/view)")
say(f"  render_image_test alone: {t_render:7.3f} ms/view;  metrics (ms_ssim + mse + psnr) per view: "
    f"{t_metric1:7.1f} us one view per call, {t_metric8:7.1f} us in one call of 8  "
    f"= {100 * t_metric1 / (t_render * 1e3):.2f} % / {100 * t_metric8 / (t_render * 1e3):.2f} % of the render")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
