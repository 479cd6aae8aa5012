"""Timing of the distortion loss (-d) at tools/bench_train.py's shape: 262 144 random rays of the 800x800 D-NeRF-shaped
scene, marched by estimator.sampling with the trained field's density.  Forward + backward to the densities of
  fused     losses.distortion_from_density (ced_distortion_loss_density: weights, loss and d sigma in one pass)
  weights   render.py's _WeightsFn (HIP weights, float64-cumsum backward) + the weights route (ced_distortion_loss)
  torch     a float32 torch closed form on segmented cumsums (the stand-in for torch_efficient_distloss) on _WeightsFn
and train.train_step with -d -ae against every regulariser off (LR 0: the same samples every step)."""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ced_nerf_amd import losses, synthetic as S
from ced_nerf_amd.nerfacc_api import OccGridEstimator, _packed_info_from
from ced_nerf_amd.render import _WeightsFn
from ced_nerf_amd.train import TrainableField, train_step

dev = "cuda:0"; T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
N_RAYS = int(os.environ.get("N_RAYS", "262144"))
sc = S.make_scene("dnerf", 800, 800, "trained"); cfg = sc["cfg"]
est = OccGridEstimator(cfg["aabb"], 128, cfg["grid_levels"]).to(dev); est.set_binaries(T(sc["binaries"]))
field = TrainableField(sc["params"], dev)
o = T(sc["origins"]).reshape(-1, 3); d = T(sc["viewdirs"]).reshape(-1, 3); ts1 = T(sc["timestamps"])
bk = T(sc["render"]["render_bkgd"])
g = torch.Generator(device=dev).manual_seed(0)
idx = torch.randint(0, o.shape[0], (N_RAYS,), device=dev, generator=g)
ro, rd = o[idx].contiguous(), d[idx].contiguous()
ts = ts1.reshape(-1, 1).float().expand(N_RAYS, 1)
fused = field.shared_inference(); fused.train()
sigma_fn = lambda a, b, r: fused.query_rays(ro, rd, r, a, b, ts, want_rgb=False)[1]
torch.manual_seed(0)
ri, t0, t1 = est.sampling(ro, rd, sigma_fn=sigma_fn, near_plane=cfg["near_plane"], far_plane=cfg["far_plane"],
                          render_step_size=cfg["render_step_size"], stratified=True, sigma_field=(fused, ts, True))
t0, t1 = t0.contiguous(), t1.contiguous()
sig0 = sigma_fn(t0, t1, ri).reshape(-1).float().contiguous()
packed = _packed_info_from(ri, N_RAYS)
print(f"{N_RAYS} rays, {t0.shape[0]} samples ({t0.shape[0] / N_RAYS:.2f} per ray, longest ray {int(packed[:, 1].max())})")


def torch_closed_form(w, t0, t1, packed):
    """flatten_eff_distloss's arithmetic in float32 torch: prefix sums by one global cumsum, re-based per ray."""
    m, s = (t0 + t1) / 2, t1 - t0
    cnt = packed[:, 1]
    base = torch.repeat_interleave(packed[:, 0], cnt)
    last = (cnt > 0).nonzero().max() + 1
    cw = torch.cumsum(w, 0); cwm = torch.cumsum(w * m, 0)
    w_prefix = (cw - w) - (cw - w)[base]
    wm_prefix = (cwm - w * m) - (cwm - w * m)[base]
    return ((2 * w * (m * w_prefix - wm_prefix)).sum() + ((1 / 3) * s * w * w).sum()) / last


def route_fused(sig):
    return losses.distortion_from_density(t0, t1, sig, packed)


def route_weights(sig):
    w = _WeightsFn.apply(sig, t0, t1, packed)[0]
    return losses._DistortionFn.apply(w, t0, t1, packed)


def route_torch(sig):
    w = _WeightsFn.apply(sig, t0, t1, packed)[0]
    return torch_closed_form(w, t0, t1, packed)


def timed(fn, reps=50, warm=5):
    """mean ms of forward + backward, CUDA events around `reps` back-to-back calls"""
    for _ in range(warm):
        s = sig0.clone().requires_grad_(); fn(s).backward()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        s = sig0.clone().requires_grad_(); fn(s).backward()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def kernel_only(reps=200):
    from ced_nerf_amd import ops
    for _ in range(5):
        ops.distortion_loss_density(packed, sig0, t0, t1)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        ops.distortion_loss_density(packed, sig0, t0, t1)
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


vals = {k: float(f(sig0.clone().requires_grad_()).detach()) for k, f in
        (("fused", route_fused), ("weights", route_weights), ("torch", route_torch))}
print("loss  " + "  ".join(f"{k} {v:.9g}" for k, v in vals.items()))
print(f"ops.distortion_loss_density alone (loss + d sigma, 2 launches + allocations): {kernel_only() * 1e3:.1f} us")
for name, fn in (("fused", route_fused), ("weights + _WeightsFn", route_weights), ("torch f32 closed form + _WeightsFn", route_torch)):
    print(f"{name:36s} forward + backward: {timed(fn) * 1e3:8.1f} us")

opt = torch.optim.Adam(field.parameters(), lr=0.0, eps=1e-15, fused=True)
target = torch.rand(N_RAYS, 3, device=dev, generator=g)
for label, kw in (("train_step (no regulariser)", {}), ("train_step -d -ae", dict(distortion_loss=True, acc_entropy_loss=True)),
                  ("train_step (no regulariser)", {}), ("train_step -d -ae", dict(distortion_loss=True, acc_entropy_loss=True))):
    n_s = []
    for it in range(13):
        if it == 3:
            torch.cuda.synchronize(); tic = time.perf_counter()
        out = train_step(field, est, opt, ro, rd, ts1, target, cfg["render_step_size"], near_plane=cfg["near_plane"],
                         far_plane=cfg["far_plane"], render_bkgd=bk, **kw)
        n_s.append(out["n_samples"])
    torch.cuda.synchronize(); dt = (time.perf_counter() - tic) / 10
    print(f"{label:28s} {N_RAYS} rays: {dt * 1e3:.2f} ms/step, {np.mean(n_s[3:]):.0f} samples/step, terms {out['loss_terms']}")
