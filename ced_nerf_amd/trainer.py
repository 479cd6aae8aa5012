"""The training loop of train_real.py:185-520 on this package's pieces.

`fit` draws each step's batch with the one-launch sampler (`trainset.TrainViews.batch`, or DyNeRF's importance sampler
`TrainViews.batch_importance` when given sampling weights), refreshes the occupancy grid,
runs `train.train_step` (HIP sampling, field, compositing, losses) under the reference's optimiser, grad scaler,
learning-rate schedule and dynamic ray batch, and evaluates held-out views with `metrics.evaluate_views`.

    python -m ced_nerf_amd.trainer --data_root DATA --scene lego [-df -f -w -te -ta -o -d -wr -ae] [--max_steps N]

trains a scene folder with the flags of opt.py and prints the reference's progress and evaluation lines.  The scene
name picks the loader and the preset (`scenes.preset_of`): D-NeRF synthetic, HyperNeRF (`vrig_chicken`, ...) or DyNeRF
(`coffee_martini`, ...; importance-sampled by the folder's weight files or by maps computed on the device).
`--load_model PATH` skips training; `--render_video DIR` writes the render path's frames as PNGs.
"""
from __future__ import annotations

import argparse
import math
import os
import time
from typing import Dict, Optional

import numpy as np
import torch

from . import synthetic
from .metrics import evaluate_views
from .nerfacc_api import OccGridEstimator
from .train import CameraRefinement, TrainableField, next_num_rays, refresh_occupancy, train_step
from .trainset import BKGD_MODES, CAMERA_PINHOLE, VIEW_MODES, TrainViews


def _preset(name: str, max_steps: int, init_batch_size: int, target_sample_batch_size: int, lr: float, milestones,
            train_bkgd: str, test_bkgd: str, view_mode: str) -> Dict:
    c = synthetic.CONFIGS[name]          # the scene constants this package already keeps (train_real.py:86-175)
    return dict(max_steps=max_steps, init_batch_size=init_batch_size, target_sample_batch_size=target_sample_batch_size,
                lr=lr, weight_decay=0.0, aabb=list(c["aabb"]), near_plane=c["near_plane"], far_plane=c["far_plane"],
                moving_step=c["moving_step"], hash_dst_resolution=c["hash_max_res"],
                grid_resolution=c["grid_resolution"], grid_levels=c["grid_levels"],
                render_step_size=c["render_step_size"], alpha_thre=c["alpha_thre"], cone_angle=c["cone_angle"],
                milestones=tuple(milestones), train_bkgd=train_bkgd, test_bkgd=test_bkgd, view_mode=view_mode,
                log2_hashmap_size=21)


# train_real.py:85-182.  milestones are (numerator, denominator) pairs: milestone = max_steps * num // den, the
# reference's integer arithmetic.  Backgrounds: D-NeRF passes no color_bkgd_aug (train_real.py:101), whose default is
# white; HyperNeRF black; DyNeRF random for training and black for evaluation.  View mode: D-NeRF batches over images
# (a view per ray), HyperNeRF draws one view per step.
PRESETS: Dict[str, Dict] = {
    "dnerf": _preset("dnerf", 20000, 1024, 1 << 18, 1e-2, ((1, 2), (3, 4), (9, 10)), "white", "white", "per_ray"),
    "hypernerf": _preset("hypernerf", 20000, 1024, 1 << 18, 1e-2, ((1, 2), (3, 4), (9, 10)), "black", "black",
                         "one_per_step"),
    # DyNeRF's ISG / IST importance sampling (dnerf_3d_video_IS.py:401-440) is fit's `sampling_weights` argument, with the
    # maps of ced_nerf_amd.importance; without it the rays are uniform.
    "dynerf": _preset("dynerf", 40000, 1024, 1 << 20, 1e-2, ((1, 2), (3, 4), (5, 6), (9, 10)), "random", "black",
                      "one_per_step"),
}

def milestone_steps(milestones, max_steps: int):
    return [max_steps * num // den for num, den in milestones]


def make_scheduler(optimizer, max_steps: int, milestones):
    """train_real.py:278-290: LinearLR(0.01 -> 1 over 100 steps) chained with MultiStepLR(milestones, 0.33)."""
    return torch.optim.lr_scheduler.ChainedScheduler([
        torch.optim.lr_scheduler.LinearLR(optimizer, start_factor=0.01, total_iters=100),
        torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=milestone_steps(milestones, max_steps), gamma=0.33),
    ])


def resolve_config(preset: str = "dnerf", max_steps: Optional[int] = None, **overrides) -> Dict:
    """The preset's constants with `overrides` applied; ValueError on an unknown preset, key or mode."""
    if preset not in PRESETS:
        raise ValueError(f"preset={preset!r}: one of {sorted(PRESETS)}")
    cfg = dict(PRESETS[preset])
    unknown = set(overrides) - set(cfg)
    if unknown:
        raise ValueError(f"unknown settings {sorted(unknown)} (known: {sorted(cfg)})")
    cfg.update(overrides)
    if max_steps is not None:
        cfg["max_steps"] = int(max_steps)
    if cfg["max_steps"] < 1:
        raise ValueError(f"max_steps must be >= 1, got {cfg['max_steps']}")
    for key in ("train_bkgd",):
        if cfg[key] not in BKGD_MODES:
            raise ValueError(f"{key}={cfg[key]!r}: one of {sorted(BKGD_MODES)}")
    if cfg["test_bkgd"] not in ("white", "black"):
        raise ValueError(f"test_bkgd={cfg['test_bkgd']!r}: 'white' or 'black'")
    if cfg["view_mode"] not in VIEW_MODES:
        raise ValueError(f"view_mode={cfg['view_mode']!r}: one of {sorted(VIEW_MODES)}")
    if int(cfg["init_batch_size"]) < 1:
        raise ValueError(f"init_batch_size must be >= 1, got {cfg['init_batch_size']}")
    return cfg


def fit(train_views: TrainViews, test_views: Optional[TrainViews] = None, preset: str = "dnerf",
        max_steps: Optional[int] = None, seed: int = 42, *, use_div_offsets: bool = False,
        use_time_embedding: bool = False, use_time_attenuation: bool = False, use_feat_predict: bool = False,
        use_weight_predict: bool = False, table_dtype=np.float16, distortion_loss: bool = False,
        acc_entropy_loss: bool = False, opacity_loss: bool = False, weight_rgbper: bool = False,
        eval_every: int = 0, log_every: int = 10000, save_path: Optional[str] = None, verbose: bool = True,
        sampling_weights: Optional[torch.Tensor] = None, weights_subsampled: int = 1,
        ist_weights: Optional[torch.Tensor] = None, ist_from_step: Optional[int] = None, refine_poses: bool = False,
        refine_times: bool = False, refine_lr: float = 1e-3, **overrides) -> Dict:
    """Trains a field on `train_views` as train_real.py:185-520 does and evaluates it on `test_views`.

    Setup: OccGridEstimator(aabb, grid_resolution, grid_levels); a TrainableField with the reference's initialisation
    (synthetic.init_field_params(regime="init") on estimator.aabbs[-1]) and the flags of train_real.py:253-265
    (table_dtype float16 is the reference's table; float32 also trains); Adam(lr, eps=1e-15, fused) -- apex FusedAdam's
    counterpart; GradScaler(2**10); LinearLR + MultiStepLR.  Per step, in the reference's order: batch, occupancy
    refresh (every 16 steps), train_step (MSE colour loss, the enabled regularisers -d -ae -o -wr, the grad scaler),
    dynamic num_rays, scheduler.  A step with no samples is skipped (train_real.py:351-352): no optimiser, scaler or
    scheduler step, num_rays unchanged.  Steps 0 .. max_steps, as the reference's range(max_steps + 1).

    `sampling_weights` (DyNeRF, dnerf_3d_video_IS.py:401-440): a float32 device tensor of V * (H // s) * (W // s) cell
    weights, s = `weights_subsampled` (importance.isg_weights(...).reshape(-1), or the reference's isg_weights.pt); the
    batch is then `TrainViews.batch_importance`, num_rays // s^2 cells without replacement, and the dynamic ray count
    follows the number of rays returned.  From step `ist_from_step` on the map is `ist_weights` (the reference's
    switch_to_ist, which train_real.py:301-309 has commented out: by default ISG throughout).  The history records then
    carry "sampling": "isg" or "ist".  Without `sampling_weights` the batches are the uniform ones.

    refine_poses / refine_times: a `train.CameraRefinement` over the training views (a rotation and a shift of the
    camera, a time offset, per view; zero at the start) is trained with the field, in a parameter group of its own with
    learning rate refine_lr under the same schedule; the batches then carry their view indices.  Evaluation uses the
    test views' own poses.  The result's "refinement" is the module's state dict (None when off) and the saved file
    gains a "camera_refinement" key.

    `overrides` replace preset constants (max_steps, target_sample_batch_size, lr, log2_hashmap_size, ...).
    Returns {"field", "inference", "estimator", "train_seconds", "history", "eval", "evals", "config", "refinement"}: history holds a
    dict per step (step, lr, num_rays, n_samples, loss, scale, skipped, occ_refreshed, seconds: the loop's wall time
    when the step's loss had been read back, evaluations excluded); eval is evaluate_views' result
    on test_views after the last step (None without test views); evals the (step, result) pairs of every eval_every.
    save_path: torch.save({"radiance_field": inference.state_dict(), "occupancy_grid": estimator.state_dict()})."""
    cfg = resolve_config(preset, max_steps, **overrides)
    if sampling_weights is None and (ist_weights is not None or ist_from_step is not None):
        raise ValueError("ist_weights / ist_from_step switch an importance-sampled run: sampling_weights is missing")
    if (ist_weights is None) != (ist_from_step is None):
        raise ValueError("ist_weights and ist_from_step go together")
    dev = train_views.device
    if dev.type != "cuda":
        raise NotImplementedError("fit trains on the GPU: the views must be on a cuda device")
    torch.manual_seed(seed)                    # the occupancy refresh's draws (train_real.py:82, set_random_seed(42))
    np.random.seed(seed)
    steps = int(cfg["max_steps"])
    flags = dict(use_div_offsets=use_div_offsets, use_time_embedding=use_time_embedding,
                 use_time_attenuation=use_time_attenuation)
    estimator = OccGridEstimator(cfg["aabb"], cfg["grid_resolution"], cfg["grid_levels"]).to(dev)
    params = synthetic.init_field_params(estimator.aabbs[-1].cpu().numpy(), cfg["moving_step"], cfg["hash_dst_resolution"],
                                         int(cfg["log2_hashmap_size"]), regime="init", seed=seed, table_dtype=table_dtype,
                                         **flags)
    field = TrainableField(params, dev, use_feat_predict=use_feat_predict, use_weight_predict=use_weight_predict, seed=seed)
    inference = field.shared_inference()
    optimizer = torch.optim.Adam(field.parameters(), lr=cfg["lr"], eps=1e-15, weight_decay=cfg["weight_decay"], fused=True)
    refinement = None
    if refine_poses or refine_times:
        refinement = CameraRefinement(len(train_views), poses=refine_poses, times=refine_times).to(dev)
        optimizer.add_param_group(dict(params=list(refinement.parameters()), lr=float(refine_lr)))
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10)
    scheduler = make_scheduler(optimizer, steps, cfg["milestones"])
    losses = dict(distortion_loss=distortion_loss, acc_entropy_loss=acc_entropy_loss, opacity_loss=opacity_loss,
                  weight_rgbper=weight_rgbper)
    render = dict(near_plane=cfg["near_plane"], far_plane=cfg["far_plane"], render_step_size=cfg["render_step_size"],
                  cone_angle=cfg["cone_angle"], alpha_thre=cfg["alpha_thre"])

    def evaluate():
        if test_views is None:
            return None
        return evaluate_views(inference, estimator, test_views.test_views(bkgd=cfg["test_bkgd"]), **render)

    batch_extra = {} if refinement is None else dict(return_indices=True)
    refine = lambda data: {} if refinement is None else dict(refinement=refinement, view_indices=data["indices"][:, 0])
    num_rays = int(cfg["init_batch_size"])
    target = int(cfg["target_sample_batch_size"])
    history, evals = [], []
    eval_seconds = 0.0
    torch.cuda.synchronize(dev)
    tic = time.time()
    for step in range(steps + 1):
        field.train()
        estimator.train()
        if sampling_weights is None:
            data = train_views.batch(num_rays, step, bkgd=cfg["train_bkgd"], view_mode=cfg["view_mode"], seed=seed,
                                     **batch_extra)
        else:
            use_ist = ist_from_step is not None and step >= ist_from_step
            data = train_views.batch_importance(num_rays, step, ist_weights if use_ist else sampling_weights,
                                                weights_subsampled, bkgd=cfg["train_bkgd"], seed=seed, **batch_extra)
        rays, pixels, ts = data["rays"], data["pixels"], data["timestamps"]
        version = estimator.binaries._version
        refresh_occupancy(field, estimator, step, ts, cfg["render_step_size"])
        refreshed = estimator.binaries._version != version
        lr = optimizer.param_groups[0]["lr"]
        out = train_step(field, estimator, optimizer, rays.origins, rays.viewdirs, ts, pixels, cfg["render_step_size"],
                         near_plane=cfg["near_plane"], far_plane=cfg["far_plane"], cone_angle=cfg["cone_angle"],
                         alpha_thre=cfg["alpha_thre"], render_bkgd=data["color_bkgd"], grad_scaler=scaler,
                         rgb_loss="mse", skip_empty=True, **losses, **refine(data))
        skipped = bool(out.get("skipped", False))
        rec = dict(step=step, lr=lr, num_rays=num_rays, n_samples=out["n_samples"], loss=out["loss"],
                   scale=float(scaler.get_scale()), skipped=skipped, occ_refreshed=refreshed,
                   seconds=time.time() - tic - eval_seconds)
        if sampling_weights is not None:
            rec["sampling"] = "ist" if use_ist else "isg"
            rec["n_rays"] = int(data["pixels"].shape[0])      # num_rays // s^2 cells of s^2 rays
        history.append(rec)
        if not skipped:
            num_rays = next_num_rays(int(data["pixels"].shape[0]), out["n_samples"], target) if target > 0 else num_rays
            scheduler.step()
        if verbose and (step % log_every == 0 or step == steps):
            psnr = -10.0 * math.log10(out["loss"]) if out["loss"] > 0 else float("inf")
            print(f"elapsed_time={time.time() - tic - eval_seconds:.2f}s | step={step} | loss={out['loss']:.5f} | "
                  f"psnr={psnr:.2f} | n_rendering_samples={out['n_samples']:d} | num_rays={rec['num_rays']:d} | ",
                  flush=True)
        if eval_every and step > 0 and step % eval_every == 0 and step != steps:
            t0 = time.time()
            evals.append((step, evaluate()))
            eval_seconds += time.time() - t0
    torch.cuda.synchronize(dev)
    train_seconds = time.time() - tic - eval_seconds
    field.sync_half_table()
    if save_path:
        ckpt = {"radiance_field": inference.state_dict(), "occupancy_grid": estimator.state_dict()}
        if refinement is not None:
            ckpt["camera_refinement"] = refinement.state_dict()
        torch.save(ckpt, save_path)
    result = evaluate()
    if result is not None:
        evals.append((steps, result))
        if verbose:
            print(f"evaluation: psnr_avg={result['psnr_avg']}, ssim_avg={result['ssim_avg']}", flush=True)
    return dict(field=field, inference=inference, estimator=estimator, train_seconds=train_seconds, history=history,
                eval=result, evals=evals, config=cfg,
                refinement=None if refinement is None else refinement.state_dict())


def build_modules(cfg: Dict, device, *, use_div_offsets: bool = False, use_time_embedding: bool = False,
                  use_time_attenuation: bool = False, use_feat_predict: bool = False, use_weight_predict: bool = False,
                  hash_dtype: torch.dtype = torch.float16):
    """(DNGPradianceField, OccGridEstimator) as train_real.py:185-187, 253-265 constructs them for a resolved config:
    the modules a checkpoint of a run with these flags loads into (`checkpoint.load_checkpoint`)."""
    from .model import DNGPradianceField
    estimator = OccGridEstimator(cfg["aabb"], cfg["grid_resolution"], cfg["grid_levels"]).to(device)
    field = DNGPradianceField(aabb=estimator.aabbs[-1].clone(), dst_resolution=cfg["hash_dst_resolution"],
                              log2_hashmap_size=int(cfg["log2_hashmap_size"]), moving_step=cfg["moving_step"],
                              use_div_offsets=use_div_offsets, use_time_embedding=use_time_embedding,
                              use_time_attenuation=use_time_attenuation, use_feat_predict=use_feat_predict,
                              use_weight_predict=use_weight_predict, hash_dtype=hash_dtype).to(device)
    return field.eval(), estimator.eval()


def load_scene(data_root: str, scene: str, kind: str, split: str, factor: Optional[int] = None, device="cuda",
               read_image=None) -> TrainViews:
    """One split of a scene folder through the loader of its dataset kind (`scenes.preset_of`)."""
    if kind == "dnerf":
        return TrainViews.from_dnerf_folder(data_root, scene, split, device=device)
    extra = {} if factor is None else dict(factor=factor)
    if kind == "hypernerf":
        return TrainViews.from_hypernerf_folder(data_root, scene, split, device=device, read_image=read_image, **extra)
    if kind == "dynerf":
        return TrainViews.from_dynerf_folder(data_root, scene, split, device=device, read_image=read_image, **extra)
    raise ValueError(f"dataset kind {kind!r}: one of {sorted(PRESETS)}")


def dynerf_sampling(train: TrainViews, ist_from_step: Optional[int] = None, verbose: bool = True) -> Dict:
    """fit's importance-sampling arguments for DyNeRF views: the folder's `isg_weights.pt` / `ist_weights.pt` with the
    loader's `weights_subsampled` where they were shipped, otherwise `importance.isg_weights(views, n_cameras,
    gamma=2e-2)` / `importance.ist_weights(views, n_cameras)` computed on the device at the loaded resolution
    (weights_subsampled = 1).  The IST map is only needed with `ist_from_step`."""
    from . import importance
    if hasattr(train, "isg_weights"):
        out = dict(sampling_weights=train.isg_weights, weights_subsampled=train.weights_subsampled)
        source = f"isg_weights.pt ({train.isg_weights.numel()} cells, weights_subsampled={train.weights_subsampled})"
    else:
        out = dict(sampling_weights=importance.isg_weights(train, train.n_cameras, gamma=2e-2).reshape(-1),
                   weights_subsampled=1)
        source = f"computed on the device ({out['sampling_weights'].numel()} cells, gamma=2e-2, weights_subsampled=1)"
    if verbose:
        print(f"ISG sampling weights: {source}", flush=True)
    if ist_from_step is not None:
        if hasattr(train, "ist_weights") and hasattr(train, "isg_weights"):
            ist, source = train.ist_weights, "ist_weights.pt"
        elif hasattr(train, "isg_weights"):
            raise ValueError("the folder ships isg_weights.pt without ist_weights.pt: --ist_from_step needs both maps "
                             "at one resolution")
        else:
            ist, source = importance.ist_weights(train, train.n_cameras).reshape(-1), "computed on the device"
        out.update(ist_weights=ist, ist_from_step=int(ist_from_step))
        if verbose:
            print(f"IST sampling weights from step {ist_from_step}: {source}", flush=True)
    return out


def write_video_frames(out_dir: str, inference, estimator, cfg: Dict, test: TrainViews, kind: str,
                       n_frames: Optional[int] = None, flow: bool = False, flow_max: Optional[float] = None) -> int:
    """train_real.py:531-558 up to the encoder: renders DyNeRF's spiral path (`render_poses`) or, for the other two
    kinds, the test views' cameras at their times with `video.render_video` on black with 1024 samples per ray, and
    writes `rgb_%04d.png` / `depth_%04d.png` (8-bit normalised depth) into `out_dir`.  Returns the frame count.
    flow=True (pinhole paths only): also `flow_%04d.png`, the frame's optical flow into its own camera over one frame of
    the path -- dt = 1 / frames for the spiral, the mean spacing of the views' times otherwise -- as the expected flow of
    the visible surface (flow / coverage, nothing where coverage < 1e-3) on `ops.flow_to_rgb8`'s colour wheel, fully
    saturated at flow_max pixels (default: the largest magnitude of the frames written).  The frames are mirrored along
    the width like the rgb frames, and the flow's x component with them, so the hue is the direction seen in the PNG."""
    from . import cameras, ops
    from .video import render_video
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("--render_video writes PNGs with PIL (Pillow), which is not installed") from e
    dev = test.device
    if kind == "dynerf":
        total = len(test.render_poses)
        rays_of = lambda i: test.render_path_rays(i)[0]
        time_of = lambda i: torch.full((1, 1), float(i) / total, device=dev, dtype=torch.float32)
        projector_of = lambda i: cameras.pinhole_projector(test.K[0], test.render_poses[i], opengl=test.opengl, device=dev)
        dt = 1.0 / total
    else:
        total = len(test)
        rays_of = test.view_rays
        time_of = lambda i: test.timestamps[i].reshape(1, 1)
        projector_of = lambda i: cameras.pinhole_projector(test.K[i], test.c2w[i], opengl=test.opengl, device=dev)
        dt = float(test.timestamps.max() - test.timestamps.min()) / max(total - 1, 1) if flow else 0.0
    if flow and test.model != CAMERA_PINHOLE:
        raise ValueError("flow=True needs pinhole cameras (D-NeRF test views, the DyNeRF spiral): these views have "
                         "distorted HyperNeRF cameras, for which no projector is built")
    n = total if n_frames is None else max(0, min(int(n_frames), total))
    render = dict(near_plane=cfg["near_plane"], far_plane=cfg["far_plane"], render_step_size=cfg["render_step_size"],
                  cone_angle=cfg["cone_angle"], alpha_thre=cfg["alpha_thre"], render_bkgd=torch.zeros(3, device=dev))
    frames = render_video(inference, estimator, rays_of, time_of, n, max_samples=1024, render_kwargs=render,
                          to_host=True, optical_flow=(projector_of, dt) if flow else None)
    os.makedirs(out_dir, exist_ok=True)
    for i, frame in enumerate(frames):
        Image.fromarray(frame["rgb"]).save(os.path.join(out_dir, f"rgb_{i:04d}.png"))
        Image.fromarray(frame["depth"]).save(os.path.join(out_dir, f"depth_{i:04d}.png"))
    if flow and frames:
        seen = [frame["flow_coverage_f32"] >= 1e-3 for frame in frames]
        expected = [torch.where(s, frame["flow_f32"] / frame["flow_coverage_f32"].clamp_min(1e-3), torch.zeros((), device=dev))
                    .contiguous() for s, frame in zip(seen, frames)]
        if flow_max is None:
            flow_max = max(float(e.norm(dim=-1).max()) for e in expected)
        flow_max = flow_max if flow_max > 0 else 1.0
        mirror = torch.tensor([-1.0, 1.0], device=dev)                   # render_video's frames are flipped along the width
        for i, e in enumerate(expected):
            Image.fromarray(ops.flow_to_rgb8(e * mirror, flow_max).cpu().numpy()).save(os.path.join(out_dir, f"flow_{i:04d}.png"))
    return len(frames)


def build_parser() -> argparse.ArgumentParser:
    """The CLI's arguments (flag names of opt.py)."""
    p = argparse.ArgumentParser(description="Train a D-NeRF synthetic, HyperNeRF or DyNeRF scene (train_real.py's loop)")
    p.add_argument("--data_root", required=True)
    p.add_argument("--scene", required=True)
    p.add_argument("--dataset", default="auto", choices=["auto", "dnerf", "hypernerf", "dynerf"],
                   help="the folder's kind; auto looks the scene name up in the reference's scene tables")
    p.add_argument("--factor", type=int, default=None, help="image downscale (default 2 for HyperNeRF, 4 for DyNeRF)")
    p.add_argument("--train_split", default="train", choices=["train", "trainval"])
    p.add_argument("--test_split", default="test")
    p.add_argument("--max_steps", type=int, default=None)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--log2_hashmap_size", type=int, default=21)
    p.add_argument("--save_path", default=None)
    p.add_argument("--load_model", default=None, metavar="PATH", help="skip training and load this model.pth")
    p.add_argument("--assume_tcnn_layout", default=None, help="for a --load_model file written by the reference")
    p.add_argument("--render_video", default=None, metavar="DIR", help="write rgb_%%04d.png / depth_%%04d.png here")
    p.add_argument("--video_frames", type=int, default=None, help="render only the first N frames of the path")
    p.add_argument("--video_flow", action="store_true",
                   help="with --render_video: also write flow_%%04d.png, the optical flow over one frame of the path (pinhole cameras)")
    p.add_argument("--video_flow_max", type=float, default=None, metavar="PX",
                   help="flow magnitude in pixels at full saturation (default: the largest of the frames written)")
    p.add_argument("--time_bins", type=int, default=None, metavar="B",
                   help="with --render_video: render through B time slices of the occupancy grid (TimeSlicedOccGrid.from_field)")
    p.add_argument("--time_bin_samples", type=int, default=5, metavar="S", help="probe times per bin of --time_bins")
    p.add_argument("--ist_from_step", type=int, default=None, help="DyNeRF: sample by the IST map from this step on")
    p.add_argument("--refine_poses", action="store_true", help="learn a rotation and a shift per training view")
    p.add_argument("--refine_times", action="store_true", help="learn a time offset per training view")
    p.add_argument("--refine_lr", type=float, default=1e-3, help="learning rate of --refine_poses / --refine_times")
    p.add_argument("-df", "--use_div_offsets", action="store_true")
    p.add_argument("-f", "--use_feat_predict", action="store_true")
    p.add_argument("-w", "--use_weight_predict", action="store_true")
    p.add_argument("-te", "--use_time_embedding", action="store_true")
    p.add_argument("-ta", "--use_time_attenuation", action="store_true")
    p.add_argument("-ms", "--moving_step", type=float, default=None)
    p.add_argument("-o", "--use_opacity_loss", action="store_true")
    p.add_argument("-d", "--distortion_loss", action="store_true")
    p.add_argument("-wr", "--weight_rgbper", action="store_true")
    p.add_argument("-ae", "--acc_entorpy_loss", action="store_true")
    return p


def main(argv=None) -> int:
    """CLI over a D-NeRF synthetic, HyperNeRF or DyNeRF scene folder, with the flag names of opt.py."""
    from . import checkpoint, scenes
    p = build_parser()
    a = p.parse_args(argv)
    if a.dataset != "auto":
        kind = a.dataset
    else:
        try:
            kind = scenes.preset_of(a.scene)
        except ValueError:
            # a D-NeRF-layout folder under a name of its own trains as before
            if not os.path.exists(os.path.join(a.data_root, a.scene, f"transforms_{a.train_split}.json")):
                raise
            kind = "dnerf"
    if a.ist_from_step is not None and kind != "dynerf":
        p.error("--ist_from_step belongs to DyNeRF's importance sampling")
    train_split, test_split = (a.train_split, a.test_split) if kind == "dnerf" else ("train", "test")
    extra = {} if a.moving_step is None else dict(moving_step=a.moving_step)
    extra["log2_hashmap_size"] = a.log2_hashmap_size
    flags = dict(use_div_offsets=a.use_div_offsets, use_time_embedding=a.use_time_embedding,
                 use_time_attenuation=a.use_time_attenuation, use_feat_predict=a.use_feat_predict,
                 use_weight_predict=a.use_weight_predict)
    if a.video_flow and not a.render_video:
        p.error("--video_flow goes with --render_video DIR")
    if a.time_bins is not None:
        from . import ops
        if not a.render_video:
            p.error("--time_bins goes with --render_video DIR")
        if not (1 <= a.time_bins <= ops.TIME_MAX_BINS and 1 <= a.time_bin_samples <= ops.TIME_MAX_TIMES):
            p.error(f"--time_bins takes 1 .. {ops.TIME_MAX_BINS}, --time_bin_samples 1 .. {ops.TIME_MAX_TIMES}")
    test = load_scene(a.data_root, a.scene, kind, test_split, a.factor)
    if a.video_flow and test.model != CAMERA_PINHOLE:
        p.error("--video_flow needs pinhole cameras (D-NeRF test views, the DyNeRF spiral): these views have distorted "
                "HyperNeRF cameras, for which no projector is built")
    if a.load_model:                             # train_real.py:189-190, 524-529: no training set, no loop
        cfg = resolve_config(kind, a.max_steps, **extra)
        ckpt = checkpoint.read_checkpoint(a.load_model)
        state = ckpt["radiance_field"]
        dtype = torch.float16 if checkpoint.is_reference_state(state) else state["hash_table"].dtype
        inference, estimator = build_modules(cfg, test.device, hash_dtype=dtype, **flags)
        checkpoint.load_checkpoint(ckpt, inference, estimator, assume_tcnn_layout=a.assume_tcnn_layout)
        print(f"loaded {a.load_model}", flush=True)
    else:
        train = load_scene(a.data_root, a.scene, kind, train_split, a.factor)
        sampling = dynerf_sampling(train, a.ist_from_step) if kind == "dynerf" else {}
        log_every = 10000 if a.max_steps is None else max(1, min(10000, a.max_steps))
        res = fit(train, test, preset=kind, max_steps=a.max_steps, seed=a.seed, distortion_loss=a.distortion_loss,
                  acc_entropy_loss=a.acc_entorpy_loss, opacity_loss=a.use_opacity_loss, weight_rgbper=a.weight_rgbper,
                  log_every=log_every, save_path=a.save_path, refine_poses=a.refine_poses, refine_times=a.refine_times,
                  refine_lr=a.refine_lr, **flags, **sampling, **extra)
        inference, estimator, cfg = res["inference"], res["estimator"], res["config"]
    if a.render_video:
        grid = estimator.eval()
        if a.time_bins is not None:
            from .nerfacc_api import TimeSlicedOccGrid
            grid = TimeSlicedOccGrid.from_field(inference.eval(), grid, n_bins=a.time_bins, times_per_bin=a.time_bin_samples,
                                                render_step_size=cfg["render_step_size"])
            shares = ", ".join(f"{100.0 * v:.1f}" for v in grid.occupied_fraction().tolist())
            print(f"{a.time_bins} time slices of the occupancy grid; occupied share of the union per bin (%): {shares}", flush=True)
        n = write_video_frames(a.render_video, inference.eval(), grid, cfg, test, kind, a.video_frames,
                               flow=a.video_flow, flow_max=a.video_flow_max)
        print(f"wrote {n} rgb and depth{' and flow' if a.video_flow else ''} frames to {a.render_video}", flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
