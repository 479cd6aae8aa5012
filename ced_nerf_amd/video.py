"""The video step: render a camera path frame by frame and hand back the 8-bit frames
the reference writes to `rgb_render.mp4` / `depth_render.mp4` (train_real.py:531-558; the viewer's `render_frame`,
gui.py:205-237, is the same call for one frame).

The reference renders the frames one after another and converts each on the host.  Here the frames of the path are a
stream through `dist.PipelinedRenderer` (several frames in flight on one GPU, each a complete `render_image_test`
call, so every frame's pixels are those of rendering it alone), rays are generated on the device from the camera
(`cameras.pinhole_rays`) or supplied, and the float images are turned into uint8 on the device
(`ops.frame_to_rgb8`, `ops.depth_to_u8`).  Encoding to mp4 (imageio) and cv2's TURBO colour map for the depth video
are host-side table/codec work and are left to the caller: `depth` frames are the normalised 8-bit depths that
`cv2.applyColorMap` takes as input.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from . import ops
from .dist import PipelinedRenderer, ShardedRenderer
from .nerfacc_api import TimeSlicedOccGrid
from .utils import Rays, render_motion, render_normals, render_optical_flow, render_scene_flow, render_surface


def frame_to_uint8(rgb: torch.Tensor, depth: torch.Tensor, flip_w: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """(rgb [H,W,3] f32, depth [H,W,1] f32) -> (uint8 [H,W,3], uint8 [H,W]) as train_real.py:556-557 builds them."""
    return ops.frame_to_rgb8(rgb.contiguous(), flip_w), ops.depth_to_u8(depth.contiguous(), flip_w)


@torch.no_grad()
def render_video(radiance_field, estimator, rays_of_frame: Callable[[int], Rays], timestamps_of_frame: Callable[[int], torch.Tensor],
                 n_frames: int, max_samples: int = 1024, render_kwargs: Optional[Dict] = None, frames_in_flight: int = 3,
                 flip_w: bool = True, to_host: bool = False, keep_float: bool = False, frames_per_call: int = 1,
                 motion: bool = False, normals: bool = False, scene_flow: bool = False,
                 optical_flow: Optional[Tuple[Callable[[int], Callable], float]] = None,
                 surface: Optional[Dict] = None) -> List[Dict]:
    """Render frames 0..n_frames-1 of a path.

    rays_of_frame(i) -> Rays with [H,W,3] device tensors (e.g. `cameras.pinhole_rays(K, c2w_i, W, H)`; it is called on
    the rendering thread of the frame's lane with that lane's stream current, so device ray generation overlaps the
    other frames); timestamps_of_frame(i) -> the frame's [1,1] time.  Returns one dict per frame: `rgb` uint8 [H,W,3],
    `depth` uint8 [H,W] (torch tensors on the device, or numpy arrays with to_host=True), `n_samples`; with
    keep_float=True also the float images `rgb_f32`, `opacity_f32`, `depth_f32`.
    frames_per_call > 1 (up to 8): that many consecutive frames go through one native call (ced_render_frames_test:
    shared launches, each frame on its own schedule -- same pixels, larger launches); `n_samples` is then reported
    per call on its first frame's entry and the others carry None.
    motion=True: every frame's dict also carries `motion_f32` [H,W,3], the deformation field's motion map
    (`utils.render_motion`) rendered after the frame on the frame's rays and time with the march options of
    render_kwargs; the frames themselves are rendered exactly as without it.
    normals=True: likewise `normals_f32` [H,W,3], the frame's normal map (`utils.render_normals`).
    scene_flow=True: likewise `scene_flow_f32` [H,W,3] (`utils.render_scene_flow`'s flow3d).
    optical_flow=(projector_of_frame, dt): likewise `flow_f32` [H,W,2] and `flow_coverage_f32` [H,W,1],
    `utils.render_optical_flow` with project = projector_of_frame(i) (e.g. `cameras.pinhole_projector(K, c2w_i)`) and the
    time step dt; the expected flow of the visible surface, in pixels per dt, is flow_f32 / flow_coverage_f32.
    surface=dict(sigma_thresh=...[, max_iters=, tol=]): likewise `surface_depth_f32` [H,W,1], `surface_normals_f32` [H,W,3]
    and `surface_hit` [H,W,1] bool: the first point of every ray at which the density reaches sigma_thresh
    (`utils.render_surface`'s depth, normal and hit), not a weighted mean over the ray's samples.
    estimator may be a `TimeSlicedOccGrid`: every native call then marches through `estimator.at_time(the times of its
    frames)` -- the frames' times are read to the host once, before the pipeline starts -- and the post passes resolve
    their grid per frame (`utils.grid_for`)."""
    if n_frames <= 0:
        return []
    device = radiance_field.aabb.device if hasattr(radiance_field, "aabb") else torch.device("cuda")
    per_call = max(1, min(8, int(frames_per_call)))
    n_calls = (n_frames + per_call - 1) // per_call
    n_lanes = max(1, min(int(frames_in_flight), n_calls))
    lanes = [ShardedRenderer(radiance_field, estimator, 1, 0, device, max_samples=max_samples,
                             render_kwargs=render_kwargs, tile_order=True, units=per_call) for _ in range(n_lanes)]
    pipe = PipelinedRenderer(lanes)
    n_steps = (n_calls + n_lanes - 1) // n_lanes
    # frames of the call (lane, step); the tail of the path repeats the last frame
    frames_of = lambda lane, step: [min((step * n_lanes + lane) * per_call + k, n_frames - 1) for k in range(per_call)]

    # a sliced grid: one host read of all the frames' times, and every call's grid (with its distance field) built and
    # finished here, on this thread, before the pipeline's lane threads start
    grids = None
    if isinstance(estimator, TimeSlicedOccGrid):
        host_times = torch.cat([timestamps_of_frame(i).reshape(-1)[:1] for i in range(n_frames)]).tolist()
        grids = {}
        for step in range(n_steps):
            for lane in range(n_lanes):
                grids[lane, step] = estimator.at_time([host_times[i] for i in frames_of(lane, step)])
                grids[lane, step].occupancy_accel()
        torch.cuda.synchronize(device)

    def before_frame(lane, step):
        if grids is not None:
            lanes[lane].estimator = grids[lane, step]
        rs = [rays_of_frame(i) for i in frames_of(lane, step)]
        lanes[lane].set_rays(torch.stack([r.origins for r in rs]), torch.stack([r.viewdirs for r in rs]))

    def times(lane, step):
        return torch.cat([timestamps_of_frame(i).reshape(-1)[:1] for i in frames_of(lane, step)])

    steps = pipe.render_steps(times, n_steps, before_frame)
    frames = []
    for step, row in enumerate(steps):
        for lane, out in enumerate(row):
            for k in range(per_call):
                i = (step * n_lanes + lane) * per_call + k
                if i >= n_frames:
                    break
                rgb, depth = out["rgb"][k], out["depth"][k]
                rgb8, d8 = frame_to_uint8(rgb, depth, flip_w)
                f = {"rgb": rgb8.cpu().numpy() if to_host else rgb8, "depth": d8.cpu().numpy() if to_host else d8,
                     "n_samples": int(out["total_samples"]) if (per_call == 1 or k == 0) else None}
                if keep_float:
                    f.update(rgb_f32=rgb, opacity_f32=out["opacity"][k], depth_f32=depth)
                frames.append(f)
    kw = {k: v for k, v in (render_kwargs or {}).items()
          if k in ("near_plane", "far_plane", "render_step_size", "cone_angle", "alpha_thre")}
    for key, on, render in (("motion_f32", motion, render_motion), ("normals_f32", normals, render_normals),
                            ("scene_flow_f32", scene_flow, render_scene_flow)):
        if not on:
            continue
        for i, f in enumerate(frames):
            f[key] = render(radiance_field, estimator, rays_of_frame(i), timestamps=timestamps_of_frame(i), **kw)[0]
    if optical_flow is not None:
        projector_of_frame, dt = optical_flow
        for i, f in enumerate(frames):
            flow, _, coverage, _ = render_optical_flow(radiance_field, estimator, rays_of_frame(i), projector_of_frame(i), dt,
                                                       timestamps=timestamps_of_frame(i), **kw)
            f.update(flow_f32=flow, flow_coverage_f32=coverage)
    if surface is not None:
        unknown = set(surface) - {"sigma_thresh", "max_iters", "tol"}
        if unknown:
            raise ValueError(f"surface= takes sigma_thresh, max_iters and tol, got {sorted(unknown)}")
        skw = {k: v for k, v in kw.items() if k != "alpha_thre"}
        for i, f in enumerate(frames):
            s = render_surface(radiance_field, estimator, rays_of_frame(i), timestamps=timestamps_of_frame(i), colors=False,
                               **skw, **surface)
            f.update(surface_depth_f32=s["depth"], surface_normals_f32=s["normal"], surface_hit=s["hit"])
    return frames
