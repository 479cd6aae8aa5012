"""Render drivers: host mirror of cednerf/utils.py (render_image :46-150, render_image_test :153-318).

Same signatures and return tuples as the reference; the per-sample work (positions, field,
weights, per-ray accumulation) runs in the HIP kernels through `ced_nerf_amd.ops`.
"""
from __future__ import annotations

import collections
import random
from typing import Optional

import numpy as np
import torch

from . import ops
from .nerfacc_api import (OccGridEstimator, TimeSlicedOccGrid, _packed_info_from, accumulate_along_rays, march_packed, ray_aabb_intersect,
                          render_weight_from_density, sort_intersections)
from .render import rendering

# datasets/utils.py:8,13-15
Rays = collections.namedtuple("Rays", ("origins", "viewdirs"))


def namedtuple_map(fn, tup):
    """Apply `fn` to each element of `tup` and cast to `tup`'s namedtuple."""
    return type(tup)(*(None if x is None else fn(x) for x in tup))


def set_random_seed(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


class _TruncExp(torch.autograd.Function):
    """cednerf/utils.py:27-43: exp in float32; the backward multiplies by exp(clamp(x, max=15)) so that large
    pre-activations give finite gradients."""

    @staticmethod
    def forward(ctx, x):
        x = x.float()
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.exp(torch.clamp(x, max=15))


trunc_exp = _TruncExp.apply


_EVAL_PASS_RAYS = 1 << 21     # rays per internal eval pass of render_image


def grid_for(estimator, timestamps):
    """The occupancy grid a render at `timestamps` marches through: `estimator.at_time(timestamps)` for a TimeSlicedOccGrid
    (the OR of the bins that cover the range of the times; one host read for a device tensor), the estimator itself --
    the same object, nothing read -- for anything else.  Every renderer calls it first thing."""
    if isinstance(estimator, TimeSlicedOccGrid) and timestamps is not None:
        return estimator.at_time(timestamps)
    return estimator


def _flatten_rays(rays: Rays):
    rays_shape = rays.origins.shape
    if len(rays_shape) == 3:
        height, width, _ = rays_shape
        num_rays = height * width
        rays = namedtuple_map(lambda r: r.reshape([num_rays] + list(r.shape[2:])), rays)
    else:
        num_rays, _ = rays_shape
    return rays, rays_shape, num_rays


@torch.no_grad()
def render_image(
    radiance_field: torch.nn.Module,
    estimator: OccGridEstimator,
    rays: Rays,
    near_plane: float = 0.0,
    far_plane: float = 1e10,
    render_step_size: float = 1e-3,
    render_bkgd: Optional[torch.Tensor] = None,
    cone_angle: float = 0.0,
    alpha_thre: float = 0.0,
    test_chunk_size: int = 8192,
    timestamps: Optional[torch.Tensor] = None,
    native: Optional[bool] = None,
):
    """Render the pixels of an image (cednerf/utils.py:46-150).
    Returns (colors, opacities, depths, n_rendering_samples, extras[list per chunk]).
    In eval mode with the HIP field the pass runs on ced_render_image: the visibility filter of `sampling` and
    `rendering` from ONE field evaluation per sample, rays stopped where their transmittance falls below the filter's
    threshold -- the same arrays bit for bit (tests/test_gpu_parity.py).  native=False forces the staged composition
    (sampling with sigma_fn, then rendering) that training mode always uses."""
    estimator = grid_for(estimator, timestamps)
    if timestamps is None:
        raise NotImplementedError("DNGPradianceField needs timestamps (dnerf path of cednerf/utils.py:78-86)")
    rays, rays_shape, num_rays = _flatten_rays(rays)
    results, extra_info = [], []
    if native is None:
        native = (not radiance_field.training) and hasattr(radiance_field, "_descriptor") and rays.origins.is_cuda
    if native:
        assert not radiance_field.training, "the native render_image pass is the eval path"
    # The reference renders 8192 rays per pass in eval mode to bound memory (cednerf/utils.py:59,108-112).
    # Rays are independent, so here a pass covers up to `_EVAL_PASS_RAYS` rays (HBM is not the
    # constraint on MI355X) and its outputs are then cut into the reference's `test_chunk_size`
    # pieces, so the returned `extras` list and every value in it are those of the chunked loop.
    training = bool(radiance_field.training)
    if training:
        pass_rays = torch.iinfo(torch.int32).max
    else:
        pass_rays = max(test_chunk_size, (_EVAL_PASS_RAYS // test_chunk_size) * test_chunk_size)
    for i in range(0, num_rays, pass_rays):
        chunk_rays = namedtuple_map(lambda r: r[i:i + pass_rays].contiguous().float(), rays)
        ts = timestamps[i:i + pass_rays] if training else timestamps
        n_pass = chunk_rays.origins.shape[0]
        two_pass = native and float(alpha_thre) > 0.0
        if native and not two_pass:
            bk = None if render_bkgd is None else render_bkgd.to(chunk_rays.origins.device, torch.float32).reshape(-1).contiguous()
            chunked = n_pass > test_chunk_size
            tq = ts.reshape(-1).float().contiguous()

            def run(t_all0, t_all1, packed_all):
                return ops.render_image_eval_native(radiance_field._descriptor(), chunk_rays.origins, chunk_rays.viewdirs,
                                                    packed_all, t_all0, t_all1, 1e-4, 0.0, tq, False, bk,
                                                    chunk_rays=test_chunk_size if chunked else 0)

            # The march of every ray to the far plane needs the sample total before it can store (count pass, scan, fill
            # pass).  Consecutive frames of a video march about the same number of samples, so once a pass of this size
            # has been rendered the march runs in ONE pass into arrays 25 % larger than the last total; should a frame
            # not fit (the device-side total says so after the render) it is redone with the exact two-pass march.
            hints = estimator.__dict__.setdefault("_march_totals", {})
            hint = hints.get(n_pass)
            out = None
            if hint is not None and estimator.one_pass_march:
                cap = int(hint * 1.25) + 65536
                t_all0, t_all1, packed_all, total_dev = estimator.march_onepass(
                    chunk_rays.origins, chunk_rays.viewdirs, near_plane, far_plane, render_step_size, cone_angle, cap)
                out = run(t_all0, t_all1, packed_all)
                total = int(total_dev.item())
                hints[n_pass] = total
                if total > cap:
                    out = None
            if out is None:
                t_all0, t_all1, _, packed_all = estimator.march(
                    chunk_rays.origins, chunk_rays.viewdirs, near_plane=near_plane, far_plane=far_plane,
                    render_step_size=render_step_size, stratified=False, cone_angle=cone_angle, want_ray_indices=False)
                hints[n_pass] = int(t_all0.shape[0])
                out = run(t_all0, t_all1, packed_all)
            rgb, opacity, depth, ex, offsets, _ = out
            extras = {k: ex[k] for k in ("weights", "alphas", "trans", "sigmas", "rgbs", "ray_indices", "t_starts", "t_ends")}
            # a pass's pixels stay whole (cutting them into chunks only to concatenate them again would be ~250 slice
            # calls); the per-chunk `extras` are views cut by one split() per array
            results.append([rgb, opacity, depth, int(extras["t_starts"].shape[0])])
            if not chunked:
                extra_info.append(extras)
                continue
            starts = list(range(0, n_pass, test_chunk_size)) + [n_pass]
            bounds = offsets[torch.tensor(starts, device=offsets.device)].tolist()
            sizes = [bounds[c + 1] - bounds[c] for c in range(len(starts) - 1)]
            cut = {k: v.split(sizes) for k, v in extras.items()}
            extra_info.extend([{k: cut[k][c] for k in cut} for c in range(len(sizes))])
            continue

        def sigma_fn(t_starts, t_ends, ray_indices):
            return radiance_field.query_rays(chunk_rays.origins, chunk_rays.viewdirs, ray_indices, t_starts, t_ends,
                                             ts, want_rgb=False)[1]

        def rgb_sigma_fn(t_starts, t_ends, ray_indices):
            return radiance_field.query_rays(chunk_rays.origins, chunk_rays.viewdirs, ray_indices, t_starts, t_ends,
                                             ts, want_rgb=True)

        # With an alpha threshold most marched samples may be dropped without ending their ray (C3, C4): the native pass
        # is then the filter alone on the density-only kernel (front to back, rays stopped at the transmittance test)
        # and the whole field only on the survivors -- `sampling` and `rendering` as the reference stages them.
        ray_indices, t_starts, t_ends = estimator.sampling(
            chunk_rays.origins, chunk_rays.viewdirs, sigma_fn=sigma_fn, near_plane=near_plane, far_plane=far_plane,
            render_step_size=render_step_size, stratified=training, cone_angle=cone_angle, alpha_thre=alpha_thre,
            sigma_field=(radiance_field, ts, training) if two_pass else None)
        rgb, opacity, depth, extras = rendering(t_starts, t_ends, ray_indices, n_rays=n_pass,
                                                rgb_sigma_fn=rgb_sigma_fn, render_bkgd=render_bkgd)
        extras["ray_indices"] = ray_indices
        extras["t_starts"] = t_starts
        extras["t_ends"] = t_ends
        if training or n_pass <= test_chunk_size:
            results.append([rgb, opacity, depth, len(t_starts)])
            extra_info.append(extras)
            continue
        # cut the pass into the reference's chunks: samples are sorted by ray, so each chunk owns a
        # contiguous sample range (one small device->host copy of the range boundaries)
        starts = list(range(0, n_pass, test_chunk_size)) + [n_pass]
        bounds = torch.searchsorted(ray_indices, torch.tensor(starts, device=rgb.device)).tolist()
        sizes = [bounds[c + 1] - bounds[c] for c in range(len(starts) - 1)]
        extras["ray_indices"] = ray_indices % test_chunk_size         # relative to the ray's chunk
        cut = {k: v.split(sizes) for k, v in extras.items()}
        results.append([rgb, opacity, depth, len(t_starts)])          # the pixels of a pass stay whole
        extra_info.extend([{k: cut[k][c] for k in cut} for c in range(len(sizes))])
    colors, opacities, depths, n_rendering_samples = [
        torch.cat(r, dim=0) if isinstance(r[0], torch.Tensor) else r for r in zip(*results)
    ]
    return (colors.view((*rays_shape[:-1], -1)), opacities.view((*rays_shape[:-1], -1)),
            depths.view((*rays_shape[:-1], -1)), sum(n_rendering_samples), extra_info)


def _check_eval_frame(radiance_field, timestamps, who):
    if timestamps is None:
        raise NotImplementedError("DNGPradianceField needs timestamps (dnerf path of cednerf/utils.py:78-86)")
    if radiance_field.training:
        raise NotImplementedError(f"{who} renders eval frames (one time per frame)")


def _render_sample_values(radiance_field, estimator, rays, near_plane, far_plane, render_step_size, cone_angle, alpha_thre,
                          test_chunk_size, timestamps, return_samples, who, key, values_fn):
    """What `render_motion`, `render_normals` and the flow maps share: per-sample quantities composited with the
    volume-rendering weights on exactly the samples `render_image` takes in eval mode.
    values_fn(o, d, ray_indices, t_starts, t_ends, ts) -> [S,C], named `key` in the per-chunk sample dicts; or, with `key` a
    tuple of names, a dict of per-sample tensors that holds at least those names: each named one ([S,C] float, or [S] bool
    taken as 0 / 1) becomes an image, in that order, and every entry of the dict goes into the sample dicts.
    Returns (image [H,W,C] per name, opacity [H,W,1], n_samples[, samples])."""
    estimator = grid_for(estimator, timestamps)
    _check_eval_frame(radiance_field, timestamps, who)
    rays, rays_shape, num_rays = _flatten_rays(rays)
    ts = timestamps
    pass_rays = max(test_chunk_size, (_EVAL_PASS_RAYS // test_chunk_size) * test_chunk_size)
    keys = (key,) if isinstance(key, str) else tuple(key)
    images, opacities, samples, n_samples = [[] for _ in keys], [], [], 0
    for i in range(0, num_rays, pass_rays):
        chunk_rays = namedtuple_map(lambda r: r[i:i + pass_rays].contiguous().float(), rays)
        o, d = chunk_rays.origins, chunk_rays.viewdirs
        n_pass = o.shape[0]

        def sigma_fn(t_starts, t_ends, ray_indices):
            return radiance_field.query_rays(o, d, ray_indices, t_starts, t_ends, ts, want_rgb=False)[1]

        ray_indices, t_starts, t_ends = estimator.sampling(
            o, d, sigma_fn=sigma_fn, near_plane=near_plane, far_plane=far_plane, render_step_size=render_step_size,
            stratified=False, cone_angle=cone_angle, alpha_thre=alpha_thre, sigma_field=(radiance_field, ts, False))
        values = values_fn(o, d, ray_indices, t_starts, t_ends, ts)
        if isinstance(key, str):
            values = {key: values}
        sigmas = sigma_fn(t_starts, t_ends, ray_indices)
        packed = _packed_info_from(ray_indices, n_pass)
        weights, _, _ = render_weight_from_density(t_starts, t_ends, sigmas, packed_info=packed)
        for k, out in zip(keys, images):
            v = values[k]
            out.append(accumulate_along_rays(weights, values=v if v.dim() == 2 else v.float()[:, None], packed_info=packed))
        opacities.append(accumulate_along_rays(weights, values=None, packed_info=packed))
        n_samples += int(t_starts.shape[0])
        if not return_samples:
            continue
        extras = {"ray_indices": ray_indices, "t_starts": t_starts, "t_ends": t_ends, "weights": weights, **values}
        if n_pass <= test_chunk_size:
            samples.append(extras)
            continue
        # the reference's chunks, as render_image cuts them: samples are sorted by ray
        starts = list(range(0, n_pass, test_chunk_size)) + [n_pass]
        bounds = packed[:, 0][torch.tensor(starts[:-1], device=o.device)].tolist() + [int(t_starts.shape[0])]
        sizes = [bounds[c + 1] - bounds[c] for c in range(len(starts) - 1)]
        extras["ray_indices"] = ray_indices % test_chunk_size
        cut = {k: v.split(sizes) for k, v in extras.items()}
        samples.extend([{k: cut[k][c] for k in cut} for c in range(len(sizes))])
    out = [torch.cat(parts, dim=0) for parts in images]
    out = [im.view((*rays_shape[:-1], im.shape[-1])) for im in out]
    opacity = torch.cat(opacities, dim=0).view((*rays_shape[:-1], 1))
    if return_samples:
        return (*out, opacity, n_samples, samples)
    return (*out, opacity, n_samples)


@torch.no_grad()
def render_motion(
    radiance_field: torch.nn.Module,
    estimator: OccGridEstimator,
    rays: Rays,
    near_plane: float = 0.0,
    far_plane: float = 1e10,
    render_step_size: float = 1e-3,
    cone_angle: float = 0.0,
    alpha_thre: float = 0.0,
    test_chunk_size: int = 8192,
    timestamps: Optional[torch.Tensor] = None,
    return_samples: bool = False,
):
    """Per-pixel motion map of the deformation field: the motion network's move vectors (`query_move`) composited with
    the volume-rendering weights, on exactly the samples `render_image` takes in eval mode for the same arguments
    (`estimator.sampling` with the field's density, stratified=False, the same passes and chunks).
    Returns (motion [H,W,3], opacity [H,W,1], n_samples): motion = sum_i w_i * move_i along each ray, NOT normalised --
    the expected displacement of the visible surface is motion / opacity (where opacity > 0); opacity is
    `render_image`'s.  Rays that meet no sample have motion = 0 and opacity = 0.  With return_samples=True a fourth
    value is the list of per-chunk dicts `ray_indices` (relative to the chunk when the frame has several), `t_starts`,
    `t_ends`, `weights`, `move`.  rays: [H,W,3] or flat [N,3], as `render_image`."""
    def move_fn(o, d, ray_indices, t_starts, t_ends, ts):
        return radiance_field.query_move_rays(o, d, ray_indices, t_starts, t_ends, ts)[0]

    return _render_sample_values(radiance_field, estimator, rays, near_plane, far_plane, render_step_size, cone_angle,
                                 alpha_thre, test_chunk_size, timestamps, return_samples, "render_motion", "move", move_fn)


@torch.no_grad()
def render_normals(
    radiance_field: torch.nn.Module,
    estimator: OccGridEstimator,
    rays: Rays,
    near_plane: float = 0.0,
    far_plane: float = 1e10,
    render_step_size: float = 1e-3,
    cone_angle: float = 0.0,
    alpha_thre: float = 0.0,
    test_chunk_size: int = 8192,
    timestamps: Optional[torch.Tensor] = None,
    return_samples: bool = False,
):
    """Per-pixel normal map: the field's normals at the samples (`query_normals`: the unit vector towards lower density
    from the density's analytic gradient with respect to the observed point, 0 outside the box) composited with the
    volume-rendering weights, on exactly `render_motion`'s samples for the same arguments.
    Returns (normals [H,W,3], opacity [H,W,1], n_samples): normals = sum_i w_i * n_i along each ray, NOT normalised -- its
    length is at most the opacity, and the surface normal is normals / |normals| where that is > 0.  Rays that meet no
    sample have normals = 0 and opacity = 0.  With return_samples=True a fourth value is the list of per-chunk dicts, as
    `render_motion`'s with `normal` in place of `move`."""
    def normal_fn(o, d, ray_indices, t_starts, t_ends, ts):
        dlog = radiance_field.query_density_gradient_rays(o, d, ray_indices, t_starts, t_ends, ts,
                                                          want=(False, False, True, False))[2]
        return ops.unit_or_zero(-dlog)

    return _render_sample_values(radiance_field, estimator, rays, near_plane, far_plane, render_step_size, cone_angle,
                                 alpha_thre, test_chunk_size, timestamps, return_samples, "render_normals", "normal", normal_fn)


@torch.no_grad()
def render_surface(
    radiance_field: torch.nn.Module,
    estimator: OccGridEstimator,
    rays: Rays,
    sigma_thresh: float = 1.0,
    near_plane: float = 0.0,
    far_plane: float = 1e10,
    render_step_size: float = 1e-3,
    cone_angle: float = 0.0,
    test_chunk_size: int = 8192,
    timestamps: Optional[torch.Tensor] = None,
    max_iters: int = 32,
    tol: float = 0.0,
    render_bkgd: Optional[torch.Tensor] = None,
    normals: bool = True,
    colors: bool = True,
):
    """The visible surface as a level set of the density: per ray the FIRST point at which the density reaches
    sigma_thresh, located to float32 resolution -- where `render_image`'s depth is a weighted mean that floats in front of
    or behind the surface wherever the density is soft.  Eval frames only (one time per frame).  Per pass of rays:
    every sample of the grid is marched to the far plane (`estimator.march`, no visibility filter), the density is taken
    at every sample (`query_rays`), ced_surface_first_crossing finds each ray's first sample at or above the threshold
    and the bracket before it, and ced_field_level_set bisects the density on that bracket (`query_level_set` states the
    verdicts), all rows of the pass in one launch.
    "First" means first at the marching step: structure thinner than render_step_size that lies between two samples'
    midpoints can be missed, exactly as `render_image` can miss it, and the bracket then closes on a later crossing.
    Returns a dict shaped like `rays` ([H,W,.] or flat [N,.]):
        hit [..,1] bool       status 0 or 1: a crossing, or a first sample that already lies at or above the threshold
        depth [..,1]          the distance t along the ray; 0 on misses
        position [..,3]       origin + direction * depth in float32 (a multiply, then an add); 0 on misses
        normal [..,3]         `query_normals`(position, t)[0]; 0 on misses, and without normals=True
        rgb [..,3]            the field's colour at `position` seen along the ray's direction; on misses render_bkgd if
                              given, else 0; 0 without colors=True
        sigma, width [..,1]   the density at `position` and the width of the final bracket (the bisection's, also for
                              status 2; 0 for status -1)
        status [..,1] int32   0 / 1 / 2 as `query_level_set`; -1: no sample of the ray reaches the threshold.  Status 2 (the
                              density at the candidate's midpoint, re-evaluated, is below the threshold) counts as a miss
        sample [..,1] int64   the index, within the ray's marched samples, of the candidate sample; -1 if none
        n_samples, n_evals    Python ints: samples marched, density evaluations of the bisection."""
    estimator = grid_for(estimator, timestamps)
    _check_eval_frame(radiance_field, timestamps, "render_surface")
    thresh, max_iters, tol = ops.check_level_set(sigma_thresh, max_iters, tol)
    rays, rays_shape, num_rays = _flatten_rays(rays)
    dev = rays.origins.device
    ts = timestamps.reshape(-1).float().contiguous()[:1]
    pass_rays = max(test_chunk_size, (_EVAL_PASS_RAYS // test_chunk_size) * test_chunk_size)
    bk = None if render_bkgd is None else render_bkgd.to(dev, torch.float32).reshape(-1)
    out = {k: torch.zeros((num_rays, c), device=dev, dtype=dt) for k, c, dt in (
        ("depth", 1, torch.float32), ("position", 3, torch.float32), ("normal", 3, torch.float32), ("rgb", 3, torch.float32),
        ("sigma", 1, torch.float32), ("width", 1, torch.float32))}
    out["status"] = torch.full((num_rays, 1), -1, device=dev, dtype=torch.int32)
    out["sample"] = torch.full((num_rays, 1), -1, device=dev, dtype=torch.int64)
    n_samples = n_evals = 0
    for i in range(0, num_rays, pass_rays):
        o = rays.origins[i:i + pass_rays].contiguous().float()
        d = rays.viewdirs[i:i + pass_rays].contiguous().float()
        t_starts, t_ends, ray_indices, packed = estimator.march(
            o, d, near_plane=near_plane, far_plane=far_plane, render_step_size=render_step_size, stratified=False,
            cone_angle=cone_angle)
        n_samples += int(t_starts.shape[0])
        if t_starts.shape[0] == 0:
            continue
        sigmas = radiance_field.query_rays(o, d, ray_indices, t_starts, t_ends, ts, want_rgb=False)[1]
        k, lo, hi = ops.surface_first_crossing(packed, t_starts, t_ends, sigmas.reshape(-1), thresh)
        cand = torch.nonzero(k >= 0).squeeze(1)
        if cand.numel() == 0:
            continue
        oc, dc = o[cand].contiguous(), d[cand].contiguous()
        t, x, sg, width, status, evals = ops.field_level_set(radiance_field._descriptor(), oc, dc, lo[cand].contiguous(),
                                                             hi[cand].contiguous(), ts, thresh, max_iters, tol)
        n_evals += int(evals.sum().item())
        rows = cand + i
        ok = status < 2
        out["status"][rows, 0] = status
        out["sample"][rows, 0] = k[cand] - packed[cand, 0]
        out["sigma"][rows, 0] = sg
        out["width"][rows, 0] = width
        out["depth"][rows, 0] = torch.where(ok, t, torch.zeros_like(t))
        out["position"][rows] = torch.where(ok[:, None], x, torch.zeros_like(x))
        hit_rows, xh = rows[ok], x[ok].contiguous()
        if hit_rows.numel() and (normals or colors):
            th = ts.expand(xh.shape[0]).contiguous()
            if normals:
                out["normal"][hit_rows] = radiance_field.query_normals(xh, th)[0]
            if colors:
                out["rgb"][hit_rows] = radiance_field(xh, th, dc[ok].contiguous())[0]
    hit = (out["status"] == 0) | (out["status"] == 1)
    if bk is not None:
        out["rgb"] = torch.where(hit, out["rgb"], bk.expand(num_rays, 3))
    out["hit"] = hit
    res = {k: v.view((*rays_shape[:-1], v.shape[-1])) for k, v in out.items()}
    res["n_samples"], res["n_evals"] = n_samples, n_evals
    return res


@torch.no_grad()
def render_scene_flow(
    radiance_field: torch.nn.Module,
    estimator: OccGridEstimator,
    rays: Rays,
    near_plane: float = 0.0,
    far_plane: float = 1e10,
    render_step_size: float = 1e-3,
    cone_angle: float = 0.0,
    alpha_thre: float = 0.0,
    test_chunk_size: int = 8192,
    timestamps: Optional[torch.Tensor] = None,
    return_samples: bool = False,
):
    """Per-pixel scene flow: the velocity of the material point at every sample (`query_scene_flow`: v = -(I + J_x)^-1
    d move / dt from one fused launch, 0 and flagged where the warp folds) composited with the volume-rendering weights,
    on exactly `render_motion`'s samples for the same arguments.
    Returns (flow3d [H,W,3], opacity [H,W,1], coverage [H,W,1], n_samples): flow3d = sum_i w_i * v_i in world units per
    unit of time, coverage = sum_i w_i * valid_i <= opacity, neither normalised -- the expected velocity of the visible
    surface is flow3d / coverage (where coverage > 0).  Rays that meet no sample have zeros.  With return_samples=True a
    fifth value is the list of per-chunk dicts, as `render_motion`'s with `velocity` [S,3], `det` [S] and `valid` [S] bool
    in place of `move`."""
    _check_eval_frame(radiance_field, timestamps, "render_scene_flow")
    if not rays.origins.is_cuda:
        raise NotImplementedError("Only support cuda inputs: render_scene_flow runs on the HIP kernels (no CPU fallback).")

    def flow_fn(o, d, ray_indices, t_starts, t_ends, ts):
        v, det, valid = radiance_field.query_scene_flow_rays(o, d, ray_indices, t_starts, t_ends, ts)
        return {"velocity": v, "det": det, "valid": valid}

    flow3d, coverage, opacity, *rest = _render_sample_values(
        radiance_field, estimator, rays, near_plane, far_plane, render_step_size, cone_angle, alpha_thre, test_chunk_size,
        timestamps, return_samples, "render_scene_flow", ("velocity", "valid"), flow_fn)
    return (flow3d, opacity, coverage, *rest)


def sample_positions(o, d, ray_indices, t_starts, t_ends):
    """The sample positions the field kernels evaluate, in their own fp32 expression: o + (d * (t0 + t1)) / 2."""
    return o[ray_indices] + (d[ray_indices] * (t_starts + t_ends)[:, None]) / 2.0


@torch.no_grad()
def render_optical_flow(
    radiance_field: torch.nn.Module,
    estimator: OccGridEstimator,
    rays: Rays,
    project,
    dt: float,
    near_plane: float = 0.0,
    far_plane: float = 1e10,
    render_step_size: float = 1e-3,
    cone_angle: float = 0.0,
    alpha_thre: float = 0.0,
    test_chunk_size: int = 8192,
    timestamps: Optional[torch.Tensor] = None,
    return_samples: bool = False,
):
    """Per-pixel optical flow, in pixels per `dt`: every sample x_i is moved along its scene flow by dt, both points are
    projected, and the image-plane displacements are composited on `render_scene_flow`'s samples:
        flow2d = sum_i w_i * ok_i * (project(x_i + dt * v_i) - project(x_i)),   ok_i = valid_i and both points in front.
    project(points [S,3]) -> (pixels [S,2], in_front [S] bool) is any callable of that shape, applied to device tensors
    (`cameras.pinhole_projector` is the one shipped); it may project into another camera than the rays', e.g. the next
    frame's, if it is given that camera.  dt is a time difference in the units of `timestamps` (one frame of a path).
    Returns (flow2d [H,W,2], opacity [H,W,1], coverage [H,W,1], n_samples): coverage = sum_i w_i * ok_i <= opacity; the
    expected flow of the visible surface is flow2d / coverage.  With return_samples=True a fifth value is the list of
    per-chunk dicts, `render_scene_flow`'s plus `flow` [S,2] (the displacement, 0 where not ok) and `ok` [S] bool."""
    _check_eval_frame(radiance_field, timestamps, "render_optical_flow")
    if not rays.origins.is_cuda:
        raise NotImplementedError("Only support cuda inputs: render_optical_flow runs on the HIP kernels (no CPU fallback).")
    dt = float(dt)

    def flow_fn(o, d, ray_indices, t_starts, t_ends, ts):
        v, det, valid = radiance_field.query_scene_flow_rays(o, d, ray_indices, t_starts, t_ends, ts)
        x = sample_positions(o, d, ray_indices, t_starts, t_ends)
        p0, front0 = project(x)
        p1, front1 = project(x + dt * v)
        ok = valid & front0 & front1
        flow = torch.where(ok[:, None], (p1 - p0).float(), torch.zeros((), device=x.device))
        return {"flow": flow.contiguous(), "ok": ok, "velocity": v, "det": det, "valid": valid}

    flow2d, coverage, opacity, *rest = _render_sample_values(
        radiance_field, estimator, rays, near_plane, far_plane, render_step_size, cone_angle, alpha_thre, test_chunk_size,
        timestamps, return_samples, "render_optical_flow", ("flow", "ok"), flow_fn)
    return (flow2d, opacity, coverage, *rest)


@torch.no_grad()
def render_image_test(
    max_samples: int,
    radiance_field: torch.nn.Module,
    estimator: OccGridEstimator,
    rays: Rays,
    near_plane: float = 0.0,
    far_plane: float = 1e10,
    render_step_size: float = 1e-3,
    render_bkgd: Optional[torch.Tensor] = None,
    cone_angle: float = 0.0,
    alpha_thre: float = 0.0,
    early_stop_eps: float = 1e-4,
    timestamps: Optional[torch.Tensor] = None,
    tracer=None,
    field_stream=None,
    field_max_workgroups: int = 0,
):
    """Iterative eval renderer with per-iteration early termination (cednerf/utils.py:153-318).
    Returns (rgb, opacity, depth, total_samples).  `alpha_thre` is accepted and unused, as in the
    reference.  The whole loop runs inside the native library (ced_render_image_test): four
    launches per iteration, the N_samples schedule computed on the device; `render_image_test_staged` is the
    same algorithm driven from Python through the nerfacc-shaped ops."""
    estimator = grid_for(estimator, timestamps)
    if timestamps is None:
        raise NotImplementedError("DNGPradianceField needs timestamps (dnerf path of cednerf/utils.py:186-194)")
    rays, rays_shape, N_rays = _flatten_rays(rays)
    rays_o = rays.origins.contiguous().float()
    rays_d = rays.viewdirs.contiguous().float()
    bk = None if render_bkgd is None else render_bkgd.to(rays_o.device, torch.float32).reshape(-1).contiguous()
    ts = timestamps.reshape(-1).float().contiguous()
    rgb, opacity, depth, total = ops.render_image_test_native(
        radiance_field._descriptor(), rays_o, rays_d, estimator.binaries, estimator.aabbs.contiguous(), near_plane,
        far_plane, render_step_size, cone_angle, early_stop_eps, max_samples, ts, bool(radiance_field.training), bk,
        tracer=tracer, field_stream=field_stream, accel=estimator.occupancy_accel(), max_workgroups=field_max_workgroups)
    return (rgb.view((*rays_shape[:-1], -1)), opacity.view((*rays_shape[:-1], -1)),
            depth.view((*rays_shape[:-1], -1)), total)


@torch.no_grad()
def render_frames_test(
    max_samples: int,
    radiance_field: torch.nn.Module,
    estimator: OccGridEstimator,
    rays: Rays,
    near_plane: float = 0.0,
    far_plane: float = 1e10,
    render_step_size: float = 1e-3,
    render_bkgd: Optional[torch.Tensor] = None,
    cone_angle: float = 0.0,
    alpha_thre: float = 0.0,
    early_stop_eps: float = 1e-4,
    timestamps: Optional[torch.Tensor] = None,
    tracer=None,
    field_stream=None,
    field_max_workgroups: int = 0,
    exchange=None,
):
    """`render_image_test` for a stack of frames in one native call (ced_render_frames_test): rays.origins / viewdirs
    are [F, ..., 3] (F <= 64 frames of equal size), timestamps holds F times.  The frames share the launches of an
    iteration but each keeps its own reference loop, so frame f of the result equals
    `render_image_test(rays[f], timestamps[f])` bit for bit.  Returns (rgb [F,...,3], opacity [F,...,1],
    depth [F,...,1], [total_samples of every frame]).
    exchange (ops.ScheduleExchange): rays[f] is this rank's share of frame f, whose other rays other ranks render; the
    loop of every frame is then the WHOLE image's (N_rays // N_alive over all ranks, cednerf/utils.py:231-235)."""
    estimator = grid_for(estimator, timestamps)              # the range of the frames' times
    if timestamps is None:
        raise NotImplementedError("DNGPradianceField needs timestamps (dnerf path of cednerf/utils.py:186-194)")
    if radiance_field.training:
        raise NotImplementedError("render_frames_test renders eval frames (one time per frame)")
    shape = tuple(rays.origins.shape)
    assert len(shape) >= 3 and shape[-1] == 3 and tuple(rays.viewdirs.shape) == shape, "rays must be [F, ..., 3]"
    n_frames = shape[0]
    rays_o = rays.origins.reshape(-1, 3).contiguous().float()
    rays_d = rays.viewdirs.reshape(-1, 3).contiguous().float()
    bk = None if render_bkgd is None else render_bkgd.to(rays_o.device, torch.float32).reshape(-1).contiguous()
    ts = timestamps.reshape(-1).float().contiguous()
    assert ts.numel() == n_frames, "one timestamp per frame"
    rgb, opacity, depth, totals = ops.render_frames_test_native(
        radiance_field._descriptor(), n_frames, rays_o, rays_d, estimator.binaries, estimator.aabbs.contiguous(),
        near_plane, far_plane, render_step_size, cone_angle, early_stop_eps, max_samples, ts, bk,
        tracer=tracer, field_stream=field_stream, accel=estimator.occupancy_accel(), max_workgroups=field_max_workgroups,
        exchange=exchange)
    return rgb.view((*shape[:-1], 3)), opacity.view((*shape[:-1], 1)), depth.view((*shape[:-1], 1)), totals


@torch.no_grad()
def render_image_test_staged(
    max_samples: int,
    radiance_field: torch.nn.Module,
    estimator: OccGridEstimator,
    rays: Rays,
    near_plane: float = 0.0,
    far_plane: float = 1e10,
    render_step_size: float = 1e-3,
    render_bkgd: Optional[torch.Tensor] = None,
    cone_angle: float = 0.0,
    alpha_thre: float = 0.0,
    early_stop_eps: float = 1e-4,
    timestamps: Optional[torch.Tensor] = None,
):
    """render_image_test (cednerf/utils.py:153-318) staged from Python through the nerfacc-shaped
    ops (count -> scan -> fill marching, field, composite_step): the reference's own structure,
    kept for per-kernel profiling and as a cross-check of the native loop."""
    estimator = grid_for(estimator, timestamps)
    if timestamps is None:
        raise NotImplementedError("DNGPradianceField needs timestamps (dnerf path of cednerf/utils.py:186-194)")
    rays, rays_shape, N_rays = _flatten_rays(rays)
    rays_o = rays.origins.contiguous().float()
    rays_d = rays.viewdirs.contiguous().float()
    device = rays_o.device
    opacity = torch.zeros(N_rays, 1, device=device)
    depth = torch.zeros(N_rays, 1, device=device)
    rgb = torch.zeros(N_rays, 3, device=device)
    ray_mask = torch.ones(N_rays, device=device).bool()
    min_samples = 1 if cone_angle == 0 else 4
    iter_samples = total_samples = 0
    near_planes = torch.full_like(rays_o[..., 0], fill_value=near_plane)
    far_planes = torch.full_like(rays_o[..., 0], fill_value=far_plane)
    aabbs = estimator.aabbs.contiguous()
    t_mins, t_maxs, hits = ray_aabb_intersect(rays_o, rays_d, aabbs)
    t_sorted, t_indices = sort_intersections(t_mins, t_maxs)
    opc_thres = 1 - early_stop_eps
    op_flat, dp_flat = opacity.view(-1), depth.view(-1)
    binaries = estimator.binaries
    # Per-iteration bookkeeping stays on the device: the composite kernel updates the ray mask and
    # counts the surviving rays / composited samples; the host reads both with one 16-byte copy
    # (the single sync per iteration that the reference's `ray_mask.sum().item()` also pays).
    stats = torch.zeros((max(int(max_samples), 1) + 1, 2), device=device, dtype=torch.int64)
    host_stats = torch.zeros((2,), dtype=torch.int64).pin_memory()
    stream = torch.cuda.current_stream()
    N_alive = N_rays
    it = 0
    while iter_samples < max_samples:
        if N_alive == 0:
            break
        N_samples = max(min(N_rays // N_alive, 64), min_samples)
        iter_samples += N_samples
        bound = N_alive * N_samples                       # host-known upper bound of this iteration's samples
        counts = torch.empty((N_rays,), device=device, dtype=torch.int64)
        march = (rays_o, rays_d, binaries, aabbs, near_planes, far_planes, render_step_size, cone_angle, N_samples,
                 ray_mask, t_sorted, t_indices, hits)
        ops.traverse_grids_raw(*march, 0, counts=counts)
        incl = torch.cumsum(counts, 0)
        t_starts = torch.empty((bound,), device=device, dtype=torch.float32)
        t_ends = torch.empty((bound,), device=device, dtype=torch.float32)
        ray_indices = torch.empty((bound,), device=device, dtype=torch.int64)
        packed_info = torch.empty((N_rays, 2), device=device, dtype=torch.int64)
        # fill; the termination planes overwrite the near planes in place (cednerf/utils.py:301)
        ops.traverse_grids_raw(*march, 3, base=incl, counts=counts, t_starts=t_starts, t_ends=t_ends,
                               ray_indices=ray_indices, termination_planes=near_planes, packed_info_out=packed_info)
        rgbs, sigmas = radiance_field.query_rays(rays_o, rays_d, ray_indices, t_starts, t_ends, timestamps,
                                                 want_rgb=True, n_dev=incl[-1:])
        ops.composite_step_(packed_info, t_starts, t_ends, sigmas, rgbs, rgb, op_flat, dp_flat, opc_thres, N_samples,
                            ray_mask, stats[it])
        host_stats.copy_(stats[it], non_blocking=True)
        stream.synchronize()
        N_alive = int(host_stats[0])
        total_samples += int(host_stats[1])
        it += 1

    bk = None if render_bkgd is None else render_bkgd.to(device, torch.float32).reshape(-1).contiguous()
    ops.finalize_pixels_(bk, rgb, op_flat, dp_flat)
    return (rgb.view((*rays_shape[:-1], -1)), opacity.view((*rays_shape[:-1], -1)),
            depth.view((*rays_shape[:-1], -1)), total_samples)


# nerfacc's example name for the same role (BASELINE.json north_star)
render_image_with_occgrid = render_image
