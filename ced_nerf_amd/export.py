"""The radiance field itself as sparse voxel volumes, one per time step: what vis.py:13-46 hands to nerfvis.add_nerf,
up to the data nerfvis would consume, plus two plain file writers.

The grid is reso^3 cells over the bounding cube of the field's box (vis.py:40-41).  Cell centres, the occupancy mask, the
density threshold and the embedding x direction broadcast of the colour head run in HIP (csrc/bake.hip,
ced_field_rgb_bcast); the density in between is the field's own `ced_field_forward`, so `sigma` and `embedding` are
`query_density`'s bits in every mlp_precision.

    python -m ced_nerf_amd.export --load_model model.pth --preset dnerf -df -te --times 0,0.5,1 --out volumes/

`extract_mesh` / `extract_mesh_sequence` turn the same lattice of cell centres into a triangle mesh per time step: naive
surface nets on the device (csrc/mesh.hip), the vertices coloured by the field's own head.  `--mesh` writes them next to
the volumes.

`extract_mesh_tracked` / `track_mesh` give ONE mesh that moves instead: the mesh of a reference time, its faces shared by
every time step, its vertices carried through time by inverting the warp (DNGPradianceField.track_points,
ced_field_track).  `--mesh --mesh_track T_REF` writes it.
"""
from __future__ import annotations

import argparse
import os
import struct
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .nerfacc_api import TimeSlicedOccGrid
from .utils import grid_for

_CPU = "Only support cuda inputs: the volume export runs on the HIP kernels (no CPU fallback)."


def _cube(field, center, radius):
    """vis.py:40-41 on field.aabb: centre of the box, largest half extent."""
    aabb = field.aabb.detach().float().cpu()
    if center is None:
        center = ((aabb[3:] + aabb[:3]) / 2.0).tolist()
    if radius is None:
        radius = ((aabb[3:] - aabb[:3]) / 2.0).max().item()
    return [float(c) for c in center], float(radius)


def _check_grid(reso, center, radius):
    if not isinstance(reso, (int, np.integer)) or isinstance(reso, bool) or not 1 <= int(reso) <= 2048:
        raise ValueError(f"reso must be an int in 1 .. 2048, got {reso!r}")
    if len(center) != 3 or not all(np.isfinite(c) for c in center):
        raise ValueError(f"center must be 3 finite numbers, got {center!r}")
    if not (np.isfinite(radius) and radius > 0):
        raise ValueError(f"radius must be positive and finite, got {radius!r}")


def _origin_and_step(reso: int, center, radius: float):
    """lo_a = center_a - radius, h = (2 radius) / reso in fp32: the values ced_bake_candidates derives"""
    r = np.float32(radius)
    lo = np.asarray(center, np.float32) - r
    return lo, (np.float32(2.0) * r) / np.float32(reso)


def voxel_centers(reso: int, center, radius: float, device="cuda") -> torch.Tensor:
    """[reso^3, 3] centres of the cells of the cube [center - radius, center + radius]^3, flat index
    (ix * reso + iy) * reso + iz: p_a = lo_a + (i_a + 0.5) * h_a in fp32, multiply then add -- the torch restatement of
    what ced_bake_candidates computes per cell."""
    center = [float(c) for c in center]
    _check_grid(reso, center, radius)
    lo, h = _origin_and_step(reso, center, radius)
    i = torch.arange(int(reso), device=device, dtype=torch.float32) + 0.5
    step = torch.tensor(float(h), device=device, dtype=torch.float32)
    axes = [torch.tensor(float(lo[a]), device=device, dtype=torch.float32) + i * step for a in range(3)]
    return torch.stack(torch.meshgrid(axes, indexing="ij"), dim=-1).reshape(-1, 3)


def _check_dirs(dirs):
    if dirs is None:
        return None
    if not isinstance(dirs, torch.Tensor):
        dirs = torch.as_tensor(np.asarray(dirs, np.float32))
    if dirs.dim() != 2 or dirs.shape[1] != 3 or dirs.shape[0] < 1:
        raise ValueError(f"dirs must be [D, 3] with D >= 1, got {list(dirs.shape)}")
    return dirs


def _field_device(field) -> torch.device:
    dev = field.hash_table.device
    if dev.type != "cuda":
        raise NotImplementedError(_CPU)
    return dev


def _time_value(t) -> float:
    if isinstance(t, torch.Tensor):
        if t.numel() != 1:
            raise ValueError(f"t must be a float or a one-element tensor, got shape {list(t.shape)}")
        return float(t.reshape(-1)[0].item())
    return float(t)


def _candidates(reso, center, radius, dev, estimator, max_cells_per_launch):
    """(index [n], xyz [n,3]) of every cell worth evaluating, slab by slab"""
    binaries = aabbs = None
    if estimator is not None:
        binaries, aabbs = estimator.binaries, estimator.aabbs
        if not binaries.is_cuda:
            raise NotImplementedError(_CPU)
        binaries, aabbs = binaries.contiguous(), aabbs.float().contiguous()
    total = int(reso) ** 3
    parts = []
    for first in range(0, total, max_cells_per_launch):
        parts.append(ops.bake_candidates(reso, center, radius, first, min(max_cells_per_launch, total - first), dev,
                                         binaries, aabbs))
    if len(parts) == 1:
        return parts[0]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


def _candidates_by_time(reso, center, radius, dev, estimator, max_cells_per_launch):
    """t -> `_candidates`: computed once and shared by every time, or, through a TimeSlicedOccGrid, per time from the grid
    of that time (`utils.grid_for`)"""
    if isinstance(estimator, TimeSlicedOccGrid):
        return lambda t: _candidates(reso, center, radius, dev, grid_for(estimator, t), max_cells_per_launch)
    shared = _candidates(reso, center, radius, dev, estimator, max_cells_per_launch)
    return lambda t: shared


def _bake(field, cand, t: float, sigma_thresh: float, dirs, apply_act: bool, max_rows: int, meta: Dict) -> Dict:
    desc = field._descriptor()
    index, xyz = cand
    n = index.shape[0]
    parts = []
    for a in range(0, n, max_rows):
        b = min(n, a + max_rows)
        tt = torch.full((b - a,), t, device=xyz.device, dtype=torch.float32)
        _, sigma, emb = ops.field_forward(desc, xyz[a:b], tt, None, want_geo=True)
        parts.append(ops.bake_select(index[a:b], xyz[a:b], sigma, emb, sigma_thresh))
        del sigma, emb, tt
    if len(parts) == 1:
        kept = parts[0]
    elif parts:
        kept = tuple(torch.cat([p[k] for p in parts]) for k in range(4))
    else:
        dev = xyz.device
        kept = (torch.empty((0,), device=dev, dtype=torch.int64), torch.empty((0, 3), device=dev),
                torch.empty((0,), device=dev), torch.empty((0, 15), device=dev))
    out = dict(index=kept[0], xyz=kept[1], sigma=kept[2], embedding=kept[3])
    if dirs is not None:
        out["rgb"] = ops.field_rgb_bcast(desc, dirs, kept[3], apply_act)
    out.update(meta, t=t)
    return out


def _setup(field, reso, sigma_thresh, dirs, estimator, center, radius, max_cells_per_launch):
    center, radius = _cube(field, center, radius)
    _check_grid(reso, center, radius)
    if int(max_cells_per_launch) < 1:
        raise ValueError(f"max_cells_per_launch must be >= 1, got {max_cells_per_launch}")
    dirs = _check_dirs(dirs)
    dev = _field_device(field)
    if dirs is not None:
        if not dirs.is_cuda:
            raise NotImplementedError(_CPU)
        dirs = dirs.to(dev).float().contiguous()
    return dev, center, radius, dirs, int(max_cells_per_launch)


@torch.no_grad()
def bake_sequence(field, times: Sequence, reso: int = 128, sigma_thresh: float = 1.0, dirs=None, estimator=None,
                  apply_act: bool = False, center=None, radius=None, max_cells_per_launch: int = 1 << 22) -> List[Dict]:
    """`bake_volume` at every time of `times`: the candidate cells (the occupancy mask and the centres) are computed once
    and reused for every time."""
    dev, center, radius, dirs, max_cells = _setup(field, reso, sigma_thresh, dirs, estimator, center, radius,
                                                  max_cells_per_launch)
    times = [_time_value(t) for t in times]
    with torch.cuda.device(dev):
        cand_at = _candidates_by_time(int(reso), center, radius, dev, estimator, max_cells)
        meta = dict(reso=int(reso), center=center, radius=radius, apply_act=bool(apply_act))
        return [_bake(field, cand_at(t), t, float(sigma_thresh), dirs, apply_act, max_cells, meta) for t in times]


def bake_volume(field, t, reso: int = 128, sigma_thresh: float = 1.0, dirs=None, estimator=None, apply_act: bool = False,
                center=None, radius=None, max_cells_per_launch: int = 1 << 22) -> Dict:
    """The occupied volume of `field` at time t (a float or a one-element tensor; every cell takes it): of the reso^3
    cells over the cube [center - radius, center + radius]^3 (default: vis.py:40-41 on field.aabb) those with
    density >= sigma_thresh, in ascending cell order.  Returns
        index [M] int64 (flat cell index (ix * reso + iy) * reso + iz), xyz [M,3] (cell centres, `voxel_centers`' values),
        sigma [M] and embedding [M,15] (query_density(xyz, t, return_feat=True)'s bits),
        rgb [M,D,3] for dirs [D,3] (_query_rgb on every pair, sigmoid iff apply_act; absent without dirs),
        reso, center, radius, t (and apply_act, for the file writers).
    estimator: an OccGridEstimator; only cells its grid marks (smallest level that contains the centre) are evaluated.
    Grids larger than max_cells_per_launch cells run in slabs; the result does not depend on that value."""
    return bake_sequence(field, [t], reso, sigma_thresh, dirs, estimator, apply_act, center, radius,
                         max_cells_per_launch)[0]


def nerfvis_eval_fn(field, t=0.0):
    """The eval_fn of vis.py:24-34 for nerfvis.Scene.add_nerf(..., use_dirs=True): x [N,1,3], dirs [1,D,3] ->
    (rgb [N,D,3] before the activation, density [N,1]) at time t (the reference's commented version uses zeros)."""
    t = _time_value(t)

    @torch.no_grad()
    def eval_fn(x: torch.Tensor, dirs: torch.Tensor):
        if not (x.is_cuda and dirs.is_cuda):
            raise NotImplementedError(_CPU)
        pts = x.reshape(-1, 3)
        tt = torch.full((pts.shape[0], 1), t, device=x.device, dtype=torch.float32)
        res = field.query_density(pts, tt, return_feat=True)
        rgb = ops.field_rgb_bcast(field._descriptor(), dirs.reshape(-1, 3).float().contiguous(),
                                  res["base_mlp_out"].contiguous(), apply_act=False)
        return rgb, res["density"]

    return eval_fn


# ---- meshes ----------------------------------------------------------------------------------------------------------
MESH_MAX_RESO = 512                               # the dense density lattice is 4 * reso^3 bytes: 512 MiB
MESH_NORMALS = ("lattice", "field")               # where a mesh's vertex normals come from


def check_mesh_normals(normals) -> str:
    """`normals` of the mesh extractors, or ValueError."""
    if not isinstance(normals, str) or normals not in MESH_NORMALS:
        raise ValueError(f"normals must be one of {MESH_NORMALS}, got {normals!r}")
    return normals


def _check_mesh_reso(reso):
    if not isinstance(reso, (int, np.integer)) or isinstance(reso, bool) or not 1 <= int(reso) <= MESH_MAX_RESO:
        raise ValueError(f"reso must be an int in 1 .. {MESH_MAX_RESO} for a mesh, got {reso!r}")


def _vertex_values(field, vertices, normals, t: float, dirs, apply_act: bool, field_normals: bool) -> Dict:
    """What a mesh carries per vertex besides its position: sigma, embedding, the normals (the given ones, or the field's
    own slope at the vertices) and the colours."""
    v, dev = vertices.shape[0], vertices.device
    res = field.query_density(vertices, torch.full((v, 1), t, device=dev, dtype=torch.float32), return_feat=True)
    if field_normals:                                                            # the field's own slope at the vertices
        normals = field.query_normals(vertices, torch.full((v,), t, device=dev, dtype=torch.float32))[0]
    out = dict(normals=normals, sigma=res["density"].reshape(v), embedding=res["base_mlp_out"])
    if isinstance(dirs, str):                                                    # "normal": head-on, one direction each
        head_on = torch.where((normals == 0).all(-1, keepdim=True), normals.new_tensor([0.0, 0.0, 1.0]), -normals)
        out["rgb"] = field._query_rgb(head_on, out["embedding"], apply_act).view(v, 1, 3)
    elif dirs is not None:
        out["rgb"] = ops.field_rgb_bcast(field._descriptor(), dirs, out["embedding"], apply_act)
    return out


def _mesh(field, cand, t: float, sigma_thresh: float, dirs, apply_act: bool, max_rows: int, meta: Dict,
          field_normals: bool = False, refine: bool = False, refine_reach: float = 1.0) -> Dict:
    desc = field._descriptor()
    index, xyz = cand
    reso, dev = meta["reso"], xyz.device
    lattice = torch.zeros((reso ** 3,), device=dev, dtype=torch.float32)         # cells that are no candidates stay 0
    for a in range(0, index.shape[0], max_rows):
        b = min(index.shape[0], a + max_rows)
        tt = torch.full((b - a,), t, device=dev, dtype=torch.float32)
        _, sigma, _ = ops.field_forward(desc, xyz[a:b], tt, None, want_geo=False)
        lattice.index_copy_(0, index[a:b], sigma)
        del sigma, tt
    vertices, normals, cube, faces = ops.mesh_surface_nets(lattice.view(reso, reso, reso), sigma_thresh, meta["center"],
                                                           meta["radius"])
    del lattice
    out = dict(vertices=vertices, faces=faces, cube=cube)
    out.update(_vertex_values(field, vertices, normals, t, dirs, apply_act, field_normals))
    out.update(meta, t=t, dirs=dirs, normals_kind="field" if field_normals else "lattice")
    return refine_mesh(field, out, reach=refine_reach) if refine else out


def _check_reach(reach) -> float:
    try:
        reach_f = float(reach)
    except (TypeError, ValueError):
        raise ValueError(f"reach must be a positive finite number (in lattice spacings), got {reach!r}") from None
    if not (np.isfinite(reach_f) and reach_f > 0):
        raise ValueError(f"reach must be a positive finite number (in lattice spacings), got {reach!r}")
    return reach_f


@torch.no_grad()
def refine_mesh(field, mesh: Dict, reach: float = 1.0, max_iters: int = 32, tol: float = 0.0) -> Dict:
    """Move the vertices of `mesh` (a dict from `extract_mesh`) onto the level set density == sigma_thresh itself.  Surface
    nets put a vertex at the centroid of its lattice cube's edge crossings, up to a cell away from the surface: mesh["sigma"]
    scatters widely around the threshold.  Here each vertex v with a non-zero normal n (towards lower density) becomes the
    row o = v, d = -n, lo = -reach * h, hi = +reach * h of `DNGPradianceField.query_level_set` (h = the lattice spacing
    2 radius / reso, the mesh's t and sigma_thresh, one launch for all vertices): the bracket starts reach * h outside the
    surface nets' position and ends reach * h inside.  A row with a crossing (status 0) moves to it; every other row -- a
    zero normal, a bracket that starts at or above the threshold or never reaches it -- keeps its vertex, bit for bit.
    Returns a new mesh dict:
        vertices [V,3], refined [V] bool, offset [V] (the signed distance moved along n; 0 where not refined),
        width [V] (of the final bracket: density(vertex + n * width) < sigma_thresh <= sigma on refined vertices),
        sigma, embedding, rgb (if the mesh has colours) and, for a mesh extracted with normals="field", normals:
        re-evaluated at the new vertices as `extract_mesh` evaluates them,
        faces, cube, reso, center, radius, t, sigma_thresh, apply_act: the mesh's own.
    A hand-built mesh dict needs vertices, normals, reso, center, radius, t and sigma_thresh; without `dirs` it comes back
    without colours."""
    reach = _check_reach(reach)
    thresh, max_iters, tol = ops.check_level_set(mesh["sigma_thresh"], max_iters, tol)
    vertices, normals = mesh["vertices"], mesh["normals"]
    if not vertices.is_cuda:
        raise NotImplementedError(_CPU)
    t = _time_value(mesh["t"])
    _, h = _origin_and_step(int(mesh["reso"]), mesh["center"], mesh["radius"])
    with torch.cuda.device(vertices.device):
        v = vertices.shape[0]
        hi = torch.full((v,), float(np.float32(reach) * h), device=vertices.device, dtype=torch.float32)
        if v:
            s, x, _, width, status, _ = field.query_level_set(vertices, -normals, -hi, hi, t, thresh, max_iters, tol)
        else:
            s, x, width = hi, vertices, hi
            status = torch.ones((0,), device=vertices.device, dtype=torch.int32)
        refined = (status == 0) & (normals != 0).any(-1)
        out = dict(mesh)
        if "dirs" not in mesh:                                                   # a hand-built mesh: its colours cannot follow
            out.pop("rgb", None)
        out["vertices"] = torch.where(refined[:, None], x, vertices)
        out["refined"] = refined
        out["offset"] = torch.where(refined, -s, torch.zeros_like(s))
        out["width"] = torch.where(refined, width, torch.zeros_like(width))
        out.update(_vertex_values(field, out["vertices"], normals, t, mesh.get("dirs"), bool(mesh.get("apply_act", False)),
                                  mesh.get("normals_kind") == "field"))
    return out


@torch.no_grad()
def extract_mesh_sequence(field, times: Sequence, reso: int = 128, sigma_thresh: float = 1.0, dirs=None, estimator=None,
                          apply_act: bool = False, center=None, radius=None,
                          max_cells_per_launch: int = 1 << 22, normals: str = "lattice", refine: bool = False,
                          refine_reach: float = 1.0) -> List[Dict]:
    """`extract_mesh` at every time of `times`: the candidate cells (the occupancy mask and the centres) are computed
    once and reused for every time."""
    field_normals = check_mesh_normals(normals) == "field"
    refine_reach = _check_reach(refine_reach)
    _check_mesh_reso(reso)
    by_normal = isinstance(dirs, str)
    if by_normal and dirs != "normal":
        raise ValueError(f"dirs must be None, a [D, 3] tensor or 'normal', got {dirs!r}")
    dev, center, radius, tensor_dirs, max_cells = _setup(field, reso, sigma_thresh, None if by_normal else dirs, estimator,
                                                         center, radius, max_cells_per_launch)
    times = [_time_value(t) for t in times]
    with torch.cuda.device(dev):
        cand_at = _candidates_by_time(int(reso), center, radius, dev, estimator, max_cells)
        meta = dict(reso=int(reso), center=center, radius=radius, sigma_thresh=float(sigma_thresh),
                    apply_act=bool(apply_act))
        return [_mesh(field, cand_at(t), t, float(sigma_thresh), "normal" if by_normal else tensor_dirs, apply_act, max_cells,
                      meta, field_normals, bool(refine), refine_reach) for t in times]


def extract_mesh(field, t, reso: int = 128, sigma_thresh: float = 1.0, dirs=None, estimator=None, apply_act: bool = False,
                 center=None, radius=None, max_cells_per_launch: int = 1 << 22, normals: str = "lattice",
                 refine: bool = False, refine_reach: float = 1.0) -> Dict:
    """The iso-surface density == sigma_thresh of `field` at time t as a triangle mesh: naive surface nets (the
    definition is in include/cednerf_hip.h) on the lattice of `voxel_centers`(reso, center, radius), reso <= 512, whose
    densities are query_density's bits (0 at the cells an `estimator` does not mark).  Returns
        vertices [V,3], normals [V,3] (unit, towards lower density; zero where the density gradient vanishes):
        normals="lattice" (the default) central differences of the reso^3 lattice, normals="field" the field's analytic
        gradient at the vertices, `DNGPradianceField.query_normals`(vertices, t)[0], which resolves what the hash grid's
        fine levels hold; everything else is the same mesh; any other value raises ValueError,
        faces [F,3] int32 (counter-clockwise seen from outside), cube [V] int64 (the lattice cube of each vertex),
        sigma [V] and embedding [V,15] (query_density(vertices, t, return_feat=True)'s bits),
        rgb [V,D,3]: for dirs [D,3] _query_rgb on every pair; for dirs="normal" D = 1 and every vertex is viewed head-on,
        along -normal ((0,0,1) where the normal is zero); the sigmoid iff apply_act; absent without dirs,
        reso, center, radius, t, sigma_thresh, apply_act (and dirs, normals_kind: what `refine_mesh` re-evaluates with).
    The mesh is closed away from the lattice border and open on it; its vertex and face order do not depend on the run
    or on max_cells_per_launch.
    refine=True: the result is `refine_mesh`(field, mesh, reach=refine_reach) -- the vertices moved along their normals
    onto density == sigma_thresh, with `refined`, `offset` and `width` per vertex; refine=False leaves the mesh as it is."""
    return extract_mesh_sequence(field, [t], reso, sigma_thresh, dirs, estimator, apply_act, center, radius,
                                 max_cells_per_launch, normals, refine, refine_reach)[0]


# ---- a mesh that moves -----------------------------------------------------------------------------------------------
_REF_KEYS = ("faces", "cube", "sigma", "embedding", "rgb", "normals")


@torch.no_grad()
def track_mesh(field, mesh: Dict, t_src, times: Sequence, max_iters: int = 32, tol: float = 1e-6,
               method: str = "fixed_point", normals: bool = False, velocities: bool = False) -> Dict:
    """Carry the vertices of `mesh` (a dict from `extract_mesh`, extracted at time t_src) to every time of `times`: each
    vertex is a material point, its canonical coordinate is query_move(vertex, t_src)[0], and its position at time t
    solves x + move(x, t) = canonical (`DNGPradianceField.track_points`, started at the vertex; `method` as there).  Returns
        vertices_t [T,V,3], converged [T,V] bool, step [T,V], evals [T,V] int32, canonical [V,3], times [T], t_ref,
        faces, cube, sigma, embedding, normals (and rgb if present): the reference mesh's own, valid at t_ref ONLY --
        faces are shared by all times; colours are not recomputed per time,
        reso, center, radius, sigma_thresh, apply_act,
        normals=True (the mesh must have normals): normals_t [T,V,3], the reference normals carried along, whichever the
        mesh has (extract_mesh's normals="lattice" or "field").  The surface
        is a level set of the canonical density pulled back through the warp, whose gradient at (x, t) is
        (I + J_x(x, t))^T times the canonical gradient, so n_t is (I + J_t(x_t))^T (I + J_ref(x_ref))^-T n_ref, normalised,
        velocities=True: velocities_t [T,V,3] and det_t [T,V], `DNGPradianceField.query_velocity` at the tracked vertices.
    Neither solver is damped: a vertex that does not converge is reported in `converged`, its position the last iterate."""
    max_iters, tol = ops.check_solve(max_iters, tol)
    ops.check_method(method)
    t_ref = _time_value(t_src)
    times = [_time_value(t) for t in times]
    vertices = mesh["vertices"]
    if normals and "normals" not in mesh:
        raise ValueError("normals=True needs a mesh with normals")
    if not vertices.is_cuda:
        raise NotImplementedError(_CPU)
    with torch.cuda.device(vertices.device):
        tr = field.track_points(vertices, t_ref, times, max_iters=max_iters, tol=tol, method=method)
        moving = {}
        if normals or velocities:
            n_v = vertices.shape[0]
            tt = tr["times"].repeat_interleave(n_v)
            jac_t = field.query_move_jacobian(tr["positions"].reshape(-1, 3), tt)[1].view(len(times), n_v, 3, 4)
            grad_t, inv_t, det_t = ops.warp_gradient(jac_t)
            if normals:
                jac_ref = field.query_move_jacobian(vertices, torch.full((n_v,), t_ref, device=vertices.device))[1]
                inv_ref = ops.warp_gradient(jac_ref)[1]
                canonical_grad = (inv_ref.transpose(-1, -2) @ mesh["normals"][..., None])          # [V,3,1]
                n_t = (grad_t.transpose(-1, -2) @ canonical_grad).squeeze(-1)
                # a zero reference normal (vanishing density gradient) stays zero
                moving["normals_t"] = n_t / n_t.norm(dim=-1, keepdim=True).clamp_min(torch.finfo(n_t.dtype).tiny)
            if velocities:
                moving["velocities_t"] = -(inv_t @ jac_t[..., 3:]).squeeze(-1)
                moving["det_t"] = det_t
    out = {k: mesh[k] for k in _REF_KEYS if k in mesh}
    out.update({k: mesh[k] for k in ("reso", "center", "radius", "sigma_thresh", "apply_act") if k in mesh})
    out.update(vertices_t=tr["positions"], converged=tr["converged"], step=tr["step"], evals=tr["evals"],
               canonical=tr["canonical"], times=times, t_ref=t_ref)
    out.update(moving)
    return out


@torch.no_grad()
def extract_mesh_tracked(field, t_ref, times: Sequence, reso: int = 128, sigma_thresh: float = 1.0, dirs=None,
                         estimator=None, apply_act: bool = False, center=None, radius=None,
                         max_cells_per_launch: int = 1 << 22, max_iters: int = 32, tol: float = 1e-6,
                         method: str = "fixed_point", normals=False, velocities: bool = False, refine: bool = False,
                         refine_reach: float = 1.0) -> Dict:
    """`extract_mesh` at t_ref followed by `track_mesh` to `times`: one mesh with shared faces and per-time vertex
    positions (see `track_mesh` for the result, `method`, `normals` and `velocities`).  normals: False / True as
    `track_mesh`'s, on the lattice normals; "lattice" or "field": the reference mesh takes those normals
    (`extract_mesh`'s normals=) and they are carried along.  refine / refine_reach: `extract_mesh`'s; the reference
    mesh is refined before it is tracked."""
    max_iters, tol = ops.check_solve(max_iters, tol)
    ops.check_method(method)
    kind = "lattice" if isinstance(normals, bool) else check_mesh_normals(normals)
    mesh = extract_mesh(field, t_ref, reso, sigma_thresh, dirs, estimator, apply_act, center, radius, max_cells_per_launch,
                        normals=kind, refine=refine, refine_reach=refine_reach)
    return track_mesh(field, mesh, t_ref, times, max_iters=max_iters, tol=tol, method=method, normals=bool(normals),
                      velocities=velocities)


def tracked_frame(tracked: Dict, k: int) -> Dict:
    """Time step k of a tracked mesh as a dict `save_mesh_ply` writes: the vertices of that time, the shared faces, the
    reference colours -- and that time's normals where the mesh was tracked with normals=True (`normals_t`); the
    reference normals belong to t_ref only and are never used."""
    out = dict(vertices=tracked["vertices_t"][k], faces=tracked["faces"], t=tracked["times"][k])
    out.update({key: tracked[key] for key in ("rgb", "apply_act") if key in tracked})
    if "normals_t" in tracked:
        out["normals"] = tracked["normals_t"][k]
    return out


# ---- files -----------------------------------------------------------------------------------------------------------
_ARRAYS = ("index", "xyz", "sigma", "embedding", "rgb")


def save_npz(path: str, volume: Dict) -> None:
    """The volume's arrays and scalars as a numpy .npz (index, xyz, sigma, embedding, rgb if present, reso, center,
    radius, t, apply_act: whether rgb holds colours after the sigmoid)."""
    out = {k: volume[k].detach().cpu().numpy() for k in _ARRAYS if k in volume}
    out.update(reso=np.int64(volume["reso"]), center=np.asarray(volume["center"], np.float32),
               radius=np.float32(volume["radius"]), t=np.float32(volume["t"]),
               apply_act=np.bool_(volume.get("apply_act", False)))
    np.savez(path, **out)


def ply_header(n: int) -> bytes:
    return ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {int(n)}\n"
            "property float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\n"
            "property float sigma\nend_header\n").encode("ascii")


PLY_RECORD = struct.Struct("<fffBBBf")            # 19 bytes per vertex, no padding


def save_ply(path: str, volume: Dict, dirs_reduce: str = "mean") -> None:
    """A binary little-endian point cloud: x y z, red green blue, sigma.  The colour is the sigmoid of rgb (applied here
    unless the volume was baked with apply_act) averaged over the directions; grey 128 without rgb."""
    if dirs_reduce != "mean":
        raise ValueError(f"dirs_reduce={dirs_reduce!r}: only 'mean'")
    xyz = volume["xyz"].detach().cpu().numpy().astype("<f4")
    sigma = volume["sigma"].detach().cpu().numpy().astype("<f4")
    n = xyz.shape[0]
    if "rgb" in volume:
        rgb = volume["rgb"].detach().cpu().numpy().astype(np.float64)
        if not volume.get("apply_act", False):
            rgb = 1.0 / (1.0 + np.exp(-rgb))
        col = np.clip(np.rint(255.0 * rgb.mean(axis=1)), 0, 255).astype(np.uint8)
    else:
        col = np.full((n, 3), 128, np.uint8)
    rec = np.empty(n, dtype=np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3), ("sigma", "<f4")]))
    assert rec.dtype.itemsize == PLY_RECORD.size
    rec["xyz"], rec["rgb"], rec["sigma"] = xyz, col, sigma
    with open(path, "wb") as f:
        f.write(ply_header(n))
        f.write(rec.tobytes())


_MESH_ARRAYS = ("vertices", "normals", "faces", "cube", "sigma", "embedding", "rgb", "refined", "offset", "width")


def save_mesh_npz(path: str, mesh: Dict) -> None:
    """The mesh's arrays and scalars as a numpy .npz (vertices, normals, faces, cube, sigma, embedding, rgb if present,
    refined / offset / width of a refined mesh, reso, center, radius, t, sigma_thresh, apply_act)."""
    out = {k: mesh[k].detach().cpu().numpy() for k in _MESH_ARRAYS if k in mesh}
    out.update(reso=np.int64(mesh["reso"]), center=np.asarray(mesh["center"], np.float32),
               radius=np.float32(mesh["radius"]), t=np.float32(mesh["t"]), sigma_thresh=np.float32(mesh["sigma_thresh"]),
               apply_act=np.bool_(mesh.get("apply_act", False)))
    np.savez(path, **out)


_TRACKED_ARRAYS = ("vertices_t", "converged", "step", "evals", "canonical", "normals_t", "velocities_t", "det_t") + _REF_KEYS


def save_tracked_npz(path: str, tracked: Dict) -> None:
    """A tracked mesh as a numpy .npz: vertices_t, converged, step, evals, canonical, times, t_ref, the moving normals_t,
    velocities_t and det_t where the mesh was tracked with them, and the reference
    mesh's faces, cube, sigma, embedding, normals, rgb, reso, center, radius, sigma_thresh -- each if present, so the
    result of track_mesh on a hand-built mesh dict (vertices and faces only) is saved too -- and apply_act (False if absent)."""
    out = {k: tracked[k].detach().cpu().numpy() for k in _TRACKED_ARRAYS if k in tracked}
    out.update(times=np.asarray(tracked["times"], np.float32), t_ref=np.float32(tracked["t_ref"]))
    kinds = dict(reso=np.int64, center=lambda v: np.asarray(v, np.float32), radius=np.float32, sigma_thresh=np.float32)
    out.update({k: kind(tracked[k]) for k, kind in kinds.items() if k in tracked})   # track_mesh's rule: what the mesh had
    out["apply_act"] = np.bool_(tracked.get("apply_act", False))
    np.savez(path, **out)


def mesh_ply_header(n_vertices: int, n_faces: int, normals: bool = True) -> bytes:
    return ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {int(n_vertices)}\n"
            "property float x\nproperty float y\nproperty float z\n"
            + ("property float nx\nproperty float ny\nproperty float nz\n" if normals else "") +
            "property uchar red\nproperty uchar green\nproperty uchar blue\n"
            f"element face {int(n_faces)}\n"
            "property list uchar int vertex_indices\nend_header\n").encode("ascii")


MESH_PLY_VERTEX = struct.Struct("<ffffffBBB")     # 27 bytes per vertex, no padding
MESH_PLY_VERTEX_PLAIN = struct.Struct("<fffBBB")  # 15 bytes per vertex of a mesh without normals
MESH_PLY_FACE = struct.Struct("<Biii")            # 13 bytes per triangle: the count 3, then the vertex ids


def save_mesh_ply(path: str, mesh: Dict) -> None:
    """A binary little-endian triangle mesh: x y z nx ny nz red green blue per vertex, a uchar-counted int list per face.
    The colour follows save_ply: the sigmoid of rgb (applied here unless the mesh was extracted with apply_act) averaged
    over the directions; grey 128 without rgb.  A mesh without `normals` (a frame of a tracked mesh, `tracked_frame`) is
    written without the three normal properties: x y z red green blue per vertex."""
    xyz = mesh["vertices"].detach().cpu().numpy().astype("<f4")
    nrm = mesh["normals"].detach().cpu().numpy().astype("<f4") if "normals" in mesh else None
    tri = mesh["faces"].detach().cpu().numpy().astype("<i4")
    n = xyz.shape[0]
    if "rgb" in mesh:
        rgb = mesh["rgb"].detach().cpu().numpy().astype(np.float64)
        if not mesh.get("apply_act", False):
            rgb = 1.0 / (1.0 + np.exp(-rgb))
        col = np.clip(np.rint(255.0 * rgb.mean(axis=1)), 0, 255).astype(np.uint8)
    else:
        col = np.full((n, 3), 128, np.uint8)
    frec = np.empty(tri.shape[0], dtype=np.dtype([("n", "u1"), ("ids", "<i4", 3)]))
    if nrm is None:
        vrec = np.empty(n, dtype=np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]))
        assert vrec.dtype.itemsize == MESH_PLY_VERTEX_PLAIN.size and frec.dtype.itemsize == MESH_PLY_FACE.size
        vrec["xyz"], vrec["rgb"] = xyz, col
    else:
        vrec = np.empty(n, dtype=np.dtype([("xyz", "<f4", 3), ("normal", "<f4", 3), ("rgb", "u1", 3)]))
        assert vrec.dtype.itemsize == MESH_PLY_VERTEX.size and frec.dtype.itemsize == MESH_PLY_FACE.size
        vrec["xyz"], vrec["normal"], vrec["rgb"] = xyz, nrm, col
    frec["n"], frec["ids"] = 3, tri
    with open(path, "wb") as f:
        f.write(mesh_ply_header(n, tri.shape[0], normals=nrm is not None))
        f.write(vrec.tobytes())
        f.write(frec.tobytes())


def fibonacci_dirs(n: int) -> np.ndarray:
    """n unit directions spread over the sphere (golden-angle spiral), [n,3] float32"""
    k = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], -1).astype(np.float32)


# ---- command line ----------------------------------------------------------------------------------------------------
def make_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m ced_nerf_amd.export",
                                description="Write the field of a model.pth as sparse voxel volumes, one per time")
    p.add_argument("--load_model", required=True, metavar="PATH")
    p.add_argument("--preset", required=True, choices=["dnerf", "hypernerf", "dynerf"])
    p.add_argument("--assume_tcnn_layout", default=None, help="for a --load_model file written by the reference")
    p.add_argument("--log2_hashmap_size", type=int, default=21)
    p.add_argument("-ms", "--moving_step", type=float, default=None)
    p.add_argument("-df", "--use_div_offsets", action="store_true")
    p.add_argument("-f", "--use_feat_predict", action="store_true")
    p.add_argument("-w", "--use_weight_predict", action="store_true")
    p.add_argument("-te", "--use_time_embedding", action="store_true")
    p.add_argument("-ta", "--use_time_attenuation", action="store_true")
    p.add_argument("--times", type=parse_times, default=[0.0], help="comma-separated times in [0, 1], e.g. 0,0.5,1")
    p.add_argument("--reso", type=int, default=128)
    p.add_argument("--sigma_thresh", type=float, default=1.0)
    p.add_argument("--n_dirs", type=int, default=0, help="view directions to evaluate the colour for (0: no colour)")
    p.add_argument("--no_occupancy", action="store_true", help="evaluate every cell, not only those the grid marks")
    p.add_argument("--mesh", action="store_true", help="also write a triangle mesh per time: mesh_%%04d.ply / .npz")
    p.add_argument("--mesh_dirs", type=parse_mesh_dirs, default="normal", metavar="normal|N",
                   help="view directions of the mesh colours: 'normal' (every vertex head-on) or N directions spread over "
                        "the sphere and averaged (0: no colour)")
    p.add_argument("--mesh_normals", choices=MESH_NORMALS, default="lattice",
                   help="vertex normals of the meshes: central differences of the density lattice, or the field's analytic "
                        "gradient at the vertices")
    p.add_argument("--mesh_refine", action="store_true",
                   help="with --mesh: move every vertex along its normal onto density == sigma_thresh (bisection on the field)")
    p.add_argument("--mesh_refine_reach", type=float, default=1.0, metavar="R",
                   help="--mesh_refine: how far from a vertex the surface is searched, in lattice spacings")
    p.add_argument("--mesh_track", type=float, default=None, metavar="T_REF",
                   help="with --mesh: also write ONE mesh that moves -- the mesh of time T_REF, its vertices tracked to every "
                        "time of --times by inverting the warp: tracked_%%04d.ply per time and tracked.npz")
    p.add_argument("--track_iters", type=int, default=32, help="--mesh_track: most evaluations of the motion network per vertex and time")
    p.add_argument("--track_tol", type=float, default=1e-6, help="--mesh_track: a vertex has converged when its last update is <= this")
    p.add_argument("--mesh_track_method", choices=ops.SOLVE_METHODS, default="fixed_point",
                   help="--mesh_track: how the warp is inverted -- the fixed-point iteration, or Newton's method on the warp's "
                        "Jacobian, which converges on most vertices the fixed point loses")
    p.add_argument("--mesh_track_normals", action="store_true",
                   help="--mesh_track: carry the normals along (tracked_%%04d.ply get normals, tracked.npz gets normals_t)")
    p.add_argument("--device", default="cuda")
    p.add_argument("--out", required=True, metavar="DIR")
    return p


def parse_mesh_dirs(text: str):
    if text == "normal":
        return text
    try:
        n = int(text)
    except ValueError:
        n = -1
    if n < 0:
        raise argparse.ArgumentTypeError(f"--mesh_dirs {text!r}: 'normal' or a number of directions >= 0")
    return n


def parse_times(text: str) -> List[float]:
    try:
        times = [float(v) for v in text.split(",") if v.strip() != ""]
    except ValueError:
        raise argparse.ArgumentTypeError(f"--times {text!r}: comma-separated numbers")
    if not times:
        raise argparse.ArgumentTypeError("--times: no time given")
    return times


def main(argv=None) -> int:
    from . import checkpoint, trainer
    a = make_parser().parse_args(argv)
    if a.n_dirs < 0:
        raise SystemExit("--n_dirs must be >= 0")
    if a.mesh_track is not None and not a.mesh:
        raise SystemExit("--mesh_track needs --mesh")
    if a.mesh_refine and not a.mesh:
        raise SystemExit("--mesh_refine needs --mesh")
    if not (np.isfinite(a.mesh_refine_reach) and a.mesh_refine_reach > 0):
        raise SystemExit("--mesh_refine_reach must be positive")
    extra = {} if a.moving_step is None else dict(moving_step=a.moving_step)
    cfg = trainer.resolve_config(a.preset, None, log2_hashmap_size=a.log2_hashmap_size, **extra)
    ckpt = checkpoint.read_checkpoint(a.load_model)
    state = ckpt["radiance_field"]
    dtype = torch.float16 if checkpoint.is_reference_state(state) else state["hash_table"].dtype
    field, estimator = trainer.build_modules(
        cfg, torch.device(a.device), hash_dtype=dtype, use_div_offsets=a.use_div_offsets,
        use_time_embedding=a.use_time_embedding, use_time_attenuation=a.use_time_attenuation,
        use_feat_predict=a.use_feat_predict, use_weight_predict=a.use_weight_predict)
    checkpoint.load_checkpoint(ckpt, field, estimator, assume_tcnn_layout=a.assume_tcnn_layout)
    dirs = torch.from_numpy(fibonacci_dirs(a.n_dirs)).to(field.hash_table.device) if a.n_dirs else None
    os.makedirs(a.out, exist_ok=True)
    volumes = bake_sequence(field, a.times, reso=a.reso, sigma_thresh=a.sigma_thresh, dirs=dirs,
                            estimator=None if a.no_occupancy else estimator)
    for i, vol in enumerate(volumes):
        stem = os.path.join(a.out, f"volume_{i:04d}")
        save_npz(stem + ".npz", vol)
        save_ply(stem + ".ply", vol)
        print(f"t={vol['t']:g}: {vol['index'].shape[0]} of {a.reso ** 3} cells -> {stem}.npz / .ply", flush=True)
    if a.mesh:
        if a.mesh_dirs == "normal" or a.mesh_dirs == 0:
            mesh_dirs = a.mesh_dirs or None
        else:
            mesh_dirs = torch.from_numpy(fibonacci_dirs(a.mesh_dirs)).to(field.hash_table.device)
        meshes = extract_mesh_sequence(field, a.times, reso=a.reso, sigma_thresh=a.sigma_thresh, dirs=mesh_dirs,
                                       estimator=None if a.no_occupancy else estimator, normals=a.mesh_normals,
                                       refine=a.mesh_refine, refine_reach=a.mesh_refine_reach)
        for i, mesh in enumerate(meshes):
            stem = os.path.join(a.out, f"mesh_{i:04d}")
            save_mesh_npz(stem + ".npz", mesh)
            save_mesh_ply(stem + ".ply", mesh)
            print(f"t={mesh['t']:g}: {mesh['vertices'].shape[0]} vertices, {mesh['faces'].shape[0]} triangles -> "
                  f"{stem}.npz / .ply", flush=True)
            if a.mesh_refine:
                share = 100.0 * float(mesh["refined"].float().mean()) if mesh["refined"].numel() else 0.0
                print(f"t={mesh['t']:g}: {share:.2f} % of the vertices refined onto sigma == {a.sigma_thresh:g}", flush=True)
        if a.mesh_track is not None:
            ref = extract_mesh(field, a.mesh_track, reso=a.reso, sigma_thresh=a.sigma_thresh, dirs=mesh_dirs,
                               estimator=None if a.no_occupancy else estimator, normals=a.mesh_normals,
                               refine=a.mesh_refine, refine_reach=a.mesh_refine_reach)
            tracked = track_mesh(field, ref, a.mesh_track, a.times, max_iters=a.track_iters, tol=a.track_tol,
                                 method=a.mesh_track_method, normals=a.mesh_track_normals)
            save_tracked_npz(os.path.join(a.out, "tracked.npz"), tracked)
            n_vertices = tracked["vertices_t"].shape[1]
            lost = (~tracked["converged"]).sum(dim=1).tolist()
            for i, t in enumerate(tracked["times"]):
                stem = os.path.join(a.out, f"tracked_{i:04d}")
                save_mesh_ply(stem + ".ply", tracked_frame(tracked, i))
                share = 100.0 * lost[i] / max(n_vertices, 1)
                print(f"t={t:g}: {n_vertices} vertices tracked from t_ref={tracked['t_ref']:g}, {lost[i]} ({share:.2f} %) "
                      f"not converged -> {stem}.ply", flush=True)
            print(f"tracked mesh: {tracked['faces'].shape[0]} shared triangles -> {os.path.join(a.out, 'tracked.npz')}",
                  flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
