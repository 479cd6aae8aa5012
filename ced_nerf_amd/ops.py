"""Torch-tensor front-end of the C ABI (``include/cednerf_hip.h``).

PyTorch is used for device memory and streams only; all arithmetic happens in the HIP kernels.
Every wrapper validates device / dtype / contiguity (mirroring the reference's asserts,
cednerf/render.py:16-22,74-79) and enqueues on the current torch stream.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib, profiling
from .hashgrid import level_tables


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t: Optional[torch.Tensor], dtype: torch.dtype, name: str, allow_none: bool = False):
    if t is None:
        if allow_none:
            return None
        raise ValueError(f"{name} is required")
    if not t.is_cuda:
        raise NotImplementedError(f"Only support cuda inputs ({name} is on {t.device}).")
    _check_current_device(t.device.index, name)
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def _check_current_device(index, name: str) -> None:
    """The library launches on the CURRENT device and stream (`_stream()`), with raw pointers: a tensor of another
    device would be dereferenced on the wrong GPU (a memory fault, not an exception).  Refuse instead."""
    cur = torch.cuda.current_device()
    if index is not None and index != cur:
        raise RuntimeError(f"{name} lives on cuda:{index} but the current device is cuda:{cur}: wrap the call in "
                           f"`with torch.cuda.device({index}):` (the kernels launch on the current device's stream)")


def _p(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def _as_u8(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if t is None:
        return None
    return t.view(torch.uint8) if t.dtype == torch.bool else t


# ----------------------------------------------------------------------------------------------
# field parameters on the device
# ----------------------------------------------------------------------------------------------
def make_hash_desc(table: torch.Tensor, base_res: int, max_res: int, n_levels: int, log2_hashmap_size: int,
                   temporal: bool = False) -> Tuple[_lib.HashDesc, Dict]:
    tabs = level_tables(base_res, max_res, n_levels, log2_hashmap_size)
    width = 8 if temporal else 2
    if table.dtype not in (torch.float32, torch.float16):
        raise TypeError("hash table must be float32 or float16")
    if tuple(table.shape) != (tabs["total"], width) or not table.is_contiguous() or not table.is_cuda:
        raise ValueError(f"hash table must be a contiguous cuda tensor of shape {(tabs['total'], width)}, "
                         f"got {tuple(table.shape)} on {table.device}")
    d = _lib.HashDesc()
    d.n_levels = n_levels
    d.table_dtype = 0 if table.dtype == torch.float32 else 1
    d.temporal = int(bool(temporal))
    for l in range(n_levels):
        d.scale[l] = float(tabs["scale"][l])
        d.res[l] = int(tabs["res"][l])
        d.offset[l] = int(tabs["offset"][l])
        d.size[l] = int(tabs["size"][l])
        d.hashed[l] = int(tabs["hashed"][l])
    d.table = table.data_ptr()
    d.total_entries = int(tabs["total"])
    return d, tabs


def pack_field_weights(use_div_offsets: bool, time_mode: int, xyz_wrap, mlp_base, mlp_head,
                       mlp_precision: int = _lib.MLP_F32, table_dtype: int = 0, temporal: bool = False) -> np.ndarray:
    """Host: natural W[out][in] float32 arrays -> MFMA-fragment-order blob (ced_pack_field_weights for the
    fp32 kernel, ced_pack_field_weights_half_for for the f16x2 / f16 kernels; the latter returns uint32 words).
    table_dtype (0 = float32, 1 = float16 entries) and temporal describe the hash table the blob is used with: the
    half-precision kernels differ in their weight placements by table as well as by mode."""
    L = _lib.lib()
    mats = [np.ascontiguousarray(np.asarray(w, np.float32)) for w in list(xyz_wrap) + list(mlp_base) + list(mlp_head)]
    base_in = 41 if time_mode else 32
    n_mo = 6 if use_div_offsets else 3
    want = [(64, 32), (64, 64), (64, 64), (n_mo, 64), (64, base_in), (16, 64), (64, 19), (64, 64), (3, 64)]
    got = [m.shape for m in mats]
    if got != want:
        raise ValueError(f"weight shapes {got} do not match the DNGPradianceField layout {want}")
    if mlp_precision == _lib.MLP_F32_HEAD16X2:          # fp32 sigma chain + fp16 fragments of the colour head, fp32-blob sized
        n = int(L.ced_packed_weight_floats(int(use_div_offsets), int(time_mode)))
        out = np.zeros((n,), np.float32)
        rc = L.ced_pack_field_weights_mixed(int(use_div_offsets), int(time_mode),
                                            *[m.ctypes.data_as(C.c_void_p) for m in mats], out.ctypes.data_as(C.c_void_p))
        _lib.check(rc, "pack_field_weights_mixed")
        return out
    if mlp_precision != _lib.MLP_F32:
        n = int(L.ced_packed_weight_words(int(use_div_offsets), int(time_mode), int(mlp_precision)))
        if n <= 0:
            raise ValueError(f"mlp_precision={mlp_precision}")
        out = np.zeros((n,), np.uint32)
        rc = L.ced_pack_field_weights_half_for(int(use_div_offsets), int(time_mode), int(mlp_precision), int(table_dtype),
                                               int(bool(temporal)), *[m.ctypes.data_as(C.c_void_p) for m in mats],
                                               out.ctypes.data_as(C.c_void_p))
        _lib.check(rc, "pack_field_weights_half_for")
        return out
    n = int(L.ced_packed_weight_floats(int(use_div_offsets), int(time_mode)))
    out = np.zeros((n,), np.float32)
    rc = L.ced_pack_field_weights(int(use_div_offsets), int(time_mode),
                                  *[m.ctypes.data_as(C.c_void_p) for m in mats], out.ctypes.data_as(C.c_void_p))
    _lib.check(rc, "pack_field_weights")
    return out


# ----------------------------------------------------------------------------------------------
# marching
# ----------------------------------------------------------------------------------------------
def ray_aabb_intersect(rays_o, rays_d, aabbs, near_plane=-float("inf"), far_plane=float("inf"),
                       miss_value=float("inf")):
    _chk(rays_o, torch.float32, "rays_o"); _chk(rays_d, torch.float32, "rays_d"); _chk(aabbs, torch.float32, "aabbs")
    assert rays_o.ndim == 2 and rays_o.shape[-1] == 3 and rays_o.shape == rays_d.shape
    assert aabbs.ndim == 2 and aabbs.shape[-1] == 6
    n, m = rays_o.shape[0], aabbs.shape[0]
    t_mins = torch.empty((n, m), device=rays_o.device, dtype=torch.float32)
    t_maxs = torch.empty_like(t_mins)
    hits = torch.empty((n, m), device=rays_o.device, dtype=torch.bool)
    rc = _lib.lib().ced_ray_aabb_intersect(n, _p(rays_o), _p(rays_d), m, _p(aabbs), near_plane, far_plane,
                                           miss_value, _p(t_mins), _p(t_maxs), _p(hits), _stream())
    _lib.check(rc, "ray_aabb_intersect")
    return t_mins, t_maxs, hits


def sort_intersections(t_mins, t_maxs):
    """ced_sort_intersections: (t_sorted [n, 2m] f32, t_indices [n, 2m] int64) = torch.sort(cat([t_mins, t_maxs], -1),
    stable=True) per ray, in one launch."""
    _chk(t_mins, torch.float32, "t_mins"); _chk(t_maxs, torch.float32, "t_maxs")
    assert t_mins.ndim == 2 and t_mins.shape == t_maxs.shape
    n, m = t_mins.shape
    t_sorted = torch.empty((n, 2 * m), device=t_mins.device, dtype=torch.float32)
    t_indices = torch.empty((n, 2 * m), device=t_mins.device, dtype=torch.int64)
    rc = _lib.lib().ced_sort_intersections(n, m, _p(t_mins), _p(t_maxs), _p(t_sorted), _p(t_indices), _stream())
    _lib.check(rc, "sort_intersections")
    return t_sorted, t_indices


def traverse_grids_raw(rays_o, rays_d, binaries, aabbs, near_planes, far_planes, step_size, cone_angle, limit,
                       rays_mask, t_sorted, t_indices, hits, mode, base=None, counts=None, t_starts=None,
                       t_ends=None, ray_indices=None, termination_planes=None, packed_info_out=None):
    L = _lib.lib()
    n = rays_o.shape[0]
    m, res = binaries.shape[0], binaries.shape[1]
    with profiling.span("traverse", n):
        rc = L.ced_traverse_grids(n, _p(rays_o), _p(rays_d), _p(_as_u8(binaries)), m, res, _p(aabbs), _p(near_planes),
                                  _p(far_planes), float(step_size), float(cone_angle), int(limit),
                                  _p(_as_u8(rays_mask)), _p(t_sorted), _p(t_indices), _p(_as_u8(hits)), int(mode),
                                  _p(base), _p(counts), _p(t_starts), _p(t_ends), _p(ray_indices),
                                  _p(termination_planes), _p(packed_info_out), _stream())
    _lib.check(rc, "traverse_grids")


# ----------------------------------------------------------------------------------------------
# hash grid / field
# ----------------------------------------------------------------------------------------------
def hash_encode(desc: _lib.HashDesc, x: torch.Tensor, t: Optional[torch.Tensor] = None) -> torch.Tensor:
    _chk(x, torch.float32, "x")
    assert x.ndim == 2 and x.shape[-1] == 3
    if t is not None:
        _chk(t, torch.float32, "t")
        assert t.numel() == x.shape[0]
    out = torch.empty((x.shape[0], 2 * desc.n_levels), device=x.device, dtype=torch.float32)
    rc = _lib.lib().ced_hash_encode(C.byref(desc), x.shape[0], _p(x), _p(t), _p(out), _stream())
    _lib.check(rc, "hash_encode")
    return out


def hash_encode_backward(desc: _lib.HashDesc, x: torch.Tensor, dy: torch.Tensor,
                         grad_table: Optional[torch.Tensor] = None, want_dx: bool = True, dx_scaled: bool = False,
                         want_table: bool = True):
    """ced_hash_encode_backward: (grad_table [E,2] fp32 -- accumulated into when given, else fresh --, dx [n,3] or None).
    want_table=False: the position gradient alone (grad_table returned as None)."""
    _chk(x, torch.float32, "x"); _chk(dy, torch.float32, "dy")
    n = x.shape[0]
    assert x.shape == (n, 3) and dy.numel() == n * 2 * desc.n_levels, f"{x.shape} v.s. {dy.shape}"
    assert want_table or want_dx
    if not want_table:
        grad_table = None
    elif grad_table is None:
        grad_table = torch.zeros((int(desc.total_entries), 2), device=x.device, dtype=torch.float32)
    else:
        _chk(grad_table, torch.float32, "grad_table")
        assert grad_table.shape == (int(desc.total_entries), 2)
    dx = torch.empty((n, 3), device=x.device, dtype=torch.float32) if want_dx else None
    rc = _lib.lib().ced_hash_encode_backward(C.byref(desc), n, _p(x), _p(dy), _p(grad_table), _p(dx), int(dx_scaled),
                                             _stream())
    _lib.check(rc, "hash_encode_backward")
    return grad_table, dx


def hash_encode_backward_temporal(desc: _lib.HashDesc, x: torch.Tensor, t: torch.Tensor, dy: torch.Tensor,
                                  grad_table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ced_hash_encode_backward_temporal (hash_encoder_inter.py:202-275): grad_table [E, 8] fp32, accumulated into when
    given.  The temporal encoder has a table gradient only (the reference's autograd function returns none for positions)."""
    _chk(x, torch.float32, "x"); _chk(dy, torch.float32, "dy"); _chk(t, torch.float32, "t")
    n = x.shape[0]
    assert desc.temporal, "not a temporal table"
    assert x.shape == (n, 3) and t.numel() == n and dy.numel() == n * 2 * desc.n_levels, f"{x.shape} {t.shape} {dy.shape}"
    if grad_table is None:
        grad_table = torch.zeros((int(desc.total_entries), 8), device=x.device, dtype=torch.float32)
    else:
        _chk(grad_table, torch.float32, "grad_table")
        assert grad_table.shape == (int(desc.total_entries), 8)
    rc = _lib.lib().ced_hash_encode_backward_temporal(C.byref(desc), n, _p(x), _p(t), _p(dy), _p(grad_table), _stream())
    _lib.check(rc, "hash_encode_backward_temporal")
    return grad_table


def _points(positions, t, who) -> int:
    """The rows of an op on positions [n,3] and t [n] (any shape of n elements), checked -> n."""
    _chk(positions, torch.float32, "positions"); _chk(t, torch.float32, "t")
    n = positions.shape[0]
    if positions.shape != (n, 3) or t.numel() != n:
        raise ValueError(f"{who}: positions [n,3], t [n]: got {list(positions.shape)}, {list(t.shape)}")
    return n


def _ray_samples(rays_o, rays_d, ray_indices, t_starts, t_ends, timestamps, t_per_ray):
    """The samples of a ray batch, checked -> (n, their ctypes arguments in the C order: rays_o .. t_per_ray)."""
    _chk(rays_o, torch.float32, "rays_o"); _chk(rays_d, torch.float32, "rays_d")
    _chk(ray_indices, torch.int64, "ray_indices")
    _chk(t_starts, torch.float32, "t_starts"); _chk(t_ends, torch.float32, "t_ends")
    _chk(timestamps, torch.float32, "timestamps")
    n = ray_indices.shape[0]
    if t_starts.shape != (n,) or t_ends.shape != (n,):
        raise ValueError(f"t_starts [n], t_ends [n] for ray_indices [n]: got {list(t_starts.shape)}, {list(t_ends.shape)}, "
                         f"{list(ray_indices.shape)}")
    if t_per_ray and timestamps.numel() != rays_o.shape[0]:
        raise ValueError("per-ray timestamps must have one entry per ray")
    return n, (_p(rays_o), _p(rays_d), _p(ray_indices), _p(t_starts), _p(t_ends), _p(timestamps), int(bool(t_per_ray)))


def _outputs(spec, n, dev, want, out, who):
    """The output buffers of an op, one per (name, trailing shape, dtype) of spec, None where not computed: fresh ones where
    `want` says so, or the given `out` buffers, checked."""
    if out is None and len(want) != len(spec):
        raise ValueError(f"{who}: want= takes one flag per output {tuple(name for name, _, _ in spec)}")
    outs = list(out) if out is not None else [torch.empty((n,) + shape, device=dev, dtype=dtype) if w else None
                                              for (_, shape, dtype), w in zip(spec, want)]
    if len(outs) != len(spec) or all(o is None for o in outs):
        raise ValueError(f"{who}: no output requested")
    if out is not None:
        for i, (o, (_, shape, dtype)) in enumerate(zip(outs, spec)):
            _chk(o, dtype, f"out[{i}]", allow_none=True)
            if o is not None and o.shape != (n,) + shape:
                raise ValueError(f"{who}: out[{i}] must be {[n, *shape]}, got {list(o.shape)}")
    return outs


_F32_3, _F32_1 = ((3,), torch.float32), ((), torch.float32)
_FORWARD = (("rgb", *_F32_3), ("sigma", *_F32_1), ("geo", (15,), torch.float32))
_MOVE = (("x_move", *_F32_3), ("move", *_F32_3), ("x_norm", *_F32_3), ("selector", (), torch.bool))


def field_forward(desc: _lib.FieldDesc, positions, t, directions=None, want_geo=False):
    n = _points(positions, t, "field_forward")
    if directions is not None:
        _chk(directions, torch.float32, "directions")
        assert directions.shape == positions.shape, f"{positions.shape} v.s. {directions.shape}"
    rgb, sigma, geo = _outputs(_FORWARD, n, positions.device, (directions is not None, True, want_geo), None, "field_forward")
    rc = _lib.lib().ced_field_forward(C.byref(desc), n, _p(positions), _p(t), _p(directions), _p(rgb), _p(sigma),
                                      _p(geo), _stream())
    _lib.check(rc, "field_forward")
    return rgb, sigma, geo


def field_forward_rays(desc: _lib.FieldDesc, rays_o, rays_d, ray_indices, t_starts, t_ends, timestamps,
                       t_per_ray: bool, want_rgb: bool, n_dev: Optional[torch.Tensor] = None):
    """n_dev: optional device int64 scalar; the kernel evaluates min(len(ray_indices), n_dev) samples."""
    n, rays = _ray_samples(rays_o, rays_d, ray_indices, t_starts, t_ends, timestamps, t_per_ray)
    rgb, sigma = _outputs(_FORWARD[:2], n, rays_o.device, (want_rgb, True), None, "field_forward_rays")
    with profiling.span("field", n):
        rc = _lib.lib().ced_field_forward_rays(C.byref(desc), n, _p(n_dev), *rays, int(bool(want_rgb)), _p(rgb), _p(sigma),
                                               _stream())
    _lib.check(rc, "field_forward_rays")
    return rgb, sigma


def field_move(desc: _lib.FieldDesc, positions, t, want=(True, True, True, True)):
    """ced_field_move: query_move plus the normalisation that follows it.  want = which of (x_move [n,3], move [n,3],
    x_norm [n,3], selector [n] bool) to compute; the others come back as None."""
    n = _points(positions, t, "field_move")
    x_move, move, x_norm, sel = _outputs(_MOVE, n, positions.device, want, None, "field_move")
    rc = _lib.lib().ced_field_move(C.byref(desc), n, _p(positions), _p(t), _p(x_move), _p(move), _p(x_norm),
                                   _p(_as_u8(sel)), _stream())
    _lib.check(rc, "field_move")
    return x_move, move, x_norm, sel


def field_move_rays(desc: _lib.FieldDesc, rays_o, rays_d, ray_indices, t_starts, t_ends, timestamps, t_per_ray: bool,
                    want_x_norm: bool = False, n_dev: Optional[torch.Tensor] = None, out=None):
    """ced_field_move_rays: (move [n,3], x_norm [n,3] or None) at the sample positions of `field_forward_rays`.
    n_dev as there; out = (move, x_norm) buffers to write into instead of fresh ones."""
    n, rays = _ray_samples(rays_o, rays_d, ray_indices, t_starts, t_ends, timestamps, t_per_ray)
    move, x_norm = _outputs(_MOVE[1:3], n, rays_o.device, (True, want_x_norm), out, "field_move_rays")
    rc = _lib.lib().ced_field_move_rays(C.byref(desc), n, _p(n_dev), *rays, _p(move), _p(x_norm), _stream())
    _lib.check(rc, "field_move_rays")
    return move, x_norm


MAX_SOLVE_ITERS = 1024                            # ced_field_move_inverse / ced_field_track: 1 <= max_iters <= 1024


def check_solve(max_iters, tol):
    """(max_iters, tol) of the fixed-point solve as (int, float), or ValueError: an int in 1 .. 1024, a number >= 0."""
    if isinstance(max_iters, bool) or not isinstance(max_iters, (int, np.integer)) or not 1 <= int(max_iters) <= MAX_SOLVE_ITERS:
        raise ValueError(f"max_iters must be an int in 1 .. {MAX_SOLVE_ITERS}, got {max_iters!r}")
    try:
        tol_f = float(tol)
    except (TypeError, ValueError):
        raise ValueError(f"tol must be a number >= 0, got {tol!r}") from None
    if not tol_f >= 0.0:                          # refuses a NaN too
        raise ValueError(f"tol must be a number >= 0, got {tol!r}")
    return int(max_iters), tol_f


SOLVE_METHODS = ("fixed_point", "newton")        # how the warp's inverse is solved


def check_method(method) -> str:
    """`method` of the inverse solvers, or ValueError."""
    if method not in SOLVE_METHODS:
        raise ValueError(f"method must be one of {SOLVE_METHODS}, got {method!r}")
    return method


def _move_inverse(entry: str, desc, target, t, init, max_iters, tol):
    max_iters, tol = check_solve(max_iters, tol)
    _chk(target, torch.float32, "target"); _chk(t, torch.float32, "t"); _chk(init, torch.float32, "init", allow_none=True)
    n = target.shape[0]
    if target.shape != (n, 3) or t.numel() != n or (init is not None and init.shape != (n, 3)):
        raise ValueError(f"target [n,3], t [n], init [n,3]: got {list(target.shape)}, {list(t.shape)}, "
                         f"{None if init is None else list(init.shape)}")
    dev = target.device
    x = torch.empty((n, 3), device=dev, dtype=torch.float32)
    step = torch.empty((n,), device=dev, dtype=torch.float32)
    evals = torch.empty((n,), device=dev, dtype=torch.int32)
    rc = getattr(_lib.lib(), "ced_" + entry)(C.byref(desc), n, _p(target), _p(t), _p(init), max_iters, tol, _p(x), _p(step),
                                             _p(evals), _stream())
    _lib.check(rc, entry)
    return x, step, evals


def _track(entry: str, desc, target, times, init, max_iters, tol):
    max_iters, tol = check_solve(max_iters, tol)
    _chk(target, torch.float32, "target"); _chk(times, torch.float32, "times")
    _chk(init, torch.float32, "init", allow_none=True)
    p, nt = target.shape[0], times.shape[0]
    if target.shape != (p, 3) or times.shape != (nt,) or (init is not None and init.shape != (p, 3)):
        raise ValueError(f"target [P,3], times [T], init [P,3]: got {list(target.shape)}, {list(times.shape)}, "
                         f"{None if init is None else list(init.shape)}")
    dev = target.device
    x = torch.empty((nt, p, 3), device=dev, dtype=torch.float32)
    step = torch.empty((nt, p), device=dev, dtype=torch.float32)
    evals = torch.empty((nt, p), device=dev, dtype=torch.int32)
    rc = getattr(_lib.lib(), "ced_" + entry)(C.byref(desc), p, nt, _p(target), _p(times), _p(init), max_iters, tol, _p(x),
                                             _p(step), _p(evals), _stream())
    _lib.check(rc, entry)
    return x, step, evals


def field_move_inverse(desc: _lib.FieldDesc, target, t, init=None, max_iters: int = 32, tol: float = 1e-6):
    """ced_field_move_inverse: per row the solution x of x + move(x, t) = target by fixed-point iteration from init (or
    from target), at most max_iters evaluations, stopped at step <= tol.  target [n,3], t [n], init [n,3] or None ->
    (x [n,3], step [n], evals [n] int32); include/cednerf_hip.h states the iteration."""
    return _move_inverse("field_move_inverse", desc, target, t, init, max_iters, tol)


def field_track(desc: _lib.FieldDesc, target, times, init=None, max_iters: int = 32, tol: float = 1e-6):
    """ced_field_track: `field_move_inverse` for every (time, point) pair without expanding either input.  target [P,3],
    times [T], init [P,3] or None (shared by all times) -> (x [T,P,3], step [T,P], evals [T,P] int32), each row with
    the bits of `field_move_inverse` on the expanded rows."""
    return _track("field_track", desc, target, times, init, max_iters, tol)


def field_move_jacobian(desc: _lib.FieldDesc, positions, t, want=(True, True)):
    """ced_field_move_jacobian: (move [n,3], jac [n,3,4]) at positions [n,3], t [n], from one launch.  jac[r, a, b] =
    d move_a / d (x, y, z, t)_b by forward mode through the motion network in desc's mlp_precision; `move` has
    `field_move`'s bits.  want = which of the two to compute; the other comes back as None."""
    n = _points(positions, t, "field_move_jacobian")
    move, jac = _outputs((_MOVE[1], ("jac", (3, 4), torch.float32)), n, positions.device, want, None, "field_move_jacobian")
    rc = _lib.lib().ced_field_move_jacobian(C.byref(desc), n, _p(positions), _p(t), _p(move), _p(jac), _stream())
    _lib.check(rc, "field_move_jacobian")
    return move, jac


VELOCITY_OUTPUTS = ("velocity", "det", "valid")   # ced_field_velocity's outputs, in `want=` order
_VELOCITY = (("velocity", *_F32_3), ("det", *_F32_1), ("valid", (), torch.bool))


def field_velocity(desc: _lib.FieldDesc, positions, t, want=(True, True, True)):
    """ced_field_velocity: (velocity [n,3], det [n], valid [n] bool) at positions [n,3], t [n], from one launch: the
    velocity v = -(I + J_x)^-1 d move / dt of the material point that sits there, J being `field_move_jacobian`'s (its
    bits), det = det(I + J_x), valid = det >= 2^-20 and v finite; v is 0 where not valid (include/cednerf_hip.h states every
    operation).  want = which of the three to compute; the others come back as None."""
    n = _points(positions, t, "field_velocity")
    v, det, valid = _outputs(_VELOCITY, n, positions.device, want, None, "field_velocity")
    rc = _lib.lib().ced_field_velocity(C.byref(desc), n, _p(positions), _p(t), _p(v), _p(det), _p(_as_u8(valid)), _stream())
    _lib.check(rc, "field_velocity")
    return v, det, valid


def field_velocity_rays(desc: _lib.FieldDesc, rays_o, rays_d, ray_indices, t_starts, t_ends, timestamps, t_per_ray: bool,
                        want=(True, True, True), n_dev: Optional[torch.Tensor] = None, out=None):
    """ced_field_velocity_rays: `field_velocity` at the sample positions of `field_forward_rays`.  n_dev as there; out =
    the three buffers (or None each) to write into instead of fresh ones, which then decides what is computed."""
    n, rays = _ray_samples(rays_o, rays_d, ray_indices, t_starts, t_ends, timestamps, t_per_ray)
    v, det, valid = _outputs(_VELOCITY, n, rays_o.device, want, out, "field_velocity_rays")
    rc = _lib.lib().ced_field_velocity_rays(C.byref(desc), n, _p(n_dev), *rays, _p(v), _p(det), _p(_as_u8(valid)), _stream())
    _lib.check(rc, "field_velocity_rays")
    return v, det, valid


GRADIENT_OUTPUTS = ("sigma", "grad", "dlog", "dlog_canonical")   # ced_field_density_gradient's outputs, in `want=` order
_GRADIENT = (("sigma", *_F32_1), ("grad", *_F32_3), ("dlog", *_F32_3), ("dlog_canonical", *_F32_3))
EXP15 = float(np.float32(np.exp(15.0)))                             # trunc_exp's backward clamps there (3269017.25)


def field_density_gradient(desc: _lib.FieldDesc, positions, t, want=(True, True, True, True)):
    """ced_field_density_gradient: (sigma [n], grad [n,3], dlog [n,3], dlog_canonical [n,3]) at positions [n,3], t [n],
    from one launch.  sigma has `field_forward`'s bits; dlog_canonical is the gradient of the pre-activation density with
    respect to the canonical point x + move(x, t), dlog = (I + J_x)^T dlog_canonical with respect to x, grad =
    min(sigma, e^15) * dlog; all zero outside the box (include/cednerf_hip.h states every operation).  want = which of
    the four to compute; the others come back as None."""
    n = _points(positions, t, "field_density_gradient")
    outs = _outputs(_GRADIENT, n, positions.device, want, None, "field_density_gradient")
    rc = _lib.lib().ced_field_density_gradient(C.byref(desc), n, _p(positions), _p(t), *[_p(o) for o in outs], _stream())
    _lib.check(rc, "field_density_gradient")
    return tuple(outs)


def field_density_gradient_rays(desc: _lib.FieldDesc, rays_o, rays_d, ray_indices, t_starts, t_ends, timestamps,
                                t_per_ray: bool, want=(True, True, True, True), n_dev: Optional[torch.Tensor] = None,
                                out=None):
    """ced_field_density_gradient_rays: `field_density_gradient` at the sample positions of `field_forward_rays`.  n_dev
    as there; out = the four buffers (or None each) to write into instead of fresh ones, which then decides what is
    computed."""
    n, rays = _ray_samples(rays_o, rays_d, ray_indices, t_starts, t_ends, timestamps, t_per_ray)
    outs = _outputs(_GRADIENT, n, rays_o.device, want, out, "field_density_gradient_rays")
    rc = _lib.lib().ced_field_density_gradient_rays(C.byref(desc), n, _p(n_dev), *rays, *[_p(o) for o in outs], _stream())
    _lib.check(rc, "field_density_gradient_rays")
    return tuple(outs)


def unit_or_zero(v: torch.Tensor) -> torch.Tensor:
    """v / |v| along the last axis, 0 where v is 0 (a normal where the field has a slope, none where it has not)."""
    length = v.norm(dim=-1, keepdim=True)
    return torch.where(length > 0, v / length, torch.zeros_like(v))


def field_move_inverse_newton(desc: _lib.FieldDesc, target, t, init=None, max_iters: int = 32, tol: float = 1e-6):
    """ced_field_move_inverse_newton: `field_move_inverse`'s arguments and outputs, solved by Newton's method on
    `field_move_jacobian` (include/cednerf_hip.h states the iteration).  `step` is the max-norm residual
    |x + move(x, t) - target| of the returned x; a row has converged iff step <= tol."""
    return _move_inverse("field_move_inverse_newton", desc, target, t, init, max_iters, tol)


def field_track_newton(desc: _lib.FieldDesc, target, times, init=None, max_iters: int = 32, tol: float = 1e-6):
    """ced_field_track_newton: `field_track`'s broadcast on the Newton iteration, each row with the bits of
    `field_move_inverse_newton` on the expanded rows."""
    return _track("field_track_newton", desc, target, times, init, max_iters, tol)


def warp_gradient(jac: torch.Tensor):
    """The 3 x 3 algebra of the warp's derivative, shared by the velocity and the moving normals: from jac [..., 3, 4]
    (`field_move_jacobian`) the deformation gradient A = I + jac[..., :3] [..., 3, 3], its inverse by the adjugate and
    its determinant [...], in jac's dtype.  Where det is 0 the inverse is not finite."""
    A = jac[..., :3] + torch.eye(3, device=jac.device, dtype=jac.dtype)
    rows = [torch.linalg.cross(A[..., (a + 1) % 3, :], A[..., (a + 2) % 3, :], dim=-1) for a in range(3)]
    cof = torch.stack(rows, -2)                                          # cofactors: cof[a] = A[a+1] x A[a+2]
    det = (A[..., 0, :] * cof[..., 0, :]).sum(-1)
    return A, cof.transpose(-1, -2) / det[..., None, None], det


def field_rgb(desc: _lib.FieldDesc, directions, embedding, apply_act: bool = True):
    """ced_field_rgb: mlp_head on [SH(directions), embedding [n,15]] -> rgb [n,3] (sigmoid iff apply_act)."""
    _chk(directions, torch.float32, "directions"); _chk(embedding, torch.float32, "embedding")
    n = directions.shape[0]
    assert directions.shape == (n, 3) and embedding.shape == (n, 15), f"{directions.shape} v.s. {embedding.shape}"
    rgb = torch.empty((n, 3), device=directions.device, dtype=torch.float32)
    rc = _lib.lib().ced_field_rgb(C.byref(desc), n, _p(directions), _p(embedding), int(bool(apply_act)), _p(rgb), _stream())
    _lib.check(rc, "field_rgb")
    return rgb


def field_rgb_bcast(desc: _lib.FieldDesc, directions, embedding, apply_act: bool = True):
    """ced_field_rgb_bcast: mlp_head on every (embedding [m,15], direction [d,3]) pair -> rgb [m,d,3], neither input
    expanded in memory; each row has the bits of `field_rgb` on the expanded inputs."""
    _chk(directions, torch.float32, "directions"); _chk(embedding, torch.float32, "embedding")
    m, d = embedding.shape[0], directions.shape[0]
    assert directions.shape == (d, 3) and embedding.shape == (m, 15), f"{directions.shape} v.s. {embedding.shape}"
    rgb = torch.empty((m, d, 3), device=embedding.device, dtype=torch.float32)
    rc = _lib.lib().ced_field_rgb_bcast(C.byref(desc), m, d, _p(directions), _p(embedding), int(bool(apply_act)), _p(rgb),
                                        _stream())
    _lib.check(rc, "field_rgb_bcast")
    return rgb


# ----------------------------------------------------------------------------------------------
# volume export (csrc/bake.hip)
# ----------------------------------------------------------------------------------------------
def _bake_workspace(n: int, dev):
    nbytes = int(_lib.lib().ced_bake_workspace_bytes(n))
    return torch.empty((nbytes // 8,), device=dev, dtype=torch.int64), nbytes


def bake_candidates(reso: int, center, radius: float, first_cell: int, n_cells: int, device, binaries=None, aabbs=None):
    """ced_bake_candidates on cells [first_cell, first_cell + n_cells) of the reso^3 grid over the cube
    [center - radius, center + radius]^3: (index [n] int64 ascending, xyz [n,3]) of the cells an occupancy grid
    (binaries [levels,R,R,R] bool, aabbs [levels,6]) marks -- all of them without one.  With a grid the count is read
    back once, so the outputs are allocated at their size."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise NotImplementedError(f"Only support cuda inputs (device is {dev}).")
    _check_current_device(dev.index, "device")
    levels = res = 0
    if binaries is not None:
        binaries = _chk(_as_u8(binaries), torch.uint8, "binaries"); _chk(aabbs, torch.float32, "aabbs")
        levels, res = binaries.shape[0], binaries.shape[1]
        assert binaries.shape == (levels, res, res, res) and aabbs.shape == (levels, 6), (binaries.shape, aabbs.shape)
    c3 = (C.c_float * 3)(*[float(v) for v in center])
    ws, ws_bytes = _bake_workspace(n_cells, dev)
    count = torch.empty((1,), device=dev, dtype=torch.int64)

    def call(capacity, index, xyz):
        rc = _lib.lib().ced_bake_candidates(int(reso), c3, float(radius), int(first_cell), int(n_cells), _p(binaries),
                                            _p(aabbs), levels, res, capacity, _p(index), _p(xyz), _p(count), _p(ws),
                                            ws_bytes, _stream())
        _lib.check(rc, "bake_candidates")

    n = int(n_cells)
    if binaries is not None:
        call(0, None, None)
        n = int(count.item())
    index = torch.empty((n,), device=dev, dtype=torch.int64)
    xyz = torch.empty((n, 3), device=dev, dtype=torch.float32)
    if n > 0:
        call(n, index, xyz)
    return index, xyz


def bake_select(index, xyz, sigma, embedding, sigma_thresh: float):
    """ced_bake_select: the rows with sigma >= sigma_thresh (never a NaN), in their order: (index [m], xyz [m,3],
    sigma [m], embedding [m,15]).  The count is read back once, so the outputs are allocated at their size."""
    _chk(index, torch.int64, "index"); _chk(xyz, torch.float32, "xyz")
    _chk(sigma, torch.float32, "sigma"); _chk(embedding, torch.float32, "embedding")
    n = index.shape[0]
    assert index.shape == (n,) and xyz.shape == (n, 3) and sigma.shape == (n,) and embedding.shape == (n, 15)
    dev = index.device
    ws, ws_bytes = _bake_workspace(n, dev)
    count = torch.empty((1,), device=dev, dtype=torch.int64)

    def call(capacity, outs):
        rc = _lib.lib().ced_bake_select(n, _p(index), _p(xyz), _p(sigma), _p(embedding), float(sigma_thresh), capacity,
                                        _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(outs[3]), _p(count), _p(ws), ws_bytes,
                                        _stream())
        _lib.check(rc, "bake_select")

    call(0, (None,) * 4)
    m = int(count.item())
    outs = (torch.empty((m,), device=dev, dtype=torch.int64), torch.empty((m, 3), device=dev, dtype=torch.float32),
            torch.empty((m,), device=dev, dtype=torch.float32), torch.empty((m, 15), device=dev, dtype=torch.float32))
    if m > 0:
        call(m, outs)
    return outs


# ----------------------------------------------------------------------------------------------
# mesh export (csrc/mesh.hip)
# ----------------------------------------------------------------------------------------------
def mesh_surface_nets(lattice, thresh: float, center, radius: float):
    """ced_mesh_vertices + ced_mesh_faces: naive surface nets (include/cednerf_hip.h has the definition) of the density
    lattice [reso,reso,reso] f32 -- node (ix,iy,iz) at the volume export's cell centre -- at the iso-value thresh:
    (vertices [V,3] f32, normals [V,3] f32, cube [V] int64 ascending cube ids, faces [F,3] int32).  Each count is read
    back once, so the outputs are allocated at their size."""
    _chk(lattice, torch.float32, "lattice")
    reso = lattice.shape[0] if lattice.dim() == 3 else 0
    if lattice.dim() != 3 or lattice.shape != (reso, reso, reso) or not 1 <= reso <= 512:
        raise ValueError(f"lattice must be [reso, reso, reso] with reso in 1 .. 512, got {list(lattice.shape)}")
    dev = lattice.device
    L = _lib.lib()
    c3 = (C.c_float * 3)(*[float(v) for v in center])
    ws_bytes = int(L.ced_mesh_workspace_bytes(reso))
    ws = torch.empty((ws_bytes // 8,), device=dev, dtype=torch.int64)
    count = torch.empty((1,), device=dev, dtype=torch.int64)

    def vertices_call(capacity, vertices, normals, cube):
        rc = L.ced_mesh_vertices(reso, c3, float(radius), _p(lattice), float(thresh), capacity, _p(vertices), _p(normals),
                                 _p(cube), _p(count), _p(ws), ws_bytes, _stream())
        _lib.check(rc, "mesh_vertices")

    vertices_call(0, None, None, None)
    v = int(count.item())
    vertices = torch.empty((v, 3), device=dev, dtype=torch.float32)
    normals = torch.empty((v, 3), device=dev, dtype=torch.float32)
    cube = torch.empty((v,), device=dev, dtype=torch.int64)
    if v > 0:
        vertices_call(v, vertices, normals, cube)

    def faces_call(capacity, faces):
        rc = L.ced_mesh_faces(reso, _p(lattice), float(thresh), _p(cube), v, capacity, _p(faces), _p(count), _p(ws),
                              ws_bytes, _stream())
        _lib.check(rc, "mesh_faces")

    faces_call(0, None)
    quads = int(count.item())
    faces = torch.empty((2 * quads, 3), device=dev, dtype=torch.int32)
    if quads > 0:
        faces_call(quads, faces)
    return vertices, normals, cube, faces


# ----------------------------------------------------------------------------------------------
# compositing
# ----------------------------------------------------------------------------------------------
def render_weights(packed_info, t_starts, t_ends, sigmas, prefix_trans=None, want=(True, True, True)):
    _chk(packed_info, torch.int64, "packed_info"); _chk(t_starts, torch.float32, "t_starts")
    _chk(t_ends, torch.float32, "t_ends"); _chk(sigmas, torch.float32, "sigmas")
    _chk(prefix_trans, torch.float32, "prefix_trans", allow_none=True)
    outs = [torch.empty_like(t_starts) if w else None for w in want]
    if t_starts.shape[0] == 0:
        return tuple(outs)
    rc = _lib.lib().ced_render_weights(packed_info.shape[0], _p(packed_info), _p(t_starts), _p(t_ends), _p(sigmas),
                                       _p(prefix_trans), _p(outs[0]), _p(outs[1]), _p(outs[2]), _stream())
    _lib.check(rc, "render_weights")
    return tuple(outs)


def accumulate_along_rays_(packed_info, weights, values, outputs):
    _chk(packed_info, torch.int64, "packed_info"); _chk(weights, torch.float32, "weights")
    _chk(values, torch.float32, "values", allow_none=True); _chk(outputs, torch.float32, "outputs")
    n_rays = packed_info.shape[0]
    C_ = outputs.shape[-1]
    assert outputs.shape == (n_rays, C_)
    if values is not None:
        assert values.shape == (weights.shape[0], C_), f"Invalid shapes: {values.shape} vs {weights.shape}"
    if weights.shape[0] == 0:
        return outputs
    rc = _lib.lib().ced_accumulate_along_rays(n_rays, _p(packed_info), _p(weights), _p(values), C_, _p(outputs),
                                              _stream())
    _lib.check(rc, "accumulate_along_rays")
    return outputs


def reduce_along_rays(ray_indices, values, n_rays: int, weights=None, mean: bool = False):
    """ced_reduce_along_rays: out [n_rays, C] = sum (or torch's include_self mean) of weights * values per ray."""
    _chk(ray_indices, torch.int64, "ray_indices"); _chk(values, torch.float32, "values")
    _chk(weights, torch.float32, "weights", allow_none=True)
    n, c = values.shape
    wc = 0 if weights is None else weights.shape[1]
    out = torch.empty((n_rays, c), device=values.device, dtype=torch.float32)
    counts = torch.empty((n_rays,), device=values.device, dtype=torch.int32) if mean else None
    rc = _lib.lib().ced_reduce_along_rays(n, _p(ray_indices), _p(values), c, _p(weights), wc, n_rays, int(bool(mean)), _p(out),
                                          _p(counts), _stream())
    _lib.check(rc, "reduce_along_rays")
    return out


def visibility_mask(packed_info, t_starts, t_ends, sigmas, early_stop_eps, alpha_thre):
    _chk(packed_info, torch.int64, "packed_info")
    mask = torch.empty(t_starts.shape, device=t_starts.device, dtype=torch.bool)
    if t_starts.shape[0] == 0:
        return mask
    rc = _lib.lib().ced_visibility_mask(packed_info.shape[0], _p(packed_info), _p(t_starts), _p(t_ends), _p(sigmas),
                                        float(early_stop_eps), float(alpha_thre), _p(mask), _stream())
    _lib.check(rc, "visibility_mask")
    return mask


def composite_backward(packed_info, t_starts, t_ends, sigmas, rgbs, d_color, d_opacity=None, d_depth=None):
    """ced_composite_backward: (d_sigmas [S], d_rgbs [S,3]) of the un-normalised colors / opacities / depths."""
    _chk(packed_info, torch.int64, "packed_info"); _chk(sigmas, torch.float32, "sigmas"); _chk(rgbs, torch.float32, "rgbs")
    _chk(t_starts, torch.float32, "t_starts"); _chk(t_ends, torch.float32, "t_ends"); _chk(d_color, torch.float32, "d_color")
    n_rays, S = packed_info.shape[0], sigmas.shape[0]
    assert rgbs.shape == (S, 3) and d_color.shape == (n_rays, 3)
    d_sig = torch.zeros((S,), device=sigmas.device, dtype=torch.float32)
    d_rgb = torch.zeros((S, 3), device=sigmas.device, dtype=torch.float32)
    if S == 0 or n_rays == 0:
        return d_sig, d_rgb
    for t, nm in ((d_opacity, "d_opacity"), (d_depth, "d_depth")):
        if t is not None:
            _chk(t, torch.float32, nm)
            assert t.numel() == n_rays
    rc = _lib.lib().ced_composite_backward(n_rays, _p(packed_info), _p(t_starts), _p(t_ends), _p(sigmas), _p(rgbs),
                                           _p(d_color), _p(d_opacity), _p(d_depth), _p(d_sig), _p(d_rgb), _stream())
    _lib.check(rc, "composite_backward")
    return d_sig, d_rgb


def _distortion_workspace(n_rays: int, S: int, density: bool, dev) -> torch.Tensor:
    n = _lib.lib().ced_distortion_workspace_bytes(n_rays, S, int(density))
    _lib.check(0 if n >= 0 else int(n), "distortion_workspace_bytes")
    return torch.empty(((n + 7) // 8,), device=dev, dtype=torch.float64)      # 8-byte aligned


def distortion_loss(packed_info, weights, t_starts, t_ends, want_grad: bool = True):
    """ced_distortion_loss: (loss [], inv_norm [], ray_loss [n_rays], dL/dw [S] unscaled or None), all on the device."""
    _chk(packed_info, torch.int64, "packed_info"); _chk(weights, torch.float32, "weights")
    _chk(t_starts, torch.float32, "t_starts"); _chk(t_ends, torch.float32, "t_ends")
    n_rays, S = packed_info.shape[0], weights.shape[0]
    assert weights.dim() == 1 and t_starts.shape == (S,) and t_ends.shape == (S,), "distortion_loss: [S] samples"
    dev = weights.device
    loss, inv_norm = torch.empty((), device=dev), torch.empty((), device=dev)
    ray_loss = torch.empty((n_rays,), device=dev)
    grad = torch.zeros((S,), device=dev) if want_grad else None
    ws = _distortion_workspace(n_rays, S, False, dev)
    rc = _lib.lib().ced_distortion_loss(n_rays, S, _p(packed_info), _p(weights), _p(t_starts), _p(t_ends), _p(ray_loss),
                                        _p(grad), _p(ws), _p(loss), _p(inv_norm), _stream())
    _lib.check(rc, "distortion_loss")
    return loss, inv_norm, ray_loss, grad


def distortion_loss_density(packed_info, sigmas, t_starts, t_ends, want_grad: bool = True):
    """ced_distortion_loss_density: (loss [], inv_norm [], ray_loss [n_rays], dL/dsigma [S] unscaled or None); the
    weights are those of render_weights(packed_info, t_starts, t_ends, sigmas) bit for bit."""
    _chk(packed_info, torch.int64, "packed_info"); _chk(sigmas, torch.float32, "sigmas")
    _chk(t_starts, torch.float32, "t_starts"); _chk(t_ends, torch.float32, "t_ends")
    n_rays, S = packed_info.shape[0], sigmas.shape[0]
    assert sigmas.dim() == 1 and t_starts.shape == (S,) and t_ends.shape == (S,), "distortion_loss_density: [S] samples"
    dev = sigmas.device
    loss, inv_norm = torch.empty((), device=dev), torch.empty((), device=dev)
    ray_loss = torch.empty((n_rays,), device=dev)
    d_sig = torch.zeros((S,), device=dev) if want_grad else None
    ws = _distortion_workspace(n_rays, S, want_grad, dev)
    rc = _lib.lib().ced_distortion_loss_density(n_rays, S, _p(packed_info), _p(sigmas), _p(t_starts), _p(t_ends), _p(ray_loss),
                                                _p(d_sig), _p(ws), _p(loss), _p(inv_norm), _stream())
    _lib.check(rc, "distortion_loss_density")
    return loss, inv_norm, ray_loss, d_sig


def _image_batch(t, name: str):
    """A [N,C,H,W] float32 CUDA tensor of any strides (read in place through them)."""
    if not t.is_cuda:
        raise NotImplementedError(f"Only support cuda inputs ({name} is on {t.device}).")
    _check_current_device(t.device.index, name)
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be torch.float32, got {t.dtype}")
    if t.dim() != 4:
        raise ValueError(f"{name} must be [N,C,H,W], got shape {tuple(t.shape)}")
    return (C.c_int64 * 4)(*t.stride())


def ssim(X, Y, win, levels: int, weights=None, data_range: float = 1.0, K=(0.01, 0.03), nonnegative: bool = False,
         want_mean: bool = True, want_mse: bool = False, want_levels: bool = False):
    """ced_ssim on two [N,C,H,W] float32 CUDA tensors (any strides): (per_image [N] f32, mean [] f32 or None,
    mse [N] f64 or None, level_means [levels,N,C,2] f64 or None), all on the device, no host synchronisation.
    win: the fp32 window (sequence of win_size floats); weights: None = single-scale SSIM (levels 1), else the MS-SSIM
    level weights (levels of them); levels 0 = the MSE alone."""
    sx, sy = _image_batch(X, "X"), _image_batch(Y, "Y")
    if tuple(X.shape) != tuple(Y.shape):
        raise ValueError(f"X and Y must have the same shape, got {tuple(X.shape)} and {tuple(Y.shape)}")
    N, Ch, H, W = X.shape
    win_arr = None if win is None else (C.c_float * len(win))(*[float(v) for v in win])
    w_arr = None if weights is None else (C.c_float * len(weights))(*[float(v) for v in weights])
    win_size = len(win) if win is not None else 1
    L = _lib.lib()
    nbytes = L.ced_ssim_workspace_bytes(N, Ch, H, W, win_size, levels)
    _lib.check(0 if nbytes >= 0 else int(nbytes), "ssim_workspace_bytes")
    dev = X.device
    ws = torch.empty(((nbytes + 7) // 8,), device=dev, dtype=torch.float64)      # 8-byte aligned
    per_image = torch.empty((N,), device=dev) if levels > 0 else None
    mean = torch.empty((), device=dev) if want_mean and levels > 0 else None
    mse = torch.empty((N,), device=dev, dtype=torch.float64) if want_mse or levels == 0 else None
    lvl = torch.empty((levels, N, Ch, 2), device=dev, dtype=torch.float64) if want_levels and levels > 0 else None
    rc = L.ced_ssim(N, Ch, H, W, _p(X), sx, _p(Y), sy, float(data_range), float(K[0]), float(K[1]), win_size, win_arr,
                    levels, w_arr, int(bool(nonnegative)), _p(per_image), _p(mean), _p(mse), _p(lvl), _p(ws), _stream())
    _lib.check(rc, "ssim")
    return per_image, mean, mse, lvl


def frame_to_rgb8(rgb, flip_w: bool = True):
    """ced_frame_to_rgb8: [H,W,3] float colours -> [H,W,3] uint8 (x 255, truncated), flipped along the width as the
    reference's video frames are (train_real.py:556)."""
    _chk(rgb, torch.float32, "rgb")
    assert rgb.dim() == 3 and rgb.shape[2] == 3, "frame_to_rgb8: rgb [H,W,3]"
    out = torch.empty(rgb.shape, device=rgb.device, dtype=torch.uint8)
    _lib.check(_lib.lib().ced_frame_to_rgb8(rgb.shape[0], rgb.shape[1], _p(rgb), int(bool(flip_w)), _p(out), _stream()),
               "frame_to_rgb8")
    return out


def flow_to_rgb8(flow, max_mag: float, flip_w: bool = True):
    """ced_flow_to_rgb8: a flow image [H,W,2] as colour [H,W,3] uint8 on the HSV wheel: hue = the direction atan2(fy, fx),
    saturation = min(|f| / max_mag, 1), value 1 -- no flow white, max_mag along +x pure red -- converted and flipped as
    `frame_to_rgb8`; a pixel that is not finite is black (include/cednerf_hip.h states the formula)."""
    _chk(flow, torch.float32, "flow")
    if flow.dim() != 3 or flow.shape[2] != 2:
        raise ValueError(f"flow_to_rgb8: flow [H,W,2], got {list(flow.shape)}")
    max_mag = float(max_mag)
    if not max_mag > 0.0:
        raise ValueError(f"flow_to_rgb8: max_mag={max_mag!r} must be > 0")
    out = torch.empty((flow.shape[0], flow.shape[1], 3), device=flow.device, dtype=torch.uint8)
    _lib.check(_lib.lib().ced_flow_to_rgb8(flow.shape[0], flow.shape[1], _p(flow), max_mag, int(bool(flip_w)), _p(out),
                                           _stream()), "flow_to_rgb8")
    return out


def depth_to_u8(depth, flip_w: bool = True):
    """ced_depth_to_u8: [H,W] (or [H,W,1]) depths -> [H,W] uint8 of the min-max normalised image (depth2img of
    train_real.py:38-41 before cv2's colour-map lookup)."""
    _chk(depth, torch.float32, "depth")
    if depth.dim() == 3:
        assert depth.shape[2] == 1
        depth = depth[..., 0]
    assert depth.dim() == 2, "depth_to_u8: depth [H,W]"
    out = torch.empty(depth.shape, device=depth.device, dtype=torch.uint8)
    ws = torch.empty((2,), device=depth.device, dtype=torch.int32)
    _lib.check(_lib.lib().ced_depth_to_u8(depth.shape[0], depth.shape[1], _p(depth), int(bool(flip_w)), _p(out), _p(ws),
                                          _stream()), "depth_to_u8")
    return out


def scatter_pixels(dest, n_pixels: int, src_rgb, src_opacity, src_depth, want_rgb8_width: int = 0, flip_w: bool = True):
    """ced_scatter_pixels: rows (marching / gather order) -> raster images.  Sources are 2-D views whose last-dim
    slices may be strided (e.g. columns of the gathered [rows, 5] payload).  Returns (rgb [n,3], opacity [n,1],
    depth [n,1], rgb8 [n,3] uint8 or None)."""
    _chk(dest, torch.int64, "dest")
    n_rows = dest.shape[0]
    for nm, t in (("src_rgb", src_rgb), ("src_opacity", src_opacity), ("src_depth", src_depth)):
        assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[0] == n_rows and t.stride(1) == 1, nm
        _check_current_device(t.device.index, nm)
    dev = dest.device
    rgb = torch.empty((n_pixels, 3), device=dev, dtype=torch.float32)
    opacity = torch.empty((n_pixels, 1), device=dev, dtype=torch.float32)
    depth = torch.empty((n_pixels, 1), device=dev, dtype=torch.float32)
    rgb8 = torch.empty((n_pixels, 3), device=dev, dtype=torch.uint8) if want_rgb8_width else None
    rc = _lib.lib().ced_scatter_pixels(n_rows, _p(src_rgb), src_rgb.stride(0), _p(src_opacity), src_opacity.stride(0),
                                       _p(src_depth), src_depth.stride(0), _p(dest), n_pixels, _p(rgb), _p(opacity),
                                       _p(depth), _p(rgb8), int(want_rgb8_width), int(bool(flip_w)), _stream())
    _lib.check(rc, "scatter_pixels")
    return rgb, opacity, depth, rgb8


def linear(x, w, transpose_w: bool = False, relu: bool = False, mask=None):
    """ced_linear: y = x w^T (w [n_out, n_in]) or, transpose_w, y = x w (w [n_in, n_out]); optional ReLU on the result
    and optional mask (y *= mask > 0, the fused ReLU derivative of the layer below)."""
    _chk(x, torch.float32, "x"); _chk(w, torch.float32, "w"); _chk(mask, torch.float32, "mask", allow_none=True)
    assert x.dim() == 2 and w.dim() == 2
    n, n_in = x.shape
    n_out = w.shape[1] if transpose_w else w.shape[0]
    if mask is not None:
        assert mask.shape == (n, n_out), f"mask {tuple(mask.shape)} vs output {(n, n_out)}"
    y = torch.empty((n, n_out), device=x.device, dtype=torch.float32)
    rc = _lib.lib().ced_linear(n, _p(x), n_in, _p(w), w.shape[0], w.shape[1], int(bool(transpose_w)), n_out, int(bool(relu)),
                               _p(mask), _p(y), _stream())
    _lib.check(rc, "linear")
    return y


def mlp_chain(x, weights, backward: bool = False, masks=None, want=None, relu_last: bool = False):
    """ced_mlp_chain.  Forward: x [n, K0], weights [W_1 .. W_L] (W_l [N_l, N_{l-1}]) -> [a_1 .. a_L] (ReLU on all but the
    last).  Backward: x = dy [n, N_L], masks[l] = the forward input of layer l (None for no mask), want[l] = whether the
    gradient with respect to layer l's input is to be stored -> [g_0 .. g_{L-1}] (None where not wanted)."""
    _chk(x, torch.float32, "x")
    L = len(weights)
    assert x.dim() == 2 and 1 <= L <= 6
    for w in weights:
        _chk(w, torch.float32, "w")
    widths = [weights[0].shape[1]] + [w.shape[0] for w in weights]
    for l in range(1, L):
        assert weights[l].shape[1] == widths[l], "mlp_chain: layer widths do not chain"
    n = x.shape[0]
    dev = x.device
    if not backward:
        assert x.shape[1] == widths[0]
        outs = [torch.empty((n, widths[l + 1]), device=dev, dtype=torch.float32) for l in range(L)]
        mk = [None] * L
    else:
        assert x.shape[1] == widths[L]
        want = [True] * L if want is None else list(want)
        outs = [torch.empty((n, widths[l]), device=dev, dtype=torch.float32) if want[l] else None for l in range(L)]
        mk = [None] * L if masks is None else list(masks)
        for l in range(L):
            _chk(mk[l], torch.float32, "mask", allow_none=True)
            assert mk[l] is None or mk[l].shape == (n, widths[l])
    vp = lambda ts: (C.c_void_p * L)(*[(t.data_ptr() if t is not None and t.numel() > 0 else None) for t in ts])
    rc = _lib.lib().ced_mlp_chain(n, L, int(bool(backward)), _p(x), (C.c_int32 * (L + 1))(*widths), vp(weights), vp(outs),
                                  vp(mk), int(bool(relu_last)), _stream())
    _lib.check(rc, "mlp_chain")
    return outs


def mlp_backward_dw_supported(widths) -> bool:
    """Shapes ced_mlp_backward_dw handles: input <= 48, 1..3 hidden layers of 64, output <= 32."""
    L = len(widths) - 1
    return 2 <= L <= 4 and 1 <= widths[0] <= 48 and 1 <= widths[L] <= 32 and all(w == 64 for w in widths[1:L])


def mlp_backward_dw(dy, weights, acts, want_g0: bool):
    """ced_mlp_backward_dw: dy [n, N_L], weights [W_0 .. W_H], acts [x, a_1 .. a_H] (the forward's layer inputs) ->
    (g0 [n, K0] or None, [dW_0 .. dW_H])."""
    _chk(dy, torch.float32, "dy")
    L = len(weights)
    widths = [weights[0].shape[1]] + [w.shape[0] for w in weights]
    assert mlp_backward_dw_supported(widths) and len(acts) == L
    n, dev = dy.shape[0], dy.device
    for w, a, k in zip(weights, acts, widths):
        _chk(w, torch.float32, "w"); _chk(a, torch.float32, "act")
        assert a.shape == (n, k), f"{a.shape} v.s. {(n, k)}"
    assert dy.shape == (n, widths[L])
    total = sum(widths[l] * widths[l + 1] for l in range(L))
    dws = torch.empty((total,), device=dev, dtype=torch.float32)
    g0 = torch.empty((n, widths[0]), device=dev, dtype=torch.float32) if want_g0 else None
    wa = (C.c_int32 * (L + 1))(*widths)
    nbytes = int(_lib.lib().ced_mlp_backward_dw_workspace_bytes(n, L, wa))
    ws = torch.empty((max(nbytes, 4) // 4,), device=dev, dtype=torch.float32)
    vp = lambda ts: (C.c_void_p * L)(*[(t.data_ptr() if t.numel() > 0 else None) for t in ts])
    rc = _lib.lib().ced_mlp_backward_dw(n, L, _p(dy), wa, vp(weights), vp(acts), _p(g0), _p(dws), _p(ws), nbytes, _stream())
    _lib.check(rc, "mlp_backward_dw")
    out, o = [], 0
    for l in range(L):
        out.append(dws[o:o + widths[l] * widths[l + 1]].view(widths[l + 1], widths[l]))
        o += widths[l] * widths[l + 1]
    return g0, out


def train_inputs(n, rays_o=None, rays_d=None, ray_indices=None, t_starts=None, t_ends=None, timestamps=None,
                 positions=None, directions=None):
    """ced_train_inputs -> (pos [n,3], enc [n,32], sh [n,4], t [n]).  Rays mode (ray_indices given: int64 [n],
    timestamps per RAY) or explicit mode (positions / directions [n,3], timestamps per sample)."""
    ref = ray_indices if ray_indices is not None else positions
    dev = ref.device
    f32 = torch.float32
    for t_, nm in ((rays_o, "rays_o"), (rays_d, "rays_d"), (t_starts, "t_starts"), (t_ends, "t_ends"),
                   (timestamps, "timestamps"), (positions, "positions"), (directions, "directions")):
        _chk(t_, f32, nm, allow_none=True)
    _chk(ray_indices, torch.int64, "ray_indices", allow_none=True)
    pos = torch.empty((n, 3), device=dev, dtype=f32)
    enc = torch.empty((n, 32), device=dev, dtype=f32)
    sh = torch.empty((n, 4), device=dev, dtype=f32)
    t = torch.empty((n,), device=dev, dtype=f32)
    rc = _lib.lib().ced_train_inputs(n, _p(rays_o), _p(rays_d), _p(ray_indices), _p(t_starts), _p(t_ends), _p(timestamps),
                                     _p(positions), _p(directions), _p(pos), _p(enc), _p(sh), _p(t), _stream())
    _lib.check(rc, "train_inputs")
    return pos, enc, sh, t


def train_inputs_backward(n, rays_o=None, rays_d=None, ray_indices=None, t_starts=None, t_ends=None, timestamps=None,
                          positions=None, directions=None, packed_info=None, d_pos=None, d_enc=None, d_sh=None, d_t=None):
    """ced_train_inputs_backward: the forward's inputs and the gradients at its outputs (None = zero) ->
    rays mode (d_rays_o [R,3], d_rays_d [R,3], d_timestamps [R]), R = rays_o.shape[0], with packed_info [R, 2] int64 the
    (first sample, count) of the non-decreasing ray_indices; explicit mode (d_positions [n,3], d_directions [n,3],
    d_timestamps [n])."""
    rays = ray_indices is not None
    ref = rays_o if rays else positions
    dev, f32 = ref.device, torch.float32
    for t_, nm in ((rays_o, "rays_o"), (rays_d, "rays_d"), (t_starts, "t_starts"), (t_ends, "t_ends"),
                   (timestamps, "timestamps"), (positions, "positions"), (directions, "directions"), (d_pos, "d_pos"),
                   (d_enc, "d_enc"), (d_sh, "d_sh"), (d_t, "d_t")):
        _chk(t_, f32, nm, allow_none=True)
    _chk(ray_indices, torch.int64, "ray_indices", allow_none=True)
    _chk(packed_info, torch.int64, "packed_info", allow_none=True)
    for t_, shape in ((d_pos, (n, 3)), (d_enc, (n, 32)), (d_sh, (n, 4)), (d_t, (n,))):
        assert t_ is None or tuple(t_.shape) == shape, f"{tuple(t_.shape)} v.s. {shape}"
    if rays:
        rows = rays_o.shape[0]
        assert ray_indices.shape == (n,) and t_starts.shape == (n,) and t_ends.shape == (n,)
        assert rays_d.shape == (rows, 3) and timestamps.shape == (rows,) and tuple(packed_info.shape) == (rows, 2)
    else:
        rows = n
        assert positions.shape == (n, 3) and directions.shape == (n, 3) and timestamps.shape == (n,)
    if d_enc is not None and d_enc.data_ptr() % 16:
        d_enc = d_enc.clone()
    if d_sh is not None and d_sh.data_ptr() % 16:
        d_sh = d_sh.clone()
    if n == 0:                       # no sample: every row is zero (an empty ray_indices has no address to tell the mode by)
        return torch.zeros((rows, 3), device=dev, dtype=f32), torch.zeros((rows, 3), device=dev, dtype=f32), \
            torch.zeros((rows,), device=dev, dtype=f32)
    g_o = torch.empty((rows, 3), device=dev, dtype=f32)
    g_d = torch.empty((rows, 3), device=dev, dtype=f32)
    g_t = torch.empty((rows,), device=dev, dtype=f32)
    rc = _lib.lib().ced_train_inputs_backward(n, rows, _p(rays_o), _p(rays_d), _p(ray_indices), _p(t_starts), _p(t_ends),
                                              _p(timestamps), _p(positions), _p(directions), _p(packed_info), _p(d_pos),
                                              _p(d_enc), _p(d_sh), _p(d_t), _p(g_o), _p(g_d), _p(g_t), _stream())
    _lib.check(rc, "train_inputs_backward")
    return g_o, g_d, g_t


def train_warp(pos, mo, aabb6, moving_step: float, use_div_offsets: bool):
    """ced_train_warp -> (xn clamped [n,3], move [n,3], selector [n] as 0 / 1 floats).  aabb6: six python floats."""
    _chk(pos, torch.float32, "pos"); _chk(mo, torch.float32, "mo")
    n = pos.shape[0]
    xn, move = torch.empty_like(pos), torch.empty_like(pos)
    sel = torch.empty((n,), device=pos.device, dtype=torch.float32)
    rc = _lib.lib().ced_train_warp(n, _p(pos), _p(mo), mo.shape[1], int(bool(use_div_offsets)), float(moving_step),
                                   (C.c_float * 6)(*aabb6), _p(xn), _p(move), _p(sel), _stream())
    _lib.check(rc, "train_warp")
    return xn, move, sel


def train_warp_backward(pos, mo, aabb6, moving_step: float, use_div_offsets: bool, d_xn, d_move=None):
    _chk(pos, torch.float32, "pos"); _chk(mo, torch.float32, "mo"); _chk(d_xn, torch.float32, "d_xn")
    _chk(d_move, torch.float32, "d_move", allow_none=True)
    d_mo = torch.empty_like(mo)
    rc = _lib.lib().ced_train_warp_backward(pos.shape[0], _p(pos), _p(mo), mo.shape[1], int(bool(use_div_offsets)),
                                            float(moving_step), (C.c_float * 6)(*aabb6), _p(d_xn), _p(d_move), _p(d_mo),
                                            _stream())
    _lib.check(rc, "train_warp_backward")
    return d_mo


def train_warp_backward_pos(pos, mo, aabb6, moving_step: float, use_div_offsets: bool, d_xn):
    """ced_train_warp_backward_pos -> d_pos [n,3]."""
    _chk(pos, torch.float32, "pos"); _chk(mo, torch.float32, "mo"); _chk(d_xn, torch.float32, "d_xn")
    assert d_xn.shape == pos.shape
    d_pos = torch.empty_like(pos)
    rc = _lib.lib().ced_train_warp_backward_pos(pos.shape[0], _p(pos), _p(mo), mo.shape[1], int(bool(use_div_offsets)),
                                                float(moving_step), (C.c_float * 6)(*aabb6), _p(d_xn), _p(d_pos), _stream())
    _lib.check(rc, "train_warp_backward_pos")
    return d_pos


def train_head_in(bout, sh, selector):
    """ced_train_head_in -> (head_in [n,19], sigma [n])."""
    _chk(bout, torch.float32, "bout"); _chk(sh, torch.float32, "sh"); _chk(selector, torch.float32, "selector")
    assert bout.dim() == 2 and bout.shape[1] == 16 and sh.shape == (bout.shape[0], 4)
    n = bout.shape[0]
    head_in = torch.empty((n, 19), device=bout.device, dtype=torch.float32)
    sigma = torch.empty((n,), device=bout.device, dtype=torch.float32)
    rc = _lib.lib().ced_train_head_in(n, _p(bout), _p(sh), _p(selector), _p(head_in), _p(sigma), _stream())
    _lib.check(rc, "train_head_in")
    return head_in, sigma


def train_head_in_backward(bout, selector, d_head_in, d_sigma):
    _chk(bout, torch.float32, "bout"); _chk(selector, torch.float32, "selector")
    _chk(d_head_in, torch.float32, "d_head_in", allow_none=True); _chk(d_sigma, torch.float32, "d_sigma", allow_none=True)
    d_bout = torch.empty_like(bout)
    rc = _lib.lib().ced_train_head_in_backward(bout.shape[0], _p(bout), _p(selector), _p(d_head_in), _p(d_sigma), _p(d_bout),
                                               _stream())
    _lib.check(rc, "train_head_in_backward")
    return d_bout


def weight_grad(x, dy):
    """ced_weight_grad: dW [n_out, n_in] = dy^T x over the sample stream (x [S, n_in], dy [S, n_out], fp32)."""
    _chk(x, torch.float32, "x"); _chk(dy, torch.float32, "dy")
    assert x.dim() == 2 and dy.dim() == 2 and x.shape[0] == dy.shape[0], "weight_grad: x [S, n_in], dy [S, n_out]"
    n, n_in, n_out = x.shape[0], x.shape[1], dy.shape[1]
    if x.data_ptr() % 16:
        x = x.clone()
    if dy.data_ptr() % 16:
        dy = dy.clone()
    dw = torch.empty((n_out, n_in), device=x.device, dtype=torch.float32)
    nbytes = int(_lib.lib().ced_weight_grad_workspace_bytes(n, n_out, n_in))
    ws = torch.empty((max(nbytes, 4) // 4,), device=x.device, dtype=torch.float32)
    rc = _lib.lib().ced_weight_grad(n, _p(x), n_in, _p(dy), n_out, _p(dw), _p(ws), nbytes, _stream())
    _lib.check(rc, "weight_grad")
    return dw


def composite_prefix_(packed_info, t_starts, t_ends, sigmas, rgbs, rgb, opacity, depth):
    _chk(packed_info, torch.int64, "packed_info"); _chk(rgbs, torch.float32, "rgbs")
    for nm, t in (("rgb", rgb), ("opacity", opacity), ("depth", depth)):
        _chk(t, torch.float32, nm)
    if t_starts.shape[0] == 0:
        return
    with profiling.span("composite", t_starts.shape[0]):
        rc = _lib.lib().ced_composite_prefix(packed_info.shape[0], _p(packed_info), _p(t_starts), _p(t_ends),
                                             _p(sigmas), _p(rgbs), _p(rgb), _p(opacity), _p(depth), _stream())
    _lib.check(rc, "composite_prefix")


def composite_step_(packed_info, t_starts, t_ends, sigmas, rgbs, rgb, opacity, depth, opc_thres, n_samples_iter,
                    ray_mask, stats):
    """composite_prefix_ + mask / alive-count / sample-count bookkeeping (cednerf/utils.py:301-307)."""
    _chk(packed_info, torch.int64, "packed_info"); _chk(stats, torch.int64, "stats")
    for nm, t in (("rgb", rgb), ("opacity", opacity), ("depth", depth)):
        _chk(t, torch.float32, nm)
    assert ray_mask.dtype == torch.bool and ray_mask.is_cuda and ray_mask.shape[0] == packed_info.shape[0]
    with profiling.span("composite", 0):
        rc = _lib.lib().ced_composite_step(packed_info.shape[0], _p(packed_info), _p(t_starts), _p(t_ends),
                                           _p(sigmas), _p(rgbs), _p(rgb), _p(opacity), _p(depth), float(opc_thres),
                                           int(n_samples_iter), _p(ray_mask), _p(stats), _stream())
    _lib.check(rc, "composite_step")


def composite_test_(sigmas, rgbs, t_start, t_end, pack_info, alive_indices, T_threshold, alpha_threshold, opacity,
                    depth, rgb):
    _chk(pack_info, torch.int64, "pack_info"); _chk(alive_indices, torch.int64, "alive_indices")
    rc = _lib.lib().ced_composite_test(alive_indices.shape[0], _p(sigmas), _p(rgbs), _p(t_start), _p(t_end),
                                       _p(pack_info), _p(alive_indices), float(T_threshold), float(alpha_threshold),
                                       _p(opacity), _p(depth), _p(rgb), _stream())
    _lib.check(rc, "composite_test")


def finalize_pixels_(bkgd, rgb, opacity, depth):
    _chk(bkgd, torch.float32, "render_bkgd", allow_none=True)
    rc = _lib.lib().ced_finalize_pixels(rgb.shape[0], _p(bkgd), _p(rgb), _p(opacity), _p(depth), _stream())
    _lib.check(rc, "finalize_pixels")


# ----------------------------------------------------------------------------------------------
# frame renderer (the whole render_image_test loop in one native call)
# ----------------------------------------------------------------------------------------------
def build_occupancy_accel(binaries: torch.Tensor) -> torch.Tensor:
    """ced_build_occupancy_accel: the brick distance field of an occupancy grid [m,res,res,res] (bool / uint8), as a
    uint8 tensor to hand to the frame renderer.  Rebuild it when the grid changes (train_real.py:332-336)."""
    assert binaries.is_cuda and binaries.is_contiguous() and binaries.ndim == 4
    _check_current_device(binaries.device.index, "binaries")
    m, res = binaries.shape[0], binaries.shape[1]
    L = _lib.lib()
    need = int(L.ced_occupancy_accel_bytes(m, res))
    if need < 0:
        raise ValueError("build_occupancy_accel: unsupported grid size")
    accel = torch.empty((need,), device=binaries.device, dtype=torch.uint8)
    _lib.check(L.ced_build_occupancy_accel(_p(_as_u8(binaries)), m, res, _p(accel), need, _stream()), "build_occupancy_accel")
    return accel


def _with_workgroups(desc: _lib.FieldDesc, max_workgroups: int) -> _lib.FieldDesc:
    """The descriptor with its per-call launch property `max_workgroups` set (a copy when it differs)."""
    if int(max_workgroups) == int(desc.max_workgroups):
        return desc
    d2 = _lib.FieldDesc()
    C.memmove(C.byref(d2), C.byref(desc), C.sizeof(_lib.FieldDesc))
    d2.max_workgroups = int(max_workgroups)
    return d2


class FrameTracer:
    """Event pairs + per-iteration counters for ced_render_image_test (see ced_frame_trace)."""

    def __init__(self, capacity: int = 96, with_events: bool = True):
        self.capacity = capacity
        self.struct = _lib.FrameTrace()
        self.struct.capacity = capacity
        self._alive = (C.c_int64 * capacity)()
        self._nsamp = (C.c_int64 * capacity)()
        self._samples = (C.c_int64 * capacity)()
        self.struct.iter_alive = self._alive
        self.struct.iter_n_samples = self._nsamp
        self.struct.iter_samples = self._samples
        self.events = None
        if with_events:
            self.events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                           for _ in range(capacity)]
            for a, b in self.events:       # torch creates the hipEvent lazily on the first record
                a.record(); b.record()
            self._b = (C.c_void_p * capacity)(*[e[0].cuda_event for e in self.events])
            self._e = (C.c_void_p * capacity)(*[e[1].cuda_event for e in self.events])
            self.struct.field_begin = self._b
            self.struct.field_end = self._e

        self.stamps = None

    def enable_device_stamps(self, device) -> None:
        """Have the field kernel itself stamp, per iteration, when its first workgroup started and its last one finished
        (device wall clock): the interval the kernel was executing -- the event pair also counts its wait for CUs."""
        self.stamps = torch.zeros((self.capacity, 2), device=device, dtype=torch.int64)
        self.struct.field_stamps = C.c_void_p(self.stamps.data_ptr())

    def field_intervals_device(self):
        """(start, end) of every field launch in ms on the device wall clock (after the stream has been synchronised);
        None for an iteration whose launch had no workgroup with work."""
        n = min(int(self.struct.n_iters), self.capacity)
        khz = int(_lib.lib().ced_wall_clock_khz())
        st = self.stamps[:n].cpu().numpy().astype(np.uint64)
        out = []
        for a, b in st:
            out.append(None if (a == np.uint64(0xffffffffffffffff) or b == 0) else (float(a) / khz, float(b) / khz))
        return out

    def iterations(self):
        n = min(int(self.struct.n_iters), self.capacity)
        return [dict(n_alive=int(self._alive[i]), n_samples=int(self._nsamp[i]), n_new=int(self._samples[i]))
                for i in range(n)]

    def field_intervals(self, ref: "torch.cuda.Event"):
        """(begin, end) of every field launch in ms after `ref` (an event recorded earlier on the device)."""
        n = min(int(self.struct.n_iters), self.capacity)
        return [(ref.elapsed_time(self.events[i][0]), ref.elapsed_time(self.events[i][1])) for i in range(n)]

    def field_ms(self):
        """Per-iteration field-kernel durations (ms); call after the stream has been synchronised."""
        n = min(int(self.struct.n_iters), self.capacity)
        return [self.events[i][0].elapsed_time(self.events[i][1]) for i in range(n)]


# One workspace + pinned hand-shake buffer per (device, stream) and call family: frames in flight on different streams
# (PipelinedRenderer) never share them.  Two caches: ced_render_image_gather reads the image workspace after
# ced_render_image has returned, so the frame calls must not reuse it.
_frame_ws: Dict[tuple, tuple] = {}
_image_ws: Dict[tuple, tuple] = {}
_ws_lock = __import__("threading").Lock()


def _cached_workspace(cache: dict, device, stream: int, need_bytes: int, host_words: int = 512):
    """(device uint8 buffer of at least need_bytes, pinned int64 buffer of at least host_words) of (device, stream)."""
    key = (device.index, stream)
    with _ws_lock:
        ws = cache.get(key)
        if ws is None or ws[0].numel() < need_bytes or ws[1].numel() < host_words:
            ws = (ws[0] if ws is not None and ws[0].numel() >= need_bytes
                  else torch.empty((max(need_bytes, 1),), device=device, dtype=torch.uint8),
                  ws[1] if ws is not None and ws[1].numel() >= host_words
                  else torch.zeros((host_words,), dtype=torch.int64).pin_memory())
            cache[key] = ws
    return ws


def render_image_test_native(desc: _lib.FieldDesc, rays_o, rays_d, binaries, aabbs, near_plane, far_plane,
                             render_step_size, cone_angle, early_stop_eps, max_samples, timestamps, t_per_ray, bkgd,
                             tracer: Optional[FrameTracer] = None, field_stream: Optional[torch.cuda.Stream] = None,
                             accel: Optional[torch.Tensor] = None, max_workgroups: int = 0):
    """ced_render_image_test.  Returns (rgb [n,3], opacity [n,1], depth [n,1], total_samples).
    field_stream: optional stream shared by concurrently rendered frames for their field kernels; accel: the grid's
    brick distance field (build_occupancy_accel; None = built inside the call); max_workgroups: workgroups of a field
    launch (0 = one per CU)."""
    _chk(rays_o, torch.float32, "rays_o"); _chk(rays_d, torch.float32, "rays_d")
    _chk(aabbs, torch.float32, "aabbs"); _chk(timestamps, torch.float32, "timestamps")
    _chk(bkgd, torch.float32, "render_bkgd", allow_none=True)
    assert rays_o.ndim == 2 and rays_o.shape[1] == 3 and rays_o.shape == rays_d.shape
    assert binaries.is_cuda and binaries.is_contiguous() and binaries.ndim == 4
    n = rays_o.shape[0]
    m, res = binaries.shape[0], binaries.shape[1]
    assert aabbs.shape == (m, 6)
    if t_per_ray:
        assert timestamps.numel() == n, "per-ray timestamps must have one entry per ray"
    dev = rays_o.device
    L = _lib.lib()
    need = int(L.ced_render_image_test_workspace_bytes(n, m, res, float(cone_angle), int(max_samples)))
    if need < 0:
        raise ValueError("render_image_test: unsupported sizes")
    ws = _cached_workspace(_frame_ws, dev, torch.cuda.current_stream().cuda_stream, need)
    rgb = torch.empty((n, 3), device=dev, dtype=torch.float32)
    opacity = torch.empty((n, 1), device=dev, dtype=torch.float32)
    depth = torch.empty((n, 1), device=dev, dtype=torch.float32)
    total = C.c_int64(0)
    rc = L.ced_render_image_test(C.byref(_with_workgroups(desc, max_workgroups)), n, _p(rays_o), _p(rays_d),
                                 _p(_as_u8(binaries)), m, res, _p(aabbs), _p(accel), float(near_plane), float(far_plane), float(render_step_size), float(cone_angle),
                                 float(early_stop_eps), int(max_samples), _p(timestamps), int(bool(t_per_ray)), _p(bkgd),
                                 _p(rgb), _p(opacity), _p(depth), _p(ws[0]), ws[0].numel(), C.c_void_p(ws[1].data_ptr()),
                                 C.byref(total), C.byref(tracer.struct) if tracer is not None else None,
                                 C.c_void_p(field_stream.cuda_stream) if field_stream is not None else None, _stream())
    _lib.check(rc, "render_image_test")
    return rgb, opacity, depth, int(total.value)


def _march_all_args(rays_o, rays_d, binaries, aabbs, accel, near_planes, far_plane, step_size, cone_angle, t_sorted,
                    t_indices, hits) -> tuple:
    """The checked inputs of ced_march_all as its arguments up to `hits`."""
    _chk(rays_o, torch.float32, "rays_o"); _chk(rays_d, torch.float32, "rays_d")
    _chk(aabbs, torch.float32, "aabbs"); _chk(near_planes, torch.float32, "near_planes")
    assert binaries.is_cuda and binaries.is_contiguous() and binaries.ndim == 4
    assert accel is not None and accel.is_cuda
    n = rays_o.shape[0]
    m, res = binaries.shape[0], binaries.shape[1]
    if m > 1:
        _chk(t_sorted, torch.float32, "t_sorted"); _chk(t_indices, torch.int64, "t_indices")
        assert t_sorted.shape == (n, 2 * m) and t_indices.shape == (n, 2 * m) and hits.shape == (n, m) and hits.is_contiguous()
    return (n, _p(rays_o), _p(rays_d), _p(_as_u8(binaries)), m, res, _p(aabbs), _p(accel), _p(near_planes), float(far_plane),
            float(step_size), float(cone_angle), _p(t_sorted) if m > 1 else None, _p(t_indices) if m > 1 else None,
            _p(_as_u8(hits)) if m > 1 else None)


def march_all(rays_o, rays_d, binaries, aabbs, accel, near_planes, far_plane: float, step_size: float, cone_angle: float,
              want_ray_indices: bool = True, t_sorted=None, t_indices=None, hits=None):
    """ced_march_all: every ray marched to the far plane on the accelerated walk.  Several grid levels need the sorted
    ray / box events (t_sorted, t_indices, hits).  Returns (t_starts, t_ends, ray_indices or None, packed_info [n,2])."""
    args = _march_all_args(rays_o, rays_d, binaries, aabbs, accel, near_planes, far_plane, step_size, cone_angle, t_sorted,
                           t_indices, hits)
    n = args[0]
    dev = rays_o.device
    L = _lib.lib()
    packed = torch.zeros((n, 2), device=dev, dtype=torch.int64)
    _lib.check(L.ced_march_all(*args, 0, _p(packed), None, None, None, 0, None, _stream()), "march_all (count)")
    counts = packed[:, 1]
    incl = torch.cumsum(counts, 0)
    packed[:, 0] = incl - counts
    total = int(incl[-1].item()) if n > 0 else 0
    t_starts = torch.empty((total,), device=dev, dtype=torch.float32)
    t_ends = torch.empty((total,), device=dev, dtype=torch.float32)
    ray_indices = torch.empty((total,), device=dev, dtype=torch.int64) if want_ray_indices else None
    if total > 0:
        _lib.check(L.ced_march_all(*args, 1, _p(packed), _p(t_starts), _p(t_ends), _p(ray_indices), 0, None, _stream()),
                   "march_all (fill)")
    return t_starts, t_ends, ray_indices, packed


def march_all_onepass(rays_o, rays_d, binaries, aabbs, accel, near_planes, far_plane: float, step_size: float,
                      cone_angle: float, capacity: int, t_sorted=None, t_indices=None, hits=None):
    """ced_march_all, one pass (fill = 2) into arrays of `capacity` samples.  Returns (t_starts, t_ends, packed_info,
    total) with `total` a DEVICE int64 scalar: the samples marched; > capacity means some rays stored nothing.  Rays'
    ranges are in workgroup arrival order (not sorted by ray)."""
    args = _march_all_args(rays_o, rays_d, binaries, aabbs, accel, near_planes, far_plane, step_size, cone_angle, t_sorted,
                           t_indices, hits)
    dev = rays_o.device
    packed = torch.empty((args[0], 2), device=dev, dtype=torch.int64)
    total = torch.zeros((1,), device=dev, dtype=torch.int64)
    t_starts = torch.empty((capacity,), device=dev, dtype=torch.float32)
    t_ends = torch.empty((capacity,), device=dev, dtype=torch.float32)
    rc = _lib.lib().ced_march_all(*args, 2, _p(packed), _p(t_starts), _p(t_ends), None, int(capacity), _p(total), _stream())
    _lib.check(rc, "march_all (one pass)")
    return t_starts, t_ends, packed, total



def _render_image(desc: _lib.FieldDesc, rays_o, rays_d, packed_info, t_starts, t_ends, early_stop_eps, alpha_thre,
                  timestamps, t_per_ray, bkgd, full: bool, chunk_rays: int, max_workgroups: int):
    """ced_render_image + ced_render_image_gather.  full: pixel sums and every per-sample output; otherwise the
    sampling-only mode (density only) and the kept samples' ray_indices, t_starts, t_ends.  Returns
    ((rgb, opacity, depth) or None, extras, ray_offsets [n+1] int64, (samples evaluated, iterations))."""
    _chk(rays_o, torch.float32, "rays_o"); _chk(rays_d, torch.float32, "rays_d")
    _chk(packed_info, torch.int64, "packed_info"); _chk(t_starts, torch.float32, "t_starts")
    _chk(t_ends, torch.float32, "t_ends"); _chk(timestamps, torch.float32, "timestamps")
    n = rays_o.shape[0]
    n_all = t_starts.shape[0]
    assert packed_info.shape == (n, 2) and t_ends.shape == (n_all,)
    if t_per_ray:
        assert timestamps.numel() == n, "per-ray timestamps must have one entry per ray"
    dev = rays_o.device
    L = _lib.lib()
    need = int(L.ced_render_image_workspace_bytes(n, n_all))
    if need < 0:
        raise ValueError("render_image: unsupported sizes")
    ws = _cached_workspace(_image_ws, dev, torch.cuda.current_stream().cuda_stream, need)
    f = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)
    pixels = (f(n, 3), f(n, 1), f(n, 1)) if full else None
    kept = torch.empty((n,), device=dev, dtype=torch.int32)
    stats = (C.c_int64 * 3)()
    rc = L.ced_render_image(C.byref(_with_workgroups(desc, max_workgroups)), n, _p(rays_o), _p(rays_d), n_all,
                            _p(packed_info), _p(t_starts), _p(t_ends), float(early_stop_eps), float(alpha_thre),
                            _p(timestamps), int(bool(t_per_ray)), _p(bkgd), *(map(_p, pixels) if full else (None,) * 3),
                            _p(kept), _p(ws[0]), ws[0].numel(), C.c_void_p(ws[1].data_ptr()), stats, None, _stream())
    mode = "" if full else " (sampling)"
    _lib.check(rc, "render_image" + mode)
    processed = int(stats[0])
    offsets = torch.zeros((n + 1,), device=dev, dtype=torch.int64)
    torch.cumsum(kept, 0, out=offsets[1:])
    total = int(stats[2])                    # = offsets[-1], without another device round trip
    extras = {"ray_indices": torch.empty((total,), device=dev, dtype=torch.int64), "t_starts": f(total), "t_ends": f(total)}
    if full:
        extras.update(sigmas=f(total), rgbs=f(total, 3), weights=f(total), trans=f(total), alphas=f(total))
    if total > 0:               # (an alpha threshold can drop every sample of a faint scene)
        names = ("ray_indices", "t_starts", "t_ends", "sigmas", "rgbs", "weights", "trans", "alphas")
        rc = L.ced_render_image_gather(n, n_all, processed, _p(ws[0]), ws[0].numel(), _p(offsets), int(chunk_rays),
                                       *(_p(extras.get(k)) for k in names), _stream())
        _lib.check(rc, "render_image_gather" + mode)
    return pixels, extras, offsets, (processed, int(stats[1]))


def render_image_eval_native(desc: _lib.FieldDesc, rays_o, rays_d, packed_info, t_starts, t_ends, early_stop_eps,
                             alpha_thre, timestamps, t_per_ray, bkgd, chunk_rays: int = 0, max_workgroups: int = 0):
    """ced_render_image + ced_render_image_gather: `sampling` (visibility filter) and `rendering` of cednerf/utils.py:115-133
    from one field evaluation per sample.  (packed_info, t_starts, t_ends): the one-shot march of all rays.
    Returns (rgb [n,3], opacity [n,1], depth [n,1], extras, ray_offsets [n+1] int64, stats) where extras holds the
    kept samples' ray_indices (relative to chunks of `chunk_rays` rays when > 0), t_starts, t_ends, sigmas, rgbs,
    weights, trans, alphas in the reference's order, and stats = (samples evaluated, iterations)."""
    _chk(bkgd, torch.float32, "render_bkgd", allow_none=True)
    assert rays_o.ndim == 2 and rays_o.shape[1] == 3 and rays_o.shape == rays_d.shape
    (rgb, opacity, depth), extras, offsets, stats = _render_image(
        desc, rays_o, rays_d, packed_info, t_starts, t_ends, early_stop_eps, alpha_thre, timestamps, t_per_ray, bkgd,
        True, chunk_rays, max_workgroups)
    return rgb, opacity, depth, extras, offsets, stats


def sampling_native(desc: _lib.FieldDesc, rays_o, rays_d, packed_info, t_starts, t_ends, early_stop_eps, alpha_thre,
                    timestamps, t_per_ray, max_workgroups: int = 0):
    """The visibility filter of OccGridEstimator.sampling (sigma_fn = the fused field) on ced_render_image's
    sampling-only mode: density evaluated front to back, rays stopped at the transmittance threshold.
    Returns the surviving (ray_indices, t_starts, t_ends) -- those of the filter over every marched sample."""
    _, extras, _, _ = _render_image(desc, rays_o, rays_d, packed_info, t_starts, t_ends, early_stop_eps, alpha_thre,
                                    timestamps, t_per_ray, None, False, 0, max_workgroups)
    return extras["ray_indices"], extras["t_starts"], extras["t_ends"]


class ScheduleExchange:
    """ced_shard_exchange for frames whose rays are dealt over the ranks of a torch.distributed group: per iteration the
    library hands the row of per-frame survivor counts to `reduce`, which enqueues an all-reduce(sum) of it on the
    calling thread's current stream (the stream the native call runs on), so that every rank's scheduling launch sees
    the image-global N_alive of cednerf/utils.py:231-235.

    One instance per concurrently running native call (a lane of PipelinedRenderer): the per-iteration rows live in a
    buffer of its own.  Collectives of one communicator must be issued in the same order on every rank, and the lanes'
    threads run independently -- so with several lanes NO lane issues its own collective: `issuer` (set by
    PipelinedRenderer) hands the row to the ONE collecting thread, which issues every lane's all-reduces and pixel gathers
    on ONE process group in an order that depends on the lanes' own message sequences only, never on timing
    (dist.PipelinedRenderer.render_steps).  Without an issuer (a renderer on its own) the all-reduce is issued here.

    global_rays: rays of the whole image; local_rays [n_frames]: the real (unpadded) rays of this rank's share of every
    frame.  `reduce_fn(tensor)` replaces the all-reduce (tests)."""

    def __init__(self, n_frames: int, global_rays: int, local_rays, device, max_samples: int, cone_angle: float,
                 group=None, reduce_fn=None):
        import torch.distributed as dist
        L = _lib.lib()
        self.n_frames = int(n_frames)
        self.iterations = int(L.ced_render_frames_test_iterations(float(cone_angle), int(max_samples)))
        self.host_words = (int(L.ced_render_frames_test_host_bytes(float(cone_angle), int(max_samples))) + 7) // 8
        self.counts = torch.zeros((self.iterations + 1, self.n_frames), device=device, dtype=torch.int64)
        self.local_rays = torch.as_tensor(local_rays, dtype=torch.int32).reshape(-1).to(device).contiguous()
        assert self.local_rays.numel() == self.n_frames
        self.group, self.error, self.calls = group, None, 0
        self._reduce_fn = reduce_fn
        self.issuer = None             # callable(exchange, row, stream_handle, iteration): see the class comment

        def _cb(user, counts_ptr, n_counts, iteration, stream):
            try:
                row = self.counts[iteration]
                assert row.data_ptr() == counts_ptr and n_counts == self.n_frames
                if self.issuer is not None and self._reduce_fn is None:
                    self.issuer(self, row, stream or 0, iteration)     # returns once the collective is enqueued on `stream`
                    self.calls += 1
                    return 0
                cur = torch.cuda.current_stream(row.device)
                if cur.cuda_stream != (stream or 0):           # not the thread's current stream: make it so
                    cur = torch.cuda.ExternalStream(stream, device=row.device)
                with torch.cuda.stream(cur):
                    if self._reduce_fn is not None:
                        self._reduce_fn(row)
                    else:
                        dist.all_reduce(row, op=dist.ReduceOp.SUM, group=self.group)
                self.calls += 1
                return 0
            except BaseException as e:                         # never let an exception cross the C frame
                self.error = e
                return 1

        self._cb = _lib.EXCHANGE_FN(_cb)
        self.struct = _lib.ShardExchange(int(global_rays), C.c_void_p(self.local_rays.data_ptr()),
                                         C.c_void_p(self.counts.data_ptr()), self._cb, None)


def render_frames_test_native(desc: _lib.FieldDesc, n_frames: int, rays_o, rays_d, binaries, aabbs, near_plane, far_plane,
                              render_step_size, cone_angle, early_stop_eps, max_samples, frame_times, bkgd,
                              tracer: Optional[FrameTracer] = None, field_stream: Optional[torch.cuda.Stream] = None,
                              accel: Optional[torch.Tensor] = None, max_workgroups: int = 0,
                              exchange: Optional[ScheduleExchange] = None):
    """ced_render_frames_test: `n_frames` frames (rays frame-major, [n_frames * rays_per_frame, 3]) through shared
    launches, every frame on its own schedule.  Returns (rgb [N,3], opacity [N,1], depth [N,1], [total_samples per frame]).
    exchange: the frames are this rank's shares of frames sharded over several ranks (ced_render_frames_test_sharded):
    one image-global schedule per frame."""
    _chk(rays_o, torch.float32, "rays_o"); _chk(rays_d, torch.float32, "rays_d")
    _chk(aabbs, torch.float32, "aabbs"); _chk(frame_times, torch.float32, "frame_times")
    _chk(bkgd, torch.float32, "render_bkgd", allow_none=True)
    assert rays_o.ndim == 2 and rays_o.shape[1] == 3 and rays_o.shape == rays_d.shape
    assert binaries.is_cuda and binaries.is_contiguous() and binaries.ndim == 4
    n = rays_o.shape[0]
    assert n_frames >= 1 and n % n_frames == 0, "rays must hold n_frames equal frames"
    assert frame_times.numel() == n_frames, "one time per frame"
    m, res = binaries.shape[0], binaries.shape[1]
    assert aabbs.shape == (m, 6)
    dev = rays_o.device
    L = _lib.lib()
    if exchange is None:
        need = int(L.ced_render_frames_test_workspace_bytes(n_frames, n // n_frames, m, res, float(cone_angle), int(max_samples)))
    else:
        need = int(L.ced_render_frames_test_sharded_workspace_bytes(n_frames, n // n_frames, int(exchange.struct.global_rays_per_frame),
                                                                    m, res, float(cone_angle), int(max_samples)))
    if need < 0:
        raise ValueError("render_frames_test: unsupported sizes (1..64 frames)")
    host_words = 512 if exchange is None else max(512, exchange.host_words)
    ws = _cached_workspace(_frame_ws, dev, torch.cuda.current_stream().cuda_stream, need, host_words)
    rgb = torch.empty((n, 3), device=dev, dtype=torch.float32)
    opacity = torch.empty((n, 1), device=dev, dtype=torch.float32)
    depth = torch.empty((n, 1), device=dev, dtype=torch.float32)
    totals = (C.c_int64 * n_frames)()
    args = (C.byref(_with_workgroups(desc, max_workgroups)), n_frames, n // n_frames, _p(rays_o),
            _p(rays_d), _p(_as_u8(binaries)), m, res, _p(aabbs), _p(accel), float(near_plane), float(far_plane), float(render_step_size),
            float(cone_angle), float(early_stop_eps), int(max_samples), _p(frame_times), _p(bkgd),
            _p(rgb), _p(opacity), _p(depth), _p(ws[0]), ws[0].numel(), C.c_void_p(ws[1].data_ptr()),
            totals, C.byref(tracer.struct) if tracer is not None else None,
            C.c_void_p(field_stream.cuda_stream) if field_stream is not None else None, _stream())
    if exchange is None:
        rc = L.ced_render_frames_test(*args)
    else:
        assert exchange.n_frames == n_frames and exchange.counts.device == dev
        exchange.error = None
        rc = L.ced_render_frames_test_sharded(*args, C.byref(exchange.struct))
        if exchange.error is not None:
            raise exchange.error
    _lib.check(rc, "render_frames_test")
    return rgb, opacity, depth, [int(v) for v in totals]


# ----------------------------------------------------------------------------------------------
# occupancy-grid maintenance
# ----------------------------------------------------------------------------------------------
def occ_cell_points(cell_indices: torch.Tensor, noise: torch.Tensor, res: int, aabb) -> torch.Tensor:
    """Jittered sample position of every listed cell of one grid level (ced_occ_cell_points)."""
    _chk(cell_indices, torch.int64, "cell_indices"); _chk(noise, torch.float32, "noise")
    n = cell_indices.shape[0]
    assert noise.shape == (n, 3)
    pos = torch.empty((n, 3), device=cell_indices.device, dtype=torch.float32)
    ab = (C.c_float * 6)(*[float(v) for v in aabb])
    rc = _lib.lib().ced_occ_cell_points(n, _p(cell_indices), _p(noise), int(res), ab, _p(pos), _stream())
    _lib.check(rc, "occ_cell_points")
    return pos


def occ_ema_update_(occs: torch.Tensor, cell_ids: torch.Tensor, density: torch.Tensor, step_size: float,
                    ema_decay: float) -> None:
    """ced_occ_ema_update, in place: every listed cell c of occs becomes fmax(occs[c] * ema_decay, the largest
    density * step_size among its entries of cell_ids); cell_ids may repeat cells, in any order."""
    _chk(occs, torch.float32, "occs"); _chk(cell_ids, torch.int64, "cell_ids"); _chk(density, torch.float32, "density")
    assert cell_ids.ndim == 1 and density.shape == cell_ids.shape
    decayed = torch.empty_like(density)                          # the call's workspace
    rc = _lib.lib().ced_occ_ema_update(cell_ids.shape[0], _p(cell_ids), _p(density), float(step_size), float(ema_decay),
                                       _p(occs), _p(decayed), decayed.numel() * 4, _stream())
    _lib.check(rc, "occ_ema_update")


# ----------------------------------------------------------------------------------------------
# time-sliced occupancy grids
# ----------------------------------------------------------------------------------------------
TIME_MAX_BINS, TIME_MAX_TIMES = 256, 64           # ced_field_density_time_max: 1 <= B <= 256, 1 <= S <= 64


def field_density_time_max(desc: _lib.FieldDesc, positions, times, out=None):
    """ced_field_density_time_max: out[b, p] = fmax over s of the density at (positions[p], times[b, s]), started from 0,
    from one launch.  positions [n,3], times [B,S] (each in [0,1]) -> [B,n]; every density has `field_forward`'s bits, a
    NaN density is ignored.  out = a [B,n] buffer to write into instead of a fresh one."""
    _chk(positions, torch.float32, "positions"); _chk(times, torch.float32, "times")
    n = positions.shape[0]
    if positions.shape != (n, 3) or times.dim() != 2:
        raise ValueError(f"field_density_time_max: positions [n,3], times [B,S]: got {list(positions.shape)}, {list(times.shape)}")
    b, s = times.shape
    if not (1 <= b <= TIME_MAX_BINS and 1 <= s <= TIME_MAX_TIMES):
        raise ValueError(f"field_density_time_max: times [B,S] with 1 <= B <= {TIME_MAX_BINS}, 1 <= S <= {TIME_MAX_TIMES}: "
                         f"got {list(times.shape)}")
    (out,) = _outputs((("out", (n,), torch.float32),), b, positions.device, (True,), None if out is None else (out,),
                      "field_density_time_max")
    rc = _lib.lib().ced_field_density_time_max(C.byref(desc), n, _p(positions), b, s, _p(times), _p(out), _stream())
    _lib.check(rc, "field_density_time_max")
    return out


def surface_first_crossing(packed_info, t_starts, t_ends, sigmas, thresh: float):
    """ced_surface_first_crossing: per ray of packed_info [N,2] the first sample with sigma >= thresh and the bracket that
    holds the crossing -> (k [N] int64, -1 where there is none; lo [N]; hi [N]).  hi is sample k's midpoint, lo the
    midpoint of the sample before it where that one ends at sample k's start, else sample k's start; 0 for k = -1."""
    _chk(packed_info, torch.int64, "packed_info")
    _chk(t_starts, torch.float32, "t_starts"); _chk(t_ends, torch.float32, "t_ends"); _chk(sigmas, torch.float32, "sigmas")
    n, s = packed_info.shape[0], t_starts.shape[0]
    if packed_info.shape != (n, 2) or t_starts.shape != (s,) or t_ends.shape != (s,) or sigmas.numel() != s:
        raise ValueError(f"surface_first_crossing: packed_info [N,2], t_starts / t_ends / sigmas [S]: got "
                         f"{list(packed_info.shape)}, {list(t_starts.shape)}, {list(t_ends.shape)}, {list(sigmas.shape)}")
    thresh = float(thresh)
    if thresh != thresh:
        raise ValueError("surface_first_crossing: thresh is a NaN")
    dev = packed_info.device
    k = torch.empty((n,), device=dev, dtype=torch.int64)
    lo = torch.empty((n,), device=dev, dtype=torch.float32)
    hi = torch.empty((n,), device=dev, dtype=torch.float32)
    rc = _lib.lib().ced_surface_first_crossing(n, _p(packed_info), _p(t_starts), _p(t_ends), _p(sigmas), thresh, _p(k), _p(lo),
                                               _p(hi), _stream())
    _lib.check(rc, "surface_first_crossing")
    return k, lo, hi


LEVEL_SET_MAX_ITERS = 64                          # ced_field_level_set: 0 <= max_iters <= 64
LEVEL_SET_OUTPUTS = ("t", "x", "sigma", "width", "status", "evals")   # its outputs, in `want=` order
_LEVEL_SET = (("t", *_F32_1), ("x", *_F32_3), ("sigma", *_F32_1), ("width", *_F32_1), ("status", (), torch.int32),
              ("evals", (), torch.int32))


def check_level_set(sigma_thresh, max_iters, tol):
    """(sigma_thresh, max_iters, tol) of the bisection as (float, int, float), or ValueError: a number > 0, an int in
    0 .. 64, a number >= 0."""
    if isinstance(max_iters, bool) or not isinstance(max_iters, (int, np.integer)) or not 0 <= int(max_iters) <= LEVEL_SET_MAX_ITERS:
        raise ValueError(f"max_iters must be an int in 0 .. {LEVEL_SET_MAX_ITERS}, got {max_iters!r}")
    try:
        thresh_f, tol_f = float(sigma_thresh), float(tol)
    except (TypeError, ValueError):
        raise ValueError(f"sigma_thresh must be a number > 0 and tol a number >= 0, got {sigma_thresh!r}, {tol!r}") from None
    if not thresh_f > 0.0:                        # refuses a NaN too
        raise ValueError(f"sigma_thresh must be a number > 0, got {sigma_thresh!r}")
    if not tol_f >= 0.0:
        raise ValueError(f"tol must be a number >= 0, got {tol!r}")
    return thresh_f, int(max_iters), tol_f


def field_level_set(desc: _lib.FieldDesc, origins, dirs, lo, hi, times, thresh: float = 1.0, max_iters: int = 32,
                    tol: float = 0.0, want=(True, True, True, True, True, True)):
    """ced_field_level_set: per row the bisection of the density along o + d * t on the bracket [lo, hi], from one launch.
    origins / dirs [n,3], lo / hi [n], times [n] or [1] (one time for all rows) -> (t [n], x [n,3], sigma [n], width [n],
    status [n] int32, evals [n] int32): status 0 = a crossing, sigma(t - width) < thresh <= sigma(t) = `sigma`; 1 = the
    bracket starts at or above the threshold (t = lo); 2 = it never reaches it (t = hi).  sigma has `field_forward`'s bits
    (include/cednerf_hip.h states every operation).  want = which of the six to compute; the others come back as None."""
    thresh, max_iters, tol = check_level_set(thresh, max_iters, tol)
    _chk(origins, torch.float32, "origins"); _chk(dirs, torch.float32, "dirs")
    _chk(lo, torch.float32, "lo"); _chk(hi, torch.float32, "hi"); _chk(times, torch.float32, "times")
    n = origins.shape[0]
    if origins.shape != (n, 3) or dirs.shape != (n, 3) or lo.shape != (n,) or hi.shape != (n,) or times.numel() not in (1, n):
        raise ValueError(f"field_level_set: origins / dirs [n,3], lo / hi [n], times [n] or [1]: got {list(origins.shape)}, "
                         f"{list(dirs.shape)}, {list(lo.shape)}, {list(hi.shape)}, {list(times.shape)}")
    t_per_row = int(times.numel() == n and n != 1)
    outs = _outputs(_LEVEL_SET, n, origins.device, want, None, "field_level_set")
    rc = _lib.lib().ced_field_level_set(C.byref(desc), n, _p(origins), _p(dirs), _p(lo), _p(hi), _p(times), t_per_row, thresh,
                                        max_iters, tol, *[_p(o) for o in outs], _stream())
    _lib.check(rc, "field_level_set")
    return tuple(outs)


def occ_time_slices_workspace(n_bins: int, levels: int, res: int, device) -> torch.Tensor:
    """The zeroed `hit` workspace of one build of time slices (ced_occ_time_slices_workspace_bytes)."""
    need = int(_lib.lib().ced_occ_time_slices_workspace_bytes(int(n_bins), int(levels), int(res)))
    if need < 0:
        raise ValueError(f"occ_time_slices: n_bins={n_bins} (1 .. {TIME_MAX_BINS}), levels={levels} (1 .. 64), res={res} (1 .. 1024)")
    return torch.zeros((need,), device=device, dtype=torch.uint8)


def occ_time_slices(cell_ids, max_sigma, step_size: float, thre: float, levels: int, res: int, union_binaries=None,
                    dilate: int = 1, workspace=None, finish: bool = True):
    """ced_occ_time_slices: B occupancy grids from the maxima of `field_density_time_max`.  cell_ids [n] int64 (level * R^3 +
    cell), max_sigma [B,n] -> bool [B, levels, R, R, R]: a listed cell is hit where max_sigma * step_size > thre (float32
    product; false for a NaN), an unlisted one is not; dilate = 1 ORs the hits over each cell's 3x3x3 neighbourhood inside
    its level; union_binaries [levels, R, R, R] bool, where given, is ANDed on.  workspace / finish: a build that hands its
    rows over in several calls makes one `occ_time_slices_workspace`, passes it to every call and finish=False (mark only,
    returns None) to all but the last."""
    _chk(cell_ids, torch.int64, "cell_ids"); _chk(max_sigma, torch.float32, "max_sigma")
    _chk(union_binaries, torch.bool, "union_binaries", allow_none=True)
    n = cell_ids.shape[0]
    if cell_ids.shape != (n,) or max_sigma.dim() != 2 or max_sigma.shape[1] != n:
        raise ValueError(f"occ_time_slices: cell_ids [n], max_sigma [B,n]: got {list(cell_ids.shape)}, {list(max_sigma.shape)}")
    b, levels, res = max_sigma.shape[0], int(levels), int(res)
    if dilate not in (0, 1) or isinstance(dilate, bool):
        raise ValueError(f"occ_time_slices: dilate must be 0 or 1, got {dilate!r}")
    grid = (levels, res, res, res)
    if union_binaries is not None and tuple(union_binaries.shape) != grid:
        raise ValueError(f"occ_time_slices: union_binaries must be {list(grid)}, got {list(union_binaries.shape)}")
    dev = cell_ids.device
    if workspace is None:
        workspace = occ_time_slices_workspace(b, levels, res, dev)
    _chk(workspace, torch.uint8, "workspace")
    out = torch.empty((b,) + grid, device=dev, dtype=torch.bool) if finish else None
    rc = _lib.lib().ced_occ_time_slices(n, _p(cell_ids), _p(max_sigma), b, float(step_size), float(thre), levels, res,
                                        _p(_as_u8(union_binaries)), int(dilate), _p(_as_u8(out)), _p(workspace),
                                        workspace.numel(), _stream())
    _lib.check(rc, "occ_time_slices")
    return out
