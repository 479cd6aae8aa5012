"""DNGPradianceField: host-side mirror of cednerf/model.py:97-488 over the fused HIP field kernel.

Same constructor signature, attributes (`aabb`, `training`, `MOVING_STEP`, ...) and call
conventions as the reference module; the tiny-cuda-nn sub-modules are replaced by plain
parameter tensors (hash table [E,2], bias-free MLP weights W[out][in]) that are re-packed into the
kernel's LDS layout whenever they change.  Forward only (rendering hot path); training is a
"next" row of SURVEY.md section 8f.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Union

import numpy as np
import torch

from . import _lib, ops
from .encoder import SinusoidalEncoder, SinusoidalEncoderWithExp
from .hashgrid import level_tables

MOVING_STEP = 1 / (4096 * 1)   # cednerf/model.py:26


def _xavier_(w: torch.Tensor, gen: Optional[torch.Generator]) -> torch.Tensor:
    n_out, n_in = w.shape
    lim = math.sqrt(6.0 / (n_in + n_out))
    with torch.no_grad():
        w.uniform_(-lim, lim, generator=gen)
    return w


class DNGPradianceField(torch.nn.Module):
    """Instance-NGP radiance field with a motion MLP (reference: cednerf/model.py:97)."""

    def __init__(
        self,
        aabb: Union[torch.Tensor, List[float]],
        num_dim: int = 3,
        use_viewdirs: bool = True,
        density_activation=None,
        geo_feat_dim: int = 15,
        base_resolution: int = 16,
        n_levels: int = 16,
        n_features_per_level: int = 2,
        dst_resolution: int = 4096,
        log2_hashmap_size: int = 19,
        use_feat_predict: bool = False,
        use_weight_predict: bool = False,
        moving_step: float = MOVING_STEP,
        use_div_offsets: bool = False,
        use_time_embedding: bool = False,
        use_time_attenuation: bool = False,
        time_inject_before_sigma: bool = True,
        hash4motion: bool = False,
        hash_dtype: torch.dtype = torch.float32,
        temporal_hash: bool = False,
        seed: Optional[int] = None,
        mlp_precision: str = "f32",
    ) -> None:
        super().__init__()
        if not isinstance(aabb, torch.Tensor):
            aabb = torch.tensor(aabb, dtype=torch.float32)
        self.register_buffer("aabb", aabb.float())
        # fixed by the fused kernel (they are the reference's defaults and what train_real.py uses)
        if num_dim != 3 or not use_viewdirs or geo_feat_dim != 15 or n_features_per_level != 2 or n_levels != 16:
            raise NotImplementedError("the HIP field kernel implements num_dim=3, use_viewdirs=True, "
                                      "geo_feat_dim=15, n_levels=16, n_features_per_level=2")
        if density_activation is not None:
            raise NotImplementedError("density_activation is fixed to trunc_exp(x - 1) (cednerf/model.py:105)")
        if hash4motion:
            raise NotImplementedError("hash4motion is never enabled by the reference (train_real.py:263)")
        if not time_inject_before_sigma:
            raise NotImplementedError("time_inject_before_sigma=False is never used by the reference")
        # use_feat_predict / use_weight_predict (run_hyper.sh:1 passes -f): the two heads only run under
        # `return_interal=self.training` (cednerf/model.py:428-443,479-484), i.e. they are inert in the eval path
        # this module implements; the flags are accepted and recorded, training with them is `train.TrainableField`.
        self.num_dim = num_dim
        self.use_viewdirs = use_viewdirs
        self.geo_feat_dim = geo_feat_dim
        self.geo_feat_dim_head = geo_feat_dim
        self.box_scale = (self.aabb[3:] - self.aabb[:3]).max() / 2
        self.use_feat_predict = use_feat_predict
        self.use_weight_predict = use_weight_predict
        self.use_time_embedding = use_time_embedding
        self.use_time_attenuation = use_time_attenuation
        self.MOVING_STEP = moving_step
        self.use_div_offsets = use_div_offsets
        self.time_inject_before_sigma = time_inject_before_sigma
        self.loose_move = False
        self.motion_input_dim = 3 + 1
        self.motion_output_dim = 3 * 2 if use_div_offsets else 3
        self.return_extra = False
        self.hash_cfg = dict(base_res=base_resolution, max_res=dst_resolution, n_levels=n_levels,
                             log2_hashmap_size=log2_hashmap_size, temporal=bool(temporal_hash))
        self.time_mode = 0 if not use_time_embedding else (2 if use_time_attenuation else 1)
        self.set_mlp_precision(mlp_precision)
        if use_time_embedding:
            self.time_encoder = SinusoidalEncoder(1, 0, 4, True)
            self.time_encoder_feat = SinusoidalEncoderWithExp(1, 0, 4, True)
        base_in = 32 + (9 if self.time_mode else 0)

        gen = None
        if seed is not None:
            gen = torch.Generator().manual_seed(seed)
        tabs = level_tables(base_resolution, dst_resolution, n_levels, log2_hashmap_size)
        width = 8 if temporal_hash else 2
        table = torch.empty((tabs["total"], width), dtype=torch.float32).uniform_(-1e-4, 1e-4, generator=gen)
        self.hash_table = torch.nn.Parameter(table.to(hash_dtype), requires_grad=False)
        P = lambda o, i: torch.nn.Parameter(_xavier_(torch.empty(o, i), gen), requires_grad=False)
        self.xyz_wrap = torch.nn.ParameterList([P(64, 32), P(64, 64), P(64, 64), P(self.motion_output_dim, 64)])
        self.mlp_base = torch.nn.ParameterList([P(64, base_in), P(16, 64)])
        self.mlp_head = torch.nn.ParameterList([P(64, 19), P(64, 64), P(3, 64)])
        self._packed: Optional[torch.Tensor] = None
        self._packed_key = None
        self._packed_src = None                              # the tensors `_packed_key` was taken from, kept alive
        self._desc: Optional[_lib.FieldDesc] = None
        self._desc_lock = __import__("threading").Lock()     # frames in flight share one field

    def set_mlp_precision(self, mlp_precision: str) -> "DNGPradianceField":
        """Arithmetic of the three MLPs (include/cednerf_hip.h): "f32" = exact fp32 MFMA chain, bit-identical
        to the CPU oracle; "f16x2" = split-fp16 MFMA, fp32-grade results; "f16" = fp16 operands with fp32
        accumulation, the precision class of the reference's tiny-cuda-nn networks (cednerf/model.py:200-222)."""
        if mlp_precision not in _lib.MLP_PRECISIONS:
            raise ValueError(f"mlp_precision must be one of {sorted(_lib.MLP_PRECISIONS)}, got {mlp_precision!r}")
        self.mlp_precision = mlp_precision
        return self

    # ---- parameter plumbing -------------------------------------------------------------------
    @classmethod
    def from_params(cls, params: Dict, device="cuda", mlp_precision: str = "f32") -> "DNGPradianceField":
        """Build from the plain-numpy parameter dict of ced_nerf_amd.synthetic.init_field_params."""
        h = params["hash"]
        table = torch.from_numpy(np.ascontiguousarray(h["table"]))
        f = cls(aabb=torch.from_numpy(np.asarray(params["aabb"], np.float32)), dst_resolution=h["max_res"],
                base_resolution=h["base_res"], n_levels=h["n_levels"], log2_hashmap_size=h["log2_hashmap_size"],
                moving_step=params["moving_step"], use_div_offsets=params["use_div_offsets"],
                use_time_embedding=params["time_mode"] != 0, use_time_attenuation=params["time_mode"] == 2,
                hash_dtype=table.dtype, temporal_hash=h.get("temporal", False), mlp_precision=mlp_precision)
        with torch.no_grad():
            f.hash_table.data = table
            for dst, src in ((f.xyz_wrap, params["xyz_wrap"]), (f.mlp_base, params["mlp_base"]),
                             (f.mlp_head, params["mlp_head"])):
                for p, w in zip(dst, src):
                    p.data = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32))
        return f.to(device)

    def export_params(self) -> Dict:
        g = lambda p: p.detach().cpu().numpy()
        return dict(aabb=g(self.aabb), moving_step=float(self.MOVING_STEP), use_div_offsets=self.use_div_offsets,
                    time_mode=self.time_mode, hash=dict(table=g(self.hash_table), **self.hash_cfg),
                    xyz_wrap=[g(p) for p in self.xyz_wrap], mlp_base=[g(p) for p in self.mlp_base],
                    mlp_head=[g(p) for p in self.mlp_head])

    def __getstate__(self):            # copy.deepcopy / pickle: drop the device-side caches and the lock
        state = self.__dict__.copy()
        for k in ("_desc_lock", "_desc", "_packed", "_packed_key", "_packed_src"):
            state.pop(k, None)
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self._packed, self._packed_key, self._packed_src, self._desc = None, None, None, None
        self._desc_lock = __import__("threading").Lock()

    def _weights(self):
        return list(self.xyz_wrap) + list(self.mlp_base) + list(self.mlp_head)

    def weights_changed(self) -> None:
        """Re-pack the MLP weights and re-read the box at the next launch.  The packed blob is keyed on the tensors'
        addresses and version counters; an update that writes them in place without advancing the counters must say so
        here.  Two kinds do: an optimiser that steps outside autograd's bookkeeping (torch's fused Adam may), and every
        in-place write through `.data` (`w.data.mul_(..)`, `w.data.copy_(..)`, `aabb.data.add_(..)`), which is as invisible
        to the key as fused Adam's.  Followed without this call: in-place writes to the tensor itself under no_grad
        (`w.copy_`, `w.mul_`), `load_state_dict`, the checkpoint loaders, `w.data = other`, `.to(device)`,
        `set_mlp_precision`, and assignments to `MOVING_STEP`, `use_div_offsets` and `time_mode`.  The hash table is
        read in place, so every write to it is seen by the next launch."""
        with self._desc_lock:
            self._packed_key = None

    def _descriptor(self) -> _lib.FieldDesc:
        with self._desc_lock:
            return self._descriptor_locked()

    def _descriptor_locked(self) -> _lib.FieldDesc:
        ws = self._weights()
        # Everything the descriptor is made from: the packed tensors by (address, version), the table by address and type
        # (it is read in place), and the python scalars written into it.  `_packed_src` keeps the storages the key was
        # taken from alive, so that after `w.data = other` the allocator cannot hand the old address to the new tensor
        # and re-issue a live key.
        key = (tuple((w.data_ptr(), w._version) for w in ws), self.hash_table.data_ptr(), str(self.hash_table.device),
               self.hash_table.dtype, self.aabb.data_ptr(), self.aabb._version, self.mlp_precision,
               self.MOVING_STEP, self.use_div_offsets, self.time_mode)
        if self._desc is not None and key == self._packed_key:
            return self._desc
        dev = self.hash_table.device
        if dev.type != "cuda":
            raise NotImplementedError("Only support cuda inputs: move the field to a GPU (no CPU fallback).")
        blob = ops.pack_field_weights(self.use_div_offsets, self.time_mode,
                                      [w.detach().cpu().numpy() for w in self.xyz_wrap],
                                      [w.detach().cpu().numpy() for w in self.mlp_base],
                                      [w.detach().cpu().numpy() for w in self.mlp_head],
                                      _lib.MLP_PRECISIONS[self.mlp_precision],
                                      table_dtype=0 if self.hash_table.dtype == torch.float32 else 1,
                                      temporal=self.hash_cfg["temporal"])
        self._packed = torch.from_numpy(blob).to(dev)
        hd, _ = ops.make_hash_desc(self.hash_table.data, **self.hash_cfg)
        d = _lib.FieldDesc()
        aabb = self.aabb.detach().cpu().numpy().astype(np.float32)
        for i in range(6):
            d.aabb[i] = float(aabb[i])
        d.moving_step = float(np.float32(self.MOVING_STEP))
        d.use_div_offsets = int(self.use_div_offsets)
        d.time_mode = int(self.time_mode)
        d.mlp_precision = _lib.MLP_PRECISIONS[self.mlp_precision]
        d.packed_weights = self._packed.data_ptr()
        d.packed_floats = int(self._packed.numel())
        d.hash = hd
        self._desc = d
        self._packed_src = [w.detach() for w in ws] + [self.aabb.detach()]
        self._packed_key = key
        return d

    # ---- reference API ------------------------------------------------------------------------
    @torch.no_grad()
    def hash_encoder(self, x: torch.Tensor, t: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The `hash_encoder(x_move)` call of cednerf/model.py:384: x [N,3] in [0,1] -> [N,32]."""
        d = self._descriptor()
        return ops.hash_encode(d.hash, x.reshape(-1, 3).float().contiguous(),
                               None if t is None else t.reshape(-1).float().contiguous())

    @torch.no_grad()
    def query_move(self, x: torch.Tensor, t: torch.Tensor, return_normalized: bool = False):
        """cednerf/model.py:354-365: the motion network's displacement of x at time t.  x is viewed as [-1, 3], t as
        [-1, 1]; returns (x_move, move), both [N, 3], move = xyz_wrap(Frequency(x, t)) * MOVING_STEP (plus the tanh'd fine
        offsets with use_div_offsets) and x_move = x + move -- the values the fused forward computes internally, in this
        field's mlp_precision, bit for bit (ced_field_move).  return_normalized=True also returns what query_density
        derives from x_move (:378-383): x_norm = (x_move - aabb_min) / (aabb_max - aabb_min) and the boolean selector
        all(0 < x_norm < 1)."""
        if not x.is_cuda:
            raise NotImplementedError("Only support cuda inputs: query_move runs on the HIP kernel (no CPU fallback).")
        x_move, move, x_norm, selector = ops.field_move(
            self._descriptor(), x.reshape(-1, 3).float().contiguous(), t.reshape(-1).float().contiguous(),
            want=(True, True, return_normalized, return_normalized))
        if return_normalized:
            return x_move, move, x_norm, selector
        return x_move, move

    @torch.no_grad()
    def query_move_jacobian(self, x: torch.Tensor, t: torch.Tensor):
        """The motion network's displacement and its derivative: (move [N,3], jac [N,3,4]) with jac[n, a, b] =
        d move_a / d (x, y, z, t)_b at (x, t), by forward mode through the network in this field's mlp_precision, from
        one launch (ced_field_move_jacobian; include/cednerf_hip.h states the operation order).  `move` has
        `query_move`'s bits.  I + jac[:, :, :3] is the deformation gradient of the warp x -> x + move(x, t), jac[:, :, 3]
        its time derivative at a fixed x.  In "f16" the derivative is that of the fp16-rounded network, whose ReLU
        masks differ from the exact network's on a few rows."""
        if not (x.is_cuda and t.is_cuda):
            raise NotImplementedError("Only support cuda inputs: query_move_jacobian runs on the HIP kernel (no CPU fallback).")
        return ops.field_move_jacobian(self._descriptor(), x.reshape(-1, 3).float().contiguous(),
                                       t.reshape(-1).float().contiguous())

    @torch.no_grad()
    def query_velocity(self, x: torch.Tensor, t: torch.Tensor):
        """The velocity of the material point that sits at x at time t (the scene flow): its canonical coordinate
        c = x + move(x, t) does not change, so (I + J_x) v + d move / dt = 0 and v = -(I + J_x)^-1 d move / dt.
        Returns (v [N,3], det [N]) with det = det(I + J_x); where det <= 0 the warp folds and v means little.
        `query_scene_flow` is the same quantity from one fused launch, guarded: 0 and flagged where the warp folds."""
        _, jac = self.query_move_jacobian(x, t)
        _, inv, det = ops.warp_gradient(jac)
        return -(inv @ jac[..., 3:]).squeeze(-1), det

    @torch.no_grad()
    def query_scene_flow(self, x: torch.Tensor, t: torch.Tensor):
        """The scene flow at (x, t): `query_velocity`'s v = -(I + J_x)^-1 d move / dt from ONE launch that keeps the
        Jacobian in registers (ced_field_velocity; include/cednerf_hip.h states every operation), with a guard.  Returns
        (v [N,3], det [N], valid [N] bool): det = det(I + J_x) as computed; valid = det >= 2^-20 and v finite; where not
        valid -- the warp folds there, or the Jacobian is not finite -- v is exactly 0 instead of an infinity, so that a
        sum of w_i * v_i along a ray is not poisoned by one sample.  x is viewed as [-1, 3], t as [-1]."""
        if not (x.is_cuda and t.is_cuda):
            raise NotImplementedError("Only support cuda inputs: query_scene_flow runs on the HIP kernel (no CPU fallback).")
        return ops.field_velocity(self._descriptor(), x.reshape(-1, 3).float().contiguous(), t.reshape(-1).float().contiguous())

    @torch.no_grad()
    def query_density_gradient(self, x: torch.Tensor, t: torch.Tensor, canonical: bool = False):
        """The density and its spatial gradient: (density [N,1], grad [N,3]) at (x, t), grad being what
        torch.autograd.grad(density.sum(), x) returns on the reference's graph (cednerf/model.py:354-445) -- the time
        encoding a constant, trunc_exp's clamped backward, the hash grid's slope inside the cell the encode selects, zero
        outside the box -- by forward mode through the warp and mlp_base in this field's mlp_precision, from one launch
        (ced_field_density_gradient; include/cednerf_hip.h states the operations).  `density` has `query_density`'s
        bits.  canonical=True: the gradient with respect to the canonical point x + move(x, t) instead, i.e. without the
        warp's (I + J_x)^T."""
        density, grad = self._density_gradient(x, t, canonical, want_grad=True)
        return density, grad

    @torch.no_grad()
    def query_normals(self, x: torch.Tensor, t: torch.Tensor, canonical: bool = False):
        """(normals [N,3], density [N,1]): the unit vector towards lower density, -g / |g| with g the gradient of the
        PRE-ACTIVATION density (`query_density_gradient`'s direction without sigma's twenty decades of range); 0 where g
        is 0 or the point leaves the box.  canonical=True: in the canonical frame."""
        density, dlog = self._density_gradient(x, t, canonical, want_grad=False)
        return ops.unit_or_zero(-dlog), density

    def _density_gradient(self, x, t, canonical, want_grad):
        if not (x.is_cuda and t.is_cuda):
            raise NotImplementedError("Only support cuda inputs: the density's gradient runs on the HIP kernel (no CPU fallback).")
        sigma, grad, dlog, dlog_c = ops.field_density_gradient(
            self._descriptor(), x.reshape(-1, 3).float().contiguous(), t.reshape(-1).float().contiguous(),
            want=(True, want_grad and not canonical, not want_grad and not canonical, bool(canonical)))
        if canonical:
            out = sigma.clamp(max=ops.EXP15)[:, None] * dlog_c if want_grad else dlog_c
        else:
            out = grad if want_grad else dlog
        return sigma[:, None], out

    @torch.no_grad()
    def query_level_set(self, origins: torch.Tensor, directions: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor,
                        t: torch.Tensor, sigma_thresh: float = 1.0, max_iters: int = 32, tol: float = 0.0):
        """Where the density reaches sigma_thresh along rays: per row the ray origins + directions * s, a bracket
        [lo, hi] of distances and a time t ([N], or one value for all rows), bisected on `query_density` in this field's
        mlp_precision, from one launch that keeps the rows in registers (ced_field_level_set; include/cednerf_hip.h states
        it operation by operation).  origins / directions are viewed as [-1, 3], lo / hi as [-1].  Returns
        (t [N], x [N,3], sigma [N], width [N], status [N] int32, evals [N] int32):
            status 0  a crossing: density(x) = sigma >= sigma_thresh > density one `width` back along the ray; with
                      tol = 0 and enough rounds (max_iters 0 .. 64) width is 0 or one float32 spacing at t,
            status 1  the bracket starts at or above the threshold: t = lo, width = 0,
            status 2  the bracket's end is below the threshold (or NaN): t = hi, width = hi - lo.
        The bisection stops when hi - lo <= tol, when the midpoint is an endpoint, or after max_iters rounds; evals counts
        the density evaluations (the two endpoints included)."""
        sigma_thresh, max_iters, tol = ops.check_level_set(sigma_thresh, max_iters, tol)
        if not (origins.is_cuda and directions.is_cuda and lo.is_cuda and hi.is_cuda):
            raise NotImplementedError("Only support cuda inputs: query_level_set runs on the HIP kernel (no CPU fallback).")
        o = origins.reshape(-1, 3).float().contiguous()
        times = torch.as_tensor(t, dtype=torch.float32, device=o.device).reshape(-1).contiguous()
        return ops.field_level_set(self._descriptor(), o, directions.reshape(-1, 3).float().contiguous(),
                                   lo.reshape(-1).float().contiguous(), hi.reshape(-1).float().contiguous(), times,
                                   sigma_thresh, max_iters, tol)

    @torch.no_grad()
    def query_move_inverse(self, c: torch.Tensor, t: torch.Tensor, max_iters: int = 32, tol: float = 1e-6,
                           init: Optional[torch.Tensor] = None, method: str = "fixed_point"):
        """The inverse of the warp: per row the x with x + move(x, t) = c, `move` being `query_move`'s.  The density at
        (x, t) is the canonical density at x + move(x, t), so x is where the material point with canonical coordinate c
        sits at time t.  Solved by fixed-point iteration x <- c - move(x, t) from init (default: c), at most max_iters
        (1 .. 1024) evaluations of the motion network in this field's mlp_precision, stopped when the largest component
        of the update is <= tol (ced_field_move_inverse; include/cednerf_hip.h states it operation by operation).
        c is viewed as [-1, 3], t as [-1]; returns (x [N,3], step [N] the size of the last update, evals [N] int32).  A
        row has converged iff step <= tol; the iteration converges where move(., t) is a contraction and reports the
        rows where it did not (evals == max_iters, step > tol) instead of hiding them.
        method="newton" solves the same equation by Newton's method on `query_move_jacobian`, fused into one launch
        (ced_field_move_inverse_newton): `step` is then the max-norm residual |x + move(x, t) - c| of the returned x, a row
        has converged iff step <= tol, it converges on most rows where the fixed point does not, and where the warp folds
        (det(I + J_x) <= 0) it may land on another preimage of c.  An unknown method raises ValueError."""
        max_iters, tol = ops.check_solve(max_iters, tol)
        solve = ops.field_move_inverse_newton if ops.check_method(method) == "newton" else ops.field_move_inverse
        if not (c.is_cuda and t.is_cuda and (init is None or init.is_cuda)):
            raise NotImplementedError("Only support cuda inputs: query_move_inverse runs on the HIP kernel (no CPU fallback).")
        return solve(self._descriptor(), c.reshape(-1, 3).float().contiguous(), t.reshape(-1).float().contiguous(),
                     None if init is None else init.reshape(-1, 3).float().contiguous(), max_iters, tol)

    @torch.no_grad()
    def track_points(self, x: torch.Tensor, t_src, times, max_iters: int = 32, tol: float = 1e-6,
                     method: str = "fixed_point") -> Dict:
        """Where the material points seen at x [P,3] at time t_src (a number, a one-element tensor or [P]) sit at every
        time of `times` ([T]: a sequence or a tensor).  Returns a dict:
            canonical [P,3]  query_move(x, t_src)[0], the points' canonical coordinates,
            positions [T,P,3], step [T,P], evals [T,P] int32  `query_move_inverse`(canonical, times[k]) started at x,
            converged [T,P] bool  step <= tol,
            times [T].
        One launch for all P x T rows (ced_field_track; method="newton": ced_field_track_newton, see
        `query_move_inverse`), neither input expanded in memory."""
        max_iters, tol = ops.check_solve(max_iters, tol)
        track = ops.field_track_newton if ops.check_method(method) == "newton" else ops.field_track
        if not x.is_cuda:
            raise NotImplementedError("Only support cuda inputs: track_points runs on the HIP kernels (no CPU fallback).")
        pts = x.reshape(-1, 3).float().contiguous()
        n = pts.shape[0]
        ts = torch.as_tensor(t_src, dtype=torch.float32, device=pts.device).reshape(-1)
        if ts.numel() == 1:
            ts = ts.expand(n)
        elif ts.numel() != n:
            raise ValueError(f"t_src must be a scalar or hold one time per point ({n}), got {ts.numel()} values")
        tt = torch.as_tensor(times, dtype=torch.float32, device=pts.device).reshape(-1).contiguous()
        desc = self._descriptor()
        canonical = ops.field_move(desc, pts, ts.contiguous(), want=(True, False, False, False))[0]
        positions, step, evals = track(desc, canonical, tt, pts, max_iters, tol)
        return dict(canonical=canonical, positions=positions, step=step, evals=evals, converged=step <= tol, times=tt)

    @torch.no_grad()
    def _query_rgb(self, dir: torch.Tensor, embedding: torch.Tensor, apply_act: bool = True):
        """cednerf/model.py:447-466: colour from view directions and the density branch's embedding
        (results['base_mlp_out']): dir is normalised, mapped to [0, 1] and SH-encoded, mlp_head runs on
        [SH(4), embedding(15)] in this field's mlp_precision, the sigmoid is applied iff apply_act.  Returns
        embedding.shape[:-1] + [3]."""
        if not (dir.is_cuda and embedding.is_cuda):
            raise NotImplementedError("Only support cuda inputs: _query_rgb runs on the HIP kernel (no CPU fallback).")
        rgb = ops.field_rgb(self._descriptor(), dir.reshape(-1, 3).float().contiguous(),
                            embedding.reshape(-1, self.geo_feat_dim).float().contiguous(), apply_act)
        return rgb.view(list(embedding.shape[:-1]) + [3])

    @torch.no_grad()
    def query_density(self, x, t, return_feat: bool = False, return_interal: bool = False):
        """cednerf/model.py:367-445 (eval: no training-only `interal_output`)."""
        if return_interal and self.training and (self.use_feat_predict or self.use_weight_predict):
            raise NotImplementedError("the feature/weight prediction heads (cednerf/model.py:428-443) run in training "
                                      "only; this module is the eval path")
        shp = x.shape
        _, sigma, geo = ops.field_forward(self._descriptor(), x.reshape(-1, 3).float().contiguous(),
                                          t.reshape(-1).float().contiguous(), None, want_geo=return_feat)
        results = {"density": sigma.view(list(shp[:-1]) + [1])}
        if return_feat:
            results["base_mlp_out"] = geo.view(list(shp[:-1]) + [self.geo_feat_dim])
        return results

    @torch.no_grad()
    def forward(self, positions: torch.Tensor, t: torch.Tensor, directions: torch.Tensor = None):
        """cednerf/model.py:468-488: returns (rgb [N,3], {'density': [N,1], 'base_mlp_out': [N,15]})."""
        if self.use_viewdirs and (directions is not None):
            assert positions.shape == directions.shape, f"{positions.shape} v.s. {directions.shape}"
        if directions is None:
            raise NotImplementedError("directions are required (use_viewdirs=True)")
        shp = positions.shape
        rgb, sigma, geo = ops.field_forward(self._descriptor(), positions.reshape(-1, 3).float().contiguous(),
                                            t.reshape(-1).float().contiguous(),
                                            directions.reshape(-1, 3).float().contiguous(), want_geo=True)
        results = {"density": sigma.view(list(shp[:-1]) + [1]),
                   "base_mlp_out": geo.view(list(shp[:-1]) + [self.geo_feat_dim])}
        return rgb.view(list(shp[:-1]) + [3]), results

    # fused closures of the render drivers (cednerf/utils.py:74-104,181-195)
    @torch.no_grad()
    def query_rays(self, rays_o, rays_d, ray_indices, t_starts, t_ends, timestamps, want_rgb: bool = True,
                   n_dev: Optional[torch.Tensor] = None):
        ts = timestamps.reshape(-1).float().contiguous()
        per_ray = bool(self.training)
        return ops.field_forward_rays(self._descriptor(), rays_o, rays_d, ray_indices, t_starts, t_ends, ts, per_ray,
                                      want_rgb, n_dev=n_dev)

    @torch.no_grad()
    def query_move_rays(self, rays_o, rays_d, ray_indices, t_starts, t_ends, timestamps, want_x_norm: bool = False,
                        n_dev: Optional[torch.Tensor] = None):
        """`query_move` at the samples `query_rays` evaluates (same positions, same per-ray / per-frame timestamps):
        returns (move [S,3], x_norm [S,3] or None)."""
        ts = timestamps.reshape(-1).float().contiguous()
        return ops.field_move_rays(self._descriptor(), rays_o, rays_d, ray_indices, t_starts, t_ends, ts,
                                   bool(self.training), want_x_norm, n_dev=n_dev)


    @torch.no_grad()
    def query_density_gradient_rays(self, rays_o, rays_d, ray_indices, t_starts, t_ends, timestamps,
                                    want=(True, True, True, True), n_dev: Optional[torch.Tensor] = None):
        """`ops.field_density_gradient` at the samples `query_rays` evaluates (same positions, same per-ray / per-frame
        timestamps): returns (sigma [S], grad [S,3], dlog [S,3], dlog_canonical [S,3]), None where want= is False."""
        ts = timestamps.reshape(-1).float().contiguous()
        return ops.field_density_gradient_rays(self._descriptor(), rays_o, rays_d, ray_indices, t_starts, t_ends, ts,
                                               bool(self.training), want, n_dev=n_dev)

    @torch.no_grad()
    def query_scene_flow_rays(self, rays_o, rays_d, ray_indices, t_starts, t_ends, timestamps, want=(True, True, True),
                              n_dev: Optional[torch.Tensor] = None):
        """`query_scene_flow` at the samples `query_rays` evaluates (same positions, same per-ray / per-frame timestamps):
        returns (v [S,3], det [S], valid [S] bool), None where want= is False."""
        if not (rays_o.is_cuda and rays_d.is_cuda):
            raise NotImplementedError("Only support cuda inputs: query_scene_flow_rays runs on the HIP kernel (no CPU fallback).")
        ts = timestamps.reshape(-1).float().contiguous()
        return ops.field_velocity_rays(self._descriptor(), rays_o, rays_d, ray_indices, t_starts, t_ends, ts,
                                       bool(self.training), want, n_dev=n_dev)


def make_occ_eval_fn(radiance_field: "DNGPradianceField", timestamps: torch.Tensor, render_step_size: float):
    """The occ_eval_fn closure of train_real.py:324-328: a random training timestamp per point,
    density(x, t) * render_step_size."""
    def occ_eval_fn(x):
        t_idxs = torch.randint(0, len(timestamps), (x.shape[0],), device=x.device)
        t = timestamps[t_idxs]
        return radiance_field.query_density(x, t)["density"] * render_step_size
    return occ_eval_fn


# spelling used by BASELINE.json's north_star
DNGPRadianceField = DNGPradianceField
