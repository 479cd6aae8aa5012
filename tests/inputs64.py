"""Gradients at the INPUTS of the training forward -- ray origins, ray directions, per-ray times -- in float64 (test
infrastructure).  No model code of its own: the field is tests/field64.py's (`F.field_forward_rays`, which composes
F.frequency4, F.mlp, F.warp, F.hash_encode, F.sh2 and F.TruncExp) with rays_o, rays_d and ts as leaves; with the temporal
table F.hash_encode detaches what it is handed, so neither position nor time receives a gradient through the lookup.
`train_inputs_backward` restates the input stage's backward from its formulas, for the operator tests.
"""
import math

import numpy as np
import torch

import field64 as F

K1 = 0.48860251190291987


def train_inputs_backward(v, dirs, d_pos=None, d_enc=None, d_sh=None, d_t=None):
    """The backward of the input stage per sample, in float64, from its formulas.  v [n,4] = (x, y, z, t), dirs [n,3];
    upstream gradients d_pos [n,3], d_enc [n,32], d_sh [n,4], d_t [n] (None = zero).
    -> (g_pos [n,3], g_dir [n,3], g_t [n]) and (A_pos, A_dir, A_t), the sums of the absolute values of the elementary
    terms of each, with |sin|, |cos| and |w| replaced by 1 (what an absolute error of the recomputed sin / cos / w
    multiplies)."""
    n = v.shape[0]
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    d_pos = z(n, 3) if d_pos is None else d_pos.double()
    d_enc = z(n, 32) if d_enc is None else d_enc.double()
    d_sh = z(n, 4) if d_sh is None else d_sh.double()
    d_t = z(n) if d_t is None else d_t.double()
    v, dirs = v.double(), dirs.double()
    k = 2.0 ** torch.arange(4, dtype=torch.float64)
    ang = math.pi * v[:, :, None] * k                                   # [n, 4, 4]
    de = d_enc.reshape(n, 4, 4, 2)
    g_v = (math.pi * k * (de[..., 0] * torch.cos(ang) - de[..., 1] * torch.sin(ang))).sum(dim=-1)
    A_v = (math.pi * k * (de[..., 0].abs() + de[..., 1].abs())).sum(dim=-1)
    g_pos, A_pos = d_pos + g_v[:, :3], d_pos.abs() + A_v[:, :3]
    g_t, A_t = d_t + g_v[:, 3], d_t.abs() + A_v[:, 3]
    nrm = dirs.norm(dim=-1, keepdim=True)
    w = dirs / nrm
    g_w = torch.stack([-K1 * d_sh[:, 3], -K1 * d_sh[:, 1], K1 * d_sh[:, 2]], dim=-1)
    g_dir = (g_w - w * (w * g_w).sum(dim=-1, keepdim=True)) / nrm
    A_dir = (g_w.abs() + g_w.abs().sum(dim=-1, keepdim=True)) / nrm
    return (g_pos, g_dir, g_t), (A_pos, A_dir, A_t)


def reduce_rays(g, A, t_mid, ray_indices, n_rays):
    """Per-sample (g_pos, g_dir, g_t) and their absolute sums -> per ray (d_rays_o, d_rays_d, d_ts) and the absolute sums
    of the terms of each: d_rays_o = sum g_pos, d_rays_d = sum (g_pos t_mid + g_dir), d_ts = sum g_t."""
    tm = t_mid.double()[:, None]
    rows = lambda x: torch.zeros(n_rays, *x.shape[1:], dtype=torch.float64).index_add(0, ray_indices, x)
    (g_pos, g_dir, g_t), (A_pos, A_dir, A_t) = g, A
    return ((rows(g_pos), rows(g_pos * tm + g_dir), rows(g_t)),
            (rows(A_pos), rows(A_pos * tm.abs() + A_dir), rows(A_t)))


def upstream(n, seed):
    """Gradients at the input stage's four outputs, drawn like F.hash_dy: magnitudes in [0.5, 2], random signs, some
    samples all zero.  -> dict(d_pos [n,3], d_enc [n,32], d_sh [n,4], d_t [n]) float32."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, width in (("d_pos", 3), ("d_enc", 32), ("d_sh", 4), ("d_t", 1)):
        g = (rng.uniform(0.5, 2.0, size=(n, width)) * rng.choice([-1.0, 1.0], size=(n, width))).astype(np.float32)
        for i in (3, 40, 41, n // 2, n - 1):
            if 0 <= i < n and n > 4:
                g[i] = 0.0
        out[name] = g
    out["d_t"] = out["d_t"][:, 0].copy()
    return out


def whole_field_run(pb, dtype, density_weight=0.1):
    """F.whole_field_run with rays_o, rays_d and ts as leaves -> ({parameter: gradient}, {"rays_o" | "rays_d" | "ts":
    gradient}) of the same loss."""
    P = F.make_params(pb["params"], dtype, pb["heads"])
    cv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    leaves = {k: cv(pb[k]).requires_grad_() for k in ("rays_o", "rays_d", "ts")}
    out = F.field_forward_rays(P, pb["params"], leaves["rays_o"], leaves["rays_d"], torch.from_numpy(pb["ri"]), cv(pb["t0"]),
                               cv(pb["t1"]), leaves["ts"])
    wr = cv(pb["wr"])
    loss = (out["rgb"] * wr).sum() + out["sigma"].sum() * density_weight + out["latent_losses"].sum() * 1e3 \
        + out["weight_losses"].sum() + (out["move"] * wr).sum() * 1e2
    loss.backward()
    return {k: v.grad for k, v in P.items()}, {k: v.grad for k, v in leaves.items()}


def render_loss(P, params, rays_o, rays_d, ts, ri, t0, t1, target, bkgd):
    """Mean squared colour error of the rays composited on fixed samples (train.align_view's loss)."""
    out = F.field_forward_rays(P, params, rays_o, rays_d, ri, t0, t1, ts)
    comp = F.composite(out["sigma"], out["rgb"], t0, t1, ri, rays_o.shape[0], bkgd)
    return torch.nn.functional.mse_loss(comp["colors"], target), comp["colors"]
