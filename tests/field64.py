"""An independent differentiable model of the TRAINING forward, in plain torch on the CPU (test infrastructure).

Written from the model's definition (oracle/oracle.py's `hash_levels` / `time_encode`, the reference's
cednerf/model.py:97-488, utils.py:27-43, render.py:101-124); it imports nothing of ced_nerf_amd.train / .ops / .losses, and
every derivative comes from torch.autograd.  The working dtype is a parameter: float64 is the reference the HIP gradients
are held to, float32 gives the noise floor of fp32 arithmetic on the same graph (`e32` of the tests).

Two places follow the encode's fp32 contract instead of exact arithmetic, both detached:
  * the cell index g = floor(clamp(x, 0, 1) * scale + 0.5) is computed in float32, so a sample lands in the cell the
    kernels (and the C oracle) use;
  * the VALUE of the fraction is the float32 one, (x * scale + 0.5) - g with x, the product and the sum rounded to
    float32 -- the position the encode is defined on (hash_encoder_half.py:131, cednerf_oracle.c: hash_encode_one) -- and
    its DERIVATIVE is d frac / dx = scale, exact.  The exact fraction x64 * scale64 + 0.5 - g differs from it by up to
    half an ulp of the scaled position (2^-13 at max_res 4096): a property of the inputs' format, 2000 times the
    per-entry summation bound the table gradient is held to, and not what the tests are after.
The temporal key-frame k and t_frac = 3t - floor(3t) likewise use the float32 product 3t (hash_encoder_inter.py:148-160).
"""
import math

import numpy as np
import torch

from oracle.oracle import hash_levels

PRIME_Y, PRIME_Z = 2654435761, 805459861
U = 2.0 ** -24                       # unit roundoff of float32
HALF_PI32 = float(np.float32(0.5 * math.pi))           # encoder.py:41,83 adds float32(0.5 * pi)


# ---------------------------------------------------------------------------------------------------------------------
# hash grid
# ---------------------------------------------------------------------------------------------------------------------
def levels_of(cfg):
    return hash_levels(cfg["base_res"], cfg["max_res"], cfg["n_levels"], cfg["log2_hashmap_size"])


def _cell(x, scale32, dx_scaled=True, fp32_position=True):
    """x [n,3] (working dtype, may require grad) -> (g int64 [n,3], frac [n,3]): see the module docstring.
    dx_scaled False: the derivative is taken w.r.t. the scaled position (d frac / dx = 1), the reference's own convention
    (hash_encoder_half.py:212-213).  fp32_position False: the exact fraction x * scale + 0.5 - g of the working dtype (a
    smooth function of x inside a cell: what torch.autograd.gradcheck can difference)."""
    xc = x.clamp(0.0, 1.0)                                  # torch's rule: the gradient passes where 0 <= x <= 1
    x32 = xc.detach().to(torch.float32)
    pos32 = x32 * torch.tensor(scale32, dtype=torch.float32) + torch.tensor(0.5, dtype=torch.float32)
    g32 = torch.floor(pos32)
    if not fp32_position:
        return g32.to(torch.int64), xc * float(scale32) + 0.5 - g32.to(x.dtype)
    lin = xc * float(scale32) if dx_scaled else xc
    frac = (pos32 - g32).to(x.dtype) + (lin - lin.detach())
    return g32.to(torch.int64), frac


def _corner(lv, l, g, frac, c):
    """corner c (bit a set: the upper neighbour on axis a) -> (table entry int64 [n], per-axis weights [n,3])."""
    bits = torch.tensor([(c >> a) & 1 for a in range(3)], dtype=torch.int64)
    p = g + bits
    if int(lv["hashed"][l]):
        idx = p[:, 0] ^ ((p[:, 1] * PRIME_Y) & 0xffffffff) ^ ((p[:, 2] * PRIME_Z) & 0xffffffff)
    else:
        r = int(lv["res"][l])
        idx = (p[:, 0] + p[:, 1] * r + p[:, 2] * r * r) & 0xffffffff
    idx = int(lv["offset"][l]) + idx % int(lv["size"][l])
    wa = torch.where(bits.bool()[None, :], frac, 1.0 - frac)
    return idx, wa


def keyframe(t):
    """t [n] -> (k int64 [n], t_frac float32 [n]) of the temporal table, in the reference's float32 arithmetic."""
    ts = t.detach().to(torch.float32) * torch.tensor(3.0, dtype=torch.float32)
    fl = torch.floor(ts)
    return fl.clamp(max=2.0).to(torch.int64), ts - fl


def hash_encode(x, table, cfg, t=None, dx_scaled=True, fp32_position=True):
    """x [n,3], table [E,2] or (temporal, with t [n]) [E,8], both of the working dtype -> features [n, 2 L].
    Differentiable in the table and -- non-temporal tables only, as in the reference -- in x (`_cell` for the switches)."""
    lv = levels_of(cfg)
    temporal = bool(cfg.get("temporal", False))
    n = x.shape[0]
    if temporal:
        x = x.detach()
        k, tf = keyframe(t)
        tf = tf.to(table.dtype)[:, None]
        tab = table.reshape(-1, 4, 2)
        rows = torch.arange(n)
    out = []
    for l in range(cfg["n_levels"]):
        g, frac = _cell(x, lv["scale"][l], dx_scaled, fp32_position)
        corners = [_corner(lv, l, g, frac, c) for c in range(8)]
        idx = torch.stack([ci for ci, _ in corners], dim=1)                          # [n, 8]
        w = torch.stack([(wa[:, 0] * wa[:, 1]) * wa[:, 2] for _, wa in corners], dim=1)
        if temporal:
            e = tab[idx]                                                             # [n, 8, 4, 2]
            f = e[rows, :, k] * (1.0 - tf)[:, None] + e[rows, :, k + 1] * tf[:, None]
        else:
            f = table[idx]                                                           # [n, 8, 2]: one gather per level
        out.append((w[:, :, None] * f).sum(dim=1))
    return torch.cat(out, dim=1)


def hash_grad_stats(x, dy, table, cfg, t=None, dx_scaled=False):
    """What the derived bounds of the hash-backward tests need, in float64:
      m [E] (temporal: [E,4])       number of (sample, level, corner) contributions to the entry (key-frame slot); levels
                                    whose two dy are both zero contribute nothing (hash_encoder_half.py:209)
      A [E,2] (temporal: [E,4,2])   sum of |w dy| (temporal: |w dy tw|) over those contributions
      B [n,3]                       (non-temporal) per sample and axis, the sum over levels and corners of
                                    (|f0 g0| + |f1 g1|) * (the other two weights) [* scale if dx_scaled]"""
    lv = levels_of(cfg)
    temporal = bool(cfg.get("temporal", False))
    x = x.detach().double(); dy = dy.detach().double().reshape(x.shape[0], cfg["n_levels"], 2)
    table = table.detach().double()
    E = table.shape[0]
    if temporal:
        k, tf = keyframe(t)
        tw = torch.stack([1.0 - tf.double(), tf.double()], dim=1)      # [n, 2]: key-frames k, k + 1
        m = torch.zeros(E * 4, dtype=torch.float64); A = torch.zeros(E * 4, 2, dtype=torch.float64)
    else:
        m = torch.zeros(E, dtype=torch.float64); A = torch.zeros(E, 2, dtype=torch.float64)
    B = torch.zeros(x.shape[0], 3, dtype=torch.float64)
    for l in range(cfg["n_levels"]):
        g, frac = _cell(x, lv["scale"][l])
        gl = dy[:, l]
        live = ((gl != 0).any(dim=1)).double()
        for c in range(8):
            idx, wa = _corner(lv, l, g, frac, c)
            w = (wa[:, 0] * wa[:, 1]) * wa[:, 2]
            if temporal:
                for j in range(2):
                    slot = idx * 4 + k + j
                    m.index_add_(0, slot, live)
                    A.index_add_(0, slot, (w * tw[:, j]).abs()[:, None] * gl.abs())
            else:
                m.index_add_(0, idx, live)
                A.index_add_(0, idx, w.abs()[:, None] * gl.abs())
                dots = (table[idx].abs() * gl.abs()).sum(dim=1) * (float(lv["scale"][l]) if dx_scaled else 1.0)
                others = torch.stack([wa[:, 1] * wa[:, 2], wa[:, 0] * wa[:, 2], wa[:, 0] * wa[:, 1]], dim=1).abs()
                B += dots[:, None] * others
    if temporal:
        return m.reshape(E, 4), A.reshape(E, 4, 2), None
    return m, A, B


def table_grad_terms32(x, dy, cfg, t=None):
    """The per-corner terms of the table gradient in the reference's float32 arithmetic (w = (wx wy) wz, w dy, and for the
    temporal table (w dy)(1 - t_frac), (w dy) t_frac), summed per entry in float64: the C oracle's sums term for term.
    -> [E,2] float64 (temporal [E,8])."""
    lv = levels_of(cfg)
    temporal = bool(cfg.get("temporal", False))
    x = x.detach().float(); dy = dy.detach().float().reshape(x.shape[0], cfg["n_levels"], 2)
    E = int(lv["total"])
    out = torch.zeros(E * 4 if temporal else E, 2, dtype=torch.float64)
    if temporal:
        k, tf = keyframe(t)
    for l in range(cfg["n_levels"]):
        g, frac = _cell(x, lv["scale"][l])
        gl = dy[:, l]
        live = (gl != 0).any(dim=1)
        for c in range(8):
            idx, wa = _corner(lv, l, g, frac, c)
            term = (((wa[:, 0] * wa[:, 1]) * wa[:, 2])[:, None] * gl)[live]
            if temporal:
                out.index_add_(0, (idx * 4 + k)[live], (term * (1.0 - tf)[live, None]).double())
                out.index_add_(0, (idx * 4 + k + 1)[live], (term * tf[live, None]).double())
            else:
                out.index_add_(0, idx[live], term.double())
    return out.reshape(E, 8) if temporal else out


# ---------------------------------------------------------------------------------------------------------------------
# the field
# ---------------------------------------------------------------------------------------------------------------------
def frequency4(v):
    """tcnn Frequency(n_frequencies=4) on [n, D]: [dim][freq k][sin, cos] of pi 2^k v."""
    ang = math.pi * v[:, :, None] * (2.0 ** torch.arange(4, dtype=v.dtype))
    return torch.stack([torch.sin(ang), torch.cos(ang)], dim=-1).reshape(v.shape[0], 8 * v.shape[1])


def mlp(h, weights):
    """bias-free, ReLU between the layers, linear last layer; W[out][in]."""
    for w in weights[:-1]:
        h = torch.relu(h @ w.t())
    return h @ weights[-1].t()


class TruncExp(torch.autograd.Function):
    """utils.py:27-43: forward exp(x), backward g * exp(min(x, 15))."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return torch.exp(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.exp(x.clamp(max=15.0))


def time_encode(t, move_norm=None):
    """encoder.py:36-44 (move_norm None) / :75-90; t, move_norm [n,1] -> [n,9].  No gradient (model.py:386-396)."""
    with torch.no_grad():
        t = t.detach()
        s = [t * float(2 ** k) for k in range(4)]
        if move_norm is None:
            return torch.cat([t] + [torch.sin(p) for p in s] + [torch.sin(p + HALF_PI32) for p in s], dim=1)
        cols = [t]
        for k, p in enumerate(s):
            att = torch.exp(-1.0 * (move_norm.detach() * float(k * 2 ** k)))
            cols += [torch.sin(p) * att, torch.sin(p + HALF_PI32) * att]
        return torch.cat(cols, dim=1)


def warp(pos, mo, aabb, moving_step, use_div):
    """model.py:356-383 -> (xn clamped, x_move unclamped normalised, move, selector)."""
    move = mo[:, :3] * moving_step
    if use_div:
        move = move + torch.tanh(mo[:, 3:6]) * moving_step
    x_move = (pos + move - aabb[:3]) / (aabb[3:] - aabb[:3])
    selector = ((x_move > 0.0) & (x_move < 1.0)).all(dim=-1)            # open at 0 and 1
    return x_move.clamp(0.0, 1.0), x_move, move, selector


def sh2(dirs):
    """SH degree 2 of the direction as tcnn sees it: (d / |d| + 1) / 2 mapped back to [-1, 1] (model.py:447-455)."""
    u = (dirs / dirs.norm(dim=-1, keepdim=True) + 1.0) / 2.0
    w = u * 2.0 - 1.0
    return torch.stack([torch.full_like(w[:, 0], 0.28209479177387814), -0.48860251190291987 * w[:, 1],
                        0.48860251190291987 * w[:, 2], -0.48860251190291987 * w[:, 0]], dim=-1)


PARAM_GROUPS = ("xyz_wrap", "mlp_base", "mlp_head", "mlp_feat_prediction", "mlp_weight_prediction")


def make_params(params, dtype, heads=None):
    """The `params` dict of TrainableField (+ heads: {"mlp_feat_prediction": [W0, W1], "mlp_weight_prediction": [...]}, numpy
    or torch) -> {name: leaf tensor}, named as TrainableField.named_parameters() names them.  An fp16 table is read as its
    exact values."""
    P = {}
    leaf = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64)).to(dtype).requires_grad_()
    P["hash_table"] = leaf(np.asarray(params["hash"]["table"]).astype(np.float64))
    for grp in PARAM_GROUPS:
        src = params.get(grp) if grp in params else (heads or {}).get(grp)
        for i, w in enumerate(src or []):
            P[f"{grp}.{i}"] = leaf(w.detach().cpu().numpy() if torch.is_tensor(w) else w)
    return P


def _group(P, grp):
    return [P[f"{grp}.{i}"] for i in range(sum(1 for k in P if k.startswith(grp + ".")))]


def field_forward(P, params, pos, t, dirs):
    """positions [n,3], t [n], directions [n,3] (working dtype) -> dict(rgb, sigma, move, selector, xn, x_move, hash_feat,
    bout[, latent_losses, weight_losses])."""
    dtype = pos.dtype
    aabb = torch.as_tensor(np.asarray(params["aabb"], np.float64)).to(dtype)
    cfg = {k: v for k, v in params["hash"].items() if k != "table"}
    t1 = t.reshape(-1, 1)
    mo = mlp(frequency4(torch.cat([pos, t1], dim=-1)), _group(P, "xyz_wrap"))
    xn, x_move, move, selector = warp(pos, mo, aabb, float(params["moving_step"]), bool(params["use_div_offsets"]))
    hash_feat = hash_encode(xn, P["hash_table"], cfg, t1[:, 0])
    feat = hash_feat
    mode = int(params["time_mode"])
    if mode:
        te = time_encode(t1) if mode == 1 else time_encode(t1, move.detach().norm(dim=-1, keepdim=True))
        feat = torch.cat([feat, te], dim=-1)
    bout = mlp(feat, _group(P, "mlp_base"))
    sigma = TruncExp.apply(bout[:, 0] - 1.0) * selector.to(dtype)
    rgb = torch.sigmoid(mlp(torch.cat([sh2(dirs), bout[:, 1:]], dim=-1), _group(P, "mlp_head")))
    out = dict(rgb=rgb, sigma=sigma, move=move, selector=selector, xn=xn, x_move=x_move, hash_feat=hash_feat, bout=bout)
    fp, wp = _group(P, "mlp_feat_prediction"), _group(P, "mlp_weight_prediction")
    if fp or wp:
        temp = frequency4(torch.cat([x_move, t1], dim=-1))                      # model.py:431-441
        if fp:
            out["latent_losses"] = torch.nn.functional.huber_loss(mlp(temp, fp), hash_feat, reduction="none") \
                * selector[:, None].to(dtype)
        if wp:
            out["weight_losses"] = mlp(temp, wp)
    return out


def field_forward_rays(P, params, rays_o, rays_d, ray_indices, t_starts, t_ends, ts_per_ray):
    """utils.py:86-104: positions o + d (t_start + t_end) / 2, the ray's direction and time."""
    pos = rays_o[ray_indices] + rays_d[ray_indices] * ((t_starts + t_ends)[:, None] / 2.0)
    return field_forward(P, params, pos, ts_per_ray.reshape(-1)[ray_indices], rays_d[ray_indices])


# ---------------------------------------------------------------------------------------------------------------------
# compositing and the losses of a training step
# ---------------------------------------------------------------------------------------------------------------------
def _ray_layout(ray_indices, n_rays):
    """ray-packed samples (grouped by ray, ascending) -> (counts [n_rays], position of each sample inside its ray)."""
    cnt = torch.bincount(ray_indices, minlength=n_rays)
    start = torch.cumsum(cnt, 0) - cnt
    return cnt, torch.arange(ray_indices.shape[0]) - start[ray_indices]


def _exclusive_ray_sum(v, ray_indices, n_rays):
    """sum of v over the earlier samples of the same ray (a cumulative sum per ray, not across rays)."""
    cnt, k = _ray_layout(ray_indices, n_rays)
    pad = torch.zeros(n_rays, max(int(cnt.max()) if cnt.numel() else 0, 1), dtype=v.dtype)
    pad = pad.index_put((ray_indices, k), v)
    return (torch.cumsum(pad, dim=1) - pad)[ray_indices, k]


def composite(sigma, rgb, t_starts, t_ends, ray_indices, n_rays, bkgd=None):
    """render.py:58-95: T_i = exp(-sum_{j<i} s_j d_j), a_i = 1 - exp(-s_i d_i), w = T a; colours, opacities, background."""
    sd = sigma * (t_ends - t_starts)
    trans = torch.exp(-_exclusive_ray_sum(sd, ray_indices, n_rays))
    weights = trans * (1.0 - torch.exp(-sd))
    colors = torch.zeros(n_rays, 3, dtype=sigma.dtype).index_add(0, ray_indices, weights[:, None] * rgb)
    opac = torch.zeros(n_rays, 1, dtype=sigma.dtype).index_add(0, ray_indices, weights[:, None])
    if bkgd is not None:
        colors = colors + bkgd * (1.0 - opac)
    return dict(colors=colors, opacities=opac, weights=weights, trans=trans)


def head_terms(out, comp, ray_indices, n_rays):
    """render.py:101-124: per-ray latent loss (sum, detached weights) and weight loss (mean with the +1 of
    scatter_reduce_'s include_self, weights with their gradient, huber against the transmittance)."""
    dtype = comp["weights"].dtype
    res = {}
    w = comp["weights"][:, None]
    if "latent_losses" in out:
        res["latent_losses"] = torch.zeros(n_rays, out["latent_losses"].shape[1], dtype=dtype).index_add(
            0, ray_indices, w.detach() * out["latent_losses"])
    if "weight_losses" in out:
        wl = torch.nn.functional.huber_loss(out["weight_losses"], comp["trans"][:, None], reduction="none") \
            * out["selector"][:, None].to(dtype)
        cnt = torch.bincount(ray_indices, minlength=n_rays).to(dtype) + 1.0
        res["weight_losses"] = torch.zeros(n_rays, 1, dtype=dtype).index_add(0, ray_indices, w * wl) / cnt[:, None]
    return res


def distortion(weights, t_starts, t_ends, ray_indices, n_rays):
    """sum_rays [ sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i s_i w_i^2 ] / (1 + the largest ray index with a sample); samples in
    marching order, so |m_i - m_j| = m_i - m_j for j < i."""
    m, s = (t_starts + t_ends) / 2.0, t_ends - t_starts
    before_w = _exclusive_ray_sum(weights, ray_indices, n_rays)
    before_wm = _exclusive_ray_sum(weights * m, ray_indices, n_rays)
    total = (2.0 * weights * (m * before_w - before_wm)).sum() + (s * weights * weights).sum() / 3.0
    return total / (int(ray_indices.max()) + 1)


def step_loss(out, comp, target, t_starts, t_ends, ray_indices, n_rays, rgb_loss="smooth_l1", distortion_loss=False,
              acc_entropy_loss=False, opacity_loss=False, weight_rgbper=False, factor=1e-3):
    """train_real.py:369-409 as train_step states it -> (loss, {term: unscaled value})."""
    F = torch.nn.functional
    loss = F.smooth_l1_loss(comp["colors"], target) if rgb_loss == "smooth_l1" else F.mse_loss(comp["colors"], target)
    acc = comp["opacities"]
    terms = {}
    if opacity_loss:
        terms["opacity"] = (-torch.xlogy(acc, acc)).mean()
    if distortion_loss:
        terms["distortion"] = distortion(comp["weights"], t_starts, t_ends, ray_indices, n_rays)
    if acc_entropy_loss:
        tl = (1.0 - acc).clamp(1e-6, 1.0 - 1e-6)
        terms["acc_entropy"] = -(tl * torch.log(tl) + (1.0 - tl) * torch.log(1.0 - tl)).mean()
    if weight_rgbper:
        per = (out["rgb"] - target[ray_indices]).pow(2).sum(dim=-1)
        terms["weight_rgbper"] = (per * comp["weights"].detach()).sum() / target.shape[0]
    for v in terms.values():
        loss = loss + factor * v
    for v in head_terms(out, comp, ray_indices, n_rays).values():
        loss = loss + v.mean()
    return loss, terms


def rel_err(a, b):
    """||a - b|| / ||b|| in float64."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


# ---------------------------------------------------------------------------------------------------------------------
# shared inputs of the CPU and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
# tests/test_gpu_parity.py's FIELD_CASES (the flag combinations of the field tests), restated so that the CPU tests import
# no GPU module
FIELD_CASES = [
    dict(), dict(use_div_offsets=True), dict(use_time_embedding=True),
    dict(use_time_embedding=True, use_time_attenuation=True, use_div_offsets=True),
    dict(table_dtype=np.float16), dict(temporal_hash=True, table_dtype=np.float16, use_time_embedding=True),
]
STEP = 1.0 / 4096.0


def level0_faces():
    """float32 coordinates whose level-0 fraction (scale 15) is exactly 0 in the encode's arithmetic."""
    faces = []
    for j in range(1, 15):
        x = np.float32((j - 0.5) / 15.0)
        for cand in (x, np.nextafter(x, np.float32(1)), np.nextafter(x, np.float32(0))):
            if np.float32(cand * np.float32(15.0)) + np.float32(0.5) == np.float32(j):
                faces.append(cand)
                break
    return np.array(faces, np.float32)


def ray_ordered_points(n, seed, ray_len=1531):
    """n float32 points in [0,1]^3 in marching order: rays through the unit cube, consecutive samples 1/4096 apart (about
    250 samples per level-0 cell, 2-4 per cell at max_res 1024).  Every third ray starts near a face and runs out of the cube,
    its coordinates clamped to exactly 0 or 1 for the rest (what the warp hands the encode); stretches lie exactly on
    level-0 cell faces; (0,0,0), (1,1,1) and (0.5,0.5,0.5) are among the points."""
    rng = np.random.default_rng(seed)
    n_rays = -(-n // ray_len)
    o = rng.uniform(0.05, 0.95, size=(n_rays, 3))
    d = rng.normal(size=(n_rays, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    for r in range(0, n_rays, 3):
        a = r % 3
        o[r, a] = rng.uniform(0.9, 0.98); d[r] = np.abs(d[r]) * np.where(np.arange(3) == a, 1.0, 0.3) + [0.3, 0.2, 0.1]
        d[r] /= np.linalg.norm(d[r])
    k = np.arange(n_rays * ray_len) % ray_len
    r = np.arange(n_rays * ray_len) // ray_len
    x = np.clip(o[r] + d[r] * (k * STEP)[:, None], 0.0, 1.0).astype(np.float32)[:n]
    faces = level0_faces()
    for i, start in enumerate(range(29, n - 12, 997)):                # runs of 9 samples on a level-0 face, one axis each
        x[start:start + 9, i % 3] = faces[i % len(faces)]
    if n > 8:
        x[5] = 0.0; x[6] = 1.0; x[7] = 0.5
    return x


def hash_dy(n, n_levels, seed):
    """dL/dy [n, 2 L]: magnitudes in [0.5, 2], random signs; every 7th sample has two levels zeroed and a few samples are all
    zero, so skipped samples sit inside runs."""
    rng = np.random.default_rng(seed)
    dy = (rng.uniform(0.5, 2.0, size=(n, 2 * n_levels)) * rng.choice([-1.0, 1.0], size=(n, 2 * n_levels))).astype(np.float32)
    dy[::7, 4:8] = 0.0
    for i in (3, 40, 41, n // 2, n - 1):
        if 0 <= i < n and n > 4:
            dy[i] = 0.0
    return dy


def temporal_times(n, seed, ray_len=1531):
    """One time per ray (as in training), the key-frame edge values, and runs of consecutive samples that alternate
    between two key-frame pairs."""
    rng = np.random.default_rng(seed)
    t = np.repeat(rng.uniform(0, 1, size=-(-n // ray_len)), ray_len)[:n].astype(np.float32)
    edge = np.array([0.0, 1.0, 1.0 / 3.0, 2.0 / 3.0, 0.999999], np.float32)
    if n >= 64:
        t[10:15] = edge
        for start in range(100, n - 40, 1200):
            t[start:start + 40:2] = 0.3; t[start + 1:start + 40:2] = 0.4
    else:
        t[:min(n, 5)] = edge[:min(n, 5)]
    return t


def random_table(cfg, dtype, seed):
    width = 8 if cfg.get("temporal", False) else 2
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(size=(int(levels_of(cfg)["total"]), width)) * 0.5).astype(dtype)


def xavier_heads(n_levels, seed):
    rng = np.random.default_rng(seed)

    def xav(o, i):
        lim = math.sqrt(6.0 / (i + o))
        return rng.uniform(-lim, lim, size=(o, i)).astype(np.float32)
    return {"mlp_feat_prediction": [xav(64, 32), xav(2 * n_levels, 64)], "mlp_weight_prediction": [xav(64, 32), xav(1, 64)]}


def whole_field_case(case, max_res=64, log2T=15):
    """The whole-field gradient problem of FIELD_CASES[case]: the "init" regime with the table times 3000 (features of
    order 0.3), both prediction heads, 64 rays / about 4000 ray-packed samples in marching order, a time per ray; a third
    of the rays leave the box.  max_res 64: a gradient of this graph is a discontinuous function of the normalised position
    (cell faces for dx, ReLU masks downstream), and a level of scale s magnifies the half-ulp by which two correct fp32
    evaluations of that position differ to s * 3e-8 of a cell; at max_res 1024 one sample in about 3000 changes cell
    between two evaluations and each such event moves a gradient's norm by 1e-3 .. 1e-2 (measured on this model, float32
    against float64).  The fine levels' backward is held to its own bound at the operator (test_gpu_train_gradients 3a)."""
    from ced_nerf_amd import synthetic as S
    kw = dict(FIELD_CASES[case])
    params = S.init_field_params([-1.5, -1.5, -1.5, 1.5, 1.5, 1.5], 1e-3, max_res, log2T, regime="init", seed=21 + case, **kw)
    tab = params["hash"]["table"]
    params["hash"]["table"] = (tab.astype(np.float32) * np.float32(3000.0)).astype(tab.dtype)
    rng = np.random.default_rng(60 + case)
    n_rays = 64
    o = rng.uniform(-0.4, 0.4, size=(n_rays, 3)).astype(np.float32)
    d = rng.normal(size=(n_rays, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    cnt = rng.integers(40, 86, size=n_rays); cnt[[7, 30]] = 0                       # two rays without a sample
    first = rng.uniform(0.0, 1.9, size=n_rays)
    first[::3] = rng.uniform(1.2, 1.7, size=first[::3].shape)                       # these cross the box's faces
    ri = np.repeat(np.arange(n_rays), cnt).astype(np.int64)
    k = np.arange(ri.shape[0]) - (np.cumsum(cnt) - cnt)[ri]
    t0 = (first[ri] + 5e-3 * k).astype(np.float32); t1 = (t0 + np.float32(5e-3)).astype(np.float32)
    ts = rng.uniform(0, 1, size=n_rays).astype(np.float32)
    wr = rng.normal(size=(ri.shape[0], 3)).astype(np.float32)
    return dict(params=params, heads=xavier_heads(params["hash"]["n_levels"], 5 + case), rays_o=o, rays_d=d, ri=ri, t0=t0,
                t1=t1, ts=ts, wr=wr, f16=np.asarray(tab).dtype == np.float16)


def whole_field_run(pb, dtype, density_weight=0.1, plain_exp=False):
    """field64 on a whole_field_case in `dtype`: -> (outputs, {parameter: gradient}) of the piece test's loss
    (rgb wr).sum() + 0.1 density.sum() + 1e3 latent.sum() + weight.sum() + 1e2 (move wr).sum()."""
    P = make_params(pb["params"], dtype, pb["heads"])
    cv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    ri = torch.from_numpy(pb["ri"])
    global TruncExp
    keep = TruncExp
    if plain_exp:                     # the rule the trunc_exp test must tell apart: exp's own derivative
        class _Plain:
            apply = staticmethod(torch.exp)
        TruncExp = _Plain
    try:
        out = field_forward_rays(P, pb["params"], cv(pb["rays_o"]), cv(pb["rays_d"]), ri, cv(pb["t0"]), cv(pb["t1"]),
                                 cv(pb["ts"]))
    finally:
        TruncExp = keep
    wr = cv(pb["wr"])
    loss = (out["rgb"] * wr).sum() + out["sigma"].sum() * density_weight + out["latent_losses"].sum() * 1e3 \
        + out["weight_losses"].sum() + (out["move"] * wr).sum() * 1e2
    loss.backward()
    return out, {k: v.grad for k, v in P.items()}


def noise_floor(g32, g64):
    """e32 per parameter: ||g32 - g64|| / ||g64||."""
    return {k: rel_err(g32[k], g64[k]) for k in g64}
