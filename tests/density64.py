"""numpy model of the density's spatial derivative, for tests/test_density_gradient_cpu.py and
tests/test_gpu_density_gradient.py.

`base_gradient` is a forward-mode model of the CANONICAL half of the field -- hash encode, time encoding, mlp_base -- on a
float32 normalised position x_norm (the device's own, so that model and kernel sit in the same hash cells), the time and
the row's |move| (for the attenuated time features).  Per level the cell and the fraction are the encode's fp32 ones
(`tests/field64.py:_cell`, dx_scaled: d frac / d x_norm = scale, exact); the features, their three x-tangents and the
time features (tangent 0: the time encoding is a constant) go through mlp_base in float64 or float32, optionally with the
weights and every layer's inputs -- primal and tangents alike -- rounded as an mlp_precision rounds them
(`warp64.rounder`: "f32" to float32, "f16" to one float16, "f16x2" to hi + lo).  The tangents are carried scaled by
2^-K, K = ceil(log2(finest level scale)), as the kernel carries them (exact; it matters only where a float16 would
overflow or go subnormal), and unscaled at the end.  `world_gradients` states include/cednerf_hip.h's last three lines.
"""
import math

import numpy as np

from oracle.oracle import hash_levels
from warp64 import rounder

PRIME_Y, PRIME_Z = 2654435761, 805459861
BASE_MODES = {"f32": "f32", "f32+h16x2": "f32", "f16": "f16", "f16x2": "f16x2"}       # mlp_precision -> mlp_base's
EXP15 = np.float32(math.exp(15.0))                                                   # 3269017.25
HALF_PI32 = np.float32(0.5 * math.pi)


def levels_of(params):
    h = params["hash"]
    return hash_levels(h["base_res"], h["max_res"], h["n_levels"], h["log2_hashmap_size"])


def tangent_log2(params):
    """K = ceil(log2(the finest level's scale))"""
    return int(math.ceil(math.log2(float(levels_of(params)["scale"].max()))))


def _corner_index(lv, l, p):
    """p [n,3] int64 lattice points -> table entry [n] of level l"""
    if int(lv["hashed"][l]):
        idx = p[:, 0] ^ ((p[:, 1] * PRIME_Y) & 0xffffffff) ^ ((p[:, 2] * PRIME_Z) & 0xffffffff)
    else:
        r = int(lv["res"][l])
        idx = (p[:, 0] + p[:, 1] * r + p[:, 2] * r * r) & 0xffffffff
    return int(lv["offset"][l]) + idx % int(lv["size"][l])


def hash_features(params, x_norm, t, dtype=np.float64, exact_fraction=False):
    """x_norm [n,3] float32 in [0,1], t [n] -> (features [n, 2L], d features / d x_norm [n, 2L, 3]) in `dtype`.
    exact_fraction: the fraction x * scale + 0.5 - g of float64 instead of the encode's fp32 one (a smooth function of x
    inside a cell: what a finite difference can be held against); x_norm may then be float64."""
    lv = levels_of(params)
    table = np.asarray(params["hash"]["table"]).astype(dtype)
    n = x_norm.shape[0]
    temporal = bool(params["hash"].get("temporal", False))
    if temporal:
        ts = np.asarray(t, np.float32) * np.float32(3.0)
        fl = np.floor(ts)
        k = np.minimum(fl, np.float32(2.0)).astype(np.int64)
        tf = (ts - fl).astype(dtype)[:, None]
        table = table.reshape(-1, 4, 2)
    rows = np.arange(n)
    feats, dfeats = [], []
    for l in range(int(lv["n_levels"])):
        scale32 = np.float32(lv["scale"][l])
        x32 = np.clip(x_norm, 0.0, 1.0).astype(np.float32)
        pos32 = x32 * scale32 + np.float32(0.5)
        g32 = np.floor(pos32)
        g = g32.astype(np.int64)
        if exact_fraction:
            frac = np.clip(x_norm, 0.0, 1.0).astype(np.float64) * np.float64(scale32) + 0.5 - g32.astype(np.float64)
        else:
            frac = (pos32 - g32).astype(dtype)
        w = np.stack([1 - frac, frac], 0)                                # [corner bit, n, axis]
        f = np.zeros((n, 2), dtype)
        df = np.zeros((n, 2, 3), dtype)
        for c in range(8):
            bits = [(c >> a) & 1 for a in range(3)]
            idx = _corner_index(lv, l, g + np.asarray(bits, np.int64))
            if temporal:
                e = table[idx]                                           # [n, 4, 2]
                v = e[rows, k] * (1 - tf) + e[rows, k + 1] * tf
            else:
                v = table[idx]
            wa = [w[bits[a], :, a] for a in range(3)]
            f += ((wa[0] * wa[1]) * wa[2])[:, None] * v
            for a in range(3):
                others = wa[(a + 1) % 3] * wa[(a + 2) % 3]
                df[:, :, a] += ((1 if bits[a] else -1) * others)[:, None] * v
        feats.append(f)
        dfeats.append(df * dtype(scale32))
    return np.concatenate(feats, 1), np.concatenate(dfeats, 1)


def time_features(time_mode, t, move_norm, dtype=np.float64):
    """the nine time features (cednerf/encoder.py:36-44 / :75-90) [n,9]: t, then time_mode 1: sin(2^k t) k = 0..3 and
    sin(2^k t + pi/2) k = 0..3; time_mode 2: (sin, cos) per k, attenuated by exp(-|move| k 2^k)"""
    t = np.asarray(t).astype(dtype)
    s = [t * dtype(2 ** k) for k in range(4)]
    half_pi = dtype(HALF_PI32)
    if time_mode == 1:
        return np.stack([t] + [np.sin(p) for p in s] + [np.sin(p + half_pi) for p in s], -1)
    mn = np.asarray(move_norm).astype(dtype)
    cols = [t]
    for k, p in enumerate(s):
        att = np.exp(-(mn * dtype(k * 2 ** k)))
        cols += [np.sin(p) * att, np.sin(p + half_pi) * att]
    return np.stack(cols, -1)


def base_gradient(params, x_norm, t, move_norm=None, dtype=np.float64, mode=None, exact_fraction=False):
    """(raw [n], d raw / d x_norm [n,3], pre): the pre-activation density (mlp_base's output 0), its derivative with
    respect to the normalised canonical position, and `pre`, the list of mlp_base's hidden pre-activations ([n,64])"""
    rnd = rounder(mode, dtype)
    carry = dtype(2.0 ** -tangent_log2(params))
    h, dh = hash_features(params, x_norm, t, dtype, exact_fraction)
    dh = dh * carry
    if params["time_mode"]:
        te = time_features(params["time_mode"], t, move_norm, dtype)
        h = np.concatenate([h, te], 1)
        dh = np.concatenate([dh, np.zeros((h.shape[0], 9, 3), dtype)], 1)
    ws = [rnd(np.asarray(w, dtype)) for w in params["mlp_base"]]
    pre = []
    for i, w in enumerate(ws):
        z = rnd(h) @ w.T
        dz = np.einsum("of,nfb->nob", w, rnd(dh))
        if i < len(ws) - 1:
            pre.append(z)
            on = z > 0
            h, dh = np.where(on, z, 0), np.where(on[:, :, None], dz, 0)
        else:
            h, dh = z, dz
    return h[:, 0], dh[:, 0] / carry, pre


def world_gradients(dlog_canonical, jac, density):
    """include/cednerf_hip.h's lines in the inputs' dtype (float32: IEEE single, no contraction):
    dlog = dlog_canonical + J_x^T dlog_canonical, grad = min(density, e^15) * dlog"""
    dc, J = dlog_canonical, jac
    dlog = np.stack([dc[:, b] + ((J[:, 0, b] * dc[:, 0] + J[:, 1, b] * dc[:, 1]) + J[:, 2, b] * dc[:, 2]) for b in range(3)], -1)
    slope = np.minimum(density.reshape(-1), EXP15.astype(dc.dtype))
    return dlog, slope[:, None] * dlog


def canonical_gradient(params, draw, dtype=np.float64):
    """d raw / d x_norm -> dlog_canonical = diag(1 / extent) d raw / d x_norm, extent formed in float32 as the kernel does"""
    aabb = np.asarray(params["aabb"], np.float32)
    return draw / (aabb[3:] - aabb[:3]).astype(dtype)
