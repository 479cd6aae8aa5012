"""numpy statements of the level-set entries, for tests/test_level_set_cpu.py and tests/test_gpu_level_set.py.

* `first_crossing`: ced_surface_first_crossing's definition (include/cednerf_hip.h), sample by sample.
* `bisect_f32`: ced_field_level_set's lines in numpy float32 (IEEE single, no contraction) on a caller-supplied f.
* `raw64` / `raw_model`: the pre-activation density minus one -- log(sigma) -- of the float64 model (tests/density64.py
  behind tests/warp64.py's move), -inf outside the box; `raw_model` also with the operands rounded as an mlp_precision
  rounds them.
"""
import numpy as np

import density64 as D
import warp64 as W


def first_crossing(packed, t0, t1, sigma, thresh):
    """packed [N,2] int64, t0 / t1 / sigma [S] float32 -> (k [N] int64, lo [N] float32, hi [N] float32)"""
    packed = np.asarray(packed, np.int64).reshape(-1, 2)
    t0, t1, sigma = (np.asarray(a, np.float32) for a in (t0, t1, sigma))
    n = packed.shape[0]
    k = np.full(n, -1, np.int64)
    lo = np.zeros(n, np.float32)
    hi = np.zeros(n, np.float32)
    two = np.float32(2.0)
    for r in range(n):
        s0, cnt = int(packed[r, 0]), int(packed[r, 1])
        for i in range(s0, s0 + cnt):
            if sigma[i] >= np.float32(thresh):                           # False for a NaN
                k[r] = i
                hi[r] = np.float32(t0[i] + t1[i]) / two
                if i > s0 and t1[i - 1] == t0[i]:
                    lo[r] = np.float32(t0[i - 1] + t1[i - 1]) / two
                else:
                    lo[r] = t0[i]
                break
    return k, lo, hi


def bisect_f32(f, o, d, lo, hi, thresh, max_iters, tol):
    """f(points [n,3] float32) -> sigma [n] float32.  o / d [n,3], lo / hi [n] -> dict(t, x, sigma, width, status, evals,
    lo): the header's lines, every operation rounded to float32; `lo` is the bracket's lower end at the stop."""
    f32 = np.float32
    o, d = np.asarray(o, f32), np.asarray(d, f32)
    lo, hi = np.asarray(lo, f32).copy(), np.asarray(hi, f32).copy()
    thresh, tol, two = f32(thresh), f32(tol), f32(2.0)

    def point(t):
        return (o + (d * t[:, None]).astype(f32)).astype(f32)

    with np.errstate(invalid="ignore", over="ignore"):
        s_lo = np.asarray(f(point(lo)), f32)
        s_hi = np.asarray(f(point(hi)), f32)
        n = lo.shape[0]
        evals = np.full(n, 2, np.int32)
        status = np.where(s_lo >= thresh, 1, np.where(~(s_hi >= thresh), 2, 0)).astype(np.int32)
        active = status == 0
        for _ in range(int(max_iters)):
            width = (hi - lo).astype(f32)
            m = ((lo + hi).astype(f32) / two).astype(f32)
            active = active & ~((width <= tol) | (m == lo) | (m == hi))
            if not active.any():
                break
            s = np.asarray(f(point(m)), f32)
            up = active & (s >= thresh)                                  # a NaN goes to lo
            down = active & ~up
            hi = np.where(up, m, hi)
            s_hi = np.where(up, s, s_hi)
            lo = np.where(down, m, lo)
            evals = evals + active.astype(np.int32)
        inside = status == 1
        t = np.where(inside, lo, hi).astype(f32)
        return dict(t=t, x=point(t), sigma=np.where(inside, s_lo, s_hi).astype(f32),
                    width=np.where(inside, f32(0.0), (hi - lo).astype(f32)).astype(f32), status=status, evals=evals, lo=lo)


def _mlp(ws, h, rnd):
    """warp64.move_jacobian's / density64.base_gradient's primal chain: every layer's operands through `rnd`"""
    ws = [rnd(np.asarray(w, np.float64)) for w in ws]
    for i, w in enumerate(ws):
        h = rnd(h) @ w.T
        if i < len(ws) - 1:
            h = np.maximum(h, 0)
    return h


def raw_model(params, x, t, mode=None):
    """log(sigma) = raw - 1 at positions x [n,3], times t [n], in float64; mode: an mlp_precision whose operand rounding
    the motion network and mlp_base apply (None: none).  -inf outside the box.  The primal halves of
    warp64.move_jacobian and density64.base_gradient, on their features, without the tangents."""
    x = np.asarray(x, np.float64)
    t = np.asarray(t, np.float64).reshape(-1)
    h = _mlp(params["xyz_wrap"], W.features(np.concatenate([x, t[:, None]], -1), np.float64),
             W.rounder(None if mode is None else W.MOTION_MODES[mode], np.float64))
    step = np.float64(np.float32(params["moving_step"]))
    move = (h[:, :3] + np.tanh(h[:, 3:]) if params["use_div_offsets"] else h) * step
    aabb = np.asarray(params["aabb"], np.float32).astype(np.float64)
    xn = ((x + move) - aabb[:3]) / (aabb[3:] - aabb[:3])
    inside = ((xn > 0) & (xn < 1)).all(-1)
    raw = np.full(len(x), -np.inf)
    if inside.any():
        xi, ti = np.clip(xn[inside], 0.0, 1.0).astype(np.float32), t[inside].astype(np.float32)
        feats = hash_features64(params, xi, ti)
        if params["time_mode"]:
            mnorm = np.sqrt((move[inside] * move[inside]).sum(-1))
            feats = np.concatenate([feats, D.time_features(params["time_mode"], ti, mnorm, np.float64)], 1)
        raw[inside] = _mlp(params["mlp_base"], feats, W.rounder(None if mode is None else D.BASE_MODES[mode], np.float64))[:, 0] - 1.0
    return raw


def hash_features64(params, x_norm, t):
    """density64.hash_features' features (same cells, same fp32 fractions, float64 interpolation) without their tangents"""
    lv = D.levels_of(params)
    table = np.asarray(params["hash"]["table"]).astype(np.float64)
    n = x_norm.shape[0]
    temporal = bool(params["hash"].get("temporal", False))
    if temporal:
        ts = np.asarray(t, np.float32) * np.float32(3.0)
        fl = np.floor(ts)
        k = np.minimum(fl, np.float32(2.0)).astype(np.int64)
        tf = (ts - fl).astype(np.float64)[:, None]
        table = table.reshape(-1, 4, 2)
    rows = np.arange(n)
    feats = []
    for l in range(int(lv["n_levels"])):
        pos32 = x_norm.astype(np.float32) * np.float32(lv["scale"][l]) + np.float32(0.5)
        g32 = np.floor(pos32)
        g = g32.astype(np.int64)
        frac = (pos32 - g32).astype(np.float64)
        w = np.stack([1 - frac, frac], 0)
        f = np.zeros((n, 2))
        for c in range(8):
            bits = [(c >> a) & 1 for a in range(3)]
            idx = D._corner_index(lv, l, g + np.asarray(bits, np.int64))
            v = table[idx]
            if temporal:
                v = v[rows, k] * (1 - tf) + v[rows, k + 1] * tf
            f += ((w[bits[0], :, 0] * w[bits[1], :, 1]) * w[bits[2], :, 2])[:, None] * v
        feats.append(f)
    return np.concatenate(feats, 1)


def raw64(params, x, t):
    return raw_model(params, x, t, None)
