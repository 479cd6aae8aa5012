"""A float64 model of the per-ray sums of csrc/composite.hip, its float32 evaluation, rounding bounds and test problems.

Plain numpy, independent of oracle/ and of ced_nerf_amd/.  A problem is ray-packed: packed[r] = (start, count) indexes
the sample arrays t0, t1, sigma [S] and rgb [S, 3]; slots that no ray owns may lie between rays (`gapped`).  The model
pads every ray to the longest one ([n_rays, L] arrays, padding contributes exact zeros) and takes every per-ray prefix
with `cumsum` in forward order:

    dt_i = t1_i - t0_i,  sd_i = sigma_i dt_i,  acc_i = sum_{j<i} sd_j,
    T_i = p exp(-acc_i),  a_i = 1 - exp(-sd_i),  w_i = T_i a_i          (p: a carried-in prefix, 1 - opacity)
    colour = colour_0 + sum_i w_i rgb_i,  opacity = opacity_0 + sum_i w_i,  depth = depth_0 + sum_i w_i (t0_i + t1_i) / 2
    d sigma_i = dt_i (g_i (T_i - w_i) - sum_{k>i} g_k w_k),  d rgb_i = w_i d_colour,
    g_i = <d_colour, rgb_i> + d_opacity + d_depth (t0_i + t1_i) / 2.

Every function takes `dtype`: float64 is the model, float32 is the same statement evaluated honestly in float32 (a
sequential float32 cumsum, numpy's float32 exp) -- what a float32 evaluation costs, with no knowledge of any kernel.

Bounds (u = 2^-24, first order; TINY = 2^-126 is the absolute floor of anything that leaves the normal range).  They
count the roundings of ANY float32 evaluation that sums in forward order, not those of a particular kernel:

  exp     a float32 exp that is good to E_EXP = 6 u relative: a degree-6 Taylor kernel on |r| <= ln2/2 truncates at
          r^7/5040 <= 1.2e-7 = 2.0 u, its Horner chain adds <= 1.5 u (the last step 1 u, the one before |r| u, ...), the
          two-step argument reduction <= 2 u |r| = 0.7 u: 4.2 u, rounded up to 6.  A libm exp is within 1 ulp = 2 u.
  acc_i   sd_j carries 2 roundings (dt, the product), the sum of i terms i - 1 additions: |d acc_i| <= (i + 2) u acc_i.
  T_i     |dT_i| <= T_i (expm1((i + 2) u acc_i) + (E_EXP + 2) u) + TINY; the 2 u are the prefix's own rounding and the
          product with it (present or not).
  a_i     e = exp(-sd): |da_i| <= u (a_i + e (E_EXP + 2 sd_i)) + TINY (argument error 2 u sd, the exp, the subtraction).
  w_i     |dw_i| <= a_i dT_i + T_i da_i + u w_i + TINY.
  sums    out = out_0 + sum of m terms w_i v_i added in order: each term errs by |v_i| (dw_i + 2 u w_i) (v itself may
          carry one rounding -- the midpoint -- and the product one), the m additions by at most
          (m + 1) u (|out_0| + sum |w_i v_i|):  bound = sum_i |v_i| (dw_i + 2 u w_i) + (m + 1) u (|out_0| + sum|w v|).
  g_i     five terms, a product each (the depth term two roundings), four additions: |dg_i| <= 6 u G_i,
          G_i = sum of the absolute terms.
  d sigma dt_i [ |g_i| (dT_i + dw_i + u |T_i - w_i|) + |T_i - w_i| dg_i + u |g_i (T_i - w_i)|
                 + sum_{k>i} (|g_k| dw_k + w_k dg_k + u |g_k| w_k) + m_i u sum_{k>i} |g_k| w_k       (m_i = cnt - 1 - i)
                 + u (|g_i (T_i - w_i)| + sum_{k>i} |g_k| w_k) ] + 2 u |d sigma_i| + TINY
          (the subtraction, the rounding of dt and the last product).
  d rgb   |d_colour| dw_i + u |w_i d_colour| + TINY.
  composite_test  T is a running product: dT' <= (1 - a) dT + T (da + u (1 - a)) + u T' + TINY; a ray is `robust` when
          no decision of its float64 run (a > a_thr, T <= T_thr) lies within the bound of its operands; only robust rays
          are compared with float64 (decisions themselves are compared bit for bit elsewhere).
"""
import zlib

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
E_EXP = 6.0
EPS32 = float(np.finfo(np.float32).eps)
EXP15 = float(np.float32(np.exp(15.0)))         # the ceiling of the field's density activation
SENTINEL = np.uint32(0x7FA5C3E1)                # a NaN payload no kernel produces: marks untouched output slots
LONG_LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 4099)
EDGE_N = (1, 63, 64, 65, 255, 256, 257, 513)
WALL_SIGMAS = (1e3, 1e5, EXP15)
GAP_CAP = 48


class Problem:
    def __init__(self, name, packed, t0, t1, sigma, rgb):
        self.name = name
        self.packed = np.ascontiguousarray(packed, np.int64).reshape(-1, 2)
        self.t0, self.t1, self.sigma, self.rgb = t0, t1, sigma, rgb
        self.n_rays, self.S = self.packed.shape[0], t0.shape[0]
        cnt = self.packed[:, 1]
        self.L = int(cnt.max()) if self.n_rays else 0
        k = np.arange(self.L)[None, :]
        self.valid = k < cnt[:, None]
        self.idx = np.where(self.valid, self.packed[:, :1] + k, 0)
        self.used = np.zeros(self.S, bool)
        self.used[self.idx[self.valid]] = True

    def gather(self, x, dtype):
        out = np.zeros(self.valid.shape + x.shape[1:], dtype)
        out[self.valid] = x[self.idx[self.valid]]
        return out

    def scatter(self, padded, fill=np.nan):
        out = np.full((self.S,) + padded.shape[2:], fill, padded.dtype)
        out[self.idx[self.valid]] = padded[self.valid]
        return out

    def ray_indices(self):
        """[S] ray of every slot, -1 where no ray owns it"""
        return self.scatter(np.broadcast_to(np.arange(self.n_rays)[:, None], self.valid.shape).astype(np.int64), -1)


# ----------------------------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------------------------
def _excl_cumsum(x):
    return np.concatenate([np.zeros_like(x[:, :1]), np.cumsum(x[:, :-1], axis=1, dtype=x.dtype)], axis=1)


def _seq_sum(init, terms):
    """init + terms[:, 0] + terms[:, 1] + ... in that order, in the arrays' dtype"""
    return np.cumsum(np.concatenate([init[:, None], terms], axis=1), axis=1, dtype=terms.dtype)[:, -1]


def forward(pb, prefix=None, dtype=np.float64, per_sample=False):
    """Padded [n_rays, L] dt, tmid, sd, acc, T, a, w.  prefix: None, [n_rays], or [S] with per_sample."""
    dt_ = np.dtype(dtype)
    t0, t1, sg = (pb.gather(x, dt_) for x in (pb.t0, pb.t1, pb.sigma))
    with np.errstate(under="ignore", over="ignore"):
        dt = t1 - t0
        sd = sg * dt
        acc = _excl_cumsum(sd)
        T = np.exp(-acc)
        if prefix is not None:
            p = np.asarray(prefix)
            T = T * (pb.gather(p, dt_) if per_sample else p.astype(dt_)[:, None])
        a = -np.expm1(-sd) if dt_ == np.float64 else dt_.type(1) - np.exp(-sd)
        w = T * a
    v = pb.valid
    return dict(dt=dt, tmid=(t0 + t1) / dt_.type(2), sd=sd, acc=acc, T=np.where(v, T, 0), a=np.where(v, a, 0),
                w=np.where(v, w, 0))


def forward_bounds(f):
    """dT, da, dw of a float64 `forward` result"""
    i = np.arange(f["T"].shape[1])[None, :]
    with np.errstate(under="ignore"):
        dT = f["T"] * (np.expm1(np.minimum((i + 2) * U * f["acc"], 700.0)) + (E_EXP + 2) * U) + TINY
        e = np.exp(-f["sd"])
        da = U * (f["a"] + e * (E_EXP + 2 * f["sd"])) + TINY
        dw = f["a"] * dT + f["T"] * da + U * f["w"] + TINY
    return dT, da, dw


def sum_bound(w, dw, v, out0, cnt):
    """bound of out0 + sum_i w_i v_i (v None: 1); w, dw, v padded float64"""
    av = 1.0 if v is None else np.abs(v)
    return (av * (dw + 2 * U * w)).sum(1) + (cnt + 1) * U * (np.abs(out0) + (av * w).sum(1))


def composite(pb, state=None, dtype=np.float64, want_bounds=False):
    """Per-ray colour [n, 3], opacity [n], depth [n]; state = carried-in (rgb [n, 3], opacity [n], depth [n]), whose
    opacity also gives the prefix 1 - opacity.  Rays without samples keep their state."""
    dt_ = np.dtype(dtype)
    n = pb.n_rays
    if state is None:
        rgb0, op0, dp0 = np.zeros((n, 3), dt_), np.zeros(n, dt_), np.zeros(n, dt_)
        prefix = None
    else:
        rgb0, op0, dp0 = (np.asarray(x).astype(dt_) for x in state)
        prefix = dt_.type(1) - op0
    f = forward(pb, prefix, dt_)
    c = pb.gather(pb.rgb, dt_)
    w = f["w"]
    out = dict(f=f, rgb=np.stack([_seq_sum(rgb0[:, k], w * c[:, :, k]) for k in range(3)], 1),
               opacity=_seq_sum(op0, w), depth=_seq_sum(dp0, w * f["tmid"]))
    if want_bounds:
        _, _, dw = forward_bounds(f)
        cnt = pb.packed[:, 1]
        out["bounds"] = dict(rgb=np.stack([sum_bound(w, dw, c[:, :, k], rgb0[:, k], cnt) for k in range(3)], 1),
                             opacity=sum_bound(w, dw, None, op0, cnt), depth=sum_bound(w, dw, f["tmid"], dp0, cnt))
    return out


def accumulate(pb, weights, values, out0, dtype=np.float64):
    """out0 [n, C] + sum_i weights_i values_i (values None: C = 1) and, for float64, its bound (m + 2) u sum|term|."""
    dt_ = np.dtype(dtype)
    w = pb.gather(weights, dt_)[:, :, None]
    term = w if values is None else w * pb.gather(values, dt_)
    out = np.stack([_seq_sum(out0[:, k].astype(dt_), term[:, :, k]) for k in range(out0.shape[1])], 1)
    bound = (pb.packed[:, 1:2] + 2) * U * (np.abs(out0) + np.abs(term).sum(1)) + TINY
    return out, bound


def finalize(bkgd, rgb, opacity, depth, dtype=np.float64):
    """(rgb + bkgd (1 - opacity), depth / max(opacity, eps32)) and their bounds (three roundings; one)."""
    dt_ = np.dtype(dtype)
    rgb, op, dp = (np.asarray(x).astype(dt_) for x in (rgb, opacity, depth))
    out = rgb
    b_rgb = np.zeros(rgb.shape)
    if bkgd is not None:
        part = np.asarray(bkgd).astype(dt_)[None, :] * (dt_.type(1) - op)[:, None]
        out = rgb + part
        b_rgb = U * (np.abs(out) + 2 * np.abs(part)) + TINY
    d = dp / np.maximum(op, dt_.type(EPS32))
    return out, d, b_rgb, U * np.abs(d) + TINY


def composite_test(pb, alive, opacity, depth, rgb, T_thr, a_thr, dtype=np.float64):
    """The test-time recurrence: per entry n of `alive` (ray alive[n], samples packed[n]): T = 1 - opacity[ray]; for
    each sample with a > a_thr: accumulate w = a T, T <- T (1 - a), stop (alive[n] = -1) once T <= T_thr.  An entry
    without samples only gets alive[n] = -1.  -> dict: alive, opacity, depth, rgb (new arrays), bounds (per output),
    robust [n] (see the module docstring), stopped [n] (the entry ran into T <= T_thr)."""
    dt_ = np.dtype(dtype)
    one = dt_.type(1)
    n = pb.n_rays
    cnt = pb.packed[:, 1]
    t0, t1, sg = (pb.gather(x, dt_) for x in (pb.t0, pb.t1, pb.sigma))
    cs = pb.gather(pb.rgb, dt_)
    op_in = np.asarray(opacity).astype(dt_).reshape(-1)
    T = one - op_in[alive]
    dT = U * np.abs(T) + TINY
    stopped = np.zeros(n, bool)
    fragile = np.zeros(n, bool)
    acc = np.zeros((n, 5), dt_)                          # r, g, b, depth, opacity
    absum = np.zeros((n, 5)); prop = np.zeros((n, 5)); m = np.zeros(n)
    T_thr, a_thr = dt_.type(np.float32(T_thr)), dt_.type(np.float32(a_thr))
    with np.errstate(under="ignore", over="ignore"):
        for k in range(pb.L):
            live = pb.valid[:, k] & ~stopped
            sd = sg[:, k] * (t1[:, k] - t0[:, k])
            e = np.exp(-sd)
            a = one - e
            act = live & (a > a_thr)
            w = a * T
            v = np.stack([cs[:, k, 0], cs[:, k, 1], cs[:, k, 2], (t0[:, k] + t1[:, k]) / dt_.type(2), np.ones(n, dt_)], 1)
            acc = np.where(act[:, None], acc + w[:, None] * v, acc)
            Tn = T * (one - a)
            # bounds
            da = U * (np.abs(a) + e * (E_EXP + 2 * np.abs(sd))) + TINY
            fragile |= live & (np.abs(a - a_thr) <= da)
            dw = a * dT + T * da + U * w + TINY
            absum += np.where(act[:, None], np.abs(w[:, None] * v), 0)
            prop += np.where(act[:, None], np.abs(v) * (dw + 2 * U * w)[:, None], 0)
            m += act
            dTn = (one - a) * dT + T * (da + U * (one - a)) + U * Tn + TINY
            fragile |= act & (np.abs(Tn - T_thr) <= dTn)
            T = np.where(act, Tn, T); dT = np.where(act, dTn, dT)
            stopped |= act & (T <= T_thr)
    alive_out = np.where(stopped | (cnt == 0), -1, alive)
    has = cnt > 0
    outs, bounds = [], []
    for base, cols in ((opacity, [4]), (depth, [3]), (rgb, [0, 1, 2])):
        o = np.asarray(base).astype(dt_).reshape(-1, len(cols)).copy()
        b = np.zeros(o.shape)
        o[alive[has]] = o[alive[has]] + acc[has][:, cols]
        b[alive[has]] = prop[has][:, cols] + (m[has, None] + 1) * U * absum[has][:, cols] + U * np.abs(o[alive[has]]) + TINY
        outs.append(o); bounds.append(b)
    return dict(alive=alive_out, opacity=outs[0], depth=outs[1], rgb=outs[2], robust=~fragile, stopped=stopped,
                bounds=dict(opacity=bounds[0], depth=bounds[1], rgb=bounds[2]))


def backward(pb, d_color, d_opacity=None, d_depth=None, dtype=np.float64, want_bounds=False):
    """-> d_sigma [S], d_rgb [S, 3] (NaN in slots no ray owns) and, with want_bounds, their bounds (same layout) and
    the absolute sum of d_sigma's terms."""
    dt_ = np.dtype(dtype)
    n = pb.n_rays
    f = forward(pb, None, dt_)
    c = pb.gather(pb.rgb, dt_)
    dc = np.asarray(d_color).astype(dt_)
    dop = np.zeros(n, dt_) if d_opacity is None else np.asarray(d_opacity).astype(dt_).reshape(-1)
    ddp = np.zeros(n, dt_) if d_depth is None else np.asarray(d_depth).astype(dt_).reshape(-1)
    T, a, w, dt, tmid = f["T"], f["a"], f["w"], f["dt"], f["tmid"]
    terms = [dc[:, None, 0] * c[:, :, 0], dc[:, None, 1] * c[:, :, 1], dc[:, None, 2] * c[:, :, 2],
             np.broadcast_to(dop[:, None], T.shape), ddp[:, None] * tmid]
    g = np.where(pb.valid, (((terms[0] + terms[1]) + terms[2]) + terms[3]) + terms[4], 0)

    def suffix(x):                                       # sum_{k>i} x_k, summed from the ray's end
        inc = np.cumsum(x[:, ::-1], axis=1, dtype=x.dtype)[:, ::-1]
        return np.concatenate([inc[:, 1:], np.zeros_like(x[:, :1])], axis=1)

    with np.errstate(under="ignore", over="ignore"):
        TW = T * np.exp(-f["sd"]) if dt_ == np.float64 else T - w
        TW = np.where(pb.valid, TW, 0)
        d_sig = dt * (g * TW - suffix(g * w))
        d_rgb = w[:, :, None] * dc[:, None, :]
    out = [pb.scatter(d_sig), pb.scatter(d_rgb)]
    if want_bounds:
        dT, da, dw = forward_bounds(f)
        G = np.where(pb.valid, sum(np.abs(t) for t in terms), 0)
        dg = 6 * U * G
        ag = np.abs(g)
        X1 = ag * np.abs(TW)
        dX1 = ag * (dT + dw + U * np.abs(TW)) + np.abs(TW) * dg + U * X1
        m_i = np.maximum(pb.packed[:, 1:2] - 1 - np.arange(pb.L)[None, :], 0)
        S_abs = suffix(ag * w)
        dS = suffix(np.where(pb.valid, ag * dw + w * dg + U * ag * w, 0)) + m_i * U * S_abs
        b_sig = np.abs(dt) * (dX1 + dS + U * (X1 + S_abs)) + 2 * U * np.abs(d_sig) + TINY
        b_rgb = np.abs(dc)[:, None, :] * dw[:, :, None] + U * np.abs(d_rgb) + TINY
        A = np.abs(dt) * (ag * (T + w) + S_abs)            # the absolute sum of d sigma_i's terms
        out += [pb.scatter(b_sig), pb.scatter(b_rgb), pb.scatter(A)]
    return tuple(out)


# ----------------------------------------------------------------------------------------------------------------------
# problems: shape families x density regimes, each a pure function of (names, seed)
# ----------------------------------------------------------------------------------------------------------------------
def _rng(seed, *names):
    return np.random.default_rng([int(seed)] + [zlib.crc32(s.encode()) for s in names])


def wall_layout(r, cnt):
    """(first wall sample, wall length, wall sigma) of ray r with cnt samples: the wall ends the ray (r % 3 == 0), sits in
    its middle (1) or starts it (2)"""
    length = np.minimum(cnt, 8 + r % 5)
    start = np.where(r % 3 == 0, cnt - length, np.where(r % 3 == 1, (cnt - length) // 2, 0))
    return start, length, np.asarray(WALL_SIGMAS)[(r // 3) % 3]


def shape_counts(shape, seed=0):
    """-> (counts [n_rays], cap or None): cap = slots per ray of a gapped layout"""
    rng = _rng(seed, "shape", shape)
    if shape.startswith("edge"):
        n = int(shape[4:])
        counts = rng.integers(0, 41, size=n)
        counts[rng.uniform(size=n) < 0.3] = 0
        if n >= 63:
            counts[-1] = 40; counts[0] = 0; counts[1] = 1       # the last lane of the grid works, the first does not
        return counts, None
    if shape == "long":
        return np.tile(np.asarray(LONG_LENGTHS), 4), None
    if shape == "all_empty":
        return np.zeros(300, np.int64), None
    if shape == "gapped":
        counts = rng.integers(0, GAP_CAP + 1, size=130)
        counts[:4] = (GAP_CAP, 0, 1, GAP_CAP)
        return counts, GAP_CAP
    if shape == "wallrays":
        r = np.arange(96)
        pre = rng.integers(20, 41, size=96)
        wall = 8 + r % 5
        post = rng.integers(5, 21, size=96)
        # r % 3 == 0: pre + wall; 1: the wall in the middle of pre + wall + pre (+ 0); 2: wall + post
        return np.where(r % 3 == 0, pre + wall, np.where(r % 3 == 1, 2 * pre + wall, wall + post)), None
    raise KeyError(shape)


def make(shape, regime, seed=0):
    counts, cap = shape_counts(shape, seed)
    counts = np.asarray(counts, np.int64)
    n = counts.shape[0]
    starts = np.arange(n) * cap if cap else np.cumsum(counts) - counts
    S = n * cap if cap else int(counts.sum())
    L = int(counts.max()) if n else 0
    k = np.arange(L)[None, :]
    valid = k < counts[:, None]
    r = np.arange(n)[:, None]
    rng = _rng(seed, "regime", shape, regime)
    u = lambda lo, hi: rng.uniform(lo, hi, size=(n, L))
    if regime in ("mixed", "zeros"):                    # the law of test_gpu_parity._packed_problem, sorted per ray
        t0 = np.sort(np.where(valid, u(0, 5), np.inf), axis=1)
        dt = u(1e-3, 2e-2)
        sg = u(0, 1) ** 4 * 300
        if regime == "zeros":
            sg[(r % 4 == 0) & (k >= 0)] = 0.0
            third = counts[:, None] // 3
            sg[(r % 4 == 1) & (k >= third) & (k < 2 * third)] = 0.0
            dt[u(0, 1) < 0.1] = 0.0
    elif regime == "thin":
        t0 = np.sort(np.where(valid, u(0, 5), np.inf), axis=1)
        dt = u(1e-3, 2e-2)
        sg = u(0, 1) * 0.049 / (np.maximum(counts, 1)[:, None] * dt)
    elif regime == "saturated":
        t0 = np.sort(np.where(valid, u(0, 5), np.inf), axis=1)
        dt = u(1e-3, 2e-2)
        sg = u(220, 400) / dt
    elif regime == "wall":
        t0 = u(0.5, 2.0)[:, :1] + k * 6e-3
        dt = 5e-3 * u(0.9, 1.1)
        sg = u(0, 2)
        ws, wl, wsig = wall_layout(r, counts[:, None])
        in_wall = (k >= ws) & (k < ws + wl)
        sg = np.where(in_wall, wsig, sg)
    else:
        raise KeyError(regime)
    t0 = np.where(valid, t0, 0).astype(np.float32)
    t1 = (t0.astype(np.float64) + dt).astype(np.float32)
    if regime == "zeros":
        t1 = np.where(dt == 0.0, t0, t1)
    rgb = rng.uniform(0, 1, size=(n, L, 3))
    pb = Problem(f"{shape}/{regime}", np.stack([starts, counts], -1), np.zeros(S, np.float32), np.zeros(S, np.float32),
                 np.zeros(S, np.float32), np.zeros((S, 3), np.float32))
    fill = np.float32(np.nan)
    pb.t0, pb.t1, pb.sigma, pb.rgb = (pb.scatter(x.astype(np.float32), fill) for x in (t0, t1, sg, rgb))
    return pb


def ray_state(pb, seed=0):
    """carried-in (rgb [n, 3], opacity [n], depth [n]), float32"""
    rng = _rng(seed, "state", pb.name)
    op = rng.uniform(0, 0.9, size=pb.n_rays).astype(np.float32)
    return ((rng.uniform(0, 1, size=(pb.n_rays, 3)) * op[:, None]).astype(np.float32), op,
            (rng.uniform(0, 4, size=pb.n_rays) * op).astype(np.float32))


def stepper_setup(pb, seed=0):
    """composite_test's inputs: -> (problem, alive [n] (distinct rays of n + 50), opacity [N, 1], depth [N, 1],
    rgb [N, 3], stop_rays).  Up to three rays with >= 3 samples are made to stop exactly at their first, a middle and
    their last sample: nothing before it passes the alpha threshold, and it is opaque."""
    rng = _rng(seed, "test_time", pb.name)
    t0, t1, sg = pb.t0.copy(), pb.t1.copy(), pb.sigma.copy()
    rays = np.flatnonzero(pb.packed[:, 1] >= 3)[:3]
    for j, r in enumerate(rays):
        s0, c = pb.packed[r]
        p = (0, c // 2, c - 1)[j]
        sg[s0:s0 + p] = 0.0
        t1[s0 + p] = np.float32(t0[s0 + p] + np.float32(5e-3))
        sg[s0 + p] = 1e5
    n_total = pb.n_rays + 50
    alive = rng.permutation(n_total)[:pb.n_rays].astype(np.int64)
    q = Problem(pb.name + "/test_time", pb.packed, t0, t1, sg, pb.rgb)
    return (q, alive, rng.uniform(0, 0.5, size=(n_total, 1)).astype(np.float32),
            rng.uniform(0, 1, size=(n_total, 1)).astype(np.float32), rng.uniform(0, 1, size=(n_total, 3)).astype(np.float32), rays)


T_THR, A_THR = 1e-2, 1e-3


def worst(got, want, bound, mask=None):
    """max |got - want| / bound over mask (0 when the mask is empty); NaN or inf in got counts as infinite"""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
    m = np.ones(got.shape, bool) if mask is None else np.broadcast_to(mask, got.shape)
    if not m.any():
        return 0.0
    if not np.isfinite(got[m]).all():
        return np.inf
    err, b = np.abs(got[m] - want[m]), bound[m]
    if not (err[b == 0] == 0).all() or np.isnan(err).any() or np.isnan(b).any():      # a zero bound asks for equality
        return np.inf
    return float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0


GRADS = ("all", "color", "opacity", "depth")


def ray_grads(pb, which, seed=0):
    """(d_color [n, 3], d_opacity [n], d_depth [n]) float32 normal variates; all three, or one with the others zero"""
    rng = _rng(seed, "grads", pb.name)
    g = [rng.normal(size=(pb.n_rays, 3)).astype(np.float32), rng.normal(size=pb.n_rays).astype(np.float32),
         rng.normal(size=pb.n_rays).astype(np.float32)]
    if which != "all":
        keep = GRADS.index(which) - 1
        g = [x if i == keep else np.zeros_like(x) for i, x in enumerate(g)]
    return tuple(g)


SHAPES = tuple(f"edge{n}" for n in EDGE_N) + ("long", "all_empty", "gapped", "wallrays")
REGIMES = ("thin", "mixed", "zeros", "saturated", "wall")
# forward: every shape with the mixed law, the long rays and the wave-edge grid with every regime, the walls
FORWARD_CASES = tuple((s, "mixed") for s in SHAPES) + tuple(("long", g) for g in REGIMES if g != "mixed") + \
    tuple(("edge257", g) for g in REGIMES if g != "mixed") + (("gapped", "zeros"), ("gapped", "saturated"),
                                                              ("wallrays", "wall"))
BACKWARD_CASES = tuple((s, g) for s in SHAPES for g in REGIMES)


# ----------------------------------------------------------------------------------------------------------------------
# reduce_along_rays
# ----------------------------------------------------------------------------------------------------------------------
RUN_LENGTHS = (1, 63, 64, 65, 200, 1025)
REDUCE_N = (1, 63, 64, 65, 257)


def reduce_problem(n_rays, C, weights, seed=0):
    """Packed runs whose lengths cycle through RUN_LENGTHS over the rays that have samples (every seventh ray of a
    problem with more than 3 rays has none).  -> ray_indices [S], values [S, C], weights (None, [S, 1] or [S, C])"""
    rng = _rng(seed, "reduce", str(n_rays), str(C), str(weights))
    lens = np.asarray([RUN_LENGTHS[(r + n_rays) % len(RUN_LENGTHS)] for r in range(n_rays)])
    if n_rays > 3:
        lens[4::7] = 0
    if n_rays > 64:
        lens[70:] = np.minimum(lens[70:], 65)           # keeps S small; the long runs sit in the first rays
    ri = np.repeat(np.arange(n_rays), lens).astype(np.int64)
    S = ri.shape[0]
    vals = rng.normal(size=(S, C)).astype(np.float32)
    w = None if weights == "none" else rng.uniform(-1, 2, size=(S, 1 if weights == "one" else C)).astype(np.float32)
    return ri, vals, w


def reduce64(ri, vals, w, n_rays, mean):
    """float64 np.add.at; -> out [n_rays, C], bound (m_r + 2) u sum|term| (+ the mean's division), counts m_r"""
    term = vals.astype(np.float64) * (1.0 if w is None else w.astype(np.float64))
    out = np.zeros((n_rays, vals.shape[1])); ab = np.zeros_like(out)
    np.add.at(out, ri, term); np.add.at(ab, ri, np.abs(term))
    m = np.bincount(ri, minlength=n_rays)
    bound = (m[:, None] + 2) * U * ab
    if mean:
        out = out / (m[:, None] + 1); bound = bound / (m[:, None] + 1) + U * np.abs(out)
    return out, bound + TINY, m
