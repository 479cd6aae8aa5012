"""The per-ray sums of csrc/composite.hip against tests/composite64.py at hard ray shapes.

Shapes (composite64.SHAPES): n_rays at grid and wave edges (1, 63, 64, 65, 255, 256, 257, 513; 30 % empty rays), rays of
0 .. 4099 samples, 300 empty rays, rays with unused (NaN-filled) slots between them, rays that run into a wall.  Density
regimes: thin, the mixed law of test_gpu_parity, exact zeros (sigma and dt), saturated (a = 1, T = 0), walls of
sigma = 1e3, 1e5, e^15 behind 20-40 thin samples.

composite_prefix_ and composite_step_ run composite_core.hpp's composite_ray on walk_samples<4> -- the frame renderer's
loop (frame_composite_kernel) -- so these cases are the hard-shape test of that walker too: edge257 and edge513 hold every
per-ray count 0 .. 12, long holds 0, 1, 3, 4, 5, 63 .. 65, ..., 4099 (whole batches, batches plus a one-by-one rest, no
batch at all; test_composite64_cpu.py asserts the counts).

Forward kernels, two checks per case:
 (a) bit for bit against the C oracle: weights / transmittance / alpha with and without a per-sample prefix,
     accumulate_along_rays_, the visibility mask, composite_test; composite_prefix_ and composite_step_ against the
     oracle's weights (prefix 1 - opacity[ray]) followed by its accumulate into the carried-in colour, opacity and depth
     ("same operation order as the unfused sequence"), composite_step_'s mask and counters from those bits,
     finalize_pixels_ against its three float32 lines in numpy.  Per-sample outputs are pre-filled with a sentinel bit
     pattern, which every slot outside [start, start + cnt) must still hold.
 (b) against float64 within the bounds derived in composite64's docstring, which the model's own float32 evaluation
     meets on the CPU (test_composite64_cpu.py).  In short, with u = 2^-24 and an exp good to 6 u:
       T_i      T_i (expm1((i + 2) u acc_i) + 8 u)         the float32 prefix sum's absolute error, the exp, the prefix
       a_i      u (a_i + e^-sd (6 + 2 sd_i))
       w_i      a_i dT_i + T_i da_i + u w_i
       sums     sum_i |v_i| (dw_i + 2 u w_i) + (m + 1) u (|out_0| + sum |w_i v_i|)     (accumulate alone: (m + 2) u sum|term|)
       d sigma  dt_i [ |g_i| (dT_i + dw_i + u |T_i - w_i|) + |T_i - w_i| 6 u G_i + sum_{k>i} (|g_k| dw_k + 6 u G_k w_k)
                + (m_i + 2) u sum_{k>i} |g_k| w_k + 2 u |g_i (T_i - w_i)| ] + 2 u |d sigma_i|
       d rgb    |d_colour| dw_i + u |w_i d_colour|
     Decisions (visibility, ray_mask, alive) are compared through (a) only; composite_test is compared with float64 on
     the rays none of whose decisions lies within the bound of its operands.

Backward: ops.composite_backward on every shape x regime with random d_colour, d_opacity, d_depth and each alone: d sigma
and d rgb within their bounds, exact zeros in d rgb where the forward weight is 0, nothing but finite numbers, sentinels
untouched outside the rays' samples, and d rgb == fl32(w_i d_colour) bit for bit with the forward kernel's w.

reduce_along_rays: packed runs of 1 .. 1025 equal indices, n in {1, 63, 64, 65, 257}, sum and mean, weights none / one
column / per channel, C in {1, 3, 5}, against float64 np.add.at within (m_r + 2) u sum|term|, the same inputs shuffled,
and the mean's divisor exact.

Every test prints its figures (FWD64 / BWD / REDUCE: the largest error / bound).  Measured on an MI355X:
  forward (b), the largest error / bound per case over T, a, w (with and without prefix), accumulate, composite_prefix_ /
    composite_step_ (fresh and carried-in state) and composite_test: at most 0.73 (composite_test's colour on
    edge257/saturated; 0.69 gapped/saturated), elsewhere at most 0.48; the per-sample T, a, w at most 0.33.
    finalize_pixels_ sits at its bound by construction, 0.69 .. 0.997: its depth is ONE division, whose bound u |d| is
    the rounding itself (half an ulp of a value just above a power of two), its colour three roundings.
  backward, error / bound, the largest over the shapes and the four gradient sets, d sigma / d rgb:
      regime      this kernel       the parent kernel (prefix recovered by subtracting back from the total, __expf)
      thin        0.14 / 0.08       0.15 / 0.12
      mixed       0.20 / 0.31       4.1 / 176         (long/mixed; edge*/mixed 0.1 .. 1.2 / 0.5 .. 6.8)
      zeros       0.20 / 0.28       6.3 / 422
      saturated   5e-89 / 9e-59     the same (T underflows to 0 in both)
      wall        0.19 / 0.29       1.2e4 / 3.6e4
    the wall cases one by one (d sigma / d rgb; this kernel | parent):
      edge1     0.04 / 0.07 | 0.15 / 0.70  (a single ray, the wall its last samples: sigma = 1e3, total depth 50)
      edge63    0.07 / 0.19 | 6.5e3 / 2.0e4      edge64    0.15 / 0.25 | 2.4e3 / 1.2e4      edge65    0.14 / 0.20 | 4.8e3 / 2.2e4
      edge255   0.15 / 0.19 | 1.2e4 / 3.6e4      edge256   0.16 / 0.20 | 6.4e3 / 2.7e4      edge257   0.11 / 0.21 | 9.2e3 / 3.1e4
      edge513   0.17 / 0.29 | 9.1e3 / 3.2e4      long      0.08 / 0.17 | 4.4e3 / 2.1e4      gapped    0.15 / 0.22 | 6.2e3 / 2.7e4
      wallrays  0.19 / 0.22 | 8.8e3 / 2.4e4
    The parent's d rgb differed from fl32(w d_colour) of the forward kernel's w at 502 492 elements over the 60 cases (none
    in `saturated`); this kernel's at none.
  reduce_along_rays: at most 0.33 of the bound (n = 65, C = 5, per-channel weights, runs of up to 1025), packed or shuffled.
  Also found at the new shapes: ced_composite_test refused an empty sample set (NULL sample arrays with n_alive > 0, as
  all_empty gives) instead of setting every entry to -1; it now asks only for the arrays it reads.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import composite64 as M
from conftest import assert_bitexact

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BKGD = np.float32([0.2, 0.5, 0.9])
OPC_THRES = 0.95


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def _cases(cases):
    return [pytest.param(s, g, id=f"{s}-{g}") for s, g in cases]


@functools.lru_cache(maxsize=None)
def _problem(shape, regime):
    return M.make(shape, regime)


def _dev(pb):
    return T(pb.packed), T(pb.t0), T(pb.t1), T(pb.sigma), T(pb.rgb)


def _sentinel(*shape):
    return torch.full(shape, int(M.SENTINEL), dtype=torch.int32, device=DEV).view(torch.float32)


def _untouched(t, pb, name):
    """every slot no ray owns still holds the sentinel"""
    bits = N(t.view(torch.int32)).view(np.uint32)
    assert (bits[~pb.used] == M.SENTINEL).all(), f"{name}: a slot outside every ray's [start, start + cnt) was written"


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _weights(pb, D, prefix=None):
    """ced_render_weights into sentinel-filled outputs"""
    from ced_nerf_amd import _lib
    w, tr, al = _sentinel(pb.S), _sentinel(pb.S), _sentinel(pb.S)
    if pb.S:
        _lib.check(_lib.lib().ced_render_weights(pb.n_rays, _ptr(D[0]), _ptr(D[1]), _ptr(D[2]), _ptr(D[3]), _ptr(prefix),
                                                 _ptr(w), _ptr(tr), _ptr(al), _stream()), "render_weights")
    return w, tr, al


def _backward(pb, D, grads):
    """ced_composite_backward into sentinel-filled outputs"""
    from ced_nerf_amd import _lib
    ds, dr = _sentinel(pb.S), _sentinel(pb.S, 3)
    if pb.S:
        _lib.check(_lib.lib().ced_composite_backward(pb.n_rays, _ptr(D[0]), _ptr(D[1]), _ptr(D[2]), _ptr(D[3]), _ptr(D[4]),
                                                     _ptr(grads[0]), _ptr(grads[1]), _ptr(grads[2]), _ptr(ds), _ptr(dr),
                                                     _stream()), "composite_backward")
    return ds, dr


def _n_samples_iter(pb):
    cnt = pb.packed[:, 1]
    return int(np.bincount(cnt[cnt > 0]).argmax()) if (cnt > 0).any() else 1


def _state(pb):
    """carried-in colour, opacity, depth; every third ray, and every second of those with n_samples_iter samples, is
    already over the opacity threshold"""
    rgb0, op0, dp0 = M.ray_state(pb)
    op0 = op0.copy(); op0[::3] = np.float32(0.97)
    op0[np.flatnonzero(pb.packed[:, 1] == _n_samples_iter(pb))[::2]] = np.float32(0.97)
    return rgb0, op0, dp0


def _expected_composite(oracle, pb, rgb0, op0, dp0):
    """the unfused sequence from the oracle's pieces: weights with prefix 1 - opacity[ray], three accumulates"""
    ri = pb.ray_indices()
    prefix = np.where(ri >= 0, (np.float32(1) - op0)[np.maximum(ri, 0)], np.float32(np.nan)).astype(np.float32)
    w, _, _ = oracle.render_weight_from_density(pb.t0, pb.t1, pb.sigma, pb.packed, prefix)
    tmid = ((pb.t0 + pb.t1) / np.float32(2))[:, None]
    return (oracle.accumulate_along_rays_(w, pb.rgb, pb.packed, rgb0.copy()),
            oracle.accumulate_along_rays_(w, None, pb.packed, op0[:, None].copy())[:, 0],
            oracle.accumulate_along_rays_(w, tmid, pb.packed, dp0[:, None].copy())[:, 0])


# ----------------------------------------------------------------------------------------------------------------------
# forward (a): bit for bit
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,regime", _cases(M.FORWARD_CASES))
def test_forward_bit_exact(oracle, shape, regime):
    from ced_nerf_amd import _lib, ops
    pb = _problem(shape, regime)
    D = _dev(pb)
    u = pb.used
    prefix = np.where(u, M._rng(0, "prefix").uniform(0, 1, size=pb.S), np.nan).astype(np.float32)
    for pf in (None, prefix):
        want = oracle.render_weight_from_density(pb.t0, pb.t1, pb.sigma, pb.packed, pf)
        got = _weights(pb, D, None if pf is None else T(pf))
        for g, w, nm in zip(got, want, ("weights", "trans", "alphas")):
            assert_bitexact(N(g)[u], w[u], f"{nm} prefix={pf is not None}")
            _untouched(g, pb, nm)
    w0 = np.where(u, oracle.render_weight_from_density(pb.t0, pb.t1, pb.sigma, pb.packed, None)[0], np.nan).astype(np.float32)
    rgb0, op0, dp0 = _state(pb)
    for vals, out0 in ((pb.rgb, rgb0), (None, op0[:, None])):
        want = oracle.accumulate_along_rays_(w0, vals, pb.packed, out0.copy())
        got = T(out0.copy())
        ops.accumulate_along_rays_(D[0], T(w0), None if vals is None else D[4], got)
        assert_bitexact(N(got), want, f"accumulate C={out0.shape[1]}")
    for eps, thre in ((1e-4, 0.0), (1e-4, 1e-2), (0.0, 0.5)):
        want = oracle.visibility_mask(pb.t0, pb.t1, pb.sigma, pb.packed, eps, thre)
        mask = torch.full((pb.S,), 0xA5, dtype=torch.uint8, device=DEV)
        if pb.S:
            _lib.check(_lib.lib().ced_visibility_mask(pb.n_rays, _ptr(D[0]), _ptr(D[1]), _ptr(D[2]), _ptr(D[3]), float(eps),
                                                      float(thre), _ptr(mask), _stream()), "visibility_mask")
        assert_bitexact(N(mask)[u], want.astype(np.uint8)[u], f"visibility eps={eps} thre={thre}")
        assert (N(mask)[~u] == 0xA5).all()
    # composite_prefix_ / composite_step_ / finalize_pixels_
    zero = (np.zeros((pb.n_rays, 3), np.float32), np.zeros(pb.n_rays, np.float32), np.zeros(pb.n_rays, np.float32))
    for nm, st in (("fresh", zero), ("carried", (rgb0, op0, dp0))):
        want = _expected_composite(oracle, pb, *st)
        got = [T(x.copy()) for x in st]
        ops.composite_prefix_(*D, *got)
        for g, w, k in zip(got, want, ("rgb", "opacity", "depth")):
            assert_bitexact(N(g), w, f"composite_prefix {nm} {k}")
        got = [T(x.copy()) for x in st]
        n_iter = _n_samples_iter(pb)
        mask = torch.ones(pb.n_rays, dtype=torch.bool, device=DEV)
        stats = torch.zeros(2, dtype=torch.int64, device=DEV)
        ops.composite_step_(*D, *got, OPC_THRES, n_iter, mask, stats)
        for g, w, k in zip(got, want, ("rgb", "opacity", "depth")):
            assert_bitexact(N(g), w, f"composite_step {nm} {k}")
        alive = (want[1] <= np.float32(OPC_THRES)) & (pb.packed[:, 1] == n_iter)
        assert_bitexact(N(mask), alive, f"composite_step {nm} ray_mask")
        assert N(stats).tolist() == [int(alive.sum()), int(pb.packed[:, 1].sum())], (nm, N(stats))
        if shape == "all_empty":
            assert N(stats).tolist() == [0, 0] and not N(mask).any()
        elif regime == "thin" and nm == "carried":                      # both sides of the threshold, both of the count
            cnt_ok = pb.packed[:, 1] == n_iter
            assert alive.any() and (cnt_ok & ~alive).any() and (pb.packed[:, 1] < n_iter).any()
        for bk in (BKGD, None):
            o, r, d = want[1], want[0], want[2]
            w_rgb = r if bk is None else r + bk[None, :] * (np.float32(1) - o)[:, None]
            w_dp = d / np.maximum(o, np.float32(M.EPS32))
            g_rgb, g_dp = T(r.copy()), T(d.copy())
            ops.finalize_pixels_(None if bk is None else T(bk), g_rgb, T(o), g_dp)
            assert_bitexact(N(g_rgb), w_rgb.astype(np.float32), f"finalize {nm} rgb"); assert_bitexact(N(g_dp), w_dp, f"finalize {nm} depth")
    # composite_test
    q, alive, op, dp, rgb, _ = M.stepper_setup(pb)
    w_alive, w_op, w_dp, w_rgb = alive.copy(), op.copy(), dp.copy(), rgb.copy()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    oracle.lib().ced_o_composite_test(C.c_int64(q.n_rays), p(q.sigma), p(q.rgb), p(q.t0), p(q.t1), p(q.packed), p(w_alive),
                                      C.c_float(M.T_THR), C.c_float(M.A_THR), p(w_op), p(w_dp), p(w_rgb))
    g_alive, g_op, g_dp, g_rgb = T(alive), T(op), T(dp), T(rgb)
    ops.composite_test_(T(q.sigma), T(q.rgb), T(q.t0), T(q.t1), T(q.packed), g_alive, M.T_THR, M.A_THR, g_op, g_dp, g_rgb)
    assert_bitexact(N(g_alive), w_alive, "composite_test alive")
    assert_bitexact(N(g_op), w_op, "composite_test opacity"); assert_bitexact(N(g_dp), w_dp, "composite_test depth")
    assert_bitexact(N(g_rgb), w_rgb, "composite_test rgb")
    assert (w_alive[q.packed[:, 1] == 0] == -1).all()
    if shape == "all_empty":
        assert (w_alive == -1).all() and np.array_equal(w_op, op)


# ----------------------------------------------------------------------------------------------------------------------
# forward (b): against float64 within the derived bounds
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,regime", _cases(M.FORWARD_CASES))
def test_forward_against_float64(shape, regime):
    from ced_nerf_amd import ops
    pb = _problem(shape, regime)
    D = _dev(pb)
    u = pb.used
    ratios = {}
    prefix = np.where(u, M._rng(0, "prefix").uniform(0, 1, size=pb.S), np.nan).astype(np.float32)
    for nm, pf in (("plain", None), ("prefix", prefix)):
        f = M.forward(pb, pf, per_sample=True)
        got = _weights(pb, D, None if pf is None else T(pf))
        for g, k, b in zip(got, ("w", "T", "a"), np.asarray(M.forward_bounds(f))[[2, 0, 1]]):
            ratios[f"{nm} {k}"] = M.worst(N(g)[u], pb.scatter(f[k])[u], pb.scatter(b)[u])
    rgb0, op0, dp0 = _state(pb)
    w32 = np.where(u, N(_weights(pb, D)[0]), np.nan).astype(np.float32)
    got = T(rgb0.copy())
    ops.accumulate_along_rays_(D[0], T(w32), D[4], got)
    want, bound = M.accumulate(pb, w32, pb.rgb, rgb0)
    ratios["accumulate"] = M.worst(N(got), want, bound)
    for nm, st in (("fresh", None), ("carried", (rgb0, op0, dp0))):
        m = M.composite(pb, st, want_bounds=True)
        z = st if st is not None else (np.zeros((pb.n_rays, 3), np.float32), np.zeros(pb.n_rays, np.float32), np.zeros(pb.n_rays, np.float32))
        for fn in ("prefix", "step"):
            got = [T(x.copy()) for x in z]
            if fn == "prefix":
                ops.composite_prefix_(*D, *got)
            else:
                ops.composite_step_(*D, *got, OPC_THRES, _n_samples_iter(pb), torch.ones(pb.n_rays, dtype=torch.bool, device=DEV),
                                    torch.zeros(2, dtype=torch.int64, device=DEV))
            for g, k in zip(got, ("rgb", "opacity", "depth")):
                ratios[f"{fn} {nm} {k}"] = M.worst(N(g), m[k], m["bounds"][k])
        r32, o32, d32 = (N(g) for g in got)
        fin = M.finalize(BKGD, r32, o32, d32)
        g_rgb, g_dp = T(r32.copy()), T(d32.copy())
        ops.finalize_pixels_(T(BKGD), g_rgb, T(o32), g_dp)
        ratios[f"final {nm} rgb"] = M.worst(N(g_rgb), fin[0], fin[2]); ratios[f"final {nm} depth"] = M.worst(N(g_dp), fin[1], fin[3])
    q, alive, op, dp, rgb, _ = M.stepper_setup(pb)
    r64 = M.composite_test(q, alive, op, dp, rgb, M.T_THR, M.A_THR)
    ok = r64["robust"]
    robust = np.ones(op.shape[0], bool); robust[alive[~ok]] = False      # per target ray; untouched rays must stay equal
    assert ok.mean() >= 0.9 or pb.n_rays < 10
    g_alive, g_op, g_dp, g_rgb = T(alive), T(op), T(dp), T(rgb)
    ops.composite_test_(T(q.sigma), T(q.rgb), T(q.t0), T(q.t1), T(q.packed), g_alive, M.T_THR, M.A_THR, g_op, g_dp, g_rgb)
    assert np.array_equal(N(g_alive)[ok], r64["alive"][ok])
    for g, k in ((g_op, "opacity"), (g_dp, "depth"), (g_rgb, "rgb")):
        ratios[f"test {k}"] = M.worst(N(g), r64[k], r64["bounds"][k], robust[:, None])
    top = sorted(ratios.items(), key=lambda kv: -kv[1])[:4]
    print(f"FWD64 {pb.name}: err/bound max {top[0][1]:.3f}; " + ", ".join(f"{k} {v:.3f}" for k, v in top))
    assert max(ratios.values()) <= 1.0, {k: v for k, v in ratios.items() if v > 1.0}


# ----------------------------------------------------------------------------------------------------------------------
# backward
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,regime", _cases(M.BACKWARD_CASES))
def test_backward_against_float64(shape, regime):
    from ced_nerf_amd import ops
    pb = _problem(shape, regime)
    D = _dev(pb)
    u = pb.used
    ri = pb.ray_indices()
    w = N(_weights(pb, D)[0])                                           # the forward kernel's weights
    ratios, not_forward, problems = {}, 0, []
    for which in M.GRADS:
        g = M.ray_grads(pb, which)
        ds, dr = _backward(pb, D, [T(x) for x in g])
        _untouched(ds, pb, "d_sigmas"); _untouched(dr, pb, "d_rgbs")
        ds, dr = N(ds), N(dr)
        if which == "all":                                              # the wrapper: the same bits, zeros elsewhere
            o_ds, o_dr = (N(x) for x in ops.composite_backward(*D, *[T(x) for x in g]))
            assert_bitexact(o_ds[u], ds[u], "ops d_sigmas"); assert_bitexact(o_dr[u], dr[u], "ops d_rgbs")
            assert not o_ds[~u].any() and not o_dr[~u].any()
        if not (np.isfinite(ds[u]).all() and np.isfinite(dr[u]).all()):
            problems.append(f"{which}: NaN or inf")
        w_ds, w_dr, b_ds, b_dr, _ = M.backward(pb, *g, want_bounds=True)
        ratios[which] = (M.worst(ds[u], w_ds[u], b_ds[u]), M.worst(dr[u], w_dr[u], b_dr[u]))
        if (dr[u][w[u] == 0] != 0).any():
            problems.append(f"{which}: d_rgb is not 0 where the weight is 0")
        fwd = (w[u, None] * g[0][ri[u]]).astype(np.float32)
        not_forward += int((dr[u].view(np.uint32) != fwd.view(np.uint32)).sum())
    print(f"BWD {pb.name}: err/bound d_sigma " + ", ".join(f"{k} {a:.3g}" for k, (a, _) in ratios.items()) + "; d_rgb " +
          ", ".join(f"{k} {b:.3g}" for k, (_, b) in ratios.items()) + f"; d_rgb != fl32(w d_colour) at {not_forward} elements")
    assert not problems, problems
    assert max(max(v) for v in ratios.values()) <= 1.0, ratios
    assert not_forward == 0, "the backward does not see the forward kernel's weights"


# ----------------------------------------------------------------------------------------------------------------------
# reduce_along_rays
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", ["none", "one", "channel"])
@pytest.mark.parametrize("C_", [1, 3, 5])
@pytest.mark.parametrize("n", M.REDUCE_N)
def test_reduce_along_rays(n, C_, weights):
    from ced_nerf_amd import ops
    ri, vals, w = M.reduce_problem(n, C_, weights)
    perm = M._rng(0, "shuffle").permutation(ri.shape[0])
    worst = {}
    for mean in (False, True):
        want, bound, m = M.reduce64(ri, vals, w, n, mean)
        for nm, p in (("packed", None), ("shuffled", perm)):
            r_, v_, w_ = (x if p is None or x is None else x[p] for x in (ri, vals, w))
            got = N(ops.reduce_along_rays(T(r_), T(v_), n, None if w_ is None else T(w_), mean=mean))
            worst[f"{'mean' if mean else 'sum'} {nm}"] = M.worst(got, want, bound)
            assert (got[m == 0] == 0).all()
    print(f"REDUCE n={n} C={C_} weights={weights} (runs up to {int(np.bincount(ri, minlength=n).max())}): err/bound " +
          ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_reduce_mean_divisor_is_exact():
    """ones summed are the run's length exactly, in any order; the mean is that over length + 1, rounded once"""
    from ced_nerf_amd import ops
    ri, vals, _ = M.reduce_problem(257, 3, "none")
    ones = np.ones_like(vals)
    m = np.bincount(ri, minlength=257).astype(np.float32)
    for p in (np.arange(ri.shape[0]), M._rng(0, "shuffle").permutation(ri.shape[0])):
        got = N(ops.reduce_along_rays(T(ri[p]), T(ones), 257, None, mean=False))
        assert_bitexact(got, np.repeat(m[:, None], 3, 1), "sum of ones")
        got = N(ops.reduce_along_rays(T(ri[p]), T(ones), 257, None, mean=True))
        assert_bitexact(got, np.repeat((m / (m + np.float32(1)))[:, None], 3, 1), "mean of ones")
