"""GPU suite: the derivative of the warp (csrc/field_jacobian.hip: ced_field_move_jacobian, ced_field_move_inverse_newton,
ced_field_track_newton) and what stands on it -- DNGPradianceField.query_move_jacobian / query_velocity /
query_move_inverse(method="newton") / track_points(method="newton"), export.track_mesh(normals=, velocities=).

References (tests/warp64.py, pinned on the CPU by tests/test_warp_jacobian_cpu.py): a float64 forward-mode model of the
motion network with the weights and every layer's inputs rounded as the field's mlp_precision rounds them, for the
Jacobian; include/cednerf_hip.h's Newton iteration in numpy float32 on K launches of query_move_jacobian, for the bits of
the fused solver; a float64 Newton solve of x + move(x, t) = c for what the solver promises.  Every bound is computed here
on the CPU from the difference between a model run in float32 and in float64, never from the kernels' results.

Inputs: those of tests/test_gpu_track.py -- rng 7, 4099 rows, aabb +-1.5, log2 table 15, moving steps 1/32 and 1/8."""
import functools

import numpy as np
import pytest
import torch

import warp64 as W
from test_gpu_track import DEV, FLAGS, MARGIN, MODES, SIZES, STEP, N, T, _field, _inputs, _params, _read_ply

pytestmark = pytest.mark.gpu

COARSE = 1.0 / 8
TILE = 16                                                               # rows of one wave tile of the Jacobian kernels
TABLES = [("f16x2", "f16"), ("f16x2", "temporal"), ("f16", "temporal"), ("f32", "f16")]


@functools.lru_cache(maxsize=None)
def _np_inputs():
    pos, t = _inputs()
    return N(pos), N(t)


@functools.lru_cache(maxsize=None)
def _model(div, tm, step, mode, dtype):
    """(move, jac, pre) of the model on the 4099 inputs, rounded as `mode`'s motion network, in float64 or float32"""
    pos, t = _np_inputs()
    return W.move_jacobian(_params(div, tm, step), pos, t, np.dtype(dtype).type, mode)


def _gpu_move_jac(f, t_dev):
    def fn(x, t):
        mv, jac = f.query_move_jacobian(T(x), t_dev)
        return N(mv), N(jac)
    return fn


# ---- 1. move is query_move's -------------------------------------------------------------------------------------------
def _check_move_is_query_move(f, what):
    from ced_nerf_amd import ops
    pos, t = _inputs()
    want = f.query_move(pos, t)[1]
    full = f.query_move_jacobian(pos, t)
    assert torch.equal(full[0], want), (what, int((full[0] != want).sum()))
    assert bool(torch.isfinite(full[1]).all()) and float(full[1][:, :, :3].abs().max()) > 1e-3 and float(full[1][:, :, 3].abs().max()) > 1e-3
    for n in SIZES:
        mv, jac = f.query_move_jacobian(pos[:n], t[:n])
        assert mv.shape == (n, 3) and jac.shape == (n, 3, 4) and mv.dtype == jac.dtype == torch.float32
        assert torch.equal(mv, want[:n]), (what, n)
        assert torch.equal(jac, full[1][:n]), (what, n)                 # a row does not depend on n
    d = f._descriptor()
    only_move = ops.field_move_jacobian(d, pos, t, want=(True, False))
    only_jac = ops.field_move_jacobian(d, pos, t, want=(False, True))
    assert only_move[1] is None and only_jac[0] is None
    assert torch.equal(only_move[0], want) and torch.equal(only_jac[1], full[1])
    with pytest.raises(ValueError, match="no output"):
        ops.field_move_jacobian(d, pos, t, want=(False, False))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("div,tm", FLAGS)
def test_move_is_query_moves_bit_for_bit(div, tm, mode):
    """query_move_jacobian's move == query_move's with torch.equal, for every n of SIZES, and a row's Jacobian is the same
    at every n; either output alone is the same."""
    _check_move_is_query_move(_field(div, tm, mode), (div, tm, mode))


@pytest.mark.parametrize("mode,table", TABLES)
def test_move_is_query_moves_on_the_other_tables(mode, table):
    """both f16x2 blob layouts (K = 32 placements on an fp16 table, pair form on a temporal one)"""
    _check_move_is_query_move(_field(True, 0, mode, STEP, table), (mode, table))


# ---- 2. accuracy of the Jacobian ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("step", [STEP, COARSE])
@pytest.mark.parametrize("div,tm", FLAGS)
def test_jacobian_accuracy(div, tm, step, mode):
    """query_move_jacobian against the float64 forward-mode model of the mode-rounded network, on the rows none of whose
    hidden pre-activations lies within 1e-5 (of the layer's largest) of zero -- a ReLU mask may differ there; at most 2 % of
    the rows may be left out.  Bound: 4 x the largest difference between that model run in float32 (sines included) and
    in float64, 8 x for f16 (decided by a handful of fp16 double roundings); first the primal, by the same rule.
    CPU model: the bound's base is 5.1e-7 / 6.0e-7 (step 1/32, fine offsets off / on) and 2.0e-6 / 2.4e-6 (1/8) for f32 and
    f16x2, 9.2e-5 / 1.4e-4 and 3.7e-4 / 5.7e-4 for f16; 0.63 % (f32), 0.66 % (f16x2), 0.49 % (f16) of the rows are left out.
    Measured on an MI355X, max |J - model| on the kept rows: f32 7.8e-8 / 8.4e-8 (1/32) and 3.1e-7 / 3.4e-7 (1/8), f16x2 7.4e-8 /
    1.1e-7 and 3.0e-7 / 4.4e-7, f16 8.7e-5 / 1.0e-4 and 3.5e-4 / 4.1e-4; f16 against the UNROUNDED float64 Jacobian (printed, not
    asserted): max 6.1e-2 / 6.3e-2, median 6.3e-5 / 8.4e-5 at 1/32."""
    mm = W.MOTION_MODES[mode]
    f = _field(div, tm, mode, step)
    pos, t = _inputs()
    mv, jac = f.query_move_jacobian(pos, t)
    m64, j64, pre = _model(div, tm, step, mm, "float64")
    m32, j32, _ = _model(div, tm, step, mm, "float32")
    keep = W.kept_rows(pre)
    left_out = 1.0 - float(keep.mean())
    factor = 8 if mm == "f16" else 4
    bound_m = factor * float(np.abs(m32 - m64)[keep].max())
    bound_j = factor * float(np.abs(j32 - j64)[keep].max())
    err_m = float(np.abs(N(mv) - m64)[keep].max())
    err_j = float(np.abs(N(jac) - j64)[keep].max())
    err_all = float(np.abs(N(jac) - j64).max())
    print(f"jacobian [{mode} div={div} tm={tm} step={step:g}]: {100 * left_out:.2f} % of rows left out; max |move - model| = "
          f"{err_m:.3e} (bound {bound_m:.3e}), max |J - model| = {err_j:.3e} (bound {bound_j:.3e}; every row: {err_all:.3e}), "
          f"max |J| = {float(np.abs(j64).max()):.3f}")
    if mm == "f16":
        exact = _model(div, tm, step, None, "float64")[1]
        dist = np.abs(N(jac) - exact).max((1, 2))
        print(f"    f16 against the UNROUNDED float64 Jacobian: max {float(dist.max()):.3e}, median {float(np.median(dist)):.3e}")
    assert left_out <= 0.02
    assert err_m <= bound_m
    assert err_j <= bound_j


# ---- 3. the fused Newton solver is the composition ---------------------------------------------------------------------
def _assert_same(got, want, what):
    for g, w, name in zip(got, want, ("x", "step", "evals")):
        w = T(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert torch.equal(g, w), (what, name, int((g != w).sum()))


def _check_newton_is_the_composition(f, what):
    pos, t = _inputs()
    c = f.query_move(pos, t)[0]
    c_np, pos_np, t_np = N(c), N(pos), N(t)
    fn = _gpu_move_jac(f, t)
    several = False
    for K in (1, 4, 32):
        for tol in (0.0, 1e-6):
            for init, init_np in ((None, None), (pos, pos_np)):
                want = W.newton_f32(fn, c_np, t_np, K, tol, init_np)
                ev = want[2]
                assert int(ev.min()) >= 1 and int(ev.max()) <= K
                for n in SIZES:
                    got = f.query_move_inverse(c[:n], t[:n], max_iters=K, tol=tol, init=None if init is None else init[:n],
                                               method="newton")
                    assert got[0].shape == (n, 3) and got[1].shape == (n,) and got[2].dtype == torch.int32
                    _assert_same(got, tuple(w[:n] for w in want), (what, K, tol, n, init is not None))
                if tol > 0 and K == 32 and init is None:
                    tiles = ev[:len(ev) // TILE * TILE].reshape(-1, TILE)
                    several = several or max(len(np.unique(row)) for row in tiles) >= 3
    assert several, "the rows of one tile must stop at >= 3 different rounds for the freeze to be exercised"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("div,tm", FLAGS)
def test_newton_is_the_composition_bit_for_bit(div, tm, mode):
    """query_move_inverse(method="newton") == K launches of query_move_jacobian with the header's fp32 lines in numpy float32
    on the host (IEEE single, no contraction): x, step and evals with torch.equal, for K in 1, 4, 32, tol in 0, 1e-6, every n
    of SIZES, started at the target and at an `init` of its own."""
    _check_newton_is_the_composition(_field(div, tm, mode), (div, tm, mode))


@pytest.mark.parametrize("mode,table", TABLES)
def test_newton_is_the_composition_on_the_other_tables(mode, table):
    _check_newton_is_the_composition(_field(True, 0, mode, STEP, table), (mode, table))


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
@pytest.mark.parametrize("use_init", [False, True])
def test_newton_broadcast_equals_explicit_rows(mode, use_init):
    """ops.field_track_newton(c [P], times [T]) == ops.field_move_inverse_newton on the expanded rows r = k * P + p."""
    from ced_nerf_amd import ops
    f = _field(True, 2, mode)
    pos, t = _inputs()
    d = f._descriptor()
    for P in (1, 33, 257):
        c = f.query_move(pos[:P], t[:P])[0]
        init = pos[:P].contiguous() if use_init else None
        for n_t in (1, 3):
            times = T(np.asarray([0.8, 0.1, 0.45][:n_t], np.float32))
            x, step, evals = ops.field_track_newton(d, c, times, init, max_iters=32, tol=1e-6)
            assert x.shape == (n_t, P, 3) and step.shape == (n_t, P) and evals.shape == (n_t, P)
            want = ops.field_move_inverse_newton(d, c.repeat(n_t, 1), times.repeat_interleave(P),
                                                 None if init is None else init.repeat(n_t, 1), max_iters=32, tol=1e-6)
            for g, w in zip((x.view(-1, 3), step.view(-1), evals.view(-1)), want):
                assert torch.equal(g, w), (P, n_t)
            tr = f.track_points(pos[:P], t[:P], times, method="newton")
            if use_init:
                assert torch.equal(tr["positions"], x) and torch.equal(tr["converged"], step <= 1e-6)
            if n_t == 3 and P > 1:
                assert not torch.equal(x[0], x[1])


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
def test_a_newton_row_does_not_depend_on_its_tile(mode):
    """rows that stop at different rounds: each one's x, step, evals at n = 4099 (beside rows that go on after it has
    stopped) are those of the row solved alone"""
    f = _field(True, 2, mode)
    pos, t = _inputs()
    c = f.query_move(pos, t)[0]
    x, step, evals = f.query_move_inverse(c, t, max_iters=32, tol=1e-6, method="newton")
    ev = N(evals)
    values = np.unique(ev)
    assert len(values) >= 3, values
    for v in values:
        r = int(np.flatnonzero(ev == v)[0])
        alone = f.query_move_inverse(c[r:r + 1], t[r:r + 1], max_iters=32, tol=1e-6, method="newton")
        for g, w in zip(alone, (x[r:r + 1], step[r:r + 1], evals[r:r + 1])):
            assert torch.equal(g, w), (r, int(v))


# ---- 4. it inverts the warp --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "f16x2"])
@pytest.mark.parametrize("div,tm", FLAGS)
def test_newton_inverts_the_warp(div, tm, mode):
    """Moving step 1/32, K = 32, tol = 1e-6: every row converges; |x + query_move(x) - c| <= MARGIN (test_gpu_track's
    1.64e-6); |x - float64 solve| <= tol * max_row ||(I + J64)^-1||_inf + MARGIN -- Newton stops at the first residual
    <= tol, so that is what the definition promises.  CPU model: 2 .. 4 / 2 .. 5 evaluations (fine offsets off / on).
    Measured on an MI355X: the same evaluations (mean 3.09 / 3.32), residual 9.8e-7 / 1.0e-6, |x - float64 solve| 1.17e-6
    against 3.28e-6 / 3.51e-6."""
    K, tol = 32, 1e-6
    params = _params(div, tm)
    f = _field(div, tm, mode)
    pos, t = _inputs()
    c = f.query_move(pos, t)[0]
    x, step, evals = f.query_move_inverse(c, t, max_iters=K, tol=tol, method="newton")
    assert bool((step <= tol).all()), int((~(step <= tol)).sum())
    resid = float((x + f.query_move(x, t)[1] - c).abs().max())
    x64 = W.solve64(params, N(c), N(t))
    assert np.isfinite(x64).all()
    inv64 = W.gradient_inverse(W.move_jacobian(params, x64, N(t).astype(np.float64))[1])[1]
    norm = float(np.abs(inv64).sum(-1).max())
    vs64 = float(np.abs(N(x).astype(np.float64) - x64).max())
    print(f"newton [{mode} div={div} tm={tm}]: evals {int(evals.min())}..{int(evals.max())} (mean {float(evals.float().mean()):.2f}), "
          f"max |x + move(x) - c| = {resid:.3e}, max |x - float64 solve| = {vs64:.3e} (bound {tol * norm + MARGIN:.3e}, "
          f"max ||(I + J)^-1||_inf = {norm:.3f}), max |x - x_src| = {float((x - pos).abs().max()):.3e}")
    assert resid <= MARGIN
    assert vs64 <= tol * norm + MARGIN


# ---- 5. it converges where the fixed point does not --------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "f16x2"])
@pytest.mark.parametrize("div,tm", FLAGS)
def test_newton_converges_where_the_fixed_point_does_not(div, tm, mode):
    """Moving step 1/8, K = 32, tol = 1e-6: Newton leaves at most HALF the share of unconverged rows the fixed-point
    iteration leaves on the same rows (CPU model: 0.07 % against 2.8 %, 0.51 % against 9.3 %); converged == (step <= tol);
    unconverged rows ran exactly K evaluations; converged rows satisfy the equation within MARGIN through query_move.
    Unconverged rows need not exist.  The rest sits where the warp folds (det(I + J_x) <= 0 on 0.17 % / 0.68 % of the rows).
    Measured on an MI355X: 0.07 % against 2.81 % (f16x2: 2.78 %), 0.41 % (f16x2: 0.46 %) against 9.37 %."""
    K, tol = 32, 1e-6
    f = _field(div, tm, mode, COARSE)
    pos, t = _inputs()
    c = f.query_move(pos, t)[0]
    fixed = f.query_move_inverse(c, t, max_iters=K, tol=tol, method="fixed_point")
    x, step, evals = f.query_move_inverse(c, t, max_iters=K, tol=tol, method="newton")
    ok = step <= tol
    share_fixed = 1.0 - float((fixed[1] <= tol).float().mean())
    share = 1.0 - float(ok.float().mean())
    resid = (x + f.query_move(x, t)[1] - c).abs().max(-1).values
    det = f.query_velocity(pos, t)[1]
    print(f"step 1/8 [{mode} div={div} tm={tm}]: not converged by K = {K}: newton {100 * share:.2f} %, fixed point "
          f"{100 * share_fixed:.2f} % of {len(ok)} rows; newton evals on converged rows {int(evals[ok].min())}..{int(evals[ok].max())} "
          f"(mean {float(evals[ok].float().mean()):.2f}), max residual {float(resid[ok].max()):.3e}; det(I + J_x) <= 0 on "
          f"{100 * float((det <= 0).float().mean()):.2f} % of the inputs")
    assert share_fixed > 0 and share <= 0.5 * share_fixed
    assert bool((evals[~ok] == K).all()) and bool((evals[ok] <= K).all()) and bool((evals >= 1).all())
    assert float(resid[ok].max()) <= MARGIN
    tr = f.track_points(pos, t, [0.5], max_iters=K, tol=tol, method="newton")
    assert torch.equal(tr["converged"], tr["step"] <= tol)
    assert bool((tr["evals"][~tr["converged"]] == K).all())
    again = f.query_move_inverse(c, t, max_iters=K, tol=tol)               # the default is still the fixed point
    assert all(torch.equal(a, b) for a, b in zip(again, fixed))


# ---- 6. velocity and normals -------------------------------------------------------------------------------------------
P_SMALL = 257
H_TIME = 1e-6


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
@pytest.mark.parametrize("div,tm", FLAGS)
def test_velocity_is_the_time_derivative_of_the_track(div, tm, mode):
    """query_velocity at tracked positions x (Newton, step 1/32, 257 rows) against the central difference in t of the
    float64 solve of the material point sitting at x: (x64(t + h) - x64(t - h)) / 2h with c = x + move64(x, t).
    h = 1e-6: on the CPU the float64 analytic v and the difference agree to 2.1e-10 there (h = 1e-5: 7.6e-3 -- a ReLU kink
    inside the stencil; h = 1e-7: 1.8e-9), |v| <= 0.26.  Bound: 4 x (numpy float32 model of v against float64), 3.2e-7 /
    4.0e-7 on the CPU.  Rows with a hidden pre-activation within 1e-5 of zero are left out (the stencil may cross the kink)."""
    params = _params(div, tm)
    f = _field(div, tm, mode)
    pos, t = _inputs()
    pos, t = pos[:P_SMALL], t[:P_SMALL]
    c = f.query_move(pos, t)[0]
    x, step, _ = f.query_move_inverse(c, t, method="newton")
    assert bool((step <= 1e-6).all())
    v, det = f.query_velocity(x, t)
    assert v.shape == (P_SMALL, 3) and det.shape == (P_SMALL,)
    xs, ts = N(x).astype(np.float64), N(t).astype(np.float64)
    _, j64, pre = W.move_jacobian(params, xs, ts)
    keep = W.kept_rows(pre)
    assert keep.mean() >= 0.95
    v64, det64 = W.velocity(j64)
    c64 = xs + W.move64(params, xs, ts)
    fd = (W.solve64(params, c64, ts + H_TIME, start=xs) - W.solve64(params, c64, ts - H_TIME, start=xs)) / (2 * H_TIME)
    j32 = W.move_jacobian(params, N(x), N(t), np.float32)[1]
    v32, det32 = W.velocity(j32)
    bound = 4 * float(np.abs(v32 - v64)[keep].max())
    bound_det = 4 * float(np.abs(det32 - det64)[keep].max())
    err = float(np.abs(N(v) - fd)[keep].max())
    err_det = float(np.abs(N(det) - det64)[keep].max())
    print(f"velocity [{mode} div={div} tm={tm}]: max |v| = {float(np.abs(v64).max()):.3f}, float64 analytic against central "
          f"difference {float(np.abs(v64 - fd)[keep].max()):.3e}; max |query_velocity - difference| = {err:.3e} (bound {bound:.3e}); "
          f"max |det - det64| = {err_det:.3e} (bound {bound_det:.3e}); det in {float(det.min()):.3f} .. {float(det.max()):.3f}")
    assert float(np.abs(v64 - fd)[keep].max()) <= 1e-8
    assert err <= bound and err_det <= bound_det


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
@pytest.mark.parametrize("div,tm", FLAGS)
def test_normals_move_with_the_mesh(div, tm, mode):
    """track_mesh(method="newton", normals=True, velocities=True) on 257 vertices with unit normals of their own:
    normals_t have unit length within 1e-6; at t_ref they are the mesh's normals within 4 x the numpy float32 model's own
    error there; at the other times they are the float64 model's (I + J_t)^T (I + J_ref)^-T n_ref, normalised, within
    4 x (numpy float32 model against float64), both models evaluated at the tracked positions."""
    from ced_nerf_amd import export as E
    params = _params(div, tm)
    f = _field(div, tm, mode)
    pos, _ = _inputs()
    vertices = pos[:P_SMALL].contiguous()
    n_ref = np.random.default_rng(11).normal(size=(P_SMALL, 3))
    n_ref /= np.linalg.norm(n_ref, axis=-1, keepdims=True)
    mesh = dict(vertices=vertices, faces=torch.zeros((1, 3), dtype=torch.int32, device=DEV), normals=T(n_ref.astype(np.float32)))
    t_ref, times = 0.37, [0.0, 0.37, 1.0]
    tracked = E.track_mesh(f, mesh, t_ref, times, method="newton", normals=True, velocities=True)
    assert bool(tracked["converged"].all())
    nt = tracked["normals_t"]
    assert nt.shape == (3, P_SMALL, 3) and tracked["velocities_t"].shape == (3, P_SMALL, 3) and tracked["det_t"].shape == (3, P_SMALL)
    assert float((nt.norm(dim=-1) - 1).abs().max()) <= 1e-6
    assert torch.equal(tracked["normals"], mesh["normals"])
    ref_t = np.full(P_SMALL, t_ref)
    n32_ref = N(mesh["normals"])
    j64_ref = W.move_jacobian(params, N(vertices).astype(np.float64), ref_t)[1]
    j32_ref = W.move_jacobian(params, N(vertices), ref_t.astype(np.float32), np.float32)[1]
    for k, tk in enumerate(times):
        xk = N(tracked["vertices_t"][k])
        tt = np.full(P_SMALL, tk)
        n64 = W.carried_normals(W.move_jacobian(params, xk.astype(np.float64), tt)[1], j64_ref, n32_ref.astype(np.float64))
        n32 = W.carried_normals(W.move_jacobian(params, xk, tt.astype(np.float32), np.float32)[1], j32_ref, n32_ref)
        assert n32.dtype == np.float32
        if tk == t_ref:
            want, bound = n32_ref, 4 * float(np.abs(n32 - n32_ref).max())
        else:
            want, bound = n64, 4 * float(np.abs(n32 - n64).max())
        err = float(np.abs(N(nt[k]) - want).max())
        turned = float(np.abs(N(nt[k]) - n32_ref).max())
        print(f"normals [{mode} div={div} tm={tm}] t = {tk:g}: max |n_t - reference| = {err:.3e} (bound {bound:.3e}), "
              f"max |n_t - n_ref| = {turned:.3e}")
        assert err <= bound, (tk, err, bound)
        if tk != t_ref:
            assert turned > 1e-3
        v, det = f.query_velocity(tracked["vertices_t"][k], torch.full((P_SMALL,), tk, device=DEV))
        assert torch.allclose(tracked["velocities_t"][k], v, rtol=0, atol=1e-6) and torch.allclose(tracked["det_t"][k], det, rtol=0, atol=1e-6)
    plain = E.track_mesh(f, mesh, t_ref, times, method="newton")
    assert "normals_t" not in plain and "velocities_t" not in plain and torch.equal(plain["vertices_t"], tracked["vertices_t"])


def test_tracked_mesh_with_moving_normals(tmp_path):
    """extract_mesh_tracked(method="newton", normals=True) on the volume tests' field (reso 32, three times): the reference
    mesh is extract_mesh's, every frame satisfies the equation, frame k's PLY carries normals_t[k], the npz holds them"""
    from ced_nerf_amd import export as E
    from test_gpu_export import _density, _field as export_field
    f = export_field(True, 2, "f32")
    t_ref, times = 0.37, [0.0, 0.37, 1.0]
    thresh = float(_density(True, 2, "f32", 32, t_ref)[1].median())
    kw = dict(reso=32, sigma_thresh=thresh, dirs="normal")
    ref = E.extract_mesh(f, t_ref, **kw)
    tracked = E.extract_mesh_tracked(f, t_ref, times, method="newton", normals=True, **kw)
    v = ref["vertices"].shape[0]
    assert v > 100 and torch.equal(tracked["faces"], ref["faces"]) and torch.equal(tracked["normals"], ref["normals"])
    assert bool(tracked["converged"].all()) and tracked["normals_t"].shape == (3, v, 3) and "velocities_t" not in tracked
    at_ref = float((tracked["vertices_t"][1] - ref["vertices"]).abs().max())
    lengths = tracked["normals_t"].norm(dim=-1)
    has_normal = ref["normals"].norm(dim=-1) > 0
    print(f"tracked mesh with normals: V = {v}, max |vertices_t(t_ref) - vertices| = {at_ref:.3e}, max |n_t(t_ref) - n_ref| = "
          f"{float((tracked['normals_t'][1] - ref['normals']).abs().max()):.3e}")
    assert at_ref <= MARGIN
    assert float((lengths[:, has_normal] - 1).abs().max()) <= 1e-6 and bool((lengths[:, ~has_normal] == 0).all())
    for k, tk in enumerate(times):
        p = tracked["vertices_t"][k]
        r = float((p + f.query_move(p, torch.full((v,), tk, device=DEV))[1] - tracked["canonical"]).abs().max())
        assert r <= MARGIN, (tk, r)
    E.save_tracked_npz(str(tmp_path / "tracked.npz"), tracked)
    with np.load(tmp_path / "tracked.npz") as z:
        assert np.array_equal(z["normals_t"], N(tracked["normals_t"])) and np.array_equal(z["normals"], N(ref["normals"]))
    for k in range(3):
        frame = E.tracked_frame(tracked, k)
        E.save_mesh_ply(str(tmp_path / f"tracked_{k}.ply"), frame)
        w, fr, normals = _read_ply(tmp_path / f"tracked_{k}.ply")
        assert normals and np.array_equal(w["normal"], N(tracked["normals_t"][k]))
        assert np.array_equal(w["xyz"], N(tracked["vertices_t"][k])) and np.array_equal(fr["ids"], N(ref["faces"]))
    # the default is what it was: no normals in the frames
    default = E.extract_mesh_tracked(f, t_ref, times, **kw)
    assert "normals_t" not in default and "normals" not in E.tracked_frame(default, 0)
