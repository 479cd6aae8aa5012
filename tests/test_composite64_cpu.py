"""tests/composite64.py checked on the CPU: its generators, its float64 model (against autograd of its own forward and
against the C oracle), and its bounds -- the model evaluated in float32 must meet every bound the GPU tests use."""
import ctypes as C

import numpy as np
import pytest
import torch

import composite64 as M

U = M.U


def _problems(cases):
    return [pytest.param(s, g, id=f"{s}-{g}") for s, g in cases]


# ----------------------------------------------------------------------------------------------------------------------
# generators
# ----------------------------------------------------------------------------------------------------------------------
def test_generators_produce_what_they_name():
    from ced_nerf_amd import ops
    assert M.EXP15 == ops.EXP15
    for n in M.EDGE_N:
        pb = M.make(f"edge{n}", "mixed")
        cnt = pb.packed[:, 1]
        assert pb.n_rays == n and cnt.min() >= 0 and cnt.max() <= 40
        assert np.array_equal(pb.packed[:, 0], np.cumsum(cnt) - cnt) and pb.S == cnt.sum()
        if n >= 255:
            assert 0.15 < (cnt == 0).mean() < 0.45
    # the sample walker (composite_core.hpp: walk_samples) loads kU = 4 samples at a time and finishes one by one:
    # test_gpu_compositing's shapes must hold every count around one and two batches (asserted: a new seed may not lose them)
    kU = 4
    assert set(range(2 * kU + 1)) <= set(M.make("edge257", "mixed").packed[:, 1])
    pb = M.make("long", "mixed")
    assert {kU - 1, kU, kU + 1} <= set(pb.packed[:, 1])
    assert sorted(set(pb.packed[:, 1])) == sorted(M.LONG_LENGTHS) and pb.n_rays == 60 and pb.S <= 2e5
    pb = M.make("all_empty", "mixed")
    assert pb.n_rays == 300 and pb.S == 0 and not pb.packed.any()
    pb = M.make("gapped", "mixed")
    assert np.array_equal(pb.packed[:, 0], np.arange(pb.n_rays) * M.GAP_CAP) and pb.packed[:, 1].max() == M.GAP_CAP
    assert pb.S == pb.n_rays * M.GAP_CAP and 0 < pb.used.sum() < pb.S
    for x in (pb.t0, pb.t1, pb.sigma, pb.rgb[:, 0]):
        assert np.isnan(x[~pb.used]).all() and np.isfinite(x[pb.used]).all()
    assert np.array_equal(pb.ray_indices() >= 0, pb.used)
    assert M.make("long", "wall").t0.tobytes() == M.make("long", "wall").t0.tobytes()
    assert M.make("long", "wall", 1).sigma.tobytes() != M.make("long", "wall", 0).sigma.tobytes()


@pytest.mark.parametrize("shape", ["edge257", "long", "gapped", "wallrays"])
def test_density_regimes(shape):
    f32 = lambda pb: M.forward(pb, dtype=np.float32)
    pb = M.make(shape, "thin")
    assert (M.forward(pb)["sd"].sum(1) <= 0.05).all()
    pb = M.make(shape, "saturated")
    f = f32(pb)
    assert (f["sd"][pb.valid] >= 200).all() and (f["a"][pb.valid] == 1).all() and (f["T"][:, 1:][pb.valid[:, 1:]] == 0).all()
    pb = M.make(shape, "zeros")
    f = f32(pb)
    whole = (np.where(pb.valid, f["sd"], 0).sum(1) == 0) & (pb.packed[:, 1] > 0)
    assert whole.any() and (f["dt"][pb.valid] == 0).any()
    inside = ((f["sd"] == 0) & pb.valid).sum(1)
    assert ((inside >= 3) & ~whole).any()
    pb = M.make(shape, "wall")
    sig = pb.gather(pb.sigma, np.float64)
    for s in M.WALL_SIGMAS:
        assert (np.float32(s) == sig[pb.valid]).any()
    assert (sig[pb.valid] <= 2).any() or shape != "wallrays"


def test_wall_rays_are_not_vacuous():
    """every wall ray with a part in front of its wall has >= 20 samples there whose |d sigma| is >= 1e-3 of the ray's
    largest, and walls end rays, sit inside them and start them"""
    pb = M.make("wallrays", "wall")
    r = np.arange(pb.n_rays)
    ws, wl, wsig = M.wall_layout(r, pb.packed[:, 1])
    assert (wl >= 8).all() and set(np.unique(wsig)) == set(M.WALL_SIGMAS)
    assert (ws[r % 3 == 2] == 0).all() and (ws[r % 3 != 2] >= 20).all()
    assert ((ws + wl)[r % 3 == 0] == pb.packed[r % 3 == 0, 1]).all() and ((ws + wl)[r % 3 == 1] < pb.packed[r % 3 == 1, 1]).all()
    pre = np.arange(pb.L)[None, :] < ws[:, None]
    for which in M.GRADS:
        ds, _ = M.backward(pb, *M.ray_grads(pb, which))
        d = np.abs(pb.gather(ds, np.float64))
        if which == "opacity":
            # d_opacity alone: d sigma_i = dt_i d_opacity T_end exactly (the sums telescope), so behind a wall the whole
            # gradient vanishes; what the kernel must get right there is the cancellation itself
            # (T_end <= e^-40 behind the thinnest wall; float64 leaves the rounding of terms of size dt |d_opacity|)
            assert (d.max(1) <= 1e-12 * np.abs(M.ray_grads(pb, which)[1])).all()
            continue
        n_big = ((d >= 1e-3 * d.max(1, keepdims=True)) & pre).sum(1)
        assert (n_big[r % 3 != 2] >= 20).all(), (which, n_big)


# ----------------------------------------------------------------------------------------------------------------------
# the float64 model
# ----------------------------------------------------------------------------------------------------------------------
def _torch_forward(pb, sg, rgb):
    """the model's forward restated on torch float64 tensors (padded), for autograd"""
    t0, t1 = (torch.from_numpy(pb.gather(x, np.float64)) for x in (pb.t0, pb.t1))
    v = torch.from_numpy(pb.valid)
    sd = torch.where(v, sg * (t1 - t0), torch.zeros_like(sg))
    acc = torch.cat([torch.zeros_like(sd[:, :1]), torch.cumsum(sd[:, :-1], 1)], 1)
    w = torch.where(v, torch.exp(-acc) * -torch.expm1(-sd), torch.zeros_like(sg))
    return (w[:, :, None] * rgb).sum(1), w.sum(1), (w * (t0 + t1) / 2).sum(1)


@pytest.mark.parametrize("shape,regime", _problems([("edge257", "mixed"), ("long", "mixed"), ("wallrays", "wall"),
                                                    ("gapped", "wall")]))
def test_backward_is_the_derivative_of_the_forward(shape, regime):
    pb = M.make(shape, regime)
    dc, dop, ddp = M.ray_grads(pb, "all")
    sg = torch.from_numpy(pb.gather(pb.sigma, np.float64)).requires_grad_()
    rgb = torch.from_numpy(pb.gather(pb.rgb, np.float64)).requires_grad_()
    col, op, dp = _torch_forward(pb, sg, rgb)
    m = M.composite(pb)
    for got, want in ((col, m["rgb"]), (op, m["opacity"]), (dp, m["depth"])):
        assert np.abs(got.detach().numpy() - want).max() <= 1e-12
    ((col * torch.from_numpy(dc).double()).sum() + (op * torch.from_numpy(dop).double()).sum() +
     (dp * torch.from_numpy(ddp).double()).sum()).backward()
    ds, dr, _, _, A = M.backward(pb, dc, dop, ddp, want_bounds=True)
    ds, dr, A = pb.gather(ds, np.float64), pb.gather(dr, np.float64), pb.gather(A, np.float64)
    # float64 against float64: every term of d sigma_i rounded a few times and summed in another order, (L + 2) 2^-53 of
    # the absolute sum A_i of its terms per operation; 64 covers the operations per term of both evaluations
    tol = 64 * (pb.L + 2) * 2.0 ** -53
    assert (np.abs(sg.grad.numpy() - ds) <= tol * A + 1e-300).all()
    assert (np.abs(rgb.grad.numpy() - dr) <= tol * np.abs(dr) + 1e-300).all()


@pytest.mark.parametrize("shape,regime", _problems([("edge513", "mixed"), ("long", "thin"), ("wallrays", "wall"),
                                                    ("gapped", "zeros"), ("long", "saturated")]))
def test_model_against_the_oracle(oracle, shape, regime):
    pb = M.make(shape, regime)
    dc, dop, ddp = M.ray_grads(pb, "all")
    w_ds, w_dr = oracle.composite_backward(pb.packed, pb.t0, pb.t1, pb.sigma, pb.rgb, dc, dop, ddp)
    ds, dr, _, _, A = M.backward(pb, dc, dop, ddp, want_bounds=True)
    u = pb.used
    # both float64.  The oracle recovers every prefix by subtracting back from the ray's total: an absolute error of
    # (cnt + 2) 2^-53 total in the optical depth, i.e. that relative error in T_i, on top of the roundings of the terms
    # (64 (L + 2) 2^-53 of their absolute sum A_i, as above)
    tot = pb.scatter(np.broadcast_to(M.forward(pb)["sd"].sum(1, keepdims=True), pb.valid.shape).copy())
    rel = (pb.L + 2) * 2.0 ** -53 * (64 + 2 * tot[u])
    err = np.abs(w_ds[u] - ds[u])
    assert (err <= rel * A[u] + 1e-300).all(), float((err / (rel * A[u] + 1e-300)).max())
    # (the oracle's a = 1 - exp(-sd) also cancels: 2^-53 absolute in a)
    adc = np.abs(dc[pb.ray_indices()[u]])
    assert (np.abs(w_dr[u] - dr[u]) <= rel[:, None] * np.abs(dr[u]) + 4 * 2.0 ** -53 * adc + 1e-300).all()
    # the oracle's float32 forward within the bounds of a float32 evaluation
    w, tr, al = oracle.render_weight_from_density(pb.t0, pb.t1, pb.sigma, pb.packed)
    f = M.forward(pb)
    dT, da, dw = M.forward_bounds(f)
    for got, want, bound in ((tr, f["T"], dT), (al, f["a"], da), (w, f["w"], dw)):
        assert M.worst(got[u], pb.scatter(want)[u], pb.scatter(bound)[u]) <= 1.0


def test_the_oracles_exp_is_within_its_bound(oracle):
    """E_EXP u relative (TINY absolute below the normal range), on a dense grid over the whole range of arguments"""
    x = np.concatenate([-np.logspace(-8, np.log10(104.0), 20000), np.linspace(-104, 0, 20001)]).astype(np.float32)
    got = np.array([oracle.lib().ced_o_expf(C.c_float(float(v))) for v in x], np.float64)
    want = np.exp(x.astype(np.float64))
    assert (np.abs(got - want) <= M.E_EXP * U * want + M.TINY).all(), float((np.abs(got - want) / (U * want + M.TINY)).max())


# ----------------------------------------------------------------------------------------------------------------------
# the float32 evaluation of the model meets every bound the GPU tests use
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,regime", _problems(M.FORWARD_CASES))
def test_float32_model_meets_the_forward_bounds(shape, regime):
    pb = M.make(shape, regime)
    u = pb.used
    ratios = {}
    prefix = np.where(u, M._rng(0, "prefix").uniform(0, 1, size=pb.S), np.nan).astype(np.float32)
    for nm, pf in (("plain", None), ("prefix", prefix)):
        f, f32 = M.forward(pb, pf, per_sample=True), M.forward(pb, pf, np.float32, per_sample=True)
        for k, b in zip(("T", "a", "w"), M.forward_bounds(f)):
            ratios[f"{nm} {k}"] = M.worst(f32[k], f[k], b, pb.valid)
    for nm, st in (("fresh", None), ("carried", M.ray_state(pb))):
        m, m32 = M.composite(pb, st, want_bounds=True), M.composite(pb, st, np.float32)
        for k in ("rgb", "opacity", "depth"):
            ratios[f"{nm} {k}"] = M.worst(m32[k], m[k], m["bounds"][k])
        fin, fin32 = M.finalize([0.2, 0.5, 0.9], m32["rgb"], m32["opacity"], m32["depth"]), \
            M.finalize(np.float32([0.2, 0.5, 0.9]), m32["rgb"], m32["opacity"], m32["depth"], np.float32)
        ratios[f"{nm} final rgb"] = M.worst(fin32[0], fin[0], fin[2])
        ratios[f"{nm} final depth"] = M.worst(fin32[1], fin[1], fin[3])
    w32 = pb.scatter(M.forward(pb, dtype=np.float32)["w"])
    out0 = M.ray_state(pb)[0]
    acc, b = M.accumulate(pb, w32, pb.rgb, out0)
    ratios["accumulate"] = M.worst(M.accumulate(pb, w32, pb.rgb, out0, np.float32)[0], acc, b)
    q, alive, op, dp, rgb, _ = M.stepper_setup(pb)
    r64 = M.composite_test(q, alive, op, dp, rgb, M.T_THR, M.A_THR)
    r32 = M.composite_test(q, alive, op, dp, rgb, M.T_THR, M.A_THR, np.float32)
    ok = r64["robust"]
    robust = np.ones(op.shape[0], bool); robust[alive[~ok]] = False      # per target ray; untouched rays must stay equal
    assert np.array_equal(r32["alive"][ok], r64["alive"][ok])
    assert ok.mean() >= 0.9 or pb.n_rays < 10
    for k in ("opacity", "depth", "rgb"):
        ratios[f"test {k}"] = M.worst(r32[k], r64[k], r64["bounds"][k], robust[:, None])
    print(f"F32MODEL forward {pb.name}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios


def test_forced_stops_cover_first_middle_last():
    pb = M.make("edge257", "mixed")
    q, alive, op, dp, rgb, rays = M.stepper_setup(pb)
    assert len(rays) == 3
    out = M.composite_test(q, alive, op, dp, rgb, M.T_THR, M.A_THR, np.float32)
    assert (out["alive"][rays] == -1).all() and out["stopped"][rays].all()
    assert (out["alive"][pb.packed[:, 1] == 0] == -1).all() and (out["alive"] != -1).any()
    # nothing behind the stop is composited: the opaque sample alone gives opacity 1 - (1 - opacity_0) * 0
    assert np.allclose(out["opacity"][alive[rays], 0], 1.0, atol=1e-6)
    out = M.composite_test(M.make("all_empty", "mixed"), *M.stepper_setup(M.make("all_empty", "mixed"))[1:5], M.T_THR, M.A_THR)
    assert (out["alive"] == -1).all() and not out["stopped"].any()


@pytest.mark.parametrize("shape,regime", _problems(M.BACKWARD_CASES))
def test_float32_model_meets_the_backward_bounds(shape, regime):
    pb = M.make(shape, regime)
    u = pb.used
    worst = {}
    for which in M.GRADS:
        g = M.ray_grads(pb, which)
        ds, dr, bs, br, _ = M.backward(pb, *g, want_bounds=True)
        ds32, dr32 = M.backward(pb, *g, dtype=np.float32)
        assert np.isfinite(ds[u]).all() and np.isfinite(dr[u]).all() and np.isfinite(bs[u]).all()
        worst[which] = (M.worst(ds32[u], ds[u], bs[u]), M.worst(dr32[u], dr[u], br[u]))
    print(f"F32MODEL backward {pb.name}: " + ", ".join(f"{k} {a:.3f}/{b:.3f}" for k, (a, b) in worst.items()))
    assert max(max(v) for v in worst.values()) <= 1.0, worst


def test_reduce_problem_runs():
    for n in M.REDUCE_N:
        ri, vals, w = M.reduce_problem(n, 3, "one")
        runs = np.bincount(ri, minlength=n)
        assert set(runs[runs > 0]) <= set(M.RUN_LENGTHS) and (np.diff(ri) >= 0).all() and w.shape == (ri.shape[0], 1)
    runs = np.bincount(M.reduce_problem(65, 1, "none")[0], minlength=65)
    assert set(runs[runs > 0]) == set(M.RUN_LENGTHS) and (runs == 0).any()
