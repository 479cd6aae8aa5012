"""tests/field64.py -- the float64 model the training gradients are held to -- pinned without a GPU: its forward against the
C oracle, its derivatives against finite differences, its table-gradient scatter against the oracle's float64 sums, and
the float32 noise floor `e32` of the whole-field cases that tests/test_gpu_train_gradients.py uses as its yardstick.

Noise floor: e32 = ||g32 - g64|| / ||g64|| per parameter must stay <= 1e-3 on the reference alone.  It is bimodal: about
1e-6 when no sample changes a hash cell or a ReLU mask between the float32 and the float64 evaluation, 1e-4 .. 1e-3 per
such event (field64.whole_field_case says why the cases use max_res 64, where all six cases meet the cap; at max_res 256
and 1024 cases 1, 3 and 5 resp. 0, 1, 2, 4 and 5 exceeded it with 3e-3 .. 8e-3 on xyz_wrap / mlp_base.0 / mlp_head.0)."""
import numpy as np
import pytest
import torch

import field64 as F

CASES = range(len(F.FIELD_CASES))


def _forward_problem(case):
    from ced_nerf_amd import synthetic as S
    kw = dict(F.FIELD_CASES[case])
    p = S.init_field_params([-1.5, -1.5, -1.5, 1.5, 1.5, 1.5], 1e-3, 1024, 15, regime="init", seed=3 + case, **kw)
    tab = p["hash"]["table"]
    p["hash"]["table"] = (tab.astype(np.float32) * np.float32(3000.0)).astype(tab.dtype)
    rng = np.random.default_rng(5)
    n = 2003
    pos = rng.uniform(-1.6, 1.6, size=(n, 3)).astype(np.float32)                    # some points outside the box
    t = rng.uniform(0, 1, size=n).astype(np.float32); t[2] = 0; t[3] = 1
    d = rng.normal(size=(n, 3)).astype(np.float32)
    return p, pos, t, d


@pytest.mark.parametrize("case", CASES)
def test_forward_matches_the_c_oracle(oracle, case):
    """rgb 2e-5, density 2e-4 relative with the same zero pattern (test_trainable_field_matches_fused_kernel's bounds; the
    fp16-table cases 5e-5 / 2e-4 as in test_training_on_the_reference_table_types); hash features within 1e-6 of the largest."""
    p, pos, t, d = _forward_problem(case)
    want = oracle.OracleField(p).forward(pos, t, d, want_geo=True, want_xnorm=True)
    P = F.make_params(p, torch.float64)
    cv = lambda a: torch.from_numpy(a).double()
    with torch.no_grad():
        out = F.field_forward(P, p, cv(pos), cv(t), cv(d))
    f16 = p["hash"]["table"].dtype == np.float16
    sig, rgb = out["sigma"].numpy(), out["rgb"].numpy()
    assert np.array_equal(sig == 0, want["density"] == 0) and 0 < (sig == 0).sum() < sig.shape[0]
    assert np.abs(rgb - want["rgb"]).max() <= (5e-5 if f16 else 2e-5)
    nz = want["density"] != 0
    assert (np.abs(sig[nz] - want["density"][nz]) / want["density"][nz]).max() <= 2e-4
    assert np.abs(out["xn"].numpy() - np.clip(want["x_norm"], 0, 1)).max() <= 2e-7
    assert np.abs(out["bout"].numpy()[:, 1:] - want["base_mlp_out"]).max() <= (5e-5 if f16 else 2e-5)
    of = oracle.OracleField({"hash": p["hash"]})
    x = F.ray_ordered_points(3001, 2)
    tt = F.temporal_times(3001, 3)
    cfg = {k: v for k, v in p["hash"].items() if k != "table"}
    feats = of.hash_encode(x, tt if cfg["temporal"] else None)
    with torch.no_grad():
        got = F.hash_encode(cv(x), P["hash_table"], cfg, torch.from_numpy(tt)).numpy()
    assert np.abs(feats).max() > 0.05 and np.abs(got - feats).max() <= 1e-6 * np.abs(feats).max()


SMALL = dict(base_res=4, max_res=32, n_levels=4, log2_hashmap_size=6)          # dense and hashed levels, 256 entries


def _interior_points(cfg, n, seed):
    """points whose fraction lies in [0.05, 0.95] on every level and axis"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.02, 0.98, size=(20000, 3))
    fr = (x[:, None, :] * F.levels_of(cfg)["scale"][:, None].astype(np.float64) + 0.5) % 1.0
    x = x[((fr >= 0.05) & (fr <= 0.95)).all(axis=(1, 2))]
    assert x.shape[0] >= n
    return torch.from_numpy(x[:n].copy())


def test_model_derivatives_against_finite_differences():
    gc = lambda fn, inp: torch.autograd.gradcheck(fn, inp, eps=1e-6, atol=1e-7, rtol=1e-5)
    x = _interior_points(SMALL, 4, 0).requires_grad_()
    tab = torch.from_numpy(F.random_table(SMALL, np.float64, 1)).requires_grad_()
    assert gc(lambda a, b: F.hash_encode(a, b, SMALL, fp32_position=False), (x, tab))
    tcfg = dict(SMALL, temporal=True)
    ttab = torch.from_numpy(F.random_table(tcfg, np.float64, 2)).requires_grad_()
    tt = torch.tensor([0.1, 0.4, 0.7, 1.0], dtype=torch.float64)
    assert gc(lambda b: F.hash_encode(x.detach(), b, tcfg, tt, fp32_position=False), (ttab,))
    # the value of the fp32-position form is the exact form's up to the position's rounding; its derivative is the same
    y0 = F.hash_encode(x, tab, SMALL); y1 = F.hash_encode(x, tab, SMALL, fp32_position=False)
    assert (y0 - y1).abs().max().item() <= 32 * F.U * 8 * tab.abs().max().item()
    up = torch.randn_like(y0)
    for a, b in zip(torch.autograd.grad((y0 * up).sum(), (x, tab)), torch.autograd.grad((y1 * up).sum(), (x, tab))):
        assert (a - b).abs().max().item() <= 1e-4 * b.abs().max().item()
    # the warp (both heads of the motion MLP), away from the box's faces
    rng = np.random.default_rng(3)
    pos = torch.from_numpy(rng.uniform(-1.2, 1.2, size=(5, 3)))
    mo = torch.from_numpy(rng.normal(size=(5, 6))).requires_grad_()
    aabb = torch.tensor([-1.5, -1.5, -1.5, 1.5, 1.5, 1.5], dtype=torch.float64)
    assert gc(lambda m: F.warp(pos, m, aabb, 0.05, True)[:3], (mo,))
    # compositing: three rays (one empty), every output
    ri = torch.tensor([0, 0, 0, 2, 2, 2, 2])
    t0 = torch.tensor([0.1, 0.2, 0.3, 0.0, 0.1, 0.2, 0.3], dtype=torch.float64); t1 = t0 + 0.1
    sig = torch.from_numpy(rng.uniform(0.5, 5.0, size=7)).requires_grad_()
    rgb = torch.from_numpy(rng.uniform(0, 1, size=(7, 3))).requires_grad_()
    bk = torch.ones(3, dtype=torch.float64)

    def comp(s, c):
        o = F.composite(s, c, t0, t1, ri, 3, bk)
        return o["colors"], o["opacities"], o["trans"], F.distortion(o["weights"], t0, t1, ri, 3)
    assert gc(comp, (sig, rgb))
    # trunc_exp: exp's derivative below 15, the clamped one above
    v = torch.tensor([-2.0, 3.0, 14.0, 16.0, 20.0], dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(F.TruncExp.apply(v).sum(), v)
    assert torch.equal(g, torch.exp(v.detach().clamp(max=15.0)))


@pytest.mark.parametrize("kind", ["f32", "f16", "levels8", "temporal"])
def test_table_gradient_scatter_equals_the_oracles_sums(oracle, kind):
    """On a ray-ordered batch: the per-corner terms in the reference's float32 arithmetic, summed per entry in float64, are
    the C oracle's float64 sums to 1e-12 (same indices, same skip rule, same key-frame slots); and autograd's float64
    gradient of the model differs from them by the terms' own float32 roundings only (3 for w dy, 5 with the key-frame
    weight: each entry within 5 u A_e)."""
    cfg, dtype = HASH_KINDS[kind]
    table = F.random_table(cfg, dtype, 4)
    n = 4099
    x, dy, t = F.ray_ordered_points(n, 7), F.hash_dy(n, cfg["n_levels"], 8), F.temporal_times(n, 9)
    of = oracle.OracleField({"hash": dict(cfg, table=table)})
    temporal = cfg["temporal"]
    want = of.hash_encode_backward_temporal(x, t, dy) if temporal else of.hash_encode_backward(x, dy, want_dx=False)[0]
    tt = torch.from_numpy(t)
    got = F.table_grad_terms32(torch.from_numpy(x), torch.from_numpy(dy), cfg, tt).numpy()
    assert np.abs(want).max() > 1.0 and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    tab = torch.from_numpy(table.astype(np.float64)).requires_grad_()
    y = F.hash_encode(torch.from_numpy(x).double(), tab, cfg, tt)
    (y * torch.from_numpy(dy).double()).sum().backward()
    m, A, _ = F.hash_grad_stats(torch.from_numpy(x), torch.from_numpy(dy), tab, cfg, tt)
    err = np.abs(tab.grad.numpy() - want).reshape(A.shape)
    assert (err <= 5 * F.U * A.numpy()).all()
    assert (want.reshape(A.shape)[(m == 0).numpy()] == 0).all() and int((m > 100).sum()) > 0       # long runs are there


HASH_KINDS = {      # the tables of the hash-backward tests: (configuration, table dtype)
    "f32": (dict(base_res=16, max_res=1024, n_levels=16, log2_hashmap_size=15, temporal=False), np.float32),
    "f16": (dict(base_res=16, max_res=4096, n_levels=16, log2_hashmap_size=13, temporal=False), np.float16),
    "levels8": (dict(base_res=16, max_res=256, n_levels=8, log2_hashmap_size=15, temporal=False), np.float32),
    "temporal": (dict(base_res=16, max_res=1024, n_levels=16, log2_hashmap_size=13, temporal=True), np.float32),
}


@pytest.mark.parametrize("case", CASES)
def test_float32_noise_floor_of_the_whole_field_cases(case):
    """A condition on the reference, not a measurement: the float32 evaluation of the same graph on the same inputs gives
    every parameter's gradient within 1e-3 (in the norm) of the float64 one."""
    pb = F.whole_field_case(case)
    out64, g64 = F.whole_field_run(pb, torch.float64)
    out32, g32 = F.whole_field_run(pb, torch.float32)
    assert torch.equal(out32["selector"], out64["selector"]) and 0 < int(out64["selector"].sum()) < pb["ri"].shape[0]
    assert 3500 <= pb["ri"].shape[0] <= 4500
    e32 = F.noise_floor(g32, g64)
    print("E32", case, " ".join(f"{k}={v:.1e}" for k, v in e32.items()))
    assert len(e32) == 14 and all(float(g.norm()) > 0 for g in g64.values())
    assert max(e32.values()) <= 1e-3, e32
