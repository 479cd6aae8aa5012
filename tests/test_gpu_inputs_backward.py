"""Gradients at the rays and times in front of the field (ced_train_inputs_backward, ced_train_warp_backward_pos, the
autograd nodes that use them, CameraRefinement, train_step's refinement, align_view) against float64.

1, 2  The operator against inputs64.train_inputs_backward at the float32 positions the forward produced (what the kernel
      recomputes), per ray (explicit mode: per sample, m = 1) and component:  |got - want| <= (m_r + c) u A_r, u = 2^-24,
      m_r the ray's sample count, A_r the sum of the absolute values of the ray's elementary terms with |sin|, |cos| and
      |w| replaced by 1 (inputs64's A), c = 24 the roundings on the longest path of one term through the kernel:
        a Frequency term fl(pi 2^k) * (e_s * cos - e_c * sin): sin / cos to 4 u absolute (the argument pi * r with
        fl(pi) and one rounding, 1.2 u; the polynomials), product 1, difference 1, fl(pi) and the product 1.5      8
        the sample's sum ((a0 + a1) + a2) + a3 and the upstream gradient                                            4
        times t_mid, plus the direction term (d_rays_d only)                                                          2
        the direction term g_w - w (w . g_w), over |d|: w to 6 u absolute (norm 2.5, division 1, + 1 at magnitude
        2: 2, - 1: 1), K d_sh 1.5, a product and two sums of the dot product 3.5 on top of 7.5 per factor pair,
        w * dot 6 + 11 + 1, the difference 1, the division by the norm 3.5, the sum into the ray's term 1           23.5
      and any order of summing m_r terms adds at most (m_r - 1) u A_r.
3     The warp's d_pos on the nine points of test_warp_rules_on_the_faces_of_the_box, that test's bound.
4     Whole field: the gradients at rays_o, rays_d and ts within 4 e32 of field64's, e32 the error of field64's own
      float32 evaluation; the 14 parameter gradients bit-identical to a run without input gradients.
5     train_step with a CameraRefinement.  6  align_view.
Each test prints its figures (INBWD: worst error / bound; GSTAT; ALIGN: error ratios).
"""
import numpy as np
import pytest
import torch

import field64 as F
import inputs64 as I
from test_gpu_train_gradients import T, DEV, U, _hip_field, _hip_run, small_scene  # noqa: F401 (small_scene: a fixture)
from test_inputs_backward_cpu import ALIGN_AXIS, ALIGN_DT, ALIGN_ROT, _ray_batch

pytestmark = pytest.mark.gpu

ROUNDINGS = 24
COUNTS = [0, 1, 2, 63, 64, 65, 0, 255, 256, 257, 1531, 1, 0]
UPSTREAM = ("d_pos", "d_enc", "d_sh", "d_t")


def _check(tag, got, want, absum, m):
    for name, g, w, a in zip(("origins", "directions", "times"), got, want, absum):
        g = g.cpu().double()
        mm = m[:, None] if g.dim() == 2 else m
        bound = (mm + ROUNDINGS) * U * a
        err = (g - w).abs()
        print(f"INBWD {tag} {name}: err/bound max {float((err / bound.clamp_min(1e-300)).max()):.3f}, "
              f"largest |want| {float(w.abs().max()):.3e}")
        assert (err <= bound).all(), (tag, name)
        assert (g[mm.expand_as(g) == 0] == 0).all()


def test_operator_rays_mode():
    from ced_nerf_amd import ops
    from ced_nerf_amd.nerfacc_api import _packed_info_from
    b = _ray_batch(COUNTS, 3)
    n, R = b["n"], b["n_rays"]
    f32 = lambda k: T(b[k].astype(np.float32))
    o, d, ts, t0, t1, ri = f32("o"), f32("d"), f32("ts"), f32("t0"), f32("t1"), T(b["ri"])
    assert float((d.norm(dim=-1) - 1).abs().max()) > 0.4                              # |rays_d| != 1 on some rays
    up = {k: T(v) for k, v in I.upstream(n, 5).items()}
    packed = _packed_info_from(ri, R)
    fwd = dict(rays_o=o, rays_d=d, ray_indices=ri, t_starts=t0, t_ends=t1, timestamps=ts, packed_info=packed)
    pos, _, _, tt = ops.train_inputs(n, o, d, ri, t0, t1, ts)
    got = ops.train_inputs_backward(n, **fwd, **up)
    again = ops.train_inputs_backward(n, **fwd, **up)
    assert all(torch.equal(a, c) for a, c in zip(got, again))                           # the same bits every launch
    assert got[0].shape == (R, 3) and got[1].shape == (R, 3) and got[2].shape == (R,)
    v = torch.cat([pos, tt[:, None]], dim=-1).cpu()
    tm = ((t0 + t1) / 2.0).cpu()                                                        # float32, as the forward rounds it
    up64 = {k: x.cpu() for k, x in up.items()}
    g, A = I.train_inputs_backward(v, d[ri].cpu(), **up64)
    want, absum = I.reduce_rays(g, A, tm, ri.cpu(), R)
    m = torch.tensor(COUNTS, dtype=torch.float64)
    _check("rays", got, want, absum, m)
    assert float(want[0].abs().max()) > 1.0 and float(want[1].abs().max()) > 1.0 and float(want[2].abs().max()) > 1.0
    for k in UPSTREAM:                                                                  # NULL = zeros
        one = ops.train_inputs_backward(n, **fwd, **{**up, k: None})
        two = ops.train_inputs_backward(n, **fwd, **{**up, k: torch.zeros_like(up[k])})
        assert all(torch.equal(a, c) for a, c in zip(one, two)), k
    none = ops.train_inputs_backward(n, **fwd)
    assert all(float(x.abs().max()) == 0.0 for x in none)
    empty = ops.train_inputs_backward(0, o, d, ri[:0], t0[:0], t1[:0], ts, packed_info=_packed_info_from(ri[:0], R))
    assert all(float(x.abs().max()) == 0.0 for x in empty) and empty[0].shape == (R, 3)


@pytest.mark.parametrize("n", [1, 3, 64, 257])
def test_operator_explicit_mode(n):
    from ced_nerf_amd import ops
    rng = np.random.default_rng(n)
    pos = T(rng.uniform(-1.5, 1.5, size=(n, 3)).astype(np.float32))
    d = T((rng.normal(size=(n, 3)) * rng.uniform(0.5, 3.0, size=(n, 1))).astype(np.float32))
    ts = T(rng.uniform(0, 1, size=n).astype(np.float32))
    up = {k: T(v) for k, v in I.upstream(n, 7).items()}
    got = ops.train_inputs_backward(n, positions=pos, directions=d, timestamps=ts, **up)
    again = ops.train_inputs_backward(n, positions=pos, directions=d, timestamps=ts, **up)
    assert all(torch.equal(a, c) for a, c in zip(got, again))
    want, absum = I.train_inputs_backward(torch.cat([pos, ts[:, None]], dim=-1).cpu(), d.cpu(), **{k: x.cpu() for k, x in up.items()})
    _check(f"explicit{n}", got, want, absum, torch.ones(n, dtype=torch.float64))
    for k in UPSTREAM:
        one = ops.train_inputs_backward(n, positions=pos, directions=d, timestamps=ts, **{**up, k: None})
        two = ops.train_inputs_backward(n, positions=pos, directions=d, timestamps=ts, **{**up, k: torch.zeros_like(up[k])})
        assert all(torch.equal(a, c) for a, c in zip(one, two)), k


@pytest.mark.parametrize("use_div", [False, True])
def test_warp_position_gradient_on_the_faces_of_the_box(use_div):
    from ced_nerf_amd import ops
    aabb6 = [-1.5, -1.0, -2.0, 1.5, 1.0, 2.0]
    pos = np.array([[-1.5, 0, 0], [1.5, 0, 0], [0, -1.0, 0], [0, 1.0, 2.0], [0, 0.5, -1.0], [1.75, 0, 0], [0, 0, -2.5],
                    [-1.5, -1.0, -2.0], [1.5, 1.0, 2.0]], np.float32)
    n, w = pos.shape[0], 6 if use_div else 3
    mo = np.zeros((n, w), np.float32)
    d_xn = np.random.default_rng(0).uniform(0.5, 2.0, size=(n, 3)).astype(np.float32)
    d_pos = ops.train_warp_backward_pos(T(pos), T(mo), aabb6, 0.25, use_div, T(d_xn))
    pos64 = torch.from_numpy(pos).double().requires_grad_()
    xn64, _, _, _ = F.warp(pos64, torch.zeros(n, w, dtype=torch.float64), torch.tensor(aabb6, dtype=torch.float64), 0.25, use_div)
    (xn64 * torch.from_numpy(d_xn).double()).sum().backward()
    want = pos64.grad
    assert int((want == 0).sum()) >= 2 and int((want != 0).sum()) >= 20               # cut outside, passed on the faces
    assert torch.equal(d_pos.cpu() == 0, want == 0)
    assert (d_pos.cpu().double() - want).abs().max().item() <= 4 * U * want.abs().max().item()


def _hip_run_inputs(tf, pb, density_weight=0.1):
    """_hip_run with rays_o, rays_d and ts requiring gradients -> ({parameter: gradient}, {input: gradient})."""
    tf.zero_grad(set_to_none=True)
    leaves = {k: T(pb[k]).requires_grad_() for k in ("rays_o", "rays_d", "ts")}
    rgb, res = tf.forward_rays(leaves["rays_o"], leaves["rays_d"], T(pb["ri"]), T(pb["t0"]), T(pb["t1"]), leaves["ts"][:, None],
                               return_internal=True)
    io = res["interal_output"]
    wr = T(pb["wr"])
    loss = (rgb * wr).sum() + res["density"].sum() * density_weight + io["latent_losses"].sum() * 1e3 \
        + io["weight_losses"].sum() + (io["move"] * wr).sum() * 1e2
    loss.backward()
    return {k: p.grad.detach().cpu() for k, p in tf.named_parameters()}, {k: v.grad.detach().cpu() for k, v in leaves.items()}


def _spy_on_the_table_gradient(monkeypatch):
    """Records (positions, dy, times) of every table-gradient launch."""
    from ced_nerf_amd import ops
    seen = []
    plain_bwd, temporal_bwd = ops.hash_encode_backward, ops.hash_encode_backward_temporal

    def spy(desc, x, dy, *a, **kw):
        if kw.get("want_table", True):
            seen.append((x.clone(), dy.clone(), None))
        return plain_bwd(desc, x, dy, *a, **kw)

    def spy_temporal(desc, x, t, dy, *a, **kw):
        seen.append((x.clone(), dy.clone(), t.clone()))
        return temporal_bwd(desc, x, t, dy, *a, **kw)
    monkeypatch.setattr(ops, "hash_encode_backward", spy)
    monkeypatch.setattr(ops, "hash_encode_backward_temporal", spy_temporal)
    return seen


def _check_table_gradients(tag, seen, tf, g_a, g_b):
    """Two launches of the table gradient: the same inputs bit for bit, results within 2 (m_e + 4) u A_e per entry."""
    assert len(seen) == 2 and all(torch.equal(a, b) for a, b in zip(seen[0][:2], seen[1][:2]))
    x, dy, t = (None if v is None else v.cpu() for v in seen[0])
    cfg = dict(tf.hash_cfg)
    cfg.setdefault("temporal", False)
    m, A, _ = F.hash_grad_stats(x, dy, g_a.cpu(), cfg, t)
    gap = (g_a.cpu().double() - g_b.cpu().double()).abs().reshape(A.shape)
    bound = 2 * (m[..., None] + (5 if cfg["temporal"] else 4)) * U * A
    print(f"GSTAT {tag} hash_table: largest gap between the two runs / bound "
          f"{float((gap / bound.clamp_min(1e-300)).max()):.3f}, entries that differ {int((gap > 0).sum())} of {int((A > 0).sum())}")
    assert (gap <= bound).all() and float(A.max()) > 0


@pytest.mark.parametrize("case", range(len(F.FIELD_CASES)))
def test_whole_field_input_gradients(case, monkeypatch):
    """The parameter gradients of a run with input gradients against a run without: 13 of the 14 bit for bit.  The 14th,
    hash_table, is summed by hardware float atomics in an order that changes from launch to launch, so no two launches
    need agree in its last bits; for it the INPUTS of the table-gradient kernel (positions, dy) are bit-identical in the
    two runs, and the two results differ per entry by at most 2 (m_e + 4) u A_e: each is within (m_e + 4) u A_e of the
    exact sum of the same terms (test_gpu_train_gradients 3a; 5 roundings with the temporal table)."""
    pb = F.whole_field_case(case)
    _, gi64 = I.whole_field_run(pb, torch.float64)
    _, gi32 = I.whole_field_run(pb, torch.float32)
    e32 = F.noise_floor(gi32, gi64)
    tf = _hip_field(pb)
    seen = _spy_on_the_table_gradient(monkeypatch)
    _, g_plain = _hip_run(tf, pb)
    g_par, g_in = _hip_run_inputs(tf, pb)
    _check_table_gradients(f"inputs case{case}", seen, tf, g_plain["hash_table"], g_par["hash_table"])
    g_par, g_plain = ({k: v for k, v in g.items() if k != "hash_table"} for g in (g_par, g_plain))
    tf.fused_glue = False
    _, g_torch = _hip_run_inputs(tf, pb)
    bad = {}
    for tag, g in (("hip", g_in), ("torch_glue", g_torch)):
        for k in ("rays_o", "rays_d", "ts"):
            err = F.rel_err(g[k], gi64[k])
            print(f"GSTAT inputs case{case} {tag} {k}: e32 {e32[k]:.2e} err {err:.2e} ratio {err / e32[k]:.2f}")
            if not err <= 4.0 * e32[k]:
                bad[(tag, k)] = (err, e32[k])
    for k in ("rays_o", "rays_d", "ts"):
        assert (g_in[k][[7, 30]] == 0).all()                                             # the two rays without a sample
    differ = [k for k in g_plain if not torch.equal(g_par[k], g_plain[k])]
    print(f"GSTAT inputs case{case}: parameter gradients that differ from the run without input gradients: {differ}")
    assert len(g_plain) == 13 and not differ, differ
    assert not bad, bad


def test_train_step_with_a_camera_refinement(small_scene, monkeypatch):
    """train_step (SGD, lr = 0) on 2048 rays of the 96x72 scene, four views: a zero CameraRefinement leaves the loss and
    every field gradient bit-identical (hash_table: as in test_whole_field_input_gradients), and its own gradients are within 4 e32 of field64's on the samples the step drew."""
    from ced_nerf_amd import train as TR
    sc, est, _ = small_scene
    cfg = sc["cfg"]
    field = TR.TrainableField(sc["params"], DEV, use_feat_predict=True, use_weight_predict=True)
    heads = {g: [w.detach().cpu().numpy() for w in getattr(field, g)] for g in ("mlp_feat_prediction", "mlp_weight_prediction")}
    gen = torch.Generator(device=DEV).manual_seed(1)
    n_all = sc["origins"].shape[0] * sc["origins"].shape[1]
    idx = torch.randint(0, n_all, (2048,), device=DEV, generator=gen)
    target = torch.rand(2048, 3, device=DEV, generator=gen)
    o = T(sc["origins"]).reshape(-1, 3)[idx].contiguous(); d = T(sc["viewdirs"]).reshape(-1, 3)[idx].contiguous()
    view = (idx % 4).contiguous()
    bk = T(sc["render"]["render_bkgd"])
    rec = {}
    real = TR.rendering_train

    def spy(t_starts, t_ends, ray_indices, n_rays, rgb_sigma_fn, **kw):
        rec.update(t0=t_starts, t1=t_ends, ri=ray_indices)
        return real(t_starts, t_ends, ray_indices, n_rays, rgb_sigma_fn, **kw)
    monkeypatch.setattr(TR, "rendering_train", spy)
    ref = TR.CameraRefinement(4).to(DEV)
    seen = _spy_on_the_table_gradient(monkeypatch)
    outs, grads = [], []
    for extra in ({}, dict(refinement=ref, view_indices=view)):
        torch.manual_seed(11)
        outs.append(TR.train_step(field, est, torch.optim.SGD(field.parameters(), lr=0.0), o, d, T(sc["timestamps"]), target,
                                  cfg["render_step_size"], near_plane=cfg["near_plane"], far_plane=cfg["far_plane"],
                                  render_bkgd=bk, **extra))
        grads.append({k: p.grad.detach().clone() for k, p in field.named_parameters()})
    assert outs[0]["n_samples"] == outs[1]["n_samples"] == rec["ri"].shape[0] > 1000
    _check_table_gradients("step_refinement", seen, field, grads[0]["hash_table"], grads[1]["hash_table"])
    differ = [k for k in grads[0] if k != "hash_table" and not torch.equal(grads[0][k], grads[1][k])]
    print(f"STEP refinement: loss {outs[0]['loss']!r} / {outs[1]['loss']!r}; field gradients that differ: {differ}")
    assert outs[0]["loss"] == outs[1]["loss"] and not differ
    # the float64 (and float32) model on the recorded samples
    t0, t1, ri = (rec[k].cpu() for k in ("t0", "t1", "ri"))
    res = {}
    for dtype in (torch.float64, torch.float32):
        P = F.make_params(sc["params"], dtype, heads)
        cv = lambda a: a.detach().cpu().to(dtype)
        m = TR.CameraRefinement(4).to(dtype)
        ts = torch.full((2048, 1), float(sc["timestamps"].reshape(-1)[0]), dtype=dtype)
        oo, dd, tt = m(cv(o), cv(d), ts, view.cpu())
        out = F.field_forward_rays(P, sc["params"], oo, dd, ri, cv(t0), cv(t1), tt[:, 0])
        comp = F.composite(out["sigma"], out["rgb"], cv(t0), cv(t1), ri, 2048, cv(bk))
        loss, _ = F.step_loss(out, comp, cv(target), cv(t0), cv(t1), ri, 2048)
        loss.backward()
        res[dtype] = {k: p.grad for k, p in m.named_parameters()}
    e32 = F.noise_floor(res[torch.float32], res[torch.float64])
    bad = {}
    for k, p in ref.named_parameters():
        err = F.rel_err(p.grad, res[torch.float64][k])
        print(f"GSTAT step_refinement {k}: e32 {e32[k]:.2e} hip {err:.2e} ratio {err / e32[k]:.2f}")
        if not err <= 4.0 * e32[k]:
            bad[k] = (err, e32[k])
    assert set(e32) == {"rot", "trans", "dt"} and not bad, bad


def test_align_view_recovers_a_pose_and_a_time_offset(small_scene, monkeypatch):
    """The target is the scene rendered (1024 samples per ray at most, no jitter) from rays turned by ALIGN_ROT about
    ALIGN_AXIS at time t + ALIGN_DT: from zero, align_view brings both errors down (test_inputs_backward_cpu runs the same
    problem through the float64 model, on fixed samples; here stratified=False fixes them likewise -- with the training
    jitter the loss between two renders of this field stays near 2e-3, four hundred times what the rotation adds to it).
    The step sizes are Adam's, per parameter: a tenth of each offset."""
    from ced_nerf_amd import train as TR
    sc, est, _ = small_scene
    cfg = sc["cfg"]
    field = TR.TrainableField(sc["params"], DEV)
    o, d = T(sc["origins"]).reshape(-1, 3), T(sc["viewdirs"]).reshape(-1, 3)
    bk = T(sc["render"]["render_bkgd"])
    t = float(sc["timestamps"].reshape(-1)[0])
    star = TR.CameraRefinement(1).to(DEV)
    rot_star = T((ALIGN_AXIS * ALIGN_ROT).astype(np.float32))
    render = dict(render_step_size=cfg["render_step_size"], near_plane=cfg["near_plane"], far_plane=cfg["far_plane"])
    with torch.no_grad():
        star.rot[0] = rot_star; star.dt[0] = ALIGN_DT
        oo, dd, tt = star(o, d, torch.full((o.shape[0], 1), t, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV))
        oo, dd, tt = oo.contiguous(), dd.contiguous(), tt.contiguous()
        fused = field.shared_inference()
        fused.train()
        ri, t0, t1 = est.sampling(oo, dd, sigma_fn=lambda a, b, r: fused.query_rays(oo, dd, r, a, b, tt, want_rgb=False)[1],
                                  stratified=False, sigma_field=(fused, tt, True), **render)
        pixels = TR.rendering_train(t0, t1, ri, o.shape[0], lambda a, b, r: field.forward_rays(oo, dd, r, a, b, tt),
                                    render_bkgd=bk)[0]
    weights = {k: p.detach().clone() for k, p in field.named_parameters()}
    # the field is frozen: the MLPs take their input-gradient-only route and no table gradient is launched
    from ced_nerf_amd import ops

    def no_weight_gradient(*a, **kw):
        raise AssertionError("align_view computed a weight gradient")
    table_bwd = ops.hash_encode_backward

    def position_gradient_only(*a, **kw):
        assert kw.get("want_table", True) is False, "align_view computed a table gradient"
        return table_bwd(*a, **kw)
    for name in ("weight_grad", "mlp_backward_dw", "hash_encode_backward_temporal"):
        monkeypatch.setattr(ops, name, no_weight_gradient)
    monkeypatch.setattr(ops, "hash_encode_backward", position_gradient_only)
    out = TR.align_view(field, est, pixels, o, d, t, steps=60, lr=ALIGN_ROT / 10, lr_time=ALIGN_DT / 10, num_rays=4096,
                        render_bkgd=bk, stratified=False, **render)
    assert all(p.requires_grad and p.grad is None and torch.equal(p, weights[k]) for k, p in field.named_parameters())
    rot_err, dt_err = float((out["rot"] - rot_star).norm()), abs(float(out["dt"]) - ALIGN_DT)
    print(f"ALIGN: rotation error {ALIGN_ROT:.3e} -> {rot_err:.3e} ({rot_err / ALIGN_ROT:.3f}), time error {ALIGN_DT:.3e} -> "
          f"{dt_err:.3e} ({dt_err / ALIGN_DT:.3f}); loss {out['history'][0]:.3e} -> {out['history'][-1]:.3e}")
    assert len(out["history"]) == 60 and rot_err < ALIGN_ROT and dt_err < ALIGN_DT
