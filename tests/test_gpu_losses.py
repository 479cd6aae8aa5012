"""The training regularisers on the GPU: the HIP distortion loss (csrc/losses.hip) in its two routes against float64
oracles written here -- the O(n^2) pairwise sum for hand-built batches, a segmented-cumsum closed form at the training
bench's size -- its determinism, and train_step's loss switches (-d / -ae / -o / -wr, MSE)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------------------------
# float64 oracles
# ------------------------------------------------------------------------------------------------------------------
def _pairwise64(packed, w, t0, t1):
    """sum_rays [sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i s_i w_i^2] / n_norm, float64, differentiable in w."""
    total = w.new_zeros(())
    last = -1
    for r, (s0, cnt) in enumerate(packed.tolist()):
        if cnt == 0:
            continue
        last = r
        sl = slice(s0, s0 + cnt)
        m = (t0[sl] + t1[sl]) / 2
        s = t1[sl] - t0[sl]
        wr = w[sl]
        total = total + wr @ (m[:, None] - m[None, :]).abs() @ wr + (s * wr * wr).sum() / 3
    return total / (last + 1) if last >= 0 else total


def _weights64(packed, sig, t0, t1):
    """render_weight_from_density in float64 (differentiable in sig)."""
    out = []
    for s0, cnt in packed.tolist():
        sd = sig[s0:s0 + cnt] * (t1[s0:s0 + cnt] - t0[s0:s0 + cnt])
        acc = torch.cumsum(sd, 0) - sd
        out.append(torch.exp(-acc) * (1 - torch.exp(-sd)))
    return torch.cat(out) if out else sig.new_zeros(0)


def _closed_form64(packed, w, t0, t1):
    """The same loss and dL/dw (unscaled and scaled) from segmented cumsums, float64, any size."""
    w, t0, t1 = w.double(), t0.double(), t1.double()
    m, s = (t0 + t1) / 2, t1 - t0
    start, cnt = packed[:, 0], packed[:, 1]
    ray_of = torch.repeat_interleave(torch.arange(packed.shape[0], device=w.device), cnt)
    base = start[ray_of]

    def seg_excl(v):                                          # sum_{j<i} v_j within the ray
        c = torch.cumsum(v, 0)
        c0 = torch.cat([c.new_zeros(1), c])
        return c0[:-1] - c0[base]

    def seg_total(v):
        c0 = torch.cat([v.new_zeros(1), torch.cumsum(v, 0)])
        return c0[base + cnt[ray_of]] - c0[base]
    W_lt, WM_lt = seg_excl(w), seg_excl(w * m)
    W_gt, WM_gt = seg_total(w) - W_lt - w, seg_total(w * m) - WM_lt - w * m
    loss_sum = (2 * w * (m * W_lt - WM_lt)).sum() + (s * w * w).sum() / 3
    grad = 2 * (m * (W_lt - W_gt) + (WM_gt - WM_lt)) + 2.0 / 3.0 * s * w
    has = (cnt > 0).nonzero()
    n_norm = int(has.max()) + 1 if has.numel() else 1
    return loss_sum / n_norm, grad, n_norm


# ------------------------------------------------------------------------------------------------------------------
# hand-built batches
# ------------------------------------------------------------------------------------------------------------------
def _batch(counts, seed, zero_weights=False):
    """Ray-packed samples in marching order: per ray a start in [0.5, 2], intervals of 1e-3..2e-2 with occasional gaps;
    weights that sum to at most ~1 per ray (like rendering weights); densities with a moderate optical depth."""
    rng = np.random.default_rng(seed)
    t0s, t1s, ws, sigs = [], [], [], []
    for cnt in counts:
        s = rng.uniform(1e-3, 2e-2, cnt).astype(np.float32)
        gap = (rng.uniform(0, 1e-2, cnt) * (rng.random(cnt) < 0.3)).astype(np.float32)
        t0 = np.zeros(cnt, np.float32)
        t = np.float32(rng.uniform(0.5, 2.0))
        for i in range(cnt):
            t0[i] = t
            t = np.float32(np.float32(t + s[i]) + gap[i])
        t0s.append(t0); t1s.append((t0 + s).astype(np.float32))
        ws.append((rng.random(cnt) * (2.0 / max(cnt, 1))).astype(np.float32))
        sigs.append((rng.random(cnt) * (8.0 / max(cnt, 1)) * rng.uniform(0.2, 2.0) / s).astype(np.float32))
    cat = lambda a: np.concatenate(a) if a else np.zeros(0, np.float32)
    counts = np.asarray(counts, np.int64)
    packed = np.stack([np.cumsum(counts) - counts, counts], -1).astype(np.int64)
    w = cat(ws)
    if zero_weights:
        w = np.zeros_like(w)
    return T(packed), T(w), T(cat(t0s)), T(cat(t1s)), T(cat(sigs))


BATCHES = {
    "mixed": [0, 1, 2, 37, 1500, 0, 5, 0, 0],                # 0 / 1 / 2 / 37 / 1500 samples, trailing empty rays
    "zero_weights": [3, 0, 37, 1500, 2, 0],
    "single": [1],
}


def _get(name, seed=0):
    return _batch(BATCHES[name], seed, zero_weights=name == "zero_weights")


def _n_norm(packed):
    has = (packed[:, 1] > 0).nonzero()
    return int(has.max()) + 1 if has.numel() else 0


@pytest.mark.parametrize("name", list(BATCHES))
def test_distortion_weights_route_matches_pairwise_oracle(name):
    from ced_nerf_amd import ops
    packed, w, t0, t1, _ = _get(name)
    loss, inv_norm, ray_loss, grad = ops.distortion_loss(packed, w, t0, t1)
    n_norm = _n_norm(packed)
    assert inv_norm.item() == pytest.approx(1.0 / n_norm, rel=1e-7)
    w64 = w.double().requires_grad_()
    want = _pairwise64(packed, w64, t0.double(), t1.double())
    (g64,) = torch.autograd.grad(want, w64) if want.requires_grad else (torch.zeros_like(w64),)
    g64 = g64 * n_norm                                         # the kernel's gradient is unscaled
    if name == "zero_weights":
        assert loss.item() == 0.0 and float(ray_loss.abs().max()) == 0.0
    else:
        assert abs(loss.item() - want.item()) <= 1e-5 * abs(want.item()), (loss.item(), want.item())
    err = float((grad.double() - g64).abs().max())
    assert err <= 1e-6 * float(g64.abs().max()), (err, float(g64.abs().max()))
    # per-ray losses: the empty rays give 0
    assert torch.all(ray_loss[packed[:, 1] == 0] == 0)


@pytest.mark.parametrize("name", ["mixed", "single"])
def test_distortion_drop_in_autograd(name):
    """losses.distortion(ray_ids, w, t0, t1): [S] and [S,1], n_norm = ray_ids.max() + 1, gradient to w only."""
    from ced_nerf_amd import losses
    packed, w, t0, t1, _ = _get(name)
    ray_ids = torch.repeat_interleave(torch.arange(packed.shape[0], device=DEV), packed[:, 1])
    w64 = w.double().requires_grad_()
    want = _pairwise64(packed, w64, t0.double(), t1.double())
    (g64,) = torch.autograd.grad(want, w64)
    for shape in ((-1,), (-1, 1)):
        wg = w.clone().reshape(shape).requires_grad_()
        got = losses.distortion(ray_ids.reshape(shape), wg, t0.reshape(shape), t1.reshape(shape))
        assert got.dim() == 0
        assert abs(got.item() - want.item()) <= 1e-5 * want.item()
        (2.5 * got).backward()
        assert wg.grad.shape == wg.shape
        err = float((wg.grad.reshape(-1).double() - 2.5 * g64).abs().max())
        assert err <= 1e-6 * 2.5 * float(g64.abs().max()), err


def test_distortion_empty_inputs():
    from ced_nerf_amd import losses, ops
    e = torch.zeros(0, device=DEV)
    loss, inv, ray_loss, grad = ops.distortion_loss(torch.zeros((0, 2), dtype=torch.int64, device=DEV), e, e, e)
    assert loss.item() == 0.0 and inv.item() == 0.0 and ray_loss.numel() == 0 and grad.numel() == 0
    packed = torch.zeros((4, 2), dtype=torch.int64, device=DEV)                       # rays, but no samples
    loss, inv, ray_loss, d_sig = ops.distortion_loss_density(packed, e, e, e)
    assert loss.item() == 0.0 and torch.equal(ray_loss, torch.zeros(4, device=DEV)) and d_sig.numel() == 0
    assert losses.distortion(torch.zeros(0, dtype=torch.int64, device=DEV), e, e, e).item() == 0.0


@pytest.mark.parametrize("name", list(BATCHES))
def test_distortion_fused_route_matches_float64_autograd(name):
    from ced_nerf_amd import ops
    packed, _, t0, t1, sig = _get(name, seed=5)
    loss, inv_norm, ray_loss, d_sig = ops.distortion_loss_density(packed, sig, t0, t1)
    # the loss is the weights route's, bit for bit, fed by the forward's weights
    w, _, _ = ops.render_weights(packed, t0, t1, sig)
    loss_w, inv_w, ray_loss_w, _ = ops.distortion_loss(packed, w, t0, t1)
    assert torch.equal(loss, loss_w) and torch.equal(inv_norm, inv_w) and torch.equal(ray_loss, ray_loss_w)
    sig64 = sig.double().requires_grad_()
    want = _pairwise64(packed, _weights64(packed, sig64, t0.double(), t1.double()), t0.double(), t1.double())
    (g64,) = torch.autograd.grad(want, sig64)
    g64 = g64 * _n_norm(packed)
    assert abs(loss.item() - want.item()) <= 1e-5 * want.item(), (loss.item(), want.item())
    err = float((d_sig.double() - g64).abs().max())
    assert err <= 1e-5 * float(g64.abs().max()), (err, float(g64.abs().max()))


def test_distortion_from_density_autograd():
    from ced_nerf_amd import losses
    packed, _, t0, t1, sig = _get("mixed", seed=6)
    s = sig.clone().requires_grad_()
    got = losses.distortion_from_density(t0, t1, s, packed)
    (3.0 * got).backward()
    sig64 = sig.double().requires_grad_()
    want = _pairwise64(packed, _weights64(packed, sig64, t0.double(), t1.double()), t0.double(), t1.double())
    (g64,) = torch.autograd.grad(want, sig64)
    assert abs(got.item() - want.item()) <= 1e-5 * want.item()
    assert float((s.grad.double() - 3.0 * g64).abs().max()) <= 1e-5 * 3.0 * float(g64.abs().max())


# ------------------------------------------------------------------------------------------------------------------
# the training bench's size: real estimator.sampling output
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bench_samples():
    """262 144 random rays of the 800x800 D-NeRF-shaped scene (tools/bench_train.py's shape), marched by
    estimator.sampling with the trained field's density: (packed, t_starts, t_ends, sigmas)."""
    from ced_nerf_amd import synthetic as S
    from ced_nerf_amd.nerfacc_api import OccGridEstimator, _packed_info_from
    from ced_nerf_amd.train import TrainableField
    sc = S.make_scene("dnerf", 800, 800, "trained")
    cfg = sc["cfg"]
    est = OccGridEstimator(cfg["aabb"], 128, cfg["grid_levels"]).to(DEV)
    est.set_binaries(T(sc["binaries"]))
    fused = TrainableField(sc["params"], DEV).shared_inference()
    fused.train()
    o = T(sc["origins"]).reshape(-1, 3); d = T(sc["viewdirs"]).reshape(-1, 3)
    g = torch.Generator(device=DEV).manual_seed(0)
    idx = torch.randint(0, o.shape[0], (262144,), device=DEV, generator=g)
    ro, rd = o[idx].contiguous(), d[idx].contiguous()
    ts = T(sc["timestamps"]).reshape(-1, 1).float().expand(ro.shape[0], 1)

    def sigma_fn(t_starts, t_ends, ray_indices):
        return fused.query_rays(ro, rd, ray_indices, t_starts, t_ends, ts, want_rgb=False)[1]
    torch.manual_seed(0)
    ri, t0, t1 = est.sampling(ro, rd, sigma_fn=sigma_fn, near_plane=cfg["near_plane"], far_plane=cfg["far_plane"],
                              render_step_size=cfg["render_step_size"], stratified=True, sigma_field=(fused, ts, True))
    sig = sigma_fn(t0, t1, ri).reshape(-1).float().contiguous()
    packed = _packed_info_from(ri, ro.shape[0])
    assert t0.shape[0] > 500_000, t0.shape
    return packed, t0.contiguous(), t1.contiguous(), sig


def test_distortion_full_size_matches_closed_form(bench_samples):
    from ced_nerf_amd import ops
    packed, t0, t1, sig = bench_samples
    w, _, _ = ops.render_weights(packed, t0, t1, sig)
    loss, inv_norm, _, grad = ops.distortion_loss(packed, w, t0, t1)
    want, g64, n_norm = _closed_form64(packed, w, t0, t1)
    assert inv_norm.item() == pytest.approx(1.0 / n_norm, rel=1e-7)
    assert abs(loss.item() - want.item()) <= 1e-5 * want.item(), (loss.item(), want.item())
    err = float((grad.double() - g64).abs().max())
    assert err <= 1e-6 * float(g64.abs().max()), (err, float(g64.abs().max()))
    loss_d, _, _, d_sig = ops.distortion_loss_density(packed, sig, t0, t1)
    assert torch.equal(loss_d, loss)
    # d sigma from the float64 dL/dw through the weights' closed-form backward (composite backward's formula)
    g = g64
    ray_of = torch.repeat_interleave(torch.arange(packed.shape[0], device=DEV), packed[:, 1])
    base = packed[:, 0][ray_of]
    sd = sig.double() * (t1 - t0).double()
    ex = torch.cumsum(sd, 0) - sd                              # optical depth before each sample, over all rays
    tr = torch.exp(-(ex - ex[base]))
    w64 = tr * (1 - torch.exp(-sd))
    c0 = torch.cat([g.new_zeros(1), torch.cumsum(g * w64, 0)])
    suffix = c0[base + packed[:, 1][ray_of]] - c0[1:]          # sum_{k>i} g_k w_k within the ray
    want_ds = (t1 - t0).double() * (g * (tr - w64) - suffix)
    err = float((d_sig.double() - want_ds).abs().max())
    assert err <= 1e-5 * float(want_ds.abs().max()), (err, float(want_ds.abs().max()))


def test_distortion_is_deterministic(bench_samples):
    from ced_nerf_amd import ops
    packed, t0, t1, sig = bench_samples
    w, _, _ = ops.render_weights(packed, t0, t1, sig)
    a = ops.distortion_loss(packed, w, t0, t1)
    b = ops.distortion_loss(packed, w, t0, t1)
    c = ops.distortion_loss_density(packed, sig, t0, t1)
    d = ops.distortion_loss_density(packed, sig, t0, t1)
    for x, y in ((a, b), (c, d)):
        for u, v in zip(x, y):
            assert torch.equal(u, v)


# ------------------------------------------------------------------------------------------------------------------
# train_step
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_scene():
    from ced_nerf_amd import synthetic as S
    from ced_nerf_amd.nerfacc_api import OccGridEstimator
    sc = S.make_scene("dnerf", 96, 72, "trained", log2_hashmap_size=15)
    cfg = sc["cfg"]
    est = OccGridEstimator(cfg["aabb"], cfg["grid_resolution"], cfg["grid_levels"]).to(DEV)
    est.set_binaries(T(sc["binaries"]))
    return sc, est


def _step(field, est, sc, idx, target, seed, **kw):
    from ced_nerf_amd.train import train_step
    cfg = sc["cfg"]
    o = T(sc["origins"]).reshape(-1, 3); d = T(sc["viewdirs"]).reshape(-1, 3)
    opt = torch.optim.SGD(field.parameters(), lr=0.0)        # the parameters stay: both calls see the same field
    torch.manual_seed(seed)
    out = train_step(field, est, opt, o[idx].contiguous(), d[idx].contiguous(), T(sc["timestamps"]), target,
                     cfg["render_step_size"], near_plane=cfg["near_plane"], far_plane=cfg["far_plane"],
                     render_bkgd=T(sc["render"]["render_bkgd"]), **kw)
    grads = {n: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for n, p in field.named_parameters()}
    return out, grads


def _rays(sc, n=2048, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    n_all = sc["origins"].shape[0] * sc["origins"].shape[1]
    return torch.randint(0, n_all, (n,), device=DEV, generator=g)


def test_train_step_explicit_defaults_match_todays_call(small_scene):
    from ced_nerf_amd.train import TrainableField
    sc, est = small_scene
    field = TrainableField(sc["params"], DEV)
    idx = _rays(sc)
    target = torch.rand(idx.shape[0], 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    a, ga = _step(field, est, sc, idx, target, 7)
    b, gb = _step(field, est, sc, idx, target, 7, rgb_loss="smooth_l1", distortion_loss=False, acc_entropy_loss=False,
                  opacity_loss=False, weight_rgbper=False, loss_weights=None)
    assert a["loss"] == b["loss"] and a["n_samples"] == b["n_samples"] and a["n_samples"] > 0
    assert a["loss_terms"] == {} and b["loss_terms"] == {}
    for n in ga:
        scale = float(ga[n].abs().max())
        assert float((ga[n] - gb[n]).abs().max()) <= 1e-6 * max(scale, 1e-30), n
    # the MSE switch: a different loss on the same samples
    c, _ = _step(field, est, sc, idx, target, 7, rgb_loss="mse")
    assert c["n_samples"] == a["n_samples"] and c["loss"] != a["loss"]


def test_train_step_distortion_gradient_matches_float64(small_scene, monkeypatch):
    """(flag on) - (flag off) parameter gradients == 1e-3 x the gradient of the float64 distortion of the same samples
    through TrainableField's torch path.  The target is the field's own render, so the colour term's gradient is exactly
    zero and the difference carries no float-atomic noise of the hash-table gradient."""
    from ced_nerf_amd import train as TR
    from ced_nerf_amd.train import TrainableField
    sc, est = small_scene
    field = TrainableField(sc["params"], DEV)
    idx = _rays(sc, seed=3)
    rec = {}
    real = TR.rendering_train

    def spy(t_starts, t_ends, ray_indices, n_rays, rgb_sigma_fn, **kw):
        out = real(t_starts, t_ends, ray_indices, n_rays, rgb_sigma_fn, **kw)
        rec.update(t0=t_starts, t1=t_ends, ri=ray_indices, n_rays=n_rays, colors=out[0].detach().clone())
        return out
    monkeypatch.setattr(TR, "rendering_train", spy)
    _step(field, est, sc, idx, torch.zeros(idx.shape[0], 3, device=DEV), 11)
    target = rec["colors"]
    off, g_off = _step(field, est, sc, idx, target, 11)
    on, g_on = _step(field, est, sc, idx, target, 11, distortion_loss=True)
    assert on["n_samples"] == off["n_samples"] > 0 and set(on["loss_terms"]) == {"distortion"}
    # the float64 reference on the recorded samples, through the torch path of the field
    from ced_nerf_amd.nerfacc_api import _packed_info_from
    t0, t1, ri = rec["t0"], rec["t1"], rec["ri"]
    packed = _packed_info_from(ri, rec["n_rays"])
    o = T(sc["origins"]).reshape(-1, 3)[idx].contiguous(); d = T(sc["viewdirs"]).reshape(-1, 3)[idx].contiguous()
    ts = T(sc["timestamps"]).reshape(-1, 1).float().expand(idx.shape[0], 1)
    field.zero_grad(set_to_none=True)
    field.fused_glue = False
    try:
        _, sigma = field.forward_rays(o, d, ri, t0, t1, ts)
    finally:
        field.fused_glue = True
    w64 = _weights64(packed, sigma.reshape(-1).double(), t0.double(), t1.double())
    dist = _closed_form_loss64(packed, w64, t0.double(), t1.double())
    assert abs(on["loss_terms"]["distortion"] - dist.item()) <= 1e-4 * dist.item()
    (1e-3 * dist).backward()
    checked = 0
    for n, p in field.named_parameters():
        want = p.grad if p.grad is not None else torch.zeros_like(p)
        scale = float(want.abs().max())
        if scale == 0.0:
            continue
        err = float(((g_on[n] - g_off[n]) - want).abs().max())
        assert err <= 1e-4 * scale, (n, err, scale)
        checked += 1
    assert checked >= 3


def _closed_form_loss64(packed, w, t0, t1):
    """_closed_form64's loss, differentiable in w (float64)."""
    m, s = (t0 + t1) / 2, t1 - t0
    start, cnt = packed[:, 0], packed[:, 1]
    ray_of = torch.repeat_interleave(torch.arange(packed.shape[0], device=w.device), cnt)
    base = start[ray_of]

    def seg_excl(v):
        c0 = torch.cat([v.new_zeros(1), torch.cumsum(v, 0)])
        return c0[:-1] - c0[base]
    loss_sum = (2 * w * (m * seg_excl(w) - seg_excl(w * m))).sum() + (s * w * w).sum() / 3
    has = (cnt > 0).nonzero()
    return loss_sum / (int(has.max()) + 1)


def test_train_step_with_every_regulariser_reduces_the_loss(small_scene):
    """-d -ae -wr -o together (train_real.py:371-396): a student whose hash table was damaged relearns a teacher's
    renders, as in test_training_steps_reduce_the_loss, and every reported term is finite."""
    from ced_nerf_amd.train import TrainableField, train_step
    from ced_nerf_amd.utils import Rays, render_image
    sc, est = small_scene
    cfg, params = sc["cfg"], sc["params"]
    rk = dict(sc["render"]); bk = T(rk["render_bkgd"])
    teacher = TrainableField(params, DEV).to_inference(DEV)
    rays = Rays(T(sc["origins"]), T(sc["viewdirs"]))
    ts = T(sc["timestamps"])
    target = render_image(teacher, est, rays, timestamps=ts, **dict(rk, render_bkgd=bk))[0].reshape(-1, 3)
    student_p = dict(params); student_p["hash"] = dict(params["hash"])
    rng = np.random.default_rng(0)
    student_p["hash"]["table"] = (params["hash"]["table"] * 0.5 + rng.normal(size=params["hash"]["table"].shape) * 0.05).astype(np.float32)
    student = TrainableField(student_p, DEV)
    opt = torch.optim.Adam([student.hash_table], lr=2e-2)
    o = rays.origins.reshape(-1, 3); d = rays.viewdirs.reshape(-1, 3)
    idx_all = ((target - bk).abs().sum(dim=1) > 1e-3).nonzero().flatten()
    assert idx_all.numel() > 500
    g = torch.Generator(device=DEV).manual_seed(1)
    losses = []
    for step in range(30):
        idx = idx_all[torch.randint(0, idx_all.numel(), (2048,), device=DEV, generator=g)]
        out = train_step(student, est, opt, o[idx].contiguous(), d[idx].contiguous(), ts, target[idx].contiguous(),
                         cfg["render_step_size"], near_plane=cfg["near_plane"], far_plane=cfg["far_plane"],
                         cone_angle=cfg["cone_angle"], alpha_thre=0.0, render_bkgd=bk, distortion_loss=True,
                         acc_entropy_loss=True, weight_rgbper=True, opacity_loss=True)
        assert out["n_samples"] > 0 and np.isfinite(out["loss"])
        assert set(out["loss_terms"]) == {"opacity", "distortion", "acc_entropy", "weight_rgbper"}
        assert all(np.isfinite(v) for v in out["loss_terms"].values()), out["loss_terms"]
        losses.append(out["loss"])
    first, last = np.mean(losses[:5]), np.mean(losses[-5:])
    print("training losses (-d -ae -wr -o)", [round(x, 5) for x in losses[::5]])
    assert last < 0.7 * first, (first, last)


def test_rendering_train_want_weights_extras(small_scene):
    """want_weights: the per-sample entries of train_real.py:379-396 (weights differentiable, as in the reference)."""
    from ced_nerf_amd import losses
    from ced_nerf_amd.render import rendering_train
    from ced_nerf_amd.train import TrainableField
    sc, est = small_scene
    field = TrainableField(sc["params"], DEV)
    idx = _rays(sc, n=1024, seed=4)
    o = T(sc["origins"]).reshape(-1, 3)[idx].contiguous(); d = T(sc["viewdirs"]).reshape(-1, 3)[idx].contiguous()
    ts = T(sc["timestamps"]).reshape(-1, 1).float().expand(idx.shape[0], 1)
    fused = field.shared_inference(); fused.train()
    cfg = sc["cfg"]
    ri, t0, t1 = est.sampling(o, d, sigma_fn=lambda a, b, r: fused.query_rays(o, d, r, a, b, ts, want_rgb=False)[1],
                              near_plane=cfg["near_plane"], far_plane=cfg["far_plane"],
                              render_step_size=cfg["render_step_size"], stratified=True, sigma_field=(fused, ts, True))
    fn = lambda a, b, r: field.forward_rays(o, d, r, a, b, ts)
    base = rendering_train(t0, t1, ri, idx.shape[0], fn)
    full = rendering_train(t0, t1, ri, idx.shape[0], fn, want_weights=True)
    assert set(base[3]) == {"sigmas", "rgbs"}
    ex = full[3]
    assert {"weights", "ray_indices", "t_starts", "t_ends"} <= set(ex) and ex["weights"].requires_grad
    for a, b in zip(base[:3], full[:3]):
        assert torch.equal(a, b)
    # the reference's literal line, through the weights' autograd node, equals the fused route
    lit = losses.distortion(ex["ray_indices"], ex["weights"], ex["t_starts"], ex["t_ends"])
    from ced_nerf_amd.nerfacc_api import _packed_info_from
    fused_loss = losses.distortion_from_density(t0, t1, ex["sigmas"], _packed_info_from(ri, int(ri.max()) + 1))
    assert torch.equal(lit.detach(), fused_loss.detach())
    s_lit, = torch.autograd.grad(lit, ex["sigmas"], retain_graph=True)
    s_fused, = torch.autograd.grad(fused_loss, ex["sigmas"])
    assert float((s_lit - s_fused).abs().max()) <= 1e-5 * float(s_fused.abs().max())
