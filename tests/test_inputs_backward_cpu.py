"""The pieces of pose / time refinement that need no GPU, in float64.

1  inputs64.train_inputs_backward + reduce_rays (the formulas ced_train_inputs_backward is defined by) against autograd of
   F.frequency4 / F.sh2 / o + d t_mid.  Bound per ray and component: (m_r + 32) 2^-53 A_r, A_r the sum of the absolute
   values of the ray's elementary terms (inputs64's A).  Derivation: both sides evaluate sin / cos at the same float64
   angle (under 1 ulp each); a Frequency term is then a product of three factors and a difference of two such products
   (4 roundings), a sample sums four of them and the upstream gradient (4), the ray's term multiplies by t_mid and adds
   the direction term (2), whose own chain -- norm, division, dot product, projection, division -- is 12 operations;
   autograd performs the same count in another order, so 2 x 16 = 32 covers both, and any order of summing m_r terms adds
   at most (m_r - 1).  About 1e-12 at these magnitudes.
2  train.rodrigues against torch.linalg.matrix_exp of [rot]x, value and gradient, at rot = 0 and at |rot| on both sides
   of the series switch (1e-4).
3  CameraRefinement at its initial zeros is the identity, bit for bit.
4  The convergence reference of test_gpu_inputs_backward's align_view test: on a fixed sample set of the same scene,
   plain gradient descent on (rot, dt) through the float64 model brings the rotation error and the time error down.
   The scene moves by moving_step = 1e-4 of its box, so a time offset of 0.1 changes a colour by about 2e-3, as much as a
   rotation of a few 1e-6 rad: the offsets (ALIGN_ROT, ALIGN_DT) are chosen so that both are visible in the same image,
   and each parameter descends with a step of its own size (1 / its curvature, measured: 9e4 per rad^2 and 3e-4 per
   unit of time squared at these samples).  Measured: rotation error x 0.37, time error x 0.006 after 40 steps.
"""
import numpy as np
import pytest
import torch

import field64 as F
import inputs64 as I


ALIGN_AXIS = np.array([0.6, -0.3, 0.74]) / np.linalg.norm([0.6, -0.3, 0.74])
ALIGN_ROT, ALIGN_DT = 1e-5, 0.1              # the known pose and time offsets of the align_view tests (rad, time units)


def _ray_batch(counts, seed):
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts)
    n_rays, n = counts.shape[0], int(counts.sum())
    o = rng.uniform(-0.5, 0.5, size=(n_rays, 3))
    d = rng.normal(size=(n_rays, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[::3] *= rng.uniform(0.5, 3.0, size=(d[::3].shape[0], 1))                 # |rays_d| != 1 on every third ray
    ts = rng.uniform(0, 1, size=n_rays)
    ri = np.repeat(np.arange(n_rays), counts)
    k = np.arange(n) - (np.cumsum(counts) - counts)[ri]
    t0 = 0.3 + 2e-3 * k
    return dict(o=o, d=d, ts=ts, ri=ri, t0=t0, t1=t0 + 2e-3, n=n, n_rays=n_rays)


def test_formulas_match_autograd_of_the_input_stage():
    b = _ray_batch([0, 1, 2, 63, 64, 65, 0, 255, 1, 0], 3)
    up = {k: torch.from_numpy(v).double() for k, v in I.upstream(b["n"], 5).items()}
    o, d, ts = (torch.from_numpy(b[k]).requires_grad_() for k in ("o", "d", "ts"))
    ri = torch.from_numpy(b["ri"])
    tm = torch.from_numpy((b["t0"] + b["t1"]) / 2.0)
    pos = o[ri] + d[ri] * tm[:, None]
    tt = ts[ri]
    enc = F.frequency4(torch.cat([pos, tt[:, None]], dim=-1))
    sh = F.sh2(d[ri])
    ((pos * up["d_pos"]).sum() + (enc * up["d_enc"]).sum() + (sh * up["d_sh"]).sum() + (tt * up["d_t"]).sum()).backward()
    g, A = I.train_inputs_backward(torch.cat([pos, tt[:, None]], dim=-1).detach(), d[ri].detach(), **up)
    got, absum = I.reduce_rays(g, A, tm, ri, b["n_rays"])
    m = torch.bincount(ri, minlength=b["n_rays"]).double()
    for name, have, want, a in zip(("rays_o", "rays_d", "ts"), got, (o.grad, d.grad, ts.grad), absum):
        mm = m[:, None] if have.dim() == 2 else m
        bound = (mm + 32) * 2.0 ** -53 * a
        err = (have - want).abs()
        print(f"INPUTS64 {name}: err/bound max {float((err / bound.clamp_min(1e-300)).max()):.3f}, bound max {float(bound.max()):.2e}")
        assert (err <= bound).all()
        assert (have[m == 0] == 0).all() and float(want.abs().max()) > 1.0


@pytest.mark.parametrize("norm", [0.0, 0.5e-4, 0.99e-4, 1.01e-4, 2e-4, 0.3, 2.5])
def test_rodrigues_matches_the_matrix_exponential(norm):
    from ced_nerf_amd.train import rodrigues
    axis = torch.tensor([0.3, -0.5, 0.81], dtype=torch.float64)
    rot0 = axis / axis.norm() * norm
    G = torch.tensor([[0.7, -1.1, 0.4], [1.3, 0.2, -0.9], [-0.6, 0.8, 1.5]], dtype=torch.float64)

    def skew(r):
        o = torch.zeros((), dtype=r.dtype)
        return torch.stack([torch.stack([o, -r[2], r[1]]), torch.stack([r[2], o, -r[0]]), torch.stack([-r[1], r[0], o])])
    out = []
    for fn in (rodrigues, lambda r: torch.linalg.matrix_exp(skew(r))):
        r = rot0.clone().requires_grad_()
        R = fn(r)
        (R * G).sum().backward()
        out.append((R.detach(), r.grad))
    # float64 evaluations of entries of order 1: a few ulp each; the series' first dropped term is |rot|^6 / 5040 < 1e-27
    assert (out[0][0] - out[1][0]).abs().max().item() <= 1e-14
    assert (out[0][1] - out[1][1]).abs().max().item() <= 1e-12
    assert torch.isfinite(out[0][1]).all()
    if norm == 0.0:                                    # the gradient of I + [rot]x
        want = torch.stack([G[2, 1] - G[1, 2], G[0, 2] - G[2, 0], G[1, 0] - G[0, 1]])
        assert torch.equal(out[0][0], torch.eye(3, dtype=torch.float64)) and torch.allclose(out[0][1], want, rtol=0, atol=1e-15)


@pytest.mark.parametrize("poses,times", [(True, True), (True, False), (False, True)])
def test_camera_refinement_starts_as_the_identity(poses, times):
    from ced_nerf_amd.train import CameraRefinement
    gen = torch.Generator().manual_seed(2)
    o, d = torch.randn(257, 3, generator=gen), torch.randn(257, 3, generator=gen)
    ts = torch.rand(257, 1, generator=gen)
    view = torch.randint(0, 5, (257,), generator=gen)
    ref = CameraRefinement(5, poses=poses, times=times)
    assert sorted(k for k, _ in ref.named_parameters()) == sorted((["rot", "trans"] if poses else []) + (["dt"] if times else []))
    assert all(float(p.detach().abs().max()) == 0.0 for p in ref.parameters())
    o2, d2, t2 = ref(o, d, ts, view)
    assert torch.equal(o2, o) and torch.equal(d2, d) and torch.equal(t2, ts) and t2.shape == ts.shape
    if poses and times:
        (o2.sum() + (d2 * d).sum() + t2.sum()).backward()
        assert all(torch.isfinite(p.grad).all() for p in ref.parameters())
        with torch.no_grad():
            ref.rot[1] = torch.tensor([0.0, 0.0, np.pi / 2]); ref.trans[1] = torch.tensor([1.0, 2.0, 3.0]); ref.dt[1] = 0.25
        x = torch.tensor([[1.0, 0.0, 0.0]])
        o3, d3, t3 = ref(x, x, torch.zeros(1, 1), torch.tensor([1]))
        assert torch.allclose(d3, torch.tensor([[0.0, 1.0, 0.0]]), atol=1e-6) and torch.equal(o3, torch.tensor([[2.0, 2.0, 3.0]]))
        assert float(t3.detach()) == 0.25


def _fixed_samples(sc, n_rays, seed, max_per_ray=48):
    """n_rays pixels of the scene whose rays cross the occupied cells, with the centres of the marching steps inside them
    (the first max_per_ray: the density of the "trained" regime ends a ray well before) -> (pixel, ray_indices, t_starts)."""
    cfg = sc["cfg"]
    O, D = sc["origins"].reshape(-1, 3).astype(np.float64), sc["viewdirs"].reshape(-1, 3).astype(np.float64)
    lo, hi = np.array(cfg["aabb"][:3]), np.array(cfg["aabb"][3:])
    R, occ, step = cfg["grid_resolution"], sc["binaries"][0], cfg["render_step_size"]
    mids = (np.arange(1600) + 0.5) * step + 2.0
    pixels, ri, t0 = [], [], []
    for p in np.random.default_rng(seed).permutation(O.shape[0]):
        c = np.floor((O[p] + D[p] * mids[:, None] - lo) / (hi - lo) * R).astype(int)
        inside = ((c >= 0) & (c < R)).all(axis=1)
        c = np.clip(c, 0, R - 1)
        hit = inside & occ[c[:, 0], c[:, 1], c[:, 2]]
        if hit.sum() < 8:
            continue
        m = mids[hit][:max_per_ray]
        ri += [len(pixels)] * len(m); t0 += list(m - step / 2); pixels.append(p)
        if len(pixels) == n_rays:
            break
    return np.array(pixels), np.array(ri, np.int64), np.array(t0, np.float32)


def test_gradient_descent_recovers_a_pose_and_a_time_offset_in_float64():
    from ced_nerf_amd import synthetic as S
    from ced_nerf_amd.train import CameraRefinement
    sc = S.make_scene("dnerf", 96, 72, "trained", log2_hashmap_size=15)
    pix, ri, t0 = _fixed_samples(sc, 64, 0)
    assert pix.shape[0] == 64 and ri.shape[0] > 2000
    f64 = torch.float64
    P = {k: v.detach() for k, v in F.make_params(sc["params"], f64).items()}
    o, d = (torch.from_numpy(sc[k].reshape(-1, 3)[pix]).to(f64) for k in ("origins", "viewdirs"))
    ts = torch.full((64, 1), float(sc["timestamps"].reshape(-1)[0]), dtype=f64)
    ri, t0 = torch.from_numpy(ri), torch.from_numpy(t0).to(f64)
    t1 = t0 + sc["cfg"]["render_step_size"]
    bk = torch.from_numpy(sc["render"]["render_bkgd"]).to(f64)
    view = torch.zeros(64, dtype=torch.int64)
    rot_star = torch.from_numpy(ALIGN_AXIS * ALIGN_ROT)

    def render(ref, target):
        oo, dd, tt = ref(o, d, ts, view)
        return I.render_loss(P, sc["params"], oo, dd, tt[:, 0], ri, t0, t1, target, bk)
    star = CameraRefinement(1).double()
    with torch.no_grad():
        star.rot[0] = rot_star; star.dt[0] = ALIGN_DT
        target = render(star, torch.zeros(64, 3, dtype=f64))[1]
    ref = CameraRefinement(1).double()
    errors = lambda: (float((ref.rot.detach()[0] - rot_star).norm()), abs(float(ref.dt.detach()[0]) - ALIGN_DT))
    before = errors()
    for _ in range(40):
        ref.zero_grad(set_to_none=True)
        render(ref, target)[0].backward()
        with torch.no_grad():
            ref.rot -= 3e-6 * ref.rot.grad; ref.dt -= 400.0 * ref.dt.grad
    after = errors()
    print(f"ALIGN64: rotation error {before[0]:.3e} -> {after[0]:.3e} ({after[0] / before[0]:.3f}), "
          f"time error {before[1]:.3e} -> {after[1]:.3e} ({after[1] / before[1]:.4f})")
    assert after[0] < before[0] and after[1] < before[1]
