"""GPU suite: the one-launch training-batch sampler (csrc/train_batch.hip, trainset.TrainViews.batch) against the numpy
statement of its random numbers, the full-frame ray kernels and the reference's pixel arithmetic, bit for bit."""
import os

import numpy as np
import pytest
import torch

from ced_nerf_amd import cameras, synthetic as S, trainset
from ced_nerf_amd.trainset import TrainViews

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def N(t):
    return t.detach().cpu().numpy()


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _pinhole_views(V=5, W=37, H=29, seed=0):
    rng = np.random.default_rng(seed)
    imgs = rng.integers(0, 256, size=(V, H, W, 4), dtype=np.uint8)
    imgs[0, :, :, 3] = 255                     # opaque and transparent pixels among the random alphas
    imgs[V - 1, :4, :, 3] = 0
    Ks, c2ws = [], []
    for v in range(V):
        f = 30.0 + 3.5 * v
        Ks.append([[f, 0, W / 2.0 + 0.25 * v], [0, f * 1.01, H / 2.0 - 0.5 * v], [0, 0, 1]])
        c2ws.append(S.look_at_c2w(4.0, 10.0 + 7.0 * v, 30.0 + 55.0 * v, True))
    Ks, c2ws = np.asarray(Ks, np.float32), np.asarray(c2ws, np.float32)
    ts = rng.random(V).astype(np.float32)
    return TrainViews.pinhole(imgs, Ks, c2ws, ts, device=DEV), imgs, Ks, c2ws, ts


def test_pinhole_per_ray_batch_is_the_restated_draws_rays_and_pixels():
    views, imgs, Ks, c2ws, ts = _pinhole_views()
    V, H, W = imgs.shape[:3]
    n = 1 << 16
    full = [cameras.pinhole_rays(Ks[v], c2ws[v], W, H, True, device=DEV) for v in range(V)]
    for bkgd in ("white", "black", "random"):
        out = views.batch(n, step=3, bkgd=bkgd, seed=11, return_indices=True)
        torch.cuda.synchronize()
        view, x, y, colour = trainset.draws(11, 3, n, V, W, H, "per_ray", bkgd)
        idx = N(out["indices"])
        assert np.array_equal(idx[:, 0], view) and np.array_equal(idx[:, 1], x) and np.array_equal(idx[:, 2], y)
        assert len(np.unique(view)) == V
        # rays: the full-frame kernel's ray of the same pixel, bit for bit
        want_o = np.empty((n, 3), np.float32)
        want_d = np.empty((n, 3), np.float32)
        for v in range(V):
            sel = view == v
            want_o[sel] = N(full[v].origins)[y[sel], x[sel]]
            want_d[sel] = N(full[v].viewdirs)[y[sel], x[sel]]
        assert bits_equal(N(out["rays"].origins), want_o)
        assert bits_equal(N(out["rays"].viewdirs), want_d)
        # pixels: the torch statement of dnerf_synthetic.py:145-158 on the same indices (float32 true division)
        rgba = torch.from_numpy(imgs)[torch.from_numpy(view).long(), torch.from_numpy(y).long(),
                                      torch.from_numpy(x).long()] / 255.0
        pixels, alpha = torch.split(rgba, [3, 1], dim=-1)
        bk = torch.from_numpy(colour)
        want_px = pixels * alpha + bk * (1.0 - alpha)
        assert bits_equal(N(out["pixels"]), want_px.numpy())
        assert bits_equal(N(out["timestamps"]), ts[view][:, None])
        assert bits_equal(N(out["color_bkgd"]), colour)
        if bkgd == "random":
            assert 0.0 <= colour.min() and colour.max() < 1.0 and len(set(colour.tolist())) == 3


def _golden_hypercams():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hypercam_rays.npz"))
    cams = []
    for tag in ("plain", "distorted"):
        cams.append(dict(orientation=g[tag + "_orientation"], position=g[tag + "_position"],
                         focal_length=float(g[tag + "_focal_length"]), principal_point=g[tag + "_principal_point"],
                         skew=float(g[tag + "_skew"]), pixel_aspect_ratio=float(g[tag + "_pixel_aspect_ratio"]),
                         radial_distortion=g[tag + "_radial_distortion"],
                         tangential_distortion=g[tag + "_tangential_distortion"]))
    return cams, tuple(int(v) for v in g["plain_image_size"])


def test_hypercam_one_per_step_batch_matches_the_full_frame_kernel():
    cams, (W, H) = _golden_hypercams()
    rng = np.random.default_rng(1)
    imgs = rng.integers(0, 256, size=(len(cams), H, W, 3), dtype=np.uint8)
    ts = np.array([0.25, 0.75], np.float32)
    views = TrainViews.hypercam(imgs, cams, ts, device=DEV)
    full = [cameras.hypercam_rays(image_size=(W, H), device=DEV, **c) for c in cams]
    n = 4099
    seen = set()
    for step in range(12):
        out = views.batch(n, step=step, bkgd="black", seed=5, return_indices=True)
        view, x, y, _ = trainset.draws(5, step, n, len(cams), W, H, "one_per_step", "black")
        idx = N(out["indices"])
        assert np.array_equal(idx, np.stack([view, x, y], 1))
        v = int(view[0])
        assert (idx[:, 0] == v).all()                      # one view per batch
        seen.add(v)
        assert bits_equal(N(out["rays"].origins), N(full[v].origins)[y, x])
        assert bits_equal(N(out["rays"].viewdirs), N(full[v].viewdirs)[y, x])
        assert bits_equal(N(out["pixels"]), imgs[v, y, x].astype(np.float32) / np.float32(255.0))
        assert bits_equal(N(out["timestamps"]), np.full((n, 1), ts[v], np.float32))
        assert bits_equal(N(out["color_bkgd"]), np.zeros(3, np.float32))
    assert seen == {0, 1}                                  # the undistorted and the distorted camera both drawn


def test_batches_are_a_function_of_seed_and_step():
    views = _pinhole_views()[0]
    a = views.batch(5000, step=9, bkgd="random", seed=3, return_indices=True)
    b = views.batch(5000, step=9, bkgd="random", seed=3, return_indices=True)
    c = views.batch(5000, step=10, bkgd="random", seed=3, return_indices=True)
    for k in ("pixels", "timestamps", "color_bkgd", "indices"):
        assert torch.equal(a[k], b[k]), k
        assert not torch.equal(a[k], c[k]), k
    assert torch.equal(a["rays"].viewdirs, b["rays"].viewdirs) and not torch.equal(a["rays"].viewdirs, c["rays"].viewdirs)


def test_draws_are_uniform_at_2_pow_20_rays():
    from scipy.stats import chi2
    views, imgs = _pinhole_views()[:2]
    V, H, W = imgs.shape[:3]
    n = 1 << 20
    out = views.batch(n, step=1, bkgd="white", seed=2024, return_indices=True)
    idx = N(out["indices"])
    view, x, y, _ = trainset.draws(2024, 1, n, V, W, H, "per_ray", "white")
    assert np.array_equal(idx, np.stack([view, x, y], 1))

    def chi_square_ok(counts):
        counts = counts.reshape(-1).astype(np.float64)
        e = counts.sum() / counts.size
        stat = ((counts - e) ** 2 / e).sum()
        return stat < chi2.ppf(1 - 1e-6, counts.size - 1), stat

    for counts in (np.bincount(idx[:, 0], minlength=V), np.bincount(idx[:, 1], minlength=W),
                   np.bincount(idx[:, 2], minlength=H), np.bincount(idx[:, 2] * W + idx[:, 1], minlength=W * H),
                   np.bincount((idx[:, 0] * H + idx[:, 2]) * W + idx[:, 1], minlength=V * W * H)):
        ok, stat = chi_square_ok(counts)
        assert ok, (counts.size, stat)


@pytest.mark.parametrize("n,V", [(1, 5), (257, 5), (257, 1), (1, 1)])
def test_edge_sizes(n, V):
    views, imgs, Ks, c2ws, ts = _pinhole_views(V=V, W=13, H=7, seed=V)
    out = views.batch(n, step=0, bkgd="black", seed=0, return_indices=True)
    view, x, y, _ = trainset.draws(0, 0, n, V, 13, 7, "per_ray", "black")
    assert np.array_equal(N(out["indices"]), np.stack([view, x, y], 1))
    assert out["pixels"].shape == (n, 3) and out["timestamps"].shape == (n, 1)
    full = np.stack([N(cameras.pinhole_rays(Ks[v], c2ws[v], 13, 7, True, device=DEV).viewdirs) for v in range(V)])
    assert bits_equal(N(out["rays"].viewdirs), full[view, y, x])
