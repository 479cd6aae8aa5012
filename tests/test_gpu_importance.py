"""GPU suite: DyNeRF's importance sampling -- the weight-map kernels (csrc/importance.hip) against their numpy
restatements bit for bit, the importance sampler (csrc/train_batch.hip, TrainViews.batch_importance) against
trainset.importance_draws in every index and against the full-frame ray kernels, and trainer.fit with ISG / IST maps."""
import numpy as np
import pytest
import torch

from ced_nerf_amd import cameras, importance, synthetic as S, trainer, trainset
from ced_nerf_amd.trainset import TrainViews

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def N(t):
    return t.detach().cpu().numpy()


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _views(imgs, seed=0):
    """RGB pinhole views (OpenCV cameras, one view per step: DyNeRF's) of `imgs` [V,H,W,3], a camera per view."""
    V, H, W = imgs.shape[:3]
    rng = np.random.default_rng(seed)
    Ks, c2ws = [], []
    for v in range(V):
        f = 30.0 + 1.5 * v
        Ks.append([[f, 0, W / 2.0 + 0.25 * (v % 5)], [0, f * 1.01, H / 2.0 - 0.5 * (v % 3)], [0, 0, 1]])
        c2ws.append(S.look_at_c2w(2.5, 10.0 + 3.0 * (v % 7), 20.0 + 17.0 * v, False))
    Ks, c2ws = np.asarray(Ks, np.float32), np.asarray(c2ws, np.float32)
    ts = rng.random(V).astype(np.float32)
    views = TrainViews.pinhole(imgs, Ks, c2ws, ts, opengl=False, device=DEV, view_mode="one_per_step")
    return views, Ks, c2ws, ts


# ---------------------------------------------------------------------------------------------------------------------
# Weight maps
# ---------------------------------------------------------------------------------------------------------------------
# (cameras, frames, height, width, largest byte value): even and odd T, T below the default frame_shift of 25 and above
# it, T = 1, sizes that are not multiples of the wave; few byte values make many equal values around the median
CLIPS = [(2, 7, 5, 9, 255), (3, 8, 13, 11, 255), (1, 30, 7, 5, 255), (2, 1, 6, 7, 255), (2, 12, 9, 10, 3),
         (1, 2, 3, 3, 255), (2, 53, 4, 5, 15)]


@pytest.mark.parametrize("c,t,h,w,top", CLIPS)
def test_weight_kernels_equal_their_restatements(c, t, h, w, top):
    rng = np.random.default_rng(c * 1000 + t)
    imgs = rng.integers(0, top + 1, size=(c * t, h, w, 3), dtype=np.uint8)
    imgs[: t, 0, 0] = imgs[0, 0, 0]                       # a static pixel
    views = _views(imgs)[0]
    med = importance.temporal_median(views, c)
    want_med = importance.temporal_median_reference(imgs, c)
    assert med.dtype == torch.uint8 and tuple(med.shape) == (c, h, w, 3)
    assert torch.equal(med.cpu(), torch.from_numpy(want_med))
    assert torch.equal(med.cpu(), torch.median(torch.from_numpy(imgs).view(c, t, h, w, 3), dim=1).values)
    for gamma in (2e-2, 1e-3):
        isg = importance.isg_weights(views, c, gamma=gamma)
        assert isg.dtype == torch.float32 and tuple(isg.shape) == (c, t, h, w)
        assert torch.equal(isg.cpu(), torch.from_numpy(importance.isg_weights_reference(imgs, c, gamma)))
        assert torch.equal(isg, importance.isg_weights(views, c, gamma=gamma, median=med))
    assert float(isg[0, :, 0, 0].abs().max()) == 0.0      # the static pixel
    for alpha, shift in ((0.1, 25), (0.1, 1), (2.5, 3), (0.1, 0)):
        ist = importance.ist_weights(views, c, alpha=alpha, frame_shift=shift)
        assert ist.dtype == torch.float32 and tuple(ist.shape) == (c, t, h, w)
        assert torch.equal(ist.cpu(), torch.from_numpy(importance.ist_weights_reference(imgs, c, alpha, shift))), (alpha, shift)


def test_weight_map_errors_on_the_device():
    imgs = np.zeros((6, 4, 5, 3), np.uint8)
    views = _views(imgs)[0]
    with pytest.raises(ValueError, match="cameras"):
        importance.temporal_median(views, 4)
    with pytest.raises(ValueError, match="median"):
        importance.isg_weights(views, 2, median=torch.zeros((3, 4, 5, 3), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="frame_shift"):
        importance.ist_weights(views, 2, frame_shift=-1)


# ---------------------------------------------------------------------------------------------------------------------
# The sampler
# ---------------------------------------------------------------------------------------------------------------------
def _check_batch(views, Ks, c2ws, ts, imgs, full, weights, num_rays, s, pool_size, seed, step, bkgd="random"):
    V, H, W = imgs.shape[:3]
    out = views.batch_importance(num_rays, step, torch.from_numpy(weights).to(DEV), weights_subsampled=s, bkgd=bkgd,
                                 seed=seed, pool_size=pool_size, return_indices=True)
    view, x, y = trainset.importance_draws(seed, step, num_rays, weights, s, pool_size, W, H)
    n = (num_rays // (s * s)) * s * s
    idx = N(out["indices"])
    assert idx.shape == (n, 3)
    assert np.array_equal(idx[:, 0], view) and np.array_equal(idx[:, 1], x) and np.array_equal(idx[:, 2], y), \
        (s, pool_size, num_rays, seed, step, int((idx != np.stack([view, x, y], 1)).any(1).sum()))
    # rays: the full-frame kernel's ray of the same pixel, bit for bit
    assert bits_equal(N(out["rays"].origins), full[0][view, y, x])
    assert bits_equal(N(out["rays"].viewdirs), full[1][view, y, x])
    assert bits_equal(N(out["pixels"]), imgs[view, y, x].astype(np.float32) / np.float32(255.0))
    assert bits_equal(N(out["timestamps"]), ts[view][:, None])
    _, _, _, colour = trainset.draws(seed, step, 1, V, W, H, "one_per_step", bkgd)
    assert bits_equal(N(out["color_bkgd"]), colour)
    return out, (view, x, y)


@pytest.fixture(scope="module")
def scene():
    rng = np.random.default_rng(5)
    V, H, W = 12, 29, 37                                   # 12 876 pixels: neither side a multiple of 2, 4 or the wave
    imgs = rng.integers(0, 256, size=(V, H, W, 3), dtype=np.uint8)
    views, Ks, c2ws, ts = _views(imgs)
    rays = [cameras.pinhole_rays(Ks[v], c2ws[v], W, H, False, device=DEV) for v in range(V)]
    full = (np.stack([N(r.origins) for r in rays]), np.stack([N(r.viewdirs) for r in rays]))
    return views, Ks, c2ws, ts, imgs, full


def _weights(kind, n, rng):
    if kind == "decades":                                  # zeros and three decades
        w = (10.0 ** rng.uniform(-3.0, 0.0, n)).astype(np.float32)
        w[rng.random(n) < 0.3] = 0.0
    elif kind == "two_values":                             # many exactly equal weights
        w = np.where(rng.random(n) < 0.5, 0.25, 1.0).astype(np.float32)
        w[rng.random(n) < 0.1] = 0.0
    elif kind == "overflow":                               # weight / variate overflows for variates below 1: equal keys (+inf)
        w = np.full(n, 3.0e38, np.float32)                 # in bulk, so the threshold itself is a tie won by the lower j
        w[rng.random(n) < 0.2] = 0.0
    else:
        raise KeyError(kind)
    return w


@pytest.mark.parametrize("s", [1, 2, 4])
@pytest.mark.parametrize("kind", ["decades", "two_values", "overflow"])
def test_batch_importance_equals_the_restated_draws(scene, s, kind):
    views, Ks, c2ws, ts, imgs, full = scene
    V, H, W = imgs.shape[:3]
    n = V * (H // s) * (W // s)
    rng = np.random.default_rng(s * 10 + len(kind))
    w = _weights(kind, n, rng)
    if kind == "overflow":
        cell, bits = trainset.importance_candidates(3, 0, w)
        assert int((bits == 0x7F800000).sum()) > n // 3    # the tie at the threshold is there
    pools = (2_000_000, max(64, n // 3))                   # every cell a candidate; a pool of a third of them
    for pool in pools:
        cand = min(n, pool)
        # k from 1 to more than one workgroup's tile of 1024 candidates' worth of selected cells
        ks = [1, 2, 63, 257, min(cand // 3, 1500)] + ([min(cand // 2, 3000)] if s == 1 else [])
        for i, k in enumerate(sorted({k for k in ks if 1 <= k <= cand // 2})):    # about 0.7 of a pool is positive
            seed, step = (11, 3) if i % 2 == 0 else (2024, 70000 + i)
            _check_batch(views, Ks, c2ws, ts, imgs, full, w, k * s * s + (s * s - 1), s, pool, seed, step)


def test_batch_importance_is_a_function_of_seed_and_step(scene):
    views, Ks, c2ws, ts, imgs, full = scene
    V, H, W = imgs.shape[:3]
    w = torch.rand(V * H * W, device=DEV)
    a = views.batch_importance(5000, 9, w, seed=3, return_indices=True)
    b = views.batch_importance(5000, 9, w, seed=3, return_indices=True)
    c = views.batch_importance(5000, 10, w, seed=3, return_indices=True)
    d = views.batch_importance(5000, 9, w, seed=4, return_indices=True)
    for k in ("pixels", "timestamps", "color_bkgd", "indices"):
        assert torch.equal(a[k], b[k]), k
        assert not torch.equal(a[k], c[k]) and not torch.equal(a[k], d[k]), k
    assert torch.equal(a["rays"].viewdirs, b["rays"].viewdirs) and torch.equal(a["rays"].origins, b["rays"].origins)
    idx = N(a["indices"]).astype(np.int64)
    cells = (idx[:, 0] * H + idx[:, 2]) * W + idx[:, 1]
    assert len(np.unique(cells)) == 5000 and np.all(np.diff(cells) > 0)    # without replacement, in cell order
    # scale invariance: the same cells from twice the weights (a power of two scales every key exactly)
    e = views.batch_importance(5000, 9, w * 2.0, seed=3, return_indices=True)
    assert torch.equal(a["indices"], e["indices"])


def test_larger_map_through_both_pool_paths():
    rng = np.random.default_rng(8)
    V, H, W = 20, 67, 101                                  # 135 340 cells
    imgs = rng.integers(0, 256, size=(V, H, W, 3), dtype=np.uint8)
    views, Ks, c2ws, ts = _views(imgs)
    rays = [cameras.pinhole_rays(Ks[v], c2ws[v], W, H, False, device=DEV) for v in range(V)]
    full = (np.stack([N(r.origins) for r in rays]), np.stack([N(r.viewdirs) for r in rays]))
    w = _weights("decades", V * H * W, rng)
    for pool, k in ((2_000_000, 20000), (100_000, 20000), (100_000, 1), (70_001, 33333)):
        _check_batch(views, Ks, c2ws, ts, imgs, full, w, k, 1, pool, seed=1, step=12345678901, bkgd="black")
    # inclusion follows the weights: the heavier half of the positive cells is drawn far more often
    out = views.batch_importance(20000, 5, torch.from_numpy(w).to(DEV), return_indices=True)
    idx = N(out["indices"]).astype(np.int64)
    drawn = w[(idx[:, 0] * H + idx[:, 2]) * W + idx[:, 1]]
    assert drawn.min() > 0 and np.median(drawn) > 2.0 * np.median(w[w > 0])


def test_too_few_positive_cells_is_a_value_error(scene):
    views, Ks, c2ws, ts, imgs, full = scene
    V, H, W = imgs.shape[:3]
    w = torch.zeros(V * H * W, device=DEV)
    w[::1000] = 1.0                                        # 13 positive cells
    positive = int((w > 0).sum())
    out = views.batch_importance(positive, 0, w, return_indices=True)
    idx = N(out["indices"]).astype(np.int64)
    assert np.array_equal((idx[:, 0] * H + idx[:, 2]) * W + idx[:, 1], np.arange(0, V * H * W, 1000))
    with pytest.raises(ValueError, match="positive"):
        views.batch_importance(positive + 1, 0, w)
    w[5] = float("nan")
    w[6] = float("inf")
    w[7] = -1.0
    with pytest.raises(ValueError, match="positive"):
        views.batch_importance(positive + 1, 0, w)
    with pytest.raises(ValueError, match="positive"):      # a pool that holds too few of them
        views.batch_importance(64, 0, w, pool_size=128)
    with pytest.raises(ValueError, match="on"):
        views.batch_importance(4, 0, w.cpu())


# ---------------------------------------------------------------------------------------------------------------------
# The training loop
# ---------------------------------------------------------------------------------------------------------------------
def _blob_clip(n_cameras=3, n_frames=8, size=40):
    """A noisy static background with one bright blob that moves across the frames, seen by n_cameras cameras."""
    rng = np.random.default_rng(17)
    yy, xx = np.mgrid[:size, :size]
    imgs, c2ws, ts = [], [], []
    for c in range(n_cameras):
        base = rng.integers(60, 120, size=(size, size, 3))
        for t in range(n_frames):
            img = base + rng.integers(-2, 3, size=(size, size, 3))
            cx, cy = 6 + 4 * t, 10 + 8 * c
            blob = np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 18.0)[..., None]
            imgs.append(np.clip(img + 130.0 * blob, 0, 255).astype(np.uint8))
            c2ws.append(S.look_at_c2w(2.5, 15.0, 30.0 + 40.0 * c, False))
            ts.append(t / (n_frames - 1))
    imgs = np.stack(imgs)
    focal = 0.5 * size / np.tan(0.45)
    K = np.array([[focal, 0, size / 2.0], [0, focal, size / 2.0], [0, 0, 1]], np.float32)
    views = TrainViews.pinhole(imgs, K, np.stack(c2ws), np.array(ts, np.float32), opengl=False, device=DEV,
                               view_mode="one_per_step")
    return views, imgs


# the DyNeRF preset on a toy clip: a coarser march and no alpha culling, so that the untrained field keeps samples
TARGET = 1 << 16
FIT = dict(preset="dynerf", log2_hashmap_size=15, target_sample_batch_size=TARGET, verbose=False, alpha_thre=0.0,
           render_step_size=5e-3)


def test_fit_with_isg_weights_and_the_ist_switch():
    views, imgs = _blob_clip()
    n_cameras, steps, switch = 3, 200, 120
    isg = importance.isg_weights(views, n_cameras)
    ist = importance.ist_weights(views, n_cameras, frame_shift=3)
    assert torch.equal(isg.cpu(), torch.from_numpy(importance.isg_weights_reference(imgs, n_cameras)))
    blob = isg[0, 2, 6:14, 10:18].mean()                   # camera 0, frame 2: the blob is at (14, 10)
    assert float(blob) > 10.0 * float(isg[0, 2, 28:, :].mean())
    kw = dict(FIT, max_steps=steps, use_time_embedding=True, use_div_offsets=True)
    w_isg, w_ist = isg.reshape(-1), ist.reshape(-1)
    calls, sample = [], views.batch_importance

    def recording(num_rays, step, weights, *a, **k):
        assert k == dict(bkgd="random", seed=42) and a == (1,)             # the preset's background, fit's seed, s = 1
        calls.append((num_rays, step, "isg" if weights is w_isg else "ist" if weights is w_ist else "?"))
        return sample(num_rays, step, weights, *a, **k)

    views.batch_importance = recording
    try:
        res = trainer.fit(views, None, sampling_weights=w_isg, ist_weights=w_ist, ist_from_step=switch, **kw)
    finally:
        del views.batch_importance
    hist = res["history"]
    assert [h["step"] for h in hist] == list(range(steps + 1))
    assert [h["sampling"] for h in hist] == ["isg"] * switch + ["ist"] * (steps + 1 - switch)
    assert hist[0]["num_rays"] == 1024 and all(h["n_rays"] == h["num_rays"] for h in hist)     # s = 1
    for a, b in zip(hist[:-1], hist[1:]):
        want = a["num_rays"] if a["skipped"] else trainer.next_num_rays(a["n_rays"], a["n_samples"], TARGET)
        assert b["num_rays"] == want, (a, b)
    assert [h["occ_refreshed"] for h in hist] == [h["step"] % 16 == 0 for h in hist]
    trained = [h for h in hist if not h["skipped"]]
    assert len(trained) > steps // 2 and all(np.isfinite(h["loss"]) for h in trained)
    assert np.mean([h["loss"] for h in trained[-20:]]) < np.mean([h["loss"] for h in trained[:20]])
    # which map every step drew from, and that the loop trained on exactly the sampler's batch of that (num_rays, step)
    assert [c[2] for c in calls] == ["isg"] * switch + ["ist"] * (steps + 1 - switch)
    assert [(c[0], c[1]) for c in calls] == [(h["num_rays"], h["step"]) for h in hist]
    # ISG throughout is the default, as the reference runs (train_real.py:301-309 has the switch commented out)
    isg_only = trainer.fit(views, None, sampling_weights=isg.reshape(-1), **dict(kw, max_steps=30))["history"]
    assert all(h["sampling"] == "isg" for h in isg_only)
    # weights on a 2x coarser grid: num_rays // 4 cells of 4 rays
    coarse = torch.nn.functional.avg_pool2d(isg.reshape(-1, 1, 40, 40), 2).reshape(-1)
    sub = trainer.fit(views, None, sampling_weights=coarse, weights_subsampled=2, **dict(kw, max_steps=20))["history"]
    assert all(h["n_rays"] == (h["num_rays"] // 4) * 4 for h in sub)


def test_fit_without_sampling_weights_is_the_uniform_loop(monkeypatch):
    """The uniform path is untouched: without sampling_weights fit trains on TrainViews.batch(num_rays, step, the preset's
    background and view mode, seed) and never calls the importance sampler.

    Two runs of the real loop cannot be compared value for value, on this commit or its parent: the training step adds
    gradients with float atomics, and the same call gave loss 0.02004328742623329 and 0.02004329115152359 at step 12 of
    two runs on one MI355X.  So the exact comparison replaces the step's arithmetic by a function of the batch alone
    (its loss and sample count then follow the batches bit for bit) and drives the parent's loop by hand beside fit."""
    views, _ = _blob_clip()
    kw = dict(FIT, max_steps=60)

    def step_of_the_batch(field, estimator, optimizer, origins, viewdirs, ts, pixels, render_step_size, **k):
        h = int(pixels.double().sum().item() * 255.0 + 0.5)
        return dict(n_samples=origins.shape[0] * (40 + h % 23), loss=float(pixels.mean()) + float(viewdirs[:, 0].sum()))

    monkeypatch.setattr(trainer, "train_step", step_of_the_batch)
    monkeypatch.setattr(views, "batch_importance", lambda *a, **k: pytest.fail("the uniform loop drew an importance batch"),
                        raising=False)
    a = trainer.fit(views, None, **kw)["history"]
    b = trainer.fit(views, None, sampling_weights=None, weights_subsampled=1, ist_weights=None, ist_from_step=None,
                    **kw)["history"]
    strip = lambda hist: [{k: v for k, v in h.items() if k != "seconds"} for h in hist]
    assert strip(a) == strip(b)
    assert set(a[0]) == {"step", "lr", "num_rays", "n_samples", "loss", "scale", "skipped", "occ_refreshed", "seconds"}
    # the parent's loop by hand: batch -> step -> next_num_rays
    num_rays = 1024
    for h in a:
        data = views.batch(num_rays, h["step"], bkgd="random", view_mode="one_per_step", seed=42)
        out = step_of_the_batch(None, None, None, data["rays"].origins, data["rays"].viewdirs, data["timestamps"],
                                data["pixels"], 5e-3)
        assert (h["num_rays"], h["n_samples"], h["loss"]) == (num_rays, out["n_samples"], out["loss"]), h
        num_rays = trainer.next_num_rays(num_rays, out["n_samples"], TARGET)
    assert len({h["num_rays"] for h in a}) > 10
    # and the real step on the uniform path: the loop's shape, as on the parent
    monkeypatch.undo()
    real = trainer.fit(views, None, **dict(kw, max_steps=20))["history"]
    assert [h["step"] for h in real] == list(range(21)) and "sampling" not in real[0]
    for x, y in zip(real[:-1], real[1:]):
        want = x["num_rays"] if x["skipped"] else trainer.next_num_rays(x["num_rays"], x["n_samples"], TARGET)
        assert y["num_rays"] == want
