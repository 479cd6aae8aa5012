"""CPU suite: DyNeRF's importance sampling (ced_nerf_amd/importance.py, trainset.importance_draws) -- the explicit float32
logarithm, the numpy restatement of the sampler as a multinomial without replacement, the weight formulas on a hand-made
clip, and the argument errors of the Python and C interfaces.

The reference's dynerf_isg_weight / dynerf_ist_weight_nice are not recorded as a fixture: their module
(datasets/dnerf_3d_video_IS.py) imports imageio (imageio.v2), which the build machine does not have, so the formulas are
checked against known answers worked out by hand below and the GPU suite compares the kernels with the restatements."""
import ctypes as C

import numpy as np
import pytest
import torch

from ced_nerf_amd import importance, trainset
from ced_nerf_amd.trainset import TrainViews


# ---------------------------------------------------------------------------------------------------------------------
# det_logf
# ---------------------------------------------------------------------------------------------------------------------
def test_det_logf_over_every_unit_value():
    """All 2^23 values unit = odd * 2^-24 the sampler can form: e = -det_logf(unit) within 1e-5 (relative) of float64's
    -log.  (Measured: 8.1e-8, at unit = 0.35352546.)"""
    odd = np.arange(1 << 23, dtype=np.uint32) * np.uint32(2) + np.uint32(1)
    unit = odd.astype(np.float32) * np.float32(2.0 ** -24)
    assert unit.min() > 0.0 and unit.max() < 1.0
    e = -trainset.det_logf_np(unit)
    assert e.dtype == np.float32 and e.min() > 0.0 and np.isfinite(e).all()
    want = -np.log(unit.astype(np.float64))
    rel = np.abs(e.astype(np.float64) - want) / want
    print(f"det_logf: max relative error of e {rel.max():.3e} at unit {unit[rel.argmax()]!r}")
    assert rel.max() <= 1e-5
    # the draw's own mapping produces exactly these values
    u = np.array([0, 1 << 9, 0xFFFFFFFF], np.uint32)
    assert np.array_equal(trainset.draw_exponential(u), e[[0, 1, -1]])


# ---------------------------------------------------------------------------------------------------------------------
# The restatement is a multinomial without replacement
# ---------------------------------------------------------------------------------------------------------------------
R = 20000


def _small_map():
    rng = np.random.default_rng(0)
    w = np.concatenate([np.zeros(8), 10.0 ** rng.uniform(-3.0, 0.0, 56)]).astype(np.float32)
    rng.shuffle(w)
    return w                                              # 64 cells = one 8 x 8 view, zeros and three decades


def _cells(view, x, y, width, height):
    return (view.astype(np.int64) * height + y) * width + x


def _torch_frequencies(w, k, seed):
    g = torch.Generator().manual_seed(seed)
    wt = torch.from_numpy(w)
    counts = np.zeros(w.shape[0])
    for _ in range(R):
        counts[torch.multinomial(wt, k, replacement=False, generator=g).numpy()] += 1
    return counts / R


def _within_bound(p1, p2):
    p = 0.5 * (p1 + p2)
    bound = 5.0 * np.sqrt(2.0 * p * (1.0 - p) / R)
    return bool(np.all(np.abs(p1 - p2) <= bound)), float(np.max(np.abs(p1 - p2) - bound))


def test_importance_draws_have_torch_multinomials_inclusion_frequencies():
    w = _small_map()
    counts = np.zeros(64)
    for step in range(R):
        view, x, y = trainset.importance_draws(7, step, 8, w, 1, 2_000_000, 8, 8)
        cells = _cells(view, x, y, 8, 8)
        assert len(np.unique(cells)) == 8                 # without replacement
        counts[cells] += 1
    ours = counts / R
    assert ours[w == 0].sum() == 0                        # zero-weight cells are never drawn
    a, b = _torch_frequencies(w, 8, 1), _torch_frequencies(w, 8, 2)
    ok, margin = _within_bound(a, b)                      # the yardstick passes its own test
    assert ok, margin
    for other in (a, b):
        ok, margin = _within_bound(ours, other)
        print(f"importance_draws vs torch.multinomial: worst |difference| - bound = {margin:.3e}")
        assert ok, margin


def test_exactly_k_positive_cells_are_all_drawn_and_fewer_is_an_error():
    w = np.zeros(3 * 4 * 5, np.float32)
    positive = np.array([2, 17, 18, 40, 59])
    w[positive] = [1e-3, 5.0, 0.25, 1.0, 3e2]
    for step in range(20):
        view, x, y = trainset.importance_draws(1, step, 5, w, 1, 2_000_000, 5, 4)
        assert np.array_equal(_cells(view, x, y, 5, 4), positive)         # ascending candidate order
    with pytest.raises(ValueError, match="positive"):
        trainset.importance_draws(1, 0, 6, w, 1, 2_000_000, 5, 4)
    w[3] = np.nan
    w[4] = np.inf
    w[5] = -1.0
    with pytest.raises(ValueError, match="positive"):                     # not numbers one can draw by
        trainset.importance_draws(1, 0, 6, w, 1, 2_000_000, 5, 4)


def test_pooled_path_draws_only_from_its_pool_and_keeps_duplicates():
    rng = np.random.default_rng(3)
    width, height, views = 6, 5, 4
    w = rng.random(views * height * width).astype(np.float32)
    n = w.shape[0]
    seen_duplicate = False
    for step in range(40):
        cell, bits = trainset.importance_candidates(9, step, w, pool_size=32)
        assert cell.shape == (32,) and cell.min() >= 0 and cell.max() < n
        assert np.array_equal(cell, trainset.draw_below(trainset.batch_draw(trainset.batch_key(9, step),
                                                                            np.arange(32, dtype=np.uint64), 3), n))
        view, x, y = trainset.importance_draws(9, step, 30, w, 1, 32, width, height)
        drawn = _cells(view, x, y, width, height)
        pool = np.bincount(cell, minlength=n)
        assert np.all(np.bincount(drawn, minlength=n) <= pool)            # only pool cells, each at most as often
        seen_duplicate |= len(np.unique(drawn)) < len(drawn)
    assert seen_duplicate                                                 # a cell that entered the pool twice


def test_subsampled_cells_expand_in_the_references_order():
    s, width, height, views = 2, 7, 5, 3                                  # 3 x 2 cells per view; column 6, row 4 unused
    hsub, wsub = height // s, width // s
    w = np.arange(1, views * hsub * wsub + 1, dtype=np.float32)
    view, x, y = trainset.importance_draws(0, 0, 4 * 5 + 3, w, s, 2_000_000, width, height)
    k = 5
    assert view.shape == x.shape == y.shape == (k * s * s,)
    for a, (ah, aw) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):       # torch.cat order: ah outer, aw inner
        part = slice(a * k, (a + 1) * k)
        assert np.array_equal(view[part], view[:k])
        assert np.array_equal(x[part], x[:k] + aw) and np.array_equal(y[part], y[:k] + ah)
    assert np.all(x[:k] % s == 0) and np.all(y[:k] % s == 0) and x.max() < wsub * s and y.max() < hsub * s
    cells = (view[:k] * hsub + y[:k] // s) * wsub + x[:k] // s
    assert np.all(np.diff(cells) > 0)                                     # ascending candidate = cell order here


def test_selection_takes_ties_at_the_threshold_from_the_lower_candidates():
    """trainset.select_largest, the selection importance_draws makes: the threshold pattern 9 occurs three times and two
    places are left for it, which the two lower candidates get."""
    bits = np.array([5, 9, 12, 9, 0, 9, 7], np.uint32)
    assert np.array_equal(trainset.select_largest(bits, 3), [1, 2, 3])
    assert np.array_equal(trainset.select_largest(bits, 1), [2])
    assert np.array_equal(trainset.select_largest(bits, 6), [0, 1, 2, 3, 5, 6])
    with pytest.raises(ValueError, match="positive"):
        trainset.select_largest(bits, 7)
    # through importance_draws: weights whose keys overflow to +inf in bulk tie at the threshold
    w = np.full(200, 3.0e38, np.float32)
    cell, keys = trainset.importance_candidates(5, 1, w)
    tied = np.flatnonzero(keys == 0x7F800000)
    assert len(tied) > 40
    view, x, y = trainset.importance_draws(5, 1, 20, w, 1, 2_000_000, 20, 10)
    assert np.array_equal((view * 10 + y) * 20 + x, tied[:20])


# ---------------------------------------------------------------------------------------------------------------------
# The weight formulas on a hand-made clip [2 cameras, 5 frames, 4, 6, 3]
# ---------------------------------------------------------------------------------------------------------------------
def _clip():
    clip = np.full((2, 5, 4, 6, 3), 100, np.uint8)
    clip[0, :, 0, 0, 0] = [10, 50, 20, 40, 30]            # odd T: median 30
    clip[0, :, 0, 1] = [[0, 0, 0], [0, 0, 0], [0, 0, 0], [255, 255, 255], [255, 255, 255]]
    clip[1, :, 2, 3, 1] = [100, 100, 100, 100, 160]
    return clip


def test_temporal_median_reference_known_answers():
    clip = _clip()
    med = importance.temporal_median_reference(clip.reshape(10, 4, 6, 3), 2)
    assert med.shape == (2, 4, 6, 3) and med.dtype == np.uint8
    assert med[0, 0, 0, 0] == 30 and med[0, 0, 1, 0] == 0 and med[1, 2, 3, 1] == 100 and med[1, 1, 1, 2] == 100
    even = clip[:, :4]                                    # even T: the lower of the two middle values, as torch.median
    med4 = importance.temporal_median_reference(even.reshape(8, 4, 6, 3), 2)
    assert med4[0, 0, 0, 0] == 20                         # of 10, 20, 40, 50
    assert med4[0, 0, 0, 0] == int(torch.median(torch.from_numpy(even[0, :, 0, 0, 0].astype(np.int64))))
    want = torch.median(torch.from_numpy(even.astype(np.int16)), dim=1).values.numpy().astype(np.uint8)
    assert np.array_equal(med4, want)
    one = importance.temporal_median_reference(clip[:, 0], 2)             # T = 1: the frame itself
    assert np.array_equal(one, clip[:, 0])


def test_isg_reference_known_answers():
    clip = _clip()
    isg = importance.isg_weights_reference(clip.reshape(10, 4, 6, 3), 2, gamma=2e-2)
    assert isg.shape == (2, 5, 4, 6) and isg.dtype == np.float32
    assert np.all(isg[1, :, 1, 1] == 0.0) and np.all(isg[0, :, 3, 5] == 0.0)      # static pixels
    assert isg[0, 4, 0, 0] == 0.0                                                 # the median frame itself
    f32 = np.float32
    d = f32(10) / f32(255) - f32(30) / f32(255)
    q = d * d
    p = q / (q + f32(2e-2) * f32(2e-2))
    assert isg[0, 0, 0, 0] == ((p + f32(0)) + f32(0)) * f32(1.0 / 3.0)
    assert 0.0 < isg[0, 0, 0, 0] < 1.0 / 3.0
    d = f32(255) / f32(255) - f32(0)
    p = (d * d) / (d * d + f32(2e-2) * f32(2e-2))
    assert isg[0, 3, 0, 1] == ((p + p) + p) * f32(1.0 / 3.0) and isg[0, 3, 0, 1] > 0.999
    assert isg[1, 4, 2, 3] > 0.0 and np.all(isg[1, :4, 2, 3] == 0.0)
    given = importance.isg_weights_reference(clip.reshape(10, 4, 6, 3), 2, 2e-2,
                                             median=importance.temporal_median_reference(clip.reshape(10, 4, 6, 3), 2))
    assert np.array_equal(isg, given)


def test_ist_reference_known_answers_and_the_end_of_clip_quirk():
    clip = _clip()
    f32 = np.float32
    ist = importance.ist_weights_reference(clip.reshape(10, 4, 6, 3), 2, alpha=0.1, frame_shift=1)
    assert ist.shape == (2, 5, 4, 6) and ist.dtype == np.float32
    # away from the clip's ends a static pixel has weight alpha; at the ends its neighbour is a zero frame: |0 - 100|
    assert np.all(ist[1, 1:4, 1, 1] == f32(0.1))
    assert ist[1, 0, 1, 1] == f32(100.0) and ist[1, 4, 1, 1] == f32(100.0)
    # 10 50 20 40 30 in the red channel, 100 elsewhere: t = 1 sees |10 - 50| and |20 - 50|
    assert ist[0, 1, 0, 0] == (f32(40.0) + f32(0.0) + f32(0.0)) / f32(3.0)
    assert ist[0, 0, 0, 0] == (f32(40.0) + f32(100.0) + f32(100.0)) / f32(3.0)   # end: max(|50-10|, |0-10|), 100, 100
    # the step 0 -> 255 between t = 2 and t = 3
    assert ist[0, 2, 0, 1] == f32(255.0) and ist[0, 3, 0, 1] == f32(255.0) and ist[0, 1, 0, 1] == f32(0.1)
    # a larger shift than the clip is long: every frame has a zero neighbour
    wide = importance.ist_weights_reference(clip.reshape(10, 4, 6, 3), 2, alpha=0.1, frame_shift=25)
    assert np.all(wide[1, :, 1, 1] == f32(100.0)) and wide[0, 4, 0, 1] == f32(255.0)
    none = importance.ist_weights_reference(clip.reshape(10, 4, 6, 3), 2, alpha=0.5, frame_shift=0)
    assert np.all(none == f32(0.5))


# ---------------------------------------------------------------------------------------------------------------------
# Argument errors
# ---------------------------------------------------------------------------------------------------------------------
def _cpu_views(V=6, H=4, W=6, channels=3):
    imgs = np.zeros((V, H, W, channels), np.uint8)
    K = np.array([[5.0, 0, 3.0], [0, 5.0, 2.0], [0, 0, 1]], np.float32)
    c2w = np.tile(np.eye(4, dtype=np.float32)[None, :3], (V, 1, 1))
    return TrainViews.pinhole(imgs, K, c2w, np.linspace(0, 1, V), opengl=False, device="cpu", view_mode="one_per_step")


def test_weight_map_argument_errors():
    views = _cpu_views()
    for fn in (importance.temporal_median, importance.isg_weights, importance.ist_weights):
        with pytest.raises(ValueError, match="cameras"):
            fn(views, 4)                                  # 6 views are not frames of 4 cameras
        with pytest.raises(ValueError, match="cameras"):
            fn(views, 0)
        with pytest.raises(ValueError, match="RGBA"):
            fn(_cpu_views(channels=4), 2)
    with pytest.raises(ValueError, match="cameras"):
        importance.temporal_median_reference(np.zeros((6, 4, 6, 3), np.uint8), 4)
    with pytest.raises(ValueError, match="uint8"):
        importance.isg_weights_reference(np.zeros((6, 4, 6, 4), np.uint8), 2)


def test_batch_importance_argument_errors():
    views = _cpu_views()
    n = 6 * 4 * 6
    w = torch.ones(n)
    with pytest.raises(ValueError, match="RGBA"):
        _cpu_views(channels=4).batch_importance(16, 0, w)
    with pytest.raises(ValueError, match="no cell"):
        views.batch_importance(3, 0, torch.ones(6 * 2 * 3), weights_subsampled=2)       # k = 3 // 4 = 0
    with pytest.raises(ValueError, match="no cell"):
        views.batch_importance(0, 0, w)
    with pytest.raises(ValueError, match="weights must be"):
        views.batch_importance(16, 0, torch.ones(n - 1))
    with pytest.raises(ValueError, match="weights must be"):
        views.batch_importance(16, 0, torch.ones(n, dtype=torch.float64))
    with pytest.raises(ValueError, match="weights must be"):
        views.batch_importance(16, 0, w, weights_subsampled=2)                          # the map of s = 1
    with pytest.raises(ValueError, match="weights_subsampled"):
        views.batch_importance(16, 0, w, weights_subsampled=0)
    with pytest.raises(ValueError, match="weights_subsampled"):
        views.batch_importance(16, 0, w, weights_subsampled=5)
    with pytest.raises(ValueError, match="bkgd"):
        views.batch_importance(16, 0, w, bkgd="grey")
    with pytest.raises(ValueError, match="pool_size"):
        views.batch_importance(16, 0, w, pool_size=0)
    with pytest.raises(ValueError, match="pool_size"):
        views.batch_importance(16, 0, w, pool_size=1 << 31)
    with pytest.raises(ValueError, match="without replacement"):
        views.batch_importance(n + 1, 0, w)
    with pytest.raises(ValueError, match="without replacement"):
        views.batch_importance(33, 0, w, pool_size=32)
    big = TrainViews.__new__(TrainViews)                  # 2^31 cells: rejected from the sizes alone
    big.n_views, big.height, big.width, big.channels = 1 << 11, 1 << 10, 1 << 10, 3
    with pytest.raises(ValueError, match="2\\^31"):
        big.batch_importance(16, 0, w)
    with pytest.raises(ValueError, match="2\\^31"):
        trainset.importance_candidates(0, 0, np.zeros(4, np.float32), pool_size=1 << 31)
    with pytest.raises(ValueError):
        trainset.importance_draws(0, 0, 3, np.ones(6, np.float32), 2, 100, 6, 4)
    with pytest.raises(ValueError, match="whole views"):
        trainset.importance_draws(0, 0, 4, np.ones(7, np.float32), 1, 100, 3, 2)


def test_fit_rejects_an_ist_switch_without_sampling_weights():
    from ced_nerf_amd import trainer
    views = _cpu_views()
    with pytest.raises(ValueError, match="sampling_weights"):
        trainer.fit(views, ist_from_step=10)
    with pytest.raises(ValueError, match="sampling_weights"):
        trainer.fit(views, ist_weights=torch.ones(4))
    with pytest.raises(ValueError, match="go together"):
        trainer.fit(views, sampling_weights=torch.ones(4), ist_from_step=10)


def test_c_abi_argument_checks_return_a_status():
    from ced_nerf_amd import _lib
    L = _lib.lib()
    for name in ("ced_temporal_median_u8", "ced_isg_weights", "ced_ist_weights", "ced_sample_importance_batch",
                 "ced_importance_batch_workspace_bytes"):
        assert name in _lib.header_symbols() and name in _lib.PROTOTYPES
    one = C.c_void_p(16)                                  # a non-null pointer that no failing call may touch
    assert L.ced_temporal_median_u8(0, 5, 4, 6, one, one, None) == -1 and b"temporal_median_u8" in L.ced_last_error_string()
    assert L.ced_temporal_median_u8(2, 5, 4, 6, None, one, None) == -1 and b"null pointer" in L.ced_last_error_string()
    assert L.ced_temporal_median_u8(1 << 20, 1 << 20, 1 << 10, 1 << 10, one, one, None) == -1
    assert L.ced_isg_weights(2, 5, 4, -6, one, one, 2e-2, one, None) == -1
    assert L.ced_isg_weights(2, 5, 4, 6, one, None, 2e-2, one, None) == -1 and b"null pointer" in L.ced_last_error_string()
    assert L.ced_isg_weights(2, 5, 4, 6, one, one, float("nan"), one, None) == -1
    assert L.ced_ist_weights(2, 5, 4, 6, one, 0.1, -1, one, None) == -1 and b"frame_shift" in L.ced_last_error_string()
    assert L.ced_ist_weights(2, 5, 4, 6, one, 0.1, 25, None, None) == -1
    # workspace sizes: header (3 x 2048 histogram words + 4) + keys + tile counts + selected cells, each 256-aligned
    assert L.ced_importance_batch_workspace_bytes(1000, 2_000_000, 10) == 24832 + 4096 + 256 + 256
    assert L.ced_importance_batch_workspace_bytes(5_000_000, 2_000_000, 65536) == 24832 + 8_000_000 + 15872 + 262144
    assert L.ced_importance_batch_workspace_bytes(1 << 31, 2_000_000, 10) == -1
    assert L.ced_importance_batch_workspace_bytes(1000, 2_000_000, 1001) == -1          # more cells than candidates
    assert L.ced_importance_batch_workspace_bytes(1000, 0, 1) == -1
    assert L.ced_importance_batch_workspace_bytes(1000, 10, 0) == -1

    def sample(model=0, n_views=6, width=6, height=4, channels=3, images=one, weights=one, s=1, pool=2_000_000, k=16,
               bkgd=2, workspace=one, ws_bytes=1 << 20, min_key=one):
        return L.ced_sample_importance_batch(model, n_views, width, height, channels, images, one, one, weights, s, pool,
                                             k, 0, 0, bkgd, one, one, one, one, one, None, min_key, workspace, ws_bytes, None)

    assert sample(model=7) == -1 and b"camera model" in L.ced_last_error_string()
    assert sample(channels=4) == -1 and b"RGB" in L.ced_last_error_string()
    assert sample(s=0) == -1 and sample(s=5) == -1
    assert sample(k=0) == -1 and sample(k=6 * 4 * 6 + 1) == -1 and sample(k=33, pool=32) == -1
    assert sample(bkgd=3) == -1
    assert sample(n_views=1 << 30, width=1 << 10, height=1 << 10) == -1                 # 2^50 cells
    assert sample(weights=None) == -1 and b"null pointer" in L.ced_last_error_string()
    assert sample(workspace=None) == -1 and sample(min_key=None) == -1
    assert sample(workspace=C.c_void_p(24)) == -1 and b"aligned" in L.ced_last_error_string()
    assert sample(ws_bytes=1024) == -1 and b"too small" in L.ced_last_error_string()
