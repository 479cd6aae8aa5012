"""CPU suite: the references of tests/occgrid_reference.py against pairwise brute force, the host twin of the
distance-field build (ced_host_build_occupancy_accel) against them at every shape and pattern the GPU suite builds on
the device (tests/test_gpu_occupancy_grid.py), and the oracle's occupancy-grid update on index lists with repeats."""
import ctypes as C

import numpy as np
import pytest

import occgrid_reference as R
from conftest import assert_bitexact


def P(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def hip():
    from ced_nerf_amd import _lib
    return _lib.lib()


def training_draw(rng, cells, occupied_fraction):
    """An index list shaped like OccGridEstimator._sample_uniform_and_occupied_cells: cells // 4 draws with replacement,
    then the occupied cells, many of which the draw already holds."""
    occupied = np.flatnonzero(rng.uniform(size=cells) < occupied_fraction)
    return np.concatenate([rng.integers(0, cells, size=cells // 4), occupied]).astype(np.int64), occupied


@pytest.mark.parametrize("res", [21, 40])
def test_ema_reference_equals_the_definition_cell_by_cell(res):
    rng = np.random.default_rng(res)
    cells = res ** 3
    ids, occupied = training_draw(rng, cells, 0.05)
    assert len(np.unique(ids)) < len(ids) - 100                      # a list with many repeats
    occs = rng.uniform(0, 1, size=cells).astype(np.float32)
    occs[rng.integers(0, cells, size=cells // 50)] = -1.0           # invisible cells
    occs[occupied[:5]] = np.nan
    occ = rng.uniform(0, 1, size=len(ids)).astype(np.float32)
    occ[rng.integers(0, len(ids), size=len(ids) // 20)] = np.nan
    occ[-3:] = np.nan                                                # occupied[-3:] listed last; some get nothing but NaNs
    decay = np.float32(0.95)
    got = R.ema_update(occs, ids, occ, 0.95)
    order = np.argsort(ids, kind="stable")
    sid, socc = ids[order], occ[order]
    starts = np.flatnonzero(np.r_[True, sid[1:] != sid[:-1]])
    ends = np.r_[starts[1:], len(sid)]
    want = occs.copy()
    for s, e in zip(starts, ends):
        v = np.float32(occs[sid[s]] * decay)
        for j in range(s, e):                                        # C's fmaxf, one value at a time
            if np.isnan(v) or socc[j] > v:
                v = socc[j] if not np.isnan(socc[j]) else v
        want[sid[s]] = v
    assert_bitexact(got, want, "ema_update")
    untouched = np.ones(cells, bool); untouched[ids] = False
    assert untouched.any() and np.array_equal(got[untouched].view(np.uint32), occs[untouched].view(np.uint32))
    # every outcome of the index assignment is max(old * decay, occ_j) for one j: the contract is the largest of them
    dec = (occs * decay).astype(np.float32)
    one = np.fmax(dec[ids], occ)
    assert np.all(np.isnan(one) | (got[ids] >= one))


def test_ema_reference_smallest_cases():
    f = np.float32
    for old, pair, want in ((1.0, (0.3, 0.6), f(1.0) * f(0.95)), (0.5, (0.3, 0.6), f(0.6)), (0.1, (0.3, 0.6), f(0.6)),
                            (-1.0, (0.3, 0.6), f(0.6)), (-1.0, (0.0, 0.0), f(0.0)), (-1.0, (-2.0, -3.0), f(-1.0) * f(0.95)),
                            (0.5, (np.nan, 0.6), f(0.6)), (1.0, (np.nan, 0.6), f(1.0) * f(0.95)), (0.5, (-0.0, 0.0), f(0.475))):
        for a, b in (pair, pair[::-1]):
            occs = np.array([7.0, old, 3.0], f)
            new = R.ema_update(occs, [1, 1], np.array([a, b], f), 0.95)
            assert new[1].view(np.uint32) == f(want).view(np.uint32) and new[0] == 7.0 and new[2] == 3.0, (old, a, b, new)
    zero = R.ema_update(np.array([-0.0], f), [0, 0], np.array([-0.0, 0.0], f), 0.95)
    assert zero.view(np.uint32)[0] == 0                               # +0 beats -0 in either order
    zero = R.ema_update(np.array([-0.0], f), [0, 0], np.array([0.0, -0.0], f), 0.95)
    assert zero.view(np.uint32)[0] == 0
    assert np.isnan(R.ema_update(np.array([np.nan], f), [0], np.array([np.nan], f), 0.95)[0])
    assert R.ema_update(np.array([np.nan], f), [0, 0], np.array([np.nan, -4.0], f), 0.95)[0] == -4.0
    same = np.array([1.0, 2.0], f)
    assert np.array_equal(R.ema_update(same, np.zeros(0, np.int64), np.zeros(0, f), 0.95), same)


@pytest.mark.parametrize("res", [21, 40])
def test_distance_reference_equals_pairwise_brute_force(res):
    rng = np.random.default_rng(7 + res)
    b = np.zeros((3, res, res, res), np.uint8)
    b[0] = rng.uniform(size=b[0].shape) < 0.002
    b[1, res - 1, 0, res // 2] = 1                                   # one cell: the bounding-box shortcut of the reference
    b[2, :3, 5:9, res - 2:] = 1                                      # a block that straddles bricks
    bdist, cdist = R.chebyshev_fields(b)
    bricks = R.brick_occupancy(b)
    for lvl in range(3):
        assert np.array_equal(cdist[lvl], np.minimum(R.brute_force_distance(b[lvl]), R.CAP + 1))
        assert np.array_equal(bdist[lvl], np.minimum(R.brute_force_distance(bricks[lvl]), R.CAP + 1))
    assert cdist.max() == R.CAP + 1 and cdist.min() == 0 and bdist.min() == 0
    # the brick array by hand: a cell belongs to brick (x // 8, y // 8, z // 8)
    want = np.zeros_like(bricks)
    for lvl, x, y, z in np.argwhere(b):
        want[lvl, x // 8, y // 8, z // 8] = True
    assert np.array_equal(bricks, want)
    empty_b, empty_c = R.chebyshev_fields(np.zeros((1, res, res, res), np.uint8))
    assert (empty_b == R.CAP + 1).all() and (empty_c == R.CAP + 1).all()


def host_build(hip, binaries):
    m, res = binaries.shape[0], binaries.shape[1]
    accel = np.zeros((int(hip.ced_occupancy_accel_bytes(m, res)),), np.uint8)
    assert hip.ced_host_build_occupancy_accel(P(np.ascontiguousarray(binaries)), m, res, P(accel)) == 0
    return accel


@pytest.mark.parametrize("m,res,pattern", R.cases(), ids=["%dx%d-%s" % c for c in R.cases()])
def test_host_twin_builds_the_reference_fields(hip, m, res, pattern):
    """What the GPU suite compares the device build with, byte for byte, is itself the definition."""
    b = R.make_pattern(m, res, pattern)
    assert np.array_equal(b, R.make_pattern(m, res, pattern))
    if pattern not in ("empty", "full"):
        assert b.any() and (res == 1 or not b.all())
    bdist, cdist = R.accel_regions(host_build(hip, b), m, res)
    R.check_fields(bdist, cdist, b, pattern)


def test_patterns_are_what_they_are_named():
    for m, res in R.SHAPES:
        nb = -(-res // 8)
        lb = R.make_pattern(m, res, "last_brick")
        for lvl in range(m):
            pts = np.argwhere(lb[lvl])
            assert len(pts) > 0 and all((p >= (nb - 1) * 8).any() for p in pts)
            assert all(((pts[:, ax] >= (nb - 1) * 8)).any() for ax in range(3))
        if m >= 3:
            el = R.make_pattern(m, res, "empty_level")
            assert not el[1].any() and el[0].any() and el[2].any()
        cells = {R.single_cell(res, n) for n in R.SINGLE_CELLS}
        assert len(cells) == (9 if res >= 3 else (8 if res == 2 else 1))
        for n in R.SINGLE_CELLS:
            assert R.make_pattern(m, res, n).sum() == m
    assert len(R.cases()) == len(R.SHAPES) * (len(R.PATTERNS) - 1) + 2


def test_ema_update_entry_reports_argument_errors(hip):
    """ced_occ_ema_update takes a workspace of n floats; every refusal comes back as a code and a message before anything
    is launched."""
    buf = np.zeros(64, np.uint8)
    ptr = P(buf)
    assert hip.ced_occ_ema_update(0, None, None, 1.0, 0.95, None, None, 0, None) == 0                   # empty list
    assert hip.ced_occ_ema_update(-1, ptr, ptr, 1.0, 0.95, ptr, ptr, 64, None) == -1
    assert hip.ced_occ_ema_update(4, None, ptr, 1.0, 0.95, ptr, ptr, 64, None) == -1 and b"null pointer" in hip.ced_last_error_string()
    assert hip.ced_occ_ema_update(4, ptr, ptr, 1.0, 0.95, ptr, None, 64, None) == -1 and b"workspace" in hip.ced_last_error_string()
    assert hip.ced_occ_ema_update(4, ptr, ptr, 1.0, 0.95, ptr, ptr, 15, None) == -1 and b"workspace" in hip.ced_last_error_string()


def test_oracle_update_with_repeated_cells_is_the_order_independent_one(oracle):
    """oracle.occ_grid_update on the draw training makes: every listed cell decays once and takes the largest of its
    samples, whatever the order of the list."""
    rng = np.random.default_rng(11)
    res, levels = 12, 2
    cells = res ** 3
    occs = rng.uniform(0, 1, size=levels * cells).astype(np.float32)
    occs[rng.integers(0, levels * cells, size=40)] = -1.0
    aabbs = oracle.make_aabbs([-1, -1, -1, 1, 1, 1], levels)
    idx = [training_draw(rng, cells, 0.05)[0] for _ in range(levels)]
    assert all(len(np.unique(i)) < len(i) for i in idx)
    noise = [rng.uniform(0, 1, size=(len(i), 3)).astype(np.float32) for i in idx]
    vals = [rng.uniform(0, 1, size=len(i)).astype(np.float32) for i in idx]
    want = occs
    for lvl in range(levels):
        want = R.ema_update(want, lvl * cells + idx[lvl], vals[lvl], 0.95)
    for order in ([np.arange(len(i)) for i in idx], [np.arange(len(i))[::-1] for i in idx], [rng.permutation(len(i)) for i in idx]):
        got, binaries = oracle.occ_grid_update(occs, aabbs, res, [i[o] for i, o in zip(idx, order)],
                                               [n[o] for n, o in zip(noise, order)],
                                               (lambda it: lambda x: next(it))(iter([v[o] for v, o in zip(vals, order)])),
                                               occ_thre=0.01, ema_decay=0.95)
        assert_bitexact(got, want, "oracle occs")
        thre = min(np.float32(want[want >= 0].astype(np.float64).mean()), np.float32(0.01))
        assert np.array_equal(binaries, want > thre)
