"""GPU suite: the marching kernels against the geometric float64 reference of tests/march64.py -- ced_traverse_grids
(march.hip) and the accelerated walk (ced_march_all), both on the helpers of csrc/march_accel.hpp, on the
cases and with the comparison of tests/test_march64_cpu.py.  The reference's own conditions (how much it decides) are
asserted there, on the CPU."""
import numpy as np
import pytest
import torch

import march64 as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def _traverse(c, limit=None, over_allocate=False, mask=None, rays=None, near=None):
    """nerfacc_api.traverse_grids on a case -> (t_starts, t_ends, packed_info, termination planes, samples) as numpy, the
    over-allocated layout compacted as its caller does (cednerf/utils.py:265-267)."""
    from ced_nerf_amd import nerfacc_api as A
    sl = slice(None) if rays is None else rays
    i_, s_, term = A.traverse_grids(T(c["o"][sl]), T(c["d"][sl]), T(c["binaries"]), T(c["aabbs"]),
                                    T(c["near"][sl] if near is None else near), T(c["far"][sl]), c["step"], c["cone_angle"],
                                    limit, over_allocate, None if mask is None else T(mask))
    return N(i_.vals[i_.is_left]), N(i_.vals[i_.is_right]), N(s_.packed_info), N(term), s_


def _scan(counts):
    counts = np.asarray(counts, np.int64)
    return np.stack([np.cumsum(counts) - counts, counts], -1)


@pytest.mark.parametrize("name", M.CASES)
def test_traverse_grids_is_the_geometric_march(name):
    """Unlimited; budgets 1 and 7, ray-packed and over-allocated; with a rays_mask (a masked ray: no samples, terminates
    at its near plane)."""
    c = M.case(name)
    ref = c["ref"]
    n = c["o"].shape[0]
    t0, t1, packed, term, _ = _traverse(c)
    tot, _ = M.check_march(ref, t0, t1, packed, term=term)
    print(f"{name}: {t0.shape[0]} samples; decided-occupied {tot[0]}, decided-empty {tot[1]}, undecided {tot[2]}")
    for limit in (1, 7):
        t0, t1, packed, term, _ = _traverse(c, limit)
        M.check_march(ref, t0, t1, packed, term=term, limit=limit)
        a0, a1, apacked, aterm, s_ = _traverse(c, limit, over_allocate=True)
        assert np.array_equal(apacked[:, 0], np.arange(n) * limit)
        assert np.array_equal(N(s_.ray_indices[s_.is_valid]), np.repeat(np.arange(n), apacked[:, 1]))
        M.check_march(ref, a0, a1, _scan(apacked[:, 1]), term=aterm, limit=limit)
    mask = np.random.default_rng(5).uniform(size=n) < 0.6
    mask[:9:2] = False
    t0, t1, packed, term, _ = _traverse(c, mask=mask)
    assert (packed[~mask, 1] == 0).all()
    assert np.array_equal(term[~mask].view(np.uint32), c["near"][~mask].view(np.uint32))
    assert np.array_equal(packed[:, 0], np.cumsum(packed[:, 1]) - packed[:, 1])
    M.check_march(M.subset(ref, np.flatnonzero(mask)), t0, t1, _scan(packed[mask, 1]), term=term[mask])


@pytest.mark.parametrize("name", M.SPECKLE_CASES)
def test_traverse_grids_kernel_and_its_host_twin_run_the_same_code(name):
    """ced_traverse_grids on the device (over-allocated, budget 7) against ced_host_march_frame's walk 3 -- the same
    function (traverse_ray, march_accel.hpp) compiled for the host -- on the same sorted events: counts, samples and the
    termination planes of all rays as bit patterns."""
    import ctypes
    from ced_nerf_amd import _lib, nerfacc_api as A
    c = M.case(name)
    limit = 7
    n = c["o"].shape[0]
    b8 = np.ascontiguousarray(c["binaries"]).astype(np.uint8)
    m, res = b8.shape[0], b8.shape[1]
    t_mins, t_maxs, hits = A.ray_aabb_intersect(T(c["o"]), T(c["d"]), T(c["aabbs"]))
    ts, ti = A.sort_intersections(t_mins, t_maxs)
    i_, s_, term = A.traverse_grids(T(c["o"]), T(c["d"]), T(c["binaries"]), T(c["aabbs"]), T(c["near"]), T(c["far"]), c["step"],
                                    c["cone_angle"], limit, True, None, ts, ti, hits)
    d_counts = N(s_.packed_info)[:, 1]
    d_valid = N(s_.is_valid).reshape(n, limit)
    vals = N(i_.vals).reshape(n, limit, 2)                   # (t_start, t_end) of every slot
    d_t0, d_t1 = vals[..., 0], vals[..., 1]
    assert (c["far"] == c["far"][0]).all()
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    o, d, aabbs, near = (np.ascontiguousarray(c[k], np.float32) for k in ("o", "d", "aabbs", "near"))
    h_ts = np.ascontiguousarray(N(ts), np.float32); h_ti = np.ascontiguousarray(N(ti), np.int64)
    h_hits = np.ascontiguousarray(N(hits).astype(np.uint8))
    counts = np.empty(n, np.int32); tt = np.zeros(n, np.float32)
    t0 = np.zeros((n, limit), np.float32); t1 = np.zeros((n, limit), np.float32)
    rc = _lib.lib().ced_host_march_frame(n, P(o), P(d), P(b8), m, res, P(aabbs), P(near), float(c["far"][0]), c["step"],
                                         c["cone_angle"], limit, P(h_ts), P(h_ti), P(h_hits), None, 0, 0, 3, P(counts), P(t0),
                                         P(t1), P(tt))
    assert rc == 0
    assert np.array_equal(counts.astype(np.int64), d_counts)
    keep = np.arange(limit)[None, :] < counts[:, None]
    assert np.array_equal(keep, d_valid)
    assert (counts < limit).any()            # rays that end below their budget: their planes are compared too
    assert np.array_equal(t0[keep].view(np.uint32), d_t0[keep].view(np.uint32))
    assert np.array_equal(t1[keep].view(np.uint32), d_t1[keep].view(np.uint32))
    assert np.array_equal(tt.view(np.uint32), N(term).view(np.uint32))


def _estimator(binaries, levels):
    from ced_nerf_amd.nerfacc_api import OccGridEstimator
    est = OccGridEstimator(M.ROI, int(binaries.shape[1]), levels).to(DEV)
    est.set_binaries(T(binaries))
    return est


def _march_kw(c):
    return dict(near_plane=0.0, far_plane=float(c["far"][0]), render_step_size=c["step"], cone_angle=c["cone_angle"],
                near_planes=T(c["near"]))


@pytest.mark.parametrize("name", M.CASES)
def test_estimator_march_is_the_geometric_march(name):
    """OccGridEstimator.march: ced_traverse_grids (fast=False) and the accelerated walk ced_march_all (fast=True) -- 1, 2
    and 4 levels, common and stratified near planes, resolutions 12, 16, 20 (not multiples of the 8-cell brick) and 128."""
    c = M.case(name)
    est = _estimator(c["binaries"], c["aabbs"].shape[0])
    assert np.array_equal(N(est.aabbs), c["aabbs"])
    o, d = T(c["o"]), T(c["d"])
    n = c["o"].shape[0]
    for fast in (False, True):
        t0, t1, ri, packed = est.march(o, d, fast=fast, **_march_kw(c))
        packed = N(packed)
        M.check_march(c["ref"], N(t0), N(t1), packed)
        assert np.array_equal(N(ri), np.repeat(np.arange(n), packed[:, 1]))


@pytest.mark.parametrize("name", ["speckle16_L1", "speckle20_L2", "speckle12_L4", "speckle16_L2_stratified", "dynerf128_L4"])
def test_one_pass_march_is_the_geometric_march(name):
    """march_onepass: with room for every sample the rays' ranges are disjoint, cover [0, total) and hold the geometric
    march; with too little room the reported total is still that of the exact march (itself checked against the
    reference here)."""
    c = M.case(name)
    est = _estimator(c["binaries"], c["aabbs"].shape[0])
    o, d = T(c["o"]), T(c["d"])
    kw = _march_kw(c)
    e0, e1, _, epacked = est.march(o, d, fast=False, **kw)
    epacked = N(epacked)
    M.check_march(c["ref"], N(e0), N(e1), epacked)
    exact = int(epacked[:, 1].sum())
    assert exact > 1000
    args = (o, d, 0.0, kw["far_plane"], c["step"], c["cone_angle"])
    t0, t1, packed, total = est.march_onepass(*args, exact + 37, near_planes=kw["near_planes"])
    t0, t1, packed = N(t0), N(t1), N(packed)
    assert int(total.item()) == exact
    first, count = packed[:, 0], packed[:, 1]
    order = np.argsort(first + (count == 0) * (1 << 40), kind="stable")
    nz = count[order] > 0
    f, k = first[order][nz], count[order][nz]
    assert f[0] == 0 and np.array_equal(f[1:], (f + k)[:-1]) and f[-1] + k[-1] == exact, "ranges overlap or leave gaps"
    idx = np.concatenate([np.arange(a, a + b) for a, b in zip(first, count)] + [np.zeros(0, np.int64)]).astype(np.int64)
    M.check_march(c["ref"], t0[idx], t1[idx], _scan(count))
    small = est.march_onepass(*args, exact // 3, near_planes=kw["near_planes"])
    assert int(small[3].item()) == exact


@pytest.mark.parametrize("name", ["speckle16_L1", "speckle20_L2", "speckle12_L4", "dynerf128_L4"])
def test_chained_budgets_concatenate_to_the_unlimited_march(name):
    """Limited traverse_grids calls, each resuming the rays that used their whole budget at the returned termination
    planes, give the unlimited call's samples bit for bit (the frame loop's use, cednerf/utils.py:301-306)."""
    c = M.case(name)

    def march(rays, near, limit):
        t0, t1, packed, term, _ = _traverse(c, limit, rays=rays, near=near)
        return t0, t1, packed[:, 1], term

    whole = _traverse(c)
    M.assert_chain_is_the_unlimited_march(*M.chain(march, c), whole[0], whole[1])


def test_time_slice_march_is_the_geometric_march_of_the_bins_union():
    """TimeSlicedOccGrid.at_time over times that cover two bins marches the OR of those bins' slices."""
    from ced_nerf_amd.nerfacc_api import TimeSlicedOccGrid
    c = M.case("speckle16_L2_stratified")
    slices = np.random.default_rng(21).uniform(size=(4, 2, 16, 16, 16)) < 0.15
    sliced = TimeSlicedOccGrid(M.ROI, 16, 2, n_bins=4, device=DEV)
    sliced.set_slices(T(slices))
    times = [0.3, 0.6]
    assert sliced.bin_range(times) == (1, 2)
    union = slices[1] | slices[2]
    assert not np.array_equal(union, slices[1]) and not np.array_equal(union, slices.any(0))
    ref = M.march_reference(c["o"], c["d"], union, c["aabbs"], c["near"], c["far"], c["step"], c["cone_angle"])
    per = M.reference_counts(ref).sum(0)
    assert per[0] > 1000 and per[2] <= 0.10 * per[0], per
    est = sliced.at_time(times)
    assert np.array_equal(N(est.aabbs), c["aabbs"])
    for fast in (False, True):
        t0, t1, _, packed = est.march(T(c["o"]), T(c["d"]), fast=fast, **_march_kw(c))
        M.check_march(ref, N(t0), N(t1), N(packed))
