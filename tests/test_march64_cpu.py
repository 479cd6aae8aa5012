"""CPU suite: the march against the geometric float64 reference of tests/march64.py -- the reference alone, the C oracle
(oracle/cednerf_oracle.c restates the DDA of csrc/march_accel.hpp, so the bit-exact suites cannot see a mistake the two
share) and the host twin of the accelerated walk (csrc/march_accel.hpp through ced_host_march_frame)."""
import ctypes as C

import numpy as np
import pytest

import march64 as M


def P(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def hip():
    from ced_nerf_amd import _lib
    return _lib.lib()


def _oracle_march(oracle, c, limit=0, binaries=None, near=None):
    return oracle.traverse_grids(c["o"], c["d"], c["binaries"] if binaries is None else binaries, c["aabbs"],
                                 c["near"] if near is None else near, c["far"], c["step"], c["cone_angle"], limit)


# ---- the reference alone ----------------------------------------------------------------------------------------------
def test_reference_decides_enough_in_every_case():
    """Conditions on the reference, before anything is compared with it: per case the undecided midpoints are at most
    10 % of the decided-occupied ones, and every named edge ray but the miss has >= 8 decided-occupied and >= 8
    decided-empty in-box midpoints in some case.  The ray along a box edge is exempt: it lies in cell-face planes of every
    level (and on the finest box's edge), the reference cannot decide it, and what is asserted of it is that it produces
    lattice intervals only (check 1 of check_march, in every comparison below)."""
    best = np.zeros((9, 2), np.int64)
    for name in M.CASES:
        ref = M.case(name)["ref"]
        per = M.reference_counts(ref)
        occ, emp, und = per.sum(0)
        n_mid = sum(x.shape[0] for x in ref["occupied"])
        print(f"{name}: {n_mid} midpoints, decided-occupied {occ}, decided-empty in box {emp}, undecided {und} "
              f"({100.0 * und / max(occ, 1):.2f} % of decided-occupied), rho <= {ref['rho'].max():.2e}")
        assert und <= 0.10 * occ, (name, und, occ)
        named = range(9) if name.startswith("block") else range(8)
        for i in named:
            if per[i, :2].min() > best[i].min():            # the case in which the ray has most of the scarcer kind
                best[i] = per[i, :2]
    for i in range(9):
        print(f"ray {i} ({M.NAMED[i]}): best case has {best[i, 0]} decided-occupied, {best[i, 1]} decided-empty midpoints")
        if i not in (M.MISS, M.ALONG_EDGE):
            assert best[i].min() >= 8, (M.NAMED[i], best[i])
    miss = M.case("speckle12_L4")["ref"]
    assert miss["lattice"][M.MISS].shape[0] == 2 and not miss["occupied"][M.MISS].any()
    # the rays in a box's face plane are decided where they are outside that box: before the finest box (on one level:
    # outside every box), and in the coarser levels behind the level-1 box
    for name, i in (("speckle16_L1", M.IN_FINE_FACE_PLANE), ("block16_L2", M.IN_FINE_FACE_PLANE),
                    ("speckle24_L3", M.IN_COARSE_FACE_PLANE), ("dynerf128_L4", M.IN_COARSE_FACE_PLANE)):
        ref = M.case(name)["ref"]
        away = ref["decided"][i] & ((ref["mid"][i] < 2.9) if i == M.IN_FINE_FACE_PLANE else (ref["mid"][i] > 6.4))
        print(f"ray {i} ({M.NAMED[i]}) in {name}: {away.sum()} decided midpoints outside the box whose face plane it lies in, "
              f"{(away & ref['occupied'][i]).sum()} of them occupied")
        assert away.sum() >= 8
    # the ray that hugs the cell face z = 0 is decided where the cells on both sides agree
    per = M.reference_counts(M.case("speckle16_L1")["ref"])[M.HUGS_CELL_FACE]
    print(f"ray {M.HUGS_CELL_FACE} ({M.NAMED[M.HUGS_CELL_FACE]}) in speckle16_L1: {per[0]} decided-occupied, {per[1]} decided-empty midpoints")
    assert per[0] >= 8 and per[1] >= 8
    # the box interval that the lattice steps over: no midpoint in it, and it is not empty
    ref = M.case("speckle20_L2")["ref"]
    i = M.SHORT_INTERVAL
    assert not ref["in_box"][i].any() and 3.49 < ref["stop_lo"][i] < ref["stop_hi"][i] < 3.51


def test_reference_known_answer_2x2x2():
    """2x2x2 grid on [-1, 1]^3, only cell (1, 0, 0) occupied, step 0.25, ray from (-2, -0.5, -0.5) along
    +x: samples start at [2, 2.25, 2.5, 2.75], the ray terminates at 3."""
    b = np.zeros((1, 2, 2, 2), bool); b[0, 1, 0, 0] = True
    ref = M.march_reference([[-2.0, -0.5, -0.5]], [[1.0, 0.0, 0.0]], b, M.make_aabbs(M.ROI, 1), 0.0, 1e10, 0.25, 0.0)
    t = ref["lattice"][0]
    assert ref["decided"][0].all()
    assert t[:-1][ref["occupied"][0]].tolist() == [2.0, 2.25, 2.5, 2.75]
    assert t[:-1][ref["in_box"][0]].tolist() == [1.0 + 0.25 * k for k in range(8)]
    want = np.array([2.0, 2.25, 2.5, 2.75, 3.0], np.float32)
    M.check_march(ref, want[:-1], want[1:], [[0, 4]], term=[3.0])
    for wrong_term in (2.75, 3.25):
        with pytest.raises(AssertionError):
            M.check_march(ref, want[:-1], want[1:], [[0, 4]], term=[wrong_term])
    with pytest.raises(AssertionError):                     # a sample short
        M.check_march(ref, want[:3], want[1:4], [[0, 3]])
    with pytest.raises(AssertionError):                     # off the lattice by an ulp
        M.check_march(ref, want[:-1], np.nextafter(want[1:], np.float32(9)), [[0, 4]])


# ---- the C oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.CASES)
def test_oracle_march_is_the_geometric_march(oracle, name):
    c = M.case(name)
    for limit in (0, 1, 7):
        w = _oracle_march(oracle, c, limit)
        tot, _ = M.check_march(c["ref"], w["t_starts"], w["t_ends"], w["packed_info"], term=w["termination_planes"], limit=limit)
    print(f"{name}: {w['t_starts'].shape[0]} samples at limit 7; decided-occupied {tot[0]}, decided-empty {tot[1]}, undecided {tot[2]}")


# ---- the host twin of the accelerated walk ----------------------------------------------------------------------------
def _build_accel(hip, binaries):
    m, res = binaries.shape[0], binaries.shape[1]
    accel = np.zeros((int(hip.ced_occupancy_accel_bytes(m, res)),), np.uint8)
    assert hip.ced_host_build_occupancy_accel(P(binaries), m, res, P(accel)) == 0
    return accel


@pytest.mark.parametrize("name", M.SPECKLE_CASES)
def test_host_twin_is_the_geometric_march(hip, oracle, name):
    """ced_host_march_frame: accel_mode 0 / 1 / 2, walk 0 / 1, the lattice table where it applies (cone angle 0, one
    near plane).  Its termination plane is specified only for a ray that used its whole budget (march_accel.hpp) --
    except in walk 3 (accel_mode 0), where it is specified for every ray."""
    c = M.case(name)
    o, d, aabbs, near = c["o"], c["d"], c["aabbs"], c["near"]
    n = o.shape[0]
    b8 = np.ascontiguousarray(c["binaries"]).astype(np.uint8)
    m, res = b8.shape[0], b8.shape[1]
    tmin, tmax, hits = oracle.ray_aabb_intersect(o, d, aabbs)
    ts, ti = oracle.sort_intersections(tmin, tmax)
    ts = np.ascontiguousarray(ts, np.float32); ti = np.ascontiguousarray(ti, np.int64)
    hits8 = np.ascontiguousarray(hits.astype(np.uint8))
    accel = _build_accel(hip, b8)
    unlimited = int(_oracle_march(oracle, c)["packed_info"][:, 1].max()) + 1
    lattices = (0, 1) if (c["cone_angle"] == 0.0 and c["common_near"]) else (0,)
    runs = 0
    for limit in (1, 7, unlimited):
        for mode in (0, 1, 2):
            for start_coarse in (0, 1):
                for use_lattice in lattices:
                    counts = np.empty(n, np.int32); tt = np.zeros(n, np.float32)
                    t0 = np.zeros((n, limit), np.float32); t1 = np.zeros((n, limit), np.float32)
                    rc = hip.ced_host_march_frame(n, P(o), P(d), P(b8), m, res, P(aabbs), P(near), float(c["far"][0]),
                                                  c["step"], c["cone_angle"], limit, P(ts), P(ti), P(hits8), P(accel), mode,
                                                  use_lattice, start_coarse, P(counts), P(t0), P(t1), P(tt))
                    assert rc == 0
                    keep = np.arange(limit)[None, :] < counts[:, None]
                    cnt = counts.astype(np.int64)
                    term = np.where(cnt == limit, tt, np.float32(np.nan))
                    M.check_march(c["ref"], t0[keep], t1[keep], np.stack([np.cumsum(cnt) - cnt, cnt], -1), term=term, limit=limit)
                    runs += 1
        # walk 3, the instantiation ced_traverse_grids' kernel runs: no distance fields, the plane of every ray specified
        counts = np.empty(n, np.int32); tt = np.zeros(n, np.float32)
        t0 = np.zeros((n, limit), np.float32); t1 = np.zeros((n, limit), np.float32)
        rc = hip.ced_host_march_frame(n, P(o), P(d), P(b8), m, res, P(aabbs), P(near), float(c["far"][0]), c["step"],
                                      c["cone_angle"], limit, P(ts), P(ti), P(hits8), None, 0, 0, 3, P(counts), P(t0), P(t1), P(tt))
        assert rc == 0
        keep = np.arange(limit)[None, :] < counts[:, None]
        cnt = counts.astype(np.int64)
        M.check_march(c["ref"], t0[keep], t1[keep], np.stack([np.cumsum(cnt) - cnt, cnt], -1), term=tt, limit=limit)
        runs += 1
    print(f"{name}: {runs} host marches pass")


# ---- sensitivity: the reference must reject wrong marches -------------------------------------------------------------
def test_reference_rejects_wrong_marches(oracle):
    c = M.case("speckle16_L1")
    rolled = np.roll(c["binaries"], 1, axis=3)
    cleared = c["binaries"].copy()
    hit = np.argwhere(cleared)
    cleared[tuple(hit[np.random.default_rng(0).choice(hit.shape[0], 20, replace=False)].T)] = False
    for what, grid in (("rolled by one cell along z", rolled), ("20 occupied cells cleared", cleared)):
        w = _oracle_march(oracle, c, binaries=grid)
        with pytest.raises(AssertionError, match="disagreements on decided midpoints") as e:
            M.check_march(c["ref"], w["t_starts"], w["t_ends"], w["packed_info"], term=w["termination_planes"])
        print(f"{what}: {str(e.value)[:160]}")


# ---- chaining ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["speckle16_L1", "speckle20_L2", "speckle12_L4", "dynerf128_L4"])
def test_oracle_chained_budgets_concatenate_to_the_unlimited_march(oracle, name):
    """Oracle against oracle (the same check runs on the device in tests/test_gpu_march.py)."""
    c = M.case(name)

    def march(rays, near, limit):
        w = oracle.traverse_grids(c["o"][rays], c["d"][rays], c["binaries"], c["aabbs"], near, c["far"][rays], c["step"],
                                  c["cone_angle"], limit)
        return w["t_starts"], w["t_ends"], w["packed_info"][:, 1], w["termination_planes"]

    whole = _oracle_march(oracle, c)
    M.assert_chain_is_the_unlimited_march(*M.chain(march, c), whole["t_starts"], whole["t_ends"])
