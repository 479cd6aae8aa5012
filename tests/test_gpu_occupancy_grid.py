"""GPU suite: the two device-built pieces of the occupancy grid that decide which cells get marched.

  ops.occ_ema_update_ (ced_occ_ema_update, csrc/occgrid.hip) against occgrid_reference.ema_update, bit for bit over the
  whole array, on index lists with repeated cells -- what OccGridEstimator._sample_uniform_and_occupied_cells hands it
  after warm-up (a draw with replacement, then the occupied cells once more);

  ops.build_occupancy_accel (csrc/accel.hip) against occgrid_reference.chebyshev_fields and, byte for byte, against
  the host twin, at sizes on both sides of every path the build takes: one brick, a partial last brick, the
  one-workgroup brick kernel at its 64 KiB of LDS (nb = 32) and the global-memory rounds beyond (nb > 32); then the
  frame renderer on such a grid with and without a caller's accel, and the estimator's cache of the fields."""
import ctypes as C

import numpy as np
import pytest
import torch

import occgrid_reference as R
from conftest import assert_bitexact

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DECAY = 0.95


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


# ---- the EMA update ---------------------------------------------------------------------------------------------------
def check_ema(occs, ids, occ, name, step_size=1.0):
    """Two launches from the same start: both equal the reference bit for bit, untouched cells included."""
    from ced_nerf_amd import ops
    occs = np.ascontiguousarray(occs, np.float32)
    ids = np.ascontiguousarray(ids, np.int64)
    occ = np.ascontiguousarray(occ, np.float32)
    step = np.float32(step_size)
    want = R.ema_update(occs, ids, (occ * step).astype(np.float32), DECAY)
    ids_t, occ_t = T(ids), T(occ)
    runs = []
    for _ in range(2):
        o = T(occs.copy())
        ops.occ_ema_update_(o, ids_t, occ_t, float(step), DECAY)
        runs.append(N(o))
    assert_bitexact(runs[0], want, name)
    assert_bitexact(runs[1], runs[0], name + ", second launch")
    return want


SMALLEST = [            # old value of the repeated cell, the two samples
    ("decayed above both", 1.0, (0.3, 0.6)),
    ("decayed between them", 0.5, (0.3, 0.6)),
    ("decayed below both", 0.1, (0.3, 0.6)),
    ("invisible cell", -1.0, (0.3, 0.6)),
    ("invisible cell, zero samples", -1.0, (0.0, 0.0)),
    ("invisible cell, samples below it", -1.0, (-2.0, -3.0)),
    ("one NaN sample, decayed below the other", 0.5, (np.nan, 0.6)),
    ("one NaN sample, decayed above the other", 1.0, (np.nan, 0.6)),
]


@pytest.mark.parametrize("name,old,pair", SMALLEST, ids=[c[0].replace(" ", "_").replace(",", "") for c in SMALLEST])
def test_ema_update_one_cell_listed_twice(name, old, pair):
    rng = np.random.default_rng(0)
    occs = rng.uniform(0, 1, size=37).astype(np.float32)
    c = 21
    occs[c] = old
    for a, b in (pair, pair[::-1]):
        want = check_ema(occs, [c, c], [a, b], name)
        valid = [v for v in (a, b) if not np.isnan(v)]
        assert want[c] == max(np.float32(old) * np.float32(DECAY), np.float32(max(valid)))


def test_ema_update_empty_list():
    occs = np.random.default_rng(1).uniform(-1, 1, size=300).astype(np.float32)
    check_ema(occs, np.zeros(0, np.int64), np.zeros(0, np.float32), "n = 0")


@pytest.mark.parametrize("repeat", [2, 64, 65, 257])
def test_ema_update_repeats_in_a_row(repeat):
    """Each of 1000 cells listed `repeat` times in a row with distinct samples: repeats inside one wave (2, 64), across
    two waves (65) and across workgroups (257)."""
    rng = np.random.default_rng(repeat)
    cells = 4096
    occs = rng.uniform(0, 1, size=cells).astype(np.float32)
    occs[rng.integers(0, cells, size=200)] = -1.0
    listed = rng.permutation(cells)[:1000]
    ids = np.repeat(listed, repeat)
    density = rng.uniform(0, 200, size=len(ids)).astype(np.float32)
    assert len(np.unique(density)) > 0.99 * len(density)
    want = check_ema(occs, ids, density, f"{repeat} in a row", step_size=5e-3)
    assert (want[listed] >= occs[listed] * np.float32(DECAY)).all()


def test_ema_update_repeats_far_apart_decay_once():
    """The same 2^20 cells listed twice, 2^20 entries apart, with samples of 0: every listed cell decays ONCE."""
    cells = 128 ** 3
    perm = np.random.default_rng(5).permutation(cells)[: 1 << 20]
    ids = np.concatenate([perm, perm])
    want = check_ema(np.ones(cells, np.float32), ids, np.zeros(len(ids), np.float32), "far apart")
    listed = np.zeros(cells, bool); listed[perm] = True
    assert (want[listed] == np.float32(DECAY)).all() and (want[~listed] == 1.0).all()


def test_update_on_the_draw_training_makes(oracle):
    """OccGridEstimator._update on the lists _sample_uniform_and_occupied_cells draws after warm-up (with replacement,
    plus the occupied cells), three calls chained: occs bit-exact against the oracle, binaries equal away from the
    threshold."""
    from ced_nerf_amd import synthetic as S
    from ced_nerf_amd.model import DNGPradianceField
    from ced_nerf_amd.nerfacc_api import OccGridEstimator
    res, levels = 32, 2
    roi = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
    p = S.init_field_params(S.enlarge_aabb(roi, 2), 1.0 / 4096, 1024, 15, regime="trained", use_time_embedding=True)
    of = oracle.OracleField(p)
    f = DNGPradianceField.from_params(p, DEV).eval()
    est = OccGridEstimator(roi, res, levels).to(DEV)
    rng = np.random.default_rng(0)
    cells = res ** 3
    step = 5e-3
    aabbs = oracle.make_aabbs(roi, levels)
    state = {"occs": np.zeros(levels * cells, np.float32)}

    def update(it, idx):
        noise = [rng.uniform(0, 1, size=(len(i), 3)).astype(np.float32) for i in idx]
        tt = [rng.uniform(0, 1, size=len(i)).astype(np.float32) for i in idx]
        o_calls, g_calls = iter(tt), iter(tt)
        occs_o, bin_o = oracle.occ_grid_update(state["occs"], aabbs, res, idx, noise,
                                               lambda x: of.forward(x, next(o_calls))["density"] * np.float32(step),
                                               occ_thre=0.01, ema_decay=DECAY)
        est._update(step=it, occ_eval_fn=lambda x: f.query_density(x, T(next(g_calls))[:, None])["density"] * step,
                    occ_thre=0.01, ema_decay=DECAY, _lvl_indices=[T(i) for i in idx], _noise=[T(n_) for n_ in noise])
        assert_bitexact(N(est.occs), occs_o, f"occs after the update of step {it}")
        thre = min(float(occs_o[occs_o >= 0].astype(np.float64).mean()), 0.01)
        away = np.abs(occs_o - thre) > 1e-6
        assert np.array_equal(N(est.binaries).reshape(-1)[away], bin_o[away])
        assert 0.0 < bin_o.mean() < 1.0
        state["occs"] = occs_o

    update(0, [np.arange(cells, dtype=np.int64)] * levels)          # warm-up: every cell once
    torch.manual_seed(0)
    for k in range(3):
        idx = [N(i).astype(np.int64) for i in est._sample_uniform_and_occupied_cells(cells // 4)]
        for lvl, i in enumerate(idx):
            assert len(np.unique(i)) < len(i), f"level {lvl}: the draw holds no repeated cell"
        update(256 + 16 * k, idx)


# ---- the distance fields ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hip():
    from ced_nerf_amd import _lib
    return _lib.lib()


def host_build(hip, binaries):
    m, res = binaries.shape[0], binaries.shape[1]
    accel = np.zeros((int(hip.ced_occupancy_accel_bytes(m, res)),), np.uint8)
    b = np.ascontiguousarray(binaries, np.uint8)
    assert hip.ced_host_build_occupancy_accel(b.ctypes.data_as(C.c_void_p), m, res, accel.ctypes.data_as(C.c_void_p)) == 0
    return accel


def device_fields(binaries_t):
    from ced_nerf_amd import ops
    m, res = binaries_t.shape[0], binaries_t.shape[1]
    return R.accel_regions(N(ops.build_occupancy_accel(binaries_t.contiguous())), m, res)


@pytest.mark.parametrize("m,res,pattern", R.cases(), ids=["%dx%d-%s" % c for c in R.cases()])
def test_device_distance_fields(hip, m, res, pattern):
    b = R.make_pattern(m, res, pattern)
    bdist, cdist = device_fields(T(b))
    R.check_fields(bdist, cdist, b, pattern)
    want_b, want_c = R.accel_regions(host_build(hip, b), m, res)
    assert np.array_equal(bdist, want_b), "brick field differs from the host twin"
    assert np.array_equal(cdist, want_c), "cell field differs from the host twin"


def test_device_distance_fields_from_bool_binaries():
    """The estimator's `binaries` are torch.bool."""
    b = R.make_pattern(2, 40, "random")
    bd, cd = device_fields(T(b).bool())
    bd8, cd8 = device_fields(T(b))
    assert np.array_equal(bd, bd8) and np.array_equal(cd, cd8)


def test_frame_renderer_on_a_grid_of_global_rounds(oracle):
    """(2, 264), one occupied blob, 24 x 18 rays: the frame with the caller's accel (brick and cell fields) and with
    none (the brick field built inside the call, its rounds through the call's workspace) are each other's and the
    oracle's bits."""
    from ced_nerf_amd import ops, synthetic as S
    from ced_nerf_amd.model import DNGPradianceField
    from ced_nerf_amd.nerfacc_api import OccGridEstimator
    m, res, w, h = 2, 264, 24, 18
    cfg = S.CONFIGS["dnerf"]
    params = S.init_field_params(S.enlarge_aabb(cfg["aabb"], 2), cfg["moving_step"], cfg["hash_max_res"], 10, regime="trained")
    origins, viewdirs = S.make_camera_rays(w, h, cfg["camera_angle_x"], S.look_at_c2w(cfg["radius"], 30.0, 30.0, cfg["opengl"]),
                                           cfg["opengl"])
    b = np.zeros((m, res, res, res), bool)
    b[0, 90:180, 95:175, 100:180] = True                            # the blob, and about the same region of space in level 1
    b[1, 111:156, 111:156, 111:156] = True
    ts = np.array([[0.5]], np.float32)
    rk = dict(near_plane=cfg["near_plane"], far_plane=cfg["far_plane"], render_step_size=cfg["render_step_size"],
              cone_angle=cfg["cone_angle"])
    bkgd = np.asarray(cfg["bkgd"], np.float32)
    oest = oracle.OracleEstimator(cfg["aabb"], res, m, b)
    w_rgb, w_op, w_dp, w_total = oracle.render_image_test(1024, oracle.OracleField(params), oest, origins, viewdirs,
                                                          timestamps=ts, alpha_thre=cfg["alpha_thre"], render_bkgd=bkgd, **rk)
    assert w_total > 1000 and 0.05 < (w_op > 0.5).mean() < 0.95      # the blob is in view and does not fill it
    f = DNGPradianceField.from_params(params, DEV).eval()
    est = OccGridEstimator(cfg["aabb"], res, m).to(DEV)
    est.set_binaries(T(b))
    for accel in (est.occupancy_accel(), None):
        rgb, op, dp, total = ops.render_image_test_native(
            f._descriptor(), T(origins.reshape(-1, 3)), T(viewdirs.reshape(-1, 3)), est.binaries, est.aabbs.contiguous(),
            rk["near_plane"], rk["far_plane"], rk["render_step_size"], rk["cone_angle"], 1e-4, 1024, T(ts.reshape(-1)), False,
            T(bkgd), accel=accel)
        tag = "caller's accel" if accel is not None else "brick field built per call"
        assert total == w_total, (tag, total, w_total)
        assert_bitexact(N(rgb), w_rgb.reshape(-1, 3), f"rgb, {tag}")
        assert_bitexact(N(op), w_op.reshape(-1, 1), f"opacity, {tag}")
        assert_bitexact(N(dp), w_dp.reshape(-1, 1), f"depth, {tag}")


def test_estimator_accel_follows_every_writer_of_binaries():
    """est.occupancy_accel() is the field of the CURRENT binaries after each way the grid can change; every change here
    moves the fields, so a stale cache cannot pass."""
    from ced_nerf_amd.nerfacc_api import OccGridEstimator
    m, res = 2, 24
    est = OccGridEstimator([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], res, m).to(DEV)
    grids = [T(R.make_pattern(m, res, p)).bool() for p in ("random", "corner3", "last_brick", "centre")]
    seen = []

    def check(what):
        got = R.accel_regions(N(est.occupancy_accel()), m, res)
        want = device_fields(est.binaries)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f"stale distance fields after {what}"
        for old in seen:
            assert not np.array_equal(got[1], old), f"{what} did not change the grid"
        seen.append(got[1].copy())
        assert est.occupancy_accel() is est.occupancy_accel()        # kept while nothing changes

    check("construction")
    est.set_binaries(grids[0])
    check("set_binaries")
    cells = res ** 3
    idx = [torch.arange(cells, device=DEV)] * m
    noise = [torch.full((cells, 3), 0.5, device=DEV)] * m
    est._update(step=0, occ_eval_fn=lambda x: (x.norm(dim=1) < 0.6).float(), _lvl_indices=idx, _noise=noise)
    assert 0 < int(est.binaries.sum()) < est.binaries.numel()
    check("_update")
    est.binaries.copy_(grids[1])
    check("binaries.copy_")
    other = OccGridEstimator([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], res, m).to(DEV)
    other.set_binaries(grids[2])
    est.load_state_dict(other.state_dict())
    assert torch.equal(est.binaries, grids[2])
    check("load_state_dict")
    est.binaries.data.copy_(grids[3])                                # bypasses the version counter
    est.invalidate_accel()
    check("a .data write and invalidate_accel")
