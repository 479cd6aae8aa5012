"""CPU suite of the time-sliced occupancy grids: the numpy reference's own properties, TimeSlicedOccGrid's bin arithmetic,
cache and state_dict, utils.grid_for on a plain estimator, the CLI flags, the C entries' argument checks (called without a
device, as tests/test_cabi_cpu.py calls entries: every case returns before a launch), and the moving ball's cell counts from
the CPU oracle's density, which tests/test_gpu_time_slices.py relies on."""
import ctypes as C

import numpy as np
import pytest
import torch

import occ_time_reference as R


# ---- the reference's own properties -------------------------------------------------------------------------------------
def _analytic(res, B):
    """maxima of a blob that walks along x: bin b's is centred at x = (b + 0.5) / B"""
    cells = np.arange(res ** 3)
    c = (np.stack([cells // (res * res), (cells // res) % res, cells % res], -1) + 0.5) / res
    centre = np.stack([(np.arange(B) + 0.5) / B, np.full(B, 0.5), np.full(B, 0.5)], -1)
    d2 = ((c[None] - centre[:, None]) ** 2).sum(-1)
    return cells.astype(np.int64), np.exp(-d2 / 0.02).astype(np.float32)


def test_reference_dilation_never_leaves_the_union():
    cells, mx = _analytic(12, 4)
    union = (np.random.default_rng(0).uniform(size=(1, 12, 12, 12)) < 0.5)
    plain = R.time_slices(cells, mx, 1.0, 0.5, 1, 12, None, 0)
    grown = R.time_slices(cells, mx, 1.0, 0.5, 1, 12, None, 1)
    kept = R.time_slices(cells, mx, 1.0, 0.5, 1, 12, union, 1)
    assert not (plain & ~grown).any() and grown.sum() > plain.sum() > 0          # dilation only adds
    assert not (kept & ~union[None]).any() and np.array_equal(kept, grown & union[None])
    assert not np.array_equal(plain[0], plain[3])                                # the blob moves
    # a single hit grows into its 27 neighbours, clipped at the level's faces and never into the next level
    one = np.zeros((1, 2 * 4 ** 3), np.float32)
    one[0, 0] = one[0, 4 ** 3 + 21] = 1.0                                        # level 0's corner, level 1's cell (1, 1, 1)
    out = R.time_slices(np.arange(2 * 4 ** 3), one, 1.0, 0.5, 2, 4, None, 1)
    assert out[0, 0].sum() == 8 and out[0, 0, :2, :2, :2].all() and out[0, 1].sum() == 27 and out[0, 1, :3, :3, :3].all()


def test_reference_one_bin_without_dilation_is_the_plain_threshold():
    rng = np.random.default_rng(1)
    mx = rng.uniform(0, 2, size=(1, 64)).astype(np.float32)
    mx[0, :4] = [np.nan, np.inf, 1.0, np.nextafter(np.float32(1.0), np.float32(2.0))]
    out = R.time_slices(np.arange(64), mx, 0.5, 0.5, 1, 4, None, 0)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(out.reshape(-1), (mx[0] * np.float32(0.5)) > np.float32(0.5))
    assert out.reshape(-1)[:4].tolist() == [False, True, False, True]
    listed = np.array([3, 9], np.int64)                                          # cells that are not listed are not hit
    assert R.time_slices(listed, np.full((1, 2), 9.0, np.float32), 1.0, 0.5, 1, 4, None, 0).reshape(-1).nonzero()[0].tolist() == [3, 9]


def test_reference_probe_times():
    t = R.probe_times(4, 3)
    assert t.dtype == np.float32 and t.shape == (4, 3) and t[0, 0] == 0 and t[-1, -1] == 1
    assert np.array_equal(t[1:, 0], t[:-1, -1])                                  # neighbouring bins share their end time
    assert np.array_equal(R.probe_times(4, 1)[:, 0], np.float32([0.125, 0.375, 0.625, 0.875]))
    from ced_nerf_amd.nerfacc_api import TimeSlicedOccGrid
    for B, S in ((1, 1), (4, 3), (16, 5), (7, 64), (256, 2)):
        assert np.array_equal(TimeSlicedOccGrid.probe_times(B, S).numpy(), R.probe_times(B, S)), (B, S)
    for B, S in ((0, 1), (257, 1), (1, 0), (1, 65)):
        with pytest.raises(ValueError):
            TimeSlicedOccGrid.probe_times(B, S)


# ---- TimeSlicedOccGrid -----------------------------------------------------------------------------------------------------
def _grid(B=8):
    from ced_nerf_amd.nerfacc_api import TimeSlicedOccGrid
    g = TimeSlicedOccGrid([-1, -1, -1, 1, 1, 1], 4, 2, B)
    slices = torch.zeros_like(g.binaries_t)
    for b in range(B):
        slices[b, b % 2].view(-1)[b] = True
    g.set_slices(slices)
    return g


def test_bin_arithmetic_of_at_time():
    g = _grid(8)
    assert g.bin_range(0.0) == (0, 0) and g.bin_range(1.0) == (7, 7)
    assert g.bin_range(0.25) == (2, 2) and g.bin_range(np.nextafter(0.25, 0.0)) == (1, 1)       # an exact edge opens its bin
    assert g.bin_range(-3.0) == (0, 0) and g.bin_range(7.0) == (7, 7)
    assert g.bin_range([0.9, 0.1]) == (0, 7) and g.bin_range((0.3,)) == (2, 2)
    assert g.bin_range(torch.tensor([[0.30, 0.55], [0.40, 0.45]])) == (2, 4)                      # three bins
    assert g.bin_range(torch.tensor(0.5)) == (4, 4)
    for bad in (float("nan"), [], torch.zeros(0)):
        with pytest.raises(ValueError):
            g.bin_range(bad)
    est = g.at_time(torch.tensor([[0.30, 0.55], [0.40, 0.45]]))
    from ced_nerf_amd.nerfacc_api import OccGridEstimator
    assert type(est) is OccGridEstimator and est.binaries.shape == (2, 4, 4, 4)
    assert torch.equal(est.binaries, g.binaries_t[2:5].any(0)) and int(est.binaries.sum()) == 3
    assert torch.equal(est.aabbs, g.aabbs) and torch.equal(est.resolution, g.resolution) and not est.training


def test_estimators_are_cached_per_range():
    g = _grid(8)
    a = g.at_time(0.30)
    assert g.at_time(0.36) is a and g.at_time([0.26, 0.37]) is a and g.at_time(0.40) is not a
    assert g.union() is g.union() and g.union() is g.at_time([0.0, 1.0])
    assert torch.equal(g.union().binaries, g.binaries_t.any(0)) and int(g.union().binaries.sum()) == 8
    assert torch.equal(g.occupied_fraction(), torch.full((8,), 0.125))
    changed = g.binaries_t.clone()
    changed[2] = False
    g.set_slices(changed)                                                # new slices: new estimators
    b = g.at_time(0.30)
    assert b is not a and int(b.binaries.sum()) == 0 and int(a.binaries.sum()) == 1
    assert torch.equal(g.occupied_fraction()[:3], torch.tensor([1 / 7, 1 / 7, 0.0]))
    from ced_nerf_amd.nerfacc_api import TimeSlicedOccGrid
    assert not bool(TimeSlicedOccGrid([-1, -1, -1, 1, 1, 1], 4, 1, 2).occupied_fraction().any())  # an empty union


def test_state_dict_round_trip():
    from ced_nerf_amd.nerfacc_api import TimeSlicedOccGrid
    g = _grid(8)
    state = g.state_dict()
    assert set(state) == {"binaries_t", "aabbs", "resolution"} and state["binaries_t"].dtype == torch.bool
    h = TimeSlicedOccGrid([-1, -1, -1, 1, 1, 1], 4, 2, 8)
    stale = h.at_time(0.3)
    h.load_state_dict(state)
    assert torch.equal(h.binaries_t, g.binaries_t) and torch.equal(h.aabbs, g.aabbs)
    assert h.at_time(0.3) is not stale and torch.equal(h.at_time(0.3).binaries, g.at_time(0.3).binaries)
    with pytest.raises(RuntimeError):
        TimeSlicedOccGrid([-1, -1, -1, 1, 1, 1], 4, 2, 4).load_state_dict(state)                  # another number of bins
    with pytest.raises(ValueError):
        TimeSlicedOccGrid([-1, -1, -1, 1, 1, 1], [4, 4, 8], 1, 4)
    with pytest.raises(ValueError):
        TimeSlicedOccGrid([-1, -1, -1, 1, 1, 1], 4, 1, 257)


def test_grid_for_is_the_identity_on_a_plain_estimator():
    from ced_nerf_amd.nerfacc_api import OccGridEstimator
    from ced_nerf_amd.utils import grid_for

    class NoRead:                                                        # a time that must not be looked at
        def __getattr__(self, name):
            raise AssertionError("grid_for read the timestamps of a plain estimator")

    est = OccGridEstimator([-1, -1, -1, 1, 1, 1], 4, 1)
    assert grid_for(est, NoRead()) is est and grid_for(est, None) is est and grid_for(None, 0.5) is None
    g = _grid(8)
    assert grid_for(g, 0.3) is g.at_time(0.3) and grid_for(g, torch.tensor([[0.1], [0.9]])) is g.union()
    assert grid_for(g, None) is g


def test_cli_parses_time_bins(capsys):
    from ced_nerf_amd import trainer
    base = ["--data_root", "x", "--scene", "y"]
    a = trainer.build_parser().parse_args(base + ["--render_video", "out", "--time_bins", "16"])
    assert a.time_bins == 16 and a.time_bin_samples == 5
    a = trainer.build_parser().parse_args(base + ["--render_video", "out", "--time_bins", "4", "--time_bin_samples", "9"])
    assert (a.time_bins, a.time_bin_samples) == (4, 9)
    assert trainer.build_parser().parse_args(base).time_bins is None
    for argv, words in ((["--dataset", "dnerf", "--time_bins", "4"], "--time_bins goes with --render_video"),
                        (["--dataset", "dnerf", "--render_video", "out", "--time_bins", "0"], "--time_bins takes 1 .. 256"),
                        (["--dataset", "dnerf", "--render_video", "out", "--time_bins", "4", "--time_bin_samples", "65"],
                         "--time_bin_samples 1 .. 64")):
        with pytest.raises(SystemExit):                                  # refused before anything is loaded
            trainer.main(base + argv)
        assert words in capsys.readouterr().err


# ---- the C entries ----------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_check_their_arguments():
    from ced_nerf_amd import _lib
    names = ("ced_field_density_time_max", "ced_occ_time_slices", "ced_occ_time_slices_workspace_bytes")
    assert "field_time_max.hip" in _lib.SOURCES
    assert all(n in _lib.PROTOTYPES and n in _lib.header_symbols() for n in names)
    from ced_nerf_amd import nerfacc_api, ops, utils
    assert all(callable(f) for f in (ops.field_density_time_max, ops.occ_time_slices, nerfacc_api.TimeSlicedOccGrid, utils.grid_for))
    L = _lib.lib()
    err = lambda: L.ced_last_error_string().decode()
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, C.c_void_p)
    d = _lib.FieldDesc()
    d.packed_weights = ptr
    d.packed_floats = L.ced_packed_weight_words(0, 0, 0)
    d.hash.n_levels = 12                                  # a table validate_hash accepts: twelve hashed levels of 8 entries
    d.hash.table = ptr
    d.hash.total_entries = 8 * 12
    for l in range(12):
        d.hash.scale[l], d.hash.res[l], d.hash.offset[l], d.hash.size[l], d.hash.hashed[l] = 1.0, 2, 8 * l, 8, 1
    tm = lambda desc, n, B, S, p=ptr: L.ced_field_density_time_max(desc, n, p, B, S, p, p, None)
    assert (tm(None, 4, 1, 1), err()) == (-1, "field_density_time_max: null descriptor")
    assert (tm(C.byref(d), -1, 1, 1), err()) == (-1, "field_density_time_max: n < 0")
    assert (tm(C.byref(d), 4, 0, 1), err()) == (-1, "field_density_time_max: n_bins=0 outside 1 .. 256")
    assert (tm(C.byref(d), 4, 257, 1), err()) == (-1, "field_density_time_max: n_bins=257 outside 1 .. 256")
    assert (tm(C.byref(d), 4, 1, 65), err()) == (-1, "field_density_time_max: n_times=65 outside 1 .. 64")
    assert (tm(C.byref(d), 4, 1, 0), err()) == (-1, "field_density_time_max: n_times=0 outside 1 .. 64")
    assert tm(C.byref(d), 0, 256, 64, None) == 0                                                   # n == 0 launches nothing
    assert (tm(C.byref(d), 4, 1, 1, None), err()) == (-1, "field_density_time_max: null positions/times/out")
    assert (tm(C.byref(d), 4, 1, 1), err()) == (-1, "field_density_time_max: the kernel needs n_levels == 16 (got 12)")

    ws = L.ced_occ_time_slices_workspace_bytes
    assert ws(16, 4, 128) == 16 * 4 * 128 ** 3 == 128 << 20 and ws(1, 1, 1) == 1
    assert all(ws(*bad) < 0 for bad in ((0, 1, 4), (257, 1, 4), (1, 0, 4), (1, 65, 4), (1, 1, 0), (1, 1, 1025)))
    sl = lambda n, B, dilate, ws_bytes, levels=1, res=4: L.ced_occ_time_slices(n, ptr, ptr, B, 1.0, 0.5, levels, res, None,
                                                                             dilate, ptr, ptr, ws_bytes, None)
    assert (sl(-1, 1, 1, 64), err()) == (-1, "occ_time_slices: n < 0")
    assert (sl(4, 0, 1, 64), err()) == (-1, "occ_time_slices: n_bins=0 outside 1 .. 256")
    assert (sl(4, 1, 2, 64), err()) == (-1, "occ_time_slices: dilate=2 must be 0 or 1")
    assert (sl(4, 1, -1, 64), err()) == (-1, "occ_time_slices: dilate=-1 must be 0 or 1")
    assert (sl(4, 1, 1, 64, levels=0), err()) == (-1, "occ_time_slices: levels=0 res=4")
    assert (sl(4, 2, 1, 127), err()) == (-1, "occ_time_slices: workspace too small (127 < 128 bytes)")
    assert L.ced_occ_time_slices(4, None, None, 1, 1.0, 0.5, 1, 4, None, 1, ptr, ptr, 64, None) == -1
    assert err() == "occ_time_slices: null cell_ids/max_sigma"


# ---- the moving ball's geometry, from the oracle's density ----------------------------------------------------------------------
def test_moving_ball_condition_holds_on_the_cpu(oracle):
    """What tests/test_gpu_time_slices.py's moving-ball test relies on, from the CPU oracle's density of ball_params:
    exp(7) at the ball's centre wherever the ball is, exp(-1) away from it; the union of the eight slices holds 2200 cells,
    the slices 1456, 1388, 1244, 1040, 1040, 1244, 1388, 1456; the slice of t = 0.45 (bin 3) holds 1040 / 2200 = 0.47 <= 3/4
    and every slice at most 0.82 of the union."""
    of = oracle.OracleField(R.ball_params())
    dens = lambda pos, t: of.forward(np.float32(pos), np.float32(t))["density"]
    assert dens([[0.4, 0, 0]], [0.0])[0] == dens([[-0.6, 0, 0]], [0.5])[0] == pytest.approx(np.exp(7.0), rel=1e-5)
    assert dens([[0.4, 0, 0]], [0.5])[0] == dens([[-1.2, 1, 1]], [0.3])[0] == pytest.approx(np.exp(-1.0), rel=1e-6)
    sl = R.ball_slices(lambda pos, t: of.forward(pos, t)["density"])
    counts = sl.reshape(8, -1).sum(1)
    n_union = int(sl.any(0).sum())
    assert n_union == 2200 and counts.tolist() == [1456, 1388, 1244, 1040, 1040, 1244, 1388, 1456]
    assert counts[min(int(0.45 * 8), 7)] <= 0.75 * n_union and (counts <= 0.82 * n_union).all()
