"""CPU suite of the level-set entries: tests/level_set64.py's own properties (first_crossing on hand-made rays, bisect_f32 on
an analytic density), and the two C entries' symbols and argument checks (called without a device, as
tests/test_time_slices_cpu.py calls entries: every case returns before a launch)."""
import ctypes as C

import numpy as np
import pytest

import level_set64 as LS

F = np.float32


# ---- first_crossing ----------------------------------------------------------------------------------------------------------
def test_first_crossing_on_hand_made_rays():
    """Seven rays, each in a state of its own: crossing at the first sample, at a middle sample behind a contiguous
    predecessor, behind a gap, at the last sample, a NaN before the crossing, no crossing, no samples."""
    t0 = F([0.0, 1.0, 2.0,   0.0, 1.0, 2.0,   0.0, 1.5, 2.5,   3.0, 4.0,   0.0, 1.0, 2.0,   5.0, 6.0])
    t1 = F([1.0, 2.0, 3.0,   1.0, 2.0, 3.0,   1.0, 2.5, 3.5,   4.0, 5.0,   1.0, 2.0, 3.0,   6.0, 7.0])
    sg = F([9.0, 0.0, 9.0,   0.0, 2.0, 9.0,   0.0, 0.5, 2.0,   0.0, 1.0,   np.nan, 0.1, 3.0,   0.5, 0.999])
    packed = np.asarray([[0, 3], [3, 3], [6, 3], [9, 2], [11, 3], [14, 2], [16, 0]], np.int64)
    k, lo, hi = LS.first_crossing(packed, t0, t1, sg, 1.0)
    assert k.dtype == np.int64 and lo.dtype == np.float32 and hi.dtype == np.float32
    assert k.tolist() == [0, 4, 8, 10, 13, -1, -1]
    assert hi.tolist() == [0.5, 1.5, 3.0, 4.5, 2.5, 0.0, 0.0]
    # first sample: its own start; contiguous predecessor: its midpoint; 1.0 != 1.5 is a gap before sample 7, but sample
    # 8's predecessor (7) is contiguous; the last sample of ray 3 follows a contiguous one; the NaN sample is a predecessor
    # like any other
    assert lo.tolist() == [0.0, 0.5, 2.0, 3.5, 1.5, 0.0, 0.0]
    # a gap directly before the crossing sample: lo is that sample's start
    k, lo, hi = LS.first_crossing([[0, 2]], F([0.0, 1.5]), F([1.0, 2.5]), F([0.0, 2.0]), 1.0)
    assert (k.tolist(), lo.tolist(), hi.tolist()) == ([1], [1.5], [2.0])
    # the predecessor of a ray's first sample belongs to another ray, touching or not
    k, lo, hi = LS.first_crossing([[0, 1], [1, 1]], F([0.0, 1.0]), F([1.0, 2.0]), F([0.0, 2.0]), 1.0)
    assert (k.tolist(), lo.tolist(), hi.tolist()) == ([-1, 1], [0.0, 1.0], [0.0, 1.5])
    # the threshold itself qualifies, the float below it does not
    below = np.nextafter(F(1.0), F(0.0))
    assert LS.first_crossing([[0, 2]], F([0, 1]), F([1, 2]), F([below, 1.0]), 1.0)[0].tolist() == [1]
    assert LS.first_crossing(np.zeros((0, 2), np.int64), F([]), F([]), F([]), 1.0)[0].shape == (0,)


# ---- bisect_f32 --------------------------------------------------------------------------------------------------------------
def _analytic(a, t_star):
    """f(t) = exp(a (t - t*)) along the x axis from the origin: p = (t, 0, 0); evaluated in float64, rounded once"""
    return lambda p: np.exp(np.float64(a) * (p[:, 0].astype(np.float64) - t_star)).astype(np.float32)


def _spacing(t):
    return np.spacing(np.abs(t).astype(np.float32))


def test_bisection_straddles_the_analytic_root():
    rng = np.random.default_rng(3)
    n = 64
    t_star = rng.uniform(0.5, 3.5, n)
    o = np.zeros((n, 3), np.float32)
    d = np.tile(F([1.0, 0.0, 0.0]), (n, 1))
    lo = (t_star - rng.uniform(0.01, 0.4, n)).astype(np.float32)
    hi = (t_star + rng.uniform(0.01, 0.4, n)).astype(np.float32)
    for a in (1.0, 40.0):
        f = _analytic(a, t_star)
        out = LS.bisect_f32(f, o, d, lo, hi, 1.0, 64, 0.0)
        assert (out["status"] == 0).all() and out["t"].dtype == np.float32 and out["evals"].dtype == np.int32
        t, w = out["t"], out["width"]
        assert (w >= 0).all() and (w <= _spacing(t)).all()                    # 0 or one float32 spacing at tol = 0
        assert np.array_equal(out["lo"], (t - w).astype(np.float32))
        # the bracket straddles t*: f rounds exp() to float32, which moves the float32 root by at most one spacing
        assert ((t - w).astype(np.float64) - _spacing(t) <= t_star).all() and (t_star <= t.astype(np.float64) + _spacing(t)).all()
        assert (out["sigma"] >= 1.0).all() and np.array_equal(out["sigma"], f(out["x"]))
        assert (f((o + d * out["lo"][:, None]).astype(np.float32)) < 1.0).all()
        assert np.array_equal(out["x"], (o + d * t[:, None]).astype(np.float32))
        assert (out["evals"] >= 2 + 15).all() and (out["evals"] <= 2 + 30).all()
        # fewer rounds, or a tolerance: wider brackets, fewer evaluations, the same invariant
        few = LS.bisect_f32(f, o, d, lo, hi, 1.0, 4, 0.0)
        assert (few["evals"] == 6).all() and (few["width"] > w).all() and (few["sigma"] >= 1.0).all()
        tol = LS.bisect_f32(f, o, d, lo, hi, 1.0, 64, 1e-3)
        assert (tol["width"] <= F(1e-3)).all() and (tol["width"] > F(1e-3) / 4).all() and (tol["evals"] < out["evals"]).all()
        none = LS.bisect_f32(f, o, d, lo, hi, 1.0, 0, 0.0)
        assert (none["evals"] == 2).all() and np.array_equal(none["t"], hi) and np.array_equal(none["width"], (hi - lo).astype(np.float32))


def test_bisection_reports_brackets_without_a_crossing():
    t_star = np.asarray([2.0, 2.0, 2.0, 2.0])
    f = _analytic(5.0, t_star)
    o = np.zeros((4, 3), np.float32)
    d = np.tile(F([1.0, 0.0, 0.0]), (4, 1))
    lo, hi = F([2.5, 2.0, 0.5, 1.0]), F([3.0, 3.0, 1.5, 3.0])
    out = LS.bisect_f32(f, o, d, lo, hi, 1.0, 32, 0.0)
    assert out["status"].tolist() == [1, 1, 2, 0]                            # inside, on the threshold, never reached, crossing
    assert out["evals"][:3].tolist() == [2, 2, 2] and out["evals"][3] > 2
    assert out["t"][:3].tolist() == [2.5, 2.0, 1.5] and out["width"][:3].tolist() == [0.0, 0.0, 1.0]
    assert np.array_equal(out["sigma"][:3], np.concatenate([f(np.stack([lo, lo * 0, lo * 0], -1))[:2], f(np.stack([hi, hi * 0, hi * 0], -1))[2:3]]))
    assert out["t"][3] == 2.0 and out["width"][3] == np.spacing(F(1.0))     # (t - width) is the float below 2
    # a NaN density: at hi it is "never reaches", at a midpoint it goes to lo
    nan_hi = LS.bisect_f32(lambda p: np.full(len(p), np.nan, np.float32), o, d, lo, hi, 1.0, 8, 0.0)
    assert nan_hi["status"].tolist() == [2, 2, 2, 2] and nan_hi["evals"].tolist() == [2, 2, 2, 2]
    f1 = _analytic(5.0, t_star[3:])
    holes = lambda p: np.where((p[:, 0] > 1.2) & (p[:, 0] < 2.2), np.nan, f1(p)).astype(np.float32)
    out = LS.bisect_f32(holes, o[3:], d[3:], lo[3:], hi[3:], 1.0, 64, 0.0)
    assert out["status"].tolist() == [0] and out["t"][0] == F(2.2) and out["sigma"][0] >= 1.0


# ---- raw_model -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("div,tm,table", [(False, 0, "f32"), (True, 2, "f32"), (True, 2, "temporal")])
def test_raw_model_is_the_models_it_abridges(div, tm, table):
    """raw_model == density64.base_gradient behind warp64.move_jacobian (their primal halves, without the tangents) to
    1e-11 in float64, unrounded and rounded as f32 / f16x2 round; -inf outside the box"""
    import density64 as D
    import warp64 as W
    from ced_nerf_amd import synthetic as S
    params = S.init_field_params([-1.5] * 3 + [1.5] * 3, 1.0 / 32, hash_max_res=256, log2_hashmap_size=15, use_div_offsets=div,
                                 use_time_embedding=tm != 0, use_time_attenuation=tm == 2, regime="trained",
                                 temporal_hash=table == "temporal")
    rng = np.random.default_rng(5)
    x = rng.uniform(-1.7, 1.7, size=(300, 3))
    t = rng.uniform(0.0, 1.0, size=300).astype(np.float32).astype(np.float64)
    for mode in (None, "f32", "f16x2"):
        move = W.move_jacobian(params, x, t, np.float64, None if mode is None else W.MOTION_MODES[mode])[0]
        aabb = np.asarray(params["aabb"], np.float32).astype(np.float64)
        xn = ((x + move) - aabb[:3]) / (aabb[3:] - aabb[:3])
        inside = ((xn > 0) & (xn < 1)).all(-1)
        raw = D.base_gradient(params, np.clip(xn, 0.0, 1.0).astype(np.float32), t.astype(np.float32), np.sqrt((move * move).sum(-1)),
                              np.float64, None if mode is None else D.BASE_MODES[mode])[0]
        got = LS.raw_model(params, x, t, mode)
        assert 50 < inside.sum() < 290 and np.array_equal(np.isfinite(got), inside), mode
        assert np.abs(got[inside] - (raw[inside] - 1.0)).max() <= 1e-11, mode          # the matrix products' batches differ
    assert np.array_equal(LS.raw64(params, x, t), LS.raw_model(params, x, t, None))


# ---- the C entries -----------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_check_their_arguments():
    from ced_nerf_amd import _lib
    names = ("ced_surface_first_crossing", "ced_field_level_set")
    assert "surface.hip" in _lib.SOURCES and "field_level_set.hip" in _lib.SOURCES
    assert all(n in _lib.PROTOTYPES and n in _lib.header_symbols() for n in names)
    from ced_nerf_amd import export, model, ops, utils
    assert all(callable(f) for f in (ops.surface_first_crossing, ops.field_level_set, model.DNGPradianceField.query_level_set,
                                     utils.render_surface, export.refine_mesh))
    L = _lib.lib()
    err = lambda: L.ced_last_error_string().decode()
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, C.c_void_p)
    fc = lambda n, p=ptr, thresh=1.0: L.ced_surface_first_crossing(n, p, p, p, p, thresh, p, p, p, None)
    assert (fc(-1), err()) == (-1, "surface_first_crossing: n_rays < 0")
    assert fc(0, None) == 0                                                                         # 0 rays launch nothing
    assert (fc(4, None), err()) == (-1, "surface_first_crossing: null pointer")
    assert (fc(4, ptr, float("nan")), err()) == (-1, "surface_first_crossing: thresh is a NaN")

    d = _lib.FieldDesc()
    d.packed_weights = ptr
    d.packed_floats = L.ced_packed_weight_words(0, 0, 0)
    d.hash.n_levels = 12                                  # a table validate_hash accepts: twelve hashed levels of 8 entries
    d.hash.table = ptr
    d.hash.total_entries = 8 * 12
    for l in range(12):
        d.hash.scale[l], d.hash.res[l], d.hash.offset[l], d.hash.size[l], d.hash.hashed[l] = 1.0, 2, 8 * l, 8, 1

    def ls(desc, n, p=ptr, thresh=1.0, max_iters=32, tol=0.0, out=ptr):
        return L.ced_field_level_set(desc, n, p, p, p, p, p, 1, thresh, max_iters, tol, out, out, out, out, out, out, None)

    D = C.byref(d)
    assert (ls(None, 4), err()) == (-1, "field_level_set: null descriptor")
    assert (ls(D, -1), err()) == (-1, "field_level_set: n < 0")
    assert (ls(D, 4, max_iters=-1), err()) == (-1, "field_level_set: max_iters=-1 outside 0 .. 64")
    assert (ls(D, 4, max_iters=65), err()) == (-1, "field_level_set: max_iters=65 outside 0 .. 64")
    assert (ls(D, 4, thresh=0.0), err()) == (-1, "field_level_set: thresh=0 must be > 0 (and not a NaN)")
    assert (ls(D, 4, thresh=float("nan")), err()) == (-1, "field_level_set: thresh=nan must be > 0 (and not a NaN)")
    assert (ls(D, 4, tol=-1.0), err()) == (-1, "field_level_set: tol=-1 must be >= 0 (and not a NaN)")
    assert (ls(D, 4, tol=float("nan")), err()) == (-1, "field_level_set: tol=nan must be >= 0 (and not a NaN)")
    assert ls(D, 0, None, max_iters=0, out=None) == 0                                              # n == 0 launches nothing
    assert (ls(D, 4, None), err()) == (-1, "field_level_set: null origins/dirs/lo/hi/times")
    assert (ls(D, 4, out=None), err()) == (-1, "field_level_set: no output requested")
    assert (ls(D, 4), err()) == (-1, "field_level_set: the kernel needs n_levels == 16 (got 12)")
    # a table beyond 32-bit byte offsets is refused in the words of the sibling entries
    d.hash.n_levels = 16
    for l in range(16):
        d.hash.scale[l], d.hash.res[l], d.hash.offset[l], d.hash.size[l], d.hash.hashed[l] = 1.0, 2, 8 * l, 8, 1
    d.hash.total_entries = 1 << 30
    rc, words = ls(D, 4), err()
    tm = L.ced_field_density_time_max(D, 4, ptr, 1, 1, ptr, ptr, None)
    assert rc == tm == -1 and words == err().replace("field_density_time_max", "field_level_set") and "field_level_set" in words


def test_python_argument_checks():
    from ced_nerf_amd import ops
    assert ops.check_level_set(1, 0, 0) == (1.0, 0, 0.0) and ops.check_level_set(np.float32(10), np.int64(64), 1e-4) == (10.0, 64, 1e-4)
    for bad in ((0.0, 32, 0.0), (-1.0, 32, 0.0), (float("nan"), 32, 0.0), (1.0, -1, 0.0), (1.0, 65, 0.0), (1.0, True, 0.0),
                (1.0, 3.0, 0.0), (1.0, 32, -1e-9), (1.0, 32, float("nan")), ("x", 32, 0.0), (1.0, 32, None)):
        with pytest.raises(ValueError):
            ops.check_level_set(*bad)
    assert ops.LEVEL_SET_OUTPUTS == ("t", "x", "sigma", "width", "status", "evals")


def test_cli_parses_mesh_refine(capsys):
    from ced_nerf_amd import export as E
    base = ["--load_model", "m", "--preset", "dnerf", "--out", "o"]
    a = E.make_parser().parse_args(base + ["--mesh", "--mesh_refine", "--mesh_refine_reach", "1.5"])
    assert a.mesh_refine and a.mesh_refine_reach == 1.5
    a = E.make_parser().parse_args(base)
    assert not a.mesh_refine and a.mesh_refine_reach == 1.0
    for argv, words in ((["--mesh_refine"], "--mesh_refine needs --mesh"),
                        (["--mesh", "--mesh_refine", "--mesh_refine_reach", "0"], "--mesh_refine_reach must be positive")):
        with pytest.raises(SystemExit) as e:                             # refused before anything is loaded
            E.main(base + argv)
        assert words in str(e.value)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError):
            E._check_reach(bad)


def test_level_set_kernels_run_without_scratch():
    """DESIGN 4.1g, "no scratch in any": LevelSetOp is built for eight table kinds x three staged planes, and none of the
    24 kernels spills a register or has a private segment."""
    from ced_nerf_amd import _lib
    from test_cabi_cpu import _kernel_notes
    stats = _kernel_notes(_lib.build())
    if stats is None:
        pytest.skip("llvm-readelf not found")
    kernels = {name: s for name, s in stats.items() if "LevelSetOp" in name}
    assert len(kernels) == 24, f"LevelSetOp: {len(kernels)} kernels in the built library"
    for name, (_, spilt, private) in kernels.items():
        assert spilt == 0 and private == 0, f"{name}: {spilt} spilt registers, {private} B private segment"
