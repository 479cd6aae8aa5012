"""The inputs of tests/test_gpu_field_variants.py and tests/test_gpu_frame_variants.py, with the CPU oracle alone.

A GPU test that compares bit for bit proves nothing on a degenerate input, so what those tests need of their inputs is
asserted here, where no GPU is needed: the eight variants are the launchers' eight selectors; the sample times straddle
the key-frames within every wave; every frame scene runs a real loop in every arithmetic mode it is rendered in; and a
temporal table makes the frame depend on its time.  These are conditions on the inputs (set before the kernels ran), not
measurements of the code under test.

The frame scenes are held to: at least 4 iterations, at least 5000 samples, at least 10 % of the pixels ended by the early
stop (opacity > 0.99) and at least 10 % see-through (0 < opacity < 0.99), at the scene's own time float32(1/3).  The two
further times of test_render_frames_test (0.8 and 1) are other frames of the same scenes; the same scene does not meet
the pixel shares at every time (sel 5 at t = 0.8 ends no ray early), so they are held to the first two conditions and to
schedules that differ.  The fuzz seeds are random configurations in the stock regime, as the existing fuzz's: they are
held to producing samples."""
import numpy as np
import pytest

import field_variants as V


def _oracle_frame(oracle, sc, mode, timestamp=None, max_samples=1024):
    cfg = sc["cfg"]
    oest = oracle.OracleEstimator(cfg["aabb"], cfg["grid_resolution"], cfg["grid_levels"], sc["binaries"])
    ts = sc["timestamps"] if timestamp is None else np.array([[timestamp]], np.float32)
    trace = []
    out = oracle.render_image_test(max_samples, oracle.OracleField(sc["params"], mlp_half=mode), oest, sc["origins"],
                                   sc["viewdirs"], timestamps=ts, trace=trace, **sc["render"])
    return out, trace


def test_variants_are_the_eight_selectors():
    from ced_nerf_amd import synthetic as S
    for sel in V.SELS:
        p = S.init_field_params(V.AABB, 1.0 / 64, 64, 8, **V.variant_kw(sel))
        assert V.selector_of(p) == sel
        assert p["hash"]["table"].shape[1] == (8 if sel & 4 else 2)
        assert p["use_div_offsets"] == bool(sel & 1) and p["xyz_wrap"][3].shape[0] == (6 if sel & 1 else 3)
        assert p["time_mode"] == (2 if sel in (3, 7) else sel & 1)


def test_sample_times_straddle_the_key_frames():
    k = V.key_times()
    assert k.dtype == np.float32 and len(set(k.tolist())) == 8 and k.min() == 0 and k.max() == 1
    # the key-frame pair changes exactly at float32(1/3) and float32(2/3) (3 t rounds to 1 and to 2 there)
    assert V.keyframe_interval(k).tolist() == [0, 2, 1, 2, 0, 1, 1, 2]
    _, t, _ = V.sample_points(1061)
    t = t.reshape(-1)
    assert t.dtype == np.float32 and t.min() == 0 and t.max() == 1
    assert np.array_equal(t[:8], k) and np.array_equal(t[-8:], k)
    for w in (32, 64):
        assert all(set(V.keyframe_interval(t[b:b + w]).tolist()) == {0, 1, 2} for b in range(0, 1061 - w, w))
    assert np.array_equal(V.sample_times(3, np.random.default_rng(0)), k[:3])


@pytest.mark.parametrize("sel", V.SELS)
def test_per_sample_inputs_are_not_degenerate(oracle, sel):
    pos, t, d = V.sample_points(1061)
    out = oracle.OracleField(V.field_params(sel)).forward(pos, t, d)
    sigma = out["density"]
    assert (sigma == 0).sum() >= 12 and (sigma > 0).sum() > 500
    assert (sigma[:8] > 0).all() and (sigma[-8:] > 0).all()          # the key-frame times are inside the box
    if sel & 4:                                                     # and the table's key-frames change the result
        other = oracle.OracleField(V.field_params(sel)).forward(pos, np.where(t < 0.5, t + np.float32(0.4), t), d)
        assert (other["density"] != sigma)[(t.reshape(-1) < 0.5) & (sigma > 0)].mean() > 0.9


@pytest.mark.parametrize("mode", V.MODES)
@pytest.mark.parametrize("sel", V.SELS)
def test_frame_scene_conditions(oracle, sel, mode):
    sc = V.frame_scene(sel)
    assert V.selector_of(sc["params"]) == sel and sc["timestamps"].reshape(-1)[0] == V.T13
    (_, op, _, total), trace = _oracle_frame(oracle, sc, mode)
    iters, samples, stopped, see_through = V.frame_conditions(trace, op)
    print(f"sel {sel} {mode}: {iters} iterations, {samples} samples, {stopped:.1%} stopped, {see_through:.1%} see-through")
    assert samples == total
    assert iters >= 4 and samples >= 5000
    assert stopped >= 0.10 and see_through >= 0.10


@pytest.mark.parametrize("sel", V.TEMPORAL_SELS)
def test_time_reaches_the_table(oracle, sel):
    """Frames of one camera at float32(1/3) and 0.8 differ; for sel 4 and 6 (no time encoding) only the table's
    key-frames can make them"""
    sc = V.frame_scene(sel)
    (a, _, _, _), _ = _oracle_frame(oracle, sc, "f32", V.T13)
    (b, _, _, _), _ = _oracle_frame(oracle, sc, "f32", np.float32(0.8))
    assert np.abs(a - b).max() > 1e-2


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
@pytest.mark.parametrize("sel", V.TEMPORAL_SELS)
def test_three_times_three_schedules(oracle, sel, mode):
    sc = V.frame_scene(sel)
    schedules = []
    for t in (V.T13, np.float32(0.8), np.float32(1.0)):
        (_, op, _, total), trace = _oracle_frame(oracle, sc, mode, t)
        assert len(trace) >= 4 and total >= 5000
        schedules.append([(it["n_alive"], it["n_samples"], it["n_new"]) for it in trace])
    assert not (schedules[0] == schedules[1] == schedules[2])


@pytest.mark.parametrize("seed", range(200, 206))
def test_fuzz_seeds_produce_samples(oracle, seed):
    from test_gpu_parity import _fuzz_scene
    sc, cfg, rng = _fuzz_scene(seed)
    before = {k: np.copy(v) for k, v in sc.items() if isinstance(v, np.ndarray)}
    sel, mode = seed % 6 + 2, V.MODES[seed % 4]
    var = V.with_variant(sc, sel, seed=seed)
    assert V.selector_of(var["params"]) == sel and var["params"]["moving_step"] == sc["params"]["moving_step"]
    assert all(np.array_equal(var[k], v) for k, v in before.items())          # rays, grid and time are the seed's
    (_, op, _, total), trace = _oracle_frame(oracle, var, mode, max_samples=int(rng.choice([64, 300, 1024])))
    assert total > 500 and (op > 0).any()
