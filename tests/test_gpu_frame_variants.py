"""Every field kernel inside the frame renderers: the eight table / time variants of tests/field_variants.py (the
launchers' selector, sel = time encoding | fp16 table << 1 | temporal table << 2) times the four arithmetic modes, on
40x30 frames, against the CPU oracle's mode of the same name -- schedule, totals, rgb and depth bit for bit, opacity
within the frame fuzz's 1e-6.

  test_render_image_test        sel 0..7 x {f32, f16x2, f16, f32+h16x2}: all 32 kernels through ced_render_image_test
                                (FrameTracer against the oracle's trace) and through the staged Python loop
  test_render_frames_test       sel 4..7 x {f32, f16x2}: three frames of one camera at t = float32(1/3), 0.8 and 1 in one
                                call; the time is handed to the field kernel per ray there, and it picks the key-frames
  test_render_image             sel 3, 4, 7, each mode once: image.hip (sample -> visibility -> render)
  test_native_sampling          sel 7: OccGridEstimator.sampling on the native visibility pass, per-ray times
  test_fuzz_table_variants      six more seeds of tests/test_gpu_parity.py's _fuzz_scene with sel = seed % 6 + 2

The frame scenes (field_variants.frame_scene) are HyperNeRF-shaped with the density row of mlp_base scaled per variant;
tests/test_field_variants_cpu.py holds them to at least 4 iterations, 5000 samples, 10 % of the pixels ended by the early
stop and 10 % see-through, in every mode used here, with the oracle alone."""
import numpy as np
import pytest
import torch

import field_variants as V
from conftest import assert_bitexact
from test_gpu_parity import N, T, _fuzz_scene, _setup

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAX_SAMPLES = 1024


def _in_mode(oracle, sc, mode):
    """test_gpu_parity._setup with both fields in arithmetic mode `mode`"""
    of, oest, f, est, rays, rk = _setup(oracle, sc)
    if mode != "f32":
        of = oracle.OracleField(sc["params"], mlp_half=mode)
        f.set_mlp_precision(mode)
    return of, oest, f, est, rays, rk


def _oracle_frame(oracle, of, oest, sc, max_samples=MAX_SAMPLES, timestamps=None):
    trace = []
    ts = sc["timestamps"] if timestamps is None else timestamps
    w = oracle.render_image_test(max_samples, of, oest, sc["origins"], sc["viewdirs"], timestamps=ts, trace=trace,
                                 **sc["render"])
    return w, [dict(n_alive=t["n_alive"], n_samples=t["n_samples"], n_new=t["n_new"]) for t in trace]


def _assert_frame(got, want, what):
    rgb, op, dp, total = got
    w_rgb, w_op, w_dp, w_total = want
    assert total == w_total, (what, total, w_total)
    assert_bitexact(N(rgb), w_rgb, f"rgb ({what})")
    assert_bitexact(N(dp), w_dp, f"depth ({what})")
    assert np.abs(N(op) - w_op).max() <= 1e-6, what


@pytest.mark.parametrize("mode", V.MODES)
@pytest.mark.parametrize("sel", V.SELS)
def test_render_image_test(oracle, sel, mode):
    from ced_nerf_amd import ops
    from ced_nerf_amd.utils import render_image_test, render_image_test_staged
    sc = V.frame_scene(sel)
    of, oest, f, est, rays, rk = _in_mode(oracle, sc, mode)
    want, want_iters = _oracle_frame(oracle, of, oest, sc)
    what = f"sel {sel} {mode}"
    tracer = ops.FrameTracer(capacity=1100, with_events=False)
    got = render_image_test(MAX_SAMPLES, f, est, rays, timestamps=T(sc["timestamps"]), tracer=tracer, **rk)
    assert tracer.iterations() == want_iters, what
    assert got[0].shape == (V.FRAME_H, V.FRAME_W, 3) and got[1].shape == (V.FRAME_H, V.FRAME_W, 1)
    _assert_frame(got, want, what)
    s_rgb, s_op, s_dp, s_total = render_image_test_staged(MAX_SAMPLES, f, est, rays, timestamps=T(sc["timestamps"]), **rk)
    assert s_total == got[3], what
    assert_bitexact(N(s_rgb), N(got[0]), f"staged vs native rgb ({what})")
    assert_bitexact(N(s_op), N(got[1]), f"staged vs native opacity ({what})")
    assert_bitexact(N(s_dp), N(got[2]), f"staged vs native depth ({what})")


FRAME_TIMES = [V.T13, np.float32(0.8), np.float32(1.0)]


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
@pytest.mark.parametrize("sel", V.TEMPORAL_SELS)
def test_render_frames_test(oracle, sel, mode):
    """One camera at three times in one ced_render_frames_test call: every frame is the frame rendered alone -- and the
    oracle's -- and the three schedules differ, which only the table's key-frames can make them do when sel has no time
    encoding"""
    from ced_nerf_amd import ops
    from ced_nerf_amd.utils import Rays, render_frames_test, render_image_test
    sc = V.frame_scene(sel)
    of, oest, f, est, rays, rk = _in_mode(oracle, sc, mode)
    alone, schedules = [], []
    for t in FRAME_TIMES:
        ts = np.array([[t]], np.float32)
        want, want_iters = _oracle_frame(oracle, of, oest, sc, timestamps=ts)
        tracer = ops.FrameTracer(capacity=1100, with_events=False)
        got = render_image_test(MAX_SAMPLES, f, est, rays, timestamps=T(ts), tracer=tracer, **rk)
        assert tracer.iterations() == want_iters, (sel, mode, t)
        _assert_frame(got, want, f"sel {sel} {mode} t={t}")
        alone.append(got)
        schedules.append(want_iters)
    assert not (schedules[0] == schedules[1] == schedules[2])
    stack = Rays(torch.stack([rays.origins] * 3), torch.stack([rays.viewdirs] * 3))
    ts = T(np.asarray(FRAME_TIMES, np.float32))
    for _ in range(2):                                             # the workspace is reused: no state may leak
        rgb, op, dp, totals = render_frames_test(MAX_SAMPLES, f, est, stack, timestamps=ts, **rk)
        torch.cuda.synchronize()
        assert rgb.shape == (3, V.FRAME_H, V.FRAME_W, 3) and len(totals) == 3
        for k in range(3):
            assert totals[k] == alone[k][3], (k, totals, [a[3] for a in alone])
            assert torch.equal(rgb[k], alone[k][0]) and torch.equal(op[k], alone[k][1]) and torch.equal(dp[k], alone[k][2])


@pytest.mark.parametrize("sel,mode", [(3, "f32"), (4, "f16"), (7, "f16x2"), (7, "f32+h16x2")])
def test_render_image(oracle, sel, mode):
    """image.hip: sampling, the visibility filter on the field's density, rendering of the survivors"""
    from ced_nerf_amd.utils import render_image
    sc = V.frame_scene(sel)
    of, oest, f, est, rays, rk = _in_mode(oracle, sc, mode)
    w = oracle.render_image(of, oest, sc["origins"], sc["viewdirs"], timestamps=sc["timestamps"], **sc["render"])
    g = render_image(f, est, rays, timestamps=T(sc["timestamps"]), **rk)
    assert g[3] == w[3] and 1000 < w[3] < w[5], (sel, mode, g[3], w[3], w[5])     # the filter removed something
    for i, nm in enumerate(("colors", "opacities", "depths")):
        assert_bitexact(N(g[i]), w[i], f"{nm} (sel {sel} {mode})")


def test_native_sampling(oracle):
    """OccGridEstimator.sampling as the training step calls it (stratified near planes, per-ray times) with a temporal
    fp16 table: the native visibility pass returns the survivors of the filter over every marched sample"""
    from ced_nerf_amd.nerfacc_api import OccGridEstimator
    from ced_nerf_amd.train import TrainableField
    sc = V.frame_scene(7)
    cfg = sc["cfg"]
    est = OccGridEstimator(cfg["aabb"], cfg["grid_resolution"], cfg["grid_levels"]).to(DEV)
    est.set_binaries(T(sc["binaries"]))
    fused = TrainableField(sc["params"], DEV).shared_inference()
    fused.train()
    o = T(sc["origins"]).reshape(-1, 3).contiguous(); d = T(sc["viewdirs"]).reshape(-1, 3).contiguous()
    ts_np = V.sample_times(o.shape[0], np.random.default_rng(4))
    assert set(V.keyframe_interval(ts_np[:64]).tolist()) == {0, 1, 2}
    ts = T(ts_np.reshape(-1, 1))

    def sigma_fn(t_starts, t_ends, ray_indices):
        return fused.query_rays(o, d, ray_indices, t_starts, t_ends, ts, want_rgb=False)[1]

    kw = dict(sigma_fn=sigma_fn, near_plane=cfg["near_plane"], far_plane=cfg["far_plane"],
              render_step_size=cfg["render_step_size"], stratified=True, cone_angle=cfg["cone_angle"],
              alpha_thre=cfg["alpha_thre"])
    torch.manual_seed(9)
    a = est.sampling(o, d, sigma_field=(fused, ts, True), **kw)
    torch.manual_seed(9)
    b = est.sampling(o, d, **kw)
    marched = est._march_totals[o.shape[0]]
    assert 1000 < b[0].numel() < marched                          # the filter removed something, and not everything
    for x, y, nm in zip(a, b, ("ray_indices", "t_starts", "t_ends")):
        assert x.dtype == y.dtype and torch.equal(x, y), nm
    torch.manual_seed(9)
    c = est.sampling(o, d, sigma_field=(fused, ts, True), **kw)   # the second batch of a size marches in one pass
    for x, y, nm in zip(c, b, ("ray_indices", "t_starts", "t_ends")):
        assert torch.equal(x, y), nm


@pytest.mark.parametrize("seed", range(200, 206))
def test_fuzz_table_variants(oracle, seed):
    """tests/test_gpu_parity.py's fuzz with the table type varied too: the variant and the mode come from the seed
    number, not from the scene's generator, so the scenes of the existing seeds stay what they are"""
    from ced_nerf_amd import ops
    from ced_nerf_amd.utils import render_image_test
    sc, cfg, rng = _fuzz_scene(seed)
    sel, mode = seed % 6 + 2, V.MODES[seed % 4]
    sc = V.with_variant(sc, sel, seed=seed)
    of, oest, f, est, rays, rk = _in_mode(oracle, sc, mode)
    max_samples = int(rng.choice([64, 300, 1024]))
    want, want_iters = _oracle_frame(oracle, of, oest, sc, max_samples)
    tracer = ops.FrameTracer(capacity=1100, with_events=False)
    got = render_image_test(max_samples, f, est, rays, timestamps=T(sc["timestamps"]), tracer=tracer, **rk)
    assert tracer.iterations() == want_iters, (cfg, sel, mode)
    _assert_frame(got, want, f"{cfg} sel {sel} {mode}")
