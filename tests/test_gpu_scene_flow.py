"""GPU suite: scene flow and optical flow (csrc/field_jacobian.hip: ced_field_velocity, ced_field_velocity_rays;
csrc/pixels.hip: ced_flow_to_rgb8) and what stands on them -- DNGPradianceField.query_scene_flow(_rays),
utils.render_scene_flow / render_optical_flow, cameras.pinhole_projector, video.render_video(scene_flow=, optical_flow=),
trainer --video_flow.

References (tests/flow64.py and tests/warp64.py, pinned on the CPU by tests/test_scene_flow_cpu.py): the header's guarded
velocity in numpy float32 on the device's own query_move_jacobian output, for the bits of the fused kernel; the float64
velocity of the mode-rounded float64 model, for what it promises; the stated sums rebuilt in torch from the returned
samples, for the maps.  Every bound is computed here from a model run in float32 and in float64, never from the kernel.

Inputs: those of tests/test_gpu_track.py -- rng 7, 4099 rows, aabb +-1.5, log2 table 15, moving steps 1/32 and 1/8; frames
of 16 x 16 rays on the toy scene of tests/test_gpu_deformation.py."""
import json
import os

import numpy as np
import pytest
import torch

import flow64 as F
import warp64 as W
from test_gpu_track import DEV, FLAGS, MODES, SIZES, STEP, N, T, _field, _inputs, _params
from test_gpu_warp_jacobian import COARSE, TABLES, _model

pytestmark = pytest.mark.gpu


# ---- 1. the fused kernel is the composition ----------------------------------------------------------------------------
def _check_composition(f, what, folds):
    from ced_nerf_amd import ops
    pos, t = _inputs()
    jac = f.query_move_jacobian(pos, t)[1]
    want = tuple(T(a) for a in F.velocity_f32(N(jac)))
    full = f.query_scene_flow(pos, t)
    for g, w, name in zip(full, want, ops.VELOCITY_OUTPUTS):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        assert torch.equal(g, w), (what, name, int((g != w).sum()))
    v, det, valid = full
    bad = int((~valid).sum())
    assert bool(torch.isfinite(v).all()) and not bool(v[~valid].any()) and float(v.abs().max()) > 1e-3
    if folds:
        assert 1 <= bad <= 0.02 * len(valid), (what, bad)
        assert bool((det[~valid] < 2.0 ** -20).all())
    else:
        assert bad == 0, (what, bad)
    for n in SIZES:                                                     # a row does not depend on n
        got = f.query_scene_flow(pos[:n], t[:n])
        assert got[0].shape == (n, 3) and got[1].shape == (n,) and got[2].shape == (n,) and got[2].dtype == torch.bool
        assert all(torch.equal(g, w[:n]) for g, w in zip(got, full)), (what, n)
    d = f._descriptor()
    for k in range(3):                                                  # each output alone
        only = ops.field_velocity(d, pos, t, want=tuple(i == k for i in range(3)))
        assert all((o is None) == (i != k) for i, o in enumerate(only)) and torch.equal(only[k], full[k]), (what, k)
    with pytest.raises(ValueError, match="no output"):
        ops.field_velocity(d, pos, t, want=(False, False, False))
    return bad


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("step", [STEP, COARSE])
@pytest.mark.parametrize("div,tm", FLAGS)
def test_velocity_is_the_composition_bit_for_bit(div, tm, step, mode):
    """query_scene_flow == the header's guarded solve in numpy float32 (flow64.velocity_f32) on the device's own
    query_move_jacobian output: v, det and valid with torch.equal, for every n of SIZES, each output alone.  Moving step
    1/8 folds: between one row and 2 % are not valid (float32 CPU model: 7 / 28 of 4099, fine offsets off / on), their v is
    exactly 0, v is finite everywhere; at 1/32 every row is valid.  Measured on an MI355X: 7 / 28 rows in every mode but f16
    with the fine offsets, 27."""
    bad = _check_composition(_field(div, tm, mode, step), (div, tm, step, mode), step == COARSE)
    print(f"composition [{mode} div={div} tm={tm} step={step:g}]: {bad} of {max(SIZES)} rows not valid")


@pytest.mark.parametrize("mode,table", TABLES)
def test_velocity_is_the_composition_on_the_other_tables(mode, table):
    """both f16x2 blob layouts (K = 32 placements on an fp16 table, pair form on a temporal one)"""
    _check_composition(_field(True, 0, mode, STEP, table), (mode, table), False)


# ---- 2. accuracy -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("div,tm", FLAGS)
def test_velocity_accuracy(div, tm, mode):
    """Step 1/32, rows kept by warp64.kept_rows (at most 2 % left out; CPU model: 0.63 %): query_scene_flow against the
    float64 velocity of the mode-rounded float64 model.  Bound: 4 x the largest difference between the header's lines on
    the model's float32 Jacobian and that float64 velocity, 8 x for f16 -- test_jacobian_accuracy's rule -- and likewise
    det.  CPU: the bound's base is 3.3e-7 / 4.3e-7 (fine offsets off / on, f32) at |v| <= 0.34.
    Measured on an MI355X, max |v - v64| on the kept rows (fine offsets off / on): f32 and f32+h16x2 8.2e-8 / 9.9e-8 against a
    base of 3.3e-7 / 4.1e-7, f16x2 7.7e-8 / 1.0e-7 (3.2e-7 / 4.3e-7), f16 9.8e-5 / 1.2e-4 (9.8e-5 / 1.2e-4); max |det - det64|:
    f32 3.3e-7 / 3.0e-7 (5.6e-7 / 7.1e-7), f16x2 3.0e-7 / 3.5e-7 (5.6e-7 / 7.8e-7), f16 5.4e-5 / 8.2e-5 (8.5e-5 / 1.4e-4)."""
    mm = W.MOTION_MODES[mode]
    f = _field(div, tm, mode)
    pos, t = _inputs()
    v, det, valid = f.query_scene_flow(pos, t)
    _, j64, pre = _model(div, tm, STEP, mm, "float64")
    _, j32, _ = _model(div, tm, STEP, mm, "float32")
    keep = W.kept_rows(pre)
    left_out = 1.0 - float(keep.mean())
    v64, det64 = W.velocity(j64)
    v32, det32, valid32 = F.velocity_f32(j32.astype(np.float32))
    factor = 8 if mm == "f16" else 4
    base_v, base_det = float(np.abs(v32 - v64)[keep].max()), float(np.abs(det32 - det64)[keep].max())
    err_v, err_det = float(np.abs(N(v) - v64)[keep].max()), float(np.abs(N(det) - det64)[keep].max())
    print(f"velocity [{mode} div={div} tm={tm}]: {100 * left_out:.2f} % of rows left out; max |v - v64| = {err_v:.3e} (bound "
          f"{factor} x {base_v:.3e}), max |det - det64| = {err_det:.3e} (bound {factor} x {base_det:.3e}), max |v| = "
          f"{float(np.abs(v64[keep]).max()):.3f}")
    assert left_out <= 0.02 and valid32.all() and bool(valid.all())
    assert err_v <= factor * base_v
    assert err_det <= factor * base_det


# ---- 3. the rays entry -------------------------------------------------------------------------------------------------
def _ray_samples(n_rays, n, seed=3):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-1.0, 1.0, size=(n_rays, 3)).astype(np.float32)
    d = rng.normal(size=(n_rays, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    ri = np.sort(rng.integers(0, n_rays, size=n)).astype(np.int64)
    t0 = rng.uniform(0.0, 2.0, size=n).astype(np.float32)
    t1 = (t0 + np.float32(0.02)).astype(np.float32)
    return rng, T(o), T(d), ri, T(t0), T(t1)


@pytest.mark.parametrize("mode,tm", [("f32", 2), ("f16", 2), ("f16x2", 0), ("f16x2", 2), ("f32+h16x2", 0)])
def test_rays_entry_is_the_points_entry_at_the_samples(mode, tm):
    """97 rays, 1 031 samples (a ragged last tile), per-ray timestamps (training mode) and one scalar (eval): all three
    outputs equal the points entry fed px = o + (d * (t0 + t1)) / 2.0f formed in torch fp32; a negative ray index is ray 0
    at distance 0; n_dev < n leaves the tail untouched"""
    from ced_nerf_amd import ops
    from ced_nerf_amd.utils import sample_positions
    n_rays, n = 97, 1031
    rng, O, Dd, ri, T0, T1 = _ray_samples(n_rays, n)
    neg = 517
    ri[neg] = -1
    RI = T(ri)
    used = RI.clamp(min=0)
    f = _field(True, tm, mode)
    pos = sample_positions(O, Dd, used, T0, T1)
    pos[neg] = O[0]
    for per_ray in (True, False):
        ts = T(rng.uniform(0.0, 1.0, size=(n_rays if per_ray else 1, 1)).astype(np.float32))
        f.train(per_ray)
        got = f.query_scene_flow_rays(O, Dd, RI, T0, T1, ts)
        f.eval()
        tq = ts.reshape(-1)[used] if per_ray else ts.reshape(-1)[:1].expand(n).contiguous()
        want = f.query_scene_flow(pos, tq)
        for g, w, name in zip(got, want, ops.VELOCITY_OUTPUTS):
            assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(g, w), (per_ray, name)
        assert bool(want[0].any())
        if not per_ray:
            only = f.query_scene_flow_rays(O, Dd, RI, T0, T1, ts, want=(False, True, False))
            assert only[0] is None and only[2] is None and torch.equal(only[1], want[1])
            keep = 700
            out = (torch.full((n, 3), 7.0, device=DEV), torch.full((n,), 7.0, device=DEV),
                   torch.ones((n,), device=DEV, dtype=torch.bool))
            want_tail = tuple(o[keep:].clone() for o in out)
            ops.field_velocity_rays(f._descriptor(), O, Dd, RI, T0, T1, ts.reshape(-1), False,
                                    n_dev=torch.tensor([keep], device=DEV, dtype=torch.int64), out=out)
            for g, w, tail in zip(out, want, want_tail):
                assert torch.equal(g[:keep], w[:keep]) and torch.equal(g[keep:], tail)
            with pytest.raises(ValueError, match="no output"):
                ops.field_velocity_rays(f._descriptor(), O, Dd, RI, T0, T1, ts.reshape(-1), False, want=(False, False, False))


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
def test_one_workgroup_walks_every_tile(mode):
    """4099 rows on a descriptor limited to one workgroup (8 waves, 33 rounds of tiles): the points and the rays entry
    give what the unlimited descriptor gives"""
    from ced_nerf_amd import ops
    f = _field(True, 2, mode)
    d, d1 = f._descriptor(), ops._with_workgroups(f._descriptor(), 1)
    pos, t = _inputs()
    full = ops.field_velocity(d, pos, t)
    assert all(torch.equal(g, w) for g, w in zip(ops.field_velocity(d1, pos, t), full))
    _, O, Dd, ri, T0, T1 = _ray_samples(97, max(SIZES), seed=5)
    ts = T(np.array([0.3], np.float32))
    rays = ops.field_velocity_rays(d, O, Dd, T(ri), T0, T1, ts, False)
    assert all(torch.equal(g, w) for g, w in zip(ops.field_velocity_rays(d1, O, Dd, T(ri), T0, T1, ts, False), rays))
    assert bool(rays[0].any())


# ---- 4. render_scene_flow ----------------------------------------------------------------------------------------------
FW = FH = 16
FOCAL = 0.5 * FW / np.tan(0.5 * 0.69)
K16 = np.array([[FOCAL, 0.0, FW / 2.0], [0.0, FOCAL, FH / 2.0], [0.0, 0.0, 1.0]], np.float32)


def _frame_setup(levels=1, azim=30.0):
    """test_render_normals_samples_weights_and_normals' toy scene and occupancy, seen through a 16 x 16 pinhole camera"""
    from ced_nerf_amd import cameras, synthetic as S
    from ced_nerf_amd.nerfacc_api import OccGridEstimator
    from test_gpu_deformation import AABB, _field as toy_field, _params as toy_params
    binaries = S.make_occupancy(AABB, resolution=32, levels=levels)
    params = toy_params("trained", True, 2, "f32", tuple(S.enlarge_aabb(AABB, 2 ** (levels - 1)).tolist()))
    f = toy_field(params, "f32")
    est = OccGridEstimator(AABB, 32, levels).to(DEV)
    est.set_binaries(T(binaries))
    est.occs = torch.full_like(est.occs, 1.0)                  # nerfacc clamps alpha_thre to occs.mean()
    c2w = S.look_at_c2w(4.0, 30.0, azim)
    return f, est, cameras.pinhole_rays(K16, c2w, FW, FH, device=DEV), c2w


def test_render_scene_flow_samples_weights_and_flow():
    """the sample set, the weights and the opacity are render_motion's; flow3d and coverage are accumulate_along_rays of
    the returned samples; velocity / det / valid are the rays entry's; coverage <= opacity, equal where every sample of the
    ray is valid; test_chunk_size=64 gives the same images; a frame that misses gives zeros; render_motion and
    render_normals return the bits they returned before the helper carried a fourth channel"""
    from ced_nerf_amd.nerfacc_api import _packed_info_from, accumulate_along_rays
    from ced_nerf_amd.utils import render_motion, render_normals, render_scene_flow
    from test_gpu_deformation import RENDER
    for levels, cone, alpha in ((1, 0.0, 0.0), (2, 0.004, 1e-2)):
        f, est, rays, _ = _frame_setup(levels)
        ts = T(np.array([[0.4]], np.float32))
        kw = dict(RENDER, cone_angle=cone, alpha_thre=alpha)
        motion, m_opacity, m_samples, ms = render_motion(f, est, rays, timestamps=ts, return_samples=True, **kw)
        normals = render_normals(f, est, rays, timestamps=ts, **kw)
        flow, opacity, coverage, n_samples, samples = render_scene_flow(f, est, rays, timestamps=ts, return_samples=True, **kw)
        assert flow.shape == (FH, FW, 3) and opacity.shape == coverage.shape == (FH, FW, 1)
        assert n_samples == m_samples > 50 and torch.equal(opacity, m_opacity) and len(samples) == len(ms) == 1
        s = samples[0]
        assert set(s) == {"ray_indices", "t_starts", "t_ends", "weights", "velocity", "det", "valid"}
        for k in ("ray_indices", "t_starts", "t_ends", "weights"):
            assert torch.equal(s[k], ms[0][k]), k
        packed = _packed_info_from(s["ray_indices"], FH * FW)
        assert torch.equal(flow.reshape(-1, 3), accumulate_along_rays(s["weights"], values=s["velocity"], packed_info=packed))
        assert torch.equal(coverage.reshape(-1, 1),
                           accumulate_along_rays(s["weights"], values=s["valid"].float()[:, None], packed_info=packed))
        O, Dd = rays.origins.reshape(-1, 3), rays.viewdirs.reshape(-1, 3)
        direct = f.query_scene_flow_rays(O, Dd, s["ray_indices"], s["t_starts"], s["t_ends"], ts)
        assert all(torch.equal(s[k], w) for k, w in zip(("velocity", "det", "valid"), direct)) and bool(s["velocity"].any())
        assert bool((coverage <= opacity).all()) and bool(torch.isfinite(flow).all())
        all_valid = torch.ones(FH * FW, device=DEV, dtype=torch.bool)
        all_valid[s["ray_indices"][~s["valid"]]] = False
        assert torch.equal(coverage.reshape(-1)[all_valid], opacity.reshape(-1)[all_valid])
        print(f"render_scene_flow [levels={levels}]: {n_samples} samples, {int((~s['valid']).sum())} not valid, "
              f"{int((~all_valid).sum())} pixels with coverage < opacity, max |flow3d| = {float(flow.abs().max()):.3e}")
        miss = opacity.reshape(-1) == 0
        assert 0 < int(miss.sum()) < FH * FW and not bool(flow.reshape(-1, 3)[miss].any()) and not bool(coverage.reshape(-1)[miss].any())
        f2, o2, c2, n2, s2 = render_scene_flow(f, est, rays, timestamps=ts, return_samples=True, test_chunk_size=64, **kw)
        assert n2 == n_samples and torch.equal(f2, flow) and torch.equal(o2, opacity) and torch.equal(c2, coverage)
        assert len(s2) == FH * FW // 64 and torch.equal(torch.cat([c["velocity"] for c in s2]), s["velocity"])
        # the three-channel maps after the helper has carried four
        again = render_motion(f, est, rays, timestamps=ts, return_samples=True, **kw)
        assert torch.equal(again[0], motion) and torch.equal(again[1], m_opacity) and again[2] == m_samples
        assert set(again[3][0]) == {"ray_indices", "t_starts", "t_ends", "weights", "move"}
        assert all(torch.equal(again[3][0][k], ms[0][k]) for k in ms[0])
        n_again = render_normals(f, est, rays, timestamps=ts, **kw)
        assert len(n_again) == 3 and torch.equal(n_again[0], normals[0]) and torch.equal(n_again[1], normals[1]) and n_again[2] == normals[2]
    away = type(rays)(rays.origins, -rays.viewdirs)
    flow, opacity, coverage, n_samples, samples = render_scene_flow(f, est, away, timestamps=ts, return_samples=True, **RENDER)
    assert n_samples == 0 and flow.shape == (FH, FW, 3) and not bool(flow.any()) and not bool(opacity.any()) and not bool(coverage.any())
    assert len(samples) == 1 and samples[0]["velocity"].shape == (0, 3) and samples[0]["valid"].shape == (0,)


# ---- 5. render_optical_flow --------------------------------------------------------------------------------------------
def test_render_optical_flow_is_the_stated_sum():
    """flow2d = sum_i w_i ok_i (project(x_i + dt v_i) - project(x_i)), ok_i = valid_i and both in front, rebuilt in torch
    from the returned samples and the projector; coverage counts ok; the samples are render_scene_flow's; with dt = 0 the
    flow is exactly 0 and coverage == opacity"""
    from ced_nerf_amd import cameras
    from ced_nerf_amd.nerfacc_api import _packed_info_from, accumulate_along_rays
    from ced_nerf_amd.utils import render_optical_flow, render_scene_flow, sample_positions
    from test_gpu_deformation import RENDER
    f, est, rays, c2w = _frame_setup(1)
    ts = T(np.array([[0.4]], np.float32))
    project = cameras.pinhole_projector(K16, c2w, device=DEV)
    dt = 0.05
    flow, opacity, coverage, n_samples, samples = render_optical_flow(f, est, rays, project, dt, timestamps=ts,
                                                                      return_samples=True, **RENDER)
    f3, o3, c3, n3, s3 = render_scene_flow(f, est, rays, timestamps=ts, return_samples=True, **RENDER)
    assert flow.shape == (FH, FW, 2) and opacity.shape == coverage.shape == (FH, FW, 1) and n_samples == n3 > 100
    s = samples[0]
    assert set(s) == set(s3[0]) | {"flow", "ok"} and all(torch.equal(s[k], s3[0][k]) for k in s3[0]) and torch.equal(opacity, o3)
    O, Dd = rays.origins.reshape(-1, 3), rays.viewdirs.reshape(-1, 3)
    x = sample_positions(O, Dd, s["ray_indices"], s["t_starts"], s["t_ends"])
    assert torch.equal(x, O[s["ray_indices"]] + (Dd[s["ray_indices"]] * (s["t_starts"] + s["t_ends"])[:, None]) / 2.0)
    p0, in0 = project(x)
    p1, in1 = project(x + dt * s["velocity"])
    ok = s["valid"] & in0 & in1
    disp = torch.where(ok[:, None], p1 - p0, torch.zeros((), device=DEV))
    packed = _packed_info_from(s["ray_indices"], FH * FW)
    assert torch.equal(s["ok"], ok) and torch.equal(s["flow"], disp)
    assert torch.equal(flow.reshape(-1, 2), accumulate_along_rays(s["weights"], values=disp, packed_info=packed))
    assert torch.equal(coverage.reshape(-1, 1), accumulate_along_rays(s["weights"], values=ok.float()[:, None], packed_info=packed))
    assert bool(in0.all()) and bool((coverage <= opacity).all()) and bool(torch.isfinite(flow).all()) and float(flow.abs().max()) > 1e-4
    # the pixel a sample projects to is its ray's own, so the expected flow is a displacement from the pixel's centre
    pix = torch.stack([s["ray_indices"] % FW, s["ray_indices"] // FW], -1).float()
    print(f"render_optical_flow: {n_samples} samples, {int((~ok).sum())} not ok, max |project(x_i) - pixel| = "
          f"{float((p0 - pix).abs().max()):.3e}, max |flow2d| = {float(flow.abs().max()):.3e} px per dt = {dt}")
    assert float((p0 - pix).abs().max()) <= 1e-3
    still, o0, c0, _ = render_optical_flow(f, est, rays, project, 0.0, timestamps=ts, **RENDER)
    assert not bool(still.any()) and torch.equal(o0, opacity) and torch.equal(c0, o0)


@pytest.mark.parametrize("opengl", [True, False])
def test_projector_round_trip_on_device_rays(opengl):
    """cameras.pinhole_rays of a 16 x 16 camera, points o + s * d (s = 0.5, 4) in torch fp32, projected on the device:
    within 4 x the error of the same formula in numpy float32 against float64 on the same points (printed: both, and the
    round trip against the pixel indices)"""
    from ced_nerf_amd import cameras, synthetic as S
    c2w = S.look_at_c2w(4.0, 30.0, 20.0, opengl=opengl)
    rays = cameras.pinhole_rays(K16, c2w, FW, FH, opengl=opengl, device=DEV)
    project = cameras.pinhole_projector(K16, c2w, opengl=opengl, device=DEV)
    O, Dd = rays.origins.reshape(-1, 3), rays.viewdirs.reshape(-1, 3)
    idx = np.stack(np.meshgrid(np.arange(FW), np.arange(FH), indexing="xy"), -1).reshape(-1, 2).astype(np.float64)
    for s in (0.5, 4.0):
        pts = O + s * Dd
        pixels, front = project(pts)
        assert pixels.dtype == torch.float32 and bool(front.all()) and not bool(project(O - s * Dd)[1].any())
        p64, _ = F.pinhole_project(K16, c2w, opengl, N(pts), np.float64)
        p32, _ = F.pinhole_project(K16, c2w, opengl, N(pts), np.float32)
        base = float(np.abs(p32 - p64).max())
        err = float(np.abs(N(pixels) - p64).max())
        trip, trip64 = float(np.abs(N(pixels) - idx).max()), float(np.abs(p64 - idx).max())
        print(f"projector [opengl={opengl}] s = {s}: max |device - float64| = {err:.3e} (numpy float32 against float64: {base:.3e}); "
              f"round trip against the pixel index: device {trip:.3e}, float64 formula on the same points {trip64:.3e}")
        assert err <= 4 * base
        assert trip <= 4 * base + trip64


# ---- 6. colour ---------------------------------------------------------------------------------------------------------
def test_flow_to_rgb8_against_the_numpy_model():
    """a 16 x 16 field with zero, saturated, NaN and infinite pixels: at most 1 off per channel (the device's atan2f may
    round across a boundary), exact on the known answers, mirrored by flip_w as frame_to_rgb8 mirrors"""
    from ced_nerf_amd import ops
    rng = np.random.default_rng(9)
    m = 3.0
    flow = rng.normal(scale=2.0, size=(16, 16, 2)).astype(np.float32)
    flow[0, 0] = [0.0, 0.0]
    flow[0, 1] = [m, 0.0]
    flow[0, 2] = [5 * m, 0.0]
    flow[0, 3] = [np.nan, 1.0]
    flow[0, 4] = [1.0, -np.inf]
    flow[0, 5] = [m / 2, 0.0]
    for flip in (False, True):
        got = N(ops.flow_to_rgb8(T(flow), m, flip_w=flip))
        want = F.flow_rgb8(flow, m, flip_w=flip)
        assert got.dtype == np.uint8 and got.shape == (16, 16, 3)
        diff = np.abs(got.astype(int) - want.astype(int))
        print(f"flow_to_rgb8 [flip_w={flip}]: {int((diff > 0).sum())} of {diff.size} channels differ from the numpy model, max {int(diff.max())}")
        assert diff.max() <= 1
        row = got[0, ::-1] if flip else got[0]
        assert row[:6].tolist() == [[255, 255, 255], [255, 0, 0], [255, 0, 0], [0, 0, 0], [0, 0, 0], [255, 127, 127]]
    plain, flipped = ops.flow_to_rgb8(T(flow), m, flip_w=False), ops.flow_to_rgb8(T(flow), m, flip_w=True)
    assert torch.equal(flipped, plain.flip(1))
    rgb = torch.rand(16, 16, 3, device=DEV)
    assert torch.equal(ops.frame_to_rgb8(rgb, flip_w=True), ops.frame_to_rgb8(rgb, flip_w=False).flip(1))
    with pytest.raises(ValueError, match="max_mag"):
        ops.flow_to_rgb8(T(flow), 0.0)
    with pytest.raises(ValueError, match=r"\[H,W,2\]"):
        ops.flow_to_rgb8(T(flow[..., :1].copy()), 1.0)


# ---- 7. video and command line -----------------------------------------------------------------------------------------
def test_render_video_flow_maps():
    """render_video(scene_flow=True, optical_flow=(projector_of_frame, dt)) on 3 frames: every frame's scene_flow_f32,
    flow_f32 and flow_coverage_f32 equal the direct calls on the frame's rays and time; rgb, depth and n_samples are those
    of a run without the flags"""
    from ced_nerf_amd import cameras, synthetic as S
    from ced_nerf_amd.utils import render_optical_flow, render_scene_flow
    from ced_nerf_amd.video import render_video
    from test_gpu_deformation import RENDER
    f, est, _, _ = _frame_setup(1)
    poses = [S.look_at_c2w(4.0, 30.0, 20.0 + 25.0 * k) for k in range(3)]
    rays_of = lambda i: cameras.pinhole_rays(K16, poses[i], FW, FH, device=DEV)
    projector_of = lambda i: cameras.pinhole_projector(K16, poses[i], device=DEV)
    times = [torch.tensor([[0.1 + 0.3 * k]], device=DEV) for k in range(3)]
    rk = dict(RENDER, cone_angle=0.0, alpha_thre=0.0)
    dt = 0.04
    plain = render_video(f, est, rays_of, lambda i: times[i], 3, max_samples=256, render_kwargs=rk)
    assert all(set(fr) == {"rgb", "depth", "n_samples"} for fr in plain)
    frames = render_video(f, est, rays_of, lambda i: times[i], 3, max_samples=256, render_kwargs=rk, scene_flow=True,
                          optical_flow=(projector_of, dt))
    torch.cuda.synchronize()
    assert all(set(fr) == {"rgb", "depth", "n_samples", "scene_flow_f32", "flow_f32", "flow_coverage_f32"} for fr in frames)
    for i, (fr, pl) in enumerate(zip(frames, plain)):
        want3 = render_scene_flow(f, est, rays_of(i), timestamps=times[i], **rk)[0]
        want2, _, cov, _ = render_optical_flow(f, est, rays_of(i), projector_of(i), dt, timestamps=times[i], **rk)
        assert fr["scene_flow_f32"].shape == (FH, FW, 3) and torch.equal(fr["scene_flow_f32"], want3) and bool(want3.any())
        assert fr["flow_f32"].shape == (FH, FW, 2) and torch.equal(fr["flow_f32"], want2) and bool(want2.any())
        assert torch.equal(fr["flow_coverage_f32"], cov)
        assert torch.equal(fr["rgb"], pl["rgb"]) and torch.equal(fr["depth"], pl["depth"]) and fr["n_samples"] == pl["n_samples"]
    assert not torch.equal(frames[0]["flow_f32"], frames[1]["flow_f32"])


def test_cli_writes_flow_frames(tmp_path):
    """trainer --load_model ... --render_video DIR --video_flow --video_frames 2 on a toy D-NeRF folder (a transforms file
    and three 16 x 12 RGBA views): two flow_*.png of the frame's size beside the rgb and depth frames"""
    Image = pytest.importorskip("PIL.Image")
    from ced_nerf_amd import synthetic as S, trainer
    width, height = 16, 12
    scene = tmp_path / "data" / "toy"
    rng = np.random.default_rng(2)
    for split in ("train", "test"):
        (scene / split).mkdir(parents=True)
        frames = []
        for i in range(3):
            Image.fromarray(rng.integers(0, 256, size=(height, width, 4), dtype=np.uint8), "RGBA").save(scene / split / f"r_{i:03d}.png")
            m = np.eye(4)
            m[:3] = S.look_at_c2w(4.0, 30.0, 40.0 * i)
            frames.append({"file_path": f"./{split}/r_{i:03d}", "time": i / 2.0, "transform_matrix": m.tolist()})
        (scene / f"transforms_{split}.json").write_text(json.dumps({"camera_angle_x": 0.69, "frames": frames}))
    cfg = trainer.resolve_config("dnerf", None, log2_hashmap_size=12)
    field, est = trainer.build_modules(cfg, torch.device(DEV), use_div_offsets=True)
    est.set_binaries(T(np.random.default_rng(4).uniform(size=tuple(est.binaries.shape)) < 0.5))
    ckpt = str(tmp_path / "model.pth")
    torch.save({"radiance_field": field.state_dict(), "occupancy_grid": est.state_dict()}, ckpt)
    out = tmp_path / "frames"
    argv = ["--data_root", str(tmp_path / "data"), "--scene", "toy", "--dataset", "dnerf", "--log2_hashmap_size", "12", "-df",
            "--load_model", ckpt, "--render_video", str(out), "--video_frames", "2"]
    assert trainer.main(argv + ["--video_flow", "--video_flow_max", "2.5"]) == 0
    names = sorted(os.listdir(out))
    assert names == [f"{kind}_{i:04d}.png" for kind in ("depth", "flow", "rgb") for i in range(2)]
    for n in names:
        with Image.open(out / n) as im:
            assert im.size == (width, height) and im.mode == ("L" if n.startswith("depth") else "RGB"), n
    plain = tmp_path / "plain"
    assert trainer.main(argv[:-4] + ["--render_video", str(plain), "--video_frames", "2"]) == 0
    assert sorted(os.listdir(plain)) == [n for n in names if not n.startswith("flow")]
    for n in os.listdir(plain):
        assert open(plain / n, "rb").read() == open(out / n, "rb").read(), n


def test_cli_refuses_flow_for_distorted_cameras(tmp_path, capsys):
    """a HyperNeRF folder has distorted cameras and no projector: --video_flow exits with a message before anything is
    loaded or trained; --video_flow without --render_video is a usage error"""
    pytest.importorskip("PIL.Image")
    import scene_toys as toys
    from ced_nerf_amd import trainer
    toys.make_hypernerf_toy(tmp_path / "data", "vrig_chicken", png=True)
    common = ["--data_root", str(tmp_path / "data"), "--scene", "vrig_chicken", "--load_model", str(tmp_path / "none.pth")]
    with pytest.raises(SystemExit) as e:
        trainer.main(common + ["--render_video", str(tmp_path / "v"), "--video_flow"])
    assert e.value.code == 2 and "no projector is built" in capsys.readouterr().err and not os.path.exists(tmp_path / "v")
    with pytest.raises(SystemExit) as e:
        trainer.main(common + ["--video_flow"])
    assert e.value.code == 2 and "--render_video" in capsys.readouterr().err
