"""CPU suite: scene flow and optical flow -- the numpy models of the GPU suite (tests/flow64.py) pinned against
tests/warp64.py, the pinhole projector against the reference's ray formula in float64, the colour wheel's known answers, and
the Python layer's refusals.  No kernel is launched here."""
import functools

import numpy as np
import pytest
import torch

import flow64 as F
import warp64 as W

AABB = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
STEP, COARSE = 1.0 / 32, 1.0 / 8
FLAGS = [(False, 0), (True, 2)]
ENTRIES = ("ced_field_velocity", "ced_field_velocity_rays", "ced_flow_to_rgb8")


@functools.lru_cache(maxsize=None)
def _params(div, tm, step):
    """tests/test_gpu_track.py's fields"""
    from ced_nerf_amd import synthetic as S
    return S.init_field_params(list(AABB), step, hash_max_res=256, log2_hashmap_size=15, use_div_offsets=div,
                               use_time_embedding=tm != 0, use_time_attenuation=tm == 2, regime="trained")


@functools.lru_cache(maxsize=None)
def _model(div, tm, step, dtype):
    pos, t = F.inputs()
    return W.move_jacobian(_params(div, tm, step), pos, t, np.dtype(dtype).type)


def _cpu_field():
    from ced_nerf_amd import synthetic as S
    from ced_nerf_amd.model import DNGPradianceField
    p = S.init_field_params([-1, -1, -1, 1, 1, 1], 1.0 / 32, 256, 10, use_div_offsets=True)
    return DNGPradianceField.from_params(p, "cpu").eval()


# ---- 1. the guard rule -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [STEP, COARSE])
@pytest.mark.parametrize("div,tm", FLAGS)
def test_guarded_velocity_is_the_newton_solve_on_the_time_column(div, tm, step):
    """velocity_f32(J) == -newton_step_f32(J, J[..., 3]) bit for bit on the rows it reports valid; 0 elsewhere; valid ==
    det >= 2^-20 and finite.  At step 1/8 the rows fold (float32 model: 7 / 28 of 4099 rows with det < 2^-20, fine
    offsets off / on), at 1/32 none does."""
    J = _model(div, tm, step, "float32")[1].astype(np.float32)
    v, det, valid = F.velocity_f32(J)
    want = -W.newton_step_f32(J, np.ascontiguousarray(J[:, :, 3]))
    assert v.dtype == det.dtype == np.float32 and valid.dtype == bool
    assert np.array_equal(v[valid], want[valid])
    assert not v[~valid].any() and np.isfinite(v).all()
    assert np.array_equal(det, W.gradient_inverse(J)[2])
    assert np.array_equal(valid, det >= np.float32(2.0 ** -20))         # no quotient overflows at these magnitudes
    bad = int((~valid).sum())
    print(f"guard [div={div} tm={tm} step={step:g}]: {bad} of {len(valid)} rows not valid, min det {float(det.min()):.3e}")
    if step == STEP:
        assert bad == 0
    else:
        assert 1 <= bad <= 0.02 * len(valid)


def test_guard_on_folds_infinities_and_nans():
    """a reflection (det = -1) passes the Newton step's |det| test but is a fold; det = 0, a NaN and an overflowing
    quotient are not valid either; the identity warp with d move / dt = (1, 2, 3) moves at (-1, -2, -3)"""
    J = np.zeros((5, 3, 4), np.float32)
    J[:, :, 3] = [1.0, 2.0, 3.0]
    J[1, 0, 0] = -2.0                                                   # A = diag(-1, 1, 1)
    J[2, 0, 0] = -1.0                                                   # singular
    J[3, 1, 2] = np.nan
    J[4, :, 3] = 3e38
    J[4, 0, 0] = J[4, 1, 1] = J[4, 2, 2] = -0.99                        # det = 1e-6 >= 2^-20, the quotient overflows
    v, det, valid = F.velocity_f32(J)
    assert valid.tolist() == [True, False, False, False, False]
    assert np.array_equal(v[0], np.float32([-1.0, -2.0, -3.0])) and not v[1:].any()
    assert det[0] == 1.0 and det[1] == -1.0 and det[2] == 0.0 and np.isnan(det[3]) and det[4] >= np.float32(2.0 ** -20)
    newton = W.newton_step_f32(J[1:2], np.ascontiguousarray(J[1:2, :, 3]))
    assert np.array_equal(newton[0], np.float32([-1.0, 2.0, 3.0]))      # the Newton step does divide by det = -1


# ---- 2. the float64 velocity -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("div,tm", FLAGS)
def test_velocity_model_against_float64(div, tm):
    """Step 1/32, kept rows: velocity_f32 on the float32 Jacobian equals warp64.velocity on the SAME Jacobian in float64
    within what rounding the header's lines in float32 can cost (flow64.velocity_rounding_bound: 8 u per line on the
    absolute sums; here at most 2.8e-7 / 3.3e-7 on |v| <= 0.34, measured 5.0e-8 / 4.5e-8), and likewise det."""
    _, j32, pre = _model(div, tm, STEP, "float32")
    j32 = j32.astype(np.float32)
    keep = W.kept_rows(pre)
    assert 1.0 - keep.mean() <= 0.02
    v, det, valid = F.velocity_f32(j32)
    v64, det64 = W.velocity(j32.astype(np.float64))
    e_v, e_det = F.velocity_rounding_bound(j32)
    err_v, err_det = np.abs(v - v64), np.abs(det - det64)
    print(f"velocity model [div={div} tm={tm}]: max |v32 - v64| = {err_v[keep].max():.3e} (bound up to {e_v[keep].max():.3e}), "
          f"max |det32 - det64| = {err_det[keep].max():.3e} (bound up to {e_det[keep].max():.3e}), max |v| = {np.abs(v64[keep]).max():.3f}")
    assert valid.all()
    assert (err_v[keep] <= e_v[keep]).all() and (err_det[keep] <= e_det[keep]).all()


@pytest.mark.parametrize("div,tm", FLAGS)
def test_float64_velocity_is_the_time_derivative_of_the_track(div, tm):
    """The float64 velocity of 257 rows is the central difference in t (h = 1e-6) of warp64.solve64's track of the material
    point that sits there, within 1e-8 -- test_velocity_is_the_time_derivative_of_the_track's bound for the float64 pair --
    and velocity_f32 on the float32 model's Jacobian is within 4 x |float32 model - float64| + that of the difference."""
    params = _params(div, tm, STEP)
    pos, t = F.inputs(257)
    xs, ts = pos.astype(np.float64), t.astype(np.float64)
    _, j64, pre = W.move_jacobian(params, xs, ts)
    keep = W.kept_rows(pre)
    assert keep.mean() >= 0.95
    v64, _ = W.velocity(j64)
    c64 = xs + W.move64(params, xs, ts)
    h = 1e-6
    fd = (W.solve64(params, c64, ts + h, start=xs) - W.solve64(params, c64, ts - h, start=xs)) / (2 * h)
    gap = float(np.abs(v64 - fd)[keep].max())
    j32 = W.move_jacobian(params, pos, t, np.float32)[1].astype(np.float32)
    v32, _, valid = F.velocity_f32(j32)
    err = float(np.abs(v32 - fd)[keep].max())
    print(f"float64 velocity against the central difference [div={div} tm={tm}]: {gap:.3e}; float32 model: {err:.3e}")
    assert gap <= 1e-8
    assert valid.all() and err <= 4 * float(np.abs(W.velocity(j32)[0] - v64)[keep].max()) + 1e-8


# ---- 3. the projector --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opengl", [True, False])
def test_projector_inverts_the_pixel_centre_rays(opengl):
    """float64, CPU tensors: points o + s * d (s = 0.5, 4) on the pixel-centre rays of the reference's formula
        direction = c2w[:3,:3] @ ((x - cx + 0.5) / fx, (y - cy + 0.5) / fy * sign, sign),  sign = -1 OpenGL / +1 OpenCV
    project to (x, y) within 1e-9 and are in front; the points o - s * d are not"""
    from ced_nerf_amd import cameras, synthetic as S
    width, height = 16, 12
    K = np.array([[21.5, 0.0, 8.25], [0.0, 19.0, 5.5], [0.0, 0.0, 1.0]])
    c2w = S.look_at_c2w(4.0, 30.0, 20.0, opengl=opengl).astype(np.float64)
    o, d, x, y = F.pinhole_rays(K, c2w, width, height, opengl)
    project = cameras.pinhole_projector(K, c2w, opengl=opengl, device="cpu")
    for s in (0.5, 4.0):
        pixels, front = project(torch.from_numpy(o + s * d))
        assert pixels.dtype == torch.float64 and pixels.shape == (width * height, 2) and front.dtype == torch.bool
        err = float(np.abs(pixels.numpy() - np.stack([x, y], -1)).max())
        print(f"projector [opengl={opengl}] s = {s}: max |pixel - index| = {err:.3e}")
        assert err <= 1e-9 and bool(front.all())
        assert not bool(project(torch.from_numpy(o - s * d))[1].any())
        mine, mine_front = F.pinhole_project(K, c2w, opengl, o + s * d, np.float64)
        assert np.abs(mine - pixels.numpy()).max() <= 1e-9 and mine_front.all()
    # float32 points keep their dtype
    assert project(torch.from_numpy((o + d).astype(np.float32)))[0].dtype == torch.float32


# ---- 4. the colour wheel -----------------------------------------------------------------------------------------------
def test_colour_wheel_known_answers():
    """zero flow is white, (max, 0) pure red, larger magnitudes saturate, a NaN or an infinity is black; the six hue
    corners land on the six pure colours; flip_w mirrors the row"""
    m = 4.0
    flow = np.zeros((1, 12, 2), np.float32)
    flow[0, 1] = [m, 0.0]
    flow[0, 2] = [3 * m, 0.0]
    flow[0, 3] = [np.nan, 1.0]
    flow[0, 4] = [0.0, np.inf]
    flow[0, 5] = [m / 2, 0.0]
    for k in range(6):                                                  # hue k / 6
        ang = 2.0 * np.pi * k / 6.0
        flow[0, 6 + k] = [m * np.cos(ang), m * np.sin(ang)]
    rgb = F.flow_rgb8(flow, m, flip_w=False)
    assert rgb.dtype == np.uint8 and rgb.shape == (1, 12, 3)
    assert rgb[0, 0].tolist() == [255, 255, 255]
    assert rgb[0, 1].tolist() == [255, 0, 0] and rgb[0, 2].tolist() == [255, 0, 0]
    assert rgb[0, 3].tolist() == [0, 0, 0] and rgb[0, 4].tolist() == [0, 0, 0]
    assert rgb[0, 5].tolist() == [255, 127, 127]                        # half the saturation, truncated
    pure = [[255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255], [255, 0, 255]]
    for k in range(6):
        assert np.abs(rgb[0, 6 + k].astype(int) - np.array(pure[k])).max() <= 1, (k, rgb[0, 6 + k])
    assert np.array_equal(F.flow_rgb8(flow, m, flip_w=True), rgb[:, ::-1])


# ---- 5. the Python layer -----------------------------------------------------------------------------------------------
def test_the_library_declares_and_binds_the_entries():
    from ced_nerf_amd import _lib, ops
    names = _lib.header_symbols()
    for name in ENTRIES:
        assert name in names and name in _lib.PROTOTYPES
        assert hasattr(_lib.lib(), name)
    assert len(_lib.PROTOTYPES[ENTRIES[0]][1]) == 8
    # the rays entry: ced_field_move_rays' arguments up to t_per_ray, then the three outputs and the stream
    assert _lib.PROTOTYPES[ENTRIES[1]][1][:10] == _lib.PROTOTYPES["ced_field_move_rays"][1][:10]
    assert len(_lib.PROTOTYPES[ENTRIES[1]][1]) == 14
    assert ops.VELOCITY_OUTPUTS == ("velocity", "det", "valid")


def test_library_refuses_bad_arguments():
    """a bad descriptor, n < 0, null inputs, no output, in that order; n == 0 is fine without pointers"""
    import ctypes as C
    from ced_nerf_amd import _lib
    L = _lib.lib()
    err = L.ced_last_error_string
    point = lambda ref, n, pos, t, *outs: L.ced_field_velocity(ref, n, pos, t, *outs, None)
    rays = lambda ref, n, *ptrs: L.ced_field_velocity_rays(ref, n, None, *ptrs[:6], 0, *ptrs[6:], None)
    assert point(None, 4, 1, 1, 1, 1, 1) == -1 and b"field_velocity" in err()
    assert rays(None, 4, *([1] * 9)) == -1 and b"field_velocity_rays" in err()
    p = np.zeros(L.ced_packed_weight_words(0, 0, _lib.MLP_F32), np.float32)
    d = _lib.FieldDesc()
    d.packed_weights = p.ctypes.data            # never dereferenced: every call below fails or returns before a launch
    d.packed_floats = p.size
    ref = C.byref(d)
    d.mlp_precision = 7
    assert point(ref, -1, 1, 1, 1, 1, 1) == -1 and b"mlp_precision" in err()
    d.mlp_precision = _lib.MLP_F32
    assert point(ref, -1, 1, 1, 1, 1, 1) == -1 and b"n < 0" in err()
    assert rays(ref, -1, *([1] * 9)) == -1 and b"n < 0" in err()
    assert point(ref, 0, None, None, None, None, None) == 0
    assert rays(ref, 0, *([None] * 9)) == 0
    assert point(ref, 4, None, 1, 1, 1, 1) == -1 and b"null" in err()
    assert point(ref, 4, 1, None, 1, 1, 1) == -1 and b"null" in err()
    assert point(ref, 4, 1, 1, None, None, None) == -1 and b"no output" in err()
    for k in range(6):
        ptrs = [1] * 9
        ptrs[k] = None
        assert rays(ref, 4, *ptrs) == -1 and b"null" in err(), k
    assert rays(ref, 4, *([1] * 6 + [None] * 3)) == -1 and b"no output" in err()
    flow = lambda h, w, src, mag, out: L.ced_flow_to_rgb8(h, w, src, mag, 1, out, None)
    assert flow(-1, 4, 1, 1.0, 1) == -1 and b"negative" in err()
    assert flow(4, 4, 1, 0.0, 1) == -1 and b"max_mag" in err()
    assert flow(4, 4, 1, float("nan"), 1) == -1 and b"max_mag" in err()
    assert flow(0, 4, None, 1.0, None) == 0
    assert flow(4, 4, None, 1.0, 1) == -1 and b"null" in err()


def test_cpu_tensors_and_training_fields_are_refused():
    from ced_nerf_amd import cameras, ops, utils
    from ced_nerf_amd.video import render_video
    f = _cpu_field()
    x, t = torch.zeros(4, 3), torch.zeros(4)
    rays = utils.Rays(origins=x, viewdirs=x)
    ts = torch.zeros(1, 1)
    project = cameras.pinhole_projector(np.eye(3), np.eye(4)[:3], device="cpu")
    for call in (lambda: f.query_scene_flow(x, t),
                 lambda: f.query_scene_flow_rays(x, x, torch.zeros(4, dtype=torch.int64), t, t, ts),
                 lambda: ops.field_velocity(None, x, t),
                 lambda: ops.flow_to_rgb8(torch.zeros(2, 2, 2), 1.0),
                 lambda: utils.render_scene_flow(f, None, rays, timestamps=ts),
                 lambda: utils.render_optical_flow(f, None, rays, project, 0.1, timestamps=ts)):
        with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
            call()
    for call in (lambda: utils.render_scene_flow(f, None, rays), lambda: utils.render_optical_flow(f, None, rays, project, 0.1)):
        with pytest.raises(NotImplementedError, match="timestamps"):
            call()
    f.train()
    for who, call in (("render_scene_flow", lambda: utils.render_scene_flow(f, None, rays, timestamps=ts)),
                      ("render_optical_flow", lambda: utils.render_optical_flow(f, None, rays, project, 0.1, timestamps=ts)),
                      ("render_motion", lambda: utils.render_motion(f, None, rays, timestamps=ts))):
        with pytest.raises(NotImplementedError, match=f"{who} renders eval frames"):
            call()
    f.eval()
    assert "scene_flow" in render_video.__doc__ and "optical_flow" in render_video.__doc__
    assert "query_scene_flow" in f.query_velocity.__doc__


def test_cli_has_the_flow_flags(tmp_path):
    from ced_nerf_amd import trainer
    with pytest.raises(SystemExit) as e:
        trainer.main(["--help"])
    assert e.value.code == 0
    import inspect
    assert "flow_max" in inspect.signature(trainer.write_video_frames).parameters
