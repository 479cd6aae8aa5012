"""CPU suite: the derivative of the warp -- the three entries' declarations and refusals, the Python layer's argument
checks, the command line, the tracked mesh's moving normals in its files, and the float64 reference of the GPU suite
(tests/warp64.py) pinned against a complex-step derivative.  No kernel is launched here."""
import functools

import numpy as np
import pytest
import torch

import warp64 as W

ENTRIES = ("ced_field_move_jacobian", "ced_field_move_inverse_newton", "ced_field_track_newton")
AABB = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
FLAGS = [(False, 0), (True, 2)]


def _cpu_field():
    from ced_nerf_amd import synthetic as S
    from ced_nerf_amd.model import DNGPradianceField
    p = S.init_field_params([-1, -1, -1, 1, 1, 1], 1.0 / 32, 256, 10, use_div_offsets=True)
    return DNGPradianceField.from_params(p, "cpu").eval()


@functools.lru_cache(maxsize=None)
def _params(div, tm, step):
    from ced_nerf_amd import synthetic as S
    return S.init_field_params(list(AABB), step, hash_max_res=256, log2_hashmap_size=15, use_div_offsets=div,
                               use_time_embedding=tm != 0, use_time_attenuation=tm == 2, regime="trained")


def _inputs(n):
    rng = np.random.default_rng(7)
    pos = rng.uniform(-1.6, 1.6, size=(4099, 3)).astype(np.float32)
    t = rng.uniform(0.0, 1.0, size=(4099,)).astype(np.float32)
    return pos[:n], t[:n]


def test_the_library_declares_and_binds_the_three_entries():
    from ced_nerf_amd import _lib, ops
    names = _lib.header_symbols()
    for name in ENTRIES:
        assert name in names and name in _lib.PROTOTYPES
        assert hasattr(_lib.lib(), name)
    assert len(_lib.PROTOTYPES["ced_field_move_jacobian"][1]) == 7
    # the Newton entries take the fixed-point entries' arguments
    assert _lib.PROTOTYPES["ced_field_move_inverse_newton"] == _lib.PROTOTYPES["ced_field_move_inverse"]
    assert _lib.PROTOTYPES["ced_field_track_newton"] == _lib.PROTOTYPES["ced_field_track"]
    assert callable(ops.field_move_jacobian) and callable(ops.field_move_inverse_newton) and callable(ops.field_track_newton)
    assert "field_jacobian.hip" in _lib.SOURCES


def test_library_refuses_bad_arguments():
    """the C entries report, in the order of the fixed-point entries: a bad descriptor, n < 0, max_iters outside 1 .. 1024,
    tol < 0 or NaN, null inputs, no output; n == 0 is fine without pointers; P * T must not overflow"""
    import ctypes as C
    from ced_nerf_amd import _lib
    L = _lib.lib()
    err = L.ced_last_error_string
    assert L.ced_field_move_jacobian(None, 4, 1, 1, 1, 1, None) == -1 and b"field_move_jacobian" in err()
    assert L.ced_field_move_inverse_newton(None, 4, 1, 1, None, 32, 1e-6, 1, 1, 1, None) == -1
    assert L.ced_field_track_newton(None, 4, 2, 1, 1, None, 32, 1e-6, 1, 1, 1, None) == -1
    p = np.zeros(L.ced_packed_weight_words(0, 0, _lib.MLP_F32), np.float32)
    d = _lib.FieldDesc()
    d.packed_weights = p.ctypes.data            # never dereferenced: every call below fails or returns before a launch
    d.packed_floats = p.size
    ref = C.byref(d)
    # the descriptor comes first: a bad one is reported even with n < 0 and a bad max_iters
    d.mlp_precision = 7
    assert L.ced_field_move_jacobian(ref, -1, 1, 1, 1, 1, None) == -1 and b"mlp_precision" in err()
    assert L.ced_field_move_inverse_newton(ref, -1, 1, 1, None, 0, -1.0, 1, 1, 1, None) == -1 and b"mlp_precision" in err()
    assert L.ced_field_track_newton(ref, -1, 2, 1, 1, None, 0, -1.0, 1, 1, 1, None) == -1 and b"mlp_precision" in err()
    d.mlp_precision = _lib.MLP_F32
    # then n < 0, before max_iters / tol
    assert L.ced_field_move_jacobian(ref, -1, 1, 1, 1, 1, None) == -1 and b"n < 0" in err()
    assert L.ced_field_move_inverse_newton(ref, -1, 1, 1, None, 0, 1e-6, 1, 1, 1, None) == -1 and b"n < 0" in err()
    assert L.ced_field_track_newton(ref, -1, 2, 1, 1, None, 0, 1e-6, 1, 1, 1, None) == -1 and b"n_points" in err()
    assert L.ced_field_track_newton(ref, 1 << 40, 1 << 40, 1, 1, None, 0, 1e-6, 1, 1, 1, None) == -1 and b"overflow" in err()
    # then the solver's arguments, before the pointers
    for iters, tol in ((0, 1e-6), (-3, 1e-6), (1025, 1e-6), (32, -1e-9), (32, float("nan"))):
        assert L.ced_field_move_inverse_newton(ref, 4, None, None, None, iters, tol, None, None, None, None) == -1, (iters, tol)
        assert b"field_move_inverse_newton" in err() and (b"max_iters" in err() or b"tol" in err())
        assert L.ced_field_track_newton(ref, 4, 2, None, None, None, iters, tol, None, None, None, None) == -1, (iters, tol)
        assert b"field_track_newton" in err() and (b"max_iters" in err() or b"tol" in err())
    # n == 0 needs no pointers
    assert L.ced_field_move_jacobian(ref, 0, None, None, None, None, None) == 0
    assert L.ced_field_move_inverse_newton(ref, 0, None, None, None, 32, 0.0, None, None, None, None) == 0
    assert L.ced_field_track_newton(ref, 0, 5, None, None, None, 1, 0.0, None, None, None, None) == 0
    assert L.ced_field_track_newton(ref, 5, 0, None, None, None, 1024, 0.0, None, None, None, None) == 0
    # null inputs, then no output
    assert L.ced_field_move_jacobian(ref, 4, None, 1, 1, 1, None) == -1 and b"null" in err()
    assert L.ced_field_move_jacobian(ref, 4, 1, None, 1, 1, None) == -1 and b"null" in err()
    assert L.ced_field_move_jacobian(ref, 4, 1, 1, None, None, None) == -1 and b"no output" in err()
    assert L.ced_field_move_inverse_newton(ref, 4, None, 1, None, 32, 1e-6, None, None, None, None) == -1 and b"null" in err()
    assert L.ced_field_move_inverse_newton(ref, 4, 1, None, None, 32, 1e-6, 1, 1, 1, None) == -1 and b"null" in err()
    assert L.ced_field_move_inverse_newton(ref, 4, 1, 1, None, 32, 1e-6, None, None, None, None) == -1 and b"no output" in err()
    assert L.ced_field_track_newton(ref, 4, 2, None, 1, None, 32, 1e-6, None, None, None, None) == -1 and b"null" in err()
    assert L.ced_field_track_newton(ref, 4, 2, 1, None, None, 32, 1e-6, 1, 1, 1, None) == -1 and b"null" in err()
    assert L.ced_field_track_newton(ref, 4, 2, 1, 1, None, 32, 1e-6, None, None, None, None) == -1 and b"no output" in err()


def test_cpu_tensors_are_refused():
    from ced_nerf_amd import export, ops
    f = _cpu_field()
    c, t = torch.zeros(4, 3), torch.zeros(4)
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        f.query_move_jacobian(c, t)
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        f.query_velocity(c, t)
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        f.query_move_inverse(c, t, method="newton")
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        f.track_points(c, 0.5, [0.0, 1.0], method="newton")
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        ops.field_move_jacobian(None, c, t)
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        ops.field_move_inverse_newton(None, c, t)
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        ops.field_track_newton(None, c, torch.zeros(2))
    mesh = dict(vertices=c, faces=torch.zeros(0, 3, dtype=torch.int32), normals=torch.ones(4, 3))
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        export.track_mesh(f, mesh, 0.5, [0.0, 1.0], method="newton", normals=True, velocities=True)
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        export.extract_mesh_tracked(f, 0.5, [0.0, 1.0], reso=8, method="newton", normals=True)


@pytest.mark.parametrize("bad", ["Newton", "fixed", "", None, 3])
def test_an_unknown_method_is_a_value_error(bad):
    from ced_nerf_amd import export, ops
    f = _cpu_field()
    c, t = torch.zeros(4, 3), torch.zeros(4)
    with pytest.raises(ValueError, match="method"):
        f.query_move_inverse(c, t, method=bad)
    with pytest.raises(ValueError, match="method"):
        f.track_points(c, 0.5, [0.0, 1.0], method=bad)
    with pytest.raises(ValueError, match="method"):
        export.track_mesh(f, dict(vertices=c), 0.5, [0.0], method=bad)
    with pytest.raises(ValueError, match="method"):
        export.extract_mesh_tracked(f, 0.5, [0.0], reso=8, method=bad)
    assert ops.SOLVE_METHODS == ("fixed_point", "newton") and ops.check_method("newton") == "newton"
    # the solver's numbers are still checked, by the Newton entries too
    with pytest.raises(ValueError, match="max_iters"):
        ops.field_move_inverse_newton(None, c, t, max_iters=0)
    with pytest.raises(ValueError, match="tol"):
        ops.field_track_newton(None, c, t, tol=-1.0)
    with pytest.raises(ValueError, match="normals"):
        export.track_mesh(f, dict(vertices=c), 0.5, [0.0], normals=True)


def test_mesh_track_method_and_normals_flags():
    from ced_nerf_amd.export import make_parser
    base = ["--load_model", "m.pth", "--preset", "dnerf", "--out", "o"]
    a = make_parser().parse_args(base)
    assert a.mesh_track_method == "fixed_point" and a.mesh_track_normals is False
    a = make_parser().parse_args(base + ["--mesh", "--mesh_track", "0.25", "--mesh_track_method", "newton", "--mesh_track_normals"])
    assert a.mesh_track_method == "newton" and a.mesh_track_normals is True and a.mesh_track == 0.25
    a = make_parser().parse_args(base + ["--mesh_track_method", "fixed_point"])
    assert a.mesh_track_method == "fixed_point"
    with pytest.raises(SystemExit):
        make_parser().parse_args(base + ["--mesh_track_method", "secant"])


def _tracked(with_normals_t):
    rng = np.random.default_rng(5)
    v, n_f = 7, 4
    r = lambda *s: torch.from_numpy(rng.normal(size=s).astype(np.float32))
    tracked = dict(faces=torch.from_numpy(rng.integers(0, v, size=(n_f, 3)).astype(np.int32)), normals=r(v, 3), rgb=r(v, 2, 3),
                   apply_act=False, vertices_t=r(3, v, 3), converged=torch.ones(3, v, dtype=torch.bool), step=torch.zeros(3, v),
                   evals=torch.full((3, v), 4, dtype=torch.int32), canonical=r(v, 3), times=[0.0, 0.5, 1.0], t_ref=0.5)
    if with_normals_t:
        tracked.update(normals_t=r(3, v, 3), velocities_t=r(3, v, 3), det_t=r(3, v))
    return tracked


def test_tracked_frames_and_npz_with_moving_normals(tmp_path):
    """with normals_t a frame carries its time's normals (never the reference's) and its PLY has them; the npz holds
    normals_t, velocities_t and det_t; without them frames and files are what they were"""
    from ced_nerf_amd import export as E
    plain, moving = _tracked(False), _tracked(True)
    for k in range(3):
        fr = E.tracked_frame(plain, k)
        assert set(fr) == {"vertices", "faces", "t", "rgb", "apply_act"}
        E.save_mesh_ply(str(tmp_path / f"plain_{k}.ply"), fr)
        assert b"property float nx" not in (tmp_path / f"plain_{k}.ply").read_bytes()
        fr = E.tracked_frame(moving, k)
        assert set(fr) == {"vertices", "faces", "t", "rgb", "apply_act", "normals"}
        assert torch.equal(fr["normals"], moving["normals_t"][k]) and not torch.equal(fr["normals"], moving["normals"])
        E.save_mesh_ply(str(tmp_path / f"moving_{k}.ply"), fr)
        data = (tmp_path / f"moving_{k}.ply").read_bytes()
        head, _, body = data.partition(b"end_header\n")
        assert b"property float nx" in head
        rec = np.frombuffer(body[:27 * 7], dtype=np.dtype([("xyz", "<f4", 3), ("normal", "<f4", 3), ("rgb", "u1", 3)]))
        assert np.array_equal(rec["normal"], moving["normals_t"][k].numpy())
        assert np.array_equal(rec["xyz"], moving["vertices_t"][k].numpy())
        # everything but the normals is the plain frame's, byte for byte
        plain_like = dict(fr)
        del plain_like["normals"]
        E.save_mesh_ply(str(tmp_path / "again.ply"), plain_like)
        assert (tmp_path / "again.ply").read_bytes() == (tmp_path / f"plain_{k}.ply").read_bytes()
    base = {"vertices_t", "converged", "step", "evals", "canonical", "faces", "rgb", "normals", "times", "t_ref", "apply_act"}
    E.save_tracked_npz(str(tmp_path / "plain.npz"), plain)
    with np.load(tmp_path / "plain.npz") as z:
        assert set(z.files) == base
    E.save_tracked_npz(str(tmp_path / "moving.npz"), moving)
    with np.load(tmp_path / "moving.npz") as z:
        assert set(z.files) == base | {"normals_t", "velocities_t", "det_t"}
        for k in ("normals_t", "velocities_t", "det_t"):
            assert np.array_equal(z[k], moving[k].numpy())


def test_the_shared_3x3_helper_is_the_adjugate_inverse():
    from ced_nerf_amd import ops
    rng = np.random.default_rng(3)
    jac = rng.uniform(-0.35, 0.35, size=(2, 65, 3, 4))
    A, inv, det = ops.warp_gradient(torch.from_numpy(jac))
    A64, inv64, det64 = W.gradient_inverse(jac)
    assert A.shape == (2, 65, 3, 3) and det.shape == (2, 65)
    assert np.abs(A.numpy() - A64).max() == 0 and np.abs(det.numpy() - det64).max() <= 1e-15
    assert np.abs(inv.numpy() - inv64).max() <= 1e-14
    assert np.abs((inv @ A).numpy() - np.eye(3)).max() <= 1e-14
    assert np.abs(det64 - np.linalg.det(A64)).max() <= 1e-15
    A32, inv32, det32 = ops.warp_gradient(torch.from_numpy(jac.astype(np.float32)))
    assert inv32.dtype == torch.float32 and np.abs(inv32.numpy() - inv64).max() <= 1e-5


@pytest.mark.parametrize("step", [1.0 / 32, 1.0 / 8])
@pytest.mark.parametrize("div,tm", FLAGS)
def test_forward_mode_model_is_the_complex_step_derivative(div, tm, step):
    """the float64 forward-mode model of tests/warp64.py against Im move(p + i h e_b) / h, h = 1e-30, the ReLU deciding on
    the real part: equal within 1e-12 of the largest entry -- this pins the reference of the GPU suite.  (1.9e-15.)"""
    params = _params(div, tm, step)
    pos, t = _inputs(1025)
    move, jac, pre = W.move_jacobian(params, pos, t)
    assert move.dtype == np.float64 and jac.shape == (1025, 3, 4) and len(pre) == 3 and pre[0].shape == (1025, 64)
    cs = W.complex_step(params, pos, t)
    scale = np.abs(jac).max()
    err = np.abs(cs - jac).max() / scale
    print(f"step {step:g} div={div}: max |J| = {scale:.4f}, forward mode vs complex step {err:.2e} relative")
    assert 0.05 < scale < 2.0 and err <= 1e-12
    # the time column is not zero, and the model's move is the tracking suite's
    assert np.abs(jac[:, :, 3]).max() > 1e-3
    from test_gpu_track import _move_model
    assert np.array_equal(move, _move_model(params, pos, t))


@pytest.mark.parametrize("div,tm", FLAGS)
def test_numpy_newton_statement_inverts_the_model(div, tm):
    """include/cednerf_hip.h's Newton iteration in numpy float32, on the float32 model: at moving step 1/32 every row
    converges within 2 .. 5 evaluations (K = 32, tol = 1e-6), the returned step is the residual of the returned x; with
    K = 1 nothing moves; a refused determinant takes the fixed-point step"""
    params = _params(div, tm, 1.0 / 32)
    pos, t = _inputs(513)
    fn = W.model_move_jac(params, np.float32)
    c = (pos + fn(pos, t)[0]).astype(np.float32)
    x, step, evals = W.newton_f32(fn, c, t, 32, 1e-6)
    assert x.dtype == np.float32 and step.dtype == np.float32 and evals.dtype == np.int32
    assert (step <= 1e-6).all() and 2 <= evals.min() and evals.max() <= 5
    resid = np.abs((x + fn(x, t)[0]) - c).max(-1)
    assert np.array_equal(resid, step)
    assert np.abs(x - pos).max() <= 1e-5
    x1, step1, evals1 = W.newton_f32(fn, c, t, 1, 1e-6)
    assert np.array_equal(x1, c) and (evals1 == 1).all() and np.array_equal(step1, np.abs((c + fn(c, t)[0]) - c).max(-1))
    # a refused determinant falls back to the fixed-point step
    J = np.zeros((2, 3, 4), np.float32)
    J[0, 0, 0] = -1.0
    r = np.float32([[1, 2, 3], [1, 2, 3]])
    d = W.newton_step_f32(J, r)
    assert np.array_equal(d[0], r[0]) and np.array_equal(d[1], r[1])     # singular: d = r; identity: d = r as well
    J[1, 0, 0] = 1.0
    assert np.array_equal(W.newton_step_f32(J, r)[1], np.float32([0.5, 2, 3]))
