"""CPU suite: the Python layer of point tracking and the tracked mesh -- argument checks, the command line, the PLY writer.
No kernel is launched here."""
import struct

import numpy as np
import pytest
import torch


def _cpu_field():
    from ced_nerf_amd import synthetic as S
    from ced_nerf_amd.model import DNGPradianceField
    p = S.init_field_params([-1, -1, -1, 1, 1, 1], 1.0 / 32, 256, 10, use_div_offsets=True)
    return DNGPradianceField.from_params(p, "cpu").eval()


def test_the_library_declares_and_binds_the_two_entries():
    from ced_nerf_amd import _lib, ops
    names = _lib.header_symbols()
    for name in ("ced_field_move_inverse", "ced_field_track"):
        assert name in names and name in _lib.PROTOTYPES
    assert len(_lib.PROTOTYPES["ced_field_move_inverse"][1]) == 11 and len(_lib.PROTOTYPES["ced_field_track"][1]) == 12
    assert callable(ops.field_move_inverse) and callable(ops.field_track)


def test_library_refuses_bad_solver_arguments():
    """the C entries report, in this order: a bad descriptor, n < 0, max_iters outside 1 .. 1024, tol < 0 or NaN; n == 0 is
    fine without pointers; P * T must not overflow"""
    import ctypes as C
    from ced_nerf_amd import _lib
    L = _lib.lib()
    assert L.ced_field_move_inverse(None, 4, 1, 1, None, 32, 1e-6, 1, 1, 1, None) != 0
    p = np.zeros(_lib.lib().ced_packed_weight_words(0, 0, _lib.MLP_F32), np.float32)
    d = _lib.FieldDesc()
    d.packed_weights = p.ctypes.data            # never dereferenced: every call below fails or returns before a launch
    d.packed_floats = p.size
    ref = C.byref(d)
    for iters, tol in ((0, 1e-6), (-3, 1e-6), (1025, 1e-6), (32, -1e-9), (32, float("nan"))):
        assert L.ced_field_move_inverse(ref, 4, 1, 1, None, iters, tol, 1, 1, 1, None) == -1, (iters, tol)
        assert b"field_move_inverse" in L.ced_last_error_string()
        assert L.ced_field_track(ref, 4, 2, 1, 1, None, iters, tol, 1, 1, 1, None) == -1, (iters, tol)
        assert b"field_track" in L.ced_last_error_string()
    assert L.ced_field_move_inverse(ref, -1, 1, 1, None, 32, 1e-6, 1, 1, 1, None) == -1
    assert L.ced_field_move_inverse(ref, 0, None, None, None, 32, 0.0, None, None, None, None) == 0
    assert L.ced_field_track(ref, 0, 5, None, None, None, 1, 0.0, None, None, None, None) == 0
    assert L.ced_field_track(ref, 5, 0, None, None, None, 1024, 0.0, None, None, None, None) == 0
    assert L.ced_field_move_inverse(ref, 4, None, 1, None, 32, 1e-6, 1, 1, 1, None) == -1          # null target
    assert L.ced_field_move_inverse(ref, 4, 1, None, None, 32, 1e-6, 1, 1, 1, None) == -1          # null t
    assert L.ced_field_move_inverse(ref, 4, 1, 1, None, 32, 1e-6, None, None, None, None) == -1    # no output
    assert L.ced_field_track(ref, 4, 2, None, 1, None, 32, 1e-6, 1, 1, 1, None) == -1
    assert L.ced_field_track(ref, 4, 2, 1, None, None, 32, 1e-6, 1, 1, 1, None) == -1
    assert L.ced_field_track(ref, 1 << 40, 1 << 40, 1, 1, None, 32, 1e-6, 1, 1, 1, None) == -1
    assert b"overflow" in L.ced_last_error_string()
    assert L.ced_field_track(ref, -1, 2, 1, 1, None, 32, 1e-6, 1, 1, 1, None) == -1


@pytest.mark.parametrize("bad", [dict(max_iters=0), dict(max_iters=1025), dict(max_iters=-1), dict(max_iters=2.5),
                                 dict(max_iters=True), dict(tol=-1e-9), dict(tol=float("nan")), dict(tol="tight")])
def test_bad_max_iters_or_tol_is_a_value_error(bad):
    from ced_nerf_amd import export, ops
    f = _cpu_field()
    c, t = torch.zeros(4, 3), torch.zeros(4)
    with pytest.raises(ValueError, match="max_iters|tol"):
        f.query_move_inverse(c, t, **bad)
    with pytest.raises(ValueError, match="max_iters|tol"):
        f.track_points(c, 0.5, [0.0, 1.0], **bad)
    with pytest.raises(ValueError, match="max_iters|tol"):
        ops.field_move_inverse(None, c, t, **bad)
    with pytest.raises(ValueError, match="max_iters|tol"):
        ops.field_track(None, c, t, **bad)
    with pytest.raises(ValueError, match="max_iters|tol"):
        export.track_mesh(f, dict(vertices=c), 0.5, [0.0], **bad)
    with pytest.raises(ValueError, match="max_iters|tol"):
        export.extract_mesh_tracked(f, 0.5, [0.0], reso=8, **bad)
    assert ops.check_solve(1, 0) == (1, 0.0) and ops.check_solve(np.int64(1024), np.float32(0.5)) == (1024, 0.5)


def test_cpu_tensors_are_refused():
    from ced_nerf_amd import export, ops
    f = _cpu_field()
    c, t = torch.zeros(4, 3), torch.zeros(4)
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        f.query_move_inverse(c, t)
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        f.query_move_inverse(c, t, init=c)
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        f.track_points(c, 0.5, [0.0, 1.0])
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        ops.field_move_inverse(None, c, t)
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        ops.field_track(None, c, torch.zeros(2))
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        export.track_mesh(f, dict(vertices=c, faces=torch.zeros(0, 3, dtype=torch.int32)), 0.5, [0.0, 1.0])
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        export.extract_mesh_tracked(f, 0.5, [0.0, 1.0], reso=8)
    with pytest.raises(ValueError, match="one-element"):
        export.track_mesh(f, dict(vertices=c), torch.zeros(2), [0.0])


def test_mesh_track_flag():
    from ced_nerf_amd.export import main, make_parser
    base = ["--load_model", "m.pth", "--preset", "dnerf", "--out", "o"]
    a = make_parser().parse_args(base)
    assert a.mesh_track is None and a.track_iters == 32 and a.track_tol == 1e-6 and not a.mesh
    a = make_parser().parse_args(base + ["--mesh", "--mesh_track", "0.25", "--times", "0,0.5,1", "--track_iters", "64",
                                         "--track_tol", "1e-5"])
    assert a.mesh and a.mesh_track == 0.25 and a.times == [0.0, 0.5, 1.0] and a.track_iters == 64 and a.track_tol == 1e-5
    with pytest.raises(SystemExit):
        make_parser().parse_args(base + ["--mesh_track", "soon"])
    with pytest.raises(SystemExit, match="--mesh_track needs --mesh"):
        main(base + ["--mesh_track", "0.25"])


def _mesh(with_normals=True, with_rgb=True):
    rng = np.random.default_rng(5)
    v, n_f = 7, 4
    mesh = dict(vertices=torch.from_numpy(rng.normal(size=(v, 3)).astype(np.float32)),
                faces=torch.from_numpy(rng.integers(0, v, size=(n_f, 3)).astype(np.int32)), apply_act=False)
    if with_normals:
        mesh["normals"] = torch.from_numpy(rng.normal(size=(v, 3)).astype(np.float32))
    if with_rgb:
        mesh["rgb"] = torch.from_numpy(rng.normal(size=(v, 2, 3)).astype(np.float32))
    return mesh


def _colours(mesh):
    if "rgb" not in mesh:
        return np.full((mesh["vertices"].shape[0], 3), 128, np.uint8)
    rgb = 1.0 / (1.0 + np.exp(-mesh["rgb"].numpy().astype(np.float64)))
    return np.clip(np.rint(255.0 * rgb.mean(axis=1)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("with_rgb", [True, False])
def test_ply_of_a_mesh_with_normals_is_byte_for_byte_what_it_was(tmp_path, with_rgb):
    """the file of a dict that has `normals`, restated record by record with struct: header, 27-byte vertices, 13-byte faces"""
    from ced_nerf_amd import export as E
    mesh = _mesh(True, with_rgb)
    E.save_mesh_ply(str(tmp_path / "m.ply"), mesh)
    v, n_f = mesh["vertices"].shape[0], mesh["faces"].shape[0]
    want = ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {v}\n"
            "property float x\nproperty float y\nproperty float z\n"
            "property float nx\nproperty float ny\nproperty float nz\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\n"
            f"element face {n_f}\n"
            "property list uchar int vertex_indices\nend_header\n").encode("ascii")
    col = _colours(mesh)
    for p, n, c in zip(mesh["vertices"].tolist(), mesh["normals"].tolist(), col.tolist()):
        want += struct.pack("<ffffffBBB", *p, *n, *c)
    for tri in mesh["faces"].tolist():
        want += struct.pack("<Biii", 3, *tri)
    assert (tmp_path / "m.ply").read_bytes() == want
    assert E.mesh_ply_header(v, n_f) == E.mesh_ply_header(v, n_f, normals=True) == want[:want.index(b"end_header\n") + 11]
    assert E.MESH_PLY_VERTEX.size == 27 and E.MESH_PLY_FACE.size == 13


@pytest.mark.parametrize("with_rgb", [True, False])
def test_ply_of_a_mesh_without_normals(tmp_path, with_rgb):
    from ced_nerf_amd import export as E
    mesh = _mesh(False, with_rgb)
    E.save_mesh_ply(str(tmp_path / "m.ply"), mesh)
    v, n_f = mesh["vertices"].shape[0], mesh["faces"].shape[0]
    want = ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {v}\n"
            "property float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\n"
            f"element face {n_f}\n"
            "property list uchar int vertex_indices\nend_header\n").encode("ascii")
    assert E.mesh_ply_header(v, n_f, normals=False) == want and b"nx" not in want
    for p, c in zip(mesh["vertices"].tolist(), _colours(mesh).tolist()):
        want += struct.pack("<fffBBB", *p, *c)
    for tri in mesh["faces"].tolist():
        want += struct.pack("<Biii", 3, *tri)
    assert (tmp_path / "m.ply").read_bytes() == want
    assert E.MESH_PLY_VERTEX_PLAIN.size == 15


def test_tracked_frames_and_npz(tmp_path):
    """tracked_frame / save_tracked_npz on a hand-made tracked mesh: a frame carries the time's vertices, the shared faces and
    the reference colours, never the reference normals"""
    from ced_nerf_amd import export as E
    ref = _mesh(True, True)
    v = ref["vertices"].shape[0]
    tracked = dict(ref, vertices_t=torch.stack([ref["vertices"] + k for k in range(3)]), converged=torch.ones(3, v, dtype=torch.bool),
                   step=torch.zeros(3, v), evals=torch.full((3, v), 4, dtype=torch.int32), canonical=ref["vertices"] * 2,
                   cube=torch.arange(v), sigma=torch.ones(v), embedding=torch.zeros(v, 15), times=[0.0, 0.5, 1.0], t_ref=0.5,
                   reso=8, center=[0.0, 0.0, 0.0], radius=1.0, sigma_thresh=2.0)
    del tracked["vertices"]
    for k in range(3):
        fr = E.tracked_frame(tracked, k)
        assert set(fr) == {"vertices", "faces", "t", "rgb", "apply_act"} and fr["t"] == tracked["times"][k]
        assert torch.equal(fr["vertices"], tracked["vertices_t"][k]) and fr["faces"] is tracked["faces"]
    E.save_tracked_npz(str(tmp_path / "t.npz"), tracked)
    with np.load(tmp_path / "t.npz") as z:
        assert set(z.files) == {"vertices_t", "converged", "step", "evals", "canonical", "faces", "cube", "sigma", "embedding",
                                "rgb", "normals", "times", "t_ref", "reso", "center", "radius", "sigma_thresh", "apply_act"}
        assert z["vertices_t"].shape == (3, v, 3) and z["converged"].dtype == np.bool_ and z["evals"].dtype == np.int32
        assert np.array_equal(z["times"], np.float32([0.0, 0.5, 1.0])) and float(z["t_ref"]) == 0.5


def test_tracked_npz_of_a_bare_mesh(tmp_path):
    """save_tracked_npz keeps track_mesh's rule -- a key of the reference mesh is written if it is there: a tracked dict
    from a hand-built mesh (vertices and faces only) has no reso, center, radius, sigma_thresh"""
    from ced_nerf_amd import export as E
    faces = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    tracked = dict(faces=faces, vertices_t=torch.zeros(2, 3, 3), converged=torch.ones(2, 3, dtype=torch.bool),
                   step=torch.zeros(2, 3), evals=torch.ones(2, 3, dtype=torch.int32), canonical=torch.zeros(3, 3),
                   times=[0.0, 1.0], t_ref=0.0)
    E.save_tracked_npz(str(tmp_path / "t.npz"), tracked)
    with np.load(tmp_path / "t.npz") as z:
        assert set(z.files) == {"vertices_t", "converged", "step", "evals", "canonical", "faces", "times", "t_ref", "apply_act"}
        assert not bool(z["apply_act"]) and np.array_equal(z["faces"], faces.numpy())
