"""CPU suite of the mesh export: the definition of include/cednerf_hip.h as tests/mesh_reference.py restates it, on analytic
lattices whose meshes are known (counts, manifoldness, Euler characteristic, orientation), and the host side of
ced_nerf_amd/export.py -- the entries are declared, bound and exported and refuse bad arguments with codes; the file
writers; the parser; the argument checks.  No kernel is launched here."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

import mesh_reference as R

ENTRIES = ("ced_mesh_workspace_bytes", "ced_mesh_vertices", "ced_mesh_faces")


def _nets(S):
    return R.surface_nets(S, R.THRESH, R.CENTER, R.RADIUS)


# (lattice, reso) -> (V, F, Euler characteristic): a loop-form prototype of the definition measured these
KNOWN = {("sphere", 12): (246, 488, 2), ("sphere", 20): (672, 1340, 2),
         ("torus", 12): (352, 704, 0), ("torus", 20): (912, 1824, 0)}


@pytest.mark.parametrize("name,reso", sorted(KNOWN))
def test_analytic_surfaces_are_closed_manifolds_of_the_known_size(name, reso):
    S = {"sphere": R.sphere_lattice, "torus": R.torus_lattice}[name](reso)
    vertices, normals, cube, faces = _nets(S)
    n_v, n_f, chi = KNOWN[(name, reso)]
    print(f"{name} reso {reso}: V = {vertices.shape[0]}, F = {faces.shape[0]}, chi = {R.euler_characteristic(faces)}")
    assert (vertices.shape[0], faces.shape[0]) == (n_v, n_f)
    assert vertices.dtype == np.float32 and normals.dtype == np.float32 and cube.dtype == np.int64
    assert faces.dtype == np.int32 and faces.min() >= 0 and faces.max() < n_v
    assert np.unique(faces).size == n_v and bool((np.diff(cube) > 0).all())
    assert R.is_two_manifold(faces) and R.euler_characteristic(faces) == chi
    assert R.signed_volume(vertices, faces) > 0


@pytest.mark.parametrize("reso", [12, 20])
def test_sphere_vertices_lie_on_the_sphere_and_normals_point_outwards(reso):
    vertices, normals, _, faces = _nets(R.sphere_lattice(reso))
    h = 3.0 / reso
    rel = vertices.astype(np.float64) - np.asarray(R.SPHERE_CENTER)
    dist = np.linalg.norm(rel, axis=1)
    radial = (normals * (rel / dist[:, None])).sum(1)
    print(f"reso {reso}: max | |v - c| - 0.9 | = {np.abs(dist - R.SPHERE_RADIUS).max() / h:.3f} h, "
          f"min radial component {radial.min():.4f}")
    assert np.abs(dist - R.SPHERE_RADIUS).max() <= 0.5 * h
    assert radial.min() >= 0.9
    assert np.allclose(np.linalg.norm(normals.astype(np.float64), axis=1), 1.0, atol=1e-6)
    # the analytic volume of the sphere, to the lattice's resolution
    assert abs(R.signed_volume(vertices, faces) / (4.0 / 3.0 * np.pi * R.SPHERE_RADIUS ** 3) - 1.0) < 0.05


@pytest.mark.parametrize("reso", [12, 20])
def test_noise_inside_a_zero_border_is_closed_but_not_manifold(reso):
    vertices, _, _, faces = _nets(R.noise_lattice(reso))
    assert vertices.shape[0] > 0 and faces.shape[0] > 0
    assert R.directed_edges_balance(faces)
    assert not R.is_two_manifold(faces)
    # with the border left open, border edges emit no face: boundary edges appear, every index stays valid
    v_open, _, _, f_open = _nets(R.noise_lattice(reso, closed=False))
    assert not R.directed_edges_balance(f_open) and f_open.min() >= 0 and f_open.max() < v_open.shape[0]


def test_degenerate_sizes():
    one = R.surface_nets(np.full((1, 1, 1), 2.0, np.float32), 1.0, R.CENTER, R.RADIUS)
    assert [a.shape for a in one] == [(0, 3), (0, 3), (0,), (0, 3)]
    S = np.zeros((2, 2, 2), np.float32)
    S[1, 0, 1] = 3.0
    vertices, normals, cube, faces = R.surface_nets(S, 1.0, R.CENTER, R.RADIUS)
    assert vertices.shape == (1, 3) and cube.tolist() == [0] and faces.shape == (0, 3)
    # by hand: three edges cross, all at the inside corner (1,0,1).  In the definition's order: along x from (0,0,1),
    # mu = (1 - 0) / (3 - 0); along y from (1,0,1), mu = (1 - 3) / (0 - 3); along z from (1,0,0), mu = 1 / 3
    f = np.float32
    up, down = (f(1) - f(0)) / (f(3) - f(0)), (f(1) - f(3)) / (f(0) - f(3))
    acc = np.array([(up + f(1)) + f(1), (f(0) + down) + f(0), (f(1) + f(1)) + up], f)
    want = f(-1.5) + ((f(0) + f(0.5)) + acc / f(3)) * f(1.5)
    assert vertices[0].tolist() == want.tolist()
    length = np.sqrt((f(3) * f(3) + f(-3) * f(-3)) + f(3) * f(3))          # g = (3, -3, 3): towards the inside corner
    assert normals[0].tolist() == [-(f(3) / length), -(f(-3) / length), -(f(3) / length)]
    assert R.surface_nets(np.zeros((2, 2, 2), np.float32), 1.0, R.CENTER, R.RADIUS)[0].shape == (0, 3)


def test_special_values_and_uniform_lattices():
    S = R.special_lattice(12)
    assert np.isnan(S).any() and np.isposinf(S).any() and np.isneginf(S).any()
    vertices, normals, cube, faces = _nets(S)
    assert vertices.shape[0] > 0 and faces.shape[0] > 0
    assert np.isfinite(vertices).all() and np.isfinite(normals).all()
    lo, hi = -1.5 + 0.5 * 0.25, 1.5 - 0.5 * 0.25                            # every vertex lies inside its cube
    assert vertices.min() >= lo - 1e-6 and vertices.max() <= hi + 1e-6
    zero = (normals == 0).all(1)
    assert zero.any() and not zero.all()                                    # a NaN / inf gradient gives the zero normal
    for fill in (0.0, 5.0, np.nan, np.inf, -np.inf):                        # all outside / all inside: nothing
        out = _nets(np.full((6, 6, 6), fill, np.float32))
        assert [a.shape[0] for a in out] == [0, 0, 0, 0], fill
    # a NaN node is outside, whatever the threshold
    S = np.full((4, 4, 4), np.nan, np.float32)
    S[1:3, 1:3, 1:3] = 2.0
    assert R.surface_nets(S, -5.0, R.CENTER, R.RADIUS)[0].shape[0] == 26          # 27 cubes, the middle one all inside


# ---- the library's boundary ---------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entries():
    from ced_nerf_amd import _lib
    names = _lib.header_symbols()
    raw = C.CDLL(_lib.LIB_PATH)
    assert "mesh.hip" in _lib.SOURCES
    for n in ENTRIES:
        assert n in names, f"{n} not declared in include/cednerf_hip.h"
        assert n in _lib.PROTOTYPES, f"{n} not bound in _lib.PROTOTYPES"
        assert hasattr(raw, n), f"{n} declared but not exported by the built library"


def test_argument_errors_are_codes():
    from ced_nerf_amd import _lib
    L = _lib.lib()
    err = lambda: L.ced_last_error_string()
    assert L.ced_mesh_workspace_bytes(0) == -1 and L.ced_mesh_workspace_bytes(513) == -1
    assert L.ced_mesh_workspace_bytes(1) == 8 and L.ced_mesh_workspace_bytes(8) == 16         # 3 * 512 edges: 2 workgroups
    assert L.ced_mesh_workspace_bytes(512) == 8 * ((3 * 512 ** 3 + 1023) // 1024)
    c = (C.c_float * 3)(0, 0, 0)
    vert = lambda reso, radius=1.0, lattice=64, cap=0, count=64, wsb=1 << 20, center=c: \
        L.ced_mesh_vertices(reso, center, radius, lattice, 1.0, cap, None, None, None, count, 64, wsb, None)
    assert vert(0) == -1 and b"reso" in err()
    assert vert(513) == -1 and b"reso" in err()
    assert vert(4, center=None) == -1 and b"center" in err()
    assert vert(4, radius=0.0) == -1 and b"radius" in err()
    assert vert(4, radius=float("nan")) == -1 and b"radius" in err()
    assert vert(4, lattice=None) == -1 and b"lattice" in err()
    assert vert(4, count=None) == -1 and b"count" in err()
    assert vert(4, cap=8) == -1 and b"null output" in err()
    assert vert(8, wsb=8) == -1 and b"workspace" in err()
    face = lambda reso, lattice=64, cube=64, n_v=4, cap=0, count=64, wsb=1 << 20: \
        L.ced_mesh_faces(reso, lattice, 1.0, cube, n_v, cap, None, count, 64, wsb, None)
    assert face(0) == -1 and b"reso" in err()
    assert face(513) == -1 and b"reso" in err()
    assert face(4, lattice=None) == -1 and b"lattice" in err()
    assert face(4, n_v=-1) == -1 and b"n_vertices" in err()
    assert face(4, n_v=65) == -1 and b"n_vertices" in err()
    assert face(4, count=None) == -1 and b"count" in err()
    assert face(4, cap=8) == -1 and b"null pointer" in err()
    assert face(8, wsb=8) == -1 and b"workspace" in err()


# ---- the host API ---------------------------------------------------------------------------------------------------------
def _mesh(v=5, f=4, d=2, with_rgb=True):
    g = torch.Generator().manual_seed(8)
    mesh = dict(vertices=torch.randn(v, 3, generator=g), normals=torch.randn(v, 3, generator=g),
                faces=torch.randint(0, max(v, 1), (f, 3), generator=g, dtype=torch.int32), cube=torch.arange(v) * 5,
                sigma=torch.rand(v, generator=g) * 9, embedding=torch.randn(v, 15, generator=g), reso=12,
                center=[0.0, 0.5, 0.0], radius=1.5, t=0.25, sigma_thresh=2.5, apply_act=False)
    if with_rgb:
        mesh["rgb"] = torch.randn(v, d, 3, generator=g)
    return mesh


def test_mesh_ply_header_and_records(tmp_path):
    from ced_nerf_amd import export as E
    assert E.MESH_PLY_VERTEX.size == 27 and E.MESH_PLY_FACE.size == 13
    for with_rgb in (True, False):
        mesh = _mesh(5, 4, 2, with_rgb)
        path = tmp_path / f"m{int(with_rgb)}.ply"
        E.save_mesh_ply(str(path), mesh)
        head, _, body = path.read_bytes().partition(b"end_header\n")
        lines = head.decode("ascii").splitlines()
        assert lines[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 5"]
        assert lines[3:] == ["property float x", "property float y", "property float z", "property float nx",
                             "property float ny", "property float nz", "property uchar red", "property uchar green",
                             "property uchar blue", "element face 4", "property list uchar int vertex_indices"]
        assert len(body) == 5 * 27 + 4 * 13
        for i, rec in enumerate(struct.iter_unpack("<ffffffBBB", body[:5 * 27])):
            assert list(rec[:3]) == mesh["vertices"][i].tolist() and list(rec[3:6]) == mesh["normals"][i].tolist()
            if with_rgb:
                want = np.rint(255.0 * torch.sigmoid(mesh["rgb"][i].double()).mean(0).numpy())
                assert list(rec[6:9]) == want.astype(int).tolist()
            else:
                assert rec[6:9] == (128, 128, 128)
        for i, rec in enumerate(struct.iter_unpack("<Biii", body[5 * 27:])):
            assert rec[0] == 3 and list(rec[1:]) == mesh["faces"][i].tolist()
    # a mesh extracted with apply_act holds colours already
    mesh = _mesh(3, 1, 2)
    mesh["rgb"], mesh["apply_act"] = torch.full((3, 2, 3), 0.5), True
    E.save_mesh_ply(str(tmp_path / "act.ply"), mesh)
    body = (tmp_path / "act.ply").read_bytes().partition(b"end_header\n")[2]
    assert all(rec[6:9] == (128, 128, 128) for rec in struct.iter_unpack("<ffffffBBB", body[:3 * 27]))
    # an empty mesh is a header alone
    E.save_mesh_ply(str(tmp_path / "empty.ply"), _mesh(0, 0, 2))
    assert (tmp_path / "empty.ply").read_bytes() == E.mesh_ply_header(0, 0)


def test_mesh_npz_round_trip(tmp_path):
    from ced_nerf_amd import export as E
    arrays = ("vertices", "normals", "faces", "cube", "sigma", "embedding")
    for with_rgb in (True, False):
        mesh = _mesh(6, 7, 3, with_rgb)
        path = str(tmp_path / f"m{int(with_rgb)}.npz")
        E.save_mesh_npz(path, mesh)
        with np.load(path) as z:
            assert set(z.files) == set(arrays) | {"reso", "center", "radius", "t", "sigma_thresh", "apply_act"} | \
                ({"rgb"} if with_rgb else set())
            for k in arrays + (("rgb",) if with_rgb else ()):
                assert z[k].dtype == mesh[k].numpy().dtype and np.array_equal(z[k], mesh[k].numpy()), k
            assert z["faces"].dtype == np.int32 and z["cube"].dtype == np.int64
            assert int(z["reso"]) == 12 and z["center"].tolist() == [0.0, 0.5, 0.0] and float(z["sigma_thresh"]) == 2.5
            assert float(z["radius"]) == 1.5 and float(z["t"]) == 0.25 and not bool(z["apply_act"])


def test_cli_accepts_the_mesh_flags():
    from ced_nerf_amd import export as E
    p = E.make_parser()
    base = ["--load_model", "m.pth", "--preset", "dnerf", "--out", "o"]
    a = p.parse_args(base)
    assert a.mesh is False and a.mesh_dirs == "normal"
    a = p.parse_args(base + ["--mesh"])
    assert a.mesh is True and a.mesh_dirs == "normal"
    a = p.parse_args(base + ["--mesh", "--mesh_dirs", "6"])
    assert a.mesh and a.mesh_dirs == 6
    assert p.parse_args(base + ["--mesh", "--mesh_dirs", "normal"]).mesh_dirs == "normal"
    assert p.parse_args(base + ["--mesh", "--mesh_dirs", "0"]).mesh_dirs == 0
    for bad in ("-1", "tangent", "2.5"):
        with pytest.raises(SystemExit):
            p.parse_args(base + ["--mesh", "--mesh_dirs", bad])


def _cpu_field():
    from ced_nerf_amd.model import DNGPradianceField
    return DNGPradianceField(aabb=[-1.5, -1, -0.5, 1.5, 1, 0.5], log2_hashmap_size=12, dst_resolution=64, seed=0)


def test_invalid_arguments_and_cpu_inputs_are_refused():
    from ced_nerf_amd import export as E, ops
    f = _cpu_field()
    for reso in (0, 513, -1, 3.5, True):
        with pytest.raises(ValueError, match="reso"):
            E.extract_mesh(f, 0.0, reso=reso)
        with pytest.raises(ValueError, match="reso"):
            E.extract_mesh_sequence(f, [0.0, 1.0], reso=reso)
    with pytest.raises(ValueError, match="radius"):
        E.extract_mesh(f, 0.0, reso=4, radius=0.0)
    with pytest.raises(ValueError, match="dirs"):
        E.extract_mesh(f, 0.0, reso=4, dirs="tangent")
    with pytest.raises(ValueError, match="dirs"):
        E.extract_mesh(f, 0.0, reso=4, dirs=torch.ones(4, 2))
    with pytest.raises(ValueError, match="max_cells_per_launch"):
        E.extract_mesh(f, 0.0, reso=4, max_cells_per_launch=0)
    for dirs in (None, "normal", torch.ones(2, 3)):
        with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
            E.extract_mesh(f, 0.0, reso=4, dirs=dirs)
        with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
            E.extract_mesh_sequence(f, [0.0, 1.0], reso=4, dirs=dirs)
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        ops.mesh_surface_nets(torch.zeros(4, 4, 4), 1.0, [0, 0, 0], 1.5)
