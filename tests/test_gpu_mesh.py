"""GPU suite: the mesh export (csrc/mesh.hip, ops.mesh_surface_nets, export.extract_mesh) against tests/mesh_reference.py,
the numpy float32 restatement of the definition in include/cednerf_hip.h.  Every comparison is torch.equal: the kernels
are deterministic (order-preserving compactions, no atomics) and every operation of the definition is one float32 rounding.

Lattices: reso 12 (1 728 nodes: a partial last wave and workgroup), reso 20 (8 000 nodes: several compaction workgroups,
the last one partial) and noise at reso 48, whose 331 776 edge items make the scan of the workgroup counts span several
waves.  Fields, modes and flags are tests/test_gpu_export.py's (its cached fields and densities are reused)."""
import numpy as np
import pytest
import torch

import mesh_reference as R
from test_gpu_export import DEV, FLAGS, MODES, T, _density, _dirs, _estimator, _field, _mask_restatement

pytestmark = pytest.mark.gpu

MESH_KEYS = ("vertices", "normals", "cube", "faces")
LATTICES = {"sphere": R.sphere_lattice, "torus": R.torus_lattice, "noise": R.noise_lattice,
            "open_noise": lambda reso: R.noise_lattice(reso, closed=False), "special": R.special_lattice}


def _assert_is_reference(got, S, thresh, center=R.CENTER, radius=R.RADIUS, what=""):
    """got: (vertices, normals, cube, faces) tensors or a mesh dict; S: the lattice as numpy"""
    if isinstance(got, dict):
        got = tuple(got[k] for k in MESH_KEYS)
    want = R.surface_nets(S, thresh, center, radius)
    for k, g, w in zip(MESH_KEYS, got, want):
        w = T(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert torch.equal(g, w), (what, k, int((g != w).sum()))
    return want


def _nets(S, thresh=R.THRESH):
    from ced_nerf_amd import ops
    with torch.cuda.device(0):
        return ops.mesh_surface_nets(T(S), thresh, R.CENTER, R.RADIUS)


@pytest.mark.parametrize("reso", [12, 20])
@pytest.mark.parametrize("name", sorted(LATTICES))
def test_surface_nets_is_the_reference(name, reso):
    S = LATTICES[name](reso)
    got = _nets(S)
    want = _assert_is_reference(got, S, R.THRESH, what=(name, reso))
    print(f"{name} reso {reso}: V = {want[0].shape[0]}, F = {want[3].shape[0]}")
    assert want[0].shape[0] > 0 and want[3].shape[0] > 0
    assert got[3].dtype == torch.int32 and got[2].dtype == torch.int64
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())


def test_surface_nets_across_many_workgroups():
    """noise at reso 48: 110 592 cube items (108 workgroup counts) and 331 776 edge items (324 counts, several scan
    waves); about 100 000 vertices, so a face's binary search runs 17 steps deep"""
    S = R.noise_lattice(48)
    want = _assert_is_reference(_nets(S), S, R.THRESH, what="noise 48")
    print(f"noise reso 48: V = {want[0].shape[0]}, F = {want[3].shape[0]}")
    assert want[0].shape[0] > 50_000 and want[3].shape[0] > 100_000


def test_degenerate_and_empty_lattices():
    for S in (np.full((1, 1, 1), 2.0, np.float32), np.zeros((1, 1, 1), np.float32)):
        got = _nets(S)
        assert [tuple(g.shape) for g in got] == [(0, 3), (0, 3), (0,), (0, 3)]
    S = np.zeros((2, 2, 2), np.float32)
    S[1, 0, 1] = 3.0
    got = _nets(S)
    _assert_is_reference(got, S, R.THRESH, what="reso 2")
    assert got[0].shape == (1, 3) and got[3].shape == (0, 3)
    _assert_is_reference(_nets(np.full((2, 2, 2), 2.0, np.float32)), np.full((2, 2, 2), 2.0, np.float32), R.THRESH)
    # all outside, all inside, all NaN: counts of 0, no launch failure, typed empty outputs on the device
    for fill in (0.0, 5.0, float("nan")):
        got = _nets(np.full((12, 12, 12), fill, np.float32))
        assert [tuple(g.shape) for g in got] == [(0, 3), (0, 3), (0,), (0, 3)], fill
        assert [g.dtype for g in got] == [torch.float32, torch.float32, torch.int64, torch.int32]
        assert all(g.is_cuda for g in got)
    torch.cuda.synchronize()
    # a threshold other than 1, a cube other than the default
    from ced_nerf_amd import ops
    S = R.noise_lattice(12, closed=False)
    with torch.cuda.device(0):
        got = ops.mesh_surface_nets(T(S), 0.37, [0.1, -2.0, 3.0], 0.7)
    _assert_is_reference(got, S, 0.37, (0.1, -2.0, 3.0), 0.7, "shifted cube")


def _expected_rgb(f, mesh, dirs, act):
    v = mesh["vertices"].shape[0]
    emb = mesh["embedding"]
    if isinstance(dirs, str):
        n = mesh["normals"]
        head_on = torch.where((n == 0).all(-1, keepdim=True), torch.tensor([0.0, 0.0, 1.0], device=DEV), -n)
        return f._query_rgb(head_on[:, None], emb[:, None], act)
    d = dirs.shape[0]
    return f._query_rgb(dirs[None].expand(v, d, 3), emb[:, None].expand(v, d, 15), act)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("div,tm", FLAGS)
def test_extract_mesh_is_the_reference_on_query_density(div, tm, mode):
    """The lattice is query_density on voxel_centers, the iso-value its median (both outcomes occur): the mesh arrays are
    the reference's, sigma / embedding are query_density on the vertices, rgb is _query_rgb on the expanded inputs for
    D = 1, D = 3 and "normal", the sigmoid on and off."""
    from ced_nerf_amd.export import extract_mesh
    f = _field(div, tm, mode)
    t = 0.37
    for reso in (12, 20):
        _, sig, _ = _density(div, tm, mode, reso, t)
        thresh = float(sig.median())
        S = sig.cpu().numpy().reshape(reso, reso, reso)
        want = None
        for dirs, act in ((_dirs(1), True), (_dirs(1), False), (_dirs(3), True), (_dirs(3), False), ("normal", True),
                          ("normal", False), (None, False)):
            mesh = extract_mesh(f, t, reso=reso, sigma_thresh=thresh, dirs=dirs, apply_act=act)
            v, n_f = mesh["vertices"].shape[0], mesh["faces"].shape[0]
            if want is None:
                print(f"[{mode} div={div} tm={tm}] reso {reso}: thresh {thresh:.4g}, V = {v}, F = {n_f}")
                assert v > 0 and n_f > 0
                want = _assert_is_reference(mesh, S, thresh, what=(reso, "mesh"))
                res = f.query_density(mesh["vertices"], torch.full((v, 1), t, device=DEV), return_feat=True)
                want_sigma, want_emb = res["density"][:, 0], res["base_mlp_out"]
            for k, w in zip(MESH_KEYS, want):
                assert torch.equal(mesh[k], T(w)), (reso, k)
            assert mesh["sigma"].shape == (v,) and torch.equal(mesh["sigma"], want_sigma)
            assert mesh["embedding"].shape == (v, 15) and torch.equal(mesh["embedding"], want_emb)
            if dirs is None:
                assert "rgb" not in mesh
            else:
                d = 1 if isinstance(dirs, str) else dirs.shape[0]
                assert mesh["rgb"].shape == (v, d, 3) and mesh["rgb"].dtype == torch.float32
                assert torch.equal(mesh["rgb"], _expected_rgb(f, mesh, dirs, act)), (reso, d, act)
                if not act:
                    assert bool((mesh["rgb"] < 0).any() | (mesh["rgb"] > 1).any())
            assert mesh["reso"] == reso and mesh["t"] == t and mesh["sigma_thresh"] == thresh and mesh["apply_act"] == act
            assert mesh["radius"] == 1.5 and mesh["center"] == [0.0, 0.0, 0.0]


def _masked_lattice(sig, P, est, reso):
    """the densities with the nodes the estimator's grid does not mark set to 0"""
    keep = _mask_restatement(P, est.binaries, est.aabbs)
    assert 0 < int(keep.sum()) < reso ** 3
    return torch.where(keep, sig, torch.zeros_like(sig)), keep


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
def test_extract_mesh_with_an_occupancy_grid(mode):
    """Only marked cells are evaluated, the others hold density 0; slabs of 1 000 cells (no multiple of a workgroup's
    1 024) give the same mesh; the sequence is the single calls."""
    from ced_nerf_amd.export import extract_mesh, extract_mesh_sequence
    f = _field(True, 2, mode)
    est = _estimator((-0.75, -0.75, -0.75, 0.75, 0.75, 0.75), (0.6, 0.4), 5)
    keys = MESH_KEYS + ("sigma", "embedding", "rgb")
    for reso in (12, 20):
        t = 0.37
        P, sig, _ = _density(True, 2, mode, reso, t)
        lattice, keep = _masked_lattice(sig, P, est, reso)
        thresh = float(sig[keep].median())
        kw = dict(reso=reso, sigma_thresh=thresh, dirs="normal", estimator=est)
        mesh = extract_mesh(f, t, **kw)
        print(f"[{mode}] grid, reso {reso}: thresh {thresh:.4g}, V = {mesh['vertices'].shape[0]}, "
              f"F = {mesh['faces'].shape[0]}")
        assert thresh > 0 and mesh["vertices"].shape[0] > 0 and mesh["faces"].shape[0] > 0
        _assert_is_reference(mesh, lattice.cpu().numpy().reshape(reso, reso, reso), thresh, what=("grid", reso))
        # ... which is not the mesh of the unmasked lattice
        assert mesh["vertices"].shape != extract_mesh(f, t, reso=reso, sigma_thresh=thresh)["vertices"].shape
        slabs = extract_mesh(f, t, max_cells_per_launch=1000, **kw)
        for k in keys:
            assert torch.equal(slabs[k], mesh[k]), (reso, k)
    times = [0, 0.37, 1]
    seq = extract_mesh_sequence(f, times, **kw)
    assert len(seq) == 3 and [m["t"] for m in seq] == [0.0, 0.37, 1.0]
    for tt, m in zip(times, seq):
        one = extract_mesh(f, tt, **kw)
        for k in keys:
            assert m[k].shape == one[k].shape and torch.equal(m[k], one[k]), (tt, k)
    assert seq[0]["vertices"].shape != seq[2]["vertices"].shape or not torch.equal(seq[0]["vertices"], seq[2]["vertices"])


def _read_mesh_ply(path):
    head, _, body = path.read_bytes().partition(b"end_header\n")
    lines = head.decode("ascii").splitlines()
    v = int(next(l for l in lines if l.startswith("element vertex")).split()[-1])
    n_f = int(next(l for l in lines if l.startswith("element face")).split()[-1])
    assert len(body) == 27 * v + 13 * n_f
    vrec = np.frombuffer(body[:27 * v], dtype=np.dtype([("xyz", "<f4", 3), ("normal", "<f4", 3), ("rgb", "u1", 3)]))
    frec = np.frombuffer(body[27 * v:], dtype=np.dtype([("n", "u1"), ("ids", "<i4", 3)]))
    assert (frec["n"] == 3).all()
    return vrec, frec


def test_files_of_a_gpu_mesh_read_back(tmp_path):
    from ced_nerf_amd import export as E
    f = _field(True, 2, "f32")
    _, sig, _ = _density(True, 2, "f32", 20, 0.37)
    for dirs, act in ((_dirs(3), False), ("normal", True), (None, False)):
        mesh = E.extract_mesh(f, 0.37, reso=20, sigma_thresh=float(sig.median()), dirs=dirs, apply_act=act)
        assert mesh["faces"].shape[0] > 0
        E.save_mesh_npz(str(tmp_path / "m.npz"), mesh)
        with np.load(tmp_path / "m.npz") as z:
            for k in MESH_KEYS + ("sigma", "embedding") + (("rgb",) if dirs is not None else ()):
                assert z[k].dtype == mesh[k].cpu().numpy().dtype and np.array_equal(z[k], mesh[k].cpu().numpy()), k
            assert ("rgb" in z.files) == (dirs is not None)
            assert int(z["reso"]) == 20 and bool(z["apply_act"]) == act
        E.save_mesh_ply(str(tmp_path / "m.ply"), mesh)
        vrec, frec = _read_mesh_ply(tmp_path / "m.ply")
        assert np.array_equal(vrec["xyz"], mesh["vertices"].cpu().numpy())
        assert np.array_equal(vrec["normal"], mesh["normals"].cpu().numpy())
        assert np.array_equal(frec["ids"], mesh["faces"].cpu().numpy())
        if dirs is None:
            assert (vrec["rgb"] == 128).all()
        else:
            rgb = mesh["rgb"].double() if act else torch.sigmoid(mesh["rgb"].double())
            assert np.array_equal(vrec["rgb"], np.rint(255.0 * rgb.mean(1).cpu().numpy()).astype(np.uint8))


def test_cli_writes_meshes_next_to_the_volumes(tmp_path):
    """--mesh adds mesh_%04d.npz / .ply per time, equal to extract_mesh on the modules the checkpoint was saved from; the
    volumes are written either way and no mesh without the flag."""
    from ced_nerf_amd import export as E, trainer
    cfg = trainer.resolve_config("dnerf", None, log2_hashmap_size=14)
    flags = dict(use_div_offsets=True, use_time_embedding=True)
    field, est = trainer.build_modules(cfg, torch.device(DEV), **flags)
    est.set_binaries(T(np.random.default_rng(4).uniform(size=tuple(est.binaries.shape)) < 0.5))
    path = str(tmp_path / "model.pth")
    torch.save({"radiance_field": field.state_dict(), "occupancy_grid": est.state_dict()}, path)
    thresh = 1e-6                                         # the surface is the boundary of the grid's marked cells
    argv = ["--load_model", path, "--preset", "dnerf", "--log2_hashmap_size", "14", "-df", "-te", "--times", "0,0.5",
            "--reso", "16", "--sigma_thresh", "1e-6", "--device", DEV]
    plain, meshed = tmp_path / "plain", tmp_path / "meshed"
    assert E.main(argv + ["--out", str(plain)]) == 0
    assert E.main(argv + ["--out", str(meshed), "--mesh", "--mesh_dirs", "4"]) == 0
    names = ["volume_0000.npz", "volume_0000.ply", "volume_0001.npz", "volume_0001.ply"]
    assert sorted(p.name for p in plain.iterdir()) == names
    assert sorted(p.name for p in meshed.iterdir()) == ["mesh_0000.npz", "mesh_0000.ply", "mesh_0001.npz",
                                                        "mesh_0001.ply"] + names
    for name in names[1::2]:
        assert (plain / name).read_bytes() == (meshed / name).read_bytes()
    dirs = T(E.fibonacci_dirs(4))
    for i, t in enumerate((0.0, 0.5)):
        want = E.extract_mesh(field, t, reso=16, sigma_thresh=thresh, dirs=dirs, estimator=est)
        with np.load(meshed / f"mesh_{i:04d}.npz") as z:
            for k in MESH_KEYS + ("sigma", "embedding", "rgb"):
                assert np.array_equal(z[k], want[k].cpu().numpy()), k
            assert int(z["reso"]) == 16 and float(z["t"]) == t
        vrec, frec = _read_mesh_ply(meshed / f"mesh_{i:04d}.ply")
        assert np.array_equal(vrec["xyz"], want["vertices"].cpu().numpy())
        assert np.array_equal(frec["ids"], want["faces"].cpu().numpy())
        assert want["vertices"].shape[0] > 0 and want["faces"].shape[0] > 0
