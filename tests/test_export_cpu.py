"""CPU suite: the volume export's boundary (csrc/bake.hip, ced_field_rgb_bcast, ced_nerf_amd/export.py) -- the entries
are declared, bound and exported and refuse bad arguments with codes; voxel_centers by hand; the file writers; the
argument checks of bake_volume and the command line's parser.  No kernel is launched here."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

ENTRIES = ("ced_bake_workspace_bytes", "ced_bake_candidates", "ced_bake_select", "ced_field_rgb_bcast")


def test_header_declares_and_library_exports_the_entries():
    from ced_nerf_amd import _lib
    names = _lib.header_symbols()
    raw = C.CDLL(_lib.LIB_PATH)
    assert "bake.hip" in _lib.SOURCES
    for n in ENTRIES:
        assert n in names, f"{n} not declared in include/cednerf_hip.h"
        assert n in _lib.PROTOTYPES, f"{n} not bound in _lib.PROTOTYPES"
        assert hasattr(raw, n), f"{n} declared but not exported by the built library"


def test_argument_errors_are_codes():
    from ced_nerf_amd import _lib
    L = _lib.lib()
    err = lambda: L.ced_last_error_string()
    assert L.ced_bake_workspace_bytes(-1) == -1 and L.ced_bake_workspace_bytes(0) == 8
    assert L.ced_bake_workspace_bytes(1024) == 8 and L.ced_bake_workspace_bytes(1025) == 16
    c = (C.c_float * 3)(0, 0, 0)
    cand = lambda reso, radius, first, n, cap=0, count=64, ws=64, wsb=1 << 20, binaries=None, aabbs=None, res=0: \
        L.ced_bake_candidates(reso, c, radius, first, n, binaries, aabbs, 2 if binaries else 0, res, cap, None, None, count,
                              ws, wsb, None)
    assert cand(0, 1.0, 0, 0) == -1 and b"reso" in err()
    assert cand(4096, 1.0, 0, 0) == -1 and b"reso" in err()
    assert cand(4, 0.0, 0, 8) == -1 and b"radius" in err()
    assert cand(4, float("nan"), 0, 8) == -1 and b"radius" in err()
    assert cand(4, 1.0, 60, 5) == -1 and b"cells" in err()
    assert cand(4, 1.0, -1, 5) == -1 and b"cells" in err()
    assert cand(4, 1.0, 0, 64, count=None) == -1 and b"count" in err()
    assert cand(4, 1.0, 0, 64, cap=64) == -1 and b"null output" in err()
    assert cand(4, 1.0, 0, 64, wsb=4) == -1 and b"workspace" in err()
    assert cand(4, 1.0, 0, 64, binaries=64, aabbs=None, res=16) == -1 and b"grid" in err()
    assert cand(4, 1.0, 0, 64, binaries=64, aabbs=64, res=0) == -1 and b"grid" in err()
    sel = lambda n, cap=0, sigma=64, count=64, wsb=1 << 20: \
        L.ced_bake_select(n, None, None, sigma, None, 1.0, cap, None, None, None, None, count, 64, wsb, None)
    assert sel(-1) == -1 and b"n < 0" in err()
    assert sel(8, sigma=None) == -1 and b"sigma" in err()
    assert sel(8, cap=8) == -1 and b"null pointer" in err()
    assert sel(8, count=None) == -1 and b"count" in err()
    assert sel(5000, wsb=8) == -1 and b"workspace" in err()
    # the broadcast head: empty input is a no-op, errors name the entry
    d = _lib.FieldDesc()
    d.packed_weights = 64                    # never dereferenced: every call below fails, or returns, before a launch
    d.packed_floats = int(L.ced_packed_weight_words(0, 0, 0))
    assert L.ced_field_rgb_bcast(C.byref(d), 0, 3, None, None, 1, None, None) == 0
    assert L.ced_field_rgb_bcast(C.byref(d), 5, 0, None, None, 1, None, None) == 0
    assert L.ced_field_rgb_bcast(C.byref(d), 5, 3, 64, None, 1, 64, None) == -1 and b"field_rgb_bcast" in err()
    assert L.ced_field_rgb_bcast(C.byref(d), -1, 3, 64, 64, 1, 64, None) == -1 and b"field_rgb_bcast" in err()
    assert L.ced_field_rgb_bcast(None, 5, 3, 64, 64, 1, 64, None) == -1 and b"field_rgb_bcast" in err()
    d.packed_floats += 1
    assert L.ced_field_rgb_bcast(C.byref(d), 5, 3, 64, 64, 1, 64, None) == -1 and b"packed_floats" in err()


def test_voxel_centers_by_hand():
    from ced_nerf_amd.export import voxel_centers
    # reso 2 over [-1, 1]^3: centres at -0.5 / +0.5, z fastest
    got = voxel_centers(2, [0.0, 0.0, 0.0], 1.0, "cpu")
    want = [[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)]
    assert got.dtype == torch.float32 and got.shape == (8, 3) and got.tolist() == want
    # reso 3 over [1, 4] x [-1, 2] x [2, 5] (centre (2.5, 0.5, 3.5), radius 1.5): h = 1, centres lo + 0.5, 1.5, 2.5
    got = voxel_centers(3, [2.5, 0.5, 3.5], 1.5, "cpu")
    assert got.shape == (27, 3)
    want = [[1 + x, -1 + y, 2 + z] for x in (0.5, 1.5, 2.5) for y in (0.5, 1.5, 2.5) for z in (0.5, 1.5, 2.5)]
    assert got.tolist() == want
    assert got[(1 * 3 + 2) * 3 + 0].tolist() == [2.5, 1.5, 2.5]                 # i = (ix * reso + iy) * reso + iz
    # fp32 throughout, multiply then add: h = fl(2 * 0.3f / 3), p = fl(lo + fl(1.5f * h))
    got = voxel_centers(3, [0.1, 0.0, 0.0], 0.3, "cpu")
    r, c = np.float32(0.3), np.float32(0.1)
    h = (np.float32(2.0) * r) / np.float32(3.0)
    assert np.float32(got[9 + 3 + 1, 0].item()) == (c - r) + np.float32(1.5) * h
    for bad in (0, -3, 2.0, 4096):
        with pytest.raises(ValueError, match="reso"):
            voxel_centers(bad, [0, 0, 0], 1.0, "cpu")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="radius"):
            voxel_centers(2, [0, 0, 0], bad, "cpu")
    with pytest.raises(ValueError, match="center"):
        voxel_centers(2, [0, 0], 1.0, "cpu")


def _volume(m=5, d=2, with_rgb=True):
    g = torch.Generator().manual_seed(3)
    vol = dict(index=torch.arange(m) * 7, xyz=torch.randn(m, 3, generator=g), sigma=torch.rand(m, generator=g) * 9,
               embedding=torch.randn(m, 15, generator=g), reso=12, center=[0.0, 0.5, 0.0], radius=1.5, t=0.25,
               apply_act=False)
    if with_rgb:
        vol["rgb"] = torch.randn(m, d, 3, generator=g)
    return vol


def test_ply_header_and_records(tmp_path):
    from ced_nerf_amd import export as E
    assert E.PLY_RECORD.size == 19
    for with_rgb in (True, False):
        vol = _volume(5, 2, with_rgb)
        path = tmp_path / f"v{int(with_rgb)}.ply"
        E.save_ply(str(path), vol)
        raw = path.read_bytes()
        head, _, body = raw.partition(b"end_header\n")
        lines = head.decode("ascii").splitlines()
        assert lines[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 5"]
        assert lines[3:] == ["property float x", "property float y", "property float z", "property uchar red",
                             "property uchar green", "property uchar blue", "property float sigma"]
        assert len(body) == 5 * 19
        for i, rec in enumerate(struct.iter_unpack("<fffBBBf", body)):
            assert list(rec[:3]) == vol["xyz"][i].tolist() and rec[6] == vol["sigma"][i].item()
            if with_rgb:
                want = np.rint(255.0 * torch.sigmoid(vol["rgb"][i].double()).mean(0).numpy())
                assert list(rec[3:6]) == want.astype(int).tolist()
            else:
                assert rec[3:6] == (128, 128, 128)
    # a volume baked with apply_act holds colours already
    vol = _volume(3, 2)
    vol["rgb"], vol["apply_act"] = torch.full((3, 2, 3), 0.5), True
    E.save_ply(str(tmp_path / "act.ply"), vol)
    body = (tmp_path / "act.ply").read_bytes().partition(b"end_header\n")[2]
    assert all(rec[3:6] == (128, 128, 128) for rec in struct.iter_unpack("<fffBBBf", body))
    # an empty volume is a header alone
    E.save_ply(str(tmp_path / "empty.ply"), _volume(0, 2))
    assert (tmp_path / "empty.ply").read_bytes() == E.ply_header(0)
    with pytest.raises(ValueError, match="dirs_reduce"):
        E.save_ply(str(tmp_path / "x.ply"), _volume(), dirs_reduce="max")


def test_npz_round_trip(tmp_path):
    from ced_nerf_amd import export as E
    for with_rgb in (True, False):
        vol = _volume(6, 3, with_rgb)
        path = str(tmp_path / f"v{int(with_rgb)}.npz")
        E.save_npz(path, vol)
        with np.load(path) as z:
            assert set(z.files) == {"index", "xyz", "sigma", "embedding", "reso", "center", "radius", "t", "apply_act"} | \
                ({"rgb"} if with_rgb else set())
            for k in ("index", "xyz", "sigma", "embedding") + (("rgb",) if with_rgb else ()):
                assert z[k].dtype == vol[k].numpy().dtype and np.array_equal(z[k], vol[k].numpy()), k
            assert int(z["reso"]) == 12 and z["center"].tolist() == [0.0, 0.5, 0.0]
            assert float(z["radius"]) == 1.5 and float(z["t"]) == 0.25 and not bool(z["apply_act"])


def _cpu_field():
    from ced_nerf_amd.model import DNGPradianceField
    return DNGPradianceField(aabb=[-1.5, -1, -0.5, 1.5, 1, 0.5], log2_hashmap_size=12, dst_resolution=64, seed=0)


def test_cpu_inputs_are_refused():
    from ced_nerf_amd import _lib, export as E, ops
    f = _cpu_field()
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        E.bake_volume(f, 0.0, reso=4)
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        E.bake_sequence(f, [0.0, 1.0], reso=4, dirs=torch.ones(2, 3))
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        E.nerfvis_eval_fn(f, 0.0)(torch.zeros(4, 1, 3), torch.ones(1, 2, 3))
    d = _lib.FieldDesc()
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        ops.field_rgb_bcast(d, torch.ones(2, 3), torch.zeros(4, 15))
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        ops.bake_candidates(4, [0, 0, 0], 1.0, 0, 64, "cpu")
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        ops.bake_select(torch.zeros(4, dtype=torch.int64), torch.zeros(4, 3), torch.zeros(4), torch.zeros(4, 15), 1.0)


def test_invalid_arguments_are_value_errors():
    from ced_nerf_amd import export as E
    f = _cpu_field()
    for reso in (0, -1, 3.5, 5000):
        with pytest.raises(ValueError, match="reso"):
            E.bake_volume(f, 0.0, reso=reso)
    for radius in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="radius"):
            E.bake_volume(f, 0.0, reso=4, radius=radius)
    for dirs in (torch.ones(3), torch.ones(4, 2), torch.ones(2, 4, 3), torch.ones(0, 3)):
        with pytest.raises(ValueError, match="dirs"):
            E.bake_volume(f, 0.0, reso=4, dirs=dirs)
    with pytest.raises(ValueError, match="center"):
        E.bake_volume(f, 0.0, reso=4, center=[0.0, 1.0])
    with pytest.raises(ValueError, match="max_cells_per_launch"):
        E.bake_volume(f, 0.0, reso=4, max_cells_per_launch=0)
    with pytest.raises(ValueError, match="one-element"):
        E.nerfvis_eval_fn(f, torch.zeros(2))
    # the defaults are vis.py:40-41 on the field's box
    assert E._cube(f, None, None) == ([0.0, 0.0, 0.0], 1.5)
    assert E._cube(f, [1, 2, 3], 0.5) == ([1.0, 2.0, 3.0], 0.5)


def test_cli_arguments():
    from ced_nerf_amd import export as E
    p = E.make_parser()
    a = p.parse_args(["--load_model", "m.pth", "--preset", "hypernerf", "-df", "-te", "-ta", "-f", "-w", "--times",
                      "0,0.5,1", "--reso", "64", "--sigma_thresh", "2.5", "--n_dirs", "8", "--out", "vols"])
    assert a.load_model == "m.pth" and a.preset == "hypernerf" and a.out == "vols"
    assert a.use_div_offsets and a.use_time_embedding and a.use_time_attenuation and a.use_feat_predict
    assert a.use_weight_predict and a.times == [0.0, 0.5, 1.0] and a.reso == 64 and a.sigma_thresh == 2.5 and a.n_dirs == 8
    a = p.parse_args(["--load_model", "m.pth", "--preset", "dnerf", "--out", "o"])
    assert a.times == [0.0] and a.reso == 128 and a.sigma_thresh == 1.0 and a.n_dirs == 0
    assert not (a.use_div_offsets or a.use_time_embedding or a.use_time_attenuation or a.no_occupancy)
    for bad in (["--preset", "dnerf", "--out", "o"], ["--load_model", "m", "--preset", "llff", "--out", "o"],
                ["--load_model", "m", "--preset", "dnerf"], ["--load_model", "m", "--preset", "dnerf", "--out", "o",
                                                             "--times", "0,x"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    d = E.fibonacci_dirs(16)
    assert d.shape == (16, 3) and d.dtype == np.float32 and np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-6)
