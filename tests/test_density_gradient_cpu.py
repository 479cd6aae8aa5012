"""CPU suite: the derivative of the density -- the two entries' declarations and refusals, the Python layer's argument
checks, the command line, and the float64 reference of the GPU suite (tests/density64.py) pinned against torch.autograd on
tests/field64.py (plain tables) and against a central difference of its own primal (temporal table).  No kernel is
launched here."""
import functools

import numpy as np
import pytest
import torch

import density64 as D
import field64 as F
import warp64 as W

AABB = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
ENTRIES = ("ced_field_density_gradient", "ced_field_density_gradient_rays")


def _cpu_field():
    from ced_nerf_amd import synthetic as S
    from ced_nerf_amd.model import DNGPradianceField
    p = S.init_field_params([-1, -1, -1, 1, 1, 1], 1.0 / 32, 256, 10, use_div_offsets=True)
    return DNGPradianceField.from_params(p, "cpu").eval()


@functools.lru_cache(maxsize=None)
def _params(tm, table="f32", max_res=256):
    from ced_nerf_amd import synthetic as S
    return S.init_field_params(list(AABB), 1.0 / 32, hash_max_res=max_res, log2_hashmap_size=15, use_div_offsets=tm != 0,
                               use_time_embedding=tm != 0, use_time_attenuation=tm == 2, regime="trained",
                               table_dtype=np.float16 if table == "f16" else np.float32, temporal_hash=table == "temporal")


def _inputs(n=512):
    rng = np.random.default_rng(7)
    x = rng.uniform(0.0, 1.0, size=(n, 3)).astype(np.float32)
    t = rng.uniform(0.0, 1.0, size=(n,)).astype(np.float32)
    mn = rng.uniform(0.0, 0.05, size=(n,)).astype(np.float32)
    return x, t, mn


def test_the_library_declares_and_binds_the_two_entries():
    from ced_nerf_amd import _lib, ops
    names = _lib.header_symbols()
    for name in ENTRIES:
        assert name in names and name in _lib.PROTOTYPES
        assert hasattr(_lib.lib(), name)
    assert len(_lib.PROTOTYPES[ENTRIES[0]][1]) == 9
    # the rays entry: ced_field_move_rays' arguments up to t_per_ray, then the four outputs and the stream
    assert _lib.PROTOTYPES[ENTRIES[1]][1][:10] == _lib.PROTOTYPES["ced_field_move_rays"][1][:10]
    assert len(_lib.PROTOTYPES[ENTRIES[1]][1]) == 15
    assert callable(ops.field_density_gradient) and callable(ops.field_density_gradient_rays)
    assert "field_density_gradient.hip" in _lib.SOURCES
    assert ops.EXP15 == 3269017.25 == float(D.EXP15)


def test_library_refuses_bad_arguments():
    """a bad descriptor, n < 0, null inputs, no output, in that order; n == 0 is fine without pointers"""
    import ctypes as C
    from ced_nerf_amd import _lib
    L = _lib.lib()
    err = L.ced_last_error_string
    point = lambda ref, n, pos, t, *outs: L.ced_field_density_gradient(ref, n, pos, t, *outs, None)
    rays = lambda ref, n, *ptrs: L.ced_field_density_gradient_rays(ref, n, None, *ptrs[:6], 0, *ptrs[6:], None)
    assert point(None, 4, 1, 1, 1, 1, 1, 1) == -1 and b"field_density_gradient" in err()
    assert rays(None, 4, *([1] * 10)) == -1 and b"field_density_gradient_rays" in err()
    p = np.zeros(L.ced_packed_weight_words(0, 0, _lib.MLP_F32), np.float32)
    d = _lib.FieldDesc()
    d.packed_weights = p.ctypes.data            # never dereferenced: every call below fails or returns before a launch
    d.packed_floats = p.size
    ref = C.byref(d)
    d.mlp_precision = 7
    assert point(ref, -1, 1, 1, 1, 1, 1, 1) == -1 and b"mlp_precision" in err()
    assert rays(ref, -1, *([1] * 10)) == -1 and b"mlp_precision" in err()
    d.mlp_precision = _lib.MLP_F32
    assert point(ref, -1, 1, 1, 1, 1, 1, 1) == -1 and b"n < 0" in err()
    assert rays(ref, -1, *([1] * 10)) == -1 and b"n < 0" in err()
    # n == 0 needs no pointers
    assert point(ref, 0, None, None, None, None, None, None) == 0
    assert rays(ref, 0, *([None] * 10)) == 0
    # null inputs, then no output, then the hash table
    assert point(ref, 4, None, 1, 1, 1, 1, 1) == -1 and b"null" in err()
    assert point(ref, 4, 1, None, 1, 1, 1, 1) == -1 and b"null" in err()
    assert point(ref, 4, 1, 1, None, None, None, None) == -1 and b"no output" in err()
    for k in range(6):
        ptrs = [1] * 10
        ptrs[k] = None
        assert rays(ref, 4, *ptrs) == -1 and b"null" in err(), k
    assert rays(ref, 4, *([1] * 6 + [None] * 4)) == -1 and b"no output" in err()
    assert point(ref, 4, 1, 1, 1, None, None, None) == -1 and b"field_density_gradient" in err() and b"n_levels" in err()
    assert rays(ref, 4, *([1] * 6 + [None, None, 1, None])) == -1 and b"n_levels" in err()


def test_cpu_tensors_and_bad_arguments_are_refused():
    from ced_nerf_amd import ops, utils
    f = _cpu_field()
    x, t = torch.zeros(4, 3), torch.zeros(4)
    for call in (lambda: f.query_density_gradient(x, t), lambda: f.query_normals(x, t, canonical=True),
                 lambda: ops.field_density_gradient(None, x, t),
                 lambda: f.query_density_gradient_rays(x, x, torch.zeros(4, dtype=torch.int64), t, t, torch.zeros(1, 1))):
        with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
            call()
    assert ops.GRADIENT_OUTPUTS == ("sigma", "grad", "dlog", "dlog_canonical")
    assert callable(utils.render_normals)
    with pytest.raises(NotImplementedError, match="timestamps"):
        utils.render_normals(f, None, utils.Rays(origins=x, viewdirs=x))
    u = ops.unit_or_zero(torch.tensor([[3.0, 0.0, 4.0], [0.0, 0.0, 0.0]]))
    assert torch.equal(u, torch.tensor([[0.6, 0.0, 0.8], [0.0, 0.0, 0.0]]))


@pytest.mark.parametrize("bad", ["nonsense", "", None, True, 3])
def test_unknown_mesh_normals_are_a_value_error(bad):
    """on a CPU field: the value is checked before the device"""
    from ced_nerf_amd import export
    f = _cpu_field()
    with pytest.raises(ValueError, match="normals"):
        export.extract_mesh(f, 0.5, reso=8, normals=bad)
    with pytest.raises(ValueError, match="normals"):
        export.extract_mesh_sequence(f, [0.5], reso=8, normals=bad)
    if not isinstance(bad, bool):
        with pytest.raises(ValueError, match="normals"):
            export.extract_mesh_tracked(f, 0.5, [0.0], reso=8, normals=bad)
    for ok in export.MESH_NORMALS:
        with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
            export.extract_mesh(f, 0.5, reso=8, normals=ok)


def test_mesh_normals_flag():
    from ced_nerf_amd.export import make_parser
    base = ["--load_model", "m.pth", "--preset", "dnerf", "--out", "o"]
    assert make_parser().parse_args(base).mesh_normals == "lattice"
    assert make_parser().parse_args(base + ["--mesh", "--mesh_normals", "field"]).mesh_normals == "field"
    with pytest.raises(SystemExit):
        make_parser().parse_args(base + ["--mesh_normals", "smooth"])


# ---- the float64 model -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tm", [0, 1, 2])
@pytest.mark.parametrize("table,max_res", [("f32", 256), ("f16", 256), ("f32", 8192)])
def test_model_is_autograd_on_field64(tm, table, max_res):
    """mode None, float64, plain tables: raw and d raw / d x_norm of density64.base_gradient against field64's hash_encode
    (dx_scaled, fp32 position) + time_encode + mlp under torch.autograd, to 1e-9 of the largest magnitude"""
    params = _params(tm, table, max_res)
    x, t, mn = _inputs()
    raw, draw, pre = D.base_gradient(params, x, t, mn)
    assert raw.dtype == np.float64 and draw.shape == (len(x), 3) and len(pre) == 1 and pre[0].shape == (len(x), 64)
    P = F.make_params(params, torch.float64)
    cfg = {k: v for k, v in params["hash"].items() if k != "table"}
    xt = torch.from_numpy(x).double().requires_grad_()
    t1 = torch.from_numpy(t).double()[:, None]
    feat = F.hash_encode(xt, P["hash_table"], cfg, t1[:, 0])
    if tm:
        feat = torch.cat([feat, F.time_encode(t1) if tm == 1 else F.time_encode(t1, torch.from_numpy(mn).double()[:, None])], -1)
    out = F.mlp(feat, F._group(P, "mlp_base"))[:, 0]
    (g,) = torch.autograd.grad(out.sum(), xt)
    err_raw = float(np.abs(raw - out.detach().numpy()).max()) / float(np.abs(raw).max())
    err = float(np.abs(draw - g.numpy()).max()) / float(np.abs(draw).max())
    print(f"density64 against autograd [tm={tm} {table} max_res={max_res}]: raw {err_raw:.2e}, d raw / d x_norm {err:.2e} "
          f"(relative to max |raw| = {float(np.abs(raw).max()):.3g}, max |d raw| = {float(np.abs(draw).max()):.3g})")
    assert err_raw <= 1e-9 and err <= 1e-9
    assert float(np.abs(draw).max()) > 1.0


@pytest.mark.parametrize("tm", [0, 2])
def test_temporal_model_is_the_difference_of_its_own_primal(tm):
    """temporal table (the reference has no dx there): with the exact fraction the primal is smooth inside a cell, and
    d raw / d x_norm is its central difference (h = 1e-7) on the rows whose stencil stays in every level's cell and whose
    hidden pre-activations stay clear of zero"""
    params = _params(tm, "temporal")
    x, t, mn = _inputs()
    x = x.astype(np.float64)
    h = 1e-7
    raw, draw, pre = D.base_gradient(params, x, t, mn, exact_fraction=True)
    keep = W.kept_rows(pre)
    scales = D.levels_of(params)["scale"].astype(np.float64)
    worst = 0.0
    for a in range(3):
        e = np.zeros(3); e[a] = h
        same = np.ones(len(x), bool)
        for s in scales:
            same &= (np.floor((x + e) * s + 0.5) == np.floor((x - e) * s + 0.5)).all(-1)
        hi = D.base_gradient(params, x + e, t, mn, exact_fraction=True)
        lo = D.base_gradient(params, x - e, t, mn, exact_fraction=True)
        rows = keep & same & W.kept_rows(hi[2]) & W.kept_rows(lo[2])
        assert rows.mean() > 0.9
        fd = (hi[0] - lo[0]) / (2 * h)
        worst = max(worst, float(np.abs(fd - draw[:, a])[rows].max()) / float(np.abs(draw).max()))
    print(f"temporal density64 against its central difference [tm={tm}]: {worst:.2e} of max |d raw| = {float(np.abs(draw).max()):.3g}")
    assert worst <= 1e-6
    # and the fp32 fraction only moves the point inside its cell: same cells, nearly the same derivative
    draw32 = D.base_gradient(params, x.astype(np.float32), t, mn)[1]
    assert np.isfinite(draw32).all()


def test_rounded_models_and_the_world_lines():
    """the mode-rounded models stay near the exact one; world_gradients states the header's lines in the inputs' dtype"""
    params = _params(2)
    x, t, mn = _inputs(256)
    exact = D.base_gradient(params, x, t, mn)[1]
    scale = float(np.abs(exact).max())
    for mode in ("f32", "f16x2", "f16"):
        for dtype in (np.float64, np.float32):
            got = D.base_gradient(params, x, t, mn, dtype, mode)
            assert got[1].dtype == dtype
            dist = np.abs(got[1] - exact)[W.kept_rows(got[2])]
            if mode == "f16":                   # a float16 has 11 bits and a few ReLU masks differ: typical, not worst, distance
                assert float(np.median(dist)) <= 1e-3 * scale, dtype
            else:
                assert float(dist.max()) <= 1e-5 * scale, (mode, dtype)
    rng = np.random.default_rng(3)
    dc = rng.normal(size=(5, 3)).astype(np.float32)
    J = (rng.normal(size=(5, 3, 4)) * 0.1).astype(np.float32)
    sigma = np.asarray([0.0, 1.0, 1e3, 4e6, 1e9], np.float32)
    dlog, grad = D.world_gradients(dc, J, sigma)
    assert dlog.dtype == grad.dtype == np.float32
    want = dc.astype(np.float64) + np.einsum("nab,na->nb", J[:, :, :3].astype(np.float64), dc.astype(np.float64))
    assert np.abs(dlog - want).max() <= 1e-6
    assert np.array_equal(grad[3], D.EXP15 * dlog[3]) and np.array_equal(grad[2], np.float32(1e3) * dlog[2]) and not grad[0].any()
    assert D.tangent_log2(params) == 8 and D.tangent_log2(_params(0, "f32", 8192)) == 13
