"""GPU suite: the derivative of the density (csrc/field_density_gradient.hip: ced_field_density_gradient,
ced_field_density_gradient_rays) and what stands on it -- DNGPradianceField.query_density_gradient / query_normals /
query_density_gradient_rays, utils.render_normals, video.render_video(normals=True), export.extract_mesh(normals="field").

References: query_density for the primal's bits; include/cednerf_hip.h's last lines in numpy float32 on the kernel's own
dlog_canonical and query_move_jacobian's jac for the chain's bits; tests/density64.py (pinned on the CPU by
tests/test_density_gradient_cpu.py) and tests/warp64.py for the accuracy, fed the device's own normalised position so that
model and kernel sit in the same hash cells.  Every bound is computed here on the CPU from the difference between a model
run in float32 and in float64, never from the kernel's results.

Inputs: those of tests/test_gpu_track.py -- rng 7, 4099 rows in +-1.6, aabb +-1.5 (17 % of the rows leave the box), log2
table 15, hash_max_res 256, regime "trained", moving step 1/32."""
import functools

import numpy as np
import pytest
import torch

import density64 as D
import warp64 as W
from test_gpu_track import AABB, DEV, FLAGS, MODES, SIZES, STEP, N, T, _field, _inputs, _params

pytestmark = pytest.mark.gpu

TABLES = [("f16x2", "f16"), ("f16x2", "temporal"), ("f16", "temporal"), ("f32", "f16"), ("f32+h16x2", "temporal")]
OUTPUTS = ("sigma", "grad", "dlog", "dlog_canonical")


def _all(f, pos, t):
    from ced_nerf_amd import ops
    return ops.field_density_gradient(f._descriptor(), pos, t)


# ---- 1. the primal is query_density's ----------------------------------------------------------------------------------
def _check_primal(f, what):
    from ced_nerf_amd import ops
    pos, t = _inputs()
    want = f.query_density(pos, t)["density"]
    full = _all(f, pos, t)
    assert torch.equal(full[0], want[:, 0]), (what, int((full[0] != want[:, 0]).sum()))
    inside = f.query_move(pos, t, return_normalized=True)[3]
    assert 0.1 < 1.0 - float(inside.float().mean()) < 0.25
    for o in full[1:]:
        assert o.shape == (len(pos), 3) and o.dtype == torch.float32 and bool(torch.isfinite(o).all())
        assert not bool(o[~inside].any()) and float(o[inside].abs().max()) > 1.0
    assert not bool(full[0][~inside].any())
    density, grad = f.query_density_gradient(pos, t)
    assert density.shape == (len(pos), 1) and torch.equal(density, want) and torch.equal(grad, full[1])
    normals, density = f.query_normals(pos, t)
    length = full[2].norm(dim=-1, keepdim=True)
    assert torch.equal(density, want) and torch.equal(normals, torch.where(length > 0, -full[2] / length, torch.zeros_like(full[2])))
    assert float((normals[inside].norm(dim=-1) - 1).abs().max()) <= 1e-6
    can_grad = f.query_density_gradient(pos, t, canonical=True)[1]
    assert torch.equal(can_grad, want.clamp(max=ops.EXP15) * full[3])
    assert torch.equal(f.query_normals(pos, t, canonical=True)[0], ops.unit_or_zero(-full[3]))
    for n in SIZES:
        got = _all(f, pos[:n], t[:n])
        for g, w, name in zip(got, full, OUTPUTS):
            assert g.shape == w[:n].shape and torch.equal(g, w[:n]), (what, n, name)       # a row does not depend on n
    d = f._descriptor()
    for i, name in enumerate(OUTPUTS):
        only = ops.field_density_gradient(d, pos, t, want=tuple(j == i for j in range(4)))
        assert all((o is None) == (j != i) for j, o in enumerate(only)) and torch.equal(only[i], full[i]), (what, name)
    with pytest.raises(ValueError, match="no output"):
        ops.field_density_gradient(d, pos, t, want=(False,) * 4)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("div,tm", FLAGS)
def test_density_is_query_densitys_bit_for_bit(div, tm, mode):
    """sigma == query_density's with torch.equal at every n of SIZES; a row's outputs are the same at every n; each output
    alone is the same output of the full call; outside the box everything is 0"""
    _check_primal(_field(div, tm, mode), (div, tm, mode))


@pytest.mark.parametrize("mode,table", TABLES)
def test_density_is_query_densitys_on_the_other_tables(mode, table):
    _check_primal(_field(True, 0, mode, STEP, table), (mode, table))


# ---- 2. the chain is the stated composition ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("div,tm", FLAGS)
def test_world_gradients_are_the_headers_lines_bit_for_bit(div, tm, mode):
    """dlog and grad == include/cednerf_hip.h's lines in numpy float32 (IEEE single, no contraction) on the kernel's own
    dlog_canonical, query_move_jacobian's jac and query_density's density"""
    f = _field(div, tm, mode)
    pos, t = _inputs()
    sigma, grad, dlog, dc = _all(f, pos, t)
    jac = f.query_move_jacobian(pos, t)[1]
    w_dlog, w_grad = D.world_gradients(N(dc), N(jac), N(f.query_density(pos, t)["density"]))
    assert w_dlog.dtype == w_grad.dtype == np.float32
    assert np.array_equal(N(dlog), w_dlog), int((N(dlog) != w_dlog).sum())
    assert np.array_equal(N(grad), w_grad), int((N(grad) != w_grad).sum())
    assert float(np.abs(N(dlog) - N(dc)).max()) > 1e-3                   # the warp's Jacobian is not nothing


# ---- 3. / 4. accuracy ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _device_canonical(div, tm, mode, table, max_res):
    """the device's own (x_norm, |move|, inside) of the rows: pinned to the oracle bit for bit by test_gpu_deformation"""
    f = _field_of(div, tm, mode, table, max_res)
    pos, t = _rows(max_res)
    _, move, x_norm, inside = f.query_move(pos, t, return_normalized=True)
    return N(x_norm), np.linalg.norm(N(move).astype(np.float64), axis=-1), N(inside)


@functools.lru_cache(maxsize=None)
def _params_of(div, tm, table, max_res):
    if max_res == 256:
        return _params(div, tm, STEP, table)
    from ced_nerf_amd import synthetic as S
    return S.init_field_params(list(AABB), STEP, hash_max_res=max_res, log2_hashmap_size=15, use_div_offsets=div,
                               use_time_embedding=tm != 0, use_time_attenuation=tm == 2, regime="trained")


@functools.lru_cache(maxsize=None)
def _field_of(div, tm, mode, table, max_res):
    if max_res == 256:
        return _field(div, tm, mode, STEP, table)
    from ced_nerf_amd.model import DNGPradianceField
    return DNGPradianceField.from_params(_params_of(div, tm, table, max_res), DEV, mlp_precision=mode).eval()


def _rows(max_res):
    pos, t = _inputs()
    return (pos, t) if max_res == 256 else (pos[:257].contiguous(), t[:257].contiguous())


@functools.lru_cache(maxsize=None)
def _model(div, tm, mode, table, max_res, dtype):
    """(dlog_canonical, pre) of density64 on the device's normalised positions, rounded as `mode`'s mlp_base"""
    params = _params_of(div, tm, table, max_res)
    x_norm, mnorm, _ = _device_canonical(div, tm, mode, table, max_res)
    _, t = _rows(max_res)
    dt = np.dtype(dtype).type
    _, draw, pre = D.base_gradient(params, x_norm, N(t), mnorm, dt, D.BASE_MODES[mode])
    return D.canonical_gradient(params, draw, dt), pre


def _check_canonical_accuracy(div, tm, mode, table="f32", max_res=256):
    f = _field_of(div, tm, mode, table, max_res)
    pos, t = _rows(max_res)
    inside = _device_canonical(div, tm, mode, table, max_res)[2]
    got = _all(f, pos, t)
    assert all(bool(torch.isfinite(o).all()) for o in got)
    dc64, pre = _model(div, tm, mode, table, max_res, "float64")
    dc32, _ = _model(div, tm, mode, table, max_res, "float32")
    keep = inside & W.kept_rows(pre)
    left_out = 1.0 - float(keep.sum()) / float(inside.sum())
    factor = 8 if D.BASE_MODES[mode] == "f16" else 4
    base = float(np.abs(dc32 - dc64)[keep].max())
    err = float(np.abs(N(got[3]) - dc64)[keep].max())
    print(f"dlog_canonical [{mode} {table} max_res={max_res} div={div} tm={tm}]: {100 * left_out:.2f} % of the inside rows left "
          f"out; max |kernel - model64| = {err:.3e}, bound {factor} x {base:.3e}; max |dlog_canonical| = {float(np.abs(dc64[keep]).max()):.4g}")
    assert left_out <= 0.02
    assert err <= factor * base
    return keep, dc64, dc32, got


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("div,tm", FLAGS)
def test_canonical_gradient_accuracy(div, tm, mode):
    """dlog_canonical against density64 (float64, weights and layer inputs rounded as the mode's mlp_base rounds them) on the
    device's own x_norm and |move|, on the inside rows none of whose hidden pre-activations lies within 1e-5 of the layer's
    largest of zero (at most 2 % may be left out).  Bound: 4 x (8 x for f16) the largest difference between that model in
    float32 and in float64, computed here.
    CPU model: the bound's base is 3.7e-4 .. 5.4e-4 (f32, f16x2) and 0.18 / 0.29 (f16) on magnitudes up to 1.8e3 / 2.4e3 (fine
    offsets and time encoding off / on); 0.24 - 0.33 % of the inside rows are left out.
    Measured on an MI355X, max |dlog_canonical - model| on the kept rows: f32 and f32+h16x2 4.2e-4 / 4.6e-4, f16x2 4.4e-4 /
    5.0e-4, f16 0.29 / 0.18 (one row's fp16 double rounding, which the float32 model shares: error and base agree to four digits)."""
    _check_canonical_accuracy(div, tm, mode)


@pytest.mark.parametrize("mode,table", TABLES)
def test_canonical_gradient_accuracy_on_the_other_tables(mode, table):
    """the same on an fp16 table (f16x2: the K = 32 placements) and on a temporal one, whose derivative is the same formula
    on the time-interpolated corners.  CPU model: base 4.1e-4 .. 5.4e-4, f16 on the temporal table 0.16; 0.36 % (fp16 table) and
    0.56 - 0.59 % (temporal) of the inside rows left out.  Measured on an MI355X: 3.8e-4 .. 4.3e-4, f16 0.16."""
    _check_canonical_accuracy(True, 0, mode, table)


@pytest.mark.parametrize("mode", MODES)
def test_finest_levels_stay_in_range(mode):
    """hash_max_res 8192 (scales up to 8191: a level's slope is 8191 times a difference of table values of order 1), 257
    rows: every output finite and the accuracy bound of dlog_canonical holds -- unscaled fp16 tangents would overflow.
    CPU model: base 4.8e-3 (f32, f32+h16x2), 1.0e-2 (f16x2), 0.59 (f16) on magnitudes up to 3.5e4; no row left out.
    Measured on an MI355X: 8.4e-3, 8.5e-3, 0.59."""
    keep, dc64, _, got = _check_canonical_accuracy(True, 2, mode, "f32", 8192)
    assert float(np.abs(dc64[keep]).max()) > 1e4


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("div,tm", FLAGS)
def test_world_gradient_accuracy(div, tm, mode):
    """dlog against (I + J_x)^T dlog_canonical of the two models (density64, warp64.move_jacobian, each rounded as the mode
    rounds its network), on the rows both kept-row rules keep (at most 2 % of the inside rows left out); bound as above.
    CPU model: base 5.8e-4 .. 7.5e-4 (f32, f16x2), 0.31 / 0.18 (f16); 0.77 - 1.04 % of the inside rows left out.
    Measured on an MI355X: f32 4.1e-4 / 5.6e-4, f16x2 4.4e-4 / 5.4e-4, f16 0.31 / 0.18."""
    keep, dc64, dc32, got = _check_canonical_accuracy(div, tm, mode)
    pos, t = _inputs()
    inside = _device_canonical(div, tm, mode, "f32", 256)[2]
    mm = W.MOTION_MODES[mode]
    params = _params(div, tm, STEP, "f32")
    _, j64, pre = W.move_jacobian(params, N(pos), N(t), np.float64, mm)
    _, j32, _ = W.move_jacobian(params, N(pos), N(t), np.float32, mm)
    keep = keep & W.kept_rows(pre)
    left_out = 1.0 - float(keep.sum()) / float(inside.sum())
    sigma = N(got[0])
    dl64 = D.world_gradients(dc64, j64, sigma.astype(np.float64))[0]
    dl32 = D.world_gradients(dc32, j32, sigma)[0]
    factor = 8 if mm == "f16" else 4
    base = float(np.abs(dl32 - dl64)[keep].max())
    err = float(np.abs(N(got[2]) - dl64)[keep].max())
    print(f"dlog [{mode} div={div} tm={tm}]: {100 * left_out:.2f} % of the inside rows left out; max |kernel - model64| = {err:.3e}, "
          f"bound {factor} x {base:.3e}")
    assert left_out <= 0.02
    assert err <= factor * base


# ---- 6. the rays entry -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,tm", [("f32", 2), ("f16", 2), ("f16x2", 0), ("f16x2", 2), ("f32+h16x2", 0)])
def test_rays_entry_is_the_points_entry_at_the_samples(mode, tm):
    """97 rays, 1 031 samples, per-ray timestamps (training mode) and one scalar (eval): all four outputs equal the points
    entry fed px = o + (d * (t0 + t1)) / 2.0f formed in torch fp32; n_dev < n leaves the tail untouched"""
    from ced_nerf_amd import ops
    rng = np.random.default_rng(3)
    n_rays, n = 97, 1031
    o = rng.uniform(-1.0, 1.0, size=(n_rays, 3)).astype(np.float32)
    d = rng.normal(size=(n_rays, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    ri = np.sort(rng.integers(0, n_rays, size=n)).astype(np.int64)
    t0 = rng.uniform(0.0, 2.0, size=n).astype(np.float32)
    t1 = (t0 + np.float32(0.02)).astype(np.float32)
    f = _field(True, tm, mode)
    O, Dd, RI, T0, T1 = T(o), T(d), T(ri), T(t0), T(t1)
    pos = O[RI] + (Dd[RI] * (T0 + T1)[:, None]) / 2.0
    for per_ray in (True, False):
        ts = T(rng.uniform(0.0, 1.0, size=(n_rays if per_ray else 1, 1)).astype(np.float32))
        f.train(per_ray)
        got = f.query_density_gradient_rays(O, Dd, RI, T0, T1, ts)
        f.eval()
        tq = ts.reshape(-1)[RI] if per_ray else ts.reshape(-1)[:1].expand(n).contiguous()
        want = _all(f, pos, tq)
        for g, w, name in zip(got, want, OUTPUTS):
            assert g.shape == w.shape and torch.equal(g, w), (per_ray, name)
        assert bool(want[1].any())
        if not per_ray:
            only = f.query_density_gradient_rays(O, Dd, RI, T0, T1, ts, want=(False, False, True, False))
            assert only[0] is None and only[1] is None and only[3] is None and torch.equal(only[2], want[2])
            keep = 700
            out = tuple(torch.full((n,) if i == 0 else (n, 3), 7.0, device=DEV) for i in range(4))
            ops.field_density_gradient_rays(f._descriptor(), O, Dd, RI, T0, T1, ts.reshape(-1), False,
                                            n_dev=torch.tensor([keep], device=DEV, dtype=torch.int64), out=out)
            for g, w in zip(out, want):
                assert torch.equal(g[:keep], w[:keep]) and bool((g[keep:] == 7.0).all())


# ---- 7. render_normals -------------------------------------------------------------------------------------------------
def test_render_normals_samples_weights_and_normals(oracle):
    """the sample set and opacity are render_motion's for the same arguments; normals is accumulate_along_rays(weights,
    normal) on the returned samples; normal is the rays entry's -dlog / |dlog|; a frame that misses gives zeros"""
    from ced_nerf_amd import ops
    from ced_nerf_amd.nerfacc_api import _packed_info_from, accumulate_along_rays
    from ced_nerf_amd.utils import render_motion, render_normals
    from test_gpu_deformation import RENDER, H, W as WIDTH, _motion_setup
    for levels, cone, alpha in ((1, 0.0, 0.0), (2, 0.004, 1e-2)):
        _, f, est, _, _, _, rays = _motion_setup(oracle, levels)
        ts = T(np.array([[0.4]], np.float32))
        kw = dict(RENDER, cone_angle=cone, alpha_thre=alpha)
        normals, opacity, n_samples, samples = render_normals(f, est, rays, timestamps=ts, return_samples=True, **kw)
        motion, m_opacity, m_samples, ms = render_motion(f, est, rays, timestamps=ts, return_samples=True, **kw)
        assert normals.shape == (H, WIDTH, 3) and n_samples == m_samples > 100 and torch.equal(opacity, m_opacity)
        assert len(samples) == len(ms) == 1 and set(samples[0]) == {"ray_indices", "t_starts", "t_ends", "weights", "normal"}
        s = samples[0]
        for k in ("ray_indices", "t_starts", "t_ends", "weights"):
            assert torch.equal(s[k], ms[0][k]), k
        O, Dd = rays.origins.reshape(-1, 3), rays.viewdirs.reshape(-1, 3)
        packed = _packed_info_from(s["ray_indices"], H * WIDTH)
        assert torch.equal(normals.reshape(-1, 3), accumulate_along_rays(s["weights"], values=s["normal"], packed_info=packed))
        dlog = f.query_density_gradient_rays(O, Dd, s["ray_indices"], s["t_starts"], s["t_ends"], ts)[2]
        assert torch.equal(s["normal"], ops.unit_or_zero(-dlog)) and bool(s["normal"].any())
        miss = opacity.reshape(-1) == 0
        assert 0 < int(miss.sum()) < H * WIDTH and not bool(normals.reshape(-1, 3)[miss].any())
        assert float((normals.norm(dim=-1, keepdim=True) - opacity).max()) <= 1e-5      # a weighted sum of unit vectors
        n2, o2, c2, s2 = render_normals(f, est, rays, timestamps=ts, return_samples=True, test_chunk_size=64, **kw)
        assert c2 == n_samples and torch.equal(n2, normals) and torch.equal(o2, opacity) and len(s2) == H * WIDTH // 64
        assert torch.equal(torch.cat([c["normal"] for c in s2]), s["normal"])
    away = type(rays)(rays.origins, -rays.viewdirs)
    normals, opacity, n_samples, samples = render_normals(f, est, away, timestamps=ts, return_samples=True, **RENDER)
    assert n_samples == 0 and normals.shape == (H, WIDTH, 3) and not bool(normals.any()) and not bool(opacity.any())
    assert len(samples) == 1 and samples[0]["normal"].shape == (0, 3)


def test_render_video_normal_maps(oracle):
    """render_video(..., normals=True): normals_f32 of every frame equals render_normals on the frame's rays and time;
    without the keyword the frame dicts have the keys they always had"""
    from ced_nerf_amd import synthetic as S
    from ced_nerf_amd.utils import Rays, render_normals
    from ced_nerf_amd.video import render_video
    from test_gpu_deformation import RENDER, H, W as WIDTH, _motion_setup
    _, f, est, _, _, _, _ = _motion_setup(oracle, 1)
    frames_rays = []
    for k in range(2):
        o, d = S.make_camera_rays(WIDTH, H, 0.69, S.look_at_c2w(4.0, 30.0, 20.0 + 25.0 * k))
        frames_rays.append(Rays(origins=T(o), viewdirs=T(d)))
    times = [torch.tensor([[0.1 + 0.4 * k]], device=DEV) for k in range(2)]
    rk = dict(RENDER, cone_angle=0.0, alpha_thre=0.0)
    plain = render_video(f, est, lambda i: frames_rays[i], lambda i: times[i], 2, max_samples=256, render_kwargs=rk)
    assert all(set(fr) == {"rgb", "depth", "n_samples"} for fr in plain)
    frames = render_video(f, est, lambda i: frames_rays[i], lambda i: times[i], 2, max_samples=256, render_kwargs=rk,
                          normals=True, motion=True)
    torch.cuda.synchronize()
    assert all(set(fr) == {"rgb", "depth", "n_samples", "motion_f32", "normals_f32"} for fr in frames)
    for i, (fr, pl) in enumerate(zip(frames, plain)):
        want = render_normals(f, est, frames_rays[i], timestamps=times[i], **rk)[0]
        assert fr["normals_f32"].shape == (H, WIDTH, 3) and torch.equal(fr["normals_f32"], want) and bool(want.any())
        assert torch.equal(fr["rgb"], pl["rgb"]) and fr["n_samples"] == pl["n_samples"]
    assert not torch.equal(frames[0]["normals_f32"], frames[1]["normals_f32"])


# ---- 8. meshes ---------------------------------------------------------------------------------------------------------
def test_mesh_with_field_normals(tmp_path):
    """extract_mesh(normals="field"): the "lattice" mesh with its normals replaced by query_normals(vertices, t)[0] (unit or
    zero); dirs="normal" views along them; the files carry them; extract_mesh_tracked carries them along.  The median angle
    between the field's and the lattice's normals is printed, not asserted (MI355X, this noise-like field, reso 32: 88 degrees)."""
    from ced_nerf_amd import export as E
    from test_gpu_export import _density, _field as export_field
    from test_gpu_mesh import _read_mesh_ply
    f = export_field(True, 2, "f32")
    t = 0.37
    thresh = float(_density(True, 2, "f32", 32, t)[1].median())
    kw = dict(reso=32, sigma_thresh=thresh, dirs="normal")
    lattice = E.extract_mesh(f, t, **kw)
    assert all(torch.equal(E.extract_mesh(f, t, normals="lattice", **kw)[k], lattice[k]) for k in ("vertices", "normals", "rgb"))
    mesh = E.extract_mesh(f, t, normals="field", **kw)
    v = mesh["vertices"].shape[0]
    assert v > 100
    for k in ("vertices", "faces", "cube", "sigma", "embedding"):
        assert torch.equal(mesh[k], lattice[k]), k
    want = f.query_normals(mesh["vertices"], torch.full((v,), t, device=DEV))[0]
    assert torch.equal(mesh["normals"], want)
    length = want.norm(dim=-1)
    assert bool(((length - 1).abs() <= 1e-6).logical_or(length == 0).all()) and float((length > 0).float().mean()) > 0.9
    head_on = torch.where((want == 0).all(-1, keepdim=True), want.new_tensor([0.0, 0.0, 1.0]), -want)
    assert torch.equal(mesh["rgb"], f._query_rgb(head_on, mesh["embedding"], False).view(v, 1, 3))
    both = (length > 0) & (lattice["normals"].norm(dim=-1) > 0)
    cos = (want * lattice["normals"]).sum(-1)[both].clamp(-1, 1)
    print(f"field against lattice normals (reso 32, V = {v}): median angle {float(torch.rad2deg(torch.acos(cos)).median()):.1f} deg")
    E.save_mesh_npz(str(tmp_path / "m.npz"), mesh)
    with np.load(tmp_path / "m.npz") as z:
        assert np.array_equal(z["normals"], N(want)) and np.array_equal(z["vertices"], N(mesh["vertices"]))
    E.save_mesh_ply(str(tmp_path / "m.ply"), mesh)
    vrec, frec = _read_mesh_ply(tmp_path / "m.ply")
    assert np.array_equal(vrec["normal"], N(want)) and np.array_equal(frec["ids"], N(mesh["faces"]))
    seq = E.extract_mesh_sequence(f, [t, 0.8], normals="field", **kw)
    assert torch.equal(seq[0]["normals"], want) and not torch.equal(seq[1]["vertices"], mesh["vertices"])
    tracked = E.extract_mesh_tracked(f, t, [0.0, t], method="newton", normals="field", **kw)
    assert torch.equal(tracked["normals"], want) and tracked["normals_t"].shape == (2, v, 3)
    has = length > 0
    assert float((tracked["normals_t"][1] - want)[has].abs().max()) <= 1e-5
    plain = E.track_mesh(f, mesh, t, [0.0, t], method="newton", normals=True)
    assert torch.equal(plain["normals_t"], tracked["normals_t"])


def test_cli_writes_field_normals(tmp_path):
    from ced_nerf_amd import export as E, trainer
    from test_gpu_mesh import _read_mesh_ply
    cfg = trainer.resolve_config("dnerf", None, log2_hashmap_size=14)
    field, est = trainer.build_modules(cfg, torch.device(DEV), use_div_offsets=True, use_time_embedding=True)
    est.set_binaries(T(np.random.default_rng(4).uniform(size=tuple(est.binaries.shape)) < 0.5))
    path = str(tmp_path / "model.pth")
    torch.save({"radiance_field": field.state_dict(), "occupancy_grid": est.state_dict()}, path)
    argv = ["--load_model", path, "--preset", "dnerf", "--log2_hashmap_size", "14", "-df", "-te", "--times", "0.5",
            "--reso", "16", "--sigma_thresh", "1e-6", "--device", DEV, "--mesh", "--mesh_normals", "field", "--out", str(tmp_path / "o")]
    assert E.main(argv) == 0
    want = E.extract_mesh(field, 0.5, reso=16, sigma_thresh=1e-6, dirs="normal", estimator=est, normals="field")
    assert want["vertices"].shape[0] > 0
    assert torch.equal(want["normals"], field.query_normals(want["vertices"], torch.full((want["vertices"].shape[0],), 0.5, device=DEV))[0])
    with np.load(tmp_path / "o" / "mesh_0000.npz") as z:
        assert np.array_equal(z["normals"], N(want["normals"])) and np.array_equal(z["vertices"], N(want["vertices"]))
    vrec, _ = _read_mesh_ply(tmp_path / "o" / "mesh_0000.ply")
    assert np.array_equal(vrec["normal"], N(want["normals"]))
