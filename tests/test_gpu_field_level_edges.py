"""The rare paths the field kernels keep off the per-sample stream, bit for bit against the CPU oracle's mode of the same
name (f16x2 and f32, fp32 and fp16 plain tables):

* hash_level's dense levels (csrc/field_device.hpp) take ONE wave-uniform decision per call -- does the reference's
  `% size` act on any lane? -- and run the unwrapped indices, pair loads without a re-read test and the level offset folded
  into the (y, z) sums when it does not.  The points below sit in the last cell along y and z of every dense level (x, y,
  z = 1 exactly among them), just inside that cell and in the interior, ordered so that whole 32-sample wave tiles are
  all-interior (the new path), all-boundary and mixed (the old path, with lanes of both kinds).

  Which levels can wrap at all: a level has res = ceil(scale) + 1 points per axis and size >= res^3 entries, and the
  largest corner coordinate a position in [0, 1] reaches is floor(scale + 0.5) + 1.  That is res -- an index >= size --
  only when scale is an integer or its fraction is >= 0.5 (base 16, max 1024, 16 levels: levels 0, 2, 3, 4, 5, 7 of the
  first eight); on the other levels the largest index is res^3 - 1 and no point wraps.  The tests assert, from the
  oracle's normalised positions, that every dense level that CAN wrap has a point that does, and that the others cannot.

* the colour head's SH input comes from a per-ray array the frame renderers fill in their set-up launch
  (FieldArgs::sh_ray) instead of three loads, a square root and two divisions per sample: a 32 x 32 frame and a
  two-frame call against the oracle (schedule, sample totals, every pixel; rays that meet nothing; a frame boundary
  inside a workgroup of the set-up launch), and the same calls with the array switched off
  (ced_set_option("frame_sh_per_ray", 0)).  The scene is ced_nerf_amd.synthetic's D-NeRF-shaped one (tests/scene_toys.py
  builds dataset folders, not fields): the camera stands outside the box and its rays cross it from face to face.
"""
import numpy as np
import pytest
import torch

from conftest import assert_bitexact

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
AABB = np.array([-1.5, -1.5, -1.5, 1.5, 1.5, 1.5], np.float32)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def _max_corner(xn, tabs, lvl):
    """largest unwrapped corner index of normalised positions xn [n,3] on level lvl, as hash_level forms it (fp32)"""
    s = np.float32(tabs["scale"][lvl])
    g = np.floor(xn.astype(np.float32) * s + np.float32(0.5)).astype(np.int64)
    r = int(tabs["res"][lvl])
    return (g[:, 0] + 1) + (g[:, 1] + 1) * r + (g[:, 2] + 1) * r * r


def _can_wrap(tabs, lvl):
    s = float(tabs["scale"][lvl])
    return int(np.floor(np.float32(s) + np.float32(0.5))) + 1 == int(tabs["res"][lvl])


def _candidates(tabs, dense, rng, per_level=24):
    """normalised coordinates in [0, 1.05]^3 (above 1: outside the box, clamped to 1 exactly): per dense level the last cell
    along y, along z and along both, and points just inside it; exact ones; interior points"""
    out = []
    for lvl in dense:
        s = float(tabs["scale"][lvl])
        edge = (np.floor(np.float32(s) + np.float32(0.5)) - 0.5) / s           # first coordinate of the last cell
        for k in range(per_level):
            u = rng.uniform(0.05, 0.9, 3)
            hi = edge + (1.0 - edge) * (rng.uniform(0.05, 1.0) if k % 2 else 0.02)    # anywhere in the cell / just inside it
            if k % 3 == 0: u[1] = hi
            elif k % 3 == 1: u[2] = hi
            else: u[1] = u[2] = hi
            if k % 8 == 7: u[0] = hi
            out.append(u)
    for ex in ((1.05, 0.4, 0.3), (0.2, 1.05, 0.6), (0.7, 0.1, 1.05), (1.05, 1.05, 1.05), (0.5, 1.05, 1.05), (1.05, 0.3, 1.05)):
        out += [np.array(ex)] * 4
    out += list(rng.uniform(0.05, 0.8, (160, 3)))
    return np.array(out)


def _arrange(is_b, rng):
    """indices ordered into 32-sample tiles: 2 all-interior, 2 all-boundary, then mixed ones (every second sample of a
    tile on the boundary, then whatever is left, shuffled), ending in a ragged tile"""
    b = list(rng.permutation(np.flatnonzero(is_b)))
    i = list(rng.permutation(np.flatnonzero(~is_b)))
    assert len(i) >= 112 and len(b) >= 112, (len(i), len(b))
    order = i[:64] + b[:64]
    for k in range(32):
        order += [i[64 + k], b[64 + k]]
    rest = list(rng.permutation(i[96:] + b[96:]))
    order += rest
    if len(order) % 32 == 0:
        order = order[:-5]
    return np.array(order)


@pytest.fixture(scope="module")
def edge_fields(oracle):
    """per (log2T, table dtype): parameters, the ordered points and the per-level wrap record -- built once"""
    from ced_nerf_amd import synthetic as S
    from ced_nerf_amd.hashgrid import level_tables
    made = {}

    def get(log2t, dtype):
        key = (log2t, np.dtype(dtype).name)
        if key in made:
            return made[key]
        params = S.init_field_params(AABB, 1.0 / 4096, 1024, log2t, regime="trained", seed=7, table_dtype=dtype)
        tabs = level_tables(16, 1024, 16, log2t)
        dense = [l for l in range(16) if not tabs["hashed"][l]]
        rng = np.random.default_rng(11)
        u = _candidates(tabs, dense, rng, per_level=max(24, 240 // len(dense)))
        pos = (AABB[:3] + u * (AABB[3:] - AABB[:3])).astype(np.float32)
        t = rng.uniform(0.0, 1.0, len(pos)).astype(np.float32)
        dirs = rng.standard_normal((len(pos), 3)).astype(np.float32)
        # the moved, normalised position; the encoder sees it clamped to [0, 1] (outside the box: exactly 0 or 1)
        xn = np.clip(oracle.OracleField(params).forward(pos, t, dirs, want_xnorm=True)["x_norm"], 0.0, 1.0)
        wraps = np.stack([_max_corner(xn, tabs, l) >= int(tabs["size"][l]) for l in dense], 1)
        order = _arrange(wraps.any(1), rng)
        made[key] = dict(params=params, tabs=tabs, dense=dense, pos=pos[order], t=t[order], dirs=dirs[order],
                         xn=xn[order], wraps=wraps[order])
        return made[key]
    return get


def _check_placement(e):
    tabs, dense, wraps, xn = e["tabs"], e["dense"], e["wraps"], e["xn"]
    for k, lvl in enumerate(dense):
        if _can_wrap(tabs, lvl):
            assert wraps[:, k].any(), f"no point wraps on dense level {lvl}: the test would prove nothing"
        else:
            r = int(tabs["res"][lvl])
            assert not wraps[:, k].any() and r ** 3 - 1 < int(tabs["size"][lvl]), lvl
    assert _can_wrap(tabs, dense[0]) and sum(_can_wrap(tabs, l) for l in dense) >= (len(dense) + 1) // 2
    for a in range(3):
        assert (xn[:, a] == 1.0).any(), f"no point with coordinate {a} == 1 exactly"
    b = wraps.any(1)
    n_full = len(b) // 32
    kinds = [(b[32 * k:32 * k + 32].all(), (~b[32 * k:32 * k + 32]).all()) for k in range(n_full)]
    assert sum(1 for x in kinds if x[0]) >= 2 and sum(1 for x in kinds if x[1]) >= 2          # all-boundary, all-interior
    assert sum(1 for x in kinds if not x[0] and not x[1]) >= 2 and len(b) % 32 != 0           # mixed, ragged end
    assert 200 <= len(b) <= 900


# log2T 14: the issue's range -- two dense levels, so gather slot 0 is mixed (hash_level MODE 0, unchanged code, the
# reference point); 17: levels 0..4 dense, slot 0 takes the dense pair-load form (MODE 3) whose wrap moved off the common
# path; both with the hashed levels behind them
@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["t32", "t16"])
@pytest.mark.parametrize("prec", ["f16x2", "f32"])
@pytest.mark.parametrize("log2t", [14, 17])
def test_field_forward_on_level_boundaries_bitexact(oracle, edge_fields, log2t, prec, dtype):
    from ced_nerf_amd import ops
    from ced_nerf_amd.model import DNGPradianceField
    e = edge_fields(log2t, dtype)
    _check_placement(e)
    want = oracle.OracleField(e["params"], mlp_half=prec).forward(e["pos"], e["t"], e["dirs"], want_geo=True)
    f = DNGPradianceField.from_params(e["params"], DEV, mlp_precision=prec).eval()
    desc = f._descriptor()
    n_dense = len(e["dense"])
    assert [int(desc.hash.hashed[l]) for l in range(16)] == [0] * n_dense + [1] * (16 - n_dense)
    assert (n_dense >= 4) == (log2t == 17)
    rgb, sigma, geo = ops.field_forward(desc, T(e["pos"]), T(e["t"]), T(e["dirs"]), want_geo=True)
    torch.cuda.synchronize()
    print(f"log2T {log2t} {prec} {np.dtype(dtype).name}: {len(e['pos'])} points, {n_dense} dense levels, "
          f"{int(e['wraps'].any(1).sum())} wrap somewhere")
    assert_bitexact(N(sigma).reshape(-1), want["density"].reshape(-1), "sigma")
    assert_bitexact(N(geo), want["base_mlp_out"], "geo")
    assert_bitexact(N(rgb), want["rgb"], "rgb")


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["t32", "t16"])
def test_hash_encode_four_levels_on_level_boundaries_bitexact(oracle, dtype):
    """The encoder alone (ced_hash_encode: hash_level MODE 1 / 2 per level) on a four-level grid, base 16 to 32, 2^14
    entries per level: levels 0 and 1 dense (only level 0 can wrap: scale 15), 2 and 3 hashed."""
    from ced_nerf_amd import ops
    from ced_nerf_amd.hashgrid import level_tables
    tabs = level_tables(16, 32, 4, 14)
    dense = [l for l in range(4) if not tabs["hashed"][l]]
    assert dense == [0, 1] and _can_wrap(tabs, 0) and not _can_wrap(tabs, 1)
    rng = np.random.default_rng(3)
    x = np.clip(_candidates(tabs, dense, rng, per_level=120), 0.0, 1.0).astype(np.float32)
    wraps = _max_corner(x, tabs, 0) >= int(tabs["size"][0])
    x = x[_arrange(wraps, rng)]
    wraps = _max_corner(x, tabs, 0) >= int(tabs["size"][0])
    assert wraps[64:128].all() and not wraps[:64].any() and wraps[128:192].any() and not wraps[128:192].all()
    assert not (_max_corner(x, tabs, 1) >= int(tabs["size"][1])).any()
    for a in range(3):
        assert (x[:, a] == 1.0).any()
    table = (rng.standard_normal((int(tabs["total"]), 2)).astype(np.float32) * np.float32(0.5)).astype(dtype)
    params = dict(hash=dict(base_res=16, max_res=32, n_levels=4, log2_hashmap_size=14, table=table, temporal=False))
    want = oracle.OracleField(params).hash_encode(x)
    tab = T(table)                                   # the descriptor holds its address: keep it alive
    desc, _ = ops.make_hash_desc(tab, 16, 32, 4, 14)
    got = ops.hash_encode(desc, T(x))
    torch.cuda.synchronize()
    assert_bitexact(N(got), want, "hash_encode")


# --- per-ray SH inputs -------------------------------------------------------------------------------------------------
W = H = 32


@pytest.fixture(scope="module")
def toy_frames(oracle):
    """the 32 x 32 scene, three views of it (the third looks away: no ray meets the box), oracle frames per precision"""
    from ced_nerf_amd import synthetic as S
    sc = S.make_scene("dnerf", W, H, "trained", log2_hashmap_size=15)
    cfg = sc["cfg"]
    views = []
    for k, (elev, az) in enumerate([(30.0, 30.0), (55.0, 140.0), (10.0, 250.0)]):
        c2w = S.look_at_c2w(cfg["radius"], elev, az, cfg["opengl"])
        if k == 2:
            c2w = c2w.copy(); c2w[:3, :3] = -c2w[:3, :3]
        o, d = S.make_camera_rays(W, H, cfg["camera_angle_x"], c2w, cfg["opengl"])
        views.append((o, d, np.float32(0.25 + 0.5 * k)))
    oest = oracle.OracleEstimator(cfg["aabb"], cfg["grid_resolution"], cfg["grid_levels"], sc["binaries"])
    cache = {}

    def want(prec, k):
        if (prec, k) not in cache:
            o, d, t = views[k]
            trace = []
            out = oracle.render_image_test(1024, oracle.OracleField(sc["params"], mlp_half=prec), oest, o, d,
                                           timestamps=np.array([[t]], np.float32), trace=trace, **sc["render"])
            cache[(prec, k)] = (out, trace)
        return cache[(prec, k)]
    return sc, views, want


def _gpu_scene(sc, prec):
    from ced_nerf_amd.model import DNGPradianceField
    from ced_nerf_amd.nerfacc_api import OccGridEstimator
    cfg = sc["cfg"]
    f = DNGPradianceField.from_params(sc["params"], DEV, mlp_precision=prec).eval()
    est = OccGridEstimator(cfg["aabb"], cfg["grid_resolution"], cfg["grid_levels"]).to(DEV)
    est.set_binaries(T(sc["binaries"]))
    rk = dict(sc["render"]); rk["render_bkgd"] = T(rk["render_bkgd"])
    return f, est, rk


@pytest.mark.parametrize("prec", ["f16x2", "f32"])
def test_small_frame_and_two_frames_bitexact(oracle, toy_frames, prec):
    from ced_nerf_amd import ops
    from ced_nerf_amd.utils import Rays, render_frames_test, render_image_test
    sc, views, want = toy_frames
    f, est, rk = _gpu_scene(sc, prec)
    (w_rgb, w_op, w_dp, w_total), trace = want(prec, 0)
    o, d, t = views[0]
    tracer = ops.FrameTracer(capacity=1100, with_events=False)
    rgb, op, dp, total = render_image_test(1024, f, est, Rays(T(o), T(d)), timestamps=torch.tensor([[t]], device=DEV),
                                           tracer=tracer, **rk)
    assert total == w_total and total > 2000
    assert tracer.iterations() == [dict(n_alive=x["n_alive"], n_samples=x["n_samples"], n_new=x["n_new"]) for x in trace]
    assert (w_op == 0).any() and (w_op > 0.5).any()                     # rays without a sample, rays that hit the scene
    assert_bitexact(N(rgb), w_rgb, "rgb"); assert_bitexact(N(op), w_op, "opacity"); assert_bitexact(N(dp), w_dp, "depth")
    # two frames of 1024 rays: the set-up launch's workgroups of 256 rays end on the frame boundary; with the view that
    # sees nothing first, the second frame's rays are the only ones that ever reach the field kernel
    for pair in ((0, 1), (2, 1)):
        rays = Rays(torch.stack([T(views[k][0]) for k in pair]), torch.stack([T(views[k][1]) for k in pair]))
        ts = torch.tensor([views[k][2] for k in pair], device=DEV)
        rgb, op, dp, totals = render_frames_test(1024, f, est, rays, timestamps=ts, **rk)
        for j, k in enumerate(pair):
            (w_rgb, w_op, w_dp, w_total), _ = want(prec, k)
            assert totals[j] == w_total, (pair, j, totals, w_total)
            assert_bitexact(N(rgb[j]), w_rgb, f"frame {k} rgb"); assert_bitexact(N(op[j]), w_op, f"frame {k} opacity")
            assert_bitexact(N(dp[j]), w_dp, f"frame {k} depth")
    assert want(prec, 2)[0][3] == 0


@pytest.mark.parametrize("prec", ["f16x2", "f32", "f32+h16x2", "f16"])
def test_sh_per_ray_equals_sh_per_sample(toy_frames, prec):
    """the same field launches with FieldArgs::sh_ray set and NULL: equal samples, equal colours"""
    from ced_nerf_amd import _lib
    from ced_nerf_amd.utils import Rays, render_frames_test, render_image_test
    sc, views, _ = toy_frames
    f, est, rk = _gpu_scene(sc, prec)
    L = _lib.lib()
    rays2 = Rays(torch.stack([T(views[k][0]) for k in (0, 1)]), torch.stack([T(views[k][1]) for k in (0, 1)]))
    ts2 = torch.tensor([views[k][2] for k in (0, 1)], device=DEV)
    outs = {}
    try:
        for flag in (1, 0):
            assert L.ced_set_option(b"frame_sh_per_ray", flag) == 0
            one = render_image_test(1024, f, est, Rays(T(views[0][0]), T(views[0][1])),
                                    timestamps=torch.tensor([[views[0][2]]], device=DEV), **rk)
            two = render_frames_test(1024, f, est, rays2, timestamps=ts2, **rk)
            torch.cuda.synchronize()
            outs[flag] = (one, two)
    finally:
        L.ced_set_option(b"frame_sh_per_ray", 1)
    assert L.ced_set_option(b"frame_sh_per_ray", 2) == -1
    for a, b in zip(outs[1], outs[0]):
        assert a[3] == b[3]
        for x, y in zip(a[:3], b[:3]):
            assert torch.equal(x, y)
    assert outs[1][0][3] > 2000 and float(outs[1][0][0].std()) > 0.01
