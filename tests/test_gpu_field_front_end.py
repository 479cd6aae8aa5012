"""The tile front end of the half-precision field kernels (csrc/field_half.hip: load_tile_slots, load_tile_rays) in rays
mode: which slot loads what, what an unused slot may poison, and where a tile ends.

Through ced_field_forward_rays (64-bit ray indices; no per-ray SH array and no sample window: that entry has neither)
in the modes f16x2 and f16, every output bit for bit against the CPU oracle's mode of the same name on positions formed
in numpy float32 by the kernel's own operations, o + (d * (t0 + t1)) / 2.  The exact kernels (f32) keep their front end
and are not run here.  The forms only the frame renderer passes -- 32-bit ray indices, the per-ray SH array
(ced_set_option("frame_sh_per_ray")), per-ray and shared time there -- are covered by the tiny frames at the end.

Unused slots (ray index -1), as the kernel has always treated them (field_half.hip, tile loop): the slot is evaluated on
ray 0 with t0 + t1 taken as 0 -- position rays_o[0], time timestamps[0] -- and the result is stored in the slot, except
that a wave tile (32 consecutive slots, the last one cut at the sample count) of unused slots only is skipped and stores
nothing.  Outputs are handed in pre-filled, so "stores nothing" is checked too."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import assert_bitexact

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
AABB = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
TILE = 32                                   # samples per wave tile of the half kernels (NT = 2)
FILL = np.float32(-7.0)                     # what the output buffers hold before a launch
PRECS = ["f16x2", "f16"]
N_RAYS = 48


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _params(**kw):
    from ced_nerf_amd import synthetic as S
    return S.init_field_params(AABB, 1.0 / 64, 1024, 17, regime="trained", seed=7, **kw)


class _Fields:
    """One GPU field and one oracle field per (parameter set, precision), made on first use and kept."""

    def __init__(self, oracle):
        self.oracle, self.params, self.gpu, self.cpu = oracle, {}, {}, {}

    def get(self, prec, kind="plain"):
        from ced_nerf_amd.model import DNGPradianceField
        if kind not in self.params:
            kw = {"plain": {}, "div": dict(use_div_offsets=True), "te": dict(use_time_embedding=True)}[kind]
            self.params[kind] = _params(**kw)
            self.gpu[kind] = DNGPradianceField.from_params(self.params[kind], DEV).eval()
        if (kind, prec) not in self.cpu:
            self.cpu[kind, prec] = self.oracle.OracleField(self.params[kind], mlp_half=prec)
        f = self.gpu[kind]
        f.set_mlp_precision(prec)
        return f, self.cpu[kind, prec]


@pytest.fixture(scope="module")
def fields(oracle):
    return _Fields(oracle)


def _rays(seed=3):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-1.2, 1.2, size=(N_RAYS, 3)).astype(np.float32)
    d = rng.normal(size=(N_RAYS, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    ts = rng.uniform(0, 1, size=N_RAYS).astype(np.float32)
    return o, d, ts


def _samples(n, seed):
    """n samples on rays referenced in no order, several per ray"""
    rng = np.random.default_rng(seed)
    ri = rng.integers(0, N_RAYS, size=n).astype(np.int64)
    t0 = rng.uniform(0, 0.6, size=n).astype(np.float32)
    t1 = (t0 + np.float32(0.01)).astype(np.float32)
    return ri, t0, t1


def _launch(f, o, d, ri, t0, t1, ts, t_per_ray, n_dev=None):
    """ced_field_forward_rays into pre-filled buffers -> (rgb [n,3], sigma [n]) as numpy"""
    from ced_nerf_amd import _lib
    n = ri.shape[0]
    keep = [T(o), T(d), T(ri), T(t0), T(t1), T(ts)]
    rgb = torch.full((n, 3), float(FILL), device=DEV)
    sigma = torch.full((n,), float(FILL), device=DEV)
    nd = torch.tensor([n_dev], dtype=torch.int64, device=DEV) if n_dev is not None else None
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    desc = f._descriptor()
    rc = _lib.lib().ced_field_forward_rays(C.byref(desc), n, p(nd), *[p(t) for t in keep], int(t_per_ray), 1, p(rgb),
                                           p(sigma), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "field_forward_rays")
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), sigma.cpu().numpy()


def _expected(of, o, d, ri, t0, t1, ts, t_per_ray, n_dev=None):
    """What the kernel stores (module docstring), from the oracle's explicit-position entry"""
    n = ri.shape[0]
    n_eff = n if n_dev is None else min(n, n_dev)
    used = ri >= 0
    r = np.where(used, ri, 0)
    with np.errstate(all="ignore"):
        tm2 = np.where(used, t0 + t1, np.float32(0)).astype(np.float32)
    pos = (o[r] + (d[r] * tm2[:, None]) / np.float32(2)).astype(np.float32)
    t = ts[r] if t_per_ray else np.full(n, ts[0], np.float32)
    out = of.forward(pos, t, d[r])
    rgb, sigma = out["rgb"].copy(), out["density"].copy()
    stored = np.arange(n) < n_eff
    for b in range(0, n_eff, TILE):
        e = min(b + TILE, n_eff)
        if not used[b:e].any():
            stored[b:e] = False
    rgb[~stored] = FILL
    sigma[~stored] = FILL
    return rgb, sigma, stored & used


def _check(fields, prec, ri, t0, t1, t_per_ray, n_dev=None, kind="plain", rays=None, what=""):
    f, of = fields.get(prec, kind)
    o, d, ts = rays if rays is not None else _rays()
    rgb, sigma = _launch(f, o, d, ri, t0, t1, ts, t_per_ray, n_dev)
    w_rgb, w_sigma, live = _expected(of, o, d, ri, t0, t1, ts, t_per_ray, n_dev)
    assert_bitexact(sigma, w_sigma, f"sigma ({prec} {what})")
    assert_bitexact(rgb, w_rgb, f"rgb ({prec} {what})")
    return rgb, sigma, live


# the ragged last tile of either j (16 samples each), a lone sample, more than one workgroup's first tiles
@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 32, 33, 65, 1000])
@pytest.mark.parametrize("prec", PRECS)
def test_sample_counts(fields, prec, n):
    ri, t0, t1 = _samples(n, 100 + n)
    _, sigma, _ = _check(fields, prec, ri, t0, t1, True, what=f"n={n}")
    if n >= 65:
        assert (sigma > 0).any()


@pytest.mark.parametrize("t_per_ray", [False, True])
@pytest.mark.parametrize("prec", PRECS)
def test_shared_and_per_ray_time(fields, prec, t_per_ray):
    ri, t0, t1 = _samples(65, 7)
    _check(fields, prec, ri, t0, t1, t_per_ray, what=f"t_per_ray={t_per_ray}")


def _unused_pattern(name, n):
    m = np.zeros(n, bool)
    if name == "isolated":
        m[[0, 3, 17, 40, 63, n - 1]] = True
    elif name == "half":                    # a whole j half: second half of tile 0, first half of tile 1
        m[16:48] = True
    elif name == "tile":                    # a whole tile in the middle
        m[32:64] = True
    else:
        m[:] = True
    return m


@pytest.mark.parametrize("poison", [np.nan, 1e38])
@pytest.mark.parametrize("pattern", ["isolated", "half", "tile", "all"])
@pytest.mark.parametrize("prec", PRECS)
def test_unused_slots(fields, prec, pattern, poison):
    """t0 / t1 of an unused slot are loaded like any other and must not reach a result: not the slot's own, which is
    ray 0's at t0 + t1 = 0, and no neighbour's"""
    n = 100                                 # tiles 0..31, 32..63, 64..95 and the ragged 96..99
    ri, t0, t1 = _samples(n, 11)
    unused = _unused_pattern(pattern, n)
    ri = np.where(unused, -1, ri).astype(np.int64)
    rgb_c, sigma_c, live = _check(fields, prec, ri, t0, t1, True, what=f"{pattern}, clean")
    t0p, t1p = t0.copy(), t1.copy()
    t0p[unused] = poison
    t1p[unused] = poison
    rgb_p, sigma_p, _ = _check(fields, prec, ri, t0p, t1p, True, what=f"{pattern}, poisoned {poison}")
    assert_bitexact(sigma_p, sigma_c, "sigma, poisoned against clean")
    assert_bitexact(rgb_p, rgb_c, "rgb, poisoned against clean")
    assert np.isfinite(sigma_p).all() and np.isfinite(rgb_p).all()
    assert live.sum() == n - unused.sum()
    if pattern == "tile":
        assert (sigma_p[32:64] == FILL).all() and (rgb_p[32:64] == FILL).all()
    if pattern == "all":
        assert (sigma_p == FILL).all() and (rgb_p == FILL).all()
    if pattern in ("isolated", "half"):     # stored: ray 0 at its origin, the same value in every such slot
        assert (sigma_p[unused] != FILL).all() and len(set(sigma_p[unused].view(np.uint32).tolist())) == 1


@pytest.mark.parametrize("prec", PRECS)
def test_device_side_count(fields, prec):
    """n_dev < n: the tiles end at n_dev; a last tile of one unused slot is a tile of unused slots only"""
    ri, t0, t1 = _samples(70, 13)
    _, sigma, _ = _check(fields, prec, ri, t0, t1, True, n_dev=33, what="n_dev=33")
    assert (sigma[:33] != FILL).all() and (sigma[33:] == FILL).all()
    ri[32] = -1
    _, sigma, _ = _check(fields, prec, ri, t0, t1, True, n_dev=33, what="n_dev=33, slot 32 unused")
    assert (sigma[32:] == FILL).all()
    _check(fields, prec, ri, t0, t1, False, n_dev=17, what="n_dev=17")
    _check(fields, prec, ri, t0, t1, True, n_dev=1000, what="n_dev > n")


@pytest.mark.parametrize("prec", PRECS)
def test_ray_order(fields, prec):
    """a wave's sixteen samples of one j on one ray, and on sixteen rays in falling order"""
    n = 96
    _, t0, t1 = _samples(n, 17)
    ri = np.empty(n, np.int64)
    ri[0:16] = 5
    ri[16:32] = np.arange(40, 24, -1)
    ri[32:48] = np.arange(16)
    ri[48:64] = N_RAYS - 1
    ri[64:96] = np.repeat(np.arange(30, 14, -1), 2)
    _check(fields, prec, ri, t0, t1, True, what="ray order")


@pytest.mark.parametrize("prec", PRECS)
def test_clamps_and_selector(fields, prec):
    """positions outside the box on one axis only, on the box's faces and corners: t0 = t1 = 0 puts a sample at its ray's
    origin exactly"""
    o, d, ts = _rays()
    pts = [[1.6, 0.2, 0.3], [0.2, -1.6, 0.3], [0.2, 0.3, 1.6], [-1.7, 0.0, 0.0], [1.5, 0.0, 0.0], [-1.5, 0.0, 0.0],
           [0.0, 1.5, 0.0], [0.0, 0.0, -1.5], [1.5, 1.5, 1.5], [-1.5, -1.5, -1.5], [0.0, 0.0, 0.0], [1.4999999, 0.1, 0.1],
           [0.1, -1.4999999, 0.1], [3.0, 3.0, 3.0]]
    o[:len(pts)] = np.asarray(pts, np.float32)
    n = 33
    ri = (np.arange(n) % (len(pts) + 3)).astype(np.int64)
    z = np.zeros(n, np.float32)
    _, sigma, _ = _check(fields, prec, ri, z, z, True, rays=(o, d, ts), what="clamps")
    assert (sigma[ri < 4] == 0).all() and (sigma == 0).any() and (sigma > 0).any()


@pytest.mark.parametrize("kind", ["div", "te"])
@pytest.mark.parametrize("prec", PRECS)
def test_div_offsets_and_time_embedding(fields, prec, kind):
    ri, t0, t1 = _samples(33, 19)
    ri[[4, 20]] = -1
    _check(fields, prec, ri, t0, t1, True, kind=kind, what=kind)


# --- the frame loop's own arguments: 32-bit ray indices, the window of the sample arrays, the per-ray SH array ---
@pytest.mark.parametrize("wh", [(16, 16), (24, 8)])
def test_tiny_frame(oracle, wh):
    """render_image_test on a frame of a few tiles, f16x2: schedule, totals and every pixel bit for bit against the
    oracle, with the colour head's SH inputs per ray and per sample, and with the shared timestamp handed per ray"""
    from ced_nerf_amd import _lib, ops, synthetic as S
    from ced_nerf_amd.model import DNGPradianceField
    from ced_nerf_amd.nerfacc_api import OccGridEstimator
    from ced_nerf_amd.utils import Rays, render_image_test
    sc = S.make_scene("dnerf", wh[0], wh[1], "trained", log2_hashmap_size=17)
    cfg = sc["cfg"]
    oest = oracle.OracleEstimator(cfg["aabb"], cfg["grid_resolution"], cfg["grid_levels"], sc["binaries"])
    trace = []
    w_rgb, w_op, w_dp, w_total = oracle.render_image_test(1024, oracle.OracleField(sc["params"], mlp_half="f16x2"), oest,
                                                          sc["origins"], sc["viewdirs"], timestamps=sc["timestamps"],
                                                          trace=trace, **sc["render"])
    want_iters = [dict(n_alive=t["n_alive"], n_samples=t["n_samples"], n_new=t["n_new"]) for t in trace]
    assert w_total > 200
    f = DNGPradianceField.from_params(sc["params"], DEV).eval()
    f.set_mlp_precision("f16x2")
    est = OccGridEstimator(cfg["aabb"], cfg["grid_resolution"], cfg["grid_levels"]).to(DEV)
    est.set_binaries(T(sc["binaries"]))
    rays = Rays(origins=T(sc["origins"]), viewdirs=T(sc["viewdirs"]))
    rk = dict(sc["render"]); rk["render_bkgd"] = T(rk["render_bkgd"])
    n = wh[0] * wh[1]
    L = _lib.lib()
    try:
        for sh_per_ray in (1, 0):
            assert L.ced_set_option(b"frame_sh_per_ray", sh_per_ray) == 0
            tracer = ops.FrameTracer(capacity=1100, with_events=False)
            rgb, op, dp, total = render_image_test(1024, f, est, rays, timestamps=T(sc["timestamps"]), tracer=tracer, **rk)
            what = f"{wh[0]}x{wh[1]}, sh_per_ray={sh_per_ray}"
            assert total == w_total and tracer.iterations() == want_iters, what
            assert_bitexact(rgb.cpu().numpy(), w_rgb, f"rgb ({what})")
            assert_bitexact(op.cpu().numpy(), w_op, f"opacity ({what})")
            assert_bitexact(dp.cpu().numpy(), w_dp, f"depth ({what})")
            # per-ray time: the same timestamp once per ray
            ts = T(np.full(n, sc["timestamps"].reshape(-1)[0], np.float32))
            r2, o2, d2, t2 = ops.render_image_test_native(
                f._descriptor(), rays.origins.reshape(-1, 3).contiguous(), rays.viewdirs.reshape(-1, 3).contiguous(),
                est.binaries, est.aabbs.contiguous(), rk["near_plane"], rk["far_plane"], rk["render_step_size"],
                rk["cone_angle"], 1e-4, 1024, ts, True, rk["render_bkgd"].reshape(-1).contiguous(),
                accel=est.occupancy_accel())
            assert t2 == w_total, what
            assert_bitexact(r2.cpu().numpy().reshape(w_rgb.shape), w_rgb, f"rgb, per-ray time ({what})")
            assert_bitexact(o2.cpu().numpy().reshape(w_op.shape), w_op, f"opacity, per-ray time ({what})")
            assert_bitexact(d2.cpu().numpy().reshape(w_dp.shape), w_dp, f"depth, per-ray time ({what})")
    finally:
        L.ced_set_option(b"frame_sh_per_ray", 1)
