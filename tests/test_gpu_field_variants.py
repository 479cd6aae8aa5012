"""Every field kernel, per sample and in rays mode: eight table / time variants (tests/field_variants.py: the launchers'
selector, sel = time encoding | fp16 table << 1 | temporal table << 2) times four arithmetic modes, each output bit for
bit against the CPU oracle's mode of the same name.

  sel  table            flags                                 f32          f16x2        f16          f32+h16x2
  0    fp32             -                                     P  f  F      P  e  F      P  e  F      P  f  F
  1    fp32             te, div                               P  f  F      P  e  F      P  e  F      P  f  F
  2    fp16             -                                     P  R  F      P  R  F      P  R  F      P  R  F
  3    fp16             te + attenuation, div                 P  R  F      P  R  F      P  R  F      P  R  F
  4    temporal fp32    -                                     P  R  F      P  R  F      P  R  F      P  R  F
  5    temporal fp32    te, div                               P  R  F      P  R  F      P  R  F      P  R  F
  6    temporal fp16    -                                     P  R  F      P  R  F      P  R  F      P  R  F
  7    temporal fp16    te + attenuation, div                 P  R  F      P  R  F      P  R  F      P  R  F

P = test_per_sample here (ced_field_forward and its density-only launch), R = test_rays_mode here
(ced_field_forward_rays), F = tests/test_gpu_frame_variants.py::test_render_image_test (the frame loop; it launches the
field kernel in rays mode only).  Rays mode of sel 0 and 1: e = tests/test_gpu_field_front_end.py (f16x2, f16; kinds
plain, div, te), f = column F's frames, whose loop is what launches the exact and mixed kernels in rays mode.

With a temporal table the sample's time picks the key-frame pair (min(floor(3 t), 2)), not only the time encoding's
inputs, so the times here sit on the key-frames, one float32 to either side of them, and uniformly in between: the lanes
of one wave are in all three intervals.  The rays-mode launch, its pre-filled outputs and what an unused slot stores are
tests/test_gpu_field_front_end.py's (_launch, _expected, _check), imported."""
import numpy as np
import pytest
import torch

import field_variants as V
from conftest import assert_bitexact
from test_gpu_field_front_end import FILL, N_RAYS, _check, _rays, _samples

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HALF_MODES = ["f16x2", "f16"]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


class _Fields:
    """One GPU field per variant and one oracle field per (variant, mode), made on first use and kept; get() has the
    signature test_gpu_field_front_end._check asks for, with the selector as `kind`"""

    def __init__(self, oracle):
        self.oracle, self.params, self.gpu, self.cpu = oracle, {}, {}, {}

    def get(self, prec, kind):
        from ced_nerf_amd.model import DNGPradianceField
        if kind not in self.params:
            self.params[kind] = V.field_params(kind)
            self.gpu[kind] = DNGPradianceField.from_params(self.params[kind], DEV).eval()
        if (kind, prec) not in self.cpu:
            self.cpu[kind, prec] = self.oracle.OracleField(self.params[kind], mlp_half=prec)
        f = self.gpu[kind]
        f.set_mlp_precision(prec)
        return f, self.cpu[kind, prec]


@pytest.fixture(scope="module")
def fields(oracle):
    return _Fields(oracle)


# --- 1. per-sample mode: all 32 kernels ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", V.MODES)
@pytest.mark.parametrize("sel", V.SELS)
def test_per_sample(fields, sel, mode):
    """ced_field_forward on 1061 samples -- 33 wave tiles of the half kernels with a ragged last one, and more than one
    workgroup at 1024, 768 and 512 threads -- rgb, density and the geometry features, and the density-only launch"""
    n = 1061
    f, of = fields.get(mode, sel)
    pos, t, d = V.sample_points(n)
    iv = V.keyframe_interval(t.reshape(-1))
    assert all(set(iv[b:b + 64].tolist()) == {0, 1, 2} for b in range(0, n - 64, 64))   # every wave straddles
    want = of.forward(pos, t, d, want_geo=True)
    assert (want["density"] == 0).any() and (want["density"] > 0).any()
    rgb, res = f(T(pos), T(t), T(d))
    tag = f"sel {sel} {mode}"
    assert rgb.shape == (n, 3) and res["density"].shape == (n, 1) and res["base_mlp_out"].shape == (n, 15)
    assert_bitexact(N(res["base_mlp_out"]), want["base_mlp_out"], tag + " base_mlp_out")
    assert_bitexact(N(res["density"])[:, 0], want["density"], tag + " density")
    assert_bitexact(N(rgb), want["rgb"], tag + " rgb")
    dens = f.query_density(T(pos), T(t))
    assert_bitexact(N(dens["density"])[:, 0], want["density"], tag + " query_density")


# --- 2. rays mode: the field kernel alone -------------------------------------------------------------------------
RAYS_SELS = [2, 3, 4, 5, 6, 7]                    # sel 0 and 1 are test_gpu_field_front_end.py's


def _variant_rays(t_per_ray):
    """test_gpu_field_front_end's rays with the key-frame times per ray; shared time: ray 0 carries the float32 below 2/3"""
    o, d, _ = _rays()
    ts = V.sample_times(N_RAYS, np.random.default_rng(5))
    if not t_per_ray:
        ts = np.roll(ts, -6)
        assert ts[0] == np.nextafter(V.T23, np.float32(0))
    return o, d, ts


@pytest.mark.parametrize("t_per_ray", [False, True])
@pytest.mark.parametrize("mode", V.MODES)
@pytest.mark.parametrize("sel", RAYS_SELS)
def test_rays_mode(fields, sel, mode, t_per_ray):
    """ced_field_forward_rays: a lone sample, a ragged second half-tile, a ragged second tile, more than one workgroup.
    The samples name their rays in no order, so with per-ray time one tile's lanes are in different key-frame intervals."""
    rays = _variant_rays(t_per_ray)
    for n in (1, 17, 33, 1000):
        ri, t0, t1 = _samples(n, 100 + n)
        if t_per_ray and n >= 33:
            iv = V.keyframe_interval(rays[2][ri])
            assert set(iv[:32].tolist()) == {0, 1, 2}
        _, sigma, _ = _check(fields, mode, ri, t0, t1, t_per_ray, kind=sel, rays=rays,
                             what=f"sel {sel}, n={n}, t_per_ray={t_per_ray}")
        if n == 1000:
            assert (sigma > 0).any()


@pytest.mark.parametrize("mode", HALF_MODES)
@pytest.mark.parametrize("sel", RAYS_SELS)
def test_rays_mode_unused_slots(fields, sel, mode):
    """Unused slots (ray index -1) covering a whole half of two tiles, their t0 / t1 poisoned with NaN: the slot stores
    ray 0 at its origin and at ray 0's time, and the poison reaches neither that nor a neighbour"""
    n = 100
    rays = _variant_rays(True)
    ri, t0, t1 = _samples(n, 11)
    unused = np.zeros(n, bool)
    unused[16:48] = True
    ri = np.where(unused, -1, ri).astype(np.int64)
    rgb_c, sigma_c, live = _check(fields, mode, ri, t0, t1, True, kind=sel, rays=rays, what=f"sel {sel}, clean")
    t0p, t1p = t0.copy(), t1.copy()
    t0p[unused] = np.nan
    t1p[unused] = np.nan
    rgb_p, sigma_p, _ = _check(fields, mode, ri, t0p, t1p, True, kind=sel, rays=rays, what=f"sel {sel}, poisoned")
    assert_bitexact(sigma_p, sigma_c, "sigma, poisoned against clean")
    assert_bitexact(rgb_p, rgb_c, "rgb, poisoned against clean")
    assert np.isfinite(sigma_p).all() and np.isfinite(rgb_p).all()
    assert live.sum() == n - unused.sum()
    assert (sigma_p[unused] != FILL).all() and len(set(sigma_p[unused].view(np.uint32).tolist())) == 1
    # a tile of unused slots only stores nothing: the outputs keep what they were filled with
    ri[64:96] = -1
    _, sigma_s, _ = _check(fields, mode, ri, t0p, t1p, True, kind=sel, rays=rays, what=f"sel {sel}, skipped tile")
    assert (sigma_s[64:96] == FILL).all() and (sigma_s[96:] != FILL).all()
