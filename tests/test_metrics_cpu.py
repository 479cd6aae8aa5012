"""SSIM / MS-SSIM / PSNR without a GPU: the float64 oracle (tests/ssim_oracle.py) against a float64 torch restatement and
closed-form answers, the argument checks of ced_nerf_amd.metrics and the error convention of ced_ssim."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ssim_oracle as SO


def _torch_pyramid(X, Y, levels=5, win_size=11, sigma=1.5, data_range=1.0, K=(0.01, 0.03)):
    """The same algorithm as conv2d / avg_pool2d calls in float64 on the CPU: [levels, N, C, 2]."""
    x, y = torch.from_numpy(np.asarray(X, np.float64)), torch.from_numpy(np.asarray(Y, np.float64))
    Ch = x.shape[1]
    g = torch.from_numpy(SO.window(win_size, sigma))
    wh = g.reshape(1, 1, -1, 1).repeat(Ch, 1, 1, 1)
    ww = g.reshape(1, 1, 1, -1).repeat(Ch, 1, 1, 1)
    filt = lambda t: F.conv2d(F.conv2d(t, wh, groups=Ch), ww, groups=Ch)
    c1, c2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    out = []
    for lv in range(levels):
        mx, my = filt(x), filt(y)
        sxx, syy, sxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
        cs = (2 * sxy + c2) / (sxx + syy + c2)
        ss = (2 * mx * my + c1) / (mx * mx + my * my + c1) * cs
        out.append(torch.stack([cs.flatten(2).mean(-1), ss.flatten(2).mean(-1)], -1))
        if lv < levels - 1:
            pad = [s % 2 for s in x.shape[2:]]
            x = F.avg_pool2d(x, kernel_size=2, padding=pad)
            y = F.avg_pool2d(y, kernel_size=2, padding=pad)
    return torch.stack(out).numpy()


def _smooth(rng, shape):
    n, c, h, w = shape
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    out = np.empty(shape)
    for i in range(n):
        for j in range(c):
            f = rng.uniform(0.5, 3.0, 4)
            out[i, j] = 0.5 + 0.25 * np.sin(2 * np.pi * (f[0] * xx + f[1] * yy)) + 0.2 * np.cos(2 * np.pi * f[2] * xx * yy + f[3])
    return out


@pytest.mark.parametrize("kind,shape", [("random", (2, 3, 173, 301)), ("smooth", (2, 3, 173, 301)),
                                        ("random", (1, 1, 536, 960)), ("smooth", (1, 3, 161, 161))])
def test_oracle_agrees_with_a_torch_float64_restatement(kind, shape):
    rng = np.random.default_rng(7)
    if kind == "random":
        X = rng.random(shape)
        Y = np.clip(X + 0.1 * rng.standard_normal(shape), 0, 1)
    else:
        X = _smooth(rng, shape)
        Y = np.clip(X + 0.05 * _smooth(rng, shape) - 0.025, 0, 1)
    lv = SO.pyramid(X, Y)
    ref = _torch_pyramid(X, Y)
    assert lv.shape == (5, shape[0], shape[1], 2)
    np.testing.assert_allclose(lv, ref, rtol=0, atol=1e-12)
    np.testing.assert_allclose(SO.ms_ssim(X, Y), SO.ms_ssim_from_levels(ref), rtol=0, atol=1e-12)


@pytest.mark.parametrize("win_size", [1, 3, 15])
def test_oracle_agrees_with_the_torch_restatement_at_other_windows(win_size):
    rng = np.random.default_rng(win_size)
    X = rng.random((1, 2, 227, 301))
    Y = np.clip(X + 0.1 * rng.standard_normal(X.shape), 0, 1)
    np.testing.assert_allclose(SO.pyramid(X, Y, g=SO.window(win_size)), _torch_pyramid(X, Y, win_size=win_size), rtol=0,
                               atol=1e-12)


def test_window():
    """metrics.gaussian_window is the package's float32 torch formula; the oracle's numpy float32 one agrees to an ulp."""
    from ced_nerf_amd import metrics as M
    coords = torch.arange(11, dtype=torch.float) - 5
    g = torch.exp(-(coords ** 2) / (2 * 1.5 ** 2))
    g = g / g.sum()
    assert M.gaussian_window() == g.tolist()
    np.testing.assert_allclose(SO.window(), np.asarray(M.gaussian_window()), rtol=3e-7, atol=0)
    assert len(M.gaussian_window(7, 1.0)) == 7


def test_identical_images():
    X = np.random.default_rng(1).random((2, 3, 200, 180))
    np.testing.assert_allclose(SO.ms_ssim(X, X), 1.0, rtol=0, atol=1e-14)
    np.testing.assert_allclose(SO.ssim(X, X), 1.0, rtol=0, atol=1e-14)
    assert SO.psnr(X, X) == np.inf


def _constant_level(a, b, c1=1e-4, c2=9e-4):
    """(cs, ssim) of one level of the constant images a, b.  The float32 window sums to s1 = 1 + O(1e-8), not 1, so the
    filtered moments are mu = a s, E[x^2] = a^2 s, sigma^2 = a^2 s (1 - s) with s = s1^2 (both passes); at s = 1 this is
    cs = 1, ssim = (2ab + C1) / (a^2 + b^2 + C1)."""
    s = float(SO.window().sum()) ** 2
    v = s * (1 - s)
    cs = (2 * a * b * v + c2) / ((a * a + b * b) * v + c2)
    return cs, (2 * a * b * s * s + c1) / ((a * a + b * b) * s * s + c1) * cs


def _luminance(a, b, c1=1e-4):
    return (2 * a * b + c1) / (a * a + b * b + c1)


def test_constant_images_every_level_even():
    a, b = 0.3, 0.7
    X, Y = np.full((1, 2, 256, 256), a), np.full((1, 2, 256, 256), b)    # 256 128 64 32 16: no padding anywhere
    lv = SO.pyramid(X, Y)
    cs, ss = _constant_level(a, b)
    np.testing.assert_allclose(lv[..., 0], cs, rtol=0, atol=1e-12)
    np.testing.assert_allclose(lv[..., 1], ss, rtol=0, atol=1e-12)
    np.testing.assert_allclose(lv[..., 0], 1.0, rtol=0, atol=1e-4)       # no variance: cs = C2 / C2
    np.testing.assert_allclose(lv[..., 1], _luminance(a, b), rtol=0, atol=1e-4)
    w = np.asarray(SO.WEIGHTS, np.float32).astype(np.float64)
    np.testing.assert_allclose(SO.ms_ssim(X, Y), np.prod(np.array([cs] * 4 + [ss]) ** w), rtol=0, atol=1e-12)


def test_constant_images_with_an_odd_level():
    """536 x 960: levels 536 268 134 67 34 rows.  Pooling the 67 rows pads one zero row at the top, so the last level is
    a/2 on its first row and a elsewhere; the earlier levels stay constant."""
    a, b = 0.3, 0.7
    X, Y = np.full((1, 1, 536, 960), a), np.full((1, 1, 536, 960), b)
    lv = SO.pyramid(X, Y)
    cs, ss = _constant_level(a, b)
    np.testing.assert_allclose(lv[:4, ..., 0], cs, rtol=0, atol=1e-12)
    np.testing.assert_allclose(lv[:4, ..., 1], ss, rtol=0, atol=1e-12)
    last_x, last_y = np.full((1, 1, 34, 60), a), np.full((1, 1, 34, 60), b)
    last_x[..., 0, :] = a / 2
    last_y[..., 0, :] = b / 2
    want = np.stack(SO.level(last_x, last_y, SO.window()), -1)
    np.testing.assert_allclose(lv[4], want, rtol=0, atol=1e-12)
    assert abs(lv[4, 0, 0, 1] - ss) > 1e-3                               # the padding row shows
    assert lv[4, 0, 0, 0] < cs - 1e-3


def test_product_weights_and_relu():
    rng = np.random.default_rng(3)
    X = rng.random((2, 3, 170, 190))
    Y = np.clip(X + 0.2 * rng.standard_normal(X.shape), 0, 1)
    lv = SO.pyramid(X, Y)
    w = np.asarray(SO.WEIGHTS, np.float32).astype(np.float64)
    by_hand = np.ones((2, 3))
    for i in range(4):
        by_hand *= np.maximum(lv[i, ..., 0], 0) ** w[i]
    by_hand *= np.maximum(lv[4, ..., 1], 0) ** w[4]
    np.testing.assert_allclose(SO.ms_ssim(X, Y), by_hand.mean(1), rtol=0, atol=1e-14)
    # anti-correlated images: cs < 0 at level 0, relu makes the product 0
    Z = 1.0 - X
    lz = SO.pyramid(X, Z)
    assert np.all(lz[0, ..., 0] < 0)
    np.testing.assert_array_equal(SO.ms_ssim(X, Z), 0.0)
    assert np.all(SO.ssim(X, Z) < 0) and np.all(SO.ssim(X, Z, nonnegative=True) == 0.0)


def test_python_argument_errors():
    from ced_nerf_amd import metrics as M
    x = torch.rand(1, 3, 200, 200)
    with pytest.raises(ValueError, match="larger than 160"):
        M.ms_ssim(torch.rand(1, 3, 160, 300), torch.rand(1, 3, 160, 300), data_range=1)
    with pytest.raises(ValueError, match="odd"):
        M.ms_ssim(x, x, win_size=10)
    with pytest.raises(ValueError, match="odd"):
        M.ssim(x, x, win_size=4)
    with pytest.raises(ValueError, match="4-d"):
        M.ms_ssim(x[0], x[0])
    with pytest.raises(NotImplementedError, match="5-D"):
        M.ms_ssim(x[None], x[None])
    with pytest.raises(NotImplementedError, match="win"):
        M.ssim(x, x, win=torch.ones(1, 1, 11))
    with pytest.raises(TypeError, match="float32"):
        M.ms_ssim(x.double(), x.double())
    with pytest.raises(ValueError, match="same dimensions"):
        M.ssim(x, x[:, :2])
    with pytest.raises(RuntimeError, match="forward only"):
        M.ssim(x.clone().requires_grad_(), x)
    with pytest.raises(NotImplementedError, match="at most 15"):
        M.ssim(x, x, win_size=17)
    with pytest.raises(NotImplementedError, match="cuda"):                # no CPU fallback
        M.ms_ssim(x, x, data_range=1)
    with pytest.raises(NotImplementedError, match="cuda"):
        M.psnr(x[0].permute(1, 2, 0), x[0].permute(1, 2, 0))


def test_ced_ssim_argument_errors_are_reported_not_thrown():
    from ced_nerf_amd import _lib
    L = _lib.lib()
    st = (C.c_int64 * 4)(3 * 200 * 200, 200 * 200, 200, 1)
    win = (C.c_float * 11)(*SO.window())
    wts = (C.c_float * 5)(*SO.WEIGHTS)
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below fails its checks before any launch

    def call(n=1, c=3, h=200, w=200, x=fake, y=fake, win_size=11, levels=5, weights=wts, out=fake, mean=None, mse=None,
             ws=fake, window=win):
        return L.ced_ssim(n, c, h, w, x, st, y, st, 1.0, 0.01, 0.03, win_size, window, levels, weights, 0, out, mean, mse,
                          None, ws, None)

    assert L.ced_ssim_workspace_bytes(1, 3, 200, 200, 11, 5) > 0
    assert L.ced_ssim_workspace_bytes(1, 3, 100, 200, 11, 5) < 0          # level 4 is 7 rows
    assert L.ced_ssim_workspace_bytes(0, 3, 200, 200, 11, 5) < 0
    assert L.ced_ssim_workspace_bytes(1, 1, 1, 1 << 31, 1, 0) < 0                # a side must fit in 32 bits
    assert b"2^31" in L.ced_last_error_string()
    assert L.ced_ssim_workspace_bytes(1, 3, 227, 301, 17, 5) < 0                 # windows of at most 15
    for kwargs, msg in ((dict(n=0), b"empty"), (dict(h=-5), b"empty"), (dict(h=100), b"smaller than the 11-wide window"),
                        (dict(win_size=10), b"odd"), (dict(levels=6), b"levels"), (dict(x=None), b"null pointer"),
                        (dict(ws=None), b"null pointer"), (dict(out=None), b"null pointer"),
                        (dict(weights=None), b"weights"), (dict(window=None), b"null pointer"),
                        (dict(levels=0, mean=fake, mse=fake), b"null pointer"),
                        (dict(ws=C.c_void_p(0x1004)), b"aligned")):
        rc = call(**kwargs)
        assert rc == -1, (kwargs, rc)
        assert msg in L.ced_last_error_string(), (kwargs, L.ced_last_error_string())
