"""Float64 numpy restatement of SSIM / MS-SSIM (the algorithm of pytorch_msssim 1.0.0 as the evaluation step calls it,
written from its description, not from the package) and of the PSNR: the oracle of tests/test_metrics_cpu.py and
tests/test_gpu_metrics.py."""
import numpy as np

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def window(win_size=11, sigma=1.5):
    """The normalised Gaussian, computed in float32 as the package does (returned as float64)."""
    coords = np.arange(win_size, dtype=np.float32) - np.float32(win_size // 2)
    g = np.exp(-(coords ** 2) / np.float32(2 * sigma ** 2)).astype(np.float32)
    g = g / g.sum(dtype=np.float32)
    return g.astype(np.float64)


def filter_valid(x, g):
    """Separable valid convolution of [..., H, W] with the 1-D window g, along H and then along W."""
    w = len(g)
    h = sum(g[k] * x[..., k:x.shape[-2] - w + 1 + k, :] for k in range(w))
    return sum(g[k] * h[..., :, k:x.shape[-1] - w + 1 + k] for k in range(w))


def level(x, y, g, data_range=1.0, K=(0.01, 0.03)):
    """(cs, ssim) means over the valid region of one level, [N, C] each."""
    c1, c2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    mx, my = filter_valid(x, g), filter_valid(y, g)
    sxx = filter_valid(x * x, g) - mx * mx
    syy = filter_valid(y * y, g) - my * my
    sxy = filter_valid(x * y, g) - mx * my
    cs = (2 * sxy + c2) / (sxx + syy + c2)
    ss = (2 * mx * my + c1) / (mx * mx + my * my + c1) * cs
    return cs.mean(axis=(-2, -1)), ss.mean(axis=(-2, -1))


def pool(x):
    """avg_pool2d(kernel 2, stride 2, padding (H%2, W%2)), count_include_pad, floor mode."""
    H, W = x.shape[-2:]
    ph, pw = H % 2, W % 2
    xp = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(ph, ph), (pw, pw)])
    ho, wo = (H + 2 * ph - 2) // 2 + 1, (W + 2 * pw - 2) // 2 + 1
    return (xp[..., 0:2 * ho:2, 0:2 * wo:2] + xp[..., 1:2 * ho:2, 0:2 * wo:2]
            + xp[..., 0:2 * ho:2, 1:2 * wo:2] + xp[..., 1:2 * ho:2, 1:2 * wo:2]) / 4.0


def pyramid(X, Y, levels=5, g=None, data_range=1.0, K=(0.01, 0.03)):
    """[levels, N, C, 2]: the (cs, ssim) means of every level, before any relu."""
    g = window() if g is None else np.asarray(g, np.float64)
    x, y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    out = []
    for lv in range(levels):
        out.append(np.stack(level(x, y, g, data_range, K), axis=-1))
        if lv < levels - 1:
            x, y = pool(x), pool(y)
    return np.stack(out)


def ms_ssim_from_levels(lv, weights=WEIGHTS):
    """Per image [N]: prod_{l<L-1} relu(cs_l)^w_l * relu(ssim_{L-1})^w_{L-1}, averaged over the channels."""
    w = np.asarray(weights, np.float32).astype(np.float64)
    vals = np.concatenate([lv[:-1, ..., 0], lv[-1:, ..., 1]])
    return np.prod(np.maximum(vals, 0.0) ** w[:, None, None], axis=0).mean(axis=1)


def ms_ssim(X, Y, data_range=1.0, weights=WEIGHTS, g=None, K=(0.01, 0.03)):
    return ms_ssim_from_levels(pyramid(X, Y, len(weights), g, data_range, K), weights)


def ssim(X, Y, data_range=1.0, g=None, K=(0.01, 0.03), nonnegative=False):
    s = pyramid(X, Y, 1, g, data_range, K)[0, ..., 1]
    return (np.maximum(s, 0.0) if nonnegative else s).mean(axis=1)


def psnr(X, Y):
    mse = np.mean((np.asarray(X, np.float64) - np.asarray(Y, np.float64)) ** 2)
    with np.errstate(divide="ignore"):
        return -10.0 * np.log(mse) / np.log(10.0)
