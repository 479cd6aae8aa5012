"""The reference's evaluation step (train_real.py:443-520): PSNR and MS-SSIM of rendered views against their ground truth.

  `ms_ssim`, `ssim`    drop-ins for pytorch_msssim 1.0.0's functions (train_real.py:18,497-500) on [N,C,H,W] float32
                       CUDA tensors, strided views included; forward only
  `psnr`               -10 ln(mse) / ln 10 as train_real.py:494-495 computes it, the MSE accumulated in fp64
  `evaluate_views`     the loop of train_real.py:443-520: render every test view, score it, one host transfer at the end

All three metrics run on the HIP kernels of csrc/metrics.hip (ced_ssim): one fused pass per pyramid level and one
finishing launch, on the caller's stream, with no host synchronisation.  There is no CPU or torch fallback.
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, List, Optional, Sequence

import torch
from torch import Tensor

from . import ops
from .utils import Rays, grid_for, render_frames_test, render_image_test

MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)   # pytorch_msssim's default level weights


def gaussian_window(win_size: int = 11, win_sigma: float = 1.5) -> List[float]:
    """pytorch_msssim's _fspecial_gauss_1d, computed the same way (float32 torch on the CPU): the 1-D window as floats."""
    coords = torch.arange(win_size, dtype=torch.float)
    coords -= win_size // 2
    g = torch.exp(-(coords ** 2) / (2 * win_sigma ** 2))
    g /= g.sum()
    return g.tolist()


def _check_pair(X: Tensor, Y: Tensor, win, win_size: int) -> None:
    """pytorch_msssim's argument checks, plus what is not built (custom windows, 5-D inputs, other dtypes, gradients).
    The device is checked by ops.ssim: a CPU tensor raises there, there is no CPU fallback."""
    if not isinstance(X, Tensor) or not isinstance(Y, Tensor):
        raise TypeError("X and Y must be tensors")
    if tuple(X.shape) != tuple(Y.shape):
        raise ValueError(f"Input images should have the same dimensions, but got {tuple(X.shape)} and {tuple(Y.shape)}.")
    if X.dim() == 5:
        raise NotImplementedError("5-D (video) inputs are not built: pass [N,C,H,W] images")
    if X.dim() != 4:
        raise ValueError(f"Input images should be 4-d tensors [N,C,H,W], but got {tuple(X.shape)}")
    if win is not None:
        raise NotImplementedError("a custom `win` is not built: pass win_size / win_sigma (the Gaussian window)")
    if win_size % 2 != 1:
        raise ValueError("Window size should be odd.")
    if win_size > 15:
        raise NotImplementedError(f"win_size {win_size} is not built: the kernels stage windows of at most 15")
    for name, t in (("X", X), ("Y", Y)):
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be torch.float32, got {t.dtype}")
        if t.requires_grad:
            raise RuntimeError(f"{name} requires grad: these metrics are forward only (no gradient is built); "
                               "pass a detached tensor")


def ms_ssim(X: Tensor, Y: Tensor, data_range: float = 255, size_average: bool = True, win_size: int = 11,
            win_sigma: float = 1.5, win=None, weights: Optional[Sequence[float]] = None, K=(0.01, 0.03)) -> Tensor:
    """pytorch_msssim.ms_ssim: a 0-dim tensor (size_average) or one value per image [N], float32, on the device."""
    _check_pair(X, Y, win, win_size)
    smaller_side = min(X.shape[-2:])
    if not smaller_side > (win_size - 1) * (2 ** 4):
        raise ValueError("Image size should be larger than %d due to the 4 downsamplings in ms-ssim"
                         % ((win_size - 1) * (2 ** 4)))
    if weights is None:
        weights = MS_SSIM_WEIGHTS
    w32 = torch.tensor(weights, dtype=torch.float32).reshape(-1).tolist()     # X.new_tensor(weights): float32
    per_image, mean, _, _ = ops.ssim(X, Y, gaussian_window(win_size, win_sigma), len(w32), weights=w32,
                                     data_range=data_range, K=K, want_mean=size_average)
    return mean if size_average else per_image


def ssim(X: Tensor, Y: Tensor, data_range: float = 255, size_average: bool = True, win_size: int = 11,
         win_sigma: float = 1.5, win=None, K=(0.01, 0.03), nonnegative_ssim: bool = False) -> Tensor:
    """pytorch_msssim.ssim: a 0-dim tensor (size_average) or one value per image [N], float32, on the device.  Both sides
    must be at least win_size (the package would skip the filter along a shorter side)."""
    _check_pair(X, Y, win, win_size)
    if min(X.shape[-2:]) < win_size:
        raise ValueError(f"Image size {tuple(X.shape[-2:])} is smaller than the {win_size}-wide window")
    per_image, mean, _, _ = ops.ssim(X, Y, gaussian_window(win_size, win_sigma), 1, data_range=data_range, K=K,
                                     nonnegative=nonnegative_ssim, want_mean=size_average)
    return mean if size_average else per_image


def _mse_psnr(mse: Tensor) -> Tensor:
    return -10.0 * torch.log(mse) / math.log(10.0)


def psnr(rgb: Tensor, pixels: Tensor) -> Tensor:
    """-10 ln(mse) / ln 10 over all elements (train_real.py:494-495), a 0-dim float64 tensor on the device; the MSE is
    accumulated in fp64 by the HIP kernel, identical inputs give inf.  rgb, pixels: float32 CUDA tensors of one shape;
    [H,W,C] frames are read in place."""
    if tuple(rgb.shape) != tuple(pixels.shape):
        raise ValueError(f"rgb and pixels must have the same shape, got {tuple(rgb.shape)} and {tuple(pixels.shape)}")
    if rgb.requires_grad or pixels.requires_grad:
        raise RuntimeError("psnr is forward only: pass detached tensors")
    if rgb.dim() == 3:
        X, Y = rgb.permute(2, 0, 1)[None], pixels.permute(2, 0, 1)[None]
    elif rgb.dim() == 4:
        X, Y = rgb, pixels
    else:
        X, Y = rgb.reshape(1, 1, 1, -1), pixels.reshape(1, 1, 1, -1)
    _, _, mse, _ = ops.ssim(X, Y, None, 0)
    return _mse_psnr(mse.mean() if mse.numel() > 1 else mse[0])


def _view_metrics(rgbs: Tensor, pixels: Tensor):
    """[F,H,W,3] renders and ground truths -> (ms_ssim [F] f32, psnr [F] f64) on the device, as train_real.py:494-500
    computes them per view (ms_ssim(pixels, rgb, data_range=1))."""
    X, Y = pixels.permute(0, 3, 1, 2), rgbs.permute(0, 3, 1, 2)
    _check_pair(X, Y, None, 11)
    if not min(X.shape[-2:]) > 160:
        raise ValueError("Image size should be larger than 160 due to the 4 downsamplings in ms-ssim")
    per_image, _, mse, _ = ops.ssim(X, Y, gaussian_window(11, 1.5), 5, weights=MS_SSIM_WEIGHTS, data_range=1.0,
                                    want_mean=False, want_mse=True)
    return per_image, _mse_psnr(mse)


def _same_bkgd(a, b) -> bool:
    if a is None or b is None:
        return a is None and b is None
    return a is b or (a.shape == b.shape and a.device == b.device and bool(torch.equal(a, b)))


@torch.no_grad()
def evaluate_views(radiance_field, estimator, views: Iterable[Dict], max_samples: int = 1024, frames_per_call: int = 1,
                   keep_frames: bool = False, **render_kwargs) -> Dict:
    """The evaluation loop of train_real.py:443-520.  `views` yields the reference's test items: dicts with `rays`
    (Rays of [H,W,3]), `pixels` [H,W,3], `timestamps` and `color_bkgd`.  Each view is rendered with
    `render_image_test(max_samples, ..., render_bkgd=color_bkgd, timestamps=timestamps, **render_kwargs)` and scored on
    the device: PSNR from the fp64 MSE, and `ms_ssim(pixels.permute(2,0,1)[None], rgb.permute(2,0,1)[None],
    data_range=1)`.  The figures come back in one host transfer at the end.

    frames_per_call > 1: up to that many consecutive views of equal size and background (one timestamp each) go through
    one `render_frames_test` call and one batched metric call; every figure is bit-identical to frames_per_call=1.
    keep_frames: also return the rendered rgb frames (device tensors).

    Returns {"psnr_avg", "ssim_avg", "psnrs" [views], "ssims" [views], "n_samples" [views], ("frames")}."""
    radiance_field.eval()
    estimator.eval()
    per_call = max(1, int(frames_per_call))
    ssims: List[Tensor] = []
    psnrs: List[Tensor] = []
    totals: List[int] = []
    frames: List[Tensor] = []
    group: List[Dict] = []

    def device_of(v):
        return v["rays"].origins.device

    def flush():
        if not group:
            return
        dev = device_of(group[0])
        bkgd = group[0]["color_bkgd"]
        if len(group) == 1:
            v = group[0]
            ts = v["timestamps"].to(dev)
            rgb, _, _, total = render_image_test(max_samples, radiance_field, grid_for(estimator, ts), v["rays"], render_bkgd=bkgd,
                                                 timestamps=ts, **render_kwargs)
            rgbs, n = rgb[None], [int(total)]
        else:
            rays = Rays(origins=torch.stack([v["rays"].origins for v in group]),
                        viewdirs=torch.stack([v["rays"].viewdirs for v in group]))
            ts = torch.cat([v["timestamps"].to(dev).reshape(-1) for v in group])
            rgbs, _, _, n = render_frames_test(max_samples, radiance_field, grid_for(estimator, ts), rays, render_bkgd=bkgd,
                                               timestamps=ts, **render_kwargs)
        pix = torch.stack([v["pixels"].to(dev, torch.float32) for v in group])
        s, p = _view_metrics(rgbs, pix)
        ssims.append(s)
        psnrs.append(p)
        totals.extend(int(t) for t in n)
        if keep_frames:
            frames.extend(rgbs.unbind(0))
        group.clear()

    for v in views:
        if group:
            g = group[0]
            if (len(group) >= per_call or tuple(v["pixels"].shape) != tuple(g["pixels"].shape)
                    or v["timestamps"].numel() != 1 or device_of(v) != device_of(g)
                    or not _same_bkgd(v["color_bkgd"], g["color_bkgd"])):
                flush()
        group.append(v)
        if per_call == 1 or v["timestamps"].numel() != 1:
            flush()
    flush()
    if not totals:
        raise ValueError("evaluate_views: no views")
    host = torch.stack([torch.cat(psnrs), torch.cat(ssims).double()]).cpu()        # the one host transfer
    psnr_list, ssim_list = host[0].tolist(), host[1].tolist()
    out = dict(psnr_avg=sum(psnr_list) / len(psnr_list), ssim_avg=sum(ssim_list) / len(ssim_list), psnrs=psnr_list,
               ssims=ssim_list, n_samples=totals)
    if keep_frames:
        out["frames"] = frames
    return out
