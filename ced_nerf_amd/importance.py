"""DyNeRF's importance-sampling weight maps (csrc/importance.hip; datasets/dnerf_3d_video_IS.py:13-76, 187).

The reference spends a DyNeRF scene's rays where the pixels differ from their camera's temporal median (ISG) or change
between nearby frames (IST); its maps come from a notebook (gen_isg_ist.ipynb) that holds the whole clip in float32 on
the host.  Here the three steps run on the device from the uint8 images of a `TrainViews`, viewed as [C, T, H, W, 3]
(C cameras x T frames, camera-major, the reference's order):

    median = temporal_median(views, n_cameras)               # uint8  [C, H, W, 3]
    isg = isg_weights(views, n_cameras, gamma=2e-2)          # float32 [C, T, H, W]
    ist = ist_weights(views, n_cameras, alpha=0.1, frame_shift=25)
    data = views.batch_importance(num_rays, step, isg.reshape(-1))

The `*_reference` functions restate the formulas in numpy float32, rounding for rounding; the tests compare every bit.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .trainset import TrainViews


def _clip_shape(views: TrainViews, n_cameras: int) -> Tuple[int, int, int, int]:
    n_cameras = int(n_cameras)
    if views.channels != 3:
        raise ValueError("the sampling weights are defined on RGB views; these are RGBA")
    if n_cameras < 1 or len(views) % n_cameras:
        raise ValueError(f"{len(views)} views are not a whole number of frames of {n_cameras} cameras")
    if views.device.type != "cuda":
        raise NotImplementedError("the weight maps are computed on the GPU: the views must be on a cuda device")
    return n_cameras, len(views) // n_cameras, views.height, views.width


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def temporal_median(views: TrainViews, n_cameras: int) -> torch.Tensor:
    """uint8 [C, H, W, 3]: per camera, pixel and channel the median over the frames, the lower middle value for an even
    count (torch.median, dnerf_3d_video_IS.py:187)."""
    c, t, h, w = _clip_shape(views, n_cameras)
    out = torch.empty((c, h, w, 3), device=views.device, dtype=torch.uint8)
    with torch.cuda.device(views.device):
        rc = _lib.lib().ced_temporal_median_u8(c, t, h, w, C.c_void_p(views.images.data_ptr()),
                                               C.c_void_p(out.data_ptr()), _stream())
    _lib.check(rc, "temporal_median_u8")
    return out


def isg_weights(views: TrainViews, n_cameras: int, gamma: float = 2e-2, median: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 [C, T, H, W]: dynerf_isg_weight(images, median, gamma).  The notebook's gamma is 2e-2 (1e-3 for
    key-frames).  `median`: uint8 [C, H, W, 3] on the views' device (default: temporal_median)."""
    c, t, h, w = _clip_shape(views, n_cameras)
    if median is None:
        median = temporal_median(views, n_cameras)
    if median.dtype != torch.uint8 or tuple(median.shape) != (c, h, w, 3) or median.device != views.device:
        raise ValueError(f"median must be uint8 [{c},{h},{w},3] on {views.device}, got {tuple(median.shape)} "
                         f"{median.dtype} on {median.device}")
    median = median.contiguous()
    out = torch.empty((c, t, h, w), device=views.device, dtype=torch.float32)
    with torch.cuda.device(views.device):
        rc = _lib.lib().ced_isg_weights(c, t, h, w, C.c_void_p(views.images.data_ptr()), C.c_void_p(median.data_ptr()),
                                        float(gamma), C.c_void_p(out.data_ptr()), _stream())
    _lib.check(rc, "isg_weights")
    return out


def ist_weights(views: TrainViews, n_cameras: int, alpha: float = 0.1, frame_shift: int = 25) -> torch.Tensor:
    """float32 [C, T, H, W]: dynerf_ist_weight_nice(images, n_cameras, alpha, frame_shift)."""
    c, t, h, w = _clip_shape(views, n_cameras)
    if int(frame_shift) < 0:
        raise ValueError(f"frame_shift must be >= 0, got {frame_shift}")
    out = torch.empty((c, t, h, w), device=views.device, dtype=torch.float32)
    with torch.cuda.device(views.device):
        rc = _lib.lib().ced_ist_weights(c, t, h, w, C.c_void_p(views.images.data_ptr()), float(alpha), int(frame_shift),
                                        C.c_void_p(out.data_ptr()), _stream())
    _lib.check(rc, "ist_weights")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The three formulas in numpy (tests only)
# ---------------------------------------------------------------------------------------------------------------------
def _clip(images, n_cameras: int) -> np.ndarray:
    a = np.ascontiguousarray(images)
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[-1] != 3:
        raise ValueError(f"images must be uint8 [V,H,W,3], got {a.shape} {a.dtype}")
    if n_cameras < 1 or a.shape[0] % n_cameras:
        raise ValueError(f"{a.shape[0]} views are not a whole number of frames of {n_cameras} cameras")
    return a.reshape(n_cameras, a.shape[0] // n_cameras, *a.shape[1:])


def temporal_median_reference(images, n_cameras: int) -> np.ndarray:
    """uint8 [C, H, W, 3]: the element of rank (T - 1) // 2 of the sorted frames (torch.median's lower middle)."""
    clip = _clip(images, n_cameras)
    return np.ascontiguousarray(np.sort(clip, axis=1)[:, (clip.shape[1] - 1) // 2])


def isg_weights_reference(images, n_cameras: int, gamma: float = 2e-2, median=None) -> np.ndarray:
    """float32 [C, T, H, W]: a = u8 / 255, m = med / 255, d = a - m, q = d * d, p = q / (q + gamma^2) with gamma^2 formed
    in float32, (p0 + p1 + p2) * float32(1/3) summed left to right."""
    f32 = np.float32
    clip = _clip(images, n_cameras)
    med = temporal_median_reference(images, n_cameras) if median is None else np.asarray(median)
    a = clip.astype(f32) / f32(255.0)
    m = med[:, None].astype(f32) / f32(255.0)
    d = a - m
    q = d * d
    g2 = f32(gamma) * f32(gamma)
    p = q / (q + g2)
    out = ((p[..., 0] + p[..., 1]) + p[..., 2]) * f32(1.0 / 3.0)
    assert out.dtype == f32
    return out


def ist_weights_reference(images, n_cameras: int, alpha: float = 0.1, frame_shift: int = 25) -> np.ndarray:
    """float32 [C, T, H, W]: the reference's loop, shift by shift, a neighbour outside the clip being a zero frame."""
    f32 = np.float32
    frames = _clip(images, n_cameras).astype(f32)
    n_t = frames.shape[1]
    best = np.zeros_like(frames)
    for shift in range(1, int(frame_shift) + 1):
        left = np.zeros_like(frames)                      # frames[t + shift]
        right = np.zeros_like(frames)                     # frames[t - shift]
        if shift < n_t:
            left[:, :n_t - shift] = frames[:, shift:]
            right[:, shift:] = frames[:, :n_t - shift]
        best = np.maximum(best, np.maximum(np.abs(left - frames), np.abs(right - frames)))
    mean = ((best[..., 0] + best[..., 1]) + best[..., 2]) / f32(3.0)
    out = np.maximum(mean, f32(alpha))
    assert out.dtype == f32
    return out
