"""Full-frame ray generation on the device.

The reference builds `Rays(origins, viewdirs)` on the host for every frame and uploads them
(datasets/dnerf_synthetic.py:191-242, gui.py:43-86, datasets/hypernerf.py:169-176); here the
camera parameters go to a HIP kernel that writes the [H,W,3] tensors directly.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from .utils import Rays


def _farr(values, n):
    a = np.asarray(values, np.float32).reshape(-1)
    if a.shape[0] != n:
        raise ValueError(f"expected {n} values, got {a.shape[0]}")
    return (C.c_float * n)(*[float(v) for v in a])


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def pinhole_rays(K, c2w, width: int, height: int, opengl: bool = True, device="cuda") -> Rays:
    """Rays of a pinhole camera: K [3,3] intrinsics, c2w [3,4] (or [4,4]) camera-to-world."""
    K = np.asarray(K, np.float32)
    c2w = np.asarray(c2w, np.float32)[:3, :4]
    dev = torch.device(device)
    if dev.type != "cuda":
        raise NotImplementedError("Only support cuda devices (no CPU fallback).")
    o = torch.empty((height, width, 3), device=dev, dtype=torch.float32)
    d = torch.empty_like(o)
    with torch.cuda.device(dev):
        rc = _lib.lib().ced_generate_rays_pinhole(width, height, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]),
                                                  float(K[1, 2]), _farr(c2w, 12), int(bool(opengl)),
                                                  C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()), None, _stream())
    _lib.check(rc, "generate_rays_pinhole")
    return Rays(origins=o, viewdirs=d)


def hypercam_rays(orientation, position, focal_length: float, principal_point: Sequence[float],
                  image_size: Sequence[int], skew: float = 0.0, pixel_aspect_ratio: float = 1.0,
                  radial_distortion: Optional[Sequence[float]] = None,
                  tangential_distortion: Optional[Sequence[float]] = None, device="cuda") -> Rays:
    """Rays through the pixel centres of a HyperNeRF camera (datasets/hyper_cam.py `Camera` fields)."""
    width, height = int(image_size[0]), int(image_size[1])
    dev = torch.device(device)
    if dev.type != "cuda":
        raise NotImplementedError("Only support cuda devices (no CPU fallback).")
    o = torch.empty((height, width, 3), device=dev, dtype=torch.float32)
    d = torch.empty_like(o)
    rad = _farr(radial_distortion, 3) if radial_distortion is not None else None
    tan = _farr(tangential_distortion, 2) if tangential_distortion is not None else None
    with torch.cuda.device(dev):
        rc = _lib.lib().ced_generate_rays_hypercam(width, height, _farr(orientation, 9), _farr(position, 3),
                                                   float(focal_length), float(principal_point[0]),
                                                   float(principal_point[1]), float(skew), float(pixel_aspect_ratio),
                                                   rad, tan, C.c_void_p(o.data_ptr()), C.c_void_p(d.data_ptr()),
                                                   _stream())
    _lib.check(rc, "generate_rays_hypercam")
    return Rays(origins=o, viewdirs=d)


def pinhole_projector(K, c2w, opengl: bool = True, device="cuda"):
    """The inverse of `pinhole_rays`: returns project(points [S,3]) -> (pixels [S,2], in_front [S] bool) for the camera
    K [3,3], c2w [3,4] (or [4,4]).  Pixel units are continuous with the centre of pixel (x, y) AT (x, y): the point
    o + s * d of `pinhole_rays`' ray through pixel (x, y), s > 0, projects to (x, y).  With p_cam = R^-1 (p - o), R and o
    the rotation and translation of c2w:
        opengl=True   the camera looks down -z with y up (`pinhole_rays`' camera direction ((x - cx + 0.5) / fx,
                      -(y - cy + 0.5) / fy, -1)):  x = -fx * p_cam.x / p_cam.z + cx - 0.5,  y = fy * p_cam.y / p_cam.z + cy - 0.5,
                      in_front = p_cam.z < 0;
        opengl=False  OpenCV: down +z with y down (direction ((x - cx + 0.5) / fx, (y - cy + 0.5) / fy, 1)):
                      x = fx * p_cam.x / p_cam.z + cx - 0.5,  y = fy * p_cam.y / p_cam.z + cy - 0.5,  in_front = p_cam.z > 0.
    A point that is not in front still gets the formula's pixel (possibly infinite or NaN); mask with in_front.  Plain
    torch in the points' own device and dtype (the camera is held in float64 and cast), so it runs on CPU tensors too;
    `device` is where the camera's tensors are created first."""
    K = np.asarray(K, np.float64)
    c2w = np.asarray(c2w, np.float64)[:3, :4]
    sign = -1.0 if opengl else 1.0
    cam = {}

    def held(like):
        key = (like.device, like.dtype)
        if key not in cam:
            cam[key] = (torch.as_tensor(np.linalg.inv(c2w[:, :3]), dtype=like.dtype, device=like.device),
                        torch.as_tensor(c2w[:, 3].copy(), dtype=like.dtype, device=like.device))
        return cam[key]

    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    if torch.device(device).type == "cuda" and torch.cuda.is_available():
        held(torch.empty(0, dtype=torch.float32, device=device))

    def project(points: torch.Tensor):
        w2c, origin = held(points)
        pc = ((points - origin)[:, None, :] * w2c[None, :, :]).sum(-1)  # rows p_cam = R^-1 (p - o), without a BLAS call
        z = pc[:, 2]
        pixels = torch.stack([(sign * fx) * (pc[:, 0] / z) + (cx - 0.5), fy * (pc[:, 1] / z) + (cy - 0.5)], dim=-1)
        return pixels, (z * sign) > 0

    return project
