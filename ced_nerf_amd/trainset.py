"""Device-resident training views and the one-launch batch sampler (csrc/train_batch.hip).

The reference turns posed images into training batches in its dataset classes: D-NeRF draws a view per ray and
composites RGBA on the background with about twenty small torch launches (datasets/dnerf_synthetic.py:142-242);
HyperNeRF draws one view per step and undistorts every ray of the batch on the host in numpy before uploading it
(datasets/hypernerf.py:443-541).  `TrainViews.batch` does either in one HIP launch from uint8 images, per-view camera
blocks and timestamps kept on the device, with no host work and no upload per step.

The sampler's random numbers are a pure function of (seed, step, ray, draw); `draws` below restates them in numpy,
bit for bit ("Training batches").
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Dict, Iterator, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .utils import Rays

CAMERA_PINHOLE, CAMERA_HYPERCAM = 0, 1                  # CED_CAMERA_*
PINHOLE_FLOATS, HYPERCAM_FLOATS = 17, 22                # CED_PINHOLE_FLOATS / CED_HYPERCAM_FLOATS
VIEW_MODES = {"per_ray": 0, "one_per_step": 1}          # CED_VIEW_PER_RAY / CED_VIEW_PER_STEP
BKGD_MODES = {"white": 0, "black": 1, "random": 2}      # CED_BKGD_*


# ---------------------------------------------------------------------------------------------------------------------
# The random-number contract of train_batch.hip, restated in numpy (uint32 arithmetic wraps as on the device)
# ---------------------------------------------------------------------------------------------------------------------
def _lowbias32(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def _lo_hi(v):
    v = np.asarray(v, np.uint64)
    return (v & np.uint64(0xFFFFFFFF)).astype(np.uint32), (v >> np.uint64(32)).astype(np.uint32)


def batch_key(seed: int, step: int) -> np.uint32:
    """key = h(h(h(h(seed_lo ^ 0x243f6a88) ^ seed_hi) ^ step_lo) ^ step_hi), h = lowbias32."""
    s_lo, s_hi = _lo_hi(np.uint64(seed % (1 << 64)))
    t_lo, t_hi = _lo_hi(np.uint64(step % (1 << 64)))
    h = _lowbias32(s_lo ^ np.uint32(0x243F6A88))
    h = _lowbias32(h ^ s_hi)
    h = _lowbias32(h ^ t_lo)
    return _lowbias32(h ^ t_hi)


def batch_draw(key, ray, k: int) -> np.ndarray:
    """draw(r, k) = h(h(h(key ^ r_lo) ^ r_hi) ^ (0x9e3779b9 * (k + 1)))."""
    r_lo, r_hi = _lo_hi(ray)
    h = _lowbias32(_lowbias32(np.uint32(key) ^ r_lo) ^ r_hi)
    return _lowbias32(h ^ np.uint32((0x9E3779B9 * (k + 1)) & 0xFFFFFFFF))


def draw_below(u, n: int) -> np.ndarray:
    """An integer in [0, n): (u * n) >> 32."""
    return ((np.asarray(u, np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int32)


def draw_unit(u) -> np.ndarray:
    """A float in [0, 1): (u >> 8) * 2^-24."""
    return ((np.asarray(u, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


_BATCH_RAY = np.uint64(0xFFFFFFFFFFFFFFFF)


def draws(seed: int, step: int, num_rays: int, n_views: int, width: int, height: int, view_mode: str = "per_ray",
          bkgd: str = "white"):
    """What the sampler draws for a batch: (view, x, y) as int32 [n] each, and the background [3] float32."""
    if view_mode not in VIEW_MODES:
        raise ValueError(f"view_mode={view_mode!r}: one of {sorted(VIEW_MODES)}")
    if bkgd not in BKGD_MODES:
        raise ValueError(f"bkgd={bkgd!r}: one of {sorted(BKGD_MODES)}")
    key = batch_key(seed, step)
    rays = np.arange(num_rays, dtype=np.uint64)
    if view_mode == "per_ray":
        view = draw_below(batch_draw(key, rays, 0), n_views)
    else:
        view = np.full(num_rays, draw_below(batch_draw(key, _BATCH_RAY, 0), n_views), np.int32)
    x = draw_below(batch_draw(key, rays, 1), width)
    y = draw_below(batch_draw(key, rays, 2), height)
    if bkgd == "random":
        colour = np.array([draw_unit(batch_draw(key, _BATCH_RAY, 1 + c)) for c in range(3)], np.float32)
    else:
        colour = np.full(3, 1.0 if bkgd == "white" else 0.0, np.float32)
    return view, x, y, colour


def _u8_unit(t: torch.Tensor) -> torch.Tensor:
    """u8 / 255 as the exact float32 quotient (the sampler's).  A tensor divisor: torch's CUDA kernel would multiply by
    the reciprocal of a Python-number divisor, which differs in the last bit for 126 of the 256 values."""
    return t.float() / torch.full((), 255.0, device=t.device)


class TrainViews:
    """Posed uint8 images on one device: images [V,H,W,C] (C = 4 RGBA or 3 RGB), a camera block per view
    ([V,17] pinhole or [V,22] hypercam, include/cednerf_hip.h) and a timestamp per view."""

    def __init__(self, images: torch.Tensor, cameras: torch.Tensor, timestamps: torch.Tensor, model: int,
                 view_mode: str):
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] not in (3, 4):
            raise ValueError(f"images must be uint8 [V,H,W,3 or 4], got {tuple(images.shape)} {images.dtype}")
        n_floats = PINHOLE_FLOATS if model == CAMERA_PINHOLE else HYPERCAM_FLOATS
        if tuple(cameras.shape) != (images.shape[0], n_floats):
            raise ValueError(f"cameras must be [{images.shape[0]},{n_floats}], got {tuple(cameras.shape)}")
        if timestamps.reshape(-1).shape[0] != images.shape[0]:
            raise ValueError(f"{timestamps.numel()} timestamps for {images.shape[0]} views")
        if view_mode not in VIEW_MODES:
            raise ValueError(f"view_mode={view_mode!r}: one of {sorted(VIEW_MODES)}")
        self.images = images.contiguous()
        self.cameras = cameras.to(images.device, torch.float32).contiguous()
        self.timestamps = timestamps.to(images.device, torch.float32).reshape(-1).contiguous()
        self.model = model
        self.view_mode = view_mode
        self.n_views, self.height, self.width, self.channels = (int(v) for v in images.shape)

    def __len__(self) -> int:
        return self.n_views

    @property
    def device(self) -> torch.device:
        return self.images.device

    # -- constructors -------------------------------------------------------------------------------------------------
    @staticmethod
    def _images(images, device) -> torch.Tensor:
        t = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images))
        return t.to(device)

    @classmethod
    def pinhole(cls, images, K, c2w, timestamps, opengl: bool = True, device="cuda",
                view_mode: str = "per_ray") -> "TrainViews":
        """Pinhole views (dnerf_synthetic.py): K [3,3] or [V,3,3], c2w [V,3,4] or [V,4,4]; a ray per pixel (x, y) as
        cameras.pinhole_rays.  By default every ray draws its own view (batch_over_images=True)."""
        imgs = cls._images(images, device)
        V = imgs.shape[0]
        K = np.asarray(K, np.float32)
        K = np.broadcast_to(K, (V, 3, 3)) if K.ndim == 2 else K
        c2w = np.asarray(c2w, np.float32)[:, :3, :4]
        if K.shape != (V, 3, 3) or c2w.shape != (V, 3, 4):
            raise ValueError(f"K {K.shape} / c2w {c2w.shape} do not match {V} views")
        sign = -1.0 if opengl else 1.0
        block = np.concatenate([K[:, 0, 0:1], K[:, 1, 1:2], K[:, 0, 2:3], K[:, 1, 2:3], c2w.reshape(V, 12),
                                np.full((V, 1), sign, np.float32)], axis=1).astype(np.float32)
        ts = torch.as_tensor(np.asarray(timestamps, np.float32).reshape(-1))
        out = cls(imgs, torch.from_numpy(block), ts, CAMERA_PINHOLE, view_mode)
        out.K, out.c2w, out.opengl = np.ascontiguousarray(K), np.ascontiguousarray(c2w), bool(opengl)
        return out

    @classmethod
    def hypercam(cls, images, cameras: Sequence[Dict], timestamps, device="cuda",
                 view_mode: str = "one_per_step") -> "TrainViews":
        """HyperNeRF views (hypernerf.py): one dict per view with the fields `cameras.hypercam_rays` takes
        (orientation, position, focal_length, principal_point, and optionally skew, pixel_aspect_ratio,
        radial_distortion, tangential_distortion); rays at the pixel centres.  By default one view per batch."""
        imgs = cls._images(images, device)
        if len(cameras) != imgs.shape[0]:
            raise ValueError(f"{len(cameras)} cameras for {imgs.shape[0]} views")
        rows = []
        for cam in cameras:
            rad = cam.get("radial_distortion")
            tan = cam.get("tangential_distortion")
            row = np.concatenate([np.asarray(cam["orientation"], np.float32).reshape(9),
                                  np.asarray(cam["position"], np.float32).reshape(3),
                                  [cam["focal_length"]], np.asarray(cam["principal_point"], np.float32).reshape(2),
                                  [cam.get("skew", 0.0), cam.get("pixel_aspect_ratio", 1.0)],
                                  np.zeros(3, np.float32) if rad is None else np.asarray(rad, np.float32).reshape(3),
                                  np.zeros(2, np.float32) if tan is None else np.asarray(tan, np.float32).reshape(2)])
            rows.append(row.astype(np.float32))
        ts = torch.as_tensor(np.asarray(timestamps, np.float32).reshape(-1))
        out = cls(imgs, torch.from_numpy(np.stack(rows)), ts, CAMERA_HYPERCAM, view_mode)
        out.hyper_cameras = [dict(c) for c in cameras]
        return out

    @classmethod
    def from_dnerf_folder(cls, root: str, scene: str, split: str = "train", device="cuda") -> "TrainViews":
        """A D-NeRF synthetic scene folder (dnerf_synthetic.py:16-57): `transforms_{split}.json`, RGBA PNGs, focal
        0.5 W / tan(camera_angle_x / 2), time `frame["time"]` or i / (n - 1), OpenGL cameras."""
        try:
            from PIL import Image
        except ImportError as e:
            raise ImportError("TrainViews.from_dnerf_folder reads PNGs with PIL (Pillow), which is not installed") from e
        data_dir = os.path.join(root, scene)
        with open(os.path.join(data_dir, f"transforms_{split}.json")) as fp:
            meta = json.load(fp)
        frames = meta["frames"]
        images, c2ws, times = [], [], []
        for i, frame in enumerate(frames):
            with Image.open(os.path.join(data_dir, frame["file_path"] + ".png")) as im:
                images.append(np.asarray(im.convert("RGBA"), np.uint8))
            times.append(frame["time"] if "time" in frame else float(i) / (len(frames) - 1))
            c2ws.append(frame["transform_matrix"])
        images = np.stack(images, axis=0)
        h, w = images.shape[1:3]
        focal = 0.5 * w / np.tan(0.5 * float(meta["camera_angle_x"]))
        K = np.array([[focal, 0, w / 2.0], [0, focal, h / 2.0], [0, 0, 1]], np.float32)   # dnerf_synthetic.py:104-111
        out = cls.pinhole(images, K, np.asarray(c2ws, np.float32), np.asarray(times, np.float32), opengl=True,
                          device=device)
        out.focal = float(focal)
        return out

    # -- sampling -----------------------------------------------------------------------------------------------------
    def batch(self, num_rays: int, step: int, bkgd: str = "white", view_mode: Optional[str] = None, seed: int = 0,
              return_indices: bool = False) -> Dict:
        """The reference's training item from one sampler launch: {"rays": Rays [n,3], "pixels" [n,3],
        "timestamps" [n,1], "color_bkgd" [3]} (and "indices" int32 [n,3] = (view, x, y) with return_indices)."""
        num_rays = int(num_rays)
        if num_rays < 1:
            raise ValueError(f"num_rays must be >= 1, got {num_rays}")
        if bkgd not in BKGD_MODES:
            raise ValueError(f"bkgd={bkgd!r}: one of {sorted(BKGD_MODES)}")
        mode = self.view_mode if view_mode is None else view_mode
        if mode not in VIEW_MODES:
            raise ValueError(f"view_mode={mode!r}: one of {sorted(VIEW_MODES)}")
        dev = self.device
        if dev.type != "cuda":
            raise NotImplementedError("TrainViews.batch samples on the GPU: the views must be on a cuda device")
        f = dict(device=dev, dtype=torch.float32)
        o = torch.empty((num_rays, 3), **f)
        d = torch.empty((num_rays, 3), **f)
        px = torch.empty((num_rays, 3), **f)
        ts = torch.empty((num_rays, 1), **f)
        bk = torch.empty((3,), **f)
        idx = torch.empty((num_rays, 3), device=dev, dtype=torch.int32) if return_indices else None
        P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        with torch.cuda.device(dev):
            rc = _lib.lib().ced_sample_training_batch(
                self.model, self.n_views, self.width, self.height, self.channels, P(self.images), P(self.cameras),
                P(self.timestamps), num_rays, int(seed) % (1 << 64), int(step), VIEW_MODES[mode], BKGD_MODES[bkgd],
                P(o), P(d), P(px), P(ts), P(bk), P(idx), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, "sample_training_batch")
        out = {"rays": Rays(origins=o, viewdirs=d), "pixels": px, "timestamps": ts, "color_bkgd": bk}
        if return_indices:
            out["indices"] = idx
        return out

    # -- full frames --------------------------------------------------------------------------------------------------
    def view_rays(self, i: int) -> Rays:
        """Rays [H,W,3] of view i from the full-frame kernels (cameras.pinhole_rays / hypercam_rays)."""
        from . import cameras
        if self.model == CAMERA_PINHOLE:
            return cameras.pinhole_rays(self.K[i], self.c2w[i], self.width, self.height, opengl=self.opengl,
                                        device=self.device)
        cam = self.hyper_cameras[i]
        return cameras.hypercam_rays(cam["orientation"], cam["position"], cam["focal_length"], cam["principal_point"],
                                     (self.width, self.height), skew=cam.get("skew", 0.0),
                                     pixel_aspect_ratio=cam.get("pixel_aspect_ratio", 1.0),
                                     radial_distortion=cam.get("radial_distortion"),
                                     tangential_distortion=cam.get("tangential_distortion"), device=self.device)

    def test_views(self, bkgd: str = "white") -> Iterator[Dict]:
        """Full-frame items in the shape `metrics.evaluate_views` takes: {"rays" [H,W,3], "pixels" [H,W,3],
        "timestamps" [1,1], "color_bkgd" [3]}.  RGBA views are composited on `bkgd` (the reference's evaluation uses
        white, dnerf_synthetic.py:154-156); "random" is not an evaluation background."""
        if bkgd not in ("white", "black"):
            raise ValueError(f"test bkgd={bkgd!r}: 'white' or 'black'")
        colour = torch.full((3,), 1.0 if bkgd == "white" else 0.0, device=self.device)
        for i in range(self.n_views):
            img = self.images[i]
            if self.channels == 4:
                rgb, a = _u8_unit(img[..., :3]), _u8_unit(img[..., 3:])
                pixels = rgb * a + colour * (1.0 - a)
            else:
                pixels = _u8_unit(img)
            yield {"rays": self.view_rays(i), "pixels": pixels, "timestamps": self.timestamps[i].reshape(1, 1),
                   "color_bkgd": colour}
