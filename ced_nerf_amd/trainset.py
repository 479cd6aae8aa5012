"""Device-resident training views and the one-launch batch sampler (csrc/train_batch.hip).

The reference turns posed images into training batches in its dataset classes: D-NeRF draws a view per ray and
composites RGBA on the background with about twenty small torch launches (datasets/dnerf_synthetic.py:142-242);
HyperNeRF draws one view per step and undistorts every ray of the batch on the host in numpy before uploading it
(datasets/hypernerf.py:443-541).  `TrainViews.batch` does either in one HIP launch from uint8 images, per-view camera
blocks and timestamps kept on the device, with no host work and no upload per step.

The sampler's random numbers are a pure function of (seed, step, ray, draw); `draws` below restates them in numpy,
bit for bit ("Training batches").  `TrainViews.batch_importance` is DyNeRF's importance-sampled batch
(datasets/dnerf_3d_video_IS.py:401-440) on the same draws, restated by `importance_draws`.

Views come from arrays (`TrainViews.pinhole`, `TrainViews.hypercam`) or from the reference's scene folders
(`from_dnerf_folder`, `from_hypernerf_folder`, `from_dynerf_folder`; the conventions are `scenes.py`'s).
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Callable, Dict, Iterator, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, scenes
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


# ---------------------------------------------------------------------------------------------------------------------
# The importance sampler of train_batch.hip (ced_sample_importance_batch), restated in numpy
# ---------------------------------------------------------------------------------------------------------------------
def det_logf_np(x) -> np.ndarray:
    """ced_common.hpp's det_logf on positive normal float32 values, operation for operation in float32."""
    f32 = np.float32
    x = np.ascontiguousarray(x, f32)
    b = x.view(np.uint32)
    k = (b >> np.uint32(23)).astype(np.int32) - np.int32(127)
    m = ((b & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)).view(f32)
    big = m > f32(1.41421353816986083984375)
    m = np.where(big, m * f32(0.5), m).astype(f32)
    k = np.where(big, k + np.int32(1), k).astype(np.int32)
    f = m - f32(1.0)
    z = f * f
    p = np.full_like(f, f32(7.0376836292e-2))
    for c in (-1.1514610310e-1, 1.1676998740e-1, -1.2420140846e-1, 1.4249322787e-1, -1.6668057665e-1, 2.0000714765e-1,
              -2.4999993993e-1, 3.3333331174e-1):
        p = p * f + f32(c)
    kf = k.astype(f32)
    y = (p * f) * z
    y = y + kf * f32(-2.12194440e-4)
    y = y + z * f32(-0.5)
    r = f + y
    r = r + kf * f32(0.693359375)
    assert r.dtype == f32
    return r


def draw_exponential(u) -> np.ndarray:
    """The Exp(1) variate of a 32-bit draw: unit = ((u >> 9) * 2 + 1) * 2^-24 in (0, 1), e = -det_logf(unit)."""
    odd = (np.asarray(u, np.uint32) >> np.uint32(9)) * np.uint32(2) + np.uint32(1)
    unit = odd.astype(np.float32) * np.float32(2.0 ** -24)
    return -det_logf_np(unit)


def importance_candidates(seed: int, step: int, weights, pool_size: int = 2_000_000):
    """The sampler's candidates for a step: (cell [M] int64, key [M] uint32 bit patterns of weight / Exp(1) variate)."""
    w = np.ascontiguousarray(weights, np.float32).reshape(-1)
    n = w.shape[0]
    if n < 1 or n >= 1 << 31:
        raise ValueError(f"the weight map must have 1 .. 2^31 - 1 cells, got {n}")
    if pool_size < 1 or pool_size >= 1 << 31:
        raise ValueError(f"pool_size must be in 1 .. 2^31 - 1, got {pool_size}")
    key = batch_key(seed, step)
    if n <= pool_size:
        j = np.arange(n, dtype=np.uint64)
        cell = j.astype(np.int64)
    else:
        j = np.arange(pool_size, dtype=np.uint64)
        cell = draw_below(batch_draw(key, j, 3), n).astype(np.int64)
    e = draw_exponential(batch_draw(key, j, 4))
    wc = w[cell]
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        q = (wc / e).astype(np.float32)
    bits = np.where((wc > 0) & np.isfinite(wc), q.view(np.uint32), np.uint32(0)).astype(np.uint32)
    return cell, bits


def select_largest(bits, k: int) -> np.ndarray:
    """The sampler's selection: the candidates j of the k largest key patterns, equal keys to the lower j, in ascending
    j.  ValueError when fewer than k patterns are positive."""
    bits = np.asarray(bits, np.uint32)
    order = np.argsort(-bits.astype(np.int64), kind="stable")[:k]
    if order.shape[0] < k or bits[order[-1]] == 0:
        raise ValueError(f"fewer than {k} candidates with a positive weight")
    return np.sort(order)


def importance_draws(seed: int, step: int, num_rays: int, weights, s: int, pool_size: int, width: int, height: int):
    """What `TrainViews.batch_importance` draws: (view, x, y) as int32 [k * s * s] each, k = num_rays // s^2.  `weights`
    is the flat map of V * (height // s) * (width // s) cells."""
    s = int(s)
    if s < 1 or s > min(width, height):
        raise ValueError(f"weights_subsampled must be in 1 .. {min(width, height)}, got {s}")
    k = int(num_rays) // (s * s)
    if k < 1:
        raise ValueError(f"num_rays={num_rays} gives no cell at weights_subsampled={s}")
    hsub, wsub = height // s, width // s
    w = np.ascontiguousarray(weights, np.float32).reshape(-1)
    if w.shape[0] % (hsub * wsub):
        raise ValueError(f"{w.shape[0]} weights are not whole views of {hsub} x {wsub} cells")
    cell, bits = importance_candidates(seed, step, w, pool_size)
    chosen = cell[select_largest(bits, k)]
    view = chosen // (hsub * wsub)
    ysub = (chosen % (hsub * wsub)) // wsub
    xsub = (chosen % (hsub * wsub)) % wsub
    xs, ys = [], []
    for ah in range(s):
        for aw in range(s):
            xs.append(xsub * s + aw)
            ys.append(ysub * s + ah)
    return (np.tile(view, s * s).astype(np.int32), np.concatenate(xs).astype(np.int32),
            np.concatenate(ys).astype(np.int32))


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

    @staticmethod
    def _image_reader(read_image: Optional[Callable[[str], np.ndarray]], who: str) -> Callable[[str], np.ndarray]:
        """The `read_image` hook of the folder loaders: path -> uint8 [H,W,3].  None reads with PIL."""
        if read_image is not None:
            return read_image
        try:
            from PIL import Image
        except ImportError as e:
            raise ImportError(f"TrainViews.{who} reads PNGs with PIL (Pillow), which is not installed") from e

        def read(path: str) -> np.ndarray:
            with Image.open(path) as im:
                return np.asarray(im.convert("RGB"), np.uint8)
        return read

    @staticmethod
    def _read_rgb(read: Callable[[str], np.ndarray], path: str) -> np.ndarray:
        img = np.asarray(read(path))
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[-1] != 3:
            raise ValueError(f"{path}: expected a uint8 [H,W,3] image, got {img.shape} {img.dtype}")
        return img

    @classmethod
    def from_hypernerf_folder(cls, root: str, scene: str, split: str = "train", factor: int = 2, device="cuda",
                              read_image: Optional[Callable[[str], np.ndarray]] = None) -> "TrainViews":
        """A HyperNeRF capture (hypernerf.py:84-156, 184-268, 331-352) in `root/scene/<scene without its interp_ /
        misc_ / vrig_ prefix>`: `scene.json` (near, far, scale, center), `metadata.json` (camera_id, time_id per image
        id), `dataset.json` (ids, train_ids, val_ids), `camera/{id}.json` and `rgb/{factor}x/{id}.png`.  The split is
        `scenes.hypernerf_split`, every camera `scenes.scale_hyper_camera(json, 1 / factor, center, scale)`, a view's
        time its time_id / the largest time_id of all ids; one view per step.  ValueError naming the file when an
        image's size is not its scaled camera's (the reference's assertion, hypernerf.py:393-394).

        `read_image` (the reference's `read_image` switch as a hook): a callable path -> uint8 [H,W,3] used instead of
        PIL.  Attributes besides `TrainViews.hypercam`'s: `near`, `far`, `ids` (of the split) and `camera_ids`."""
        if split not in ("train", "test"):
            raise ValueError(f"split={split!r}: 'train' or 'test'")
        read = cls._image_reader(read_image, "from_hypernerf_folder")
        data_dir = os.path.join(root, scene, scenes.hypernerf_subfolder(scene))
        loaded = {}
        for name in ("scene", "metadata", "dataset"):
            with open(os.path.join(data_dir, name + ".json")) as fp:
                loaded[name] = json.load(fp)
        scene_json, meta, dataset = loaded["scene"], loaded["metadata"], loaded["dataset"]
        ids = list(dataset["ids"])
        train, test = scenes.hypernerf_split(ids, dataset.get("train_ids"), dataset.get("val_ids"))
        max_time = max(meta[i]["time_id"] for i in ids)
        images, cams, times, kept = [], [], [], []
        for k in (train if split == "train" else test):
            name = ids[k]
            with open(os.path.join(data_dir, "camera", f"{name}.json")) as fp:
                cam = scenes.scale_hyper_camera(json.load(fp), 1.0 / factor, scene_json["center"], scene_json["scale"])
            path = os.path.join(data_dir, "rgb", f"{int(factor)}x", f"{name}.png")
            img = cls._read_rgb(read, path)
            if (img.shape[1], img.shape[0]) != tuple(cam["image_size"]):
                raise ValueError(f"{path}: the image is {img.shape[1]} x {img.shape[0]}, its camera at 1/{factor} "
                                 f"{cam['image_size'][0]} x {cam['image_size'][1]}")
            if images and img.shape != images[0].shape:
                raise ValueError(f"{path}: the image is {img.shape[1]} x {img.shape[0]}, the views before it "
                                 f"{images[0].shape[1]} x {images[0].shape[0]}")
            images.append(img)
            cams.append(cam)
            times.append(meta[name]["time_id"] / max_time)
            kept.append(name)
        if not images:
            raise ValueError(f"{data_dir}: the {split} split is empty")
        out = cls.hypercam(np.stack(images, axis=0), cams, np.asarray(times, np.float32), device=device,
                           view_mode="one_per_step")
        out.near, out.far = float(scene_json["near"]), float(scene_json["far"])
        out.ids = kept
        out.camera_ids = [meta[name]["camera_id"] for name in kept]
        return out

    @classmethod
    def from_dynerf_folder(cls, root: str, scene: str, split: str = "train", factor: int = 4,
                           load_every: Optional[int] = None, device="cuda",
                           read_image: Optional[Callable[[str], np.ndarray]] = None) -> "TrainViews":
        """A DyNeRF (Plenoptic Video) scene folder `root/scene` (dnerf_3d_video_IS.py:78-198, 245-306):
        `poses_bounds.npy` and `images_x{factor}_list.json`, whose "videos" each list "images" with "path" (below the
        folder), "idx", "height" and the width under the reference's key "weight".  Poses: `scenes.dynerf_poses` (the
        h/w/focal column from the json and focal / factor, `correct_poses_bounds`, the 300-frame spiral, axes flipped,
        x 0.4, + (0, 0, 1.5)).  train = videos [1:] with every frame, test = video [0] with every 10th; `load_every`
        overrides both strides.  A frame's time is its idx / (frames of its video - 1).  `flame_salmon_k` reads frames
        [(k - 1) * 300, k * 300) of the folder `flame_salmon_1`, with the idx the json gives them.  OpenCV pinhole
        cameras K = [[f, 0, W/2], [0, f, H/2], [0, 0, 1]], one view per step, views camera-major (all frames of a
        camera, then the next camera), which is what `importance.isg_weights(views, n_cameras)` assumes.

        Attributes besides `TrainViews.pinhole`'s: `n_cameras`, `frames_per_camera` (views loaded per camera), `focal`,
        `render_poses` (float32 [300,3,4], see `render_path_rays`), `weights_subsampled` = int(4 / factor) (the weight
        files are made at factor 4), and `isg_weights` / `ist_weights` (flat float32 tensors on `device`) when
        `isg_weights.pt` / `ist_weights.pt` lie in the folder.  The reference loads isg_weights.pt under both names
        (dnerf_3d_video_IS.py:270-271); here each file is loaded under its own name."""
        if split not in ("train", "test"):
            raise ValueError(f"split={split!r}: 'train' or 'test'")
        stride = int(load_every) if load_every is not None else (1 if split == "train" else 10)
        if stride < 1:
            raise ValueError(f"load_every must be >= 1, got {load_every}")
        read = cls._image_reader(read_image, "from_dynerf_folder")
        folder, frame_range = scenes.dynerf_folder_and_frames(scene)
        data_dir = os.path.join(root, folder)
        poses_bounds = np.load(os.path.join(data_dir, "poses_bounds.npy"))
        list_path = os.path.join(data_dir, f"images_x{int(factor)}_list.json")
        with open(list_path) as fp:
            videos = json.load(fp)["videos"]
        if len(videos) != poses_bounds.shape[0]:
            raise ValueError(f"{list_path}: {len(videos)} videos for {poses_bounds.shape[0]} poses")
        first = videos[0]["images"][0]
        height, width = int(first["height"]), int(first["weight"])
        poses, render_poses, focal = scenes.dynerf_poses(poses_bounds, height, width, factor)
        cameras = list(range(1, len(videos))) if split == "train" else [0]
        if not cameras:
            raise ValueError(f"{list_path}: the {split} split has no video")
        images, c2ws, times, per_camera = None, [], [], None
        for cam in cameras:
            frames = videos[cam]["images"]
            if frame_range is not None:
                frames = frames[frame_range[0]:frame_range[1]]
            chosen = frames[::stride]
            if per_camera is None:
                per_camera = len(chosen)
                images = np.empty((len(cameras) * per_camera, height, width, 3), np.uint8)
            if len(chosen) != per_camera or per_camera == 0:
                raise ValueError(f"{list_path}: video {cam} gives {len(chosen)} frames, the first one {per_camera}")
            for frame in chosen:
                path = os.path.join(data_dir, frame["path"])
                img = cls._read_rgb(read, path)
                if img.shape[:2] != (height, width):
                    raise ValueError(f"{path}: the image is {img.shape[1]} x {img.shape[0]}, the list says "
                                     f"{width} x {height}")
                images[len(times)] = img
                times.append(frame["idx"] / max(len(frames) - 1, 1))
                c2ws.append(poses[cam])
        K = np.array([[focal, 0, width / 2.0], [0, focal, height / 2.0], [0, 0, 1]], np.float32)
        out = cls.pinhole(images, K, np.asarray(c2ws, np.float32), np.asarray(times, np.float32), opengl=False,
                          device=device, view_mode="one_per_step")
        out.focal = float(focal)
        out.n_cameras, out.frames_per_camera = len(cameras), per_camera
        out.render_poses = render_poses.astype(np.float32)
        out.weights_subsampled = int(4 / factor)
        for name in ("isg_weights", "ist_weights"):
            path = os.path.join(data_dir, name + ".pt")
            if os.path.exists(path):
                w = torch.load(path, map_location="cpu", weights_only=True)
                setattr(out, name, w.to(device=out.device, dtype=torch.float32).reshape(-1).contiguous())
        return out

    def render_path_rays(self, i: int) -> Tuple[Rays, torch.Tensor]:
        """Frame i of the render path of a DyNeRF scene (dnerf_3d_video_IS.py:328-371): (Rays [H,W,3] of
        `render_poses[i]` through `cameras.pinhole_rays`, timestamps [1,1] = i / number of poses)."""
        from . import cameras
        poses = getattr(self, "render_poses", None)
        if poses is None:
            raise ValueError("these views have no render path (TrainViews.from_dynerf_folder sets render_poses)")
        rays = cameras.pinhole_rays(self.K[0], poses[i], self.width, self.height, opengl=self.opengl, device=self.device)
        return rays, torch.full((1, 1), float(i) / len(poses), device=self.device, dtype=torch.float32)

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

    def batch_importance(self, num_rays: int, step: int, weights: torch.Tensor, weights_subsampled: int = 1,
                         bkgd: str = "random", seed: int = 0, pool_size: int = 2_000_000,
                         return_indices: bool = False) -> Dict:
        """The reference's importance-sampled item (dnerf_3d_video_IS.py:401-440): k = num_rays // s^2 cells of the
        weight map drawn without replacement as torch.multinomial draws them, each expanded to its s x s pixels
        (s = weights_subsampled); the dict of `batch` with k * s^2 rays.  `weights`: float32 device tensor of
        V * (H // s) * (W // s) non-negative entries, cell (view * (H // s) + ysub) * (W // s) + xsub.  More cells than
        `pool_size`: the draw is made among pool_size cells drawn uniformly with replacement first.  A pure function
        of (seed, step), restated by `importance_draws`.  Reads one word back from the device to raise ValueError
        when fewer than k candidates have a positive weight."""
        num_rays, s, pool_size = int(num_rays), int(weights_subsampled), int(pool_size)
        if bkgd not in BKGD_MODES:
            raise ValueError(f"bkgd={bkgd!r}: one of {sorted(BKGD_MODES)}")
        if self.channels != 3:
            raise ValueError("batch_importance samples RGB views; these are RGBA")
        if s < 1 or s > min(self.width, self.height):
            raise ValueError(f"weights_subsampled must be in 1 .. {min(self.width, self.height)}, got {s}")
        k = num_rays // (s * s)
        if k < 1:
            raise ValueError(f"num_rays={num_rays} gives no cell at weights_subsampled={s}")
        n_cells = self.n_views * (self.height // s) * (self.width // s)
        if n_cells >= 1 << 31:
            raise ValueError(f"{n_cells} cells: the sampler indexes below 2^31")
        if not 1 <= pool_size < 1 << 31:
            raise ValueError(f"pool_size must be in 1 .. 2^31 - 1, got {pool_size}")
        if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or weights.numel() != n_cells:
            raise ValueError(f"weights must be a float32 tensor of {n_cells} cells "
                             f"({self.n_views} x {self.height // s} x {self.width // s})")
        if k > min(n_cells, pool_size):
            raise ValueError(f"cannot draw {k} cells without replacement from {min(n_cells, pool_size)} candidates")
        dev = self.device
        if dev.type != "cuda":
            raise NotImplementedError("TrainViews.batch_importance samples on the GPU: the views must be on a cuda device")
        if weights.device != dev:
            raise ValueError(f"weights are on {weights.device}, the views on {dev}")
        weights = weights.contiguous()
        n = k * s * s
        f = dict(device=dev, dtype=torch.float32)
        o = torch.empty((n, 3), **f)
        d = torch.empty((n, 3), **f)
        px = torch.empty((n, 3), **f)
        ts = torch.empty((n, 1), **f)
        bk = torch.empty((3,), **f)
        idx = torch.empty((n, 3), device=dev, dtype=torch.int32) if return_indices else None
        L = _lib.lib()
        ws_bytes = int(L.ced_importance_batch_workspace_bytes(n_cells, pool_size, k))
        if ws_bytes < 0:
            raise ValueError(L.ced_last_error_string().decode())
        ws = torch.empty((ws_bytes // 4,), device=dev, dtype=torch.int32)
        min_key = torch.empty((1,), device=dev, dtype=torch.int32)
        P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        with torch.cuda.device(dev):
            rc = L.ced_sample_importance_batch(
                self.model, self.n_views, self.width, self.height, self.channels, P(self.images), P(self.cameras),
                P(self.timestamps), P(weights), s, pool_size, k, int(seed) % (1 << 64), int(step), BKGD_MODES[bkgd],
                P(o), P(d), P(px), P(ts), P(bk), P(idx), P(min_key), P(ws), ws_bytes,
                C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, "sample_importance_batch")
        if int(min_key.item()) == 0:               # the smallest selected key: 0 = not a positive weight
            raise ValueError(f"fewer than {k} candidates with a positive weight (step {step})")
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
