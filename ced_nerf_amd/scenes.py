"""The reference's scene-folder conventions, restated in numpy: which scene name is which dataset kind, how a
HyperNeRF capture is split and its cameras rescaled, and DyNeRF's pose normalisation and spiral render path.

Nothing here reads a file or touches torch: the two loaders (`TrainViews.from_hypernerf_folder`,
`TrainViews.from_dynerf_folder`) read the folders and call these functions on what they read.  Every function does
the reference's float64 operations in the reference's order, so its outputs can be compared value for value
(tests/golden/dynerf_poses.npz holds the reference's own outputs for two pose sets).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

# Scene-name tables: datasets/dnerf_synthetic.py:64-73, datasets/hypernerf.py:276-294, datasets/dnerf_3d_video_IS.py:205-215
DNERF_SCENES = ("bouncingballs", "hellwarrior", "hook", "jumpingjacks", "lego", "mutant", "standup", "trex")
HYPERNERF_SCENES = ("interp_aleks-teapot", "interp_chickchicken", "interp_cut-lemon", "interp_hand",
                    "interp_slice-banana", "interp_torchocolate", "misc_americano", "misc_cross-hands", "misc_espresso",
                    "misc_keyboard", "misc_oven-mitts", "misc_split-cookie", "misc_tamping", "vrig_3dprinter",
                    "vrig_broom", "vrig_chicken", "vrig_peel-banana")
DYNERF_SCENES = ("coffee_martini", "cook_spinach", "cut_roasted_beef", "flame_salmon_1", "flame_salmon_2",
                 "flame_salmon_3", "flame_salmon_4", "flame_steak", "sear_steak")
HYPERNERF_PREFIXES = ("interp_", "misc_", "vrig_")            # hypernerf.py:295-299


def preset_of(scene: str) -> str:
    """The dataset kind of a scene name, which is also its `trainer.PRESETS` key: "dnerf", "hypernerf" or "dynerf"
    (train_real.py:86,119,151).  ValueError on a name in none of the three tables."""
    for kind, names in (("dnerf", DNERF_SCENES), ("hypernerf", HYPERNERF_SCENES), ("dynerf", DYNERF_SCENES)):
        if scene in names:
            return kind
    raise ValueError(f"scene={scene!r} is in none of the scene tables (D-NeRF {list(DNERF_SCENES)}, HyperNeRF "
                     f"{list(HYPERNERF_SCENES)}, DyNeRF {list(DYNERF_SCENES)})")


def hypernerf_subfolder(scene: str) -> str:
    """The capture's folder below `root/scene`: the scene name without its interp_ / misc_ / vrig_ prefix
    (hypernerf.py:331-347)."""
    for prefix in HYPERNERF_PREFIXES:
        if scene.startswith(prefix):
            return scene[len(prefix):]
    raise ValueError(f"scene={scene!r}: a HyperNeRF scene name starts with one of {list(HYPERNERF_PREFIXES)}")


# ---------------------------------------------------------------------------------------------------------------------
# HyperNeRF
# ---------------------------------------------------------------------------------------------------------------------
def hypernerf_split(ids: Sequence, train_ids: Optional[Sequence] = None,
                    val_ids: Optional[Sequence] = None) -> Tuple[List[int], List[int]]:
    """(train, test) as indices into `ids` (hypernerf.py:104-123).  No `val_ids` (the interp_ / misc_ captures): train
    is every fourth index from 0, test each train index + 2 without the last one.  Otherwise (vrig_): the indices whose
    id is in `train_ids` / `val_ids`, in `ids` order."""
    n = len(ids)
    if not val_ids:
        train = [i for i in range(n) if i % 4 == 0]
        return train, [i + 2 for i in train][:-1]
    train_set, val_set = set(train_ids or ()), set(val_ids)
    return [i for i in range(n) if ids[i] in train_set], [i for i in range(n) if ids[i] in val_set]


def scale_hyper_camera(cam_json: Dict, ratio: float, scene_center, coord_scale: float) -> Dict:
    """A `camera/{id}.json` dict -> the camera `TrainViews.hypercam` / `cameras.hypercam_rays` take, at `ratio` of the
    full resolution and in the normalised scene frame.

    As `Camera.from_json(...).scale(ratio)` (datasets/hyper_cam.py:123-145, 306-323): the json's values become float32;
    focal length and principal point are multiplied by `ratio` in float32; `image_size` (width, height) becomes
    int(round(size * ratio)); orientation, skew, pixel aspect ratio and distortion are kept.  An old file's
    "tangential" key is read as "tangential_distortion".  Then position = (position - scene_center) * coord_scale
    (hypernerf.py:139-143), which the reference evaluates in float64 from the float32 position and rounds to float32
    when it builds the rays."""
    if not ratio > 0:
        raise ValueError(f"ratio must be positive, got {ratio}")
    f32 = np.float32
    tangential = cam_json["tangential"] if "tangential" in cam_json else cam_json["tangential_distortion"]
    position = np.asarray(cam_json["position"], f32).astype(np.float64)
    position = (position - np.asarray(scene_center, np.float64)) * float(coord_scale)
    size = np.asarray(cam_json["image_size"], np.uint32)
    return dict(orientation=np.asarray(cam_json["orientation"], f32).reshape(3, 3),
                position=position.astype(f32),
                focal_length=float(f32(cam_json["focal_length"]) * f32(ratio)),
                principal_point=np.asarray(cam_json["principal_point"], f32) * f32(ratio),
                skew=float(f32(cam_json["skew"])),
                pixel_aspect_ratio=float(f32(cam_json["pixel_aspect_ratio"])),
                radial_distortion=np.asarray(cam_json["radial_distortion"], f32),
                tangential_distortion=np.asarray(tangential, f32),
                image_size=(int(round(float(size[0]) * ratio)), int(round(float(size[1]) * ratio))))


# ---------------------------------------------------------------------------------------------------------------------
# DyNeRF (LLFF poses_bounds.npy)
# ---------------------------------------------------------------------------------------------------------------------
def _unit(v: np.ndarray) -> np.ndarray:
    return v / np.linalg.norm(v)


def average_poses(poses: np.ndarray) -> np.ndarray:
    """[3,4]: the pose `center_poses` centres on (datasets/pose_ulils.py:14-37).  Translation = mean camera centre,
    z = the normalised mean z axis, x = normalised (mean y) x z, y = z x x."""
    center = poses[..., 3].mean(0)
    z = _unit(poses[..., 2].mean(0))
    y_mean = poses[..., 1].mean(0)
    x = _unit(np.cross(y_mean, z))
    y = np.cross(z, x)
    return np.concatenate([np.stack([x, y, z], 1), center[..., None]], 1)


def center_poses(poses: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(poses in the frame of their average pose [N,3,4], that frame's inverse [4,4]) (pose_ulils.py:48-59)."""
    frame = np.eye(4)
    frame[:3] = average_poses(poses)
    bottom = np.tile(np.array([0, 0, 0, 1]), (len(poses), 1, 1))
    homogeneous = np.concatenate([poses, bottom], 1)
    inverse = np.linalg.inv(frame)
    return (inverse @ homogeneous)[:, :3], np.linalg.inv(frame)


def correct_poses_bounds(poses: np.ndarray, bounds: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """`correct_poses_bounds(poses, bounds)` with its defaults, as the DyNeRF loader calls it (pose_ulils.py:230-256).
    poses [N,3,4 or 5] in LLFF's "down, right, back" axes, bounds [N,2].  The axes become "right, up, back" (column 1,
    minus column 0, columns 2:4; a fifth h/w/focal column is dropped), translations and bounds are divided by
    0.75 * min(bounds), and the poses are centred on their average.  Returns (poses [N,3,4], the centring transform
    [4,4], bounds [N,2]); unlike the reference the inputs are left unchanged."""
    poses = np.concatenate([poses[..., 1:2], -poses[..., :1], poses[..., 2:4]], -1)
    scale = bounds.min() * 0.75
    bounds = bounds / scale
    poses[..., :3, 3] /= scale
    poses, transform = center_poses(poses)
    return poses, transform, bounds


def _spiral_average_pose(poses: np.ndarray) -> np.ndarray:
    """datasets/utils.py:35-65, the spiral's own average pose: x = normalised z x (mean y), y = x x z."""
    center = poses[..., 3].mean(0)
    z = _unit(poses[..., 2].mean(0))
    y_mean = poses[..., 1].mean(0)
    x = _unit(np.cross(z, y_mean))
    y = np.cross(x, z)
    return np.stack([x, y, z, center], 1)


def _spiral_view_matrix(z: np.ndarray, up: np.ndarray, position: np.ndarray) -> np.ndarray:
    """datasets/utils.py:23-28: columns (-x, y, z, position) with x = normalised up x z and y = normalised z x x."""
    z = _unit(z)
    x = _unit(np.cross(up, z))
    y = _unit(np.cross(z, x))
    return np.stack([-x, y, z, position], axis=1)


def generate_spiral_path(poses: np.ndarray, bounds: np.ndarray, n_frames: int = 120, n_rots: int = 2,
                         zrate: float = 0.5, dt: float = 0.75, percentile: float = 70) -> np.ndarray:
    """The forward-facing spiral of datasets/utils.py:67-112: float64 poses [N,3,4] and bounds in, [n_frames,3,4] out.
    The path circles the average pose with, per axis, the `percentile` of |camera position| as radius, `n_rots` turns
    over the frames, the depth oscillating at `zrate` of the angle; every pose looks at the point `focal` in front of
    the average pose, focal = 1 / ((1 - dt) / min(bounds) + dt / (5 max(bounds)))."""
    c2w = _spiral_average_pose(poses)
    up = _unit(poses[:, :3, 1].sum(0))
    close_depth, inf_depth = bounds.min() * 1.0, bounds.max() * 5.0
    focal = 1.0 / (((1.0 - dt) / close_depth + dt / inf_depth))
    radii = np.percentile(np.abs(poses[:, :3, 3]), percentile, 0)
    radii = np.concatenate([radii, [1.0]])
    out = []
    for theta in np.linspace(0.0, 2.0 * np.pi * n_rots, n_frames, endpoint=False):
        position = c2w @ (radii * [np.cos(theta), -np.sin(theta), -np.sin(theta * zrate), 1.0])
        look_at = c2w @ np.array([0, 0, -focal, 1.0])
        out.append(_spiral_view_matrix(position - look_at, up, position))
    return np.stack(out, axis=0)


DYNERF_SPIRAL = dict(n_frames=300, n_rots=2, zrate=0.1, dt=0.7, percentile=50)     # dnerf_3d_video_IS.py:119-127
DYNERF_POSE_SCALE = 0.4                                                           # :135-137
DYNERF_POSE_OFFSET = (0.0, 0.0, 1.5)                                              # :139-140


def dynerf_world(poses: np.ndarray) -> np.ndarray:
    """dnerf_3d_video_IS.py:132-140 on poses [N,3,4] (the cameras and the spiral alike): columns 1:3 negated,
    translations x 0.4, then + (0, 0, 1.5).  A copy."""
    out = np.array(poses, np.float64)
    out[:, :, 1:3] *= -1
    out[:, :, 3] *= DYNERF_POSE_SCALE
    out[:, :, 3] += np.array([DYNERF_POSE_OFFSET])
    return out


def dynerf_poses(poses_bounds: np.ndarray, height: int, width: int, factor: int):
    """`poses_bounds.npy` [N,17] -> (camera poses [N,3,4], render poses [300,3,4], focal) in the training frame
    (dnerf_3d_video_IS.py:90-140): the h/w/focal column takes the images' height and width and focal / factor, then
    `correct_poses_bounds`, the 300-frame spiral, and `dynerf_world` on both."""
    arr = np.asarray(poses_bounds, np.float64)
    if arr.ndim != 2 or arr.shape[1] != 17:
        raise ValueError(f"poses_bounds must be [N,17], got {arr.shape}")
    poses = arr[:, :-2].reshape(-1, 3, 5).copy()
    bounds = arr[:, -2:].copy()
    poses[:, 0, 4] = height
    poses[:, 1, 4] = width
    poses[:, 2, 4] = poses[:, 2, 4] * 1.0 / factor
    focal = float(poses[0, 2, 4])
    poses, _, bounds = correct_poses_bounds(poses, bounds)
    spiral = generate_spiral_path(poses, bounds, **DYNERF_SPIRAL)
    return dynerf_world(poses), dynerf_world(spiral), focal


def dynerf_folder_and_frames(scene: str) -> Tuple[str, Optional[Tuple[int, int]]]:
    """(folder name, frame range or None): `flame_salmon_k` is frames [(k - 1) * 300, k * 300) of the folder
    `flame_salmon_1` (dnerf_3d_video_IS.py:82-86, 165-166)."""
    if "flame_salmon" in scene:
        k = int(scene.split("_")[-1]) - 1
        return "flame_salmon_1", (k * 300, (k + 1) * 300)
    return scene, None
