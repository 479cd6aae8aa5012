"""Toy HyperNeRF and DyNeRF scene folders for tests/test_scenes_cpu.py and tests/test_gpu_scenes.py: the json / npy
files of the two layouts written into a temporary directory, and images that are a function of their path (handed to
the loaders through `read_image`, or written as PNGs where a test asks for PIL)."""
import json
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def image_of(path, width, height):
    """uint8 [height,width,3] noise seeded by the file's place below the scene folder."""
    key = "/".join(str(path).replace("\\", "/").split("/")[-2:])
    return np.random.default_rng(zlib.crc32(key.encode())).integers(0, 256, (height, width, 3), dtype=np.uint8)


def reader(width, height, log=None):
    def read(path):
        if log is not None:
            log.append(path)
        return image_of(path, width, height)
    return read


def _write_png(path, img):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(img).save(path)


def _look_at_rows(position, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """World-to-camera rotation (rows = the camera's x, y, z axes in the world; z looks at the target, y down)."""
    z = np.asarray(target, np.float64) - position
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z])


# ---------------------------------------------------------------------------------------------------------------------
# HyperNeRF
# ---------------------------------------------------------------------------------------------------------------------
def make_hypernerf_toy(root, scene="vrig_chicken", n_ids=8, width=16, height=12, factor=2, vrig=True, png=False):
    """Writes root/scene/<name>/{scene,metadata,dataset}.json and camera/{id}.json (and rgb/{factor}x/{id}.png with
    png=True).  Two rigs ("left", "right") with different intrinsics and distortion alternate over the ids; vrig=True
    trains on the left ids and validates on the right ones, vrig=False leaves val_ids empty (the every-fourth split).
    Returns what was written: {"dir", "ids", "cameras" (json dicts by id), "metadata", "scene"}."""
    name = scene.split("_", 1)[1]
    data_dir = os.path.join(str(root), scene, name)
    os.makedirs(os.path.join(data_dir, "camera"), exist_ok=True)
    scene_json = {"near": 0.0123, "far": 0.457, "scale": 0.25, "center": [0.5, -1.25, 2.0]}
    ids = [("left" if i % 2 == 0 else "right") + f"_{i // 2:06d}" for i in range(n_ids)]
    full_w, full_h = width * factor, height * factor
    rigs = {"left": dict(focal_length=1.3 * full_w, principal_point=[full_w / 2.0 + 0.75, full_h / 2.0 - 1.5], skew=0.0,
                         pixel_aspect_ratio=1.0, radial_distortion=[0.031, -0.012, 0.002],
                         tangential_distortion=[0.0011, -0.0007]),
            "right": dict(focal_length=1.1 * full_w + 0.3, principal_point=[full_w / 2.0 - 1.25, full_h / 2.0 + 0.5],
                          skew=0.1, pixel_aspect_ratio=1.01, radial_distortion=[-0.02, 0.005, -0.001],
                          tangential_distortion=[-0.0004, 0.0009])}
    cameras, metadata = {}, {}
    for i, image_id in enumerate(ids):
        rig = image_id.split("_")[0]
        angle = 0.5 * i + (0.2 if rig == "right" else 0.0)
        unit = np.array([np.cos(angle), np.sin(angle), 0.45 + 0.05 * i])                 # in the normalised frame
        unit *= 1.6 / np.linalg.norm(unit)
        position = np.asarray(scene_json["center"]) + unit / scene_json["scale"]
        cam = dict(rigs[rig], orientation=_look_at_rows(unit).tolist(), position=position.tolist(),
                   image_size=[full_w, full_h])
        cameras[image_id] = cam
        metadata[image_id] = {"camera_id": 0 if rig == "left" else 1, "time_id": 3 * (i // 2) + 1, "warp_id": i // 2,
                              "appearance_id": i // 2}
        with open(os.path.join(data_dir, "camera", image_id + ".json"), "w") as fp:
            json.dump(cam, fp)
        if png:
            path = os.path.join(data_dir, "rgb", f"{factor}x", image_id + ".png")
            _write_png(path, image_of(path, width, height))
    dataset = {"count": n_ids, "num_exemplars": n_ids, "ids": ids,
               "train_ids": [i for i in ids if i.startswith("left")] if vrig else ids,
               "val_ids": [i for i in ids if i.startswith("right")] if vrig else []}
    for fname, obj in (("scene", scene_json), ("metadata", metadata), ("dataset", dataset)):
        with open(os.path.join(data_dir, fname + ".json"), "w") as fp:
            json.dump(obj, fp)
    return dict(dir=data_dir, ids=ids, cameras=cameras, metadata=metadata, scene=scene_json, dataset=dataset)


# ---------------------------------------------------------------------------------------------------------------------
# DyNeRF
# ---------------------------------------------------------------------------------------------------------------------
def golden_poses():
    return np.load(os.path.join(GOLDEN, "dynerf_poses.npz"))


def make_dynerf_toy(root, scene="coffee_martini", n_videos=3, n_frames=5, width=16, height=12, factor=4, png=False,
                    folder=None):
    """Writes root/<folder>/poses_bounds.npy (the first n_videos rows of the golden five-camera array) and
    images_x{factor}_list.json (and the PNGs with png=True).  Returns {"dir", "poses_bounds", "videos"}."""
    data_dir = os.path.join(str(root), folder or scene)
    os.makedirs(data_dir, exist_ok=True)
    poses_bounds = golden_poses()["fixed5_poses_bounds"][:n_videos].copy()
    np.save(os.path.join(data_dir, "poses_bounds.npy"), poses_bounds)
    videos = []
    for v in range(n_videos):
        images = []
        for j in range(n_frames):
            rel = f"images_x{factor}/cam{v:02d}/{j:04d}.png"
            images.append({"path": rel, "idx": j, "height": height, "weight": width})
            if png:
                path = os.path.join(data_dir, rel)
                _write_png(path, image_of(path, width, height))
        videos.append({"video_name": f"cam{v:02d}", "images": images})
    with open(os.path.join(data_dir, f"images_x{factor}_list.json"), "w") as fp:
        json.dump({"scene": scene, "videos": videos}, fp)
    return dict(dir=data_dir, poses_bounds=poses_bounds, videos=videos)
