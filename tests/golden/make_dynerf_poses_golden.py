"""Generates tests/golden/dynerf_poses.npz by IMPORTING the reference's pose functions (run where the reference is
checked out: `python tests/golden/make_dynerf_poses_golden.py REFERENCE_DIR`; needs scipy, which
datasets/pose_ulils.py imports).

Only data leaves this script: two `poses_bounds` arrays and, for each, what the reference's `correct_poses_bounds`
(datasets/pose_ulils.py) and `generate_spiral_path` (datasets/utils.py) return for them with the arguments the DyNeRF
loader passes (datasets/dnerf_3d_video_IS.py:107-127).
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _look_at(position, target, up=(0.0, 1.0, 0.0)):
    """A camera at `position` facing `target`, in LLFF's "down, right, back" column order."""
    back = position - target
    back = back / np.linalg.norm(back)
    right = np.cross(np.asarray(up, np.float64), back)
    right = right / np.linalg.norm(right)
    true_up = np.cross(back, right)
    return np.stack([-true_up, right, back, position], axis=1)


def poses_bounds_fixed():
    """Five cameras in a shallow arc, written out by hand."""
    positions = np.array([[-2.0, 0.1, 0.3], [-1.0, -0.2, 0.1], [0.0, 0.0, 0.0], [1.1, 0.25, 0.15], [2.2, -0.1, 0.4]])
    target = np.array([0.1, 0.0, -6.0])
    bounds = np.array([[3.0, 40.0], [2.5, 55.0], [2.8, 48.0], [3.3, 61.0], [2.6, 37.5]])
    return _pack(np.stack([_look_at(p, target) for p in positions]), 2028.0, 2704.0, 1462.0, bounds)


def poses_bounds_seeded(n=19, seed=20240607):
    rng = np.random.default_rng(seed)
    positions = rng.uniform(-1.0, 1.0, (n, 3)) * np.array([12.0, 6.0, 2.0])
    targets = np.array([0.0, 0.0, -40.0]) + rng.normal(0.0, 1.5, (n, 3))
    ups = np.array([0.0, 1.0, 0.0]) + rng.normal(0.0, 0.05, (n, 3))
    near = rng.uniform(8.0, 15.0, n)
    bounds = np.stack([near, near + rng.uniform(40.0, 90.0, n)], axis=1)
    return _pack(np.stack([_look_at(p, t, u) for p, t, u in zip(positions, targets, ups)]), 2028.0, 2704.0, 1458.7, bounds)


def _pack(c2w, h, w, focal, bounds):
    hwf = np.tile(np.array([h, w, focal])[None, :, None], (len(c2w), 1, 1))
    return np.concatenate([np.concatenate([c2w, hwf], axis=2).reshape(len(c2w), 15), bounds], axis=1)


def main():
    if len(sys.argv) != 2:
        sys.exit("usage: make_dynerf_poses_golden.py REFERENCE_DIR")
    ref = sys.argv[1]
    pu = _load("ref_pose_ulils", os.path.join(ref, "datasets", "pose_ulils.py"))
    du = _load("ref_datasets_utils", os.path.join(ref, "datasets", "utils.py"))
    out = {}
    for tag, arr in (("fixed5", poses_bounds_fixed()), ("seeded19", poses_bounds_seeded())):
        out[tag + "_poses_bounds"] = arr.copy()
        poses = arr[:, :15].reshape(-1, 3, 5).copy()
        bounds = arr[:, 15:].copy()                  # the reference divides its `bounds` argument in place
        centred, transform, scaled = pu.correct_poses_bounds(poses, bounds)
        spiral = du.generate_spiral_path(centred[:, :3, :4], scaled, n_frames=300, n_rots=2, zrate=0.1, dt=0.7, percentile=50)
        out[tag + "_poses"], out[tag + "_transform"], out[tag + "_bounds"] = centred, transform, scaled
        out[tag + "_spiral"] = spiral
        assert centred.dtype == np.float64 and spiral.dtype == np.float64 and spiral.shape == (300, 3, 4)
    np.savez(os.path.join(HERE, "dynerf_poses.npz"), **out)
    print("wrote dynerf_poses.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    sys.exit(main())
