"""The scene-folder conventions (ced_nerf_amd/scenes.py) and the HyperNeRF / DyNeRF loaders of `TrainViews`, without a
GPU and (but for one test) without PIL: toy folders in tmp_path, images through the `read_image` hook, views built on
the cpu device.  The pose functions are compared with the reference's own outputs, recorded by
tests/golden/make_dynerf_poses_golden.py."""
import json
import os

import numpy as np
import pytest
import torch

import scene_toys as toys
from ced_nerf_amd import scenes
from ced_nerf_amd.trainset import CAMERA_HYPERCAM, CAMERA_PINHOLE, TrainViews

W, H = 16, 12


# ---------------------------------------------------------------------------------------------------------------------
# Pose math against the reference's recorded outputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return toys.golden_poses()


# Both sides run the same float64 numpy operations on values of order 1-100.
POSE_TOL = 1e-12


@pytest.mark.parametrize("tag,n", [("fixed5", 5), ("seeded19", 19)])
def test_pose_functions_match_the_reference(golden, tag, n):
    arr = golden[tag + "_poses_bounds"]
    assert arr.shape == (n, 17)
    before = arr.copy()
    poses, transform, bounds = scenes.correct_poses_bounds(arr[:, :15].reshape(-1, 3, 5), arr[:, 15:])
    assert np.array_equal(arr, before)                      # the inputs are left alone
    spiral = scenes.generate_spiral_path(poses, bounds, n_frames=300, n_rots=2, zrate=0.1, dt=0.7, percentile=50)
    assert spiral.shape == (300, 3, 4) and spiral.dtype == np.float64
    for got, key in ((poses, "_poses"), (transform, "_transform"), (bounds, "_bounds"), (spiral, "_spiral")):
        want = golden[tag + key]
        assert got.shape == want.shape
        diff = float(np.abs(got - want).max())
        print(f"{tag}{key}: max|diff| = {diff:.3e}")
        assert diff <= POSE_TOL, (tag, key, diff)


def test_spiral_is_a_rigid_camera_path(golden):
    spiral = scenes.generate_spiral_path(golden["fixed5_poses"], golden["fixed5_bounds"], **scenes.DYNERF_SPIRAL)
    R = spiral[:, :, :3]
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-12
    # the centred poses average to the identity frame at the origin
    avg = scenes.average_poses(golden["fixed5_poses"])
    assert np.abs(avg - np.eye(4)[:3]).max() <= 1e-12


def test_dynerf_poses_chain(golden):
    arr = golden["seeded19_poses_bounds"]
    poses, render, focal = scenes.dynerf_poses(arr, 507, 676, 4)
    assert focal == arr[0, 14] * 1.0 / 4

    def by_hand(p):
        p = p.copy()
        p[:, :, 1:3] *= -1
        p[:, :, 3] *= 0.4
        p[:, :, 3] += np.array([[0, 0, 1.5]])
        return p
    assert np.abs(poses - by_hand(golden["seeded19_poses"])).max() <= POSE_TOL
    assert np.abs(render - by_hand(golden["seeded19_spiral"])).max() <= POSE_TOL
    with pytest.raises(ValueError):
        scenes.dynerf_poses(arr[:, :16], 507, 676, 4)


# ---------------------------------------------------------------------------------------------------------------------
# Tables, split, camera scaling
# ---------------------------------------------------------------------------------------------------------------------
def test_preset_of_routes_every_table():
    assert len(scenes.DNERF_SCENES) == 8 and len(scenes.HYPERNERF_SCENES) == 17 and len(scenes.DYNERF_SCENES) == 9
    for kind, names in (("dnerf", scenes.DNERF_SCENES), ("hypernerf", scenes.HYPERNERF_SCENES),
                        ("dynerf", scenes.DYNERF_SCENES)):
        for name in names:
            assert scenes.preset_of(name) == kind
    from ced_nerf_amd import trainer
    assert {scenes.preset_of(n) for n in ("lego", "vrig_broom", "sear_steak")} <= set(trainer.PRESETS)
    for bad in ("", "chicken", "toy", "flame_salmon", "vrig_"):
        with pytest.raises(ValueError):
            scenes.preset_of(bad)
    assert scenes.hypernerf_subfolder("interp_aleks-teapot") == "aleks-teapot"
    assert scenes.hypernerf_subfolder("vrig_peel-banana") == "peel-banana"
    with pytest.raises(ValueError):
        scenes.hypernerf_subfolder("lego")
    assert scenes.dynerf_folder_and_frames("flame_salmon_3") == ("flame_salmon_1", (600, 900))
    assert scenes.dynerf_folder_and_frames("flame_steak") == ("flame_steak", None)


def test_hypernerf_split_both_branches():
    ids = [f"im{i}" for i in range(9)]
    assert scenes.hypernerf_split(ids, ids, []) == ([0, 4, 8], [2, 6])            # 10 is dropped with the last entry
    assert scenes.hypernerf_split(ids) == ([0, 4, 8], [2, 6])
    assert scenes.hypernerf_split(ids[:8], ids[:8], []) == ([0, 4], [2])
    assert scenes.hypernerf_split(ids[:1], None, None) == ([0], [])
    train_ids, val_ids = ["im7", "im1", "im4"], ["im5", "im0"]
    assert scenes.hypernerf_split(ids, train_ids, val_ids) == ([1, 4, 7], [0, 5])   # in `ids` order


def test_scale_hyper_camera():
    cam = dict(orientation=np.eye(3).tolist(), position=[1.0, 2.0, 3.5], focal_length=40.3,
               principal_point=[15.75, 12.5], skew=0.1, pixel_aspect_ratio=1.01, radial_distortion=[0.1, 0.2, 0.3],
               tangential_distortion=[0.4, 0.5], image_size=[33, 25])
    cam["tangential"] = [0.6, 0.7]                                 # an old file's key wins, as in Camera.from_json
    out = scenes.scale_hyper_camera(cam, 0.5, [0.5, -1.0, 2.0], 0.25)
    f32 = np.float32
    assert out["focal_length"] == float(f32(40.3) * f32(0.5))
    assert np.array_equal(out["principal_point"], np.array([15.75, 12.5], f32) * f32(0.5))
    assert out["image_size"] == (16, 12)                           # round-half-even of 16.5 and 12.5, as int(round())
    want = ((np.array([1.0, 2.0, 3.5], f32).astype(np.float64) - np.array([0.5, -1.0, 2.0])) * 0.25).astype(f32)
    assert out["position"].dtype == f32 and np.array_equal(out["position"], want)
    assert np.array_equal(out["tangential_distortion"], np.array([0.6, 0.7], f32))
    assert np.array_equal(out["radial_distortion"], np.array([0.1, 0.2, 0.3], f32))
    assert out["skew"] == float(f32(0.1)) and out["pixel_aspect_ratio"] == float(f32(1.01))
    with pytest.raises(ValueError):
        scenes.scale_hyper_camera(cam, 0.0, [0, 0, 0], 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# HyperNeRF toy folder
# ---------------------------------------------------------------------------------------------------------------------
def _hand_built_hypercam(toy, picks, factor=2):
    """`TrainViews.hypercam` from the toy's own records, every scaled value worked out here."""
    f32 = np.float32
    sc = toy["scene"]
    cams, images, times = [], [], []
    max_time = max(m["time_id"] for m in toy["metadata"].values())
    for k in picks:
        image_id = toy["ids"][k]
        c = toy["cameras"][image_id]
        pos = (np.asarray(c["position"], f32).astype(np.float64) - np.asarray(sc["center"])) * sc["scale"]
        cams.append(dict(orientation=np.asarray(c["orientation"], f32), position=pos.astype(f32),
                         focal_length=float(f32(c["focal_length"]) * f32(1.0 / factor)),
                         principal_point=np.asarray(c["principal_point"], f32) * f32(1.0 / factor),
                         skew=c["skew"], pixel_aspect_ratio=c["pixel_aspect_ratio"],
                         radial_distortion=c["radial_distortion"], tangential_distortion=c["tangential_distortion"]))
        images.append(toys.image_of(os.path.join(toy["dir"], "rgb", f"{factor}x", image_id + ".png"), W, H))
        times.append(toy["metadata"][image_id]["time_id"] / max_time)
    return TrainViews.hypercam(np.stack(images), cams, times, device="cpu")


@pytest.mark.parametrize("vrig,scene", [(True, "vrig_chicken"), (False, "misc_espresso")])
def test_hypernerf_toy_folder(tmp_path, vrig, scene):
    toy = toys.make_hypernerf_toy(tmp_path, scene, vrig=vrig)
    log = []
    views = {s: TrainViews.from_hypernerf_folder(str(tmp_path), scene, s, device="cpu", read_image=toys.reader(W, H, log))
             for s in ("train", "test")}
    picks = {"train": [0, 2, 4, 6], "test": [1, 3, 5, 7]} if vrig else {"train": [0, 4], "test": [2]}
    assert len(log) == sum(len(v) for v in picks.values())
    assert all(p.startswith(os.path.join(toy["dir"], "rgb", "2x")) and p.endswith(".png") for p in log)
    for split, v in views.items():
        want = _hand_built_hypercam(toy, picks[split])
        assert v.model == CAMERA_HYPERCAM and v.view_mode == "one_per_step"
        assert (v.n_views, v.height, v.width, v.channels) == (len(picks[split]), H, W, 3)
        assert v.cameras.dtype == torch.float32 and torch.equal(v.cameras, want.cameras)      # every bit
        assert torch.equal(v.images, want.images)
        assert torch.equal(v.timestamps, want.timestamps)
        assert v.ids == [toy["ids"][k] for k in picks[split]]
        assert v.camera_ids == [toy["metadata"][i]["camera_id"] for i in v.ids]
        assert v.near == 0.0123 and v.far == 0.457
    # time_id / the largest time_id of ALL ids (10, on the last pair), whichever split they are in
    assert views["train"].timestamps.tolist() == [float(np.float32(t / 10.0)) for t in ((1, 4, 7, 10) if vrig else (1, 7))]
    # the two rigs differ, and the distortion is there
    for v in views.values():
        assert np.all(v.cameras.numpy()[:, 17:22] != 0)
    if vrig:                                                        # left rig against right rig
        assert not np.array_equal(views["train"].cameras[0, 12:].numpy(), views["test"].cameras[0, 12:].numpy())


def test_hypernerf_size_mismatch_names_the_file(tmp_path):
    toy = toys.make_hypernerf_toy(tmp_path, "vrig_chicken")
    with pytest.raises(ValueError, match=r"left_000000\.png"):
        TrainViews.from_hypernerf_folder(str(tmp_path), "vrig_chicken", device="cpu", read_image=toys.reader(W, H + 1))
    with pytest.raises(ValueError, match=r"left_000000\.png"):      # the camera at 1/4 is 8 x 6
        TrainViews.from_hypernerf_folder(str(tmp_path), "vrig_chicken", factor=4, device="cpu", read_image=toys.reader(W, H))
    with pytest.raises(ValueError, match="uint8"):
        TrainViews.from_hypernerf_folder(str(tmp_path), "vrig_chicken", device="cpu",
                                         read_image=lambda p: np.zeros((H, W, 4), np.uint8))
    with pytest.raises(ValueError):
        TrainViews.from_hypernerf_folder(str(tmp_path), "vrig_chicken", split="val", device="cpu", read_image=toys.reader(W, H))
    assert toy["dataset"]["val_ids"]


# ---------------------------------------------------------------------------------------------------------------------
# DyNeRF toy folder
# ---------------------------------------------------------------------------------------------------------------------
def _dynerf_world(p):
    p = np.array(p, np.float64)
    p[:, :, 1:3] *= -1
    p[:, :, 3] *= 0.4
    p[:, :, 3] += np.array([[0, 0, 1.5]])
    return p


def test_dynerf_toy_folder(tmp_path):
    toy = toys.make_dynerf_toy(tmp_path, "coffee_martini")
    log = []
    train = TrainViews.from_dynerf_folder(str(tmp_path), "coffee_martini", "train", device="cpu", read_image=toys.reader(W, H, log))
    rel = lambda v, j: os.path.join(toy["dir"], f"images_x4/cam{v:02d}/{j:04d}.png")
    assert log == [rel(v, j) for v in (1, 2) for j in range(5)]                     # camera-major, video 0 held out
    assert (train.n_views, train.height, train.width, train.channels) == (10, H, W, 3)
    assert (train.n_cameras, train.frames_per_camera) == (2, 5)
    assert train.model == CAMERA_PINHOLE and train.view_mode == "one_per_step" and train.opengl is False
    assert torch.equal(train.images, torch.from_numpy(np.stack([toys.image_of(p, W, H) for p in log])))
    assert train.timestamps.tolist() == [float(np.float32(j / 4)) for _ in range(2) for j in range(5)]
    focal = toy["poses_bounds"][0, 14] / 4
    assert train.focal == focal
    K = np.array([[focal, 0, W / 2.0], [0, focal, H / 2.0], [0, 0, 1]], np.float32)
    assert np.array_equal(train.K, np.broadcast_to(K, (10, 3, 3)))
    assert train.cameras[:, 16].tolist() == [1.0] * 10                              # the OpenCV sign of the camera block
    assert train.weights_subsampled == 1
    assert not hasattr(train, "isg_weights") and not hasattr(train, "ist_weights")
    # poses and render path: the package's chain and, step by step, by hand
    arr = toy["poses_bounds"]
    poses, _, bounds = scenes.correct_poses_bounds(arr[:, :15].reshape(-1, 3, 5), arr[:, 15:])
    spiral = scenes.generate_spiral_path(poses, bounds, n_frames=300, n_rots=2, zrate=0.1, dt=0.7, percentile=50)
    assert train.render_poses.shape == (300, 3, 4) and train.render_poses.dtype == np.float32
    assert np.array_equal(train.render_poses, _dynerf_world(spiral).astype(np.float32))
    assert np.array_equal(train.c2w, np.repeat(_dynerf_world(poses)[1:], 5, axis=0).astype(np.float32))

    log.clear()
    test = TrainViews.from_dynerf_folder(str(tmp_path), "coffee_martini", "test", device="cpu", read_image=toys.reader(W, H, log))
    assert log == [rel(0, 0)]                                                       # every 10th frame of video 0
    assert (test.n_views, test.n_cameras, test.frames_per_camera) == (1, 1, 1)
    assert test.timestamps.tolist() == [0.0]
    assert np.array_equal(test.c2w, _dynerf_world(poses)[:1].astype(np.float32))
    assert np.array_equal(test.render_poses, train.render_poses)

    log.clear()
    every = TrainViews.from_dynerf_folder(str(tmp_path), "coffee_martini", "test", load_every=2, device="cpu",
                                          read_image=toys.reader(W, H, log))
    assert log == [rel(0, j) for j in (0, 2, 4)] and every.timestamps.tolist() == [0.0, 0.5, 1.0]
    sparse = TrainViews.from_dynerf_folder(str(tmp_path), "coffee_martini", "train", load_every=3, device="cpu",
                                           read_image=toys.reader(W, H))
    assert (sparse.n_cameras, sparse.frames_per_camera) == (2, 2)
    assert sparse.timestamps.tolist() == [0.0, 0.75, 0.0, 0.75]
    with pytest.raises(ValueError, match="0000.png"):
        TrainViews.from_dynerf_folder(str(tmp_path), "coffee_martini", device="cpu", read_image=toys.reader(W + 1, H))
    with pytest.raises(NotImplementedError):                                        # rays are made on the GPU
        train.render_path_rays(0)


def test_dynerf_render_path_matches_the_reference_spiral(tmp_path):
    """All five golden cameras: the render path is the reference's recorded spiral -> flip -> x 0.4 -> + 1.5."""
    golden = toys.golden_poses()
    toys.make_dynerf_toy(tmp_path, "sear_steak", n_videos=5, n_frames=2)
    views = TrainViews.from_dynerf_folder(str(tmp_path), "sear_steak", "test", device="cpu", read_image=toys.reader(W, H))
    # float32 rounding of values the restatement gives to POSE_TOL
    for got, want in ((views.render_poses, _dynerf_world(golden["fixed5_spiral"])),
                      (views.c2w, _dynerf_world(golden["fixed5_poses"])[:1])):
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -24 * np.abs(want).max() + POSE_TOL


def test_dynerf_factor_2_subsamples_the_weights(tmp_path):
    toys.make_dynerf_toy(tmp_path, "cook_spinach", factor=2, width=2 * W, height=2 * H)
    views = TrainViews.from_dynerf_folder(str(tmp_path), "cook_spinach", factor=2, device="cpu",
                                          read_image=toys.reader(2 * W, 2 * H))
    assert views.weights_subsampled == 2 and (views.width, views.height) == (2 * W, 2 * H)
    assert views.focal == toys.golden_poses()["fixed5_poses_bounds"][0, 14] / 2


def test_flame_salmon_reads_its_300_frames(tmp_path):
    toy = toys.make_dynerf_toy(tmp_path, "flame_salmon_2", n_videos=2, n_frames=600, width=4, height=3,
                               folder="flame_salmon_1")
    log = []
    views = TrainViews.from_dynerf_folder(str(tmp_path), "flame_salmon_2", device="cpu", read_image=toys.reader(4, 3, log))
    assert len(toy["videos"][1]["images"]) == 600
    assert log == [os.path.join(toy["dir"], f"images_x4/cam01/{j:04d}.png") for j in range(300, 600)]
    assert (views.n_views, views.n_cameras, views.frames_per_camera) == (300, 1, 300)
    # the reference divides the json's idx by the frames read - 1 (dnerf_3d_video_IS.py:168,182)
    assert views.timestamps.tolist() == [float(np.float32(j / 299)) for j in range(300, 600)]


def test_weight_files_load_under_their_own_names(tmp_path):
    toy = toys.make_dynerf_toy(tmp_path, "flame_steak")
    n = 2 * 5 * H * W
    isg = torch.arange(n, dtype=torch.float32) / n
    ist = torch.full((2, 5, H, W), 0.1, dtype=torch.float64)
    torch.save(isg, os.path.join(toy["dir"], "isg_weights.pt"))
    views = TrainViews.from_dynerf_folder(str(tmp_path), "flame_steak", device="cpu", read_image=toys.reader(W, H))
    assert torch.equal(views.isg_weights, isg) and not hasattr(views, "ist_weights")
    torch.save(ist, os.path.join(toy["dir"], "ist_weights.pt"))
    views = TrainViews.from_dynerf_folder(str(tmp_path), "flame_steak", device="cpu", read_image=toys.reader(W, H))
    assert torch.equal(views.isg_weights, isg)
    assert views.ist_weights.dtype == torch.float32 and views.ist_weights.shape == (n,)
    assert torch.equal(views.ist_weights, torch.full((n,), 0.1, dtype=torch.float32))
    assert not torch.equal(views.ist_weights, views.isg_weights)


# ---------------------------------------------------------------------------------------------------------------------
# CLI plumbing that needs no GPU, and the PIL reader
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_refuses_an_unknown_scene(tmp_path):
    from ced_nerf_amd import trainer
    with pytest.raises(ValueError, match="scene tables"):
        trainer.main(["--data_root", str(tmp_path), "--scene", "no_such_scene"])


def test_default_reader_reads_pngs_with_pil(tmp_path):
    pytest.importorskip("PIL.Image")
    toy = toys.make_hypernerf_toy(tmp_path, "vrig_broom", png=True)
    a = TrainViews.from_hypernerf_folder(str(tmp_path), "vrig_broom", device="cpu")
    b = TrainViews.from_hypernerf_folder(str(tmp_path), "vrig_broom", device="cpu", read_image=toys.reader(W, H))
    assert torch.equal(a.images, b.images) and torch.equal(a.cameras, b.cameras)
    dy = toys.make_dynerf_toy(tmp_path, "cut_roasted_beef", png=True)
    c = TrainViews.from_dynerf_folder(str(tmp_path), "cut_roasted_beef", device="cpu")
    d = TrainViews.from_dynerf_folder(str(tmp_path), "cut_roasted_beef", device="cpu", read_image=toys.reader(W, H))
    assert torch.equal(c.images, d.images) and torch.equal(c.timestamps, d.timestamps)
    assert json.load(open(os.path.join(dy["dir"], "images_x4_list.json")))["videos"][0]["images"][0]["weight"] == W
    assert toy["ids"]
