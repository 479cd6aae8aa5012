"""GPU suite: HyperNeRF and DyNeRF scene folders on the device -- the loaded views through the batch sampler, the
importance kernels and the ray generators, and `trainer.main` end to end (train, save, render the path, reload).  The
folders are the toys of tests/scene_toys.py; no real capture is involved, so nothing here asserts a PSNR."""
import os

import numpy as np
import pytest
import torch

import scene_toys as toys
from ced_nerf_amd import cameras, importance, scenes, trainer
from ced_nerf_amd.trainset import TrainViews, importance_draws

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H = 16, 12


def _equal_batches(a, b):
    assert set(a) == set(b)
    for key in a:
        if key == "rays":
            assert torch.equal(a[key].origins, b[key].origins) and torch.equal(a[key].viewdirs, b[key].viewdirs)
        else:
            assert torch.equal(a[key], b[key]), key


# ---------------------------------------------------------------------------------------------------------------------
# HyperNeRF toy on the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hyper(tmp_path_factory):
    root = tmp_path_factory.mktemp("hyper")
    toy = toys.make_hypernerf_toy(root, "vrig_chicken")
    loaded = TrainViews.from_hypernerf_folder(str(root), "vrig_chicken", "train", device=DEV, read_image=toys.reader(W, H))
    return toy, loaded


def _scaled(toy, image_id):
    return scenes.scale_hyper_camera(toy["cameras"][image_id], 0.5, toy["scene"]["center"], toy["scene"]["scale"])


def test_hypernerf_views_sample_like_hand_built_ones(hyper):
    toy, loaded = hyper
    picks = [0, 2, 4, 6]
    ids = [toy["ids"][k] for k in picks]
    cams = []
    for image_id in ids:
        c = _scaled(toy, image_id)
        c.pop("image_size")
        cams.append(c)
    images = np.stack([toys.image_of(os.path.join(toy["dir"], "rgb", "2x", i + ".png"), W, H) for i in ids])
    by_hand = TrainViews.hypercam(images, cams, [toy["metadata"][i]["time_id"] / 10.0 for i in ids], device=DEV)
    assert loaded.images.device.type == "cuda" and torch.equal(loaded.cameras, by_hand.cameras)
    views_drawn = set()
    for step in (0, 1, 7, 12):
        a = loaded.batch(256, step, bkgd="black", view_mode="one_per_step", return_indices=True)
        b = by_hand.batch(256, step, bkgd="black", view_mode="one_per_step", return_indices=True)
        _equal_batches(a, b)
        assert a["pixels"].shape == (256, 3) and torch.isfinite(a["rays"].viewdirs).all()
        views_drawn.add(int(a["indices"][0, 0]))
    assert len(views_drawn) > 1


def test_hypernerf_view_rays_are_the_scaled_cameras(hyper):
    toy, loaded = hyper
    c = _scaled(toy, toy["ids"][0])
    want = cameras.hypercam_rays(c["orientation"], c["position"], c["focal_length"], c["principal_point"], (W, H),
                                 skew=c["skew"], pixel_aspect_ratio=c["pixel_aspect_ratio"],
                                 radial_distortion=c["radial_distortion"],
                                 tangential_distortion=c["tangential_distortion"], device=DEV)
    got = loaded.view_rays(0)
    assert got.origins.shape == (H, W, 3)
    assert torch.equal(got.origins, want.origins) and torch.equal(got.viewdirs, want.viewdirs)
    # the camera sits 1.6 from the origin of the normalised frame and looks at it
    assert abs(float(got.origins[0, 0].norm()) - 1.6) < 1e-5
    centre = got.viewdirs[H // 2, W // 2]
    assert float((centre * -got.origins[0, 0] / 1.6).sum()) > 0.99


# ---------------------------------------------------------------------------------------------------------------------
# DyNeRF toy on the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dynerf(tmp_path_factory):
    root = tmp_path_factory.mktemp("dynerf")
    toy = toys.make_dynerf_toy(root, "coffee_martini")
    loaded = TrainViews.from_dynerf_folder(str(root), "coffee_martini", "train", device=DEV, read_image=toys.reader(W, H))
    return toy, loaded


def test_dynerf_weights_and_importance_batches(dynerf):
    toy, loaded = dynerf
    clip = np.stack([toys.image_of(os.path.join(toy["dir"], f"images_x4/cam{v:02d}/{j:04d}.png"), W, H)
                     for v in (1, 2) for j in range(5)])
    isg = importance.isg_weights(loaded, loaded.n_cameras)
    assert isg.shape == (2, 5, H, W)
    assert torch.equal(isg.cpu(), torch.from_numpy(importance.isg_weights_reference(clip, 2)))
    out = loaded.batch_importance(512, 3, isg.reshape(-1), loaded.weights_subsampled, seed=5, return_indices=True)
    view, x, y = importance_draws(5, 3, 512, isg.cpu().numpy(), 1, 2_000_000, W, H)
    idx = out["indices"].cpu().numpy()
    assert np.array_equal(idx[:, 0], view) and np.array_equal(idx[:, 1], x) and np.array_equal(idx[:, 2], y)
    # the pixels and times are those of the views the folder gave, camera-major
    want_px = torch.from_numpy(clip)[view, y, x].float() / torch.full((), 255.0)
    assert torch.equal(out["pixels"].cpu(), want_px)
    assert torch.equal(out["timestamps"].cpu().reshape(-1), torch.from_numpy((view % 5).astype(np.float32) / np.float32(4)))


def test_dynerf_render_path_rays(dynerf):
    _, loaded = dynerf
    rays, ts = loaded.render_path_rays(7)
    want = cameras.pinhole_rays(loaded.K[0], loaded.render_poses[7], W, H, opengl=False, device=DEV)
    assert rays.origins.shape == (H, W, 3)
    assert torch.equal(rays.origins, want.origins) and torch.equal(rays.viewdirs, want.viewdirs)
    assert ts.shape == (1, 1) and ts.device.type == "cuda" and float(ts) == float(np.float32(7 / 300))
    first = loaded.view_rays(0)                   # camera 1's pose: the loaded c2w, not the render path's
    own = cameras.pinhole_rays(loaded.K[0], loaded.c2w[0], W, H, opengl=False, device=DEV)
    assert torch.equal(first.viewdirs, own.viewdirs)


# ---------------------------------------------------------------------------------------------------------------------
# trainer.main end to end, once per dataset kind
# ---------------------------------------------------------------------------------------------------------------------
# Held-out views are scored with MS-SSIM, whose four downsamplings need more than 160 pixels a side.
EW, EH = 176, 164


def _end_to_end(tmp_path, monkeypatch, scene, extra):
    """Train 20 steps from the folder, save, render the first frames of the path; then reload the checkpoint and render
    them again.  Returns (history of the training run, first run's PNG bytes, second run's PNG bytes)."""
    pytest.importorskip("PIL.Image")
    runs = []
    real_fit = trainer.fit

    def recording_fit(*args, **kwargs):
        runs.append(real_fit(*args, **kwargs))
        return runs[-1]
    monkeypatch.setattr(trainer, "fit", recording_fit)
    ckpt = str(tmp_path / "model.pth")
    common = ["--data_root", str(tmp_path / "data"), "--scene", scene, "--log2_hashmap_size", "12", "--video_frames", "3"]
    assert trainer.main(common + ["--max_steps", "20", "--save_path", ckpt, "--render_video", str(tmp_path / "a")] + extra) == 0
    assert len(runs) == 1 and os.path.exists(ckpt)
    assert trainer.main(common + ["--load_model", ckpt, "--render_video", str(tmp_path / "b")] + extra) == 0
    assert len(runs) == 1                                        # --load_model trains nothing
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == [f"depth_{i:04d}.png" for i in range(3)] + [f"rgb_{i:04d}.png" for i in range(3)]
    assert sorted(os.listdir(tmp_path / "b")) == names
    read = lambda d: [open(tmp_path / d / n, "rb").read() for n in names]
    return runs[0], names, read("a"), read("b")


def _check_history(res):
    hist = res["history"]
    assert [h["step"] for h in hist] == list(range(21))
    trained = [h for h in hist if not h["skipped"]]
    assert trained and all(np.isfinite(h["loss"]) for h in trained)
    assert res["eval"] is not None and np.isfinite(res["eval"]["psnr_avg"])


def _frame_sizes(tmp_path, names):
    from PIL import Image
    return {n: (Image.open(tmp_path / "a" / n).size, Image.open(tmp_path / "a" / n).mode) for n in names}


def test_cli_hypernerf_end_to_end(tmp_path, monkeypatch):
    pytest.importorskip("PIL.Image")
    toys.make_hypernerf_toy(tmp_path / "data", "vrig_chicken", width=EW, height=EH, png=True)
    res, names, first, second = _end_to_end(tmp_path, monkeypatch, "vrig_chicken", ["-te", "-ta", "-df", "-f", "-ae", "-d"])
    _check_history(res)
    assert res["config"]["view_mode"] == "one_per_step" and res["config"]["train_bkgd"] == "black"
    assert first == second                                       # byte for byte
    sizes = _frame_sizes(tmp_path, names)
    assert all(sizes[n] == ((EW, EH), "RGB" if n.startswith("rgb") else "L") for n in names)


def test_cli_dynerf_end_to_end(tmp_path, monkeypatch, capsys):
    pytest.importorskip("PIL.Image")
    toys.make_dynerf_toy(tmp_path / "data", "coffee_martini", width=EW, height=EH, png=True)
    res, names, first, second = _end_to_end(tmp_path, monkeypatch, "coffee_martini", ["--ist_from_step", "10"])
    _check_history(res)
    assert [h["sampling"] for h in res["history"]] == ["isg"] * 10 + ["ist"] * 11
    assert "ISG sampling weights: computed on the device" in capsys.readouterr().out
    assert first == second
    sizes = _frame_sizes(tmp_path, names)
    assert all(sizes[n] == ((EW, EH), "RGB" if n.startswith("rgb") else "L") for n in names)
