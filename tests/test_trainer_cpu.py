"""CPU suite: the training loop's presets, schedule, the sampler's random-number contract and the D-NeRF folder reader
(ced_nerf_amd.trainer / ced_nerf_amd.trainset; nothing here launches a kernel)."""
import json

import numpy as np
import pytest
import torch

from ced_nerf_amd import trainer, trainset


def test_presets_are_train_real_constants():
    """train_real.py:85-182, literally."""
    P = trainer.PRESETS
    d = P["dnerf"]
    assert (d["max_steps"], d["init_batch_size"], d["target_sample_batch_size"], d["lr"], d["weight_decay"]) == \
        (20000, 1024, 1 << 18, 1e-2, 0.0)
    assert d["aabb"] == [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5] and (d["near_plane"], d["far_plane"]) == (0.0, 1.0e10)
    assert (d["moving_step"], d["hash_dst_resolution"], d["grid_resolution"], d["grid_levels"]) == (0.0001, 1024, 128, 1)
    assert (d["render_step_size"], d["alpha_thre"], d["cone_angle"]) == (5e-3, 0.0, 0.0)
    assert trainer.milestone_steps(d["milestones"], 20000) == [20000 // 2, 20000 * 3 // 4, 20000 * 9 // 10]
    assert (d["train_bkgd"], d["test_bkgd"], d["view_mode"], d["log2_hashmap_size"]) == ("white", "white", "per_ray", 21)
    h = P["hypernerf"]
    assert (h["max_steps"], h["init_batch_size"], h["target_sample_batch_size"], h["lr"]) == (20000, 1024, 1 << 18, 1e-2)
    assert h["aabb"] == [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0] and h["near_plane"] == 0.2
    assert (h["moving_step"], h["hash_dst_resolution"], h["grid_resolution"], h["grid_levels"]) == (1 / 4096, 4096, 128, 2)
    assert (h["render_step_size"], h["alpha_thre"], h["cone_angle"]) == (1e-3, 1e-2, 0.004)
    assert trainer.milestone_steps(h["milestones"], 20000) == [10000, 15000, 18000]
    assert (h["train_bkgd"], h["test_bkgd"], h["view_mode"]) == ("black", "black", "one_per_step")
    y = P["dynerf"]
    assert (y["max_steps"], y["init_batch_size"], y["target_sample_batch_size"], y["lr"]) == (40000, 1024, 1 << 20, 1e-2)
    assert y["aabb"] == [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0] and y["near_plane"] == 0.2
    assert (y["moving_step"], y["hash_dst_resolution"], y["grid_resolution"], y["grid_levels"]) == \
        (1 / (2048 * 4), 2048 * 4, 128, 4)
    assert (y["render_step_size"], y["alpha_thre"], y["cone_angle"]) == (1e-3, 1e-2, 0.004)
    assert trainer.milestone_steps(y["milestones"], 40000) == [40000 // 2, 40000 * 3 // 4, 40000 * 5 // 6,
                                                               40000 * 9 // 10]
    assert (y["train_bkgd"], y["test_bkgd"]) == ("random", "black")


@pytest.mark.parametrize("max_steps", [20000, 600])
def test_scheduler_factory_matches_a_hand_built_chain(max_steps):
    def lrs(sched_of):
        p = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.Adam([p], lr=1e-2, eps=1e-15)
        sched = sched_of(opt)
        out = []
        for _ in range(max_steps + 2):
            out.append(opt.param_groups[0]["lr"])
            opt.step()
            sched.step()
        return out

    ms = [max_steps // 2, max_steps * 3 // 4, max_steps * 9 // 10]
    want = lrs(lambda o: torch.optim.lr_scheduler.ChainedScheduler([
        torch.optim.lr_scheduler.LinearLR(o, start_factor=0.01, total_iters=100),
        torch.optim.lr_scheduler.MultiStepLR(o, milestones=ms, gamma=0.33)]))
    got = lrs(lambda o: trainer.make_scheduler(o, max_steps, trainer.PRESETS["dnerf"]["milestones"]))
    for s in [0, 1, 99, 100, 101] + [m + k for m in ms for k in (-1, 0, 1)]:
        assert got[s] == want[s], (s, got[s], want[s])
    assert got[0] == pytest.approx(1e-4) and got[100] == pytest.approx(1e-2)


def test_rng_restatement_is_deterministic_and_keyed_on_seed_and_step():
    a = trainset.draws(42, 7, 4096, 5, 37, 29, "per_ray", "random")
    b = trainset.draws(42, 7, 4096, 5, 37, 29, "per_ray", "random")
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    for other in (trainset.draws(42, 8, 4096, 5, 37, 29, "per_ray", "random"),
                  trainset.draws(43, 7, 4096, 5, 37, 29, "per_ray", "random")):
        assert not np.array_equal(a[0], other[0]) and not np.array_equal(a[1], other[1])
        assert not np.array_equal(a[3], other[3])
    view, x, y, bk = a
    assert view.dtype == np.int32 and 0 <= view.min() and view.max() < 5
    assert 0 <= x.min() and x.max() < 37 and 0 <= y.min() and y.max() < 29
    assert bk.dtype == np.float32 and ((bk >= 0) & (bk < 1)).all()
    one = trainset.draws(42, 7, 100, 5, 37, 29, "one_per_step", "white")
    assert (one[0] == one[0][0]).all() and np.array_equal(one[3], np.ones(3, np.float32))
    assert np.array_equal(one[1], x[:100]) and np.array_equal(one[2], y[:100])      # x, y do not depend on the mode
    # the integer and float maps of the contract
    assert trainset.draw_below(np.uint32(0xFFFFFFFF), 37) == 36 and trainset.draw_below(np.uint32(0), 37) == 0
    assert trainset.draw_unit(np.uint32(0xFFFFFFFF)) == np.float32(1 - 2.0 ** -24)
    # the numpy statement against plain Python integers (arbitrary precision, masked to 32 bits)
    def h(x):
        x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF; x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)
    seed, step = (1 << 40) + 12345, (1 << 33) + 7
    k = h(h(h(h((seed & 0xFFFFFFFF) ^ 0x243F6A88) ^ (seed >> 32)) ^ (step & 0xFFFFFFFF)) ^ (step >> 32))
    assert int(trainset.batch_key(seed, step)) == k
    for ray, kk in ((0, 0), (4095, 2), ((1 << 64) - 1, 3)):
        u = h(h(h(k ^ (ray & 0xFFFFFFFF)) ^ (ray >> 32)) ^ ((0x9E3779B9 * (kk + 1)) & 0xFFFFFFFF))
        assert int(trainset.batch_draw(k, np.uint64(ray), kk)) == u
        assert int(trainset.draw_below(np.uint32(u), 29)) == (u * 29) >> 32


def test_from_dnerf_folder_round_trip(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(0)
    scene = tmp_path / "toy"
    (scene / "train").mkdir(parents=True)
    frames, imgs = [], []
    for i in range(3):
        img = rng.integers(0, 256, size=(6, 8, 4), dtype=np.uint8)
        Image.fromarray(img, "RGBA").save(scene / "train" / f"r_{i}.png")
        c2w = np.eye(4)
        c2w[:3, 3] = [i, 2.0 * i, -1.0]
        frames.append({"file_path": f"./train/r_{i}", "transform_matrix": c2w.tolist()})
        imgs.append(img)
    (scene / "transforms_train.json").write_text(json.dumps({"camera_angle_x": 0.7, "frames": frames}))
    v = trainset.TrainViews.from_dnerf_folder(str(tmp_path), "toy", "train", device="cpu")
    assert np.array_equal(v.images.numpy(), np.stack(imgs))
    assert (v.n_views, v.height, v.width, v.channels) == (3, 6, 8, 4)
    assert np.array_equal(v.timestamps.numpy(), np.array([0.0, 0.5, 1.0], np.float32))
    focal = 0.5 * 8 / np.tan(0.5 * 0.7)
    assert v.focal == pytest.approx(focal)
    assert np.array_equal(v.c2w[:, :3, 3], np.array([[0, 0, -1], [1, 2, -1], [2, 4, -1]], np.float32))
    block = v.cameras.numpy()
    assert np.array_equal(block[:, :4], np.tile(np.float32([focal, focal, 4.0, 3.0]), (3, 1)))
    assert np.array_equal(block[:, 4:16], v.c2w.reshape(3, 12)) and (block[:, 16] == -1.0).all()


def test_bad_arguments_raise_value_error():
    with pytest.raises(ValueError):
        trainer.resolve_config("lego")
    with pytest.raises(ValueError):
        trainer.resolve_config("dnerf", train_bkgd="grey")
    with pytest.raises(ValueError):
        trainer.resolve_config("dnerf", no_such_setting=1)
    with pytest.raises(ValueError):
        trainset.draws(0, 0, 8, 1, 4, 4, "per_ray", "grey")
    imgs = np.zeros((2, 4, 4, 2), np.uint8)
    with pytest.raises(ValueError):
        trainset.TrainViews.pinhole(imgs, np.eye(3), np.tile(np.eye(4), (2, 1, 1)), [0.0, 1.0], device="cpu")
    v = trainset.TrainViews.pinhole(np.zeros((2, 4, 4, 4), np.uint8), np.eye(3), np.tile(np.eye(4), (2, 1, 1)),
                                    [0.0, 1.0], device="cpu")
    with pytest.raises(ValueError):
        v.batch(0, 0)
    with pytest.raises(ValueError):
        v.batch(16, 0, bkgd="grey")
    with pytest.raises(ValueError):
        v.batch(16, 0, view_mode="per_pixel")
