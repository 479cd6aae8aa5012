"""trainer.fit and the CLI with --refine_poses / --refine_times: the refinement trains, is returned and saved; without the
flags the result and the two-key checkpoint are as before."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ced_nerf_amd import trainer
from ced_nerf_amd.trainset import TrainViews
from test_gpu_fit import DEV, ROOT, dnerf_teacher_views

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def toy_views():
    return dnerf_teacher_views(n_train=6, n_test=2, size=48)


def test_fit_trains_returns_and_saves_the_refinement(toy_views, tmp_path):
    (tr, K, c2w, ts), _ = toy_views
    views = TrainViews.pinhole(tr, K, c2w, ts, device=DEV)
    kw = dict(preset="dnerf", max_steps=20, log2_hashmap_size=15, verbose=False)
    path = str(tmp_path / "refined.pth")
    res = trainer.fit(views, None, refine_poses=True, refine_times=True, refine_lr=1e-3, save_path=path, **kw)
    state = res["refinement"]
    assert sorted(state) == ["dt", "rot", "trans"]
    assert state["rot"].shape == (6, 3) and state["trans"].shape == (6, 3) and state["dt"].shape == (6,)
    assert all(torch.isfinite(v).all() and float(v.abs().max()) > 0 for v in state.values())     # every one was trained
    assert all(np.isfinite(h["loss"]) for h in res["history"] if not h["skipped"])
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(ckpt) == ["camera_refinement", "occupancy_grid", "radiance_field"]
    assert all(torch.equal(ckpt["camera_refinement"][k].cpu(), state[k].cpu()) for k in state)
    only_times = trainer.fit(views, None, refine_times=True, **kw)["refinement"]
    assert sorted(only_times) == ["dt"]
    path = str(tmp_path / "plain.pth")
    plain = trainer.fit(views, None, save_path=path, **kw)
    assert plain["refinement"] is None
    assert sorted(torch.load(path, map_location="cpu", weights_only=True)) == ["occupancy_grid", "radiance_field"]


def test_cli_refines_poses_and_times(toy_views, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    (tr, K, c2w, ts), (te, _, c2wt, tst) = toy_views
    scene = tmp_path / "toy"
    angle = 2.0 * np.arctan(0.5 * 48 / K[0, 0])
    for split, imgs, poses, times in (("train", tr, c2w, ts), ("test", te, c2wt, tst)):
        (scene / split).mkdir(parents=True)
        frames = []
        for i in range(len(imgs)):
            Image.fromarray(imgs[i], "RGBA").save(scene / split / f"r_{i:03d}.png")
            m = np.eye(4)
            m[:3] = poses[i]
            frames.append({"file_path": f"./{split}/r_{i:03d}", "time": float(times[i]), "transform_matrix": m.tolist()})
        (scene / f"transforms_{split}.json").write_text(json.dumps({"camera_angle_x": float(angle), "frames": frames}))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    path = tmp_path / "model.pth"
    out = subprocess.run([sys.executable, "-m", "ced_nerf_amd.trainer", "--data_root", str(tmp_path), "--scene", "toy",
                          "--max_steps", "20", "--log2_hashmap_size", "15", "--refine_poses", "--refine_times",
                          "--refine_lr", "5e-4", "--save_path", str(path)],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert "psnr_avg" in out.stdout and "step=20" in out.stdout, out.stdout
    ckpt = torch.load(str(path), map_location="cpu", weights_only=True)
    assert sorted(ckpt["camera_refinement"]) == ["dt", "rot", "trans"] and ckpt["camera_refinement"]["rot"].shape == (6, 3)
