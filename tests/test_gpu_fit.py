"""GPU suite: the training loop (trainer.fit, train_real.py:185-520) -- convergence on a synthetic teacher, the loop's
bookkeeping read from its history, empty batches, the checkpoint round trip, the HyperNeRF preset and the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ced_nerf_amd import cameras, synthetic as S, trainer
from ced_nerf_amd.metrics import evaluate_views
from ced_nerf_amd.model import DNGPradianceField
from ced_nerf_amd.nerfacc_api import OccGridEstimator
from ced_nerf_amd.train import TrainableField, next_num_rays
from ced_nerf_amd.trainset import TrainViews
from ced_nerf_amd.utils import Rays, render_image_test

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _teacher(name, log2_hashmap_size=15):
    sc = S.make_scene(name, 8, 8, "trained", log2_hashmap_size=log2_hashmap_size)
    cfg = sc["cfg"]
    field = DNGPradianceField.from_params(sc["params"], DEV).eval()
    est = OccGridEstimator(cfg["aabb"], cfg["grid_resolution"], cfg["grid_levels"]).to(DEV)
    est.set_binaries(T(sc["binaries"]))
    est.eval()
    return sc, field, est


def _render(field, est, sc, rays, t):
    r = dict(sc["render"])
    r["render_bkgd"] = torch.zeros(3, device=DEV)
    rgb, op, _, _ = render_image_test(1024, field, est, rays, timestamps=torch.full((1, 1), t, device=DEV), **r)
    return rgb, op


def _u8(a):
    return np.clip(np.rint(a * 255.0), 0, 255).astype(np.uint8)


# MS-SSIM's four downsamplings need more than 160 pixels a side (metrics.ms_ssim): held-out views are rendered larger
TEST_SIZE = 176


def dnerf_teacher_views(n_train=24, n_test=4, size=100, test_size=TEST_SIZE):
    """Teacher renders on black as uint8 RGBA (straight rgb = C / opacity, alpha = opacity) at three timestamps."""
    sc, field, est = _teacher("dnerf")
    cfg = sc["cfg"]
    times = [0.0, 0.5, 1.0]
    out = []
    for count, offset, size in ((n_train, 0.0, size), (n_test, 11.0, test_size)):
        focal = 0.5 * size / np.tan(0.5 * cfg["camera_angle_x"])
        K = np.array([[focal, 0, size / 2.0], [0, focal, size / 2.0], [0, 0, 1]], np.float32)
        imgs, c2ws, ts = [], [], []
        for i in range(count):
            c2w = S.look_at_c2w(cfg["radius"], 15.0 + 25.0 * (i % 3), offset + 360.0 * i / count, True)
            t = times[i % 3]
            rgb, op = _render(field, est, sc, cameras.pinhole_rays(K, c2w, size, size, True, device=DEV), t)
            rgb, op = rgb.cpu().numpy(), op.cpu().numpy()
            straight = np.where(op > 0, rgb / np.maximum(op, 1e-12), 0.0)
            imgs.append(np.concatenate([_u8(straight), _u8(op)], axis=-1))
            c2ws.append(c2w)
            ts.append(t)
        out.append((np.stack(imgs), K, np.stack(c2ws), np.array(ts, np.float32)))
    return out


@pytest.fixture(scope="module")
def dnerf_views():
    (tr, K, c2w, ts), (te, Kt, c2wt, tst) = dnerf_teacher_views()
    return TrainViews.pinhole(tr, K, c2w, ts, device=DEV), TrainViews.pinhole(te, Kt, c2wt, tst, device=DEV)


def _init_psnr(test_views, preset, **flags):
    """The held-out PSNR of the model fit starts from: the reference's initialisation with an empty occupancy grid."""
    cfg = trainer.PRESETS[preset]
    est = OccGridEstimator(cfg["aabb"], cfg["grid_resolution"], cfg["grid_levels"]).to(DEV)
    params = S.init_field_params(est.aabbs[-1].cpu().numpy(), cfg["moving_step"], cfg["hash_dst_resolution"], 15,
                                 regime="init", seed=42, table_dtype=np.float16, **flags)
    inf = TrainableField(params, DEV).shared_inference()
    r = dict(near_plane=cfg["near_plane"], far_plane=cfg["far_plane"], render_step_size=cfg["render_step_size"],
             cone_angle=cfg["cone_angle"], alpha_thre=cfg["alpha_thre"])
    return evaluate_views(inf, est, test_views.test_views(bkgd=cfg["test_bkgd"]), **r)["psnr_avg"]


@pytest.fixture(scope="module")
def dnerf_fit(dnerf_views, tmp_path_factory):
    train, test = dnerf_views
    path = str(tmp_path_factory.mktemp("ckpt") / "model.pth")
    res = trainer.fit(train, test, preset="dnerf", max_steps=800, log2_hashmap_size=15,
                      target_sample_batch_size=1 << 16, save_path=path, log_every=100)
    res["save_path"] = path
    return res


# 3 dB under the held-out PSNR measured on an MI355X: 11.98 dB at initialisation, 23.20 dB after the 800 steps
PSNR_FLOOR_DNERF = 20.0


def test_fit_converges_on_a_synthetic_teacher(dnerf_views, dnerf_fit):
    init = _init_psnr(dnerf_views[1], "dnerf")
    final = dnerf_fit["eval"]["psnr_avg"]
    print(f"dnerf fit: init psnr {init:.2f} dB -> {final:.2f} dB after 800 steps, train {dnerf_fit['train_seconds']:.2f} s, "
          f"ssim {dnerf_fit['eval']['ssim_avg']:.4f}")
    assert np.isfinite(final) and final >= init + 10.0, (init, final)
    assert final >= PSNR_FLOOR_DNERF, (init, final)


def test_fit_history_follows_the_reference_loop(dnerf_fit):
    hist = dnerf_fit["history"]
    cfg = dnerf_fit["config"]
    assert [h["step"] for h in hist] == list(range(801))
    # the lr of every step is the hand-built chain's, stepped once per trained step
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=cfg["lr"], eps=1e-15)
    ms = [800 // 2, 800 * 3 // 4, 800 * 9 // 10]
    sched = torch.optim.lr_scheduler.ChainedScheduler([
        torch.optim.lr_scheduler.LinearLR(opt, start_factor=0.01, total_iters=100),
        torch.optim.lr_scheduler.MultiStepLR(opt, milestones=ms, gamma=0.33)])
    for h in hist:
        assert h["lr"] == opt.param_groups[0]["lr"], h
        if not h["skipped"]:
            opt.step()
            sched.step()
    for a, b in zip(hist[:-1], hist[1:]):
        want = a["num_rays"] if a["skipped"] else next_num_rays(a["num_rays"], a["n_samples"], 1 << 16)
        assert b["num_rays"] == want, (a, b)
    assert hist[0]["num_rays"] == 1024
    assert [h["occ_refreshed"] for h in hist] == [h["step"] % 16 == 0 for h in hist]
    assert all(np.isfinite(h["loss"]) for h in hist if not h["skipped"])
    assert all(h["scale"] > 0 for h in hist)


def test_empty_batches_are_skipped(dnerf_views):
    """A single training view that looks away from the box: every batch keeps no sample, so no step changes anything."""
    size = 16
    c2w = S.look_at_c2w(4.0, 20.0, 40.0, True)
    c2w[:, 2] = -c2w[:, 2]                       # OpenGL looks down -z: flip z to face away from the origin
    c2w[:, 0] = -c2w[:, 0]                       # keep a right-handed frame
    K = np.array([[10.0, 0, 8.0], [0, 10.0, 8.0], [0, 0, 1]], np.float32)
    imgs = np.full((1, size, size, 4), 200, np.uint8)
    views = TrainViews.pinhole(imgs, K, c2w[None], [0.5], device=DEV)
    res = trainer.fit(views, None, preset="dnerf", max_steps=2, log2_hashmap_size=15, verbose=False)
    hist = res["history"]
    assert len(hist) == 3 and all(h["skipped"] and h["n_samples"] == 0 for h in hist), hist
    assert all(h["num_rays"] == 1024 and h["lr"] == hist[0]["lr"] for h in hist)
    assert all(h["scale"] == 2.0 ** 10 for h in hist)
    cfg = trainer.PRESETS["dnerf"]
    params = S.init_field_params(np.asarray(cfg["aabb"], np.float32), cfg["moving_step"], cfg["hash_dst_resolution"], 15,
                                 regime="init", seed=42, table_dtype=np.float16)
    f = res["field"]
    assert torch.equal(f.hash_table.detach().cpu(), torch.from_numpy(params["hash"]["table"].astype(np.float32)))
    for got, want in zip(list(f.xyz_wrap) + list(f.mlp_base) + list(f.mlp_head),
                         params["xyz_wrap"] + params["mlp_base"] + params["mlp_head"]):
        assert torch.equal(got.detach().cpu(), torch.from_numpy(want))
    assert res["eval"] is None


def test_checkpoint_round_trip(dnerf_views, dnerf_fit):
    state = torch.load(dnerf_fit["save_path"], map_location=DEV)
    assert set(state) == {"radiance_field", "occupancy_grid"}
    cfg = dnerf_fit["config"]
    field = DNGPradianceField(aabb=dnerf_fit["estimator"].aabbs[-1].clone(), dst_resolution=cfg["hash_dst_resolution"],
                              log2_hashmap_size=15, moving_step=cfg["moving_step"], hash_dtype=torch.float16).to(DEV)
    field.load_state_dict(state["radiance_field"])
    est = OccGridEstimator(cfg["aabb"], cfg["grid_resolution"], cfg["grid_levels"]).to(DEV)
    est.load_state_dict(state["occupancy_grid"])
    field.eval()
    est.eval()
    view = next(iter(dnerf_views[1].test_views()))
    r = dict(near_plane=cfg["near_plane"], far_plane=cfg["far_plane"], render_step_size=cfg["render_step_size"],
             cone_angle=cfg["cone_angle"], alpha_thre=cfg["alpha_thre"], render_bkgd=view["color_bkgd"],
             timestamps=view["timestamps"])
    a = render_image_test(1024, field, est, view["rays"], **r)
    inf = dnerf_fit["inference"].eval()
    b = render_image_test(1024, inf, dnerf_fit["estimator"].eval(), view["rays"], **r)
    assert a[3] == b[3] and a[3] > 0
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)


def test_hypernerf_preset_short_run():
    """run_hyper.sh's flags (-te -ta -df -f -ae -d) on synthetic HyperNeRF-camera views of a teacher, one view per step."""
    sc, field, est = _teacher("hypernerf")
    cfg = sc["cfg"]
    times = [0.0, 0.5, 1.0]

    def views(count, offset, size):
        focal = 0.5 * size / np.tan(0.5 * cfg["camera_angle_x"])
        cams, imgs, ts = [], [], []
        for i in range(count):
            c2w = S.look_at_c2w(cfg["radius"], 20.0 + 15.0 * (i % 2), offset + 360.0 * i / count, False)
            cam = dict(orientation=c2w[:3, :3].T.copy(), position=c2w[:3, 3].copy(), focal_length=float(focal),
                       principal_point=[size / 2.0, size / 2.0], radial_distortion=[0.01, -0.002, 0.0],
                       tangential_distortion=[0.0005, -0.0003])
            rays = cameras.hypercam_rays(image_size=(size, size), device=DEV, **cam)
            rgb, _ = _render(field, est, sc, rays, times[i % 3])
            cams.append(cam)
            imgs.append(_u8(rgb.cpu().numpy()))
            ts.append(times[i % 3])
        return TrainViews.hypercam(np.stack(imgs), cams, ts, device=DEV)

    train, test = views(12, 0.0, 64), views(3, 17.0, TEST_SIZE)
    flags = dict(use_time_embedding=True, use_time_attenuation=True, use_div_offsets=True)
    init = _init_psnr(test, "hypernerf", **flags)
    res = trainer.fit(train, test, preset="hypernerf", max_steps=300, log2_hashmap_size=15,
                      target_sample_batch_size=1 << 15, use_feat_predict=True, acc_entropy_loss=True,
                      distortion_loss=True, log_every=100, **flags)
    losses = [h["loss"] for h in res["history"] if not h["skipped"]]
    print(f"hypernerf fit: init psnr {init:.2f} dB -> {res['eval']['psnr_avg']:.2f} dB, {len(losses)} trained steps")
    assert len(losses) > 250 and all(np.isfinite(losses))
    assert res["eval"]["psnr_avg"] > init + 1.0, (init, res["eval"]["psnr_avg"])


def test_cli_trains_a_dnerf_folder(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    (tr, K, c2w, ts), (te, _, c2wt, tst) = dnerf_teacher_views(n_train=6, n_test=2, size=48)
    scene = tmp_path / "toy"
    angle = 2.0 * np.arctan(0.5 * 48 / K[0, 0])      # the same field of view at either size
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
    out = subprocess.run([sys.executable, "-m", "ced_nerf_amd.trainer", "--data_root", str(tmp_path), "--scene", "toy",
                          "--max_steps", "20", "--log2_hashmap_size", "15", "-df"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert "psnr_avg" in out.stdout and "step=20" in out.stdout, out.stdout
