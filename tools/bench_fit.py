"""Train-seconds and held-out PSNR / MS-SSIM of trainer.fit on a synthetic D-NeRF teacher, printed as one JSON line.

The teacher is synthetic.make_scene("dnerf", regime="trained") with its sphere occupancy; its renders on black are
stored as uint8 RGBA (straight rgb = C / opacity, alpha = opacity): TRAIN views for training and TEST held-out views
at other azimuths, at three timestamps.  The figures are this code base's, on a synthetic scene: they are not
comparable to the PSNRs the reference publishes for real captures.

    python tools/bench_fit.py [--size 400] [--steps 20000] [--train 24] [--test 4] [--log2_hashmap_size 21]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ced_nerf_amd import cameras, synthetic as S, trainer  # noqa: E402
from ced_nerf_amd.model import DNGPradianceField  # noqa: E402
from ced_nerf_amd.nerfacc_api import OccGridEstimator  # noqa: E402
from ced_nerf_amd.trainset import TrainViews  # noqa: E402
from ced_nerf_amd.utils import render_image_test  # noqa: E402

DEV = "cuda:0"


def teacher_views(count, size, azim_offset, log2_hashmap_size):
    sc = S.make_scene("dnerf", 8, 8, "trained", log2_hashmap_size=log2_hashmap_size)
    cfg = sc["cfg"]
    field = DNGPradianceField.from_params(sc["params"], DEV).eval()
    est = OccGridEstimator(cfg["aabb"], cfg["grid_resolution"], cfg["grid_levels"]).to(DEV)
    est.set_binaries(torch.from_numpy(sc["binaries"]).to(DEV))
    est.eval()
    focal = 0.5 * size / np.tan(0.5 * cfg["camera_angle_x"])
    K = np.array([[focal, 0, size / 2.0], [0, focal, size / 2.0], [0, 0, 1]], np.float32)
    render = dict(sc["render"], render_bkgd=torch.zeros(3, device=DEV))
    imgs, c2ws, ts = [], [], []
    for i in range(count):
        c2w = S.look_at_c2w(cfg["radius"], 15.0 + 25.0 * (i % 3), azim_offset + 360.0 * i / count, True)
        t = [0.0, 0.5, 1.0][i % 3]
        rgb, op, _, _ = render_image_test(1024, field, est, cameras.pinhole_rays(K, c2w, size, size, True, device=DEV),
                                          timestamps=torch.full((1, 1), t, device=DEV), **render)
        rgb, op = rgb.cpu().numpy(), op.cpu().numpy()
        straight = np.where(op > 0, rgb / np.maximum(op, 1e-12), 0.0)
        u8 = lambda a: np.clip(np.rint(a * 255.0), 0, 255).astype(np.uint8)
        imgs.append(np.concatenate([u8(straight), u8(op)], axis=-1))
        c2ws.append(c2w)
        ts.append(t)
    return TrainViews.pinhole(np.stack(imgs), K, np.stack(c2ws), np.array(ts, np.float32), device=DEV)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--size", type=int, default=400)
    p.add_argument("--steps", type=int, default=20000)
    p.add_argument("--train", type=int, default=24)
    p.add_argument("--test", type=int, default=4)
    p.add_argument("--log2_hashmap_size", type=int, default=21)
    p.add_argument("--teacher_log2_hashmap_size", type=int, default=19)
    a = p.parse_args()
    train = teacher_views(a.train, a.size, 0.0, a.teacher_log2_hashmap_size)
    test = teacher_views(a.test, a.size, 11.0, a.teacher_log2_hashmap_size)
    res = trainer.fit(train, test, preset="dnerf", max_steps=a.steps, log2_hashmap_size=a.log2_hashmap_size,
                      log_every=max(1, a.steps // 4))
    h = res["history"]
    secs = np.array([r["seconds"] for r in h])
    per_step = np.diff(secs)[199:] if len(secs) > 201 else np.diff(secs)
    ms = float(np.median(per_step) * 1e3)
    print(json.dumps({"metric": "fit_dnerf_synthetic", "size": a.size, "steps": a.steps, "train_views": a.train,
                      "test_views": a.test, "log2_hashmap_size": a.log2_hashmap_size,
                      "ms_per_step_median_after_200": round(ms, 3), "steps_per_s": round(1e3 / ms, 2),
                      "train_seconds": round(res["train_seconds"], 2), "psnr_avg": round(res["eval"]["psnr_avg"], 3),
                      "ssim_avg": round(float(res["eval"]["ssim_avg"]), 4),
                      "final_num_rays": h[-1]["num_rays"], "skipped_steps": sum(r["skipped"] for r in h)}), flush=True)


if __name__ == "__main__":
    main()
