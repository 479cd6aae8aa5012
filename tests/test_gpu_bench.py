"""bench.py's plain run end to end: the result line of the headline figure only, and --dump-outputs holding what the
timed path returned (the same bits from run to run, and the same bits as the frame rendered alone)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 256, 256


def _plain_bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--width", str(W), "--height", str(H), "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    from ced_nerf_amd import synthetic as S
    from ced_nerf_amd.model import DNGPradianceField
    from ced_nerf_amd.nerfacc_api import OccGridEstimator
    from ced_nerf_amd.utils import Rays, render_image_test
    d = _plain_bench(tmp_path / "a")
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "samples/s" and d["higher_is_better"] is True
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["mlp_precision"] == "f16x2" and d["dtype"].startswith("f32")
    assert d["windows"]["n"] == 1 and d["roofline"]["bound"] == "hbm"
    for key in ("cpu_baseline", "parity_vs_oracle", "other_mlp_precisions", "roofline_single_frame"):
        assert key not in d, key
    assert d["single_frame_latency_ms"] is None and d["render_image"] is None and d["gui_operating_point"] is None

    names = ("rgb", "opacity", "depth", "pixel_index", "samples_per_call")
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in names}
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert sum(os.path.getsize(tmp_path / "a" / f"{n}.npy") for n in names) <= 64e6
    frames = d["config"]["frames_per_step"]
    n = a["pixel_index"].shape[0]
    assert a["rgb"].shape == (frames, n, 3) and a["opacity"].shape == a["depth"].shape == (frames, n)
    assert 0 < n < W * H                                               # this step's frames exceed the budget: a sample
    # every step renders the same frames: the last step's samples are the timed samples / steps
    assert a["samples_per_call"].shape == (3,)
    assert a["samples_per_call"].sum() == pytest.approx(d["value"] * d["ms_per_step"] / 1e3, rel=1e-9)

    b = _plain_bench(tmp_path / "b")                                   # same arguments: the same outputs, bit for bit
    for nm in names:
        assert np.array_equal(a[nm].view(np.uint8), np.load(tmp_path / "b" / f"{nm}.npy").view(np.uint8)), nm
    assert b["value"] > 0

    # frame 0 of the step (lane 0's first frame: the scene's own camera) rendered alone
    sc = S.make_scene("dnerf", W, H, "trained", azim_deg=30.0)
    cfg = sc["cfg"]
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    field = DNGPradianceField.from_params(sc["params"], DEV, mlp_precision="f16x2").eval()
    est = OccGridEstimator(cfg["aabb"], cfg["grid_resolution"], cfg["grid_levels"]).to(DEV)
    est.set_binaries(T(sc["binaries"]))
    rk = dict(sc["render"]); rk["render_bkgd"] = T(rk["render_bkgd"])
    rgb, op, dp, _ = render_image_test(1024, field, est, Rays(T(sc["origins"]), T(sc["viewdirs"])),
                                       timestamps=T(sc["timestamps"]), **rk)
    idx = torch.from_numpy(a["pixel_index"].astype(np.int64)).to(DEV)
    for got, want, nm in ((a["rgb"][0], rgb.reshape(-1, 3), "rgb"), (a["opacity"][0], op.reshape(-1), "opacity"),
                          (a["depth"][0], dp.reshape(-1), "depth")):
        assert np.array_equal(got.view(np.uint32), want[idx].cpu().numpy().view(np.uint32)), nm
