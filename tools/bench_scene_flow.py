#!/usr/bin/env python
"""Time DNGPradianceField.query_scene_flow (one fused launch: ced_field_velocity, all three outputs, 17 B per row) at 2^20
rows per mlp_precision, beside the two things it is measured against: query_velocity (the Jacobian launch writing 60 B per
row plus a batched 3 x 3 inverse in torch) and the query_move_jacobian kernel alone.  ONE process, the three alternated,
median of --repeats; output allocations included on every side.  With --frame N also utils.render_scene_flow beside
utils.render_motion on an N x N frame of the synthetic D-NeRF scene.  Writes profiles/scene_flow.json.

    python tools/bench_scene_flow.py [--log2_rows 20] [--repeats 9] [--modes f32,f16,f16x2,f32+h16x2] [--frame 800]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    out = fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end), out


def spread(values):
    return (max(values) - min(values)) / statistics.median(values)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--log2_rows", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--modes", default="f32,f16,f16x2,f32+h16x2")
    ap.add_argument("--frame", type=int, default=0, help="also time render_scene_flow / render_motion on an N x N frame")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_flow.json"))
    a = ap.parse_args(argv)
    from ced_nerf_amd import synthetic as S
    from ced_nerf_amd.model import DNGPradianceField
    dev = "cuda:0"
    n = 1 << a.log2_rows
    params = S.init_field_params([-1.5] * 3 + [1.5] * 3, 1.0 / 32, hash_max_res=256, log2_hashmap_size=15,
                                 use_div_offsets=True, use_time_embedding=True, use_time_attenuation=True, regime="trained")
    rng = np.random.default_rng(7)
    x = torch.from_numpy(rng.uniform(-1.5, 1.5, size=(n, 3)).astype(np.float32)).to(dev)
    t = torch.from_numpy(rng.uniform(0.0, 1.0, size=(n,)).astype(np.float32)).to(dev)
    result = dict(rows=n, repeats=a.repeats, device=torch.cuda.get_device_name(0), modes={})
    names = ("scene_flow", "velocity", "jacobian")
    for mode in a.modes.split(","):
        field = DNGPradianceField.from_params(params, dev, mlp_precision=mode).eval()
        calls = dict(scene_flow=lambda: field.query_scene_flow(x, t), velocity=lambda: field.query_velocity(x, t),
                     jacobian=lambda: field.query_move_jacobian(x, t))
        got, want = calls["scene_flow"](), calls["velocity"]()          # warm-up of both, and that they agree
        calls["jacobian"]()
        away = got[1] > 0.25                                            # far from a fold both solves are well conditioned
        assert float(away.float().mean()) > 0.99 and float((got[0] - want[0])[away].abs().max()) <= 1e-4, \
            "query_scene_flow is not query_velocity's"
        ms = {k: [] for k in names}
        for _ in range(a.repeats):
            for k in names:
                ms[k].append(timed(calls[k])[0])
        med = {k: statistics.median(ms[k]) for k in names}
        result["modes"][mode] = dict(
            scene_flow_ms=med["scene_flow"], velocity_ms=med["velocity"], jacobian_ms=med["jacobian"],
            scene_flow_rows_per_s=n / (med["scene_flow"] * 1e-3), scene_flow_over_velocity=med["scene_flow"] / med["velocity"],
            scene_flow_over_jacobian=med["scene_flow"] / med["jacobian"], jacobian_spread=spread(ms["jacobian"]),
            scene_flow_spread=spread(ms["scene_flow"]), **{k + "_ms_all": ms[k] for k in names})
        print(json.dumps({mode: {k: v for k, v in result["modes"][mode].items() if not k.endswith("_all")}}), flush=True)
    if a.frame > 0:
        from ced_nerf_amd.nerfacc_api import OccGridEstimator
        from ced_nerf_amd.utils import Rays, render_motion, render_scene_flow
        sc = S.make_scene("dnerf", a.frame, a.frame, "trained", log2_hashmap_size=17)
        cfg = sc["cfg"]
        T = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
        field = DNGPradianceField.from_params(sc["params"], dev).eval()
        est = OccGridEstimator(cfg["aabb"], cfg["grid_resolution"], cfg["grid_levels"]).to(dev)
        est.set_binaries(T(sc["binaries"]))
        rays, ts = Rays(T(sc["origins"]), T(sc["viewdirs"])), T(sc["timestamps"])
        kw = {k: v for k, v in sc["render"].items() if k != "render_bkgd"}
        calls = dict(render_motion=lambda: render_motion(field, est, rays, timestamps=ts, **kw),
                     render_scene_flow=lambda: render_scene_flow(field, est, rays, timestamps=ts, **kw))
        ms = {k: [] for k in calls}
        samples = {k: fn()[-1] for k, fn in calls.items()}               # warm-up
        for _ in range(a.repeats):
            for k, fn in calls.items():
                ms[k].append(timed(fn)[0])
        result["frame"] = dict(size=a.frame, n_samples=samples["render_scene_flow"],
                               **{k + "_ms": statistics.median(v) for k, v in ms.items()},
                               **{k + "_ms_all": v for k, v in ms.items()})
        print(json.dumps({"frame": {k: v for k, v in result["frame"].items() if not k.endswith("_all")}}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
