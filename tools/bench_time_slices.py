#!/usr/bin/env python
"""Time the time-sliced occupancy grid (nerfacc_api.TimeSlicedOccGrid).

1. The build: `from_field` (one fused ced_field_density_time_max launch per chunk of cells, then ced_occ_time_slices) on the
   synthetic "trained" field, candidates = all cells of a --resolution^3 grid, against its composition: B * S launches of
   query_density on the same cell centres with a running torch.fmax, then the same ced_occ_time_slices.  The slices are
   asserted equal.  Also the maxima alone: the one fused launch against the B * S launches with their torch.fmax.
2. A frame: the moving ball of tests/occ_time_reference.py (radius 0.4, slides by -sin(pi t) along x; grid 32^3, 8 bins, 3
   probes, dilate 1) rendered at t = 0.45 with render_image_test through `at_time(0.45)` and through `union()`: ms and
   n_samples of both.

ONE process, the two sides of each comparison alternated, median of --repeats.  Writes profiles/time_slices.json.

    python tools/bench_time_slices.py [--resolution 128] [--bins 16] [--samples 5] [--mode f16x2] [--pixels 400] [--repeats 9]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

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


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--bins", type=int, default=16)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--mode", default="f16x2")
    ap.add_argument("--pixels", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "time_slices.json"))
    a = ap.parse_args(argv)
    import occ_time_reference as R
    from ced_nerf_amd import ops, synthetic as S
    from ced_nerf_amd.model import DNGPradianceField
    from ced_nerf_amd.nerfacc_api import TimeSlicedOccGrid
    from ced_nerf_amd.utils import Rays, render_image_test
    dev = "cuda:0"
    aabb = [-1.5] * 3 + [1.5] * 3
    res, B, Sn, step, occ_thre = a.resolution, a.bins, a.samples, 1e-2, 1e-6
    result = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats)

    # ---- 1. the build ----
    params = S.init_field_params(aabb, 1.0 / 32, hash_max_res=256, log2_hashmap_size=15, use_div_offsets=True,
                                 use_time_embedding=True, use_time_attenuation=True, regime="trained")
    field = DNGPradianceField.from_params(params, dev, mlp_precision=a.mode).eval()
    build = lambda: TimeSlicedOccGrid.from_field(field, roi_aabb=aabb, resolution=res, n_bins=B, times_per_bin=Sn,
                                                 render_step_size=step, occ_thre=occ_thre).binaries_t
    cells = torch.arange(res ** 3, device=dev)
    times = TimeSlicedOccGrid.probe_times(B, Sn, dev)

    def expanded(pos):
        rows = []
        for b in range(B):
            m = torch.zeros((cells.numel(),), device=dev)
            for s in range(Sn):
                m = torch.fmax(m, field.query_density(pos, times[b, s].expand(cells.numel()).contiguous())["density"][:, 0])
            rows.append(m)
        return torch.stack(rows)

    def composition():
        pos = ops.occ_cell_points(cells, torch.full((cells.numel(), 3), 0.5, device=dev), res, aabb)
        return ops.occ_time_slices(cells, expanded(pos), step, occ_thre, 1, res)

    assert torch.equal(build(), composition()), "from_field's slices are not the composition's"
    centres = ops.occ_cell_points(cells, torch.full((cells.numel(), 3), 0.5, device=dev), res, aabb)
    desc = field._descriptor()
    ms = {"from_field": [], "composition": [], "maxima_fused": [], "maxima_expanded": []}
    for _ in range(a.repeats):
        ms["from_field"].append(timed(build)[0])
        ms["composition"].append(timed(composition)[0])
        ms["maxima_fused"].append(timed(lambda: ops.field_density_time_max(desc, centres, times))[0])     # the maxima alone
        ms["maxima_expanded"].append(timed(lambda: expanded(centres))[0])
    f_ms, c_ms = statistics.median(ms["from_field"]), statistics.median(ms["composition"])
    evals = res ** 3 * B * Sn
    result["build"] = dict(mode=a.mode, resolution=res, bins=B, samples=Sn, density_evaluations=evals, from_field_ms=f_ms,
                           composition_ms=c_ms, from_field_evaluations_per_s=evals / (f_ms * 1e-3),
                           composition_over_from_field=c_ms / f_ms, maxima_fused_ms=statistics.median(ms["maxima_fused"]),
                           maxima_expanded_ms=statistics.median(ms["maxima_expanded"]), from_field_ms_all=ms["from_field"],
                           composition_ms_all=ms["composition"], maxima_fused_ms_all=ms["maxima_fused"],
                           maxima_expanded_ms_all=ms["maxima_expanded"])
    print(json.dumps({"build": {k: v for k, v in result["build"].items() if not k.endswith("_all")}}), flush=True)

    # ---- 2. a frame of the moving ball ----
    ball = DNGPradianceField.from_params(R.ball_params(), dev, mlp_precision=a.mode).eval()
    g = R.BALL_GRID
    sliced = TimeSlicedOccGrid.from_field(ball, roi_aabb=R.BALL_AABB, resolution=g["resolution"], n_bins=g["n_bins"],
                                          times_per_bin=g["times_per_bin"], render_step_size=g["render_step_size"],
                                          occ_thre=g["occ_thre"], dilate=g["dilate"])
    o, d = S.make_camera_rays(a.pixels, a.pixels, 0.69, S.look_at_c2w(4.0, 30.0, 30.0))
    rays = Rays(origins=torch.from_numpy(o).to(dev), viewdirs=torch.from_numpy(d).to(dev))
    ts = torch.tensor([[0.45]], device=dev)
    kw = dict(near_plane=0.0, far_plane=1e10, render_step_size=g["render_step_size"], render_bkgd=torch.zeros(3, device=dev),
              timestamps=ts)
    grids = {"at_time": sliced.at_time(0.45), "union": sliced.union()}
    frame = {k: (lambda est=est: render_image_test(1024, ball, est, rays, **kw)) for k, est in grids.items()}
    outs = {k: fn() for k, fn in frame.items()}                          # warm-up: the grids' distance fields are built here
    ms = {k: [] for k in frame}
    for _ in range(a.repeats):
        for k, fn in frame.items():
            ms[k].append(timed(fn)[0])
    diff = (outs["at_time"][0] - outs["union"][0]).abs()
    result["frame"] = dict(mode=a.mode, pixels=a.pixels * a.pixels, t=0.45, occupied_fraction=sliced.occupied_fraction().tolist(),
                           cells=dict(at_time=int(grids["at_time"].binaries.sum()), union=int(grids["union"].binaries.sum())),
                           at_time_ms=statistics.median(ms["at_time"]), union_ms=statistics.median(ms["union"]),
                           at_time_n_samples=int(outs["at_time"][3]), union_n_samples=int(outs["union"][3]),
                           rgb_diff_max=float(diff.max()), rgb_diff_mean=float(diff.mean()),
                           at_time_ms_all=ms["at_time"], union_ms_all=ms["union"])
    print(json.dumps({"frame": {k: v for k, v in result["frame"].items() if not k.endswith("_all")}}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
