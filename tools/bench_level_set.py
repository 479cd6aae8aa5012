#!/usr/bin/env python
"""Time the density's level set along rays (ced_field_level_set, utils.render_surface).

On the synthetic "trained" field, --pixels^2 camera rays (default 800^2 = 640 k) marched with --step through an
all-occupied 128^3 grid over the box, at time 0.37 and threshold --thresh:
1. kernel B: ced_field_level_set on the brackets ced_surface_first_crossing hands out for these rays (max_iters 32, tol 0),
   against
2. the unfused loop: the same lines in torch around query_density, one launch and one round trip of positions and
   densities per round.  The two are asserted equal bit for bit.
3. a frame: utils.render_surface (march, density, first crossing, bisection, normals) beside utils.render_image on the
   same rays.

ONE process, the sides of each comparison alternated, median of --repeats.  Writes profiles/level_set.json.

    python tools/bench_level_set.py [--pixels 800] [--step 1e-2] [--thresh 10] [--mode f16x2] [--repeats 9]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    out = fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end), out


def unfused(field, o, d, lo, hi, t, thresh, rounds):
    """include/cednerf_hip.h's lines around query_density (tol = 0)"""
    dens = lambda s: field.query_density(o + d * s[:, None], t)["density"][:, 0]
    lo, hi = lo.clone(), hi.clone()
    s_lo, s_hi = dens(lo), dens(hi)
    one, two, zero = (torch.full_like(lo, v, dtype=torch.int32) for v in (1, 2, 0))
    status = torch.where(s_lo >= thresh, one, torch.where(~(s_hi >= thresh), two, zero))
    evals = two.clone()
    active = status == 0
    for _ in range(rounds):
        m = (lo + hi) / 2
        active = active & ~((hi - lo <= 0) | (m == lo) | (m == hi))
        if not bool(active.any()):
            break
        s = dens(m)
        up = active & (s >= thresh)
        down = active & ~up
        hi, s_hi, lo = torch.where(up, m, hi), torch.where(up, s, s_hi), torch.where(down, m, lo)
        evals = evals + active.to(torch.int32)
    inside = status == 1
    tt = torch.where(inside, lo, hi)
    return (tt, o + d * tt[:, None], torch.where(inside, s_lo, s_hi), torch.where(inside, torch.zeros_like(lo), hi - lo),
            status, evals)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pixels", type=int, default=800)
    ap.add_argument("--step", type=float, default=1e-2)
    ap.add_argument("--thresh", type=float, default=10.0)
    ap.add_argument("--mode", default="f16x2")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "level_set.json"))
    a = ap.parse_args(argv)
    from ced_nerf_amd import ops, synthetic as S
    from ced_nerf_amd.model import DNGPradianceField
    from ced_nerf_amd.nerfacc_api import OccGridEstimator
    from ced_nerf_amd.utils import Rays, render_image, render_surface
    dev = "cuda:0"
    aabb = [-1.5] * 3 + [1.5] * 3
    params = S.init_field_params(aabb, 1.0 / 32, hash_max_res=256, log2_hashmap_size=15, use_div_offsets=True,
                                 use_time_embedding=True, use_time_attenuation=True, regime="trained")
    field = DNGPradianceField.from_params(params, dev, mlp_precision=a.mode).eval()
    est = OccGridEstimator(aabb, 128, 1).to(dev)
    est.set_binaries(torch.ones((1, 128, 128, 128), dtype=torch.bool))
    o, d = S.make_camera_rays(a.pixels, a.pixels, 0.69, S.look_at_c2w(4.0, 30.0, 30.0))
    o, d = torch.from_numpy(o).to(dev).reshape(-1, 3).contiguous(), torch.from_numpy(d).to(dev).reshape(-1, 3).contiguous()
    rays = Rays(origins=o, viewdirs=d)
    ts = torch.tensor([[0.37]], device=dev)
    result = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats, mode=a.mode, rays=int(o.shape[0]), step=a.step,
                  thresh=a.thresh)

    # ---- 1, 2. the bisection alone, on the frame's brackets ----
    t0, t1, ri, packed = est.march(o, d, render_step_size=a.step)
    sig = field.query_rays(o, d, ri, t0, t1, ts, want_rgb=False)[1]
    k, lo, hi = ops.surface_first_crossing(packed, t0, t1, sig.reshape(-1), a.thresh)
    cand = torch.nonzero(k >= 0).squeeze(1)
    oc, dc, lo, hi = o[cand].contiguous(), d[cand].contiguous(), lo[cand].contiguous(), hi[cand].contiguous()
    del t0, t1, ri, sig
    tq = ts.reshape(-1)
    tn = tq.expand(oc.shape[0]).contiguous()
    desc = field._descriptor()
    fused = lambda: ops.field_level_set(desc, oc, dc, lo, hi, tq, a.thresh, 32, 0.0)
    loop = lambda: unfused(field, oc, dc, lo, hi, tn, a.thresh, 32)
    got, want = fused(), loop()
    for g, w, name in zip(got, want, ops.LEVEL_SET_OUTPUTS):
        assert torch.equal(g, w), f"ced_field_level_set's {name} is not the unfused loop's"
    ms = {"fused": [], "unfused": []}
    for _ in range(a.repeats):
        ms["fused"].append(timed(fused)[0])
        ms["unfused"].append(timed(loop)[0])
    evals = int(got[5].sum())
    f_ms, u_ms = statistics.median(ms["fused"]), statistics.median(ms["unfused"])
    result["bisection"] = dict(rows=int(oc.shape[0]), density_evaluations=evals, rounds_max=int(got[5].max()) - 2,
                               status_counts=[int((got[4] == s).sum()) for s in (0, 1, 2)], fused_ms=f_ms, unfused_ms=u_ms,
                               unfused_over_fused=u_ms / f_ms, fused_evaluations_per_s=evals / (f_ms * 1e-3),
                               fused_ms_all=ms["fused"], unfused_ms_all=ms["unfused"])
    print(json.dumps({"bisection": {k: v for k, v in result["bisection"].items() if not k.endswith("_all")}}), flush=True)

    # ---- 3. a frame ----
    kw = dict(near_plane=0.0, far_plane=1e10, render_step_size=a.step, timestamps=ts)
    frame = {"render_surface": lambda: render_surface(field, est, rays, sigma_thresh=a.thresh, colors=False, **kw),
             "render_image": lambda: render_image(field, est, rays, render_bkgd=torch.zeros(3, device=dev), **kw)}
    outs = {k: fn() for k, fn in frame.items()}                          # warm-up: the grid's distance field is built here
    ms = {k: [] for k in frame}
    for _ in range(a.repeats):
        for name, fn in frame.items():
            ms[name].append(timed(fn)[0])
    surf = outs["render_surface"]
    s_ms, i_ms = statistics.median(ms["render_surface"]), statistics.median(ms["render_image"])
    result["frame"] = dict(render_surface_ms=s_ms, render_image_ms=i_ms, surface_over_image=s_ms / i_ms,
                           marched_samples=surf["n_samples"], bisection_evaluations=surf["n_evals"],
                           render_image_samples=int(outs["render_image"][3]), hit_share=float(surf["hit"].float().mean()),
                           render_surface_ms_all=ms["render_surface"], render_image_ms_all=ms["render_image"])
    print(json.dumps({"frame": {k: v for k, v in result["frame"].items() if not k.endswith("_all")}}), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
