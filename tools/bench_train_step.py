"""train.train_step on the 800x800 D-NeRF-shaped scene, with and without a CameraRefinement, and the input stage's
backward on a step's own samples.

    python tools/bench_train_step.py [--rays 262144] [--repeats 9] [--steps 5] [--root DIR] [--out FILE.json]

Every repeat times `--steps` steps of each variant in turn (plain, refined, plain, refined, ...) in one process, between
device synchronisations; the figure of a variant is the median of its repeats, the spread their minimum and maximum.
lr = 0 keeps the parameters, hence the sample counts, the same from step to step.  --root: the checkout to time (default:
this file's); on one without CameraRefinement only the plain variant runs, which is how a parent commit is timed beside
this one.  Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import statistics
import sys
import time


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=262144)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np
    import torch
    from ced_nerf_amd import ops, synthetic as S, train as TR
    from ced_nerf_amd.nerfacc_api import OccGridEstimator, _packed_info_from
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = "cuda:0"
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    sc = S.make_scene("dnerf", 800, 800, "trained")
    cfg = sc["cfg"]
    est = OccGridEstimator(cfg["aabb"], 128, cfg["grid_levels"]).to(dev)
    est.set_binaries(T(sc["binaries"]))
    field = TR.TrainableField(sc["params"], dev)
    o, d, ts = T(sc["origins"]).reshape(-1, 3), T(sc["viewdirs"]).reshape(-1, 3), T(sc["timestamps"])
    bk = T(sc["render"]["render_bkgd"])
    gen = torch.Generator(device=dev).manual_seed(0)
    target = torch.rand(a.rays, 3, device=dev, generator=gen)
    n_views = 100
    variants = {"plain": None}
    if hasattr(TR, "CameraRefinement"):
        variants["refined"] = TR.CameraRefinement(n_views).to(dev)
    opts = {}
    for name, ref in variants.items():
        opts[name] = torch.optim.Adam(field.parameters(), lr=0.0, eps=1e-15, fused=True)
        if ref is not None:
            opts[name].add_param_group(dict(params=list(ref.parameters()), lr=0.0))
    samples = {}

    def steps(name, count):
        for _ in range(count):
            idx = torch.randint(0, o.shape[0], (a.rays,), device=dev, generator=gen)
            extra = {} if variants[name] is None else dict(refinement=variants[name], view_indices=idx % n_views)
            out = TR.train_step(field, est, opts[name], o[idx].contiguous(), d[idx].contiguous(), ts, target,
                                cfg["render_step_size"], near_plane=cfg["near_plane"], far_plane=cfg["far_plane"],
                                render_bkgd=bk, **extra)
            samples[name] = out["n_samples"]

    for name in variants:                                  # every shape of the timed window, before it
        steps(name, 3)
    times = {name: [] for name in variants}
    for _ in range(a.repeats):
        for name in variants:
            torch.cuda.synchronize()
            tic = time.perf_counter()
            steps(name, a.steps)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - tic) / a.steps * 1e3)
    res = dict(rays=a.rays, repeats=a.repeats, steps_per_repeat=a.steps, root=os.path.abspath(a.root), step_ms={
        name: dict(median=statistics.median(v), min=min(v), max=max(v), samples_per_step=samples[name]) for name, v in times.items()})

    if hasattr(ops, "train_inputs_backward"):
        # the new backward on the samples of one step: device events around each of 20 calls
        idx = torch.randint(0, o.shape[0], (a.rays,), device=dev, generator=gen)
        ro, rd, tr = o[idx].contiguous(), d[idx].contiguous(), ts.reshape(-1).expand(a.rays).contiguous()
        fused = field.shared_inference()
        fused.train()
        ri, t0, t1 = est.sampling(ro, rd, sigma_fn=None, near_plane=cfg["near_plane"], far_plane=cfg["far_plane"],
                                  render_step_size=cfg["render_step_size"], stratified=True,
                                  sigma_field=(fused, tr.reshape(-1, 1), True))
        n = int(ri.shape[0])
        up = dict(d_pos=torch.randn(n, 3, device=dev), d_enc=torch.randn(n, 32, device=dev), d_sh=torch.randn(n, 4, device=dev),
                  d_t=torch.randn(n, device=dev))
        packed = _packed_info_from(ri, a.rays)
        call = lambda: ops.train_inputs_backward(n, ro, rd, ri, t0, t1, tr, packed_info=packed, **up)
        for _ in range(3):
            call()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
        for b, e in ev:
            b.record(); call(); e.record()
        torch.cuda.synchronize()
        us = sorted(b.elapsed_time(e) * 1e3 for b, e in ev)
        # what the call must move: per sample d_enc 128, d_sh 16, d_pos 12, d_t 4, ray index 8, interval 8 bytes; per ray
        # origin, direction, time in (28), packed_info (16) and the three outputs (28)
        nbytes = n * (128 + 16 + 12 + 4 + 8 + 8) + a.rays * (28 + 16 + 28)
        res["inputs_backward"] = dict(samples=n, rays=a.rays, call_us_median=us[len(us) // 2], call_us_min=us[0],
                                      bytes=nbytes, gbytes_per_s=nbytes / (us[len(us) // 2] * 1e-6) / 1e9)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
