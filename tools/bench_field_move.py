#!/usr/bin/env python3
"""Times ced_field_move_rays and ced_field_rgb against the fused ced_field_forward_rays at the same sample count, in the
same run (default: the training bench's 1.59 M kept samples, tools/bench_train.py).

Usage: tools/bench_field_move.py [--n 1590000] [--modes f32,f16x2,f16,f32+h16x2] [--reps 20] [--time-mode 0]
Prints one line per mode: microseconds per call (median of --reps, device events) and samples per second."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_590_000)
    ap.add_argument("--modes", default="f32,f16x2,f16,f32+h16x2")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--time-mode", type=int, default=0, choices=(0, 2))
    args = ap.parse_args()
    from ced_nerf_amd import ops, synthetic as S
    from ced_nerf_amd.model import DNGPradianceField
    dev = "cuda:0"
    n, n_rays = args.n, 4096
    params = S.init_field_params([-1.5, -1.5, -1.5, 1.5, 1.5, 1.5], 1e-4, hash_max_res=1024, log2_hashmap_size=19,
                                 use_time_embedding=args.time_mode != 0, use_time_attenuation=args.time_mode == 2,
                                 use_div_offsets=args.time_mode != 0, regime="trained")
    rng = np.random.default_rng(0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    o = T(rng.uniform(-0.2, 0.2, size=(n_rays, 3)).astype(np.float32))
    d = rng.normal(size=(n_rays, 3)); d = T((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))
    ri = T(np.sort(rng.integers(0, n_rays, size=n)).astype(np.int64))
    t0 = T(rng.uniform(0.0, 1.2, size=n).astype(np.float32)); t1 = t0 + 5e-3
    ts = T(rng.uniform(0.0, 1.0, size=n_rays).astype(np.float32))
    dirs = d[ri].contiguous()
    for mode in args.modes.split(","):
        f = DNGPradianceField.from_params(params, dev, mlp_precision=mode).eval()
        desc = f._descriptor()
        pos = (o[ri] + (d[ri] * (t0 + t1)[:, None]) / 2.0).contiguous()
        geo = ops.field_forward(desc, pos, ts[ri].contiguous(), dirs, want_geo=True)[2]
        fused = timed(lambda: ops.field_forward_rays(desc, o, d, ri, t0, t1, ts, True, True), args.reps)
        sigma = timed(lambda: ops.field_forward_rays(desc, o, d, ri, t0, t1, ts, True, False), args.reps)
        move = timed(lambda: ops.field_move_rays(desc, o, d, ri, t0, t1, ts, True), args.reps)
        rgb = timed(lambda: ops.field_rgb(desc, dirs, geo), args.reps)
        print(f"{mode:10s} n={n}  field_forward_rays {fused:8.1f} us (density only {sigma:8.1f} us)  "
              f"field_move_rays {move:8.1f} us ({n / move:7.1f} M/s)  field_rgb {rgb:8.1f} us ({n / rgb:7.1f} M/s)", flush=True)


if __name__ == "__main__":
    main()
