#!/usr/bin/env python3
"""Times export.extract_mesh (dirs="normal") beside export.bake_volume (one direction) on tools/bench_bake.py's "trained"
synthetic field, in one process, alternating the two.

Usage: tools/bench_mesh.py [--reso 128] [--modes f32] [--sigma-thresh 1.0] [--reps 9] [--json PATH]
Per mode: milliseconds per call (median of --reps; host clock around a device synchronise, since both read counts back) and
the peak of torch.cuda.max_memory_allocated above what was allocated before the call."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_bake import measure  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reso", type=int, default=128)
    ap.add_argument("--modes", default="f32")
    ap.add_argument("--sigma-thresh", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", default=None, help="also write the figures here")
    args = ap.parse_args()
    from ced_nerf_amd import export as E, synthetic as S
    from ced_nerf_amd.model import DNGPradianceField
    dev = "cuda:0"
    aabb = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
    params = S.init_field_params(aabb, 1e-4, hash_max_res=1024, log2_hashmap_size=19, use_time_embedding=True,
                                 use_time_attenuation=True, use_div_offsets=True, regime="trained")
    one_dir = torch.from_numpy(E.fibonacci_dirs(1)).to(dev)
    t = 0.5
    rows = []
    for mode in args.modes.split(","):
        f = DNGPradianceField.from_params(params, dev, mlp_precision=mode).eval()
        mesh = lambda: E.extract_mesh(f, t, reso=args.reso, sigma_thresh=args.sigma_thresh, dirs="normal")
        bake = lambda: E.bake_volume(f, t, reso=args.reso, sigma_thresh=args.sigma_thresh, dirs=one_dir)
        a, b = mesh(), bake()
        n_v, n_f, kept = int(a["vertices"].shape[0]), int(a["faces"].shape[0]), int(b["index"].shape[0])
        del a, b
        for _ in range(2):                                   # warm-up of both, every shape of the timed window
            mesh(); bake()
        times, peaks = {"mesh": [], "bake": []}, {"mesh": [], "bake": []}
        for _ in range(args.reps):                           # alternate: what shares the machine hits both alike
            for name, fn in (("mesh", mesh), ("bake", bake)):
                ms, peak = measure(fn)
                times[name].append(ms); peaks[name].append(peak)
        row = dict(mode=mode, reso=args.reso, sigma_thresh=args.sigma_thresh, vertices=n_v, faces=n_f, kept=kept,
                   cells=args.reso ** 3, reps=args.reps,
                   mesh_ms=float(np.median(times["mesh"])), bake_ms=float(np.median(times["bake"])),
                   mesh_ms_min_max=[min(times["mesh"]), max(times["mesh"])],
                   bake_ms_min_max=[min(times["bake"]), max(times["bake"])],
                   mesh_peak_mib=max(peaks["mesh"]) / 2 ** 20, bake_peak_mib=max(peaks["bake"]) / 2 ** 20)
        rows.append(row)
        print(f"{mode:10s} reso {args.reso}: {n_v} vertices, {n_f} triangles; bake keeps {kept} of {args.reso ** 3};  "
              f"extract_mesh {row['mesh_ms']:8.2f} ms, peak {row['mesh_peak_mib']:7.1f} MiB;  "
              f"bake_volume {row['bake_ms']:8.2f} ms, peak {row['bake_peak_mib']:7.1f} MiB", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
