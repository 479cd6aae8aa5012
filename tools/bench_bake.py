#!/usr/bin/env python3
"""Times export.bake_volume against the hand composition of the calls it replaces (voxel_centers -> query_density ->
torch.nonzero -> expanded _query_rgb), in one process, alternating the two, on a "trained" synthetic field.

Usage: tools/bench_bake.py [--reso 128] [--n-dirs 16] [--modes f32] [--sigma-thresh 1.0] [--reps 15] [--json PATH]
Per mode: milliseconds per call (median of --reps; host clock around a device synchronise, since both sides read counts
back) and the peak of torch.cuda.max_memory_allocated above what was allocated before the call.  The outputs of the two
are compared bit for bit before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def composition(field, t, reso, center, radius, thresh, dirs, apply_act=False):
    from ced_nerf_amd.export import voxel_centers
    P = voxel_centers(reso, center, radius, dirs.device)
    res = field.query_density(P, torch.full((P.shape[0], 1), t, device=P.device), return_feat=True)
    sig, emb = res["density"][:, 0], res["base_mlp_out"]
    keep = torch.nonzero(sig >= thresh)[:, 0]
    m, d = keep.shape[0], dirs.shape[0]
    rgb = field._query_rgb(dirs[None].expand(m, d, 3), emb[keep][:, None].expand(m, d, 15), apply_act)
    return dict(index=keep, xyz=P[keep], sigma=sig[keep], embedding=emb[keep], rgb=rgb)


def measure(fn):
    """(milliseconds, peak bytes above the starting allocation) of one call"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return ms, peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reso", type=int, default=128)
    ap.add_argument("--n-dirs", type=int, default=16)
    ap.add_argument("--modes", default="f32")
    ap.add_argument("--sigma-thresh", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--json", default=None, help="also write the figures here")
    args = ap.parse_args()
    from ced_nerf_amd import export as E, synthetic as S
    from ced_nerf_amd.model import DNGPradianceField
    dev = "cuda:0"
    aabb = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
    params = S.init_field_params(aabb, 1e-4, hash_max_res=1024, log2_hashmap_size=19, use_time_embedding=True,
                                 use_time_attenuation=True, use_div_offsets=True, regime="trained")
    dirs = torch.from_numpy(E.fibonacci_dirs(args.n_dirs)).to(dev)
    center, radius, t = [0.0, 0.0, 0.0], 1.5, 0.5
    rows = []
    for mode in args.modes.split(","):
        f = DNGPradianceField.from_params(params, dev, mlp_precision=mode).eval()
        bake = lambda: E.bake_volume(f, t, reso=args.reso, sigma_thresh=args.sigma_thresh, dirs=dirs)
        hand = lambda: composition(f, t, args.reso, center, radius, args.sigma_thresh, dirs)
        a, b = bake(), hand()
        m = int(a["index"].shape[0])
        same = all(torch.equal(a[k], b[k]) for k in ("index", "xyz", "sigma", "embedding", "rgb"))
        del a, b
        for _ in range(2):                                   # warm-up of both, every shape of the timed window
            bake(); hand()
        times, peaks = {"bake": [], "hand": []}, {"bake": [], "hand": []}
        for _ in range(args.reps):                           # alternate: what shares the machine hits both alike
            for name, fn in (("bake", bake), ("hand", hand)):
                ms, peak = measure(fn)
                times[name].append(ms); peaks[name].append(peak)
        row = dict(mode=mode, reso=args.reso, n_dirs=args.n_dirs, sigma_thresh=args.sigma_thresh, kept=m,
                   cells=args.reso ** 3, identical=bool(same), reps=args.reps,
                   bake_ms=float(np.median(times["bake"])), hand_ms=float(np.median(times["hand"])),
                   bake_ms_min_max=[min(times["bake"]), max(times["bake"])],
                   hand_ms_min_max=[min(times["hand"]), max(times["hand"])],
                   bake_peak_mib=max(peaks["bake"]) / 2 ** 20, hand_peak_mib=max(peaks["hand"]) / 2 ** 20)
        rows.append(row)
        print(f"{mode:10s} reso {args.reso} D {args.n_dirs}: kept {m} of {args.reso ** 3}, identical {same};  "
              f"bake_volume {row['bake_ms']:8.2f} ms, peak {row['bake_peak_mib']:7.1f} MiB;  "
              f"composition {row['hand_ms']:8.2f} ms, peak {row['hand_peak_mib']:7.1f} MiB", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)
    return 0 if all(r["identical"] for r in rows) else 1


if __name__ == "__main__":
    raise SystemExit(main())
