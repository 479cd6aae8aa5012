#!/usr/bin/env python
"""Time DNGPradianceField.track_points (one fused launch: ced_field_track) against the composition it replaces -- a loop of
query_move launches with the update and the per-row freeze in torch -- on P points x T times, in ONE process, the two
alternated, median of --repeats.  Asserts that the outputs are equal bit for bit, also times the fixed-point launch on its
own and counts the rounds its wave tiles run, and writes profiles/track_vs_composition.json.

--method newton times the fused Newton solver (ced_field_track_newton) instead, against ITS composition -- a loop of
query_move_jacobian launches with the 3 x 3 solve and the freeze in torch -- and against the fixed-point launch on the
same rows, and writes profiles/track_newton_vs_composition.json; whether the composition's bits are the kernel's is
reported, not asserted (the bit-for-bit check of the Newton solver is tests/test_gpu_warp_jacobian.py's, in numpy).

    python tools/bench_track.py [--points 200000] [--times 16] [--repeats 9] [--mode f16x2] [--moving_step 0.03125]
                                [--method fixed_point|newton]
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


def composition(field, canonical, times, init, max_iters, tol):
    """track_points' rows through the public pieces that exist without the fused kernel: the expanded rows, max_iters
    launches of query_move at the most, the fp32 update and the freeze in torch"""
    n_t, p = times.shape[0], canonical.shape[0]
    c = canonical.repeat(n_t, 1)
    t = times.repeat_interleave(p)
    x = init.repeat(n_t, 1)
    n = c.shape[0]
    step = torch.full((n,), float("inf"), device=c.device)
    evals = torch.zeros((n,), device=c.device, dtype=torch.int32)
    active = torch.ones((n,), device=c.device, dtype=torch.bool)
    for _ in range(max_iters):
        m = field.query_move(x, t)[1]
        x_new = c - m
        d = (x_new - x).abs()
        s = torch.fmax(torch.fmax(d[:, 0], d[:, 1]), d[:, 2])
        x = torch.where(active[:, None], x_new, x)
        step = torch.where(active, s, step)
        evals = evals + active.to(torch.int32)
        active = active & ~(s <= tol)
        if not bool(active.any()):                                       # one host sync per round: the loop's own early exit
            break
    return x.view(n_t, p, 3), step.view(n_t, p), evals.view(n_t, p)


def newton_composition(field, canonical, times, init, max_iters, tol):
    """the Newton solver's rows through query_move_jacobian and torch: include/cednerf_hip.h's lines, one torch operation
    per fp32 operation"""
    n_t, p = times.shape[0], canonical.shape[0]
    c = canonical.repeat(n_t, 1)
    t = times.repeat_interleave(p)
    x = init.repeat(n_t, 1)
    n = c.shape[0]
    step = torch.full((n,), float("inf"), device=c.device)
    evals = torch.zeros((n,), device=c.device, dtype=torch.int32)
    active = torch.ones((n,), device=c.device, dtype=torch.bool)
    for k in range(1, max_iters + 1):
        m, J = field.query_move_jacobian(x, t)
        r = (x + m) - c
        d = r.abs()
        res = torch.fmax(torch.fmax(d[:, 0], d[:, 1]), d[:, 2])
        step = torch.where(active, res, step)
        evals = evals + active.to(torch.int32)
        active = active & ~(res <= tol)
        if k == max_iters or not bool(active.any()):
            break
        A = J[:, :, :3].clone()
        for a in range(3):
            A[:, a, a] = 1.0 + J[:, a, a]
        C = [[A[:, (a + 1) % 3, (b + 1) % 3] * A[:, (a + 2) % 3, (b + 2) % 3] - A[:, (a + 1) % 3, (b + 2) % 3] * A[:, (a + 2) % 3, (b + 1) % 3]
              for b in range(3)] for a in range(3)]
        det = (A[:, 0, 0] * C[0][0] + A[:, 0, 1] * C[0][1]) + A[:, 0, 2] * C[0][2]
        dx = torch.stack([((C[0][a] * r[:, 0] + C[1][a] * r[:, 1]) + C[2][a] * r[:, 2]) / det for a in range(3)], -1)
        fine = (det.abs() >= 2.0 ** -20) & torch.isfinite(dx).all(-1)
        dx = torch.where(fine[:, None], dx, r)
        x = torch.where(active[:, None], x - dx, x)
    return x.view(n_t, p, 3), step.view(n_t, p), evals.view(n_t, p)


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
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--times", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--max_iters", type=int, default=32)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--mode", default="f16x2", choices=["f32", "f16", "f16x2", "f32+h16x2"])
    ap.add_argument("--moving_step", type=float, default=1.0 / 32)
    ap.add_argument("--method", default="fixed_point", choices=["fixed_point", "newton"])
    ap.add_argument("--out", default=None, help="default: profiles/track_vs_composition.json, or "
                                                 "profiles/track_newton_vs_composition.json with --method newton")
    a = ap.parse_args(argv)
    newton = a.method == "newton"
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "track_newton_vs_composition.json" if newton else "track_vs_composition.json")
    from ced_nerf_amd import ops, synthetic as S
    from ced_nerf_amd.model import DNGPradianceField
    dev = "cuda:0"
    params = S.init_field_params([-1.5] * 3 + [1.5] * 3, a.moving_step, hash_max_res=256, log2_hashmap_size=15,
                                 use_div_offsets=True, use_time_embedding=True, use_time_attenuation=True, regime="trained")
    field = DNGPradianceField.from_params(params, dev, mlp_precision=a.mode).eval()
    rng = np.random.default_rng(7)
    x = torch.from_numpy(rng.uniform(-1.5, 1.5, size=(a.points, 3)).astype(np.float32)).to(dev)
    times = torch.linspace(0.0, 1.0, a.times, device=dev)
    t_src = 0.5

    fused = lambda: field.track_points(x, t_src, times, max_iters=a.max_iters, tol=a.tol, method=a.method)
    tr = fused()
    compose = newton_composition if newton else composition
    composed = lambda: compose(field, tr["canonical"], times, x, a.max_iters, a.tol)
    want = composed()                                                   # warm-up of both, and the identity check
    identical = all(torch.equal(got, ref) for got, ref in zip((tr["positions"], tr["step"], tr["evals"]), want))
    assert identical or newton, "the fused kernel and the composition differ"
    # the solver's launch on its own (track_points without its ced_field_move), in the same alternation
    desc = field._descriptor()
    track = ops.field_track_newton if newton else ops.field_track
    kernel = lambda: track(desc, tr["canonical"], times, x, a.max_iters, a.tol)
    fixed = lambda: ops.field_track(desc, tr["canonical"], times, x, a.max_iters, a.tol)
    fixed_out = fixed()
    ms = {"fused": [], "composition": [], "kernel": [], "fixed_point_kernel": []}
    for _ in range(a.repeats):
        ms["fused"].append(timed(fused)[0])
        ms["composition"].append(timed(composed)[0])
        ms["kernel"].append(timed(kernel)[0])
        if newton:
            ms["fixed_point_kernel"].append(timed(fixed)[0])
    evals = tr["evals"]
    # a wave tile is 32 (Newton: 16) consecutive rows and runs to its slowest row: the rounds the kernel really executes
    tile = 16 if newton else 32
    flat = evals.reshape(-1)
    pad = (-flat.numel()) % tile
    rounds = torch.cat([flat, flat.new_zeros(pad)]).view(-1, tile).max(dim=1).values.float()
    kernel_ms = statistics.median(ms["kernel"])
    # MFMA work of one evaluation of one row, as issued (padded): 32x64, 64x64, 64x64, 64x16 multiply-adds -- five columns
    # per row with the four tangents
    flop_per_eval = 2 * (32 * 64 + 64 * 64 + 64 * 64 + 64 * 16) * (5 if newton else 1)
    mfma_tflops = float(rounds.sum()) * tile * flop_per_eval / (kernel_ms * 1e-3) / 1e12
    result = dict(points=a.points, times=a.times, rows=a.points * a.times, mode=a.mode, method=a.method, moving_step=a.moving_step,
                  max_iters=a.max_iters, tol=a.tol, repeats=a.repeats, device=torch.cuda.get_device_name(0),
                  fused_ms=statistics.median(ms["fused"]), composition_ms=statistics.median(ms["composition"]),
                  kernel_ms=kernel_ms, fused_ms_all=ms["fused"], composition_ms_all=ms["composition"], kernel_ms_all=ms["kernel"],
                  tile_rounds_mean=float(rounds.mean()), tile_rounds_max=int(rounds.max()), kernel_mfma_tflops=mfma_tflops,
                  evals_mean=float(evals.float().mean()), evals_max=int(evals.max()),
                  unconverged_share=float((~tr["converged"]).float().mean()), bit_identical=identical,
                  note="fused = track_points (ced_field_move + ced_field_track); composition = its rows through query_move and "
                       "torch, with the loop's own early exit; kernel = ced_field_track alone; all include their output allocations.  "
                       "tile_rounds = evaluations of a wave tile (32 rows; Newton: 16; its slowest row); kernel_mfma_tflops = the MFMA "
                       "work of those rounds, padding (and with Newton the four tangent columns) included, over kernel_ms")
    if newton:
        result.update(fixed_point_kernel_ms=statistics.median(ms["fixed_point_kernel"]), fixed_point_kernel_ms_all=ms["fixed_point_kernel"],
                      fixed_point_unconverged_share=float((~(fixed_out[1] <= a.tol)).float().mean()),
                      fixed_point_evals_mean=float(fixed_out[2].float().mean()))
    result["composition_over_fused"] = result["composition_ms"] / result["fused_ms"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if not k.endswith("_all")}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
