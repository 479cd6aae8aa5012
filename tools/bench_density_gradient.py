#!/usr/bin/env python
"""Time DNGPradianceField's density gradient (one fused launch: ced_field_density_gradient, all four outputs) at 2^20 rows
per mlp_precision, beside the same rows through query_density plus query_move_jacobian -- that pair does this kernel's
primal work plus the warp's tangents, so it is the yardstick; the gradient kernel adds the three tangent tiles through
mlp_base and the tangent half of the gather.  ONE process, the two alternated, median of --repeats; output allocations
included on both sides.  Writes profiles/density_gradient.json.

    python tools/bench_density_gradient.py [--log2_rows 20] [--repeats 9] [--modes f32,f16,f16x2,f32+h16x2] [--hash_max_res 256]
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


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--log2_rows", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--modes", default="f32,f16,f16x2,f32+h16x2")
    ap.add_argument("--hash_max_res", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density_gradient.json"))
    a = ap.parse_args(argv)
    from ced_nerf_amd import ops, synthetic as S
    from ced_nerf_amd.model import DNGPradianceField
    dev = "cuda:0"
    n = 1 << a.log2_rows
    params = S.init_field_params([-1.5] * 3 + [1.5] * 3, 1.0 / 32, hash_max_res=a.hash_max_res, log2_hashmap_size=15,
                                 use_div_offsets=True, use_time_embedding=True, use_time_attenuation=True, regime="trained")
    rng = np.random.default_rng(7)
    x = torch.from_numpy(rng.uniform(-1.5, 1.5, size=(n, 3)).astype(np.float32)).to(dev)
    t = torch.from_numpy(rng.uniform(0.0, 1.0, size=(n,)).astype(np.float32)).to(dev)
    result = dict(rows=n, repeats=a.repeats, hash_max_res=a.hash_max_res, device=torch.cuda.get_device_name(0), modes={})
    for mode in a.modes.split(","):
        field = DNGPradianceField.from_params(params, dev, mlp_precision=mode).eval()
        desc = field._descriptor()
        fused = lambda: ops.field_density_gradient(desc, x, t)
        pair = lambda: (field.query_density(x, t), field.query_move_jacobian(x, t))
        got, (dens, _) = fused(), pair()                                # warm-up of both, and the primal's identity
        assert torch.equal(got[0], dens["density"][:, 0]), "the gradient kernel's density is not query_density's"
        ms = {"gradient": [], "density_plus_jacobian": []}
        for _ in range(a.repeats):
            ms["gradient"].append(timed(fused)[0])
            ms["density_plus_jacobian"].append(timed(pair)[0])
        g, p = statistics.median(ms["gradient"]), statistics.median(ms["density_plus_jacobian"])
        result["modes"][mode] = dict(gradient_ms=g, density_plus_jacobian_ms=p, gradient_rows_per_s=n / (g * 1e-3),
                                     density_plus_jacobian_rows_per_s=n / (p * 1e-3), gradient_over_pair=g / p,
                                     gradient_ms_all=ms["gradient"], density_plus_jacobian_ms_all=ms["density_plus_jacobian"])
        print(json.dumps({mode: {k: v for k, v in result["modes"][mode].items() if not k.endswith("_all")}}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
