"""GPU suite: the entries of csrc/field_move.hip, csrc/field_jacobian.hip and csrc/field_density_gradient.hip do not depend
on the launch grid.

Their kernels are persistent: wave w of workgroup b takes tiles b * WAVES + w, + gridDim.x * WAVES, ...  With the default cap
of 512 workgroups of 8 waves (256 for the density gradient) every wave of the other suites' largest input (4 099 rows) takes
one tile, so the stride of that loop is exercised here: `max_workgroups` 1 and 3 at n = 257 and 4 099.  One workgroup at
4 099 rows is 129 tiles of 32 rows (257 of 16 for the Jacobian, Newton, velocity and density-gradient kernels) over 8 waves
-- many rounds, a ragged last tile, waves that run out at different rounds; three workgroups give a stride that does not
divide the tile count.  Every output must be `torch.equal` to the same call on the default descriptor, whose outputs the
neighbouring suites pin to the oracle.  The rays entries run with per-ray and with shared timestamps, and with a
device-side count below n into prefilled `out=` buffers: the rows past the count must stay as they were on every grid.

Fields: synthetic.init_field_params("trained"), fine offsets on, time_mode 0 and 2, moving step 1/32, in the four
precisions: the fp32 chain, fp16 operands, split fp16 on the K = 32 placements (time_mode 0) and on the pair form
(time_mode 2)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
AABB = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
STEP = 1.0 / 32
SIZES = (257, 4099)
WORKGROUPS = (1, 3)
MODES = ("f32", "f16", "f16x2", "f32+h16x2")
N_DIRS = 3                                                           # field_rgb_bcast: n embeddings x 3 directions


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _field(tm, mode):
    from ced_nerf_amd import synthetic as S
    from ced_nerf_amd.model import DNGPradianceField
    params = S.init_field_params(list(AABB), STEP, hash_max_res=256, log2_hashmap_size=15, use_div_offsets=True,
                                 use_time_embedding=tm != 0, use_time_attenuation=tm == 2, regime="trained")
    return DNGPradianceField.from_params(params, DEV, mlp_precision=mode).eval()


@functools.lru_cache(maxsize=None)
def _inputs():
    rng = np.random.default_rng(11)
    n = max(SIZES)
    n_rays = 97
    d = rng.normal(size=(n_rays, 3))
    t0 = rng.uniform(0.0, 2.0, size=n).astype(np.float32)
    return dict(
        pos=T(rng.uniform(-1.6, 1.6, size=(n, 3)).astype(np.float32)),
        t=T(rng.uniform(0.0, 1.0, size=(n,)).astype(np.float32)),
        times=T(rng.uniform(0.0, 1.0, size=(16,)).astype(np.float32)),
        dirs=T((rng.normal(size=(n, 3)) * rng.uniform(0.1, 5.0, size=(n, 1))).astype(np.float32)),
        geo=T(rng.normal(size=(n, 15)).astype(np.float32)),
        rays_o=T(rng.uniform(-1.0, 1.0, size=(n_rays, 3)).astype(np.float32)),
        rays_d=T((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)),
        ray_idx=T(np.sort(rng.integers(0, n_rays, size=n)).astype(np.int64)),
        t0=T(t0), t1=T((t0 + np.float32(0.02)).astype(np.float32)),
        ts_rays=T(rng.uniform(0.0, 1.0, size=(n_rays,)).astype(np.float32)),
        ts_one=T(rng.uniform(0.0, 1.0, size=(1,)).astype(np.float32)))


def _calls(n):
    """(name, fn(desc) -> tuple of tensors / None) for every entry on n rows"""
    from ced_nerf_amd import ops
    I = _inputs()
    pos, t = I["pos"][:n], I["t"][:n]
    ri, t0, t1 = I["ray_idx"][:n], I["t0"][:n], I["t1"][:n]
    # tracked points x times: 257 x 16 and 4 099 x 1
    times = I["times"][:16 if n == 257 else 1]

    def rays(ts, per_ray, keep=None):
        def fn(d):
            if keep is None:
                return ops.field_move_rays(d, I["rays_o"], I["rays_d"], ri, t0, t1, ts, per_ray, want_x_norm=True)
            # a device-side count below n: the rows past it stay as they were
            out = (torch.full((n, 3), 7.0, device=DEV), torch.full((n, 3), 7.0, device=DEV))
            return ops.field_move_rays(d, I["rays_o"], I["rays_d"], ri, t0, t1, ts, per_ray,
                                       n_dev=torch.tensor([keep], device=DEV, dtype=torch.int64), out=out)
        return fn

    def rays_of(op, fills):
        """op_rays with per-ray and shared timestamps, and shared with a device-side count below n into prefilled buffers"""
        def call(ts, per_ray, keep=None):
            def fn(d):
                if keep is None:
                    return op(d, I["rays_o"], I["rays_d"], ri, t0, t1, ts, per_ray)
                out = tuple(torch.full((n,) + shape, fill, device=DEV) for shape, fill in fills)
                return op(d, I["rays_o"], I["rays_d"], ri, t0, t1, ts, per_ray,
                          n_dev=torch.tensor([keep], device=DEV, dtype=torch.int64), out=out)
            return fn
        return [(f"{op.__name__} per-ray", call(I["ts_rays"], True)), (f"{op.__name__} shared", call(I["ts_one"], False)),
                (f"{op.__name__} shared n_dev", call(I["ts_one"], False, keep=n - 60))]

    calls = [("field_move", lambda d: ops.field_move(d, pos, t)),
             ("field_move_rays per-ray", rays(I["ts_rays"], True)),
             ("field_move_rays shared", rays(I["ts_one"], False)),
             ("field_move_rays per-ray n_dev", rays(I["ts_rays"], True, keep=n - 60)),
             ("field_move_rays shared n_dev", rays(I["ts_one"], False, keep=n - 60)),
             ("field_move_jacobian", lambda d: ops.field_move_jacobian(d, pos, t)),
             ("field_velocity", lambda d: ops.field_velocity(d, pos, t)),
             *rays_of(ops.field_velocity_rays, (((3,), 7.0), ((), 7.0), ((), True))),
             ("field_density_gradient", lambda d: ops.field_density_gradient(d, pos, t)),
             *rays_of(ops.field_density_gradient_rays, (((), 7.0), ((3,), 7.0), ((3,), 7.0), ((3,), 7.0))),
             ("field_rgb", lambda d: (ops.field_rgb(d, I["dirs"][:n], I["geo"][:n]),)),
             ("field_rgb_bcast", lambda d: (ops.field_rgb_bcast(d, I["dirs"][:N_DIRS], I["geo"][:n]),))]
    for K in (4, 32):
        for name in ("field_move_inverse", "field_move_inverse_newton"):
            calls.append((f"{name} K={K}", lambda d, e=getattr(ops, name), K=K: e(d, pos, t, max_iters=K, tol=1e-6)))
        for name in ("field_track", "field_track_newton"):
            calls.append((f"{name} K={K}", lambda d, e=getattr(ops, name), K=K: e(d, pos, times, max_iters=K, tol=1e-6)))
    return calls


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tm", [0, 2])
def test_outputs_do_not_depend_on_the_grid(tm, mode):
    """Every entry, on 1 and on 3 workgroups, n = 257 and 4 099: all outputs torch.equal to the default grid's."""
    from ced_nerf_amd import ops
    desc = _field(tm, mode)._descriptor()
    assert desc.max_workgroups == 0
    for n in SIZES:
        for name, fn in _calls(n):
            want = fn(desc)
            for w in WORKGROUPS:
                capped = ops._with_workgroups(desc, w)
                assert capped is not desc and capped.max_workgroups == w
                got = fn(capped)
                assert len(got) == len(want)
                for k, (g, x) in enumerate(zip(got, want)):
                    assert (g is None) == (x is None), (name, n, w, k)
                    if g is not None:
                        assert g.dtype == x.dtype and g.shape == x.shape, (name, n, w, k)
                        assert torch.equal(g, x), (name, n, w, k, int((g != x).sum()))
