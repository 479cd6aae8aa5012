"""GPU suite: time-sliced occupancy grids -- csrc/field_time_max.hip (ced_field_density_time_max), csrc/occgrid.hip
(ced_occ_time_slices) and what stands on them: nerfacc_api.TimeSlicedOccGrid, utils.grid_for in the renderers,
video.render_video through a sliced grid.

References: the composition the fused kernel replaces (a Python loop of query_density and torch.fmax); the numpy
restatement tests/occ_time_reference.py of the slices' definition; the CPU oracle for the render.  Every comparison is
exact (torch.equal / array_equal) except the render against the oracle, which is tests/test_gpu_parity.py's contract for
render_image_test: the sample count bit-exact, pixels within 1e-4 (and, f32, rgb and depth bit for bit).

Inputs of 1 - 3: those of tests/test_gpu_track.py -- rng 7, 4099 rows in +-1.6, aabb +-1.5, log2 table 15, hash_max_res
256, regime "trained", moving step 1/32."""
import functools

import numpy as np
import pytest
import torch

import occ_time_reference as R
from conftest import assert_bitexact
from test_gpu_density_gradient import TABLES
from test_gpu_track import AABB, DEV, FLAGS, MODES, SIZES, STEP, N, T, _field, _inputs, _params

pytestmark = pytest.mark.gpu

BINS = ((1, 1), (2, 3), (3, 5))
ALL_SIZES = tuple(sorted(set(SIZES) | {1, 15, 16, 17, 31, 32, 33}))


def _times(B, S):
    return T(R.probe_times(B, S))


def _composition(f, pos, times):
    """[B,n]: the running torch.fmax over s of query_density(pos, t[b, s]), started from zeros"""
    n = pos.shape[0]
    rows = []
    for b in range(times.shape[0]):
        m = torch.zeros((n,), device=pos.device)
        for s in range(times.shape[1]):
            m = torch.fmax(m, f.query_density(pos, times[b, s].expand(n).contiguous())["density"][:, 0])
        rows.append(m)
    return torch.stack(rows)


# ---- 1. the maxima are the composition's, bit for bit ---------------------------------------------------------------------
def _check_time_max(f, what):
    from ced_nerf_amd import ops
    pos, _ = _inputs()
    d = f._descriptor()
    for B, S in BINS:
        times = _times(B, S)
        want = _composition(f, pos, times)
        full = ops.field_density_time_max(d, pos, times)
        assert full.shape == (B, len(pos)) and full.dtype == torch.float32
        assert torch.equal(full, want), (what, B, S, int((full != want).sum()))
        for n in ALL_SIZES:                                              # a row does not depend on n
            got = ops.field_density_time_max(d, pos[:n].contiguous(), times)
            assert got.shape == (B, n) and torch.equal(got, full[:, :n]), (what, B, S, n)
        for b in range(B):                                               # outside the box at every probe: 0
            sel = torch.stack([f.query_move(pos, times[b, s].expand(len(pos)).contiguous(), return_normalized=True)[3]
                               for s in range(S)]).any(0)
            assert 0.1 < 1.0 - float(sel.float().mean()) < 0.25 and not bool(full[b][~sel].any()) and bool(full[b][sel].any())
    out = torch.full((3, 33), 7.0, device=DEV)
    assert ops.field_density_time_max(d, pos[:33].contiguous(), _times(3, 5), out=out) is out and torch.equal(out, full[:, :33])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("div,tm", FLAGS)
def test_time_max_is_the_composition_bit_for_bit(div, tm, mode):
    """field_density_time_max(pos, t [B,S])[b] == the running torch.fmax over s of query_density(pos, t[b, s]) started from
    zeros, with torch.equal, for (B, S) in (1,1), (2,3), (3,5); a row's result is the same at every n (0, 1, 15 .. 17,
    31 .. 33, 257, 4099: one row, around one and two wave tiles, several workgroups with a ragged tail); n = 0 gives an
    empty [B, 0]; rows outside the box are 0"""
    _check_time_max(_field(div, tm, mode), (div, tm, mode))


@pytest.mark.parametrize("mode,table", TABLES)
def test_time_max_is_the_composition_on_the_other_tables(mode, table):
    """fp16 and temporal tables: the f16x2 blob's K = 32 placements and its pair form, the temporal key-frame per iteration,
    one tile per wave on the fp32 temporal table"""
    _check_time_max(_field(True, 0, mode, STEP, table), (mode, table))


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
def test_time_max_ignores_nan_and_keeps_inf(mode):
    """NaN positions, and occ_time_reference.nan_inf_params' table entries of 3e38 (the densities are inf, NaN -- fp32 chain
    only --, 0 and exp(-1), changing from probe to probe): the result is torch.fmax's -- a NaN density never enters the
    maximum, an inf does.  CPU oracle, these 257 rows at t = 0 / 0.5: f32 111 / 90 NaN, 57 / 25 inf; f16x2 no NaN, 124 / 55 inf"""
    from ced_nerf_amd import ops
    from ced_nerf_amd.model import DNGPradianceField
    f = DNGPradianceField.from_params(R.nan_inf_params(), DEV, mlp_precision=mode).eval()
    pos = _inputs()[0][:257].clone()
    pos[5] = float("nan")
    pos[40, 1] = float("nan")
    times = _times(2, 3)
    want = _composition(f, pos, times)
    got = ops.field_density_time_max(f._descriptor(), pos, times)
    assert torch.equal(got, want), int((got != want).sum())
    assert not bool(torch.isnan(got).any()) and bool(torch.isinf(got).any()) and bool((got == 0).any())
    assert not bool(got[:, 5].any()) and not bool(got[:, 40].any())
    single = torch.stack([f.query_density(pos, times[0, s].expand(257).contiguous())["density"][:, 0] for s in range(3)])
    if mode == "f32":
        nan = torch.isnan(single)
        assert bool(nan.any()), "the inputs must produce NaN densities for the test to mean anything"
        mixed = nan.any(0) & ~nan.all(0)                                 # NaN at one probe, a number at another
        assert bool(mixed.any()) and torch.equal(got[0][nan.all(0)], torch.zeros_like(got[0][nan.all(0)]))


def test_time_max_refuses_bad_shapes():
    from ced_nerf_amd import ops
    d = _field(True, 2, "f32")._descriptor()
    pos = _inputs()[0][:8].contiguous()
    for bad in (torch.zeros((0, 3), device=DEV), torch.zeros((2, 65), device=DEV), torch.zeros((257, 1), device=DEV),
                torch.zeros((6,), device=DEV)):
        with pytest.raises(ValueError):
            ops.field_density_time_max(d, pos, bad)
    with pytest.raises(ValueError):
        ops.field_density_time_max(d, pos.reshape(-1), _times(1, 1))
    with pytest.raises(ValueError):
        ops.field_density_time_max(d, pos, _times(2, 3), out=torch.zeros((3, 8), device=DEV))


# ---- 2. the slices are the definition's -----------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [4, 8])
@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("B", [1, 3])
def test_slices_equal_the_numpy_restatement(res, levels, B):
    """occ_time_slices == tests/occ_time_reference.time_slices for dilate 0 / 1, with and without a union, on candidates
    that are a strict subset of the cells and maxima that include values at exactly thre / step (not a hit), one ulp above
    (a hit), NaN and inf; the same slices when the rows are handed over in two calls"""
    from ced_nerf_amd import ops
    rng = np.random.default_rng(res * 100 + levels * 10 + B)
    cells = levels * res ** 3
    ids = np.sort(rng.choice(cells, size=cells * 2 // 3, replace=False)).astype(np.int64)
    step, thre = 0.25, 0.5                                               # thre / step = 2 exactly
    mx = rng.uniform(0.0, 2.2, size=(B, len(ids))).astype(np.float32)    # one in eleven is a hit
    special = np.array([2.0, np.nextafter(np.float32(2.0), np.float32(3.0)), np.nan, np.inf, 0.0], np.float32)
    mx[:, : len(ids) // 4] = np.resize(special, (B, len(ids) // 4))
    mx = mx[:, rng.permutation(len(ids))]
    union = rng.uniform(size=(levels, res, res, res)) < 0.7
    for dilate in (0, 1):
        for uni in (None, union):
            want = R.time_slices(ids, mx, step, thre, levels, res, uni, dilate)
            got = ops.occ_time_slices(T(ids), T(mx), step, thre, levels, res, None if uni is None else T(uni), dilate)
            assert got.dtype == torch.bool and got.shape == (B, levels, res, res, res)
            assert np.array_equal(N(got), want), (dilate, uni is not None, int((N(got) != want).sum()))
            assert 0 < int(want.sum()) < want.size
            ws = ops.occ_time_slices_workspace(B, levels, res, DEV)
            half = len(ids) // 2
            assert ops.occ_time_slices(T(ids[:half]), T(mx[:, :half]), step, thre, levels, res, None if uni is None else T(uni),
                                       dilate, workspace=ws, finish=False) is None
            two = ops.occ_time_slices(T(ids[half:]), T(mx[:, half:]), step, thre, levels, res, None if uni is None else T(uni),
                                      dilate, workspace=ws)
            assert torch.equal(two, got)
    with pytest.raises(ValueError):
        ops.occ_time_slices(T(ids), T(mx), step, thre, levels, res, None, 2)
    with pytest.raises(ValueError):
        ops.occ_time_slices(T(ids), T(mx[:, :-1]), step, thre, levels, res)
    with pytest.raises(ValueError):
        ops.occ_time_slices(T(ids), T(mx), step, thre, levels, res, T(union[:, :-1]))
    with pytest.raises(RuntimeError, match="workspace too small"):
        ops.occ_time_slices(T(ids), T(mx), step, thre, levels, res, workspace=torch.zeros((B * cells - 1,), device=DEV, dtype=torch.uint8))


# ---- 3. from_field is the composition ---------------------------------------------------------------------------------------
def test_from_field_equals_the_composition():
    """R = 16, m = 2, B = 3, S = 3 on an estimator whose binaries mark 60 % of the cells: binaries_t == the numpy
    restatement on the expanded query_density maxima of the marked cells' centres; every slice is a subset of the
    estimator's grid; union() is the OR of the slices; chunk = 1000 gives the same slices as one chunk; without an
    estimator the candidates are all cells and thre = occ_thre"""
    from ced_nerf_amd.nerfacc_api import OccGridEstimator, TimeSlicedOccGrid
    res, levels, B, S, step = 16, 2, 3, 3, 1e-2
    f = _field(True, 2, "f32")
    rng = np.random.default_rng(11)
    binaries = rng.uniform(size=(levels, res, res, res)) < 0.6
    est = OccGridEstimator(AABB, res, levels).to(DEV)
    est.set_binaries(T(binaries))
    est.occs.copy_(T(rng.uniform(0.0, 4.0, size=est.occs.shape).astype(np.float32)))      # mean 2: thre = occ_thre
    occ_thre = 1e-4 * step                                               # sigma > 1e-4: about the median of this field's densities
    sliced = TimeSlicedOccGrid.from_field(f, est, n_bins=B, times_per_bin=S, render_step_size=step, occ_thre=occ_thre)
    assert sliced.binaries_t.shape == (B, levels, res, res, res) and sliced.binaries_t.dtype == torch.bool
    assert torch.equal(sliced.aabbs, est.aabbs)

    def reference(candidates_of, union, thre):
        ids, maxima = [], []
        for lvl in range(levels):
            cells = candidates_of(lvl)
            pos = T(R.cell_centres(cells, res, N(est.aabbs[lvl])))
            maxima.append(N(_composition(f, pos, _times(B, S))))
            ids.append(lvl * res ** 3 + cells)
        return R.time_slices(np.concatenate(ids), np.concatenate(maxima, axis=1), step, thre, levels, res, union, 1)

    want = reference(lambda lvl: np.nonzero(binaries[lvl].reshape(-1))[0], binaries, occ_thre)
    got = N(sliced.binaries_t)
    assert np.array_equal(got, want), int((got != want).sum())
    assert (want.reshape(B, -1).sum(1) > 0).all() and (want.reshape(B, -1).sum(1) < binaries.sum()).all()   # neither empty nor all
    assert not (got & ~binaries[None]).any()
    assert torch.equal(sliced.union().binaries, sliced.binaries_t.any(0)) and torch.equal(sliced.union().binaries, T(want.any(0)))
    assert torch.equal(sliced.occupied_fraction(), T((want.reshape(B, -1).sum(1) / want.any(0).sum()).astype(np.float32)))
    chunked = TimeSlicedOccGrid.from_field(f, est, n_bins=B, times_per_bin=S, render_step_size=step, occ_thre=occ_thre, chunk=1000)
    assert torch.equal(chunked.binaries_t, sliced.binaries_t)
    # thre follows the estimator's mean occupancy when that is the smaller one
    est.occs.mul_(occ_thre / 4.0)                                        # mean = occ_thre / 2
    low = TimeSlicedOccGrid.from_field(f, est, n_bins=B, times_per_bin=S, render_step_size=step, occ_thre=occ_thre)
    thre = float(torch.clamp(est.occs[est.occs >= 0].mean(), max=occ_thre))
    assert thre < occ_thre
    assert np.array_equal(N(low.binaries_t), reference(lambda lvl: np.nonzero(binaries[lvl].reshape(-1))[0], binaries, thre))
    # no estimator: all cells
    free = TimeSlicedOccGrid.from_field(f, roi_aabb=AABB, resolution=res, levels=levels, n_bins=B, times_per_bin=S,
                                        render_step_size=step, occ_thre=occ_thre, chunk=3000)
    assert np.array_equal(N(free.binaries_t), reference(lambda lvl: np.arange(res ** 3), None, occ_thre))


# ---- 4. a moving ball, end to end ---------------------------------------------------------------------------------------------
H = W = 64
BALL_RENDER = dict(near_plane=0.0, far_plane=1e10, render_step_size=5e-3, cone_angle=0.0, alpha_thre=0.0)


@functools.lru_cache(maxsize=None)
def _ball():
    from ced_nerf_amd import synthetic as S
    from ced_nerf_amd.model import DNGPradianceField
    from ced_nerf_amd.nerfacc_api import TimeSlicedOccGrid
    from ced_nerf_amd.utils import Rays
    params = R.ball_params()
    f = DNGPradianceField.from_params(params, DEV).eval()
    g = R.BALL_GRID
    sliced = TimeSlicedOccGrid.from_field(f, roi_aabb=R.BALL_AABB, resolution=g["resolution"], levels=g["levels"],
                                          n_bins=g["n_bins"], times_per_bin=g["times_per_bin"],
                                          render_step_size=g["render_step_size"], occ_thre=g["occ_thre"], dilate=g["dilate"])
    o, d = S.make_camera_rays(W, H, 0.69, S.look_at_c2w(4.0, 30.0, 30.0))
    return params, f, sliced, o, d, Rays(origins=T(o), viewdirs=T(d))


def test_moving_ball_slices_march_fewer_samples(oracle):
    """The hand-made field of occ_time_reference.ball_params (a ball of radius 0.4 that slides by -sin(pi t) along x), grid
    R = 32, m = 1, B = 8, S = 3, dilate 1, step 5e-3, candidates = all cells.
    Checked on the CPU with the oracle's density (tests/test_time_slices_cpu.py asserts it): the union holds 2200 cells,
    the slices 1456, 1388, 1244, 1040, 1040, 1244, 1388, 1456 -- 0.47 .. 0.66 of the union; the slice of t = 0.45 (bin 3)
    holds 1040 = 0.47 of it, within the 3/4 the test relies on.
    a. at_time(0.45).march yields, per ray, a subset of union().march's t_starts (64 x 64 rays), and strictly fewer
       samples in total;
    b. render_image_test through the sliced grid, through at_time(0.45) and through a plain estimator loaded with that
       slice's binaries are torch.equal in every output;
    c. that render is the oracle's on the same binaries: sample count bit-exact, pixels within 1e-4, rgb and depth bit for
       bit (test_gpu_parity.py's contract for render_image_test).
    Printed, not asserted: the pixel difference between the sliced and the union render."""
    from ced_nerf_amd.nerfacc_api import OccGridEstimator
    from ced_nerf_amd.utils import render_image_test
    params, f, sliced, o, d, rays = _ball()
    of = oracle.OracleField(params)
    want = R.ball_slices(lambda pos, t: of.forward(pos, t)["density"])
    got = N(sliced.binaries_t)
    assert np.array_equal(got, want), int((got != want).sum())
    union = sliced.union()
    n_union = int(union.binaries.sum())
    at = sliced.at_time(0.45)
    assert at is sliced.at_time(torch.tensor([[0.45]], device=DEV)) and torch.equal(at.binaries, sliced.binaries_t[3])
    assert 0 < int(at.binaries.sum()) <= 0.75 * n_union
    # a. the march
    O, Dd = rays.origins.reshape(-1, 3), rays.viewdirs.reshape(-1, 3)
    kw = dict(near_plane=0.0, far_plane=1e10, render_step_size=5e-3, cone_angle=0.0)
    s0, _, sri, _ = at.march(O, Dd, **kw)
    u0, _, uri, _ = union.march(O, Dd, **kw)
    assert 0 < s0.shape[0] < u0.shape[0]
    key = lambda ri, t0: set(zip(N(ri).tolist(), N(t0).view(np.uint32).tolist()))
    assert key(sri, s0) <= key(uri, u0)
    # b. three ways to the same render
    ts = T(np.array([[0.45]], np.float32))
    bk = torch.zeros(3, device=DEV)
    through = render_image_test(1024, f, sliced, rays, render_bkgd=bk, timestamps=ts, **BALL_RENDER)
    direct = render_image_test(1024, f, at, rays, render_bkgd=bk, timestamps=ts, **BALL_RENDER)
    plain_est = OccGridEstimator(R.BALL_AABB, 32, 1).to(DEV)
    plain_est.set_binaries(sliced.binaries_t[3])
    plain = render_image_test(1024, f, plain_est, rays, render_bkgd=bk, timestamps=ts, **BALL_RENDER)
    for a, b, c in zip(through[:3], direct[:3], plain[:3]):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert through[3] == direct[3] == plain[3] > 1000
    # c. the oracle on the same binaries
    oest = oracle.OracleEstimator(R.BALL_AABB, 32, 1, want[3])
    w_rgb, w_op, w_dp, w_total = oracle.render_image_test(1024, of, oest, o, d, timestamps=N(ts), render_bkgd=np.zeros(3, np.float32),
                                                          **BALL_RENDER)
    rgb, op, dp, total = through
    assert total == w_total
    for g_, w_ in ((rgb, w_rgb), (op, w_op), (dp, w_dp)):
        assert np.abs(N(g_) - w_).max() <= 1e-4
    assert_bitexact(N(rgb), w_rgb, "rgb (bit-exact)")
    assert_bitexact(N(dp), w_dp, "depth (bit-exact)")
    assert float(op.max()) > 0.9                                         # the ball is seen
    whole = render_image_test(1024, f, union, rays, render_bkgd=bk, timestamps=ts, **BALL_RENDER)
    diff = (whole[0] - rgb).abs()
    print(f"moving ball at t = 0.45: slice {int(at.binaries.sum())} of {n_union} cells; marched {s0.shape[0]} / {u0.shape[0]} samples; "
          f"rendered {total} / {whole[3]}; sliced against union render: max |rgb diff| = {float(diff.max()):.3e}, mean = "
          f"{float(diff.mean()):.3e}, max |opacity diff| = {float((whole[1] - op).abs().max()):.3e}")


# ---- 5. video and frames -----------------------------------------------------------------------------------------------------
def test_video_and_frames_resolve_their_range(monkeypatch):
    """render_video with the sliced grid over 6 frames, t = i / 5: with frames_per_call 1 and 3 every frame's pixels are
    render_image_test's through at_time of that call's range of times; render_frames_test resolves the range of its frames;
    the post passes resolve per frame; with a plain estimator render_video returns what it returns with grid_for replaced
    by the identity"""
    import ced_nerf_amd.utils as U
    from ced_nerf_amd.video import render_video
    _, f, sliced, _, _, rays = _ball()
    n = 6
    times = [torch.tensor([[i / 5.0]], device=DEV) for i in range(n)]
    bk = torch.zeros(3, device=DEV)
    rk = dict(BALL_RENDER, render_bkgd=bk)
    for per_call in (1, 3):
        frames = render_video(f, sliced, lambda i: rays, lambda i: times[i], n, max_samples=256, render_kwargs=rk,
                              keep_float=True, frames_per_call=per_call)
        torch.cuda.synchronize()
        grids = set()
        for i, fr in enumerate(frames):
            first = (i // per_call) * per_call
            grid = sliced.at_time([k / 5.0 for k in range(first, min(first + per_call, n))])
            grids.add(id(grid))
            rgb, op, dp, total = U.render_image_test(256, f, grid, rays, timestamps=times[i], **rk)
            assert torch.equal(fr["rgb_f32"], rgb) and torch.equal(fr["depth_f32"], dp) and torch.equal(fr["opacity_f32"], op)
            if per_call == 1:
                assert fr["n_samples"] == total
        assert len(grids) == (6 if per_call == 1 else 2)                 # bins 0, 1, 3, 4, 6, 7; ranges 0 .. 3 and 4 .. 7
    stack = U.Rays(origins=torch.stack([rays.origins] * 3), viewdirs=torch.stack([rays.viewdirs] * 3))
    ts3 = torch.tensor([0.2, 0.4, 0.6], device=DEV)
    a = U.render_frames_test(256, f, sliced, stack, timestamps=ts3, **rk)
    b = U.render_frames_test(256, f, sliced.at_time(ts3), stack, timestamps=ts3, **rk)
    assert sliced.bin_range(ts3) == (1, 4) and all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and list(a[3]) == list(b[3])
    kw = {k: v for k, v in BALL_RENDER.items()}
    m_sliced = U.render_motion(f, sliced, rays, timestamps=times[2], **kw)
    m_direct = U.render_motion(f, sliced.at_time(0.4), rays, timestamps=times[2], **kw)
    assert torch.equal(m_sliced[0], m_direct[0]) and m_sliced[2] == m_direct[2] and bool(m_sliced[0].any())
    # a plain estimator goes through untouched
    plain = sliced.union()
    assert U.grid_for(plain, times[0]) is plain
    with_hook = render_video(f, plain, lambda i: rays, lambda i: times[i], 3, max_samples=256, render_kwargs=rk, keep_float=True,
                             motion=True)
    monkeypatch.setattr(U, "grid_for", lambda estimator, timestamps: estimator)
    without = render_video(f, plain, lambda i: rays, lambda i: times[i], 3, max_samples=256, render_kwargs=rk, keep_float=True,
                           motion=True)
    for x, y in zip(with_hook, without):
        assert set(x) == set(y)
        for k in x:
            assert (x[k] == y[k]) if k == "n_samples" else torch.equal(x[k], y[k]), k
