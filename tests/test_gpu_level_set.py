"""GPU suite: the density's level set along rays -- csrc/surface.hip (ced_surface_first_crossing), csrc/field_level_set.hip
(ced_field_level_set) and what stands on them: DNGPradianceField.query_level_set, utils.render_surface,
video.render_video(surface=...), export.refine_mesh / extract_mesh(refine=True).

The reference of the bit-identity tests is the composition the fused kernel replaces: include/cednerf_hip.h's lines in
torch float32 around `query_density` (one launch per round).  The reference of the accuracy test is the float64 model of
tests/level_set64.py (tests/density64.py behind tests/warp64.py's move).

Fields: tests/test_gpu_track.py's (synthetic "trained", aabb [-1.5, 1.5]^3, moving step 1/32).  Rays: default_rng(11),
origins on the sphere of radius 4, aimed at points uniform in +-0.8; the first 257 are "the rays", marched with step 2e-2
through an all-occupied 128^3 one-level grid over the box."""
import functools
import math

import numpy as np
import pytest
import torch

import level_set64 as LS
from test_gpu_density_gradient import TABLES
from test_gpu_track import AABB, DEV, FLAGS, MODES, SIZES, STEP, N, T, _field, _params

pytestmark = pytest.mark.gpu

N_RAYS = 257
RENDER_STEP = 2e-2
T_FRAME = 0.37
KEYS = ("t", "x", "sigma", "width", "status", "evals")
POSITION_SLACK = 2e-6                                               # four float32 spacings at t in [4, 8)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rays_np():
    rng = np.random.default_rng(11)
    n = max(SIZES)
    v = rng.normal(size=(n, 3))
    o = 4.0 * v / np.linalg.norm(v, axis=-1, keepdims=True)
    aim = rng.uniform(-0.8, 0.8, size=(n, 3))
    d = aim - o
    dist = np.linalg.norm(d, axis=-1, keepdims=True)
    t = rng.uniform(0.0, 1.0, size=(n,))
    return o.astype(np.float32), (d / dist).astype(np.float32), dist[:, 0].astype(np.float32), t.astype(np.float32)


_BRACKETS = {}


def _brackets(f):
    """(o, d, lo, hi, t) on the device.  Per ray the densest of eight probes between the box's faces (query_density, thresh
    or no thresh) is the point `dense`; four kinds of bracket by row % 4: from in front of the box to `dense` (a crossing
    wherever `dense` reaches the threshold), from `dense` to behind the box (starts inside wherever it does), wholly outside
    the box, and a short one around the aimed point."""
    if id(f) in _BRACKETS:
        return _BRACKETS[id(f)]
    o, d, dist, t = _rays_np()
    with np.errstate(divide="ignore"):
        a, b = (-1.5 - o) / d, (1.5 - o) / d
    near, far = np.minimum(a, b).max(-1), np.maximum(a, b).min(-1)
    assert (near < far).all() and (near > 1.0).all()                    # every ray meets the box, from outside
    probes = np.stack([near + (far - near) * (j / 9.0) for j in range(1, 9)], -1).astype(np.float32)
    sig = torch.stack([f.query_density(T(o) + T(d) * T(probes[:, j])[:, None], T(t))["density"][:, 0] for j in range(8)], -1)
    dense = probes[np.arange(len(dist)), N(sig.argmax(-1))]
    kind = np.arange(len(dist)) % 4
    lo = np.select([kind == 0, kind == 1, kind == 2], [near - 0.3, dense, np.full_like(near, 0.1)], dist - 0.05)
    hi = np.select([kind == 0, kind == 1, kind == 2], [dense, far + 0.2, near - 0.1], dist + 0.05)
    _BRACKETS[id(f)] = T(o), T(d), T(lo.astype(np.float32)), T(hi.astype(np.float32)), T(t)
    return _BRACKETS[id(f)]


@functools.lru_cache(maxsize=None)
def _grid():
    from ced_nerf_amd.nerfacc_api import OccGridEstimator
    est = OccGridEstimator(AABB, 128, 1).to(DEV)
    est.set_binaries(torch.ones((1, 128, 128, 128), dtype=torch.bool))
    return est


def _frame_rays(shape=None):
    from ced_nerf_amd.utils import Rays
    o, d, _, _ = _rays_np()
    o, d = T(o[:N_RAYS]), T(d[:N_RAYS])
    if shape is not None:
        o, d = o[:shape[0] * shape[1]].reshape(*shape, 3), d[:shape[0] * shape[1]].reshape(*shape, 3)
    return Rays(origins=o, viewdirs=d)


def _frame_time():
    return torch.tensor([[T_FRAME]], device=DEV)


# ---- 1. kernel A --------------------------------------------------------------------------------------------------------------
def _hand_made_rays():
    """rays of 0, 1, 3, 4, 5, 9 and 64 samples (full batches of four and remainders), each length with a crossing at the
    first, a middle and the last sample, none, a NaN before the crossing, a gap before the crossing sample and a gap
    elsewhere; sigma 2 / 0.5 around the threshold 1"""
    t0s, t1s, sgs, packed = [], [], [], []
    at = 0
    for rep in range(2):
        for L in (0, 1, 3, 4, 5, 9, 64):
            for variant in ("first", "middle", "last", "none", "nan", "gap_before", "gap_elsewhere", "at_threshold"):
                edges = (np.float32(0.25 * rep + 0.5) + np.float32(0.1) * np.arange(L + 1, dtype=np.float32)).astype(np.float32)
                t0, t1 = edges[:-1].copy(), edges[1:].copy()
                sg = np.full(L, 0.5, np.float32)
                k = {"first": 0, "middle": L // 2, "last": L - 1, "none": -1}.get(variant, L - 1 - L // 3)
                if L and k >= 0:
                    sg[k:] = 2.0
                    sg[k + 1:: 2] = 0.25                                 # below again behind the crossing: the first stands
                if L and variant == "nan":
                    sg[:k] = np.nan
                if L and variant == "at_threshold":
                    sg[k] = 1.0
                    sg[:k] = np.nextafter(np.float32(1.0), np.float32(0.0))
                gap_at = k if variant == "gap_before" else max(k - 1, 0)
                if L and variant.startswith("gap") and gap_at > 0:
                    t0[gap_at:] += np.float32(0.05)
                    t1[gap_at:] += np.float32(0.05)
                t0s.append(t0); t1s.append(t1); sgs.append(sg)
                packed.append((at, L))
                at += L
    return np.asarray(packed, np.int64), np.concatenate(t0s), np.concatenate(t1s), np.concatenate(sgs)


def test_first_crossing_equals_its_definition():
    """ced_surface_first_crossing == level_set64.first_crossing with torch.equal on 112 hand-made rays and on their first
    1, 63, 64 and 65 (one wave, a wave +- 1); 0 rays; and rays whose samples are all empty."""
    from ced_nerf_amd import ops
    packed, t0, t1, sg = _hand_made_rays()
    want = LS.first_crossing(packed, t0, t1, sg, 1.0)
    assert len(packed) == 112 and (want[0] >= 0).sum() > 60 and (want[0] < 0).sum() > 20
    in_ray = want[0] > packed[:, 0]                                             # a crossing behind the ray's first sample
    mids = (t0 + t1) / np.float32(2.0)
    assert (want[1][in_ray] == t0[want[0][in_ray]]).any() and (want[1][in_ray] == mids[want[0][in_ray] - 1]).any()
    dev = [T(a) for a in (packed, t0, t1, sg)]
    for n in (len(packed), 1, 63, 64, 65, 0):
        got = ops.surface_first_crossing(dev[0][:n].contiguous(), dev[1], dev[2], dev[3], 1.0)
        for g, w, name in zip(got, want, ("k", "lo", "hi")):
            assert g.dtype == T(w).dtype and g.shape == (n,) and torch.equal(g, T(w[:n])), (n, name)
    empty = torch.zeros((5, 2), device=DEV, dtype=torch.int64)
    none = torch.zeros((0,), device=DEV)
    k, lo, hi = ops.surface_first_crossing(empty, none, none, none, 1.0)
    assert k.tolist() == [-1] * 5 and lo.tolist() == [0.0] * 5 and hi.tolist() == [0.0] * 5
    # another threshold: every 2.0 qualifies, no 0.5 does
    got = ops.surface_first_crossing(dev[0], dev[1], dev[2], dev[3], 2.0)
    for g, w in zip(got, LS.first_crossing(packed, t0, t1, sg, 2.0)):
        assert torch.equal(g, T(w))


# ---- 2. kernel B against the unfused loop ---------------------------------------------------------------------------------------
def _unfused(f, o, d, lo, hi, t, thresh, K, tol):
    """include/cednerf_hip.h's lines on today's pieces: one query_density launch per round, the fp32 lines and the per-row
    freeze in torch.  The position is a separate multiply and add."""
    dens = lambda s: f.query_density(o + d * s[:, None], t)["density"][:, 0]
    lo, hi = lo.clone(), hi.clone()
    tol = torch.tensor(tol, device=o.device, dtype=torch.float32)
    s_lo, s_hi = dens(lo), dens(hi)
    one, two, zero = (torch.full_like(lo, v, dtype=torch.int32) for v in (1, 2, 0))
    status = torch.where(s_lo >= thresh, one, torch.where(~(s_hi >= thresh), two, zero))
    evals = two.clone()
    active = status == 0
    for _ in range(K):
        width = hi - lo
        m = (lo + hi) / 2
        active = active & ~((width <= tol) | (m == lo) | (m == hi))
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


def _assert_same(got, want, what):
    for g, w, name in zip(got, want, KEYS):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        assert torch.equal(g, w), (what, name, int((g != w).sum()))


def _check_is_the_unfused_loop(f, what):
    from ced_nerf_amd import ops
    o, d, lo, hi, t = _brackets(f)
    desc = f._descriptor()
    for thresh, K, tol in ((1.0, 32, 0.0), (1.0, 0, 0.0), (10.0, 5, 0.0), (1.0, 32, 1e-4)):
        want = _unfused(f, o, d, lo, hi, t, thresh, K, tol)
        for n in SIZES:
            got = f.query_level_set(o[:n], d[:n], lo[:n], hi[:n], t[:n], thresh, K, tol)
            assert got[0].shape == (n,) and got[1].shape == (n, 3) and got[4].dtype == torch.int32
            _assert_same(got, tuple(w[:n] for w in want), (what, thresh, K, tol, n))
        st, ev = want[4], want[5]
        if K == 0:                                                           # the endpoint verdicts alone
            assert bool((ev == 2).all()) and torch.equal(want[0], torch.where(st == 1, lo, hi))
        if (thresh, K, tol) == (1.0, 32, 0.0):
            full = want
            counts = [int((st == s).sum()) for s in (0, 1, 2)]
            assert min(counts) >= 10, counts                                  # crossings, starts inside, never reached
            assert bool((st[2::4] == 2).all()) and bool((want[2][2::4] == 0).all())          # wholly outside the box
            assert len(torch.unique(ev[st == 0])) >= 3, "rows must stop at different rounds for the freeze to be exercised"
        if tol > 0:                                                           # stops early
            cross = st == 0
            assert bool((ev[cross] < full[5][cross]).all()) and bool((want[3][cross] <= tol).all())
            assert bool((want[3][cross] > full[3][cross]).all())
    # one time for all rows
    n = 257
    t1 = t[5:6].contiguous()
    want = _unfused(f, o[:n], d[:n], lo[:n], hi[:n], t1.expand(n).contiguous(), 1.0, 32, 0.0)
    _assert_same(ops.field_level_set(desc, o[:n].contiguous(), d[:n].contiguous(), lo[:n].contiguous(), hi[:n].contiguous(), t1,
                                     1.0, 32, 0.0), want, (what, "t_per_row = 0"))
    _assert_same(f.query_level_set(o[:n], d[:n], lo[:n], hi[:n], float(t1), 1.0, 32, 0.0), want, (what, "a float time"))
    # each output alone
    args = (desc, o[:n].contiguous(), d[:n].contiguous(), lo[:n].contiguous(), hi[:n].contiguous(), t[:n].contiguous(), 1.0, 32, 0.0)
    for i, name in enumerate(KEYS):
        only = ops.field_level_set(*args, want=tuple(j == i for j in range(6)))
        assert all((only[j] is None) == (j != i) for j in range(6)) and torch.equal(only[i], full[i][:n]), (what, name)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("div,tm", FLAGS)
def test_level_set_is_the_unfused_loop_bit_for_bit(div, tm, mode):
    """query_level_set == the torch loop around query_density: t, x, sigma, width, status and evals with torch.equal, at
    thresholds 1 and 10, max_iters 32 / 0 / 5, tol 0 and 1e-4, for every n of SIZES (rows do not depend on n), with one
    time per row and one for all, and each output requested alone."""
    _check_is_the_unfused_loop(_field(div, tm, mode), (div, tm, mode))


@pytest.mark.parametrize("mode,table", TABLES)
def test_level_set_is_the_unfused_loop_on_the_other_tables(mode, table):
    """fp16 and temporal tables: the table's kind selects the blob's layout, the gather and the tiles per wave."""
    _check_is_the_unfused_loop(_field(True, 2 if table == "temporal" else 0, mode, STEP, table), (mode, table))


def test_python_checks_on_the_device():
    f = _field(True, 2, "f32")
    o, d, lo, hi, t = (a[:8].contiguous() for a in _brackets(f))
    for kw in (dict(sigma_thresh=0.0), dict(max_iters=65), dict(max_iters=-1), dict(tol=-1.0), dict(tol=float("nan"))):
        with pytest.raises(ValueError):
            f.query_level_set(o, d, lo, hi, t, **kw)
    with pytest.raises(ValueError):
        f.query_level_set(o, d, lo[:4], hi, t)
    with pytest.raises(NotImplementedError):
        f.query_level_set(o.cpu(), d, lo, hi, t)
    assert all(a.shape[0] == 0 for a in f.query_level_set(o[:0], d[:0], lo[:0], hi[:0], t[:0]))


# ---- 3. the invariant, by re-evaluation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("div,tm", FLAGS)
def test_crossing_rows_hold_the_invariant(div, tm, mode):
    """On status-0 rows query_density(x) has sigma's bits and is >= thresh, query_density one `width` back is < thresh, and
    at tol = 0 (64 rounds) width is at most one float32 spacing at t."""
    f = _field(div, tm, mode)
    o, d, lo, hi, t = _brackets(f)
    for thresh in (1.0, 10.0):
        tt, x, sigma, width, status, evals = f.query_level_set(o, d, lo, hi, t, thresh, 64, 0.0)
        c = status == 0
        assert int(c.sum()) >= 50
        dens = lambda p: f.query_density(p, t)["density"][:, 0]
        assert torch.equal(dens(x)[c], sigma[c]) and bool((sigma[c] >= thresh).all())
        back = dens(o + d * (tt - width)[:, None])
        assert bool((back[c] < thresh).all()), int((~(back[c] < thresh)).sum())
        spacing = T(np.spacing(np.abs(N(tt))))
        assert bool((width[c] > 0).all()) and bool((width[c] <= spacing[c]).all())
        assert torch.equal(x, o + d * tt[:, None])


# ---- 4. against float64 ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _marched():
    """the frame's samples: (t0, t1, ray index, packed) as numpy, marched once"""
    r = _frame_rays()
    t0, t1, ri, packed = _grid().march(r.origins, r.viewdirs, render_step_size=RENDER_STEP)
    return N(t0), N(t1), N(ri), N(packed)


def _mid_points():
    o, d, _, _ = _rays_np()
    t0, t1, ri, _ = _marched()
    mid = ((t0 + t1) / np.float32(2.0)).astype(np.float64)
    return o[ri].astype(np.float64) + d[ri].astype(np.float64) * mid[:, None]


@functools.lru_cache(maxsize=None)
def _raw_at_mids(div, tm, mode):
    p = _mid_points()
    return LS.raw_model(_params(div, tm), p, np.full(len(p), np.float32(T_FRAME), np.float64), mode)


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
@pytest.mark.parametrize("div,tm", FLAGS)
def test_surface_is_the_float64_models(div, tm, mode):
    """At thresholds 1 and 10: k64 = each ray's first marched midpoint at which the float64 model's log-density reaches
    ln(thresh).  Rays on which a midpoint up to k64 lies within `margin` of ln(thresh) are left out (at most 5 %); on the
    rest render_surface's candidate sample is k64 exactly, and the float64 model at the returned t and at t - width lies on
    the proper side of ln(thresh) within `margin`.  margin = 4 x the largest difference between the mode-rounded model
    (D.BASE_MODES, warp64.rounder) and the float64 model at these midpoints, computed on the CPU, never from the kernel.
    Measured (the margin is the CPU's; the rest on an MI355X), rays of default_rng(11):
      margin: f32 8.07e-4 / 1.16e-3 (FLAGS[0] / FLAGS[1]), f16x2 1.30e-3 / 1.25e-3;
      rays with a crossing: threshold 1: 100 % / 98.4 %, threshold 10: 100 % / 81.7 %; rays left out: 0 % everywhere;
      float64 log-density - ln(thresh): >= 0 at t on every hit; one `width` behind at most -3.8e-5 .. -2.0e-4, i.e. below.
    With FLAGS[0] most first crossings are the box's faces, where sigma jumps from 0 to its value (up to e^6.8 there)."""
    from ced_nerf_amd.utils import render_surface
    params, f = _params(div, tm), _field(div, tm, mode)
    o, d, _, _ = _rays_np()
    t0, t1, ri, packed = _marched()
    raw = _raw_at_mids(div, tm, None)
    rounded = _raw_at_mids(div, tm, mode)
    inside = np.isfinite(raw) & np.isfinite(rounded)
    assert np.array_equal(np.isfinite(raw), np.isfinite(rounded)) and inside.mean() > 0.5
    margin = 4.0 * float(np.abs(rounded[inside] - raw[inside]).max())
    for thresh in (1.0, 10.0):
        level = math.log(thresh)
        k64 = np.full(N_RAYS, -1, np.int64)
        kept = np.ones(N_RAYS, bool)
        for r in range(N_RAYS):
            s0, cnt = int(packed[r, 0]), int(packed[r, 1])
            above = np.flatnonzero(raw[s0:s0 + cnt] >= level)
            k64[r] = above[0] if len(above) else -1
            upto = raw[s0:s0 + (k64[r] + 1 if k64[r] >= 0 else cnt)]
            kept[r] = not (np.abs(upto - level) <= margin).any()
        out = render_surface(f, _grid(), _frame_rays(), sigma_thresh=thresh, render_step_size=RENDER_STEP, timestamps=_frame_time(),
                             max_iters=64, colors=False, normals=False)
        sample, status = N(out["sample"])[:, 0], N(out["status"])[:, 0]
        t, w = N(out["depth"])[:, 0].astype(np.float64), N(out["width"])[:, 0].astype(np.float64)
        left_out = 1.0 - kept.mean()
        crossing = (k64 >= 0).mean()
        tf = np.full(N_RAYS, np.float32(T_FRAME), np.float64)
        o64, d64 = o[:N_RAYS].astype(np.float64), d[:N_RAYS].astype(np.float64)
        # The device evaluates the density at float32 points, each axis up to one spacing (4.8e-7 at |x| <= 4) from the real
        # point, and sigma jumps from 0 to its value at the box's faces, where many rays have their first crossing: at a
        # jump the float64 point of t - width may lie on the other side of it.  The model is therefore also taken
        # POSITION_SLACK further along the ray on either side, and the side's better value counts.
        at = lambda s: LS.raw64(params, o64 + d64 * s[:, None], tf)
        at_t = np.maximum(at(t), at(t + POSITION_SLACK))
        behind = np.minimum(at(t - w), at(t - w - POSITION_SLACK))
        hit0, hit = kept & (status == 0), kept & ((status == 0) | (status == 1))
        print(f"surface [{mode} div={div} tm={tm} thresh={thresh:g}]: margin {margin:.3e}; {100 * crossing:.1f} % of the rays cross, "
              f"{100 * left_out:.1f} % left out; status 0 / 1 / 2 / -1: {[int((status == s).sum()) for s in (0, 1, 2, -1)]}; "
              f"float64 log-density - ln(thresh) at t: {np.min(at_t[hit] - level, initial=0):+.3e} .. "
              f"{np.max(at_t[hit0] - level, initial=0):+.3e}, at t - width: max {np.max(behind[hit0] - level, initial=-np.inf):+.3e}")
        assert left_out <= 0.05, left_out
        assert np.array_equal(sample[kept], k64[kept]), int((sample[kept] != k64[kept]).sum())
        assert (status[kept & (k64 < 0)] == -1).all() and (status[kept & (k64 >= 0)] != -1).all()
        assert (status[kept] != 2).all()
        assert (at_t[hit] >= level - margin).all() and (behind[hit0] <= level + margin).all()
        assert hit.sum() > N_RAYS // 4


# ---- 5. render_surface ------------------------------------------------------------------------------------------------------------
def _assert_same_maps(a, b, what):
    assert set(a) == set(b)
    for k in a:
        same = torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else a[k] == b[k]
        assert same, (what, k)


def test_render_surface(monkeypatch):
    """Shapes for [H,W,3] and flat rays; misses hold zeros and hit = False; depth * d + o == position in float32; normal ==
    query_normals(position); rgb == the field's colour there; the background behind misses; two chunk sizes, and a
    TimeSlicedOccGrid, give the same maps; render_video(surface=...) returns them."""
    from ced_nerf_amd import utils
    from ced_nerf_amd.nerfacc_api import TimeSlicedOccGrid
    from ced_nerf_amd.video import render_video
    f = _field(True, 2, "f32")
    ts = _frame_time()
    kw = dict(sigma_thresh=10.0, render_step_size=RENDER_STEP, timestamps=ts)
    flat = utils.render_surface(f, _grid(), _frame_rays(), **kw)
    rays = _frame_rays()
    o, d = rays.origins, rays.viewdirs
    shapes = dict(hit=(1, torch.bool), depth=(1, torch.float32), position=(3, torch.float32), normal=(3, torch.float32),
                  rgb=(3, torch.float32), sigma=(1, torch.float32), width=(1, torch.float32), status=(1, torch.int32),
                  sample=(1, torch.int64))
    for k, (c, dt) in shapes.items():
        assert flat[k].shape == (N_RAYS, c) and flat[k].dtype == dt, k
    assert isinstance(flat["n_samples"], int) and flat["n_samples"] == len(_marched()[0]) and isinstance(flat["n_evals"], int)
    hit, status = flat["hit"][:, 0], flat["status"][:, 0]
    assert torch.equal(hit, (status == 0) | (status == 1)) and 20 < int(hit.sum()) < N_RAYS and int((status == -1).sum()) > 0
    assert flat["n_evals"] > 2 * int((status >= 0).sum())
    for k in ("depth", "position", "normal", "rgb"):
        assert bool((flat[k][~hit] == 0).all()), k
    assert bool((flat["sigma"][status == -1] == 0).all()) and bool((flat["sigma"][hit] >= 10.0).all())
    assert torch.equal((flat["depth"] * d + o)[hit], flat["position"][hit])
    th = ts.reshape(-1).expand(int(hit.sum())).contiguous()
    pos = flat["position"][hit].contiguous()
    assert torch.equal(flat["normal"][hit], f.query_normals(pos, th)[0])
    assert torch.equal(flat["rgb"][hit], f(pos, th, d[hit].contiguous())[0])
    assert torch.equal(flat["sigma"][hit, 0], f.query_density(pos, th)["density"][:, 0])
    # a background, and the maps that are not asked for
    bk = torch.tensor([0.25, 0.5, 0.75], device=DEV)
    with_bk = utils.render_surface(f, _grid(), rays, render_bkgd=bk, **kw)
    assert bool((with_bk["rgb"][~hit] == bk).all()) and torch.equal(with_bk["rgb"][hit], flat["rgb"][hit])
    bare = utils.render_surface(f, _grid(), rays, normals=False, colors=False, **kw)
    assert not bool(bare["normal"].any()) and not bool(bare["rgb"].any()) and torch.equal(bare["depth"], flat["depth"])
    # an image
    image = utils.render_surface(f, _grid(), _frame_rays((16, 16)), **kw)
    for k, (c, _) in shapes.items():
        assert image[k].shape == (16, 16, c) and torch.equal(image[k].reshape(256, c), flat[k][:256]), k
    # passes of 64 and of 100 rays
    monkeypatch.setattr(utils, "_EVAL_PASS_RAYS", 1)
    for chunk in (64, 100):
        _assert_same_maps(utils.render_surface(f, _grid(), rays, test_chunk_size=chunk, **kw), flat, chunk)
    monkeypatch.undo()
    # a sliced grid whose every slice is full
    sliced = TimeSlicedOccGrid(AABB, 128, 1, n_bins=2, device=DEV)
    sliced.set_slices(torch.ones_like(sliced.binaries_t))
    _assert_same_maps(utils.render_surface(f, sliced, rays, **kw), flat, "sliced")
    # training fields and missing times are refused
    with pytest.raises(NotImplementedError):
        utils.render_surface(f, _grid(), rays, sigma_thresh=10.0)
    with pytest.raises(ValueError):
        utils.render_surface(f, _grid(), rays, sigma_thresh=-1.0, timestamps=ts)
    # the video path
    rk = dict(near_plane=0.0, far_plane=1e10, render_step_size=RENDER_STEP, cone_angle=0.0, alpha_thre=0.0,
              render_bkgd=torch.zeros(3, device=DEV))
    frames = render_video(f, _grid(), lambda i: _frame_rays((16, 16)), lambda i: ts, 1, max_samples=256,
                          render_kwargs=rk, surface=dict(sigma_thresh=10.0))
    assert torch.equal(frames[0]["surface_depth_f32"], image["depth"]) and torch.equal(frames[0]["surface_hit"], image["hit"])
    assert torch.equal(frames[0]["surface_normals_f32"], image["normal"])
    with pytest.raises(ValueError):
        render_video(f, _grid(), lambda i: _frame_rays((16, 16)), lambda i: ts, 1, max_samples=256,
                     render_kwargs=rk, surface=dict(thresh=10.0))


# ---- 6. mesh refinement -------------------------------------------------------------------------------------------------------
# The synthetic field's density swings by decades within a cell of its finest hash level (3 / 256): a lattice over the whole
# box is far coarser than the surface it samples (reso 32 over +-1.5, h = 0.094: the float64 model alone refines 4.8 % of the
# vertices, most brackets end below the threshold again).  The test lattice is therefore 32^3 over +-0.1 (h = 0.00625, half a
# finest cell), where the float64 model alone, on the CPU reference's surface nets, refines 84.4 % at reach 1 (91.8 % at
# reach 0.5, 44.8 % at reach 2) and takes the median |log(sigma / thresh)| from 0.48 to below 1e-4.
MESH = dict(reso=32, sigma_thresh=10.0, dirs="normal", center=[0.0, 0.0, 0.0], radius=0.1)
MESH_T = 0.37


def test_refined_mesh():
    """extract_mesh(refine=False) is the mesh of the default call, key by key.  With refine=True: faces and cube are
    unchanged; on refined vertices sigma >= thresh and the density one `width` back along the normal is < thresh;
    |offset| <= reach * h; unrefined vertices are the input's bits; sigma / embedding / rgb are query_density's and
    _query_rgb's at the new vertices.  More than half of the vertices are refined -- a floor first confirmed on the CPU by
    level_set64.bisect_f32 on the float64 model along the same lattice normals -- and the median |log(sigma / thresh)| over
    the vertices, the number the feature exists for, falls.  Measured on the lattice of MESH (V = 1398): the float64 model
    on the CPU refines 84.4 % and takes the median from 0.482 to 4.5e-5; an MI355X refines 84.4 % and takes it to 5.1e-5,
    the largest |offset| 0.991 h."""
    from ced_nerf_amd import export as E
    f = _field(True, 2, "f32")
    params = _params(True, 2)
    thresh = MESH["sigma_thresh"]
    plain = E.extract_mesh(f, MESH_T, **MESH)
    off = E.extract_mesh(f, MESH_T, refine=False, **MESH)
    assert set(plain) == set(off) and "refined" not in plain
    for k in plain:
        assert torch.equal(plain[k], off[k]) if isinstance(plain[k], torch.Tensor) else plain[k] == off[k], k
    v = plain["vertices"].shape[0]
    assert v > 100
    h = float(np.float32(2.0) * np.float32(plain["radius"]) / np.float32(32))

    # the floor, from the float64 model alone
    vn, nn = N(plain["vertices"]), N(plain["normals"])
    tf = lambda p: np.full(len(p), np.float32(MESH_T), np.float64)
    f64 = lambda p: np.exp(LS.raw64(params, p.astype(np.float64), tf(p))).astype(np.float32)
    reach = np.full(v, np.float32(h), np.float32)
    cpu = LS.bisect_f32(f64, vn, -nn, -reach, reach, thresh, 32, 0.0)
    cpu_share = float((cpu["status"] == 0).mean())
    cpu_vertices = np.where((cpu["status"] == 0)[:, None], cpu["x"], vn)
    log_ratio = lambda sigma: np.abs(np.log(np.maximum(sigma.astype(np.float64), 1e-30) / thresh))
    print(f"mesh [reso 32 over +-0.1, thresh {thresh:g}, reach 1]: V = {v}; float64 model on the CPU: {100 * cpu_share:.1f} % refined, median "
          f"|log(sigma / thresh)| {np.median(log_ratio(f64(vn))):.3e} -> {np.median(log_ratio(f64(cpu_vertices))):.3e}")
    assert cpu_share > 0.5

    fine = E.extract_mesh(f, MESH_T, refine=True, **MESH)
    again = E.refine_mesh(f, plain)
    for k in fine:
        assert torch.equal(fine[k], again[k]) if isinstance(fine[k], torch.Tensor) else fine[k] == again[k], k
    assert torch.equal(fine["faces"], plain["faces"]) and torch.equal(fine["cube"], plain["cube"])
    assert torch.equal(fine["normals"], plain["normals"])                       # lattice normals stay
    for k in ("reso", "center", "radius", "t", "sigma_thresh", "apply_act"):
        assert fine[k] == plain[k], k
    r = fine["refined"]
    assert r.dtype == torch.bool and r.shape == (v,) and fine["offset"].shape == (v,) and fine["width"].shape == (v,)
    share = float(r.float().mean())
    assert torch.equal(fine["vertices"][~r], plain["vertices"][~r]) and bool((fine["offset"][~r] == 0).all())
    assert bool((fine["offset"].abs() <= np.float32(h)).all())
    n, x = plain["normals"], fine["vertices"]
    moved = (x - plain["vertices"])[r]
    assert float((moved - fine["offset"][r, None] * n[r]).abs().max()) <= 4 * np.spacing(np.float32(1.5))
    tt = torch.full((v,), MESH_T, device=DEV)
    res = f.query_density(x, tt, return_feat=True)
    assert torch.equal(fine["sigma"], res["density"][:, 0]) and torch.equal(fine["embedding"], res["base_mlp_out"])
    assert bool((fine["sigma"][r] >= thresh).all())
    # one width back along the normal, formed as the kernel forms it: v + (-n) * (t - width) with t = -offset
    s_back = -fine["offset"] - fine["width"]
    back = f.query_density(plain["vertices"] + (-n) * s_back[:, None], tt)["density"][:, 0]
    assert bool((back[r] < thresh).all()), int((~(back[r] < thresh)).sum())
    head_on = torch.where((n == 0).all(-1, keepdim=True), n.new_tensor([0.0, 0.0, 1.0]), -n)
    assert torch.equal(fine["rgb"], f._query_rgb(head_on, fine["embedding"], False).view(v, 1, 3))
    before, after = np.median(log_ratio(N(plain["sigma"]))), np.median(log_ratio(N(fine["sigma"])))
    print(f"mesh on the device: {100 * share:.1f} % refined; median |log(sigma / thresh)| {before:.3e} -> {after:.3e}; "
          f"max |offset| / h = {float(fine['offset'].abs().max()) / h:.3f}")
    assert share > 0.5 and after < before
    # field normals are re-evaluated at the new vertices
    fld = E.extract_mesh(f, MESH_T, normals="field", refine=True, **MESH)
    assert torch.equal(fld["normals"], f.query_normals(fld["vertices"], tt[:fld["vertices"].shape[0]])[0])
    assert bool(fld["refined"].any())
    with pytest.raises(ValueError):
        E.refine_mesh(f, plain, reach=0.0)
    with pytest.raises(ValueError):
        E.extract_mesh(f, MESH_T, refine=True, refine_reach=float("nan"), **MESH)


def test_refined_mesh_files(tmp_path):
    from ced_nerf_amd import export as E
    f = _field(True, 2, "f32")
    fine = E.extract_mesh(f, MESH_T, refine=True, **MESH)
    E.save_mesh_npz(str(tmp_path / "fine.npz"), fine)
    with np.load(tmp_path / "fine.npz") as z:
        for k in ("vertices", "refined", "offset", "width", "sigma", "faces"):
            assert np.array_equal(z[k], N(fine[k])), k
    plain = E.extract_mesh(f, MESH_T, **MESH)
    E.save_mesh_npz(str(tmp_path / "plain.npz"), plain)
    with np.load(tmp_path / "plain.npz") as z:
        assert "refined" not in z.files and "offset" not in z.files
