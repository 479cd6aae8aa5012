"""A geometric float64 statement of the occupancy-grid march, and the comparison with it (plain numpy; the reference
imports nothing of the project).

What the march computes (nerfacc.traverse_grids), said without a DDA: on a ray the sample
boundaries form a LATTICE,

    t_0 = near,   t_{k+1} = fl32(t_k + dt_k),   dt_k = clamp(fl32(t_k * cone_angle), step, 1e10),

and sample k = (t_k, t_{k+1}) is emitted exactly when its midpoint mid_k = t_k + dt_k / 2 lies before the far plane,
inside some level's box, and in an occupied cell of the FINEST level whose box contains it.  The ray's termination
plane is the first lattice point whose midpoint is not before the end of (outermost box, far plane).  Everything else
in csrc/march_core.hpp and csrc/march_accel.hpp -- the DDA, its look-ahead, the deferred skip, the distance fields,
the closed-form skips, the lattice table -- is a fast way of evaluating that sentence.

The lattice is float32 by definition and is compared bit for bit.  Which cell a midpoint lies in is geometry, and the
float32 walk and this float64 statement may disagree about it within a small radius of a cell face: such midpoints are
UNDECIDED and ignored, all others must agree exactly.

The radius.  rho = 2 * res * 2^-23 * max(1, t_stop, max|aabb|) + 2e-6, where t_stop is the exit of the outermost box
the ray hits, clamped by the far plane.  The float32 DDA reaches a cell boundary by at most `res` additions of delta
per axis; each addition rounds by at most half an ulp of t, about 2^-24 * t, so a boundary's t is off by at most
res * 2^-24 * t, which a unit direction turns into the same distance in position; the positions the walk derives its
first cell and boundaries from carry roundings of the coordinates' size (hence max|aabb| and 1 in the max); the two
eps = 1e-6 offsets at the ends of a segment add 2e-6.  The factor 4 (2^-23 * 2 instead of 2^-24) is margin.  rho is a
radius in POSITION on purpose: for a ray that grazes a face the error of the crossing's t is unbounded, the distance
of the midpoint from the face is not.  A midpoint is decided when the answer is the same at the eight points
p_k +- rho per axis and |mid_k - far| > rho.
"""
import numpy as np

F32 = np.float32
MAX_LATTICE = 1 << 17                      # points per ray; a case that needs more is too fine for the suite


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def lattice_f32(near, step, cone_angle, t_end, cap=MAX_LATTICE):
    """The lattice from `near` up to the second point at or beyond t_end, by the float32 recurrence (one IEEE operation
    at a time, in the order the definition gives).  Returns (t [K + 1] float32, dt [K] float32)."""
    t = F32(near); step = F32(step); cone = F32(cone_angle); big = F32(1e10)
    ts, dts = [t], []
    beyond = 0
    while beyond < 2:
        v = F32(t * cone)
        dt = min(max(v, step), big)
        t = F32(t + dt)
        dts.append(dt); ts.append(t)
        if not t > ts[-2]:
            raise ValueError("the step no longer moves t")
        if float(t) >= t_end:
            beyond += 1
        if len(ts) > cap:
            raise ValueError(f"lattice longer than {cap} points (near {near}, step {step}, to {t_end})")
    return np.asarray(ts, F32), np.asarray(dts, F32)


def _slab(o, d, lo, hi):
    """float64 ray / box interval (t_in, t_out); t_in > t_out: no intersection."""
    t_in, t_out = -np.inf, np.inf
    for a in range(3):
        if d[a] == 0.0:
            if not (lo[a] <= o[a] <= hi[a]):
                return np.inf, -np.inf
            continue
        t1, t2 = (lo[a] - o[a]) / d[a], (hi[a] - o[a]) / d[a]
        t_in, t_out = max(t_in, min(t1, t2)), min(t_out, max(t1, t2))
    return t_in, t_out


def _occupied(p, mid, binaries, aabbs, far):
    """The sentence: p [K, 3] float64 -> occupied [K] bool, in_box [K] bool (both false for mid >= far)."""
    m, res = binaries.shape[0], binaries.shape[1]
    occ = np.zeros(p.shape[0], bool); inb = np.zeros(p.shape[0], bool)
    for lvl in range(m - 1, -1, -1):                      # coarsest to finest: the finest box that holds p wins
        lo, hi = aabbs[lvl, :3], aabbs[lvl, 3:]
        inside = ((p >= lo) & (p <= hi)).all(-1)
        idx = np.clip(np.floor((p - lo) / (hi - lo) * res), 0, res - 1).astype(np.int64)
        occ = np.where(inside, binaries[lvl][idx[:, 0], idx[:, 1], idx[:, 2]], occ)
        inb |= inside
    before = mid < far
    return occ & before, inb & before


def march_reference(o, d, binaries, aabbs, near, far, step, cone_angle):
    """Per ray r (lists indexed by ray): `lattice` [K + 1] float32; `mid` [K] float64; `occupied`, `decided`, `in_box` [K]
    bool per midpoint; `rho`; `stop_lo`, `stop_hi` [n]: where along the ray the region (outermost box, mid < far) ends when
    the box is shrunk / grown by rho and the far plane pulled in / pushed out by rho (-inf: that region is empty) -- the
    termination plane is the first lattice point whose midpoint is not before the region's end.  near, far: scalars or
    [n].  A ray without a finite box interval has zero samples and terminates at `near`: its lattice is the first two
    points and nothing is occupied."""
    o = np.asarray(o, F32).astype(np.float64); d = np.asarray(d, F32).astype(np.float64)
    binaries = np.asarray(binaries).astype(bool)
    aabbs64 = np.asarray(aabbs, F32).astype(np.float64)
    n = o.shape[0]
    m, res = binaries.shape[0], binaries.shape[1]
    near = np.broadcast_to(np.asarray(near, F32), (n,)); far = np.broadcast_to(np.asarray(far, F32), (n,))
    size = float(np.abs(aabbs64).max())
    lo_out, hi_out = aabbs64[:, :3].min(0), aabbs64[:, 3:].max(0)
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
    cache = {}
    ref = dict(lattice=[], mid=[], occupied=[], decided=[], in_box=[], rho=np.zeros(n), stop_lo=np.zeros(n), stop_hi=np.zeros(n),
               n_rays=n)
    for r in range(n):
        fr = float(far[r])
        t_in, t_out = _slab(o[r], d[r], lo_out, hi_out)
        hit = t_out > t_in and t_out > 0 and np.isfinite(t_out)
        t_stop = min(t_out, fr) if hit else 0.0
        rho = 2.0 * res * 2.0 ** -23 * max(1.0, t_stop, size) + 2e-6
        ref["rho"][r] = rho
        g_in, g_out = _slab(o[r], d[r], lo_out - 2 * rho, hi_out + 2 * rho)      # the walk may see a grazed box
        t_end = min(g_out, fr + 2 * rho) if (g_out > g_in and np.isfinite(g_out)) else -np.inf
        key = (near[r].tobytes(), )
        have = cache.get(key)
        if have is None or float(have[0][-2]) < t_end:
            have = cache[key] = lattice_f32(near[r], step, cone_angle, t_end)
        t, dt = have
        K = int(np.searchsorted(t, t_end, side="left")) + 1       # t[K - 1] >= t_end: the lattice ends two points beyond
        t, dt = t[:K + 1], dt[:K]
        mid = t[:-1].astype(np.float64) + dt.astype(np.float64) / 2
        occ = np.zeros(K, bool); inb = np.zeros(K, bool); dec = np.ones(K, bool)
        sel = np.flatnonzero((mid > g_in - 2 * rho) & (mid < g_out + 2 * rho)) if g_out > g_in else np.zeros(0, np.int64)
        if sel.size:
            ms = mid[sel]
            p = o[r] + d[r] * ms[:, None]
            occ[sel], inb[sel] = _occupied(p, ms, binaries, aabbs64, fr)
            same = np.ones(sel.size, bool)
            for c in corners:
                oc, _ = _occupied(p + rho * c, ms, binaries, aabbs64, fr)
                same &= oc == occ[sel]
            dec[sel] = same
        dec &= np.abs(mid - fr) > rho
        for sign, which in ((1.0, "stop_lo"), (-1.0, "stop_hi")):
            a, b = _slab(o[r], d[r], lo_out + sign * rho, hi_out - sign * rho)
            b = min(b, fr - sign * rho)
            ref[which][r] = b if a < b else -np.inf
        ref["lattice"].append(t); ref["mid"].append(mid); ref["occupied"].append(occ); ref["decided"].append(dec)
        ref["in_box"].append(inb)
    return ref


def reference_counts(ref):
    """[n, 3] int64 per ray: decided-occupied, decided-empty-in-box, undecided midpoints."""
    out = np.zeros((ref["n_rays"], 3), np.int64)
    for r in range(ref["n_rays"]):
        occ, dec, inb = ref["occupied"][r], ref["decided"][r], ref["in_box"][r]
        out[r] = (int((dec & occ).sum()), int((dec & ~occ & inb).sum()), int((~dec).sum()))
    return out


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def check_march(ref, t_starts, t_ends, packed_info, term=None, limit=0):
    """Asserts a march's output (ray-packed t_starts / t_ends, packed_info [n, 2] = (first, count)) against the reference:
      1. every (t_start, t_end) is a lattice interval (t_k, t_{k+1}) bit for bit, k strictly increasing along the ray, and
         packed_info is the exclusive scan of the counts;
      2. emitted_k == occupied_k at every decided midpoint -- with a `limit`, for a ray that used its whole budget, up to
         its last emitted sample;
      3. with `term` [n] (NaN: this ray's plane is not specified by the code under test): a ray that used its whole budget
         terminates at its last t_end; any other at a lattice point t_j not before its last sample, with midpoint j not
         before the end of the region (outermost box, mid < far) shrunk by rho, and midpoint j - 1 before the end of that
         region grown by rho (j = 0 where the grown region is empty).  So midpoint j is not deeper than rho inside the
         region, and midpoint j - 1 is within rho of its inside or, where the lattice steps over all of a region shorter
         than a step, before it.
    Returns (totals [3], per_ray [n, 3]): decided-occupied, decided-empty-in-box, undecided midpoints."""
    t_starts = np.asarray(t_starts, F32).reshape(-1); t_ends = np.asarray(t_ends, F32).reshape(-1)
    packed = np.asarray(packed_info, np.int64)
    n = ref["n_rays"]
    assert packed.shape == (n, 2) and t_starts.shape == t_ends.shape, (packed.shape, t_starts.shape, t_ends.shape)
    counts = packed[:, 1]
    assert (counts >= 0).all() and int(counts.sum()) == t_starts.shape[0], (int(counts.sum()), t_starts.shape)
    assert np.array_equal(packed[:, 0], np.cumsum(counts) - counts), "packed_info is not the exclusive scan of the counts"
    if limit > 0:
        assert (counts <= limit).all(), f"a ray has more than limit = {limit} samples"
    if term is not None:
        term = np.asarray(term, F32).reshape(-1)
        assert term.shape == (n,)
    bad_lattice, bad_set, bad_term = [], [], []
    n_disagree = 0
    for r in range(n):
        t = ref["lattice"][r]; tb = _bits(t)
        K = t.shape[0] - 1
        s0, c = int(packed[r, 0]), int(counts[r])
        a, b = t_starts[s0:s0 + c], t_ends[s0:s0 + c]
        k = np.searchsorted(t[:-1], a, side="left")
        k = np.minimum(k, K - 1)
        ok = (tb[k] == _bits(a)) & (tb[k + 1] == _bits(b))
        if c > 1:
            ok[1:] &= k[1:] > k[:-1]
        if not ok.all():
            i = int(np.flatnonzero(~ok)[0])
            bad_lattice.append((r, i, float(a[i]), float(b[i]), float(t[k[i]]), float(t[k[i] + 1])))
            continue
        emitted = np.zeros(K, bool); emitted[k] = True
        full = limit > 0 and c == limit
        upto = int(k[-1]) + 1 if full else K
        wrong = np.flatnonzero(ref["decided"][r][:upto] & (emitted[:upto] != ref["occupied"][r][:upto]))
        if wrong.size:
            n_disagree += int(wrong.size)
            j = int(wrong[0])
            bad_set.append((r, int(wrong.size), j, float(t[j]), bool(ref["occupied"][r][j])))
        if term is not None and not np.isnan(term[r]):
            if full:
                if _bits(term[r:r + 1])[0] != _bits(b[-1:])[0]:
                    bad_term.append((r, "whole budget: not the last t_end", float(term[r]), float(b[-1])))
                continue
            j = int(np.searchsorted(t, term[r], side="left"))
            if j > K or tb[j] != _bits(term[r:r + 1])[0]:
                bad_term.append((r, "not a lattice point", float(term[r]), float(t[min(j, K)])))
            elif c and j <= int(k[-1]):
                bad_term.append((r, "before the last sample", float(term[r]), float(b[-1])))
            elif j < K and not ref["mid"][r][j] >= ref["stop_lo"][r]:
                bad_term.append((r, "too early: its midpoint is deeper than rho inside", float(term[r]), j))
            elif j > 0 and not ref["mid"][r][j - 1] < ref["stop_hi"][r]:
                bad_term.append((r, "too late: the midpoint before it is more than rho past the end", float(term[r]), j))
    msgs = []
    if bad_lattice:
        msgs.append(f"{len(bad_lattice)} rays with a non-lattice interval; first (ray, sample, t_start, t_end, lattice t_k, t_k+1): "
                    f"{bad_lattice[:3]}")
    if bad_set:
        msgs.append(f"{n_disagree} disagreements on decided midpoints over {len(bad_set)} rays; first (ray, count, k, t_k, "
                    f"reference occupied): {bad_set[:3]}")
    if bad_term:
        msgs.append(f"{len(bad_term)} termination planes wrong; first: {bad_term[:3]}")
    if msgs:
        raise AssertionError("; ".join(msgs))
    per_ray = reference_counts(ref)
    return per_ray.sum(0), per_ray


def subset(ref, rays):
    """The reference of some of the rays."""
    rays = [int(r) for r in rays]
    out = {k: [v[r] for r in rays] for k, v in ref.items() if isinstance(v, list)}
    for k in ("rho", "stop_lo", "stop_hi"):
        out[k] = ref[k][rays]
    out["n_rays"] = len(rays)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# chained budgets: what the frame loop does (cednerf/utils.py:301-306)
# ---------------------------------------------------------------------------------------------------------------------
def chain(march, c, budgets=(1, 4, 13, 64, 1 << 20)):
    """march(rays, near, limit) -> (t_starts, t_ends, counts, term): the rays that used a whole budget resume at their
    termination planes with the next one.  Returns per-ray lists of t_starts / t_ends pieces."""
    n = c["o"].shape[0]
    alive = np.arange(n); near = c["near"].copy()
    p0 = [[] for _ in range(n)]; p1 = [[] for _ in range(n)]
    for limit in budgets:
        if alive.size == 0:
            break
        t0, t1, counts, term = march(alive, near[alive], limit)
        off = np.cumsum(counts) - counts
        for i, r in enumerate(alive):
            p0[r].append(t0[off[i]:off[i] + counts[i]]); p1[r].append(t1[off[i]:off[i] + counts[i]])
        keep = counts == limit
        near[alive[keep]] = term[keep]
        alive = alive[keep]
    assert alive.size == 0
    return p0, p1


def assert_chain_is_the_unlimited_march(p0, p1, whole_t0, whole_t1):
    for pieces, whole, what in ((p0, whole_t0, "t_starts"), (p1, whole_t1, "t_ends")):
        got = np.concatenate([np.asarray(x, F32) for r in pieces for x in r] + [np.zeros(0, F32)])
        whole = np.asarray(whole, F32)
        assert got.shape == whole.shape, f"chained {what}: {got.shape[0]} samples, the unlimited march has {whole.shape[0]}"
        assert np.array_equal(_bits(got), _bits(whole)), f"chained {what} differ from the unlimited march"


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
N_RAYS = 257            # not a multiple of 64 or 256, more than one workgroup
ROI = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
# the named edge rays, by index
(AXIS, AXIS_NEG_ZERO, BODY_DIAGONAL, FACE_DIAGONAL, ALMOST_AXIS, ON_FACE, ALONG_EDGE, MISS, IN_BLOCK_PLANE, IN_FINE_FACE_PLANE,
 IN_COARSE_FACE_PLANE, SHORT_INTERVAL, HUGS_CELL_FACE, CROSSES_FACE_LATE) = range(14)
NAMED = ("axis-parallel", "axis-parallel with -0.0", "body diagonal", "face diagonal through cell edges", "almost axis-parallel",
         "origin on a box face", "along a box edge", "miss", "in a cell-face plane inside a 2x2x2 block",
         "in a face plane of the finest box", "in a face plane of the level-1 box", "box interval shorter than a step",
         "hugs a cell face with a tiny direction component", "crosses a cell face it hugs just before the far plane")


def make_aabbs(roi, levels):
    """Nested levels: level i is the roi enlarged 2**i about its centre (float32, as the estimator builds them)."""
    roi = np.asarray(roi, F32)
    c = (roi[:3] + roi[3:]) / F32(2); e = (roi[3:] - roi[:3]) / F32(2)
    return np.stack([np.concatenate([c - e * F32(2 ** i), c + e * F32(2 ** i)]) for i in range(levels)], 0).astype(F32)


def make_rays(seed, n=N_RAYS, block_plane=False):
    """n unit-direction rays: half the origins on a radius-4 sphere aimed into the roi, half uniform in [-1.8, 1.8]^3 (inside
    fine boxes, inside coarse boxes only, inside occupied cells) with random directions; the named edge rays in front."""
    rng = np.random.default_rng(seed)
    h = n // 2
    v = rng.normal(size=(h, 3)); v /= np.linalg.norm(v, axis=-1, keepdims=True)
    o_out = 4.0 * v
    d_out = rng.uniform(-1.0, 1.0, size=(h, 3)) - o_out
    o_in = rng.uniform(-1.8, 1.8, size=(n - h, 3))
    d_in = rng.normal(size=(n - h, 3))
    o = np.concatenate([o_out, o_in]); d = np.concatenate([d_out, d_in])
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    perm = rng.permutation(n)                              # both kinds in every wave
    o, d = o[perm].astype(F32), d[perm].astype(F32)
    r3, r2 = 1.0 / np.sqrt(3.0), np.sqrt(0.5)
    named = {AXIS: ((-3.0, 0.013, 0.37), (1.0, 0.0, 0.0)),
             AXIS_NEG_ZERO: ((0.29, 3.0, -0.41), (-0.0, -1.0, -0.0)),
             BODY_DIAGONAL: ((-1.5, -1.5, -1.5), (r3, r3, r3)),                # every crossing is a three-way tie
             FACE_DIAGONAL: ((-3.0, -3.0, 0.1), (r2, r2, 0.0)),
             ALMOST_AXIS: ((-3.0, 0.21, -0.33), (1.0, 1e-7, -1e-7)),
             ON_FACE: ((-1.0, 0.3, 0.2), tuple(np.array([1.0, 0.2, 0.1]) / np.linalg.norm([1.0, 0.2, 0.1]))),
             ALONG_EDGE: ((-3.0, -1.0, -1.0), (1.0, 0.0, 0.0)),
             MISS: ((9.0, 9.0, 20.0), (0.6, 0.0, 0.8)),
             # a ray IN a box's face plane (d_x = 0, o_x on the plane): the slab test's 0 * inf = NaN once lost the interval's
             # start (samples from the near plane on, outside every box) or its end (nothing behind that box)
             IN_FINE_FACE_PLANE: ((-1.0, -0.0706554651260376, -3.8532772064208984), (0.0, 0.1961161345243454, 0.9805806875228882)),
             IN_COARSE_FACE_PLANE: ((2.0, 3.5, 2.0), (0.0, -0.8637788891792297, -0.5038710236549377)),
             # enters the level-1 box at t = 3.492: with far = 3.5 and step 0.02 from near 0.3 the midpoints 3.49 and 3.51
             # step over all of the interval
             SHORT_INTERVAL: ((-5.492, 0.3, 0.2), (1.0, 0.0, 0.0)),
             # z stays within 1e-29 of the cell face z = 0 (every resolution here is even) while d_z != 0: the DDA's first z
             # boundary is the face the ray stands on, and the step across it once ended the segment at its start
             HUGS_CELL_FACE: ((-3.0, 0.3, 1e-30), (0.99875, 0.04994, -1e-30)),
             # x falls from 3.00002 through the level-2 cell face x = 3 (res 8) at t = 1.993, by 1e-5 per unit of t: with
             # far = 2 the float32 positions at both ends of the segment round into the same cell, the DDA's crossing (off
             # by the rounding error / |d_x|) lands at 1.985, and the step across it once ended the segment there
             CROSSES_FACE_LATE: ((3.0000216960906982, 0.7173625230789185, 1.7849211692810059),
                                 (-1.088861063180957e-05, 0.7663187384605408, -0.6424605846405029))}
    if block_plane:     # y = -0.625 is the face between cells 2 and 3 of a res-16 level on the roi: one 2x2x2 block
        named[IN_BLOCK_PLANE] = ((-2.0, -0.625, -1.2), (0.8, 0.0, 0.6))
    for i, (oo, dd) in named.items():
        o[i] = np.asarray(oo, F32); d[i] = np.asarray(dd, F32)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def speckle(seed, res, levels, fill):
    return np.random.default_rng(seed).uniform(size=(levels, res, res, res)) < fill


def block_speckle(seed, res, levels, fill):
    """res/2 speckle upsampled by 2: every face inside a 2x2x2 block has equal occupancy on both sides."""
    s = speckle(seed, res // 2, levels, fill)
    return s.repeat(2, 1).repeat(2, 2).repeat(2, 3)


def _spheres(levels):
    from ced_nerf_amd import synthetic as S                  # the scenes' analytic grid; the reference itself imports nothing
    return S.make_occupancy(ROI, 128, levels)


# name: (grid builder, levels, step, cone_angle, near, far, stratified near planes)
_CASES = {
    "speckle16_L1": (lambda: speckle(11, 16, 1, 0.3), 1, 0.01, 0.0, 0.0, 1e10, False),
    "speckle20_L2": (lambda: speckle(12, 20, 2, 0.4), 2, 0.02, 0.004, 0.3, 3.5, False),
    "speckle12_L4": (lambda: speckle(13, 12, 4, 0.5), 4, 0.3, 0.01, 0.0, 1e10, False),
    "speckle24_L3": (lambda: speckle(17, 24, 3, 0.35), 3, 0.02, 0.0, 0.0, 1e10, False),
    "speckle8_L3_far2": (lambda: speckle(18, 8, 3, 0.6), 3, 0.004365412945816821, 0.0, 0.3, 2.0, False),
    "speckle16_L2_stratified": (lambda: speckle(14, 16, 2, 0.2), 2, 0.05, 0.0, 0.05, 1e10, True),
    "speckle20_L1_far_before_near": (lambda: speckle(15, 20, 1, 0.4), 1, 0.02, 0.0, 2.0, 1.0, False),
    "block16_L2": (lambda: block_speckle(16, 16, 2, 0.4), 2, 0.004, 0.0, 0.0, 1e10, False),
    "dnerf128_L1": (lambda: _spheres(1), 1, 5e-3, 0.0, 0.0, 1e10, False),
    "hypernerf128_L2": (lambda: _spheres(2), 2, 1e-3, 0.004, 0.2, 1e10, False),
    "dynerf128_L4": (lambda: _spheres(4), 4, 1e-3, 0.004, 0.2, 1e10, False),
}
CASES = tuple(_CASES)
SPECKLE_CASES = tuple(c for c in CASES if c.startswith(("speckle", "block")))
_made = {}


def case(name):
    """The inputs of a case and their reference, made once: dict(o, d, binaries [m, R, R, R] bool, aabbs [m, 6], near [n],
    far [n], step, cone_angle, ref).  Do not write to it."""
    if name not in _made:
        grid, levels, step, cone, near, far, stratified = _CASES[name]
        binaries = np.ascontiguousarray(grid())
        o, d = make_rays(100 + CASES.index(name), block_plane=name.startswith("block"))
        n = o.shape[0]
        near = np.full(n, near, F32)
        if stratified:
            near = (near + np.random.default_rng(7).uniform(size=n).astype(F32) * F32(step)).astype(F32)
        c = dict(name=name, o=o, d=d, binaries=binaries, aabbs=make_aabbs(ROI, levels), near=near, far=np.full(n, far, F32),
                 step=float(step), cone_angle=float(cone), common_near=not stratified)
        c["ref"] = march_reference(o, d, binaries, c["aabbs"], near, c["far"], step, cone)
        _made[name] = c
    return _made[name]
