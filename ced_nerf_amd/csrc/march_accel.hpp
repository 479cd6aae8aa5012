// The occupancy-grid walk, every piece of it once: DDA set-up (dda_setup_axis), branch-free look-ahead batch
// (look_ahead, load_batch), the samples of one occupied cell (emit_cell), on the segment decoder, slab test and skip
// marches of march_core.hpp.  Two compositions of these pieces emit the per-ray sample sets of nerfacc.traverse_grids
// (restated independently by the CPU oracle; call site cednerf/utils.py:241-264):
//   traverse_ray_frame  the walker of the frame renderer (frame.hip), the one-shot march (march_all.hip) and the host twin
//                       (accel.hip): skips applied lazily, and -- with distance fields -- empty space at O(1) per stretch;
//   traverse_ray        ced_traverse_grids' (march.hip): no distance fields, skips marched eagerly, the termination
//                       plane of every ray.  It is a special case of the former in what it computes (checked bit for
//                       bit on the host); it stays a composition of its own for speed (see there).
// With distance fields, empty space costs O(1) per stretch instead of one DDA step per cell:
//
//   * a CHEBYSHEV DISTANCE FIELD over the grid (per cell: a lower bound of the distance in cells to the nearest
//     occupied cell; per 8^3-cell brick when only the cheap brick-level field exists) is sphere-traced along the
//     ray -- a probe with empty radius D allows D - 3 cells of travel on every axis with nothing occupied in reach
//     (conservative: the exact DDA's cells stay within one cell of the ideal line);
//   * where the probes arrive next to occupied bricks, the exact DDA state is RE-ENTERED IN CLOSED FORM: the DDA is a
//     merge of three per-axis sequences T_a(j) = fl(T_a(j-1) + delta_a), and inside one binade such a float recurrence
//     is an exact arithmetic progression of mantissas (regular_binade, march_core.hpp), so "all events with T < tau"
//     is computed per axis with integer arithmetic -- bit for bit the state the cell-by-cell walk has when it gets
//     there.  Every float the emitted samples depend on (t_last lattice, cell boundaries t_trav) is therefore
//     unchanged; only which empty cells were looked at differs.
//   * that is also all a GROUP CLEARANCE changes (group_clear: one cone per 64 consecutive rays, traced once per call
//     through the same fields): a group cleared to the far plane marches nothing, and any other clearance is only where
//     a segment's first trace starts probing (t_hint) -- the DDA set-up, cells_skipped and the re-entry are still taken
//     from the segment's start.
//
// Contract of traverse_ray_frame (what the frame loop observes): the emitted (t_start, t_end) pairs and their count
// n <= limit are those of the reference walk; t_term is exact when n == limit (the ray may stay alive and its
// termination plane becomes the next near plane, cednerf/utils.py:301) and unspecified otherwise (a ray that returns
// fewer samples than its budget is dead, utils.py:303-306, and nobody reads its plane).
// Host and device code: the CPU test-suite runs this file against the oracle through ced_host_march_frame.
#pragma once
#include <cmath>

#include "march_core.hpp"

// Diagnostic build (-DCED_MARCH_DIAG, tools/march_diag.py): every phase of the walk reports how many lanes of the wave
// are in it and how long the wave stays in it.  Nothing in the shipped library.
#if defined(CED_MARCH_DIAG) && defined(__HIP_DEVICE_COMPILE__)
__device__ void ced_diag_tick(int phase);
#define CED_DIAG_TICK(p) ced_diag_tick(p)
#else
#define CED_DIAG_TICK(p) ((void)0)
#endif

namespace ced {

constexpr int kBrickShift = 3;                 // kBrick == 8
constexpr int kLook = 8;                       // look-ahead of ced_traverse_grids' walk (cells per batch)
constexpr int kFrameLook = 4;                  // look-ahead of the frame renderer's exact walk (cells per batch)
constexpr float kMinJumpCells = 3.0f;          // the closed-form re-entry costs about as much as walking this many cells
constexpr int kCoarseRadius = 6;               // the exact walk hands over to the sphere trace at this empty radius
static_assert((1 << kBrickShift) == kBrick, "brick size");

// Emulates   k = 0; while (k < kcap && x < tau) { prev = x; x = x + d; ++k; }   (binary32, round to nearest even)
// in O(#binades).  Returns k; `prev` is the value before the last add (meaningful when k > 0).
CED_HD int count_steps(float &x, float d, float tau, int kcap, float &prev)
{
    int k = 0;
    for (;;) {
        if (k >= kcap || !(x < tau)) break;
        const float x1 = x + d;
        Binade B;
        if (regular_binade(x, x1, d, B)) {
            const uint32_t X = B.X, INC = B.INC;
            uint32_t LIM = 0x1000000u;                       // first mantissa that is not < min(tau, binade top)
            if (tau < bits_to_float(B.ex + (1u << 23))) LIM = (float_to_bits(tau) & 0x7fffffu) | 0x800000u;   // tau >= x: same binade
            // j_tau = #{ j >= 0 : X + j*INC < LIM } = floor((LIM - X - 1) / INC) + 1      (LIM > X here)
            const uint32_t Q = LIM - X - 1u;
            uint32_t q = (uint32_t)((float)Q / (float)INC);  // both < 2^24: exact operands, quotient off by <= 1
            if (q * INC > Q) --q;
            if ((q + 1u) * INC <= Q) ++q;
            uint32_t n = q + 1u;
            const uint32_t room = (uint32_t)(kcap - k);
            if (n > room) n = room;
            // the n-th add must itself stay inside the binade (a crossing add rounds on the next binade's grid)
            if (X + n * INC > 0xffffffu) --n;
            if (n >= 1u) {
                prev = B.term(n - 1u);
                x = B.term(n);
                k += (int)n;
                continue;
            }
        }
        prev = x;
        x = x1;
        ++k;
    }
    return k;
}

// All rays of a frame march on ONE lattice when cone_angle == 0: t_0 = near plane, t_{k+1} = fl(t_k + step)
// (termination planes are lattice points too).  G.lattice[e] = the first lattice point whose biased exponent is e
// (NaN: none), built once per call (build_lattice): a skip to a far target -- the first sample of a ray that enters
// the scene, ten binades from the near plane -- then starts one binade short of the target instead of at t_last.
CED_HD float skip_march_lattice(const GridSpec &G, float t_last, float target)
{
    if (G.lattice && G.step_size > 0.0f && G.cone_angle == 0.0f) {
        const float A = target - G.step_size * 0.5f;
        const int e = (int)((float_to_bits(A) >> 23) & 0xffu);
        // the answer is > A - step; the first lattice point of binade e-1 is below that whenever the binade is
        // much wider than the step (it is at most 2^(e-128) + step)
        if ((float_to_bits(A) >> 31) == 0 && e >= 2 && e <= 254 && bits_to_float((uint32_t)(e - 1) << 23) > 4.0f * G.step_size) {
            const float first = G.lattice[e - 1];
            if (first > t_last && first < A - G.step_size) t_last = first;
        }
    }
    return skip_march(t_last, target, G.step_size, G.cone_angle);
}

// Fills lattice[0..255] for the lattice that starts at `near` (see skip_march_lattice).  One thread.
CED_HD void build_lattice(float near, float step, float *lattice)
{
    for (int e = 0; e < 256; ++e) lattice[e] = bits_to_float(0x7fc00000u);
    if (!(step > 0.0f) || !(near >= 0.0f)) return;
    float t = near;
    for (int guard = 0; guard < 1024; ++guard) {
        const int e = (int)((float_to_bits(t) >> 23) & 0xffu);
        if (e >= 255 || t + step == t) break;
        if (!(lattice[e] == lattice[e])) lattice[e] = t;
        // first lattice point of a later binade: skip to the top of this one (target = 2^(e-126), so that the skip
        // stops at the first t with t + h >= top), then single steps across
        const float top = e == 0 ? bits_to_float(1u << 23) : bits_to_float((uint32_t)(e + 1) << 23);
        if (!(top < 3.0e38f)) break;
        float u = skip_march_const_step(t, top, step);
        int steps = 0;
        while ((int)((float_to_bits(u) >> 23) & 0xffu) == e && steps < 4) { const float v = u + step; if (v == u) return; u = v; ++steps; }
        if ((int)((float_to_bits(u) >> 23) & 0xffu) == e) return;          // the step no longer moves t: the lattice ends
        t = u;
    }
}

// Distance fields over the occupancy grid (accel.hip builds them):
//   bdist[lvl][bx][by][bz]  Chebyshev distance in BRICKS (8^3 cells) from brick b to the nearest brick holding an
//                           occupied cell, capped; 0 = the brick itself does.  Cheap (nb^3 bytes): built per call when
//                           the caller brings nothing.
//   cdist[lvl][x][y][z]     a lower bound of the Chebyshev distance in CELLS from the cell to the nearest occupied one
//                           (exact up to 15, the brick bound beyond; 0 = occupied).  Optional (res^3 bytes per level):
//                           with it the exact walk is only needed within three cells of an occupied cell.
// Bricks / cells outside the grid count as empty.
struct AccelSpec {
    const uint8_t *bdist;      // [n_grids, nb, nb, nb]; NULL: no acceleration (plain cell-by-cell walk)
    int nb;                    // ceil(res / kBrick)
    const uint8_t *cdist;      // [n_grids, res, res, res] or NULL
};

// lower bound of the Chebyshev cell distance from cell c to the nearest occupied cell of level lvl
CED_HD int empty_radius(const AccelSpec &S, int lvl, int res, int c0, int c1, int c2)
{
    if (S.cdist) return S.cdist[((size_t)lvl * res + c0) * res * res + (size_t)c1 * res + c2];
    const int R = S.bdist[(((size_t)lvl * S.nb + (c0 >> kBrickShift)) * S.nb + (c1 >> kBrickShift)) * S.nb + (c2 >> kBrickShift)];
    return R == 0 ? 0 : (R - 1) * kBrick + 1;
}

// Sphere-traces the distance field of level `lvl` from t_from towards t_to.  Returns true when nothing occupied can be
// met before t_to; otherwise false with t_stop = a time such that nothing occupied can be met in [t_from, t_stop) and
// the point at t_stop is within three cells of an occupied one (t_stop == t_from: no skip possible).
// A probe in cell c with empty radius D: every cell within D-1 of c is empty; travelling s cells per axis reaches cells
// at most floor(s)+1 away from c, and the exact DDA's cell is at most one more from the ideal line: s = D - 3.
// t_probe (the group clearance, below): the caller knows that nothing occupied can be met in [t_from, t_probe), and the
// probes start at max(t_from, t_probe); cells_skipped still counts from t_from, which is where the caller's DDA stands.
// Only a POSITIVE t_probe is such a claim: clearances are computed for near planes >= 0 only, 0 is their "nothing is
// claimed", and a segment that starts below 0 (a negative near plane) must not have its start moved by it.  The default,
// -inf, is no claim for any segment; the trace inside a segment (from t_c) never takes one.
CED_HD bool coarse_advance(const AccelSpec &S, int lvl, int res, const float *__restrict__ ab, const float (&o)[3],
                           const float (&d)[3], float t_from, float t_to, float &t_stop, float &cells_skipped,
                           float t_probe = -__builtin_inff())
{
    const float resf = (float)res;
    float sc[3], g = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        sc[a] = resf / (ab[3 + a] - ab[a]);                   // cells per unit length on axis a
        g = fmaxf(g, fabsf(d[a]) * sc[a]);                    // cells per unit t, Chebyshev
    }
    t_stop = t_from;
    cells_skipped = 0.0f;
    if (!(g > 0.0f) || !(g < 3.0e38f) || !(t_to - t_from < 3.0e38f)) return false;
    const float inv_g = 1.0f / g;
    float t = t_probe > 0.0f ? fmaxf(t_from, t_probe) : t_from;
    if (t >= t_to) return true;
    for (int guard = 0; guard < 8192; ++guard) {
        CED_DIAG_TICK(2);
        int c[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = clampi((int)((o[a] + d[a] * t - ab[a]) * sc[a]), 0, res - 1);
        const int D = empty_radius(S, lvl, res, c[0], c[1], c[2]);
        if (D < 4) { t_stop = t; cells_skipped = (t - t_from) * g; return false; }
        t += (float)(D - 3) * inv_g;
        if (t >= t_to) return true;
    }
    t_stop = t_from;            // not reached in practice (every probe advances at least one cell)
    return false;
}

// ---- Group clearance: the same sphere trace, once for a bundle of rays ------------------------------------------------
// A frame's rays arrive in groups of kGroupRays consecutive indices (an 8x8-pixel tile when the caller deals tiles, but
// nothing here assumes a camera).  Per group ONE cone is traced through the distance field of every level, and the
// result t_clear promises: no member ray meets an occupied cell of any level at a parameter t < t_clear (+inf: nowhere
// between the near and far planes; 0: nothing is claimed).  The first iteration of a frame skips the groups with +inf
// and hands the others' t_clear to traverse_ray_frame as t_hint.  PRECONDITION: near plane >= 0 -- every trace then runs
// over t >= 0, where the bound below holds and t_clear >= 0; with a negative near plane every group gets 0 and the
// renderers compute and pass nothing.
//
// The bound.  The group is described by a reference ray (oc, dc) -- one of its members, group_reference -- and per axis a
// the largest deviations of the members from it, dev_o[a] = max_i |o_i - oc|, dev_d[a] = max_i |d_i - dc|.
// With the probe at the reference point of parameter t, every member at parameter t' in [t, t + D] lies on axis a within
//     sc_a * (dev_o[a] + dev_d[a] * t' + |dc_a| * (t' - t))        cells
// of the probe.  As in coarse_advance, a probe cell with empty radius R lets every point within R - 3 cells on every axis
// walk only empty cells (one cell for the probe's position inside its cell, one for the exact DDA straying from the
// ideal line, and R - 1 is the last empty ring).  The expression grows with t', so the largest admissible D solves it at
// t' = t + D, axis by axis.
// A reference point outside the level's box is probed at the clamped cell: clamping an axis moves the probe towards
// the box, so no member point INSIDE the box gets farther from it on any axis (a contraction in the Chebyshev metric),
// and a member is only ever inside a level between its own entry and exit, which is where the trace runs; cells outside
// the grid count as empty.
// ALL FLOAT SLACK IS HERE: every position above is a handful of binary32 operations on numbers no larger than
// M_a = |oc_a| + dev_o[a] + max|box_a| + (|dc_a| + dev_d[a]) * t', each rounding at most 2^-24 of that; that covers the
// rounding of dev_*, of the probe's position and its conversion to a cell, and of t itself (the next probe
// stands at fl(t + D), at most 2^-24 t' beyond t + D).  kClearRel = 2^-20 of sc_a * M_a is sixteen such roundings.
// The division that solves for D and the sums of the bound's terms round relative to at most 255 * 8 cells: below
// 2^-12 cells in all, inside the constant kClearAbs = 1/16 cell.
constexpr int kGroupRays = 64;
constexpr int kGroupMaxLevels = 8;             // the renderers' kMaxGrids: group_member's v holds 6 + 2 * this at most
constexpr float kClearRel = 1.0f / 1048576.0f;
constexpr float kClearAbs = 0.0625f;
constexpr float kClearMinCells = 1.0f;         // a probe that allows less than this ends the trace (and bounds its length)

struct RayGroupBounds {
    float oc[3], dc[3], dev_o[3], dev_d[3];
};

CED_HD bool finite3(const float (&v)[3])
{
    return fabsf(v[0]) < __builtin_inff() && fabsf(v[1]) < __builtin_inff() && fabsf(v[2]) < __builtin_inff();
}

// The member that serves as the group's reference ray: at 9/16 of the group (ray 36 of 64: the centre pixel of an 8x8
// tile dealt in raster order, next to the middle of a 64-pixel strip).  Any member is sound; a central one halves dev_d.
CED_HD int group_reference(int members) { return members * 9 / 16; }

// One member's share of its group's maxima against the reference ray (oc, dc): v[0..2] = |o - oc|, v[3..5] = |d - dc|,
// and per level l the interval of the set-up's own slab test (frame_prep_kernel / decode_segment<SINGLE>: the same
// arithmetic, so a level the walk visits is a level counted here) as v[6 + 2l] = -entry, v[7 + 2l] = exit -- every
// entry of v is a maximum over the members (-inf before the first).  The host folds the members one after the other;
// on the device every lane folds its own ray and the wave reduces.  `bad`: a non-finite component.
CED_HD void group_member(const float (&o)[3], const float (&d)[3], const float (&oc)[3], const float (&dc)[3], int n_grids,
                         const float *__restrict__ aabbs, float *v, bool &bad)
{
    bad = bad || !finite3(o) || !finite3(d);
    const float inv_d[3] = { 1.0f / d[0], 1.0f / d[1], 1.0f / d[2] };
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        v[a] = fmaxf(v[a], fabsf(o[a] - oc[a]));
        v[3 + a] = fmaxf(v[3 + a], fabsf(d[a] - dc[a]));
    }
#pragma unroll
    for (int l = 0; l < kGroupMaxLevels; ++l) {        // (unrolled: v stays in registers on the device)
        float t0, t1;
        if (l >= n_grids || !slab_test(o, inv_d, aabbs + 6 * l, t0, t1)) continue;
        v[6 + 2 * l] = fmaxf(v[6 + 2 * l], -t0);
        v[7 + 2 * l] = fmaxf(v[7 + 2 * l], t1);
    }
}

// One level: [t_lo, t_hi] = the union of the members' own [entry, exit] in this level's box, clamped to the near and far
// planes.  Returns +inf when the whole of it is proven empty, else a t up to which it is.
CED_HD float group_clear_level(const AccelSpec &S, int lvl, int res, const float *__restrict__ ab, const RayGroupBounds &B,
                               float t_lo, float t_hi)
{
    if (!(t_lo < t_hi)) return __builtin_inff();          // no member is inside this level between the planes
    const float resf = (float)res;
    float sc[3], slope[3], base[3], per_t[3], g = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        sc[a] = resf / (ab[3 + a] - ab[a]);
        const float reach = fabsf(B.dc[a]) + B.dev_d[a];   // units per unit t: any member against a fixed point
        slope[a] = sc[a] * reach * (1.0f + kClearRel);
        base[a] = sc[a] * (B.dev_o[a] + kClearRel * (fabsf(B.oc[a]) + B.dev_o[a] + fmaxf(fabsf(ab[a]), fabsf(ab[3 + a])))) + kClearAbs;
        per_t[a] = sc[a] * (B.dev_d[a] + kClearRel * reach);
        g = fmaxf(g, slope[a]);
    }
    if (!(g > 0.0f) || !(g < 3.0e38f) || !(t_hi < 3.0e38f) || !(base[0] + base[1] + base[2] < 3.0e38f)) return t_lo;
    float t = t_lo;
    for (int guard = 0; guard < 8192; ++guard) {
        int c[3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
            c[a] = clampi((int)fminf(fmaxf((B.oc[a] + B.dc[a] * t - ab[a]) * sc[a], -1.0f), resf), 0, res - 1);
        const float room = (float)(empty_radius(S, lvl, res, c[0], c[1], c[2]) - 3);
        float adv = __builtin_inff();
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float left = room - (base[a] + per_t[a] * t);
            if (slope[a] > 0.0f) adv = fminf(adv, left / slope[a]);
            else if (!(left >= 0.0f)) adv = -1.0f;
        }
        if (!(adv * g >= kClearMinCells)) return t;
        t += adv;
        if (t >= t_hi) return __builtin_inff();
    }
    return t;
}

// t_clear of a group: lim[2 * lvl], lim[2 * lvl + 1] = the smallest entry and the largest exit of the members that hit
// level lvl's box (slab_test; +inf / -inf when none does).
CED_HD float group_clear(const AccelSpec &S, int n_grids, int res, const float *__restrict__ aabbs, const RayGroupBounds &B,
                         const float *__restrict__ lim, float near, float far)
{
    // near >= 0 is a precondition of the bound: the deviation term dev_d * t' (group_clear_level) is |t'| for real, and
    // 0 is only "nothing is claimed" when no segment starts below it.  With a negative (or NaN) near plane: no claim.
    if (!(near >= 0.0f)) return 0.0f;
    if (!(finite3(B.oc) && finite3(B.dc) && finite3(B.dev_o) && finite3(B.dev_d))) return 0.0f;
    float t_clear = __builtin_inff();
    for (int lvl = 0; lvl < n_grids; ++lvl)
        t_clear = fminf(t_clear, group_clear_level(S, lvl, res, aabbs + 6 * lvl, B, fmaxf(lim[2 * lvl], near), fminf(lim[2 * lvl + 1], far)));
    return t_clear;
}

// The exact DDA of one segment: per axis the time of the next boundary crossing, the time between crossings, the cell
// the walk stands in, the step direction and the first cell index past the segment's last cell.
struct Dda {
    float tdist[3], delta[3];
    int cur[3], stp[3], ovf[3];
    int safe_cell;             // the last in-grid cell index formed (look_ahead)
    bool done;                 // stepped out of the segment's last cell
};

// DDA set-up of the segment [this_tmin, this_tmax] in the level with box `ab`, one axis: the reference's arithmetic,
// operation for operation (four divisions).
CED_HD void dda_setup_axis(Dda &D, int a, int res, const float *ab, const float (&o)[3], const float (&d)[3],
                           const float (&inv_d)[3], float this_tmin, float this_tmax)
{
    const float eps = 1e-6f;
    const float resf = (float)res;
    const float ts = this_tmin + eps, te = this_tmax - eps;
    const float ext = ab[3 + a] - ab[a];
    const float vox = ext / resf;
    const float ps = o[a] + d[a] * ts;
    const float pe = o[a] + d[a] * te;
    D.cur[a] = clampi((int)(((ps - ab[a]) / ext) * resf), 0, res - 1);
    const int fin = clampi((int)(((pe - ab[a]) / ext) * resf), 0, res - 1);
    const int idelta = d[a] > 0.0f ? 1 : 0;
    const float tm = ((ab[a] + (((float)(D.cur[a] + idelta) * vox) - ps)) * inv_d[a]) + this_tmin;
    const float stepf = (d[a] == 0.0f) ? 0.0f : (d[a] > 0.0f ? 1.0f : -1.0f);
    D.stp[a] = (int)stepf;
    // An axis on which the segment starts and ends in the same cell (cur == fin) has no crossing inside the segment.  A
    // first boundary computed before te all the same (a ray that hugs a cell face with a tiny d_a stands within a
    // rounding error of that face, and tm is then off by that error / |d_a|, even behind the start) is not a crossing:
    // the one step it would take leads straight past the final cell and would end the segment there, dropping the
    // rest of it.  Such an axis is treated as a d_a == 0 axis is.
    const bool no_crossing = d[a] == 0.0f || (D.cur[a] == fin && tm < te);
    D.tdist[a] = no_crossing ? this_tmax : tm;
    D.delta[a] = (d[a] == 0.0f) ? this_tmax : (vox * inv_d[a]) * stepf;
    D.ovf[a] = fin + D.stp[a];
}

// After the three axes: the walk stands in its first cell.
CED_HD void dda_begin(Dda &D, int res)
{
    D.safe_cell = (D.cur[0] * res + D.cur[1]) * res + D.cur[2];
    D.done = false;
}

// Steps the DDA through the next LOOK cells: tt[b] = the time the walk leaves cell b of the batch (its t_trav),
// cellv[b] = the cell's index in the level's grid; returns the mask of the cells that exist (the walk can end inside
// the batch).  The path does not depend on the occupancy values, so the caller fetches the bytes of all LOOK cells
// together afterwards.  Branch-free, predicated selects only: those loads are then independent instructions in flight
// together (a data-dependent branch per cell would serialise them behind s_waitcnt).
template <int LOOK>
CED_HD unsigned look_ahead(Dda &D, int res, float this_tmax, float (&tt)[LOOK], int (&cellv)[LOOK])
{
    unsigned valid_mask = 0;
    int safe_cell = D.safe_cell;         // (locals: selects on them stay selects, members turn into branches)
    bool done = D.done;
#pragma unroll
    for (int b = 0; b < LOOK; ++b) {
        const bool live = !done;
        valid_mask |= live ? (1u << b) : 0u;
        tt[b] = fminf(fminf(D.tdist[0], fminf(D.tdist[1], D.tdist[2])), this_tmax);
        const int cell = (D.cur[0] * res + D.cur[1]) * res + D.cur[2];
        safe_cell = live ? cell : safe_cell;                // never form an out-of-grid address
        cellv[b] = safe_cell;
        const bool sx = (D.tdist[0] < D.tdist[1]) && (D.tdist[0] < D.tdist[2]);
        const bool sy = !sx && (D.tdist[1] < D.tdist[2]);
        const bool sz = !sx && !sy;
        const float nx = D.tdist[0] + D.delta[0], ny = D.tdist[1] + D.delta[1], nz = D.tdist[2] + D.delta[2];
        D.tdist[0] = (live && sx) ? nx : D.tdist[0];
        D.tdist[1] = (live && sy) ? ny : D.tdist[1];
        D.tdist[2] = (live && sz) ? nz : D.tdist[2];
        D.cur[0] += (live && sx) ? D.stp[0] : 0;
        D.cur[1] += (live && sy) ? D.stp[1] : 0;
        D.cur[2] += (live && sz) ? D.stp[2] : 0;
        // (bitwise on purpose: && / || here can come out as a short-circuit branch per cell)
        const bool over = (sx & (D.cur[0] == D.ovf[0])) | (sy & (D.cur[1] == D.ovf[1])) | (sz & (D.cur[2] == D.ovf[2]));
        done = done || (live && over);
    }
    D.safe_cell = safe_cell;
    D.done = done;
    return valid_mask;
}

// What a batch looks at, fetched together: the occupancy bytes of its cells and -- with distance fields -- the empty
// radius of the cell the walk stands in afterwards (returned; 0 without).
template <int LOOK>
CED_HD int load_batch(const uint8_t *__restrict__ grid, const int (&cellv)[LOOK], const AccelSpec &S, bool accel, const Dda &D,
                      int lvl, int res, uint8_t (&occ)[LOOK])
{
#pragma unroll
    for (int b = 0; b < LOOK; ++b) occ[b] = grid[cellv[b]];
    int radius = 0;
    if (accel) {
        const int c0 = D.done ? 0 : D.cur[0], c1 = D.done ? 0 : D.cur[1], c2 = D.done ? 0 : D.cur[2];
        radius = empty_radius(S, lvl, res, c0, c1, c2);
    }
    return radius;
}

// Where the march stands on the ray: the end of the last sample, the sample count, and the skip it owes.
// Skip targets (segment starts, boundaries of empty cells) only ever grow along the ray and the skip recurrence does
// not depend on intermediate targets, so they are applied lazily: once, right before the next emission.  (A target can
// be marginally smaller than the one before it -- a cell boundary computed a rounding error before the segment start --
// and applying both in order equals applying the larger: hence the max.)
struct MarchCursor {
    float t_last;
    int n = 0;
    bool continuous = false;   // the last thing the walk met was a sample (no skip owed to the next segment's start)
    bool has_skip = false;
    float skip_to = 0.0f;
    CED_HD void push_skip(float target)
    {
        skip_to = has_skip ? fmaxf(skip_to, target) : target;
        has_skip = true;
    }
    CED_HD void empty_cell(float t_trav)       // an empty cell, which the walk leaves at t_trav
    {
        push_skip(t_trav);
        continuous = false;
    }
    CED_HD void flush_skip(const GridSpec &G)
    {
        if (has_skip) { t_last = skip_march_lattice(G, t_last, skip_to); has_skip = false; }
    }
};

// The samples of one occupied cell, which the walk leaves at t_trav (any skip owed has been marched).  True: the budget
// is used up (the walk ends; the ray stays alive).
template <class Emit>
CED_HD bool emit_cell(const GridSpec &G, MarchCursor &C, float t_trav, Emit &emit)
{
    // one exit test per sample besides the mid-point test (a return from inside the loop costs a second exit state)
    while (C.n < G.limit) {
        float t_next;
        if (G.step_size <= 0.0f) {
            t_next = t_trav;
        } else {
            const float dt = calc_dt(C.t_last, G.cone_angle, G.step_size, 1e10f);
            if (C.t_last + dt * 0.5f >= t_trav) break;
            t_next = C.t_last + dt;
        }
        emit(C.n, C.t_last, t_next);
        C.n += 1;
        C.continuous = true;
        C.t_last = t_next;
        if (t_next >= t_trav) break;
    }
    return C.n >= G.limit;
}

// Traverses one ray; emit(i, t_start, t_end) for sample i = 0..n-1 in order; returns n.  See the contract at the top of
// the file.  start_coarse: sphere-trace from the start of every segment (first iteration of a frame: most rays miss
// everything); otherwise only after a stretch of empty cells (later iterations: a live ray stands in or next to
// occupied cells).  LOOK: cells the exact walk looks ahead.  SINGLE: one grid level (decode_segment).  PHASED: the exact
// walk as a looking loop and an emission phase (a frame's first iteration: rays travel to their first occupied cell,
// each for its own number of batches); otherwise the emission inline in the batch (rays that stand inside the object
// and emit in every batch).  Same operations per ray in the same order either way.  t_hint: nothing occupied is met
// before it (the ray's group clearance; 0 or less, and the default -inf: no claim) -- the trace at a segment's start
// probes from there.
template <int LOOK, bool SINGLE, bool PHASED, class Idx, class Emit>
CED_HD int traverse_ray_frame(const GridSpec &G, const AccelSpec &S, bool start_coarse, const float (&o)[3],
                              const float (&d)[3], float near, float far, const float *__restrict__ ts_row,
                              const Idx *__restrict__ ti_row, const uint8_t *__restrict__ hit_row, Emit &&emit,
                              float &t_term, float t_hint = -__builtin_inff())
{
    const float inv_d[3] = { 1.0f / d[0], 1.0f / d[1], 1.0f / d[2] };
    const int n_grids = SINGLE ? 1 : G.n_grids, res = G.res;
    const bool accel = S.bdist != nullptr;
    MarchCursor C{ near };
    for (int i = 0; i < 2 * n_grids - 1; ++i) {
        if (C.n >= G.limit) break;
        int lvl;
        float seg_a, seg_b;
        if (!decode_segment<SINGLE>(G, o, inv_d, ts_row, ti_row, hit_row, i, lvl, seg_a, seg_b)) continue;
        const float this_tmin = fmaxf(seg_a, near);
        const float this_tmax = fminf(seg_b, far);
        if (this_tmin >= this_tmax) continue;
        if (!C.continuous) C.push_skip(this_tmin);
        const float *ab = G.aabbs + 6 * lvl;
        // A segment that starts with a sphere trace is traced BEFORE the DDA is set up: most segments of a frame's
        // first iteration are empty, and those never need the set-up (twelve divisions).  The trace itself only needs
        // the ray and the level's box; what it returns is used by the first round below, unchanged.
        bool coarse = accel && start_coarse;
        bool traced = false;
        float t_stop0 = 0.0f, cells0 = 0.0f;
        if (coarse) {
            if (coarse_advance(S, lvl, res, ab, o, d, this_tmin, this_tmax, t_stop0, cells0, t_hint)) {
                C.continuous = false;          // the whole segment is empty cells
                continue;
            }
            traced = true;
        }
        CED_DIAG_TICK(1);
        // (the set-up stays a loop of the walker's own: the first-iteration kernel of the frame renderer sits at its
        // register cap, and with the three axes behind one more call the compiler's allocation there spills)
        Dda D;
#pragma unroll
        for (int a = 0; a < 3; ++a) dda_setup_axis(D, a, res, ab, o, d, inv_d, this_tmin, this_tmax);
        dda_begin(D, res);
        const uint8_t *grid = G.binaries + (int64_t)lvl * res * res * res;
        float t_c = this_tmin;                 // the time at which the walk stands (entry of the current cell)
        // what a batch leaves behind: whether its last cell was empty, and the empty radius of the cell after it
        bool last_empty = false;
        int radius = 0;
        // Rounds of [sphere-trace] -> [closed-form re-entry] -> [exact walk until it wants to trace again].  The three
        // phases are separate loops on purpose: the lanes of a wave then spend their time in the same phase instead
        // of every lane's phase being issued on every trip of one big loop.
        while (!D.done) {
            if (coarse) {
                coarse = false;
                float t_stop = t_stop0, cells = cells0;
                if (traced) {
                    traced = false;            // the trace from the segment's start, done above
                } else if (coarse_advance(S, lvl, res, ab, o, d, t_c, this_tmax, t_stop, cells)) {
                    C.continuous = false;      // the rest of the segment is empty cells
                    break;
                }
                if (cells >= kMinJumpCells) {          // shorter stretches are cheaper walked than jumped
                    CED_DIAG_TICK(3);
                    // re-enter the exact DDA at t_stop: per axis, take every boundary crossing with T < t_stop
                    float last_event = t_c;
                    bool any = false;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        // crossings left on this axis before the walk leaves its final cell (none for d == 0: that
                        // axis is never the strict minimum before the others have ended the walk)
                        const int kcap = D.stp[a] > 0 ? D.ovf[a] - D.cur[a] : (D.stp[a] < 0 ? D.cur[a] - D.ovf[a] : 0);
                        if (kcap <= 0) continue;
                        float prev = 0.0f;
                        const int k = count_steps(D.tdist[a], D.delta[a], t_stop, kcap, prev);
                        if (k > 0) {
                            D.cur[a] += k * D.stp[a];
                            last_event = any ? fmaxf(last_event, prev) : prev;
                            any = true;
                            if (k == kcap) D.done = true;          // stepped out of the final cell: segment over
                        }
                    }
                    if (any) {
                        C.continuous = false;                       // the cells stepped over are empty
                        const float t_in = fminf(last_event, this_tmax);       // t_trav of the last of them
                        C.push_skip(t_in);
                        t_c = t_in;
                    }
                    if (D.done) break;
                }
            }
            // exact walk, LOOK cells at a time (look_ahead, load_batch)
            if constexpr (PHASED) {
                // The walk loop only LOOKS: it runs until a batch holds an occupied cell (or the walk ends / wants to
                // trace again) and leaves the batch for the emission phase below.  The lanes of a wave reach their
                // first occupied cell in different batches; with the emission inline every such batch paid a pass
                // through the emission code (the skip-march above all) for a handful of lanes -- three quarters of the
                // instructions of a frame's first iteration.
                float tt[LOOK];
                unsigned valid_mask = 0, occ_mask = 0;
                do {
                    CED_DIAG_TICK(4);
                    int cellv[LOOK];
                    uint8_t occ[LOOK];
                    valid_mask = look_ahead<LOOK>(D, res, this_tmax, tt, cellv);
                    radius = load_batch<LOOK>(grid, cellv, S, accel, D, lvl, res, occ);
                    occ_mask = 0;
#pragma unroll
                    for (int b = 0; b < LOOK; ++b) occ_mask |= occ[b] ? (1u << b) : 0u;
                    occ_mask &= valid_mask;
                    // the empty cells in front of the batch's first occupied one (all of its cells when it has none)
                    last_empty = false;
#pragma unroll
                    for (int b = 0; b < LOOK; ++b) {
                        const bool before = (valid_mask >> b & 1u) && (occ_mask & ((2u << b) - 1u)) == 0u;
                        if (before) { C.empty_cell(tt[b]); last_empty = true; t_c = tt[b]; }
                    }
                    if (occ_mask) break;
                    // in empty space with room around the cell the walk stands in: trace ahead
                    coarse = last_empty && radius >= kCoarseRadius;
                } while (!D.done && !coarse);
                if (occ_mask) {
                    // emission phase: the batch's cells from its first occupied one on, in order -- ONE copy of the code,
                    // every lane with its own cursor
                    CED_DIAG_TICK(5);
                    for (int b = __builtin_ctz(occ_mask); b < LOOK; ++b) {
                        if (!(valid_mask >> b & 1u)) break;                 // the walk ended inside the batch
                        float t_trav = tt[0];
#pragma unroll
                        for (int k = 1; k < LOOK; ++k) t_trav = b == k ? tt[k] : t_trav;
                        if (!(occ_mask >> b & 1u)) { C.empty_cell(t_trav); last_empty = true; t_c = t_trav; continue; }
                        last_empty = false;
                        C.flush_skip(G);
                        if (emit_cell(G, C, t_trav, emit)) { t_term = C.t_last; return C.n; }
                    }
                    coarse = last_empty && radius >= kCoarseRadius;
                }
            } else {
                do {
                    CED_DIAG_TICK(4);
                    float tt[LOOK];
                    int cellv[LOOK];
                    uint8_t occ[LOOK];
                    const unsigned valid_mask = look_ahead<LOOK>(D, res, this_tmax, tt, cellv);
                    radius = load_batch<LOOK>(grid, cellv, S, accel, D, lvl, res, occ);
                    last_empty = false;
#pragma unroll
                    for (int b = 0; b < LOOK; ++b) {
                        if (!(valid_mask >> b & 1u)) continue;
                        if (!occ[b]) { C.empty_cell(tt[b]); last_empty = true; t_c = tt[b]; continue; }
                        last_empty = false;
                        CED_DIAG_TICK(5);
                        C.flush_skip(G);
                        if (emit_cell(G, C, tt[b], emit)) { t_term = C.t_last; return C.n; }
                    }
                    // in empty space with room around the cell the walk stands in: trace ahead
                    coarse = last_empty && radius >= kCoarseRadius;
                } while (!D.done && !coarse);
            }
        }
    }
    t_term = C.t_last;          // n < limit: unspecified by contract (the owed skip is not marched)
    return C.n;
}

// The walk of ced_traverse_grids (march.hip): the same pieces -- decode_segment, dda_setup_axis, look_ahead,
// load_batch, emit_cell -- composed without distance fields and with the skips marched eagerly, as soon as the next
// occupied cell is known (so t_term is the termination plane of EVERY ray: that entry returns it).  A composition of
// its own because traverse_ray_frame with a null AccelSpec, which computes the same bits, measures up to 10 % slower than
// the old walker on empty grids in that kernel, this one 12-15 % faster (tools/bench_march.py).
template <class Emit>
CED_HD int traverse_ray(const GridSpec &G, const float (&o)[3], const float (&d)[3], float near, float far,
                        const float *__restrict__ ts_row, const int64_t *__restrict__ ti_row,
                        const uint8_t *__restrict__ hit_row, Emit &&emit, float &t_term)
{
    const float inv_d[3] = { 1.0f / d[0], 1.0f / d[1], 1.0f / d[2] };
    const int res = G.res;
    const AccelSpec none{ nullptr, 0, nullptr };
    MarchCursor C{ near };
    // A segment that ends in empty cells owes one skip-march to its last empty boundary.  It is deferred to the next
    // processed segment (or to the end of the call): the t_last sequence is the same.
    bool owed = false;
    float owed_to = 0.0f;
    for (int i = 0; i < 2 * G.n_grids - 1; ++i) {
        if (C.n >= G.limit) break;
        int lvl;
        float seg_a, seg_b;
        if (!decode_segment<false>(G, o, inv_d, ts_row, ti_row, hit_row, i, lvl, seg_a, seg_b)) continue;
        const float this_tmin = fmaxf(seg_a, near);
        const float this_tmax = fminf(seg_b, far);
        if (this_tmin >= this_tmax) continue;
        if (owed) { C.t_last = skip_march(C.t_last, owed_to, G.step_size, G.cone_angle); owed = false; }
        if (!C.continuous) C.t_last = skip_march(C.t_last, this_tmin, G.step_size, G.cone_angle);
        const float *ab = G.aabbs + 6 * lvl;
        Dda D;
#pragma unroll
        for (int a = 0; a < 3; ++a) dda_setup_axis(D, a, res, ab, o, d, inv_d, this_tmin, this_tmax);
        dda_begin(D, res);
        const uint8_t *grid = G.binaries + (int64_t)lvl * res * res * res;
        // Runs of empty cells only remember the farthest boundary; the skip-march to it happens once, before the next
        // occupied cell or at the end -- the same t_last sequence as marching cell by cell, because the recurrence
        // t_last += dt does not depend on where the intermediate boundaries are.
        bool stop = false, has_pending = false;
        float pending = 0.0f;
        while (!D.done && !stop) {
            float tt[kLook];
            int cellv[kLook];
            uint8_t occ[kLook];
            const unsigned valid_mask = look_ahead<kLook>(D, res, this_tmax, tt, cellv);
            (void)load_batch<kLook>(grid, cellv, none, false, D, lvl, res, occ);
#pragma unroll
            for (int b = 0; b < kLook; ++b) {
                if (!(valid_mask >> b & 1u) || stop) continue;
                if (!occ[b]) {
                    pending = tt[b];
                    has_pending = true;
                    C.continuous = false;
                    continue;
                }
                if (has_pending) {
                    C.t_last = skip_march(C.t_last, pending, G.step_size, G.cone_angle);
                    has_pending = false;
                }
                stop = emit_cell(G, C, tt[b], emit);
            }
        }
        if (has_pending) { owed = true; owed_to = pending; }
    }
    if (owed) C.t_last = skip_march(C.t_last, owed_to, G.step_size, G.cone_angle);
    t_term = C.t_last;
    return C.n;
}

}  // namespace ced
