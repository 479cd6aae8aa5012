// The pieces of the occupancy-grid march that do not know about cells: the sample recurrence and its skip marches, the
// grid description, the ray/box slab test and the decoder of a ray's sorted entry / exit events into segments.  The
// walker itself -- ONE, for the nerfacc-shaped kernels (march.hip) and the frame renderer (frame.hip) -- is in
// march_accel.hpp.  Restates nerfacc.traverse_grids (un-vendored CUDA op; call sites cednerf/utils.py:241-264 and,
// through OccGridEstimator.sampling, cednerf/utils.py:115-125).
// Every float operation is a single IEEE op in a fixed order (-ffp-contract=off): sample boundaries are bit-exact with
// the CPU oracle -- do not "simplify" the arithmetic.  Host and device code: the CPU test-suite runs all of it.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define CED_HD __host__ __device__ __forceinline__
#else
#define CED_HD inline
#endif

namespace ced {

CED_HD float bits_to_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
CED_HD uint32_t float_to_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

CED_HD float calc_dt(float t, float cone_angle, float dt_min, float dt_max)
{
    float v = t * cone_angle;
    return fminf(fmaxf(v, dt_min), dt_max);
}

// The reference recurrence: advance t in whole steps until the next step's mid-point reaches
// `target` (nerfacc: "march until t_mid is right after t_traverse").
CED_HD float skip_march_sequential(float t_last, float target, float step_size, float cone_angle)
{
    if (step_size <= 0.0f) return target;
    for (;;) {
        float dt = calc_dt(t_last, cone_angle, step_size, 1e10f);
        if (t_last + dt * 0.5f >= target) break;
        t_last += dt;
    }
    return t_last;
}

// The float recurrence x_{j+1} = fl(x_j + d) inside one binade [2^e, 2^(e+1)): every x there is a multiple of u = ulp,
// so the add moves x by the same whole number of ulps each time (d = q*u + r rounds to q or q+1 ulps, the same way for
// every x of the binade, unless r is exactly u/2): the recurrence is an exact arithmetic progression of the integer
// mantissas, x_j = (X + j*INC) * u, while it stays below 2^24.  term(j) is x_j as a float.
struct Binade {
    uint32_t ex, X, INC;       // exponent bits of the binade; mantissa of x (hidden bit set); ulps per add
    CED_HD float term(uint32_t j) const { return bits_to_float(ex | ((X + j * INC) & 0x7fffffu)); }
};

// x1 = fl(x + d).  True when the progression holds from x: x and x1 are positive normal numbers of one binade, the add
// moves x, and it is not the tie case.  Everything else (binade crossings, the tie, tiny or huge x) takes real single
// adds at the caller.
CED_HD bool regular_binade(float x, float x1, float d, Binade &B)
{
    const uint32_t bx = float_to_bits(x), b1 = float_to_bits(x1);
    const uint32_t ex = bx & 0x7f800000u;
    const bool regular = (ex == (b1 & 0x7f800000u)) && (bx >> 31) == 0 && ex > (24u << 23) && ex < (254u << 23);
    if (!regular) return false;
    const float inc = x1 - x;                            // exact: both are multiples of u in one binade
    const float err = d - inc;                           // exact rounding error of the add
    const float u = bits_to_float(ex - (23u << 23));     // ulp of the binade
    if (!(inc > 0.0f && fabsf(err) != 0.5f * u)) return false;
    B.ex = ex;
    B.X = (bx & 0x7fffffu) | 0x800000u;
    B.INC = (uint32_t)(inc / u);                         // exact (power-of-two scaling)
    return true;
}

// Same result as skip_march_sequential for cone_angle == 0, in O(#binades) instead of O(#steps): inside a regular
// binade the index is estimated by an integer division and settled by the exact float predicate fl(t_j + h) >= target.
// (No double precision: this runs once per ray and iteration on the device.)
CED_HD float skip_march_const_step(float t, float target, float step)
{
    const float h = step * 0.5f;
    if (!(target == target)) return t;                       // NaN target (degenerate ray): nothing to march to
    for (;;) {
        if (t + h >= target) return t;
        const float t1 = t + step;
        if (t1 == t) return t;               // the step no longer moves t (t beyond 2^24 steps): the lattice ends here
        Binade B;
        if (regular_binade(t, t1, step, B)) {
            const uint32_t X = B.X, INC = B.INC;
            // J = last index whose term is still inside the binade
            const uint32_t BJ = 0xffffffu - X;
            uint32_t J = (uint32_t)((float)BJ / (float)INC);
            if (J * INC > BJ) --J;
            if ((J + 1u) * INC <= BJ) ++J;
            // estimate of the first j with t_j >= target - h, then the exact predicate settles it
            const float A = target - h;
            uint32_t j = J;
            if (A < bits_to_float(B.ex + (1u << 23))) {
                j = 0;
                if (A > t) {                              // same binade as t
                    const uint32_t BA = ((float_to_bits(A) & 0x7fffffu) | 0x800000u) - X;     // >= 1
                    uint32_t q = (uint32_t)((float)(BA - 1u) / (float)INC);
                    if (q * INC > BA - 1u) --q;
                    if ((q + 1u) * INC <= BA - 1u) ++q;
                    j = q + 1u;                           // ceil(BA / INC)
                    if (j > J) j = J;
                }
            }
            while (j > 0u && (B.term(j - 1u) + h >= target)) --j;
            while (j < J && !(B.term(j) + h >= target)) ++j;
            t = B.term(j);
            if (t + h >= target) return t;
            t = t + step;                                 // j == J: the step that leaves the binade, for real
            continue;
        }
        t = t1;
    }
}

CED_HD float skip_march(float t_last, float target, float step_size, float cone_angle)
{
    if (step_size > 0.0f && cone_angle == 0.0f) return skip_march_const_step(t_last, target, step_size);
    return skip_march_sequential(t_last, target, step_size, cone_angle);
}

CED_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct GridSpec {
    const uint8_t *binaries;   // [n_grids, res, res, res] bytes
    const float *aabbs;        // [n_grids, 6]
    int n_grids, res;
    float step_size, cone_angle;
    int limit;                 // samples per ray and call, >= 1 (the entry points pass 0x7fffffff for "unlimited")
    const float *lattice = nullptr;   // frame renderer, cone_angle == 0: first lattice point per binade (march_accel.hpp)
};

constexpr int kBrick = 8;      // cells per brick side

// nerfacc.ray_aabb_intersect with near = -inf, far = +inf (cednerf/utils.py:215), one ray and one box
CED_HD bool slab_test(const float (&o)[3], const float (&inv_d)[3], const float *__restrict__ aabb, float &tmin_out,
                      float &tmax_out)
{
    float tmin, tmax, tymin, tymax, tzmin, tzmax;
    if (inv_d[0] >= 0) { tmin = (aabb[0] - o[0]) * inv_d[0]; tmax = (aabb[3] - o[0]) * inv_d[0]; }
    else               { tmin = (aabb[3] - o[0]) * inv_d[0]; tmax = (aabb[0] - o[0]) * inv_d[0]; }
    if (inv_d[1] >= 0) { tymin = (aabb[1] - o[1]) * inv_d[1]; tymax = (aabb[4] - o[1]) * inv_d[1]; }
    else               { tymin = (aabb[4] - o[1]) * inv_d[1]; tymax = (aabb[1] - o[1]) * inv_d[1]; }
    // A ray that lies in a face plane of the box (d_a == 0 and o_a on the plane) makes 0 * inf = NaN bounds on that axis;
    // NaN compares false below and would drop an end of the interval (t_min = -inf or t_max = +inf: samples outside
    // every box, or none behind a fine box).  The box is closed: such a ray is inside that slab for all t.
    if (tmin != tmin) tmin = -__builtin_inff();
    if (tmax != tmax) tmax = __builtin_inff();
    if (tymin != tymin) tymin = -__builtin_inff();
    if (tymax != tymax) tymax = __builtin_inff();
    if (tmin > tymax || tymin > tmax) return false;
    if (tymin > tmin) tmin = tymin;
    if (tymax < tmax) tmax = tymax;
    if (inv_d[2] >= 0) { tzmin = (aabb[2] - o[2]) * inv_d[2]; tzmax = (aabb[5] - o[2]) * inv_d[2]; }
    else               { tzmin = (aabb[5] - o[2]) * inv_d[2]; tzmax = (aabb[2] - o[2]) * inv_d[2]; }
    if (tzmin != tzmin) tzmin = -__builtin_inff();
    if (tzmax != tzmax) tzmax = __builtin_inff();
    if (tmin > tzmax || tzmin > tmax) return false;
    if (tzmin > tmin) tmin = tzmin;
    if (tzmax < tmax) tmax = tzmax;
    if (tmax <= 0) return false;
    tmin_out = tmin;
    tmax_out = tmax;
    return true;
}

// Segment i of a ray: the stretch between its sorted entry / exit events i and i + 1 (cednerf/utils.py:219-225; event
// ids < n_grids enter that level, the others leave level id - n_grids), which lies in level `lvl` and spans
// [seg_a, seg_b] before the near / far clamp.  False: no such stretch (a level the ray misses, or the gap between
// leaving one level and entering another).  SINGLE: one grid level -- the only segment is the ray/box interval, which
// is recomputed here with the set-up kernel's arithmetic instead of being loaded (the rows are unused).  Idx: event ids
// are int64 in nerfacc's layout, bytes in the frame renderer's.
template <bool SINGLE, class Idx>
CED_HD bool decode_segment(const GridSpec &G, const float (&o)[3], const float (&inv_d)[3],
                           const float *__restrict__ ts_row, const Idx *__restrict__ ti_row,
                           const uint8_t *__restrict__ hit_row, int i, int &lvl, float &seg_a, float &seg_b)
{
    lvl = 0;
    if constexpr (SINGLE) {
        return slab_test(o, inv_d, G.aabbs, seg_a, seg_b);
    } else {
        const int n_grids = G.n_grids;
        const int ti = (int)ti_row[i];
        const bool entering = ti < n_grids;
        lvl = (int)(ti % n_grids);
        if (!hit_row[lvl]) return false;
        if (!entering) {
            const int tn = (int)ti_row[i + 1];
            if (tn < n_grids) return false;
            lvl = (int)(tn % n_grids);
            if (!hit_row[lvl]) return false;
        }
        seg_a = ts_row[i];
        seg_b = ts_row[i + 1];
        return true;
    }
}

}  // namespace ced
