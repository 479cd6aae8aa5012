// Bisection on the density along a ray, fused: ced_field_level_set takes per row a ray o + d * t and a bracket [lo, hi]
// and returns where the density first reaches `thresh` inside it, to float32 resolution, from one launch
// (include/cednerf_hip.h states the rules and every fp32 operation).  sigma has ced_field_forward's bits in the
// descriptor's arithmetic.  It is what utils.render_surface and export.refine_mesh locate the surface with: per round only
// the hash table's gathers touch device memory, where the unfused loop writes and reads positions and densities.
//
// Shape: tile_kernel<LevelSetOp, W, NT, 512> of field_move_device.hpp, one more op on that skeleton.
//   as TimeMaxOp (field_time_max.hip), through field_density_device.hpp: the staged plane W is the motion network AND
//     mlp_base, the sixteen levels' constants sit in LDS beside it, one workgroup per CU; motion_move, canonical_point,
//     gather_levels and mlp_base are the functions TimeMaxOp::density calls.  Here every row has a time of its own
//     (HeldTime: the fp32 chain's time features are made once per tile), so the key-frame of a temporal table and
//     mlp_base's time features are per tile: gather_levels and mlp_base run on one primal tile at a time.  MFMA columns do
//     not mix: each tile's sigma is ced_field_forward's whatever stands beside it.
//   from TrackOp (field_move.hip): a wave tile loads its rows once and keeps them, the bracket and the verdicts in
//     registers; the loop takes an opaque LDS base per round, a finished row is frozen, and the loop is left when the ballot
//     finds no active row in the wave.
// NT and the registers per arithmetic: DESIGN 4.1g.
#include "field_density_device.hpp"

namespace ced {

struct LevelSetArgs : DensityArgs {
    int64_t n;                                        // rows
    const float *origins, *dirs, *lo, *hi, *times;    // [n,3], [n,3], [n], [n], [n] or [1]
    int t_per_row;
    float thresh, tol;
    int max_iters;
    float *t, *x, *sigma, *width;                     // [n], [n,3], [n], [n]; any may be null
    int32_t *status, *evals;                          // [n]; either may be null
};

// ---- ced_field_level_set: NT 16-row tiles per wave, held in registers across the rounds ------------------------------------
template <bool TE, bool F16, bool TEMPORAL> struct LevelSetOp : TileOp, DensityLevels<F16, TEMPORAL> {
    using Args = LevelSetArgs;
    using DensityLevels<F16, TEMPORAL>::levels;
    using DensityLevels<F16, TEMPORAL>::fill_lds;
    static constexpr int kPerCu = 1;
    // 16-row tiles per wave iteration: two, as TimeMaxOp -- except on a temporal table of either entry type.  The bracket,
    // the ray and the three densities a row keeps across the rounds are 13 registers per tile more than TimeMaxOp holds,
    // and on the fp16 temporal table with a time encoding two tiles reach 256 VGPRs on the fp32 chain and spill
    // (DESIGN 4.1g has the cross-compiled counts)
    static constexpr int kTiles = TEMPORAL ? 1 : 2;

    // p = o + d * t per axis: a multiply, then an add
    template <int NT>
    __device__ __forceinline__ static void point(const float (&o)[NT][3], const float (&d)[NT][3], const float (&t)[NT],
                                                 float (&px)[NT][3])
    {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
#pragma unroll
            for (int a = 0; a < 3; ++a) px[j][a] = __fadd_rn(o[j][a], __fmul_rn(d[j][a], t[j]));
        }
    }

    // sigma of the tile's rows at their own times, on every lane (0 outside the box)
    template <typename W, int NT>
    __device__ __forceinline__ static void density(const LevelSetArgs &A, const typename W::Elem *w, int lane, const float (&px)[NT][3],
                                                   const HeldTime<NT> &time, float (&sigma)[NT])
    {
        const int g = lane >> 4, c = lane & 15;
        float mv[NT][3];
        motion_move<W, NT>(w, lane, px, time, A.moving_step, A.use_div, mv);

        float xn[NT][3], mnorm[NT];
        bool sel[NT];
        canonical_point<TE, NT>(A.aabb, px, mv, xn, sel, mnorm);

#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const float tq = time.value(j);
            const float xn1[1][3] = { { xn[j][0], xn[j][1], xn[j][2] } };
            const float mnorm1[1] = { mnorm[j] };
            float R[1][8];
            int k_lo = 0;
            float t_frac = 0.0f;
            if constexpr (TEMPORAL) temporal_keyframe(tq, k_lo, t_frac);
            gather_levels<W, F16, TEMPORAL, 1>(A, levels(), g, xn1, k_lo, t_frac, R);

            float raw[1], no_tangent[1][8], no_draw[1];
            mlp_base<W, TE, 1, 0>(A, w, lane, R, no_tangent, tq, mnorm1, raw, no_draw);
            const float sg = det_expf(raw[0] - 1.0f);
            sigma[j] = __shfl(sel[j] ? sg : 0.0f, 48 + c, 64);          // lane group 3 holds row c's raw density
        }
    }

    // w = the tile's LDS base of the staged layers
    template <typename W, int NT>
    __device__ __forceinline__ static void tile(const LevelSetArgs &A, const Shared &, const typename W::Elem *w, int64_t tile_base,
                                                int64_t, int lane)
    {
        const int g = lane >> 4, c = lane & 15;
        float o[NT][3], d[NT][3], lo[NT], hi[NT], tq[NT];
        bool active[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int64_t row = tile_base + 16 * j + c;
            const int64_t s = row < A.n ? row : A.n - 1;                 // a ragged last tile repeats the last row (never stored)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                o[j][a] = A.origins[3 * s + a];
                d[j][a] = A.dirs[3 * s + a];
            }
            lo[j] = A.lo[s];
            hi[j] = A.hi[s];
            tq[j] = A.times[A.t_per_row ? s : 0];
            active[j] = row < A.n;
        }
        const HeldTime<NT> time = hold_time<W, NT>(tq, g);

        // the endpoint verdicts
        float px[NT][3], s_lo[NT], s_hi[NT];
        point<NT>(o, d, lo, px);
        density<W, NT>(A, opaque(w), lane, px, time, s_lo);
        point<NT>(o, d, hi, px);
        density<W, NT>(A, opaque(w), lane, px, time, s_hi);
        int status[NT], evals[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            status[j] = s_lo[j] >= A.thresh ? 1 : (!(s_hi[j] >= A.thresh) ? 2 : 0);
            evals[j] = 2;
            active[j] = active[j] && status[j] == 0;
        }

        // the rounds: a row that has stopped is frozen; the loop bound is wave-uniform
        for (int it = 0; it < A.max_iters; ++it) {
            float m[NT], s_m[NT];
            bool any = false;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const float width = __fsub_rn(hi[j], lo[j]);
                m[j] = __fadd_rn(lo[j], hi[j]) / 2.0f;
                const bool stop = width <= A.tol || m[j] == lo[j] || m[j] == hi[j];
                active[j] = active[j] && !stop;
                any = any || active[j];
            }
            if (__ballot(any) == 0) break;                               // wave-uniform
            point<NT>(o, d, m, px);
            density<W, NT>(A, opaque(w), lane, px, time, s_m);
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const bool up = active[j] && s_m[j] >= A.thresh;         // a NaN goes to lo
                const bool down = active[j] && !up;
                hi[j] = up ? m[j] : hi[j];
                s_hi[j] = up ? s_m[j] : s_hi[j];
                lo[j] = down ? m[j] : lo[j];
                evals[j] += active[j] ? 1 : 0;
            }
        }

        // lane group a < 3 stores component a of x, lane group 3 the rest
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int64_t s = tile_base + 16 * j + c;
            const bool inside = status[j] == 1;
            const float t_out = inside ? lo[j] : hi[j];
            const float sg_out = inside ? s_lo[j] : s_hi[j];
            const float w_out = inside ? 0.0f : __fsub_rn(hi[j], lo[j]);
            const float x0 = __fadd_rn(o[j][0], __fmul_rn(d[j][0], t_out));
            const float x1 = __fadd_rn(o[j][1], __fmul_rn(d[j][1], t_out));
            const float x2 = __fadd_rn(o[j][2], __fmul_rn(d[j][2], t_out));
            const float xg = (g == 0) ? x0 : (g == 1) ? x1 : x2;
            if (s >= A.n) continue;
            if (g == 3) {
                if (A.t) A.t[s] = t_out;
                if (A.sigma) A.sigma[s] = sg_out;
                if (A.width) A.width[s] = w_out;
                if (A.status) A.status[s] = status[j];
                if (A.evals) A.evals[s] = evals[j];
                continue;
            }
            if (A.x) A.x[3 * s + g] = xg;
        }
    }
};

}  // namespace ced

extern "C" int ced_field_level_set(const ced_field_desc *desc, int64_t n, const float *origins, const float *dirs,
                                   const float *lo, const float *hi, const float *times, int32_t t_per_row, float thresh,
                                   int32_t max_iters, float tol, float *t, float *x, float *sigma, float *width,
                                   int32_t *status, int32_t *evals, void *stream)
{
    using namespace ced;
    const char *who = "field_level_set";
    int rc = validate_desc(desc, who);
    if (rc) return rc;
    CED_REQUIRE(n >= 0, "%s: n < 0", who);
    CED_REQUIRE(max_iters >= 0 && max_iters <= CED_LEVEL_SET_MAX_ITERS, "%s: max_iters=%d outside 0 .. %d", who, max_iters,
                CED_LEVEL_SET_MAX_ITERS);
    CED_REQUIRE(thresh > 0.0f, "%s: thresh=%g must be > 0 (and not a NaN)", who, (double)thresh);
    CED_REQUIRE(tol >= 0.0f, "%s: tol=%g must be >= 0 (and not a NaN)", who, (double)tol);
    if (n == 0) return CED_OK;
    CED_REQUIRE(origins && dirs && lo && hi && times, "%s: null origins/dirs/lo/hi/times", who);
    CED_REQUIRE(t || x || sigma || width || status || evals, "%s: no output requested", who);
    LevelSetArgs A{};
    rc = fill_density_args(desc, A, who);
    if (rc) return rc;
    A.n = n;
    A.origins = origins; A.dirs = dirs; A.lo = lo; A.hi = hi; A.times = times;
    A.t_per_row = t_per_row ? 1 : 0;
    A.thresh = thresh; A.tol = tol; A.max_iters = max_iters;
    A.t = t; A.x = x; A.sigma = sigma; A.width = width; A.status = status; A.evals = evals;
    return launch_density<LevelSetOp>(desc, A, who, stream);
}
