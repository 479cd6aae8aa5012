// The density's maximum over windows of time: ced_field_density_time_max hands out, from one launch,
//     out[b, p] = fmaxf over s = 0 .. S-1 of sigma(positions[p], times[b * S + s]),   started from 0.0f,
// sigma with ced_field_forward's bits in the descriptor's arithmetic (include/cednerf_hip.h states the rules).  It is what
// builds the time slices of an occupancy grid (nerfacc_api.TimeSlicedOccGrid): cells x bins x probe times density
// evaluations of which only positions, times and the B maxima per cell touch HBM besides the table gathers.
//
// Shape: tile_kernel<TimeMaxOp, W, NT, 512> of field_move_device.hpp, one more op on that skeleton.
//   as GradientOp (field_density_gradient.hip), through field_density_device.hpp: the staged plane W is the motion network
//     AND mlp_base, the sixteen levels' constants sit in LDS beside it, one workgroup per CU; canonical_point, gather_levels
//     and mlp_base are the functions GradientOp calls, here on NT primal tiles and no tangent tile;
//   from TrackOp (field_move.hip): a wave tile loads its rows' positions once and keeps them, and the running maxima, in
//     registers; the loop calls the motion network's device function on an opaque LDS base per round.
// The loop runs over b, s.  All rows of a tile share the time of an iteration (SharedTime): the fp32 chain's two time
// features per lane and the temporal table's key-frame are formed once per iteration, not per row; an iteration whose time
// is the previous iteration's (bin b's first probe is bin b - 1's last in TimeSlicedOccGrid.probe_times) reuses the densities
// in registers.  out[b * n + row] is stored once per bin, by lane group 0.
// Per 16-row tile and iteration: motion_move, x_norm / selector / |move|, the lane's four levels through hash_level (index
// forms 0 / 2), mlp_base, trunc_exp.  NT and the registers per arithmetic: DESIGN 4.1f.
#include "field_density_device.hpp"

namespace ced {

struct TimeMaxArgs : DensityArgs {
    int64_t n;                                        // rows (positions)
    const float *pos, *times;                         // [n,3], [n_bins * n_times]
    float *out;                                       // [n_bins, n]
    int n_bins, n_times;
};

// the time of an iteration, shared by every row of the tile: HeldTime with one value and one pair of features
struct SharedTime {
    float t, tf[2];
    __device__ __forceinline__ float value(int) const { return t; }
    __device__ __forceinline__ void features(int, int, float &f0, float &f1) const { f0 = tf[0]; f1 = tf[1]; }
};

// ---- ced_field_density_time_max: NT 16-row tiles per wave, held in registers across the bins ------------------------------
template <bool TE, bool F16, bool TEMPORAL> struct TimeMaxOp : TileOp, DensityLevels<F16, TEMPORAL> {
    using Args = TimeMaxArgs;
    using DensityLevels<F16, TEMPORAL>::levels;
    using DensityLevels<F16, TEMPORAL>::fill_lds;
    static constexpr int kPerCu = 1;
    // 16-row tiles per wave iteration: two, with no tangent tiles beside them -- except on an fp32 temporal table, whose
    // 16-byte corner loads (two key-frames each) hold 32 more registers per tile: two tiles reach 256 VGPRs and spill
    // (DESIGN 4.1f has the cross-compiled counts)
    static constexpr int kTiles = (TEMPORAL && !F16) ? 1 : 2;

    // sigma of the tile's rows at time tq, on lane group 3 (every lane computes the selector of its column's rows)
    template <typename W, int NT>
    __device__ __forceinline__ static void density(const TimeMaxArgs &A, const typename W::Elem *w, int lane, const float (&px)[NT][3],
                                                   float tq, float (&sigma)[NT])
    {
        const int g = lane >> 4;
        SharedTime time{ tq, { 0.0f, 0.0f } };
        if constexpr (!W::kHalf) time_features(tq, g, time.tf[0], time.tf[1]);
        float mv[NT][3];
        motion_move<W, NT>(w, lane, px, time, A.moving_step, A.use_div, mv);

        float xn[NT][3], mnorm[NT];
        bool sel[NT];
        canonical_point<TE, NT>(A.aabb, px, mv, xn, sel, mnorm);

        float R[NT][8];
        int k_lo = 0;
        float t_frac = 0.0f;
        if constexpr (TEMPORAL) temporal_keyframe(tq, k_lo, t_frac);
        gather_levels<W, F16, TEMPORAL, NT>(A, levels(), g, xn, k_lo, t_frac, R);

        float raw[NT], no_tangent[1][8], no_draw[1];
        mlp_base<W, TE, NT, 0>(A, w, lane, R, no_tangent, tq, mnorm, raw, no_draw);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const float sg = det_expf(raw[j] - 1.0f);
            sigma[j] = sel[j] ? sg : 0.0f;
        }
    }

    // w = the tile's LDS base of the staged layers
    template <typename W, int NT>
    __device__ __forceinline__ static void tile(const TimeMaxArgs &A, const Shared &, const typename W::Elem *w, int64_t tile_base,
                                                int64_t, int lane)
    {
        const int g = lane >> 4, c = lane & 15;
        float px[NT][3];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            int64_t s = tile_base + 16 * j + c;
            s = s < A.n ? s : A.n - 1;                                   // a ragged last tile repeats the last row (never stored)
#pragma unroll
            for (int a = 0; a < 3; ++a) px[j][a] = A.pos[3 * s + a];
        }
        // A probe time equal, bit for bit, to the one before it (neighbouring bins share their end time) is not evaluated
        // again: the density held from the last iteration IS its value.  The comparison is wave-uniform.
        float sigma[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) sigma[j] = 0.0f;
        uint32_t t_held = 0;
        bool held = false;
        for (int b = 0; b < A.n_bins; ++b) {
            float mx[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) mx[j] = 0.0f;
            for (int s = 0; s < A.n_times; ++s) {
                const float tq = A.times[b * A.n_times + s];             // wave-uniform
                if (!(held && __float_as_uint(tq) == t_held)) density<W, NT>(A, opaque(w), lane, px, tq, sigma);
                t_held = __float_as_uint(tq);
                held = true;
#pragma unroll
                for (int j = 0; j < NT; ++j) mx[j] = fmaxf(mx[j], sigma[j]);   // a NaN density is ignored
            }
            // lane group 3 holds row c's maximum; lane group 0 takes and stores it
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const float m = __shfl(mx[j], 48 + c, 64);
                const int64_t row = tile_base + 16 * j + c;
                if (g == 0 && row < A.n) A.out[(int64_t)b * A.n + row] = m;
            }
        }
    }
};

}  // namespace ced

extern "C" int ced_field_density_time_max(const ced_field_desc *desc, int64_t n, const float *positions, int32_t n_bins,
                                          int32_t n_times, const float *times, float *out, void *stream)
{
    using namespace ced;
    const char *who = "field_density_time_max";
    int rc = validate_desc(desc, who);
    if (rc) return rc;
    CED_REQUIRE(n >= 0, "%s: n < 0", who);
    CED_REQUIRE(n_bins >= 1 && n_bins <= CED_TIME_MAX_BINS, "%s: n_bins=%d outside 1 .. %d", who, n_bins, CED_TIME_MAX_BINS);
    CED_REQUIRE(n_times >= 1 && n_times <= CED_TIME_MAX_TIMES, "%s: n_times=%d outside 1 .. %d", who, n_times, CED_TIME_MAX_TIMES);
    if (n == 0) return CED_OK;
    CED_REQUIRE(positions && times && out, "%s: null positions/times/out", who);
    TimeMaxArgs A{};
    rc = fill_density_args(desc, A, who);
    if (rc) return rc;
    A.n = n;
    A.pos = positions; A.times = times; A.out = out;
    A.n_bins = n_bins; A.n_times = n_times;
    return launch_density<TimeMaxOp>(desc, A, who, stream);
}
