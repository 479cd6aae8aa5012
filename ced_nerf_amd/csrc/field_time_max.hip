// The density's maximum over windows of time: ced_field_density_time_max hands out, from one launch,
//     out[b, p] = fmaxf over s = 0 .. S-1 of sigma(positions[p], times[b * S + s]),   started from 0.0f,
// sigma with ced_field_forward's bits in the descriptor's arithmetic (include/cednerf_hip.h states the rules).  It is what
// builds the time slices of an occupancy grid (nerfacc_api.TimeSlicedOccGrid): cells x bins x probe times density
// evaluations of which only positions, times and the B maxima per cell touch HBM besides the table gathers.
//
// Shape: tile_kernel<TimeMaxOp, W, NT, 512> of field_move_device.hpp, one more op on that skeleton.
//   from GradientOp (field_density_gradient.hip): the staged plane W is the motion network AND mlp_base, the sixteen
//     levels' constants sit in LDS beside it (fill_lds), one workgroup per CU;
//   from TrackOp (field_move.hip): a wave tile loads its rows' positions once and keeps them, and the running maxima, in
//     registers; the loop calls the motion network's device function on an opaque LDS base per round.
// The loop runs over b, s.  All rows of a tile share the time of an iteration (SharedTime): the fp32 chain's two time
// features per lane and the temporal table's key-frame are formed once per iteration, not per row; an iteration whose time
// is the previous iteration's (bin b's first probe is bin b - 1's last in TimeSlicedOccGrid.probe_times) reuses the densities
// in registers.  out[b * n + row] is stored once per bin, by lane group 0.
// mlp_base is primal-only here (base_density_f32 / base_density_half): the siblings of field_density_gradient.hip's
// base_gradient_* without the three tangent tiles, the same layer functions on the same operand placement, so GradientOp's
// generated code is untouched and no tangent is computed to be thrown away.  Per 16-row tile and iteration: motion_move,
// x_norm / selector / |move| as the fused kernels form them, the lane's four levels through hash_level (index forms 0 / 2,
// as GradientOp reads them), mlp_base, trunc_exp.  NT and the registers per arithmetic: DESIGN 4.1f.
#include "field_args.hpp"
#include "field_move_device.hpp"
#include "hash_device.hpp"

namespace ced {

struct TimeMaxArgs {
    int64_t n;                                        // rows (positions)
    const float *pos, *times;                         // [n,3], [n_bins * n_times]
    float *out;                                       // [n_bins, n]
    int n_bins, n_times;
    float aabb[6];
    float moving_step;
    int use_div, time_mode;
    int raw_reg;                                      // fp32 chain: the raw density's register on lane group 3 (mixed blob: 3)
    const void *weights;
    int64_t lo_halves;
    int level_mode;                                   // 2 bits per gather slot: 2 = all four levels hashed, else 0
    const void *table;
    HashLevels levels;
};

// the time of an iteration, shared by every row of the tile: HeldTime with one value and one pair of features
struct SharedTime {
    float t, tf[2];
    __device__ __forceinline__ float value(int) const { return t; }
    __device__ __forceinline__ void features(int, int, float &f0, float &f1) const { f0 = tf[0]; f1 = tf[1]; }
};

// mlp_base on the fp32 MFMA chain (CED_MLP_F32, CED_MLP_F32_HEAD16X2): R[j] are the lane's gathered features of tile j
// (slot i = level 4i + 2(g&1) + (g>>1)); out: the raw density on lane group 3
template <bool TE, int NT>
__device__ __forceinline__ void base_density_f32(const TimeMaxArgs &A, const float *lw, int lane, const float (&R)[NT][8], float tq,
                                                 const float (&mnorm)[NT], float (&raw)[NT])
{
    using BL = Blob<TE>;
    const int g = lane >> 4;
    float B[NT][16];
    f4 D[NT][4];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        // operand element (k-step S, group g) is feature g&1 of level 2S + (g>>1): field_kernel.hpp's swap
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(R[j][2 * i]), __float_as_uint(R[j][2 * i + 1]), false, false);
            B[j][2 * i] = __uint_as_float(sw[0]);
            B[j][2 * i + 1] = __uint_as_float(sw[1]);
        }
#pragma unroll
        for (int S = 8; S < 16; ++S) B[j][S] = (TE && S < 11) ? time_feature(4 * (S - 8) + g, A.time_mode, tq, mnorm[j]) : 0.0f;
    }
    mlp_layer<BL::KS_B0, 4, NT>(lw + BL::B0, lane, B, D);
    to_operand<4, true, NT>(D, B);
    mlp_layer<16, 1, NT>(lw + BL::B1, lane, B, D);
    // named values first: a select between vector elements by a run-time index would go through memory
    const bool last = A.raw_reg != 0;
#pragma unroll
    for (int j = 0; j < NT; ++j) raw[j] = last ? D[j][0][3] : D[j][0][0];
}

// mlp_base on the fp16 MFMAs (CED_MLP_F16, CED_MLP_F16X2; K32: the blob has half_kernel_k32's placements): slot i = level
// 4i + g, features at operand elements 2i, 2i + 1 (field_half.hip); the raw density is row 15 = (lane group 3, register 3)
template <bool TE, bool SPLIT, bool K32, int NT>
__device__ __forceinline__ void base_density_half(const TimeMaxArgs &A, const _Float16 *whi, const _Float16 *wlo, int lane,
                                                  const float (&R)[NT][8], float tq, const float (&mnorm)[NT], float (&raw)[NT])
{
    using BL = HalfBlob<TE>;
    const int g = lane >> 4;
    h8 Bh[NT][2], Bl[NT][2];
    f4 D[NT][4];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = __builtin_amdgcn_fmed3f(R[j][e], -kHalfMax, kHalfMax);
        to_half8<SPLIT>(v, Bh[j][0], Bl[j][0]);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (TE && e < 3) ? time_feature(4 * e + g, A.time_mode, tq, mnorm[j]) : 0.0f;
        to_half8<SPLIT>(v, Bh[j][1], Bl[j][1]);
    }
    mlp_layer_h<BL::KS_B0, 4, NT, SPLIT>(whi + BL::B0 * kFragHalves, wlo + BL::B0 * kFragHalves, lane, Bh, Bl, D);
    to_operand_h<NT, SPLIT>(D, Bh, Bl);
    hidden_fed_layer<2, 1, NT, SPLIT, K32>(whi + BL::B1 * kFragHalves, wlo + BL::B1 * kFragHalves, lane, Bh, Bl, D);
#pragma unroll
    for (int j = 0; j < NT; ++j) raw[j] = D[j][0][3];
}

// ---- ced_field_density_time_max: NT 16-row tiles per wave, held in registers across the bins ------------------------------
template <bool TE, bool F16, bool TEMPORAL> struct TimeMaxOp : TileOp {
    using Args = TimeMaxArgs;
    static constexpr int kPerCu = 1;

    // the sixteen levels' constants, in LDS beside the staged layers
    __device__ __forceinline__ static uint32_t *levels()
    {
        __shared__ __attribute__((aligned(16))) uint32_t table[8 * CED_MAX_LEVELS];
        return table;
    }
    __device__ __forceinline__ static void fill_lds(const TimeMaxArgs &A, int tid)
    {
        if (tid < CED_MAX_LEVELS)
            store_level(levels() + tid * 8, make_level(A.levels, tid, EntryBytes<F16, TEMPORAL>::value));
    }

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

        // x_norm / selector / |move| (model.py:378-383), as the fused kernels form them
        const float extent[3] = { A.aabb[3] - A.aabb[0], A.aabb[4] - A.aabb[1], A.aabb[5] - A.aabb[2] };
        float xn[NT][3], mnorm[NT];
        bool sel[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            bool inside = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float xm = px[j][a] + mv[j][a];
                const float x = (xm - A.aabb[a]) / extent[a];
                inside = inside && (x > 0.0f && x < 1.0f);
                xn[j][a] = __builtin_fminf(__builtin_fmaxf(x, 0.0f), 1.0f);
            }
            sel[j] = inside;
            mnorm[j] = TE ? __builtin_sqrtf((mv[j][0] * mv[j][0] + mv[j][1] * mv[j][1]) + mv[j][2] * mv[j][2]) : 0.0f;
        }

        // the lane's four levels
        float R[NT][8];
        int k_lo = 0;
        float t_frac = 0.0f;
        if constexpr (TEMPORAL) temporal_keyframe(tq, k_lo, t_frac);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int level = W::kHalf ? 4 * i + g : 4 * i + 2 * (g & 1) + (g >> 1);
            const LevelConst L = load_level(levels() + level * 8);
            if (((A.level_mode >> (2 * i)) & 3) == 2) {
#pragma unroll
                for (int j = 0; j < NT; ++j) hash_level<F16, TEMPORAL, 2>(L, A.table, xn[j], k_lo, t_frac, R[j][2 * i], R[j][2 * i + 1]);
            } else {
#pragma unroll
                for (int j = 0; j < NT; ++j) hash_level<F16, TEMPORAL, 0>(L, A.table, xn[j], k_lo, t_frac, R[j][2 * i], R[j][2 * i + 1]);
            }
        }

        float raw[NT];
        if constexpr (W::kHalf) base_density_half<TE, W::kSplit, W::kK32, NT>(A, w, w + W::kPlane, lane, R, tq, mnorm, raw);
        else base_density_f32<TE, NT>(A, w, lane, R, tq, mnorm, raw);
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

// the motion network and mlp_base, adjacent at the start of every blob
template <bool TE> using TimeMaxF32 = F32Weights<Blob<TE>::H0>;
template <bool TE, bool SPLIT, bool K32> using TimeMaxHalf = HalfWeights<HalfBlob<TE>::H0 * kFragHalves, SPLIT, K32>;

// 16-row tiles per wave iteration: two, with no tangent tiles beside them -- except on an fp32 temporal table, whose
// 16-byte corner loads (two key-frames each) hold 32 more registers per tile: two tiles reach 256 VGPRs and spill
// (DESIGN 4.1f has the cross-compiled counts)
template <bool F16, bool TEMPORAL> constexpr int kTimeMaxTiles = (TEMPORAL && !F16) ? 1 : 2;

template <bool TE, bool F16, bool TEMPORAL> static void launch_time_max_table(const ced_field_desc *d, const TimeMaxArgs &A, void *stream)
{
    using Op = TimeMaxOp<TE, F16, TEMPORAL>;
    constexpr int NT = kTimeMaxTiles<F16, TEMPORAL>;
    const int mw = d->max_workgroups;
    if (d->mlp_precision == CED_MLP_F32 || d->mlp_precision == CED_MLP_F32_HEAD16X2)
        launch_tiles<Op, TimeMaxF32<TE>, NT>(A, mw, stream);
    else if (d->mlp_precision == CED_MLP_F16)
        launch_tiles<Op, TimeMaxHalf<TE, false, false>, NT>(A, mw, stream);
    else if constexpr (!TE && !TEMPORAL)                                 // half_layout_k32: the blob has the K = 32 placements
        launch_tiles<Op, TimeMaxHalf<TE, true, true>, NT>(A, mw, stream);
    else
        launch_tiles<Op, TimeMaxHalf<TE, true, false>, NT>(A, mw, stream);
}

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
    const ced_hash_desc &h = desc->hash;
    rc = validate_hash(&h, who);
    if (rc) return rc;
    CED_REQUIRE(h.n_levels == CED_MAX_LEVELS, "%s: the kernel needs n_levels == 16 (got %d)", who, h.n_levels);
    rc = require_32bit_byte_offsets(h, who);
    if (rc) return rc;
    static_assert(half_kernel_k32(false, false, true, 1024) && !half_kernel_k32(true, false, true, 1024) &&
                  !half_kernel_k32(false, true, true, 1024), "launch_time_max_table restates half_layout_k32");
    TimeMaxArgs A{};
    A.n = n;
    A.pos = positions; A.times = times; A.out = out;
    A.n_bins = n_bins; A.n_times = n_times;
    for (int i = 0; i < 6; ++i) A.aabb[i] = desc->aabb[i];
    motion_args(desc, A);
    A.time_mode = desc->time_mode;
    A.raw_reg = desc->mlp_precision == CED_MLP_F32_HEAD16X2 ? 3 : 0;
    A.table = h.table;
    fill_levels(A.levels, h);
    A.level_mode = hash_level_modes(h, false);
    switch ((desc->time_mode ? 1 : 0) | (h.table_dtype ? 2 : 0) | (h.temporal ? 4 : 0)) {
    case 0: launch_time_max_table<false, false, false>(desc, A, stream); break;
    case 1: launch_time_max_table<true, false, false>(desc, A, stream); break;
    case 2: launch_time_max_table<false, true, false>(desc, A, stream); break;
    case 3: launch_time_max_table<true, true, false>(desc, A, stream); break;
    case 4: launch_time_max_table<false, false, true>(desc, A, stream); break;
    case 5: launch_time_max_table<true, false, true>(desc, A, stream); break;
    case 6: launch_time_max_table<false, true, true>(desc, A, stream); break;
    default: launch_time_max_table<true, true, true>(desc, A, stream); break;
    }
    return check_launch(who);
}
