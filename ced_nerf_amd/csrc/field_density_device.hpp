// The canonical density on tile_kernel's skeleton (field_move_device.hpp), stated once for the ops that evaluate it after
// the warp: GradientOp (field_density_gradient.hip), TimeMaxOp (field_time_max.hip) and LevelSetOp
// (field_level_set.hip).  Such an op stages the motion
// network AND mlp_base (adjacent at the start of every blob: DensityF32 / DensityHalf), keeps the sixteen levels'
// constants in LDS beside them (DensityLevels), and per tile goes from `move` to the raw density through
//   canonical_point: x_norm, the selector and |move|, as the fused kernels form them;
//   gather_levels:   the lane's four levels through hash_level (slot_level says which they are);
//   mlp_base:        the two layers on NP primal tiles and, beside ONE primal tile, ND tangent tiles through the same
//                    layer functions -- MFMA columns do not mix, so the primal tiles compute ced_field_forward's sigma bit
//                    for bit whatever stands beside them.
// On the host: DensityArgs, the part of a kernel's argument block these read, fill_density_args, which checks the table and
// fills it from the descriptor, and launch_density, the dispatch over arithmetic, time encoding and table kind.
#pragma once
#include "field_args.hpp"
#include "field_move_device.hpp"
#include "hash_device.hpp"

namespace ced {

// the public base of an op's Args (an aggregate: Args A{} zeroes it)
struct DensityArgs {
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

// the motion network and mlp_base, adjacent at the start of every blob
template <bool TE> using DensityF32 = F32Weights<Blob<TE>::H0>;
template <bool TE, bool SPLIT, bool K32> using DensityHalf = HalfWeights<HalfBlob<TE>::H0 * kFragHalves, SPLIT, K32>;

// the sixteen levels' constants, in LDS beside the staged layers; an op inherits this beside TileOp / SampleOp and names
// fill_lds as its own
template <bool F16, bool TEMPORAL> struct DensityLevels {
    __device__ __forceinline__ static uint32_t *levels()
    {
        __shared__ __attribute__((aligned(16))) uint32_t table[8 * CED_MAX_LEVELS];
        return table;
    }
    __device__ __forceinline__ static void fill_lds(const DensityArgs &A, int tid)
    {
        if (tid < CED_MAX_LEVELS)
            store_level(levels() + tid * 8, make_level(A.levels, tid, EntryBytes<F16, TEMPORAL>::value));
    }
};

// x_norm / selector / |move| (model.py:378-383), as the fused kernels form them
template <bool TE, int NT>
__device__ __forceinline__ void canonical_point(const float (&aabb)[6], const float (&px)[NT][3], const float (&mv)[NT][3],
                                                float (&xn)[NT][3], bool (&sel)[NT], float (&mnorm)[NT])
{
    const float extent[3] = { aabb[3] - aabb[0], aabb[4] - aabb[1], aabb[5] - aabb[2] };
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        bool inside = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float xm = px[j][a] + mv[j][a];
            const float x = (xm - aabb[a]) / extent[a];
            inside = inside && (x > 0.0f && x < 1.0f);
            xn[j][a] = __builtin_fminf(__builtin_fmaxf(x, 0.0f), 1.0f);
        }
        sel[j] = inside;
        mnorm[j] = TE ? __builtin_sqrtf((mv[j][0] * mv[j][0] + mv[j][1] * mv[j][1]) + mv[j][2] * mv[j][2]) : 0.0f;
    }
}

// the level that gather slot i of lane group g reads: where mlp_base's operand of the arithmetic wants it
template <typename W> __device__ __forceinline__ int slot_level(int i, int g)
{
    return W::kHalf ? 4 * i + g : 4 * i + 2 * (g & 1) + (g >> 1);
}

// the lane's four levels of each tile at key-frame (k_lo, t_frac): R[j][2i], R[j][2i + 1] = the features of slot i
template <typename W, bool F16, bool TEMPORAL, int NT>
__device__ __forceinline__ void gather_levels(const DensityArgs &A, const uint32_t *levels, int g, const float (&xn)[NT][3], int k_lo,
                                              float t_frac, float (&R)[NT][8])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const LevelConst L = load_level(levels + slot_level<W>(i, g) * 8);
        if (((A.level_mode >> (2 * i)) & 3) == 2) {
#pragma unroll
            for (int j = 0; j < NT; ++j) hash_level<F16, TEMPORAL, 2>(L, A.table, xn[j], k_lo, t_frac, R[j][2 * i], R[j][2 * i + 1]);
        } else {
#pragma unroll
            for (int j = 0; j < NT; ++j) hash_level<F16, TEMPORAL, 0>(L, A.table, xn[j], k_lo, t_frac, R[j][2 * i], R[j][2 * i + 1]);
        }
    }
}

// a hidden layer's tangents as the next layer's operand (tangent_operand / tangent_operand_h for ND tiles beside one
// primal tile): zero wherever the primal pre-activation is not > 0
template <int ND>
__device__ __forceinline__ void grad_tangent_operand(const f4 (&Dp)[1][4], const f4 (&Dt)[ND][4], float (&Bt)[ND][16])
{
#pragma unroll
    for (int b = 0; b < ND; ++b) {
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
            for (int q = 0; q < 4; ++q) Bt[b][4 * nb + q] = Dp[0][nb][q] > 0.0f ? Dt[b][nb][q] : 0.0f;
        }
    }
}

template <bool SPLIT, int ND>
__device__ __forceinline__ void grad_tangent_operand_h(const f4 (&Dp)[1][4], const f4 (&Dt)[ND][4], h8 (&Bh)[ND][2], h8 (&Bl)[ND][2])
{
#pragma unroll
    for (int b = 0; b < ND; ++b) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = __builtin_amdgcn_fmed3f(Dt[b][2 * ks + (e >> 2)][e & 3], -kHalfMax, kHalfMax);
                v[e] = Dp[0][2 * ks + (e >> 2)][e & 3] > 0.0f ? d : 0.0f;
            }
            to_half8<SPLIT>(v, Bh[b][ks], Bl[b][ks]);
        }
    }
}

// mlp_base on the fp32 MFMA chain (CED_MLP_F32, CED_MLP_F32_HEAD16X2): R[j] are the lane's gathered features of primal
// tile j (slot i = level 4i + 2(g&1) + (g>>1)), dR[b] their tangents in direction b; out: the raw density and its
// tangents on lane group 3.  The tangent rows of the time features are zero: the time encoding is a constant.
template <bool TE, int NP, int ND>
__device__ __forceinline__ void mlp_base_f32(const DensityArgs &A, const float *lw, int lane, const float (&R)[NP][8],
                                             const float (&dR)[ND > 0 ? ND : 1][8], float tq, const float (&mnorm)[NP],
                                             float (&raw)[NP], float (&draw)[ND > 0 ? ND : 1])
{
    static_assert(ND == 0 || NP == 1, "tangent tiles stand beside one primal tile");
    using BL = Blob<TE>;
    const int g = lane >> 4;
    float Bp[NP][16], Bt[ND > 0 ? ND : 1][16];
    f4 Dp[NP][4], Dt[ND > 0 ? ND : 1][4];
    // operand element (k-step S, group g) is feature g&1 of level 2S + (g>>1): field_kernel.hpp's swap, tangents alike
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(R[j][2 * i]), __float_as_uint(R[j][2 * i + 1]), false, false);
            Bp[j][2 * i] = __uint_as_float(sw[0]);
            Bp[j][2 * i + 1] = __uint_as_float(sw[1]);
        }
#pragma unroll
        for (int b = 0; b < ND; ++b) {
            const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(dR[b][2 * i]), __float_as_uint(dR[b][2 * i + 1]), false, false);
            Bt[b][2 * i] = __uint_as_float(sw[0]);
            Bt[b][2 * i + 1] = __uint_as_float(sw[1]);
        }
    }
#pragma unroll
    for (int S = 8; S < 16; ++S) {
#pragma unroll
        for (int j = 0; j < NP; ++j) Bp[j][S] = (TE && S < 11) ? time_feature(4 * (S - 8) + g, A.time_mode, tq, mnorm[j]) : 0.0f;
#pragma unroll
        for (int b = 0; b < ND; ++b) Bt[b][S] = 0.0f;
    }
    mlp_layer<BL::KS_B0, 4, NP>(lw + BL::B0, lane, Bp, Dp);
    if constexpr (ND > 0) {
        mlp_layer<BL::KS_B0, 4, ND>(lw + BL::B0, lane, Bt, Dt);
        grad_tangent_operand(Dp, Dt, Bt);
    }
    to_operand<4, true, NP>(Dp, Bp);
    mlp_layer<16, 1, NP>(lw + BL::B1, lane, Bp, Dp);
    if constexpr (ND > 0) mlp_layer<16, 1, ND>(lw + BL::B1, lane, Bt, Dt);
    // named values first: a select between vector elements by a run-time index would go through memory
    const bool last = A.raw_reg != 0;
#pragma unroll
    for (int j = 0; j < NP; ++j) raw[j] = last ? Dp[j][0][3] : Dp[j][0][0];
#pragma unroll
    for (int b = 0; b < ND; ++b) draw[b] = last ? Dt[b][0][3] : Dt[b][0][0];
}

// mlp_base on the fp16 MFMAs (CED_MLP_F16, CED_MLP_F16X2; K32: the blob has half_kernel_k32's placements): slot i = level
// 4i + g, features at operand elements 2i, 2i + 1 (field_half.hip); the raw density is row 15 = (lane group 3, register 3)
template <bool TE, bool SPLIT, bool K32, int NP, int ND>
__device__ __forceinline__ void mlp_base_half(const DensityArgs &A, const _Float16 *whi, const _Float16 *wlo, int lane,
                                              const float (&R)[NP][8], const float (&dR)[ND > 0 ? ND : 1][8], float tq,
                                              const float (&mnorm)[NP], float (&raw)[NP], float (&draw)[ND > 0 ? ND : 1])
{
    static_assert(ND == 0 || NP == 1, "tangent tiles stand beside one primal tile");
    using BL = HalfBlob<TE>;
    const int g = lane >> 4;
    h8 Bph[NP][2], Bpl[NP][2], Bth[ND > 0 ? ND : 1][2], Btl[ND > 0 ? ND : 1][2];
    f4 Dp[NP][4], Dt[ND > 0 ? ND : 1][4];
    float v[8];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = __builtin_amdgcn_fmed3f(R[j][e], -kHalfMax, kHalfMax);
        to_half8<SPLIT>(v, Bph[j][0], Bpl[j][0]);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (TE && e < 3) ? time_feature(4 * e + g, A.time_mode, tq, mnorm[j]) : 0.0f;
        to_half8<SPLIT>(v, Bph[j][1], Bpl[j][1]);
    }
#pragma unroll
    for (int b = 0; b < ND; ++b) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = __builtin_amdgcn_fmed3f(dR[b][e], -kHalfMax, kHalfMax);
        to_half8<SPLIT>(v, Bth[b][0], Btl[b][0]);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            Bth[b][1][e] = (_Float16)0.0f;
            Btl[b][1][e] = (_Float16)0.0f;
        }
    }
    mlp_layer_h<BL::KS_B0, 4, NP, SPLIT>(whi + BL::B0 * kFragHalves, wlo + BL::B0 * kFragHalves, lane, Bph, Bpl, Dp);
    if constexpr (ND > 0) {
        mlp_layer_h<BL::KS_B0, 4, ND, SPLIT>(whi + BL::B0 * kFragHalves, wlo + BL::B0 * kFragHalves, lane, Bth, Btl, Dt);
        grad_tangent_operand_h<SPLIT>(Dp, Dt, Bth, Btl);
    }
    to_operand_h<NP, SPLIT>(Dp, Bph, Bpl);
    hidden_fed_layer<2, 1, NP, SPLIT, K32>(whi + BL::B1 * kFragHalves, wlo + BL::B1 * kFragHalves, lane, Bph, Bpl, Dp);
    if constexpr (ND > 0) hidden_fed_layer<2, 1, ND, SPLIT, K32>(whi + BL::B1 * kFragHalves, wlo + BL::B1 * kFragHalves, lane, Bth, Btl, Dt);
#pragma unroll
    for (int j = 0; j < NP; ++j) raw[j] = Dp[j][0][3];
#pragma unroll
    for (int b = 0; b < ND; ++b) draw[b] = Dt[b][0][3];
}

// mlp_base in the arithmetic of the staged weights W; w = the tile's LDS base.  An op without tangents (ND = 0) passes
// one-element arrays for dR and draw; they are not touched.
template <typename W, bool TE, int NP, int ND>
__device__ __forceinline__ void mlp_base(const DensityArgs &A, const typename W::Elem *w, int lane, const float (&R)[NP][8],
                                         const float (&dR)[ND > 0 ? ND : 1][8], float tq, const float (&mnorm)[NP],
                                         float (&raw)[NP], float (&draw)[ND > 0 ? ND : 1])
{
    if constexpr (W::kHalf) mlp_base_half<TE, W::kSplit, W::kK32, NP, ND>(A, w, w + W::kPlane, lane, R, dR, tq, mnorm, raw, draw);
    else mlp_base_f32<TE, NP, ND>(A, w, lane, R, dR, tq, mnorm, raw, draw);
}

// ---- host ---------------------------------------------------------------------------------------------------------------
// what every op on the canonical density checks of the hash table and reads from the descriptor
static int fill_density_args(const ced_field_desc *d, DensityArgs &A, const char *who)
{
    const ced_hash_desc &h = d->hash;
    int rc = validate_hash(&h, who);
    if (rc) return rc;
    CED_REQUIRE(h.n_levels == CED_MAX_LEVELS, "%s: the kernel needs n_levels == 16 (got %d)", who, h.n_levels);
    rc = require_32bit_byte_offsets(h, who);
    if (rc) return rc;
    for (int i = 0; i < 6; ++i) A.aabb[i] = d->aabb[i];
    motion_args(d, A);
    A.time_mode = d->time_mode;
    A.raw_reg = d->mlp_precision == CED_MLP_F32_HEAD16X2 ? 3 : 0;
    A.table = h.table;
    fill_levels(A.levels, h);
    A.level_mode = hash_level_modes(h, false);
    return CED_OK;
}

// Op<TE, F16 table, TEMPORAL> on Op::kTiles tiles per wave in the descriptor's arithmetic.  A ladder of its own:
// launch_motion's would instantiate the K = 32 placements for all eight table kinds, and they exist only without a time
// encoding on a plain table.
template <template <bool, bool, bool> class OpT, bool TE, bool F16, bool TEMPORAL>
static void launch_density_table(const ced_field_desc *d, const typename OpT<TE, F16, TEMPORAL>::Args &A, void *stream)
{
    using Op = OpT<TE, F16, TEMPORAL>;
    constexpr int NT = Op::kTiles;
    const int mw = d->max_workgroups;
    if (d->mlp_precision == CED_MLP_F32 || d->mlp_precision == CED_MLP_F32_HEAD16X2)
        launch_tiles<Op, DensityF32<TE>, NT>(A, mw, stream);
    else if (d->mlp_precision == CED_MLP_F16)
        launch_tiles<Op, DensityHalf<TE, false, false>, NT>(A, mw, stream);
    else if constexpr (!TE && !TEMPORAL)                                 // half_layout_k32: the blob has the K = 32 placements
        launch_tiles<Op, DensityHalf<TE, true, true>, NT>(A, mw, stream);
    else
        launch_tiles<Op, DensityHalf<TE, true, false>, NT>(A, mw, stream);
}

template <template <bool, bool, bool> class OpT, typename Args>
static int launch_density(const ced_field_desc *d, const Args &A, const char *who, void *stream)
{
    static_assert(half_kernel_k32(false, false, true, 1024) && !half_kernel_k32(true, false, true, 1024) &&
                  !half_kernel_k32(false, true, true, 1024), "launch_density_table restates half_layout_k32");
    switch ((d->time_mode ? 1 : 0) | (d->hash.table_dtype ? 2 : 0) | (d->hash.temporal ? 4 : 0)) {
    case 0: launch_density_table<OpT, false, false, false>(d, A, stream); break;
    case 1: launch_density_table<OpT, true, false, false>(d, A, stream); break;
    case 2: launch_density_table<OpT, false, true, false>(d, A, stream); break;
    case 3: launch_density_table<OpT, true, true, false>(d, A, stream); break;
    case 4: launch_density_table<OpT, false, false, true>(d, A, stream); break;
    case 5: launch_density_table<OpT, true, false, true>(d, A, stream); break;
    case 6: launch_density_table<OpT, false, true, true>(d, A, stream); break;
    default: launch_density_table<OpT, true, true, true>(d, A, stream); break;
    }
    return check_launch(who);
}

}  // namespace ced
