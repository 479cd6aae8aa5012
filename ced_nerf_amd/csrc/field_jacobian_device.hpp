// Device code of the motion network's derivative, shared by field_jacobian.hip (ced_field_move_jacobian and the Newton
// inverse) and field_density_gradient.hip (the density's gradient with respect to the observed point needs the warp's
// Jacobian of the same launch): motion_move_jacobian = motion_move of field_move_device.hpp with the four tangent tiles
// (directions x, y, z, t) beside each primal tile, in the three arithmetics.  field_jacobian.hip describes the method.
#pragma once
#include "field_move_device.hpp"

namespace ced {


constexpr int kDirs = 4;                              // tangent directions: x, y, z, t
constexpr float kPiF = 3.14159274101257324f;          // the pi of det_sinpi_phase

// ---- tangents on the fp32 MFMA chain ---------------------------------------------------------------------------------
// Tangent tile 4j + b of primal tile j is d/d(x,y,z,t)_b.  Feature k = 4S + g of the operand (lane group g, k-step S)
// belongs to dimension S / 2, frequency 2^(g/2) (S even) or 4 * 2^(g/2) (S odd), phase g & 1; its partner of the other
// phase sits on lane group g ^ 1 of the same k-step.
template <int NP>
__device__ __forceinline__ void encode_tangent(const float (&Bp)[NP][16], int g, float (&Bt)[kDirs * NP][16])
{
    const float sc0 = (float)(1 << (g >> 1));
    const float w0 = kPiF * sc0, w1 = kPiF * (4.0f * sc0);              // exact: powers of two
    const bool cosine = (g & 1) != 0;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
#pragma unroll
        for (int S = 0; S < 8; ++S) {
            const float partner = __shfl_xor(Bp[j][S], 16, 64);
            const float w = (S & 1) != 0 ? w1 : w0;
            const float d = (cosine ? -w : w) * partner;
#pragma unroll
            for (int b = 0; b < kDirs; ++b) Bt[kDirs * j + b][S] = (S >> 1) == b ? d : 0.0f;
        }
#pragma unroll
        for (int b = 0; b < kDirs; ++b) {
#pragma unroll
            for (int S = 8; S < 16; ++S) Bt[kDirs * j + b][S] = 0.0f;
        }
    }
}

// a hidden layer's tangents as the next layer's operand: zero wherever the primal pre-activation is not > 0
template <int NP>
__device__ __forceinline__ void tangent_operand(const f4 (&Dp)[NP][4], const f4 (&Dt)[kDirs * NP][4], float (&Bt)[kDirs * NP][16])
{
#pragma unroll
    for (int j = 0; j < NP; ++j) {
#pragma unroll
        for (int b = 0; b < kDirs; ++b) {
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
                for (int q = 0; q < 4; ++q) Bt[kDirs * j + b][4 * nb + q] = Dp[j][nb][q] > 0.0f ? Dt[kDirs * j + b][nb][q] : 0.0f;
            }
        }
    }
}

// jac[4a + b] = d move_a / d(x,y,z,t)_b from the last layer's accumulators, rows placed as move_vector reads them:
//   without fine offsets   (d off_a) * step
//   with                   (d off_a + (1 - th_a * th_a) * d fine_a) * step,   th_a = move_vector's tanh value
// every operation rounded on its own.  Every lane gets all twelve entries of its column's samples.
template <int NP>
__device__ __forceinline__ void jacobian_vector(const f4 (&Dp)[NP][4], const f4 (&Dt)[kDirs * NP][4], float moving_step, int use_div,
                                                int c, float (&J)[NP][12])
{
#pragma unroll
    for (int j = 0; j < NP; ++j) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float slope = 0.0f;
            if (use_div) {
                const float th = fine_tanh(fine_row(Dp[j][0], a, c));
                slope = 1.0f - th * th;
            }
#pragma unroll
            for (int b = 0; b < kDirs; ++b) {
                float v = __shfl(Dt[kDirs * j + b][0][a], c, 64);
                if (use_div) v = v + slope * fine_row(Dt[kDirs * j + b][0], a, c);
                J[j][4 * a + b] = v * moving_step;
            }
        }
    }
}

// fp32 MFMA chain (CED_MLP_F32, CED_MLP_F32_HEAD16X2): motion_move_f32 with the four tangent tiles beside each primal tile
template <int NP, typename Time>
__device__ __forceinline__ void motion_move_jacobian_f32(const float *lw, int lane, const float (&px)[NP][3], const Time &time,
                                                         float moving_step, int use_div, float (&mv)[NP][3], float (&J)[NP][12])
{
    using BL = Blob<false>;
    constexpr int NTT = kDirs * NP;
    const int g = lane >> 4, c = lane & 15;
    float Bp[NP][16], Bt[NTT][16];
    f4 Dp[NP][4], Dt[NTT][4];
    motion_encode<NP>(px, time, g, Bp);
    encode_tangent<NP>(Bp, g, Bt);
    mlp_layer<8, 4, NP>(lw + BL::M0, lane, Bp, Dp);
    mlp_layer<8, 4, NTT>(lw + BL::M0, lane, Bt, Dt);
    tangent_operand<NP>(Dp, Dt, Bt);
    to_operand<4, true, NP>(Dp, Bp);
    mlp_layer<16, 4, NP>(lw + BL::M1, lane, Bp, Dp);
    mlp_layer<16, 4, NTT>(lw + BL::M1, lane, Bt, Dt);
    tangent_operand<NP>(Dp, Dt, Bt);
    to_operand<4, true, NP>(Dp, Bp);
    mlp_layer<16, 4, NP>(lw + BL::M2, lane, Bp, Dp);
    mlp_layer<16, 4, NTT>(lw + BL::M2, lane, Bt, Dt);
    tangent_operand<NP>(Dp, Dt, Bt);
    to_operand<4, true, NP>(Dp, Bp);
    mlp_layer<16, 1, NP>(lw + BL::M3, lane, Bp, Dp);
    mlp_layer<16, 1, NTT>(lw + BL::M3, lane, Bt, Dt);
    move_vector<NP>(Dp, moving_step, use_div, c, mv);
    jacobian_vector<NP>(Dp, Dt, moving_step, use_div, c, J);
}

// ---- tangents on the fp16 MFMAs ----------------------------------------------------------------------------------------
// a hidden layer's tangents as the next layer's operand: zero wherever the primal pre-activation is not > 0, saturated to
// the fp16 range on both sides, rounded (f16) or split (f16x2) exactly as to_operand_h treats the primal
template <int NP, bool SPLIT>
__device__ __forceinline__ void tangent_operand_h(const f4 (&Dp)[NP][4], const f4 (&Dt)[kDirs * NP][4], h8 (&Bh)[kDirs * NP][2],
                                                  h8 (&Bl)[kDirs * NP][2])
{
#pragma unroll
    for (int j = 0; j < NP; ++j) {
#pragma unroll
        for (int b = 0; b < kDirs; ++b) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = __builtin_amdgcn_fmed3f(Dt[kDirs * j + b][2 * ks + (e >> 2)][e & 3], -kHalfMax, kHalfMax);
                    v[e] = Dp[j][2 * ks + (e >> 2)][e & 3] > 0.0f ? d : 0.0f;
                }
                to_half8<SPLIT>(v, Bh[kDirs * j + b][ks], Bl[kDirs * j + b][ks]);
            }
        }
    }
}

// fp16 MFMAs (CED_MLP_F16, CED_MLP_F16X2; K32: the blob has half_kernel_k32's placements): motion_move_half with the four
// tangent tiles beside each primal tile.  Lane group g owns dimension g, so the tangent of direction b is nonzero on
// lane group b alone: element e = 2 * freq + phase is 2^freq pi times element e ^ 1, negated for a cosine, formed in
// fp32 from the fp32 features and then rounded / split like them.
template <bool SPLIT, bool K32, int NP, typename Time>
__device__ __forceinline__ void motion_move_jacobian_half(const _Float16 *whi, const _Float16 *wlo, int lane, const float (&px)[NP][3],
                                                          const Time &time, float moving_step, int use_div, float (&mv)[NP][3],
                                                          float (&J)[NP][12])
{
    using BL = HalfBlob<false>;
    constexpr int NTT = kDirs * NP;
    const int g = lane >> 4, c = lane & 15;
    h8 Bph[NP][2], Bpl[NP][2], Bth[NTT][2], Btl[NTT][2];
    f4 Dp[NP][4], Dt[NTT][4];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        float f[8], d[8];
        motion_features_half(px[j], time.value(j), g, f);
        to_half8<SPLIT>(f, Bph[j][0], Bpl[j][0]);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float w = kPiF * (float)(1 << (e >> 1));
            d[e] = ((e & 1) != 0 ? -w : w) * f[e ^ 1];
        }
#pragma unroll
        for (int b = 0; b < kDirs; ++b) {
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (g == b) ? d[e] : 0.0f;
            to_half8<SPLIT>(v, Bth[kDirs * j + b][0], Btl[kDirs * j + b][0]);
        }
    }
    mlp_layer_h<1, 4, NP, SPLIT>(whi + BL::M0 * kFragHalves, wlo + BL::M0 * kFragHalves, lane, Bph, Bpl, Dp);
    mlp_layer_h<1, 4, NTT, SPLIT>(whi + BL::M0 * kFragHalves, wlo + BL::M0 * kFragHalves, lane, Bth, Btl, Dt);
    tangent_operand_h<NP, SPLIT>(Dp, Dt, Bth, Btl);
    to_operand_h<NP, SPLIT>(Dp, Bph, Bpl);
    hidden_fed_layer<2, 4, NP, SPLIT, K32>(whi + BL::M1 * kFragHalves, wlo + BL::M1 * kFragHalves, lane, Bph, Bpl, Dp);
    hidden_fed_layer<2, 4, NTT, SPLIT, K32>(whi + BL::M1 * kFragHalves, wlo + BL::M1 * kFragHalves, lane, Bth, Btl, Dt);
    tangent_operand_h<NP, SPLIT>(Dp, Dt, Bth, Btl);
    to_operand_h<NP, SPLIT>(Dp, Bph, Bpl);
    hidden_fed_layer<2, 4, NP, SPLIT, K32>(whi + BL::M2 * kFragHalves, wlo + BL::M2 * kFragHalves, lane, Bph, Bpl, Dp);
    hidden_fed_layer<2, 4, NTT, SPLIT, K32>(whi + BL::M2 * kFragHalves, wlo + BL::M2 * kFragHalves, lane, Bth, Btl, Dt);
    tangent_operand_h<NP, SPLIT>(Dp, Dt, Bth, Btl);
    to_operand_h<NP, SPLIT>(Dp, Bph, Bpl);
    hidden_fed_layer<2, 1, NP, SPLIT, K32>(whi + BL::M3 * kFragHalves, wlo + BL::M3 * kFragHalves, lane, Bph, Bpl, Dp);
    hidden_fed_layer<2, 1, NTT, SPLIT, K32>(whi + BL::M3 * kFragHalves, wlo + BL::M3 * kFragHalves, lane, Bth, Btl, Dt);
    move_vector<NP>(Dp, moving_step, use_div, c, mv);
    jacobian_vector<NP>(Dp, Dt, moving_step, use_div, c, J);
}

// the chain with its tangents in the arithmetic of the staged weights W; w = the tile's LDS base
template <typename W, int NP, typename Time>
__device__ __forceinline__ void motion_move_jacobian(const typename W::Elem *w, int lane, const float (&px)[NP][3], const Time &time,
                                                     float moving_step, int use_div, float (&mv)[NP][3], float (&J)[NP][12])
{
    if constexpr (W::kHalf)
        motion_move_jacobian_half<W::kSplit, W::kK32, NP>(w, w + W::kPlane, lane, px, time, moving_step, use_div, mv, J);
    else
        motion_move_jacobian_f32<NP>(w, lane, px, time, moving_step, use_div, mv, J);
}

}  // namespace ced
