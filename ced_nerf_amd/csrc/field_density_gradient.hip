// The spatial derivative of the density: ced_field_density_gradient / ced_field_density_gradient_rays hand out, per row
// and from one launch, sigma(x, t) with ced_field_forward's bits and the gradient of its logarithm and of itself with
// respect to the canonical point c = x + move(x, t) and to the observed point x (include/cednerf_hip.h states the rules
// and every fp32 operation).
//
// Forward mode, as field_jacobian.hip differentiates the warp: the derivative of a sample with respect to its normalised
// canonical position is three tangent vectors pushed through mlp_base beside the primal, three more 16-column operand
// tiles through the SAME layer functions on the same staged blob, in the arithmetic the descriptor selects (mlp_layer;
// mlp_layer_h / hidden_fed_layer).  MFMA columns do not mix, so the primal tile computes ced_field_forward's sigma
// whatever stands beside it.  Per 16-row tile:
//   1. motion_move_jacobian (field_jacobian_device.hpp): move with ced_field_move's bits, and the warp's Jacobian J;
//   2. x_norm, the selector and the time features, as the fused forward forms them;
//   3. per lane its four levels' features AND their three x-tangents from the same eight corner loads (hash_level_dx),
//      carried pre-scaled by 2^-K, K = ceil(log2(finest level scale)): a feature's slope is scale_l times a difference of
//      table values, beyond the fp16 range at the finest scales; 2^-K is exact and is undone in fp32 at the end;
//   4. mlp_base's two layers on the primal tile and the three tangent tiles; the tangent rows of the nine time features
//      are zero (the time encoding is a constant, its attenuation by |move| included), a hidden tangent is zeroed wherever
//      the PRIMAL pre-activation is not > 0;
//   5. the fp32 lines of the header: 1 / extent, (I + J_x)^T, the slope of trunc_exp.
//
// Shape: tile_kernel<GradientOp, W, 1, 512> of field_move_device.hpp, one more op on that skeleton.  The staged plane W is
// the motion network AND mlp_base (adjacent in every blob: 64 KB fp32 or split fp16 with a time encoding); the sixteen
// levels' constants sit in LDS beside it, as in the fused kernels, filled by the op's hook before the skeleton's barrier;
// one workgroup per CU.  The rows come from that header's SampleSrc, which the two entries fill through point_samples /
// ray_samples.  ONE 16-row primal tile per wave iteration: stage 1 holds five operand and five accumulator tiles, stage 4
// four and four beside J and the 32 gathered values; two waves per SIMD, no scratch.
#include "field_args.hpp"
#include "field_jacobian_device.hpp"
#include "hash_device.hpp"

namespace ced {

struct GradArgs {
    SampleSrc src;
    float *sigma, *grad, *dlog, *dlog_canonical;      // [n], [n,3] x 3; any may be null
    float aabb[6];
    float moving_step;
    int use_div, time_mode;
    int raw_reg;                                      // fp32 chain: the raw density's register on lane group 3 (mixed blob: 3)
    float tangent_scale, tangent_unscale;             // 2^-K, 2^K
    const void *weights;
    int64_t lo_halves;
    int level_mode;                                   // 2 bits per gather slot: 2 = all four levels hashed, else 0
    const void *table;
    HashLevels levels;
};

constexpr float kExp15 = 3269017.25f;                 // the float32 nearest e^15: trunc_exp's backward clamps there
constexpr int kGradDirs = 3;                          // tangent directions: x_norm's three axes

// a hidden layer's tangents as the next layer's operand (tangent_operand / tangent_operand_h for kGradDirs tiles beside
// one primal tile): zero wherever the primal pre-activation is not > 0
__device__ __forceinline__ void grad_tangent_operand(const f4 (&Dp)[1][4], const f4 (&Dt)[kGradDirs][4], float (&Bt)[kGradDirs][16])
{
#pragma unroll
    for (int b = 0; b < kGradDirs; ++b) {
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
#pragma unroll
            for (int q = 0; q < 4; ++q) Bt[b][4 * nb + q] = Dp[0][nb][q] > 0.0f ? Dt[b][nb][q] : 0.0f;
        }
    }
}

template <bool SPLIT>
__device__ __forceinline__ void grad_tangent_operand_h(const f4 (&Dp)[1][4], const f4 (&Dt)[kGradDirs][4], h8 (&Bh)[kGradDirs][2],
                                                       h8 (&Bl)[kGradDirs][2])
{
#pragma unroll
    for (int b = 0; b < kGradDirs; ++b) {
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

// mlp_base on the fp32 MFMA chain (CED_MLP_F32, CED_MLP_F32_HEAD16X2): R / dR are the lane's gathered features (slot i =
// level 4i + 2(g&1) + (g>>1)) and their tangents; out: the raw density and its three tangents on lane group 3
template <bool TE>
__device__ __forceinline__ void base_gradient_f32(const GradArgs &A, const float *lw, int lane, const float (&R)[8],
                                                  const float (&dR)[kGradDirs][8], float tq, float mnorm, float &raw,
                                                  float (&draw)[kGradDirs])
{
    using BL = Blob<TE>;
    const int g = lane >> 4;
    float Bp[1][16], Bt[kGradDirs][16];
    f4 Dp[1][4], Dt[kGradDirs][4];
    // operand element (k-step S, group g) is feature g&1 of level 2S + (g>>1): field_kernel.hpp's swap, tangents alike
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(R[2 * i]), __float_as_uint(R[2 * i + 1]), false, false);
        Bp[0][2 * i] = __uint_as_float(sw[0]);
        Bp[0][2 * i + 1] = __uint_as_float(sw[1]);
#pragma unroll
        for (int b = 0; b < kGradDirs; ++b) {
            sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(dR[b][2 * i]), __float_as_uint(dR[b][2 * i + 1]), false, false);
            Bt[b][2 * i] = __uint_as_float(sw[0]);
            Bt[b][2 * i + 1] = __uint_as_float(sw[1]);
        }
    }
#pragma unroll
    for (int S = 8; S < 16; ++S) {
        Bp[0][S] = (TE && S < 11) ? time_feature(4 * (S - 8) + g, A.time_mode, tq, mnorm) : 0.0f;
#pragma unroll
        for (int b = 0; b < kGradDirs; ++b) Bt[b][S] = 0.0f;
    }
    mlp_layer<BL::KS_B0, 4, 1>(lw + BL::B0, lane, Bp, Dp);
    mlp_layer<BL::KS_B0, 4, kGradDirs>(lw + BL::B0, lane, Bt, Dt);
    grad_tangent_operand(Dp, Dt, Bt);
    to_operand<4, true, 1>(Dp, Bp);
    mlp_layer<16, 1, 1>(lw + BL::B1, lane, Bp, Dp);
    mlp_layer<16, 1, kGradDirs>(lw + BL::B1, lane, Bt, Dt);
    // named values first: a select between vector elements by a run-time index would go through memory
    const bool last = A.raw_reg != 0;
    raw = last ? Dp[0][0][3] : Dp[0][0][0];
#pragma unroll
    for (int b = 0; b < kGradDirs; ++b) draw[b] = last ? Dt[b][0][3] : Dt[b][0][0];
}

// mlp_base on the fp16 MFMAs (CED_MLP_F16, CED_MLP_F16X2; K32: the blob has half_kernel_k32's placements): slot i = level
// 4i + g, features at operand elements 2i, 2i + 1 (field_half.hip); the raw density is row 15 = (lane group 3, register 3)
template <bool TE, bool SPLIT, bool K32>
__device__ __forceinline__ void base_gradient_half(const GradArgs &A, const _Float16 *whi, const _Float16 *wlo, int lane,
                                                   const float (&R)[8], const float (&dR)[kGradDirs][8], float tq, float mnorm,
                                                   float &raw, float (&draw)[kGradDirs])
{
    using BL = HalfBlob<TE>;
    const int g = lane >> 4;
    h8 Bph[1][2], Bpl[1][2], Bth[kGradDirs][2], Btl[kGradDirs][2];
    f4 Dp[1][4], Dt[kGradDirs][4];
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = __builtin_amdgcn_fmed3f(R[e], -kHalfMax, kHalfMax);
    to_half8<SPLIT>(v, Bph[0][0], Bpl[0][0]);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (TE && e < 3) ? time_feature(4 * e + g, A.time_mode, tq, mnorm) : 0.0f;
    to_half8<SPLIT>(v, Bph[0][1], Bpl[0][1]);
#pragma unroll
    for (int b = 0; b < kGradDirs; ++b) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = __builtin_amdgcn_fmed3f(dR[b][e], -kHalfMax, kHalfMax);
        to_half8<SPLIT>(v, Bth[b][0], Btl[b][0]);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            Bth[b][1][e] = (_Float16)0.0f;
            Btl[b][1][e] = (_Float16)0.0f;
        }
    }
    mlp_layer_h<BL::KS_B0, 4, 1, SPLIT>(whi + BL::B0 * kFragHalves, wlo + BL::B0 * kFragHalves, lane, Bph, Bpl, Dp);
    mlp_layer_h<BL::KS_B0, 4, kGradDirs, SPLIT>(whi + BL::B0 * kFragHalves, wlo + BL::B0 * kFragHalves, lane, Bth, Btl, Dt);
    grad_tangent_operand_h<SPLIT>(Dp, Dt, Bth, Btl);
    to_operand_h<1, SPLIT>(Dp, Bph, Bpl);
    hidden_fed_layer<2, 1, 1, SPLIT, K32>(whi + BL::B1 * kFragHalves, wlo + BL::B1 * kFragHalves, lane, Bph, Bpl, Dp);
    hidden_fed_layer<2, 1, kGradDirs, SPLIT, K32>(whi + BL::B1 * kFragHalves, wlo + BL::B1 * kFragHalves, lane, Bth, Btl, Dt);
    raw = Dp[0][0][3];
#pragma unroll
    for (int b = 0; b < kGradDirs; ++b) draw[b] = Dt[b][0][3];
}

// ---- ced_field_density_gradient, ced_field_density_gradient_rays: one 16-row tile per wave iteration -----------------------
template <bool TE, bool F16, bool TEMPORAL> struct GradientOp : SampleOp {
    using Args = GradArgs;
    static constexpr int kPerCu = 1;

    // the sixteen levels' constants, in LDS beside the staged layers
    __device__ __forceinline__ static uint32_t *levels()
    {
        __shared__ __attribute__((aligned(16))) uint32_t table[8 * CED_MAX_LEVELS];
        return table;
    }
    __device__ __forceinline__ static void fill_lds(const GradArgs &A, int tid)
    {
        if (tid < CED_MAX_LEVELS)
            store_level(levels() + tid * 8, make_level(A.levels, tid, EntryBytes<F16, TEMPORAL>::value));
    }

    // w = the tile's LDS base of the staged layers
    template <typename W, int NT>
    __device__ __forceinline__ static void tile(const GradArgs &A, const Shared &, const typename W::Elem *w, int64_t tile_base,
                                                int64_t n_eff, int lane)
    {
        static_assert(NT == 1, "one primal tile beside its three tangent tiles");
        const int g = lane >> 4, c = lane & 15;
        float px[1][3], tq[1], mv[1][3], J[1][12];
        load_samples<1>(A.src, tile_base, n_eff, c, px, tq);
        motion_move_jacobian<W, 1>(w, lane, px, RowTime<1>{ tq }, A.moving_step, A.use_div, mv, J);

        // x_norm / selector / |move| (model.py:378-383), as the fused kernels form them
        const float extent[3] = { A.aabb[3] - A.aabb[0], A.aabb[4] - A.aabb[1], A.aabb[5] - A.aabb[2] };
        float xn[3];
        bool sel = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float xm = px[0][a] + mv[0][a];
            const float x = (xm - A.aabb[a]) / extent[a];
            sel = sel && (x > 0.0f && x < 1.0f);
            xn[a] = __builtin_fminf(__builtin_fmaxf(x, 0.0f), 1.0f);
        }
        const float mnorm = TE ? __builtin_sqrtf((mv[0][0] * mv[0][0] + mv[0][1] * mv[0][1]) + mv[0][2] * mv[0][2]) : 0.0f;

        // the lane's four levels: features and x-tangents from the same corner loads
        float R[8], dR[kGradDirs][8];
        int k_lo = 0;
        float t_frac = 0.0f;
        if constexpr (TEMPORAL) temporal_keyframe(tq[0], k_lo, t_frac);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int level = W::kHalf ? 4 * i + g : 4 * i + 2 * (g & 1) + (g >> 1);
            const LevelConst L = load_level(levels() + level * 8);
            float d0[3], d1[3];
            if (((A.level_mode >> (2 * i)) & 3) == 2)
                hash_level_dx<F16, TEMPORAL, 2>(L, A.table, xn, k_lo, t_frac, A.tangent_scale, R[2 * i], R[2 * i + 1], d0, d1);
            else
                hash_level_dx<F16, TEMPORAL, 0>(L, A.table, xn, k_lo, t_frac, A.tangent_scale, R[2 * i], R[2 * i + 1], d0, d1);
#pragma unroll
            for (int b = 0; b < kGradDirs; ++b) {
                dR[b][2 * i] = d0[b];
                dR[b][2 * i + 1] = d1[b];
            }
        }

        float raw_own, draw_own[kGradDirs];
        if constexpr (W::kHalf)
            base_gradient_half<TE, W::kSplit, W::kK32>(A, w, w + W::kPlane, lane, R, dR, tq[0], mnorm, raw_own, draw_own);
        else
            base_gradient_f32<TE>(A, w, lane, R, dR, tq[0], mnorm, raw_own, draw_own);

        // lane group 3 holds row c's raw density and its tangents: every lane group takes them, then the header's fp32 lines
        const float raw = __shfl(raw_own, 48 + c, 64);
        float dc[3], dl[3], gr[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float dn = __fmul_rn(__shfl(draw_own[a], 48 + c, 64), A.tangent_unscale);
            dc[a] = sel ? __fdiv_rn(dn, extent[a]) : 0.0f;
        }
        const float sg = det_expf(raw - 1.0f);
        const float slope = __builtin_fminf(sg, kExp15);
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const float jt = __fadd_rn(__fadd_rn(__fmul_rn(J[0][b], dc[0]), __fmul_rn(J[0][4 + b], dc[1])), __fmul_rn(J[0][8 + b], dc[2]));
            dl[b] = sel ? __fadd_rn(dc[b], jt) : 0.0f;
            gr[b] = sel ? __fmul_rn(slope, dl[b]) : 0.0f;
        }

        // lane group a < 3 stores component a, lane group 3 the density
        const int64_t s = tile_base + c;
        if (s >= n_eff) return;
        if (g == 3) {
            if (A.sigma) A.sigma[s] = sel ? sg : 0.0f;
            return;
        }
        const float o_dc = (g == 0) ? dc[0] : (g == 1) ? dc[1] : dc[2];
        const float o_dl = (g == 0) ? dl[0] : (g == 1) ? dl[1] : dl[2];
        const float o_gr = (g == 0) ? gr[0] : (g == 1) ? gr[1] : gr[2];
        if (A.dlog_canonical) A.dlog_canonical[3 * s + g] = o_dc;
        if (A.dlog) A.dlog[3 * s + g] = o_dl;
        if (A.grad) A.grad[3 * s + g] = o_gr;
    }
};

// the motion network and mlp_base, adjacent at the start of every blob
template <bool TE> using GradF32 = F32Weights<Blob<TE>::H0>;
template <bool TE, bool SPLIT, bool K32> using GradHalf = HalfWeights<HalfBlob<TE>::H0 * kFragHalves, SPLIT, K32>;

template <bool TE, bool F16, bool TEMPORAL> static void launch_gradient_table(const ced_field_desc *d, const GradArgs &A, void *stream)
{
    using Op = GradientOp<TE, F16, TEMPORAL>;
    const int mw = d->max_workgroups;
    if (d->mlp_precision == CED_MLP_F32 || d->mlp_precision == CED_MLP_F32_HEAD16X2)
        launch_tiles<Op, GradF32<TE>, 1>(A, mw, stream);
    else if (d->mlp_precision == CED_MLP_F16)
        launch_tiles<Op, GradHalf<TE, false, false>, 1>(A, mw, stream);
    else if constexpr (!TE && !TEMPORAL)                                 // half_layout_k32: the blob has the K = 32 placements
        launch_tiles<Op, GradHalf<TE, true, true>, 1>(A, mw, stream);
    else
        launch_tiles<Op, GradHalf<TE, true, false>, 1>(A, mw, stream);
}

// validates the hash table, fills A from the descriptor and launches
static int launch_gradient(const ced_field_desc *d, GradArgs &A, const char *who, void *stream)
{
    const ced_hash_desc &h = d->hash;
    int rc = validate_hash(&h, who);
    if (rc) return rc;
    CED_REQUIRE(h.n_levels == CED_MAX_LEVELS, "%s: the kernel needs n_levels == 16 (got %d)", who, h.n_levels);
    rc = require_32bit_byte_offsets(h, who);
    if (rc) return rc;
    static_assert(half_kernel_k32(false, false, true, 1024) && !half_kernel_k32(true, false, true, 1024) &&
                  !half_kernel_k32(false, true, true, 1024), "launch_gradient_table restates half_layout_k32");
    for (int i = 0; i < 6; ++i) A.aabb[i] = d->aabb[i];
    motion_args(d, A);
    A.time_mode = d->time_mode;
    A.raw_reg = d->mlp_precision == CED_MLP_F32_HEAD16X2 ? 3 : 0;
    A.table = h.table;
    float finest = 1.0f;
    for (int l = 0; l < CED_MAX_LEVELS; ++l) {
        CED_REQUIRE(h.scale[l] > 0.0f && h.scale[l] <= 1073741824.0f, "%s: level %d has scale %g", who, l, (double)h.scale[l]);
        finest = h.scale[l] > finest ? h.scale[l] : finest;
    }
    fill_levels(A.levels, h);
    int e = 0;
    const float m = frexpf(finest, &e);                                  // finest = m * 2^e, 0.5 <= m < 1
    const int K = m == 0.5f ? e - 1 : e;                                 // ceil(log2(finest)), 0 .. 30
    A.tangent_scale = ldexpf(1.0f, -K);
    A.tangent_unscale = ldexpf(1.0f, K);
    A.level_mode = hash_level_modes(h, false);
    switch ((d->time_mode ? 1 : 0) | (h.table_dtype ? 2 : 0) | (h.temporal ? 4 : 0)) {
    case 0: launch_gradient_table<false, false, false>(d, A, stream); break;
    case 1: launch_gradient_table<true, false, false>(d, A, stream); break;
    case 2: launch_gradient_table<false, true, false>(d, A, stream); break;
    case 3: launch_gradient_table<true, true, false>(d, A, stream); break;
    case 4: launch_gradient_table<false, false, true>(d, A, stream); break;
    case 5: launch_gradient_table<true, false, true>(d, A, stream); break;
    case 6: launch_gradient_table<false, true, true>(d, A, stream); break;
    default: launch_gradient_table<true, true, true>(d, A, stream); break;
    }
    return check_launch(who);
}

}  // namespace ced

extern "C" int ced_field_density_gradient(const ced_field_desc *desc, int64_t n, const float *positions, const float *t,
                                          float *sigma, float *grad, float *dlog, float *dlog_canonical, void *stream)
{
    const char *who = "field_density_gradient";
    ced::GradArgs A{};
    const int rc = ced::point_samples(desc, n, positions, t, sigma || grad || dlog || dlog_canonical, who, A.src);
    if (rc || n == 0) return rc;
    A.sigma = sigma; A.grad = grad; A.dlog = dlog; A.dlog_canonical = dlog_canonical;
    return ced::launch_gradient(desc, A, who, stream);
}

extern "C" int ced_field_density_gradient_rays(const ced_field_desc *desc, int64_t n, const int64_t *n_dev, const float *rays_o,
                                               const float *rays_d, const int64_t *ray_indices, const float *t_starts,
                                               const float *t_ends, const float *timestamps, int32_t t_per_ray, float *sigma,
                                               float *grad, float *dlog, float *dlog_canonical, void *stream)
{
    const char *who = "field_density_gradient_rays";
    ced::GradArgs A{};
    const int rc = ced::ray_samples(desc, n, n_dev, rays_o, rays_d, ray_indices, t_starts, t_ends, timestamps, t_per_ray,
                                    sigma || grad || dlog || dlog_canonical, who, A.src);
    if (rc || n == 0) return rc;
    A.sigma = sigma; A.grad = grad; A.dlog = dlog; A.dlog_canonical = dlog_canonical;
    return ced::launch_gradient(desc, A, who, stream);
}
