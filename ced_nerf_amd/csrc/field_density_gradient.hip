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
// one workgroup per CU.  All of that, x_norm, the level a gather slot reads and mlp_base with its tangent tiles are
// field_density_device.hpp's, shared with TimeMaxOp (field_time_max.hip); this file keeps what the tangents add: J, the
// gather with x-tangents, the header's fp32 lines and the stores.  The rows come from SampleSrc, which the two entries
// fill through point_samples / ray_samples.  ONE 16-row primal tile per wave iteration: stage 1 holds five operand and
// five accumulator tiles, stage 4 four and four beside J and the 32 gathered values; two waves per SIMD, no scratch
// (DESIGN 4.1d).
#include "field_density_device.hpp"
#include "field_jacobian_device.hpp"

namespace ced {

struct GradArgs : DensityArgs {
    SampleSrc src;
    float *sigma, *grad, *dlog, *dlog_canonical;      // [n], [n,3] x 3; any may be null
    float tangent_scale, tangent_unscale;             // 2^-K, 2^K
};

constexpr float kExp15 = 3269017.25f;                 // the float32 nearest e^15: trunc_exp's backward clamps there
constexpr int kGradDirs = 3;                          // tangent directions: x_norm's three axes

// ---- ced_field_density_gradient, ced_field_density_gradient_rays: one 16-row tile per wave iteration -----------------------
template <bool TE, bool F16, bool TEMPORAL> struct GradientOp : SampleOp, DensityLevels<F16, TEMPORAL> {
    using Args = GradArgs;
    using DensityLevels<F16, TEMPORAL>::levels;
    using DensityLevels<F16, TEMPORAL>::fill_lds;
    static constexpr int kPerCu = 1;
    static constexpr int kTiles = 1;                  // one primal tile beside its three tangent tiles

    // w = the tile's LDS base of the staged layers
    template <typename W, int NT>
    __device__ __forceinline__ static void tile(const GradArgs &A, const Shared &, const typename W::Elem *w, int64_t tile_base,
                                                int64_t n_eff, int lane)
    {
        static_assert(NT == kTiles, "one primal tile beside its three tangent tiles");
        const int g = lane >> 4, c = lane & 15;
        float px[1][3], tq[1], mv[1][3], J[1][12];
        load_samples<1>(A.src, tile_base, n_eff, c, px, tq);
        motion_move_jacobian<W, 1>(w, lane, px, RowTime<1>{ tq }, A.moving_step, A.use_div, mv, J);

        float xn[1][3], mnorm[1];
        bool sel[1];
        canonical_point<TE, 1>(A.aabb, px, mv, xn, sel, mnorm);

        // the lane's four levels: features and x-tangents from the same corner loads
        float R[1][8], dR[kGradDirs][8];
        int k_lo = 0;
        float t_frac = 0.0f;
        if constexpr (TEMPORAL) temporal_keyframe(tq[0], k_lo, t_frac);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const LevelConst L = load_level(levels() + slot_level<W>(i, g) * 8);
            float d0[3], d1[3];
            if (((A.level_mode >> (2 * i)) & 3) == 2)
                hash_level_dx<F16, TEMPORAL, 2>(L, A.table, xn[0], k_lo, t_frac, A.tangent_scale, R[0][2 * i], R[0][2 * i + 1], d0, d1);
            else
                hash_level_dx<F16, TEMPORAL, 0>(L, A.table, xn[0], k_lo, t_frac, A.tangent_scale, R[0][2 * i], R[0][2 * i + 1], d0, d1);
#pragma unroll
            for (int b = 0; b < kGradDirs; ++b) {
                dR[b][2 * i] = d0[b];
                dR[b][2 * i + 1] = d1[b];
            }
        }

        float raw_own[1], draw_own[kGradDirs];
        mlp_base<W, TE, 1, kGradDirs>(A, w, lane, R, dR, tq[0], mnorm, raw_own, draw_own);

        // lane group 3 holds row c's raw density and its tangents: every lane group takes them, then the header's fp32 lines
        const float raw = __shfl(raw_own[0], 48 + c, 64);
        float dc[3], dl[3], gr[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float dn = __fmul_rn(__shfl(draw_own[a], 48 + c, 64), A.tangent_unscale);
            dc[a] = sel[0] ? __fdiv_rn(dn, A.aabb[3 + a] - A.aabb[a]) : 0.0f;
        }
        const float sg = det_expf(raw - 1.0f);
        const float slope = __builtin_fminf(sg, kExp15);
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const float jt = __fadd_rn(__fadd_rn(__fmul_rn(J[0][b], dc[0]), __fmul_rn(J[0][4 + b], dc[1])), __fmul_rn(J[0][8 + b], dc[2]));
            dl[b] = sel[0] ? __fadd_rn(dc[b], jt) : 0.0f;
            gr[b] = sel[0] ? __fmul_rn(slope, dl[b]) : 0.0f;
        }

        // lane group a < 3 stores component a, lane group 3 the density
        const int64_t s = tile_base + c;
        if (s >= n_eff) return;
        if (g == 3) {
            if (A.sigma) A.sigma[s] = sel[0] ? sg : 0.0f;
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

// fills A from the descriptor (the tangents' scale from the finest level's) and launches
static int launch_gradient(const ced_field_desc *d, GradArgs &A, const char *who, void *stream)
{
    const int rc = fill_density_args(d, A, who);
    if (rc) return rc;
    const ced_hash_desc &h = d->hash;
    float finest = 1.0f;
    for (int l = 0; l < CED_MAX_LEVELS; ++l) {
        CED_REQUIRE(h.scale[l] > 0.0f && h.scale[l] <= 1073741824.0f, "%s: level %d has scale %g", who, l, (double)h.scale[l]);
        finest = h.scale[l] > finest ? h.scale[l] : finest;
    }
    int e = 0;
    const float m = frexpf(finest, &e);                                  // finest = m * 2^e, 0.5 <= m < 1
    const int K = m == 0.5f ? e - 1 : e;                                 // ceil(log2(finest)), 0 .. 30
    A.tangent_scale = ldexpf(1.0f, -K);
    A.tangent_unscale = ldexpf(1.0f, K);
    return launch_density<GradientOp>(d, A, who, stream);
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
