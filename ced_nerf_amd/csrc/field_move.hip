// The deformation field on its own: DNGPradianceField.query_move (cednerf/model.py:354-365) with the normalisation that
// follows it (:378-383), and DNGPradianceField._query_rgb (:447-466).  Inside the fused field kernels the move vector and
// the head's input only ever live in registers; these entries hand them out (ced_field_move, ced_field_move_rays) and
// take the head's input from memory (ced_field_rgb; ced_field_rgb_bcast for every embedding under every direction of a
// shared list, without expanding either in memory).  ced_field_move_inverse / ced_field_track solve x + move(x, t) = c
// for x by fixed-point iteration on the same device code, the iterate held in registers.
//
// They are built from the fused kernels' own device code -- mlp_layer / to_operand (field_kernel.hpp), mlp_layer_h /
// to_operand_h / to_half8 (field_half_device.hpp), the deterministic transcendentals of ced_common.hpp -- on the same
// packed blob read at the same offsets, in the arithmetic the descriptor's mlp_precision selects for that network:
//   motion network  f32, f32+h16x2: fp32 MFMA chain      f16: fp16 operands      f16x2: split fp16
//   colour head     f32: fp32 MFMA chain      f16: fp16 operands      f16x2, f32+h16x2: split fp16
// so a value computed here is the value the fused kernel computes internally, bit for bit.  Where the fused f16x2 kernel
// runs its hidden layers on the K-doubled v_mfma_f32_16x16x32_f16 (half_kernel_k32; the blob then carries the K = 32
// placements) these kernels evaluate that instruction's four blocks of eight products, in its order, on two
// v_mfma_f32_16x16x16_f16 (mlp_layer_k32_blocks, field_move_device.hpp): the K-doubled instruction stays confined to the
// two fused kernels that hold their SIMDs alone, and these short kernels need no residency rule.
//
// Shape: one network per 32-sample wave tile, workgroups persistent over tiles -- tile_kernel of field_move_device.hpp,
// which every entry here instantiates with an op (MoveOp, TrackOp, RgbOp) and the weights of the descriptor's arithmetic.
// MoveOp reads its rows from the SampleSrc of that header, which the two move entries fill through point_samples /
// ray_samples, the argument checks every per-sample entry makes.
// Only that network's layers are staged into LDS (motion: 44 KB fp32 or split fp16, 22 KB fp16; head: 28 KB / 14 KB), not
// the fused kernel's 86 KB, so two 512-thread workgroups share a CU.
#include "ced_common.hpp"
#include "field_device.hpp"
#include "field_half_device.hpp"
#include "field_kernel.hpp"
#include "field_move_device.hpp"

namespace ced {

struct MoveArgs {
    SampleSrc src;
    float *x_move, *move, *x_norm;                    // [n,3] each, any may be null
    uint8_t *selector;                                // [n], may be null
    float aabb[6];
    float moving_step;
    int use_div;
    const void *weights;                              // the motion network's first layer inside the packed blob
    int64_t lo_halves;                                // f16x2: halves from the plane of high parts to the plane of remainders
};

struct RgbArgs {
    int64_t n;
    const float *dir, *geo;                           // [n,3], [n,15]; broadcast: [n_dirs,3], [n / n_dirs,15]
    int64_t n_dirs;                                   // broadcast only: row r reads embedding r / n_dirs, direction r % n_dirs
    int apply_act;
    float *rgb;                                       // [n,3]
    const void *weights;                              // the head's first layer inside the packed blob
    int64_t lo_halves;
};

constexpr int kHeadFloats = Blob<false>::TOTAL - Blob<false>::H0;               // fp32 layers H0..H2
constexpr int kHeadHalves = Blob<false>::HEAD_FRAGS * kFragHalves;
static_assert(HalfBlob<false>::FRAGS - HalfBlob<false>::H0 == Blob<false>::HEAD_FRAGS &&
              HalfBlob<false>::H1 - HalfBlob<false>::H0 == Blob<false>::HF_H1 &&
              HalfBlob<false>::H2 - HalfBlob<false>::H0 == Blob<false>::HF_H2,
              "the head's fragments are laid out alike in the half blobs and in the mixed blob");

// x_move / normalise / selector (model.py:378-383) from `move` -- except that x_norm leaves unclamped, as the reference
// returns it.  Lane group a < 3 stores component a, lane group 3 the selector.
template <int NT>
__device__ __forceinline__ void move_store(const MoveArgs &A, const float (&mv)[NT][3], const float (&px)[NT][3], int64_t tile_base,
                                           int64_t n_eff, int g, int c)
{
    const float extent[3] = { A.aabb[3] - A.aabb[0], A.aabb[4] - A.aabb[1], A.aabb[5] - A.aabb[2] };
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        float xm[3], xn[3];
        bool inside = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            xm[a] = px[j][a] + mv[j][a];
            const float x = (xm[a] - A.aabb[a]) / extent[a];
            inside = inside && (x > 0.0f && x < 1.0f);
            xn[a] = x;
        }
        const int64_t s = tile_base + 16 * j + c;
        if (s >= n_eff) continue;
        if (g == 3) {
            if (A.selector) A.selector[s] = inside ? 1 : 0;
            continue;
        }
        const float o_move = (g == 0) ? mv[j][0] : (g == 1) ? mv[j][1] : mv[j][2];
        const float o_xm = (g == 0) ? xm[0] : (g == 1) ? xm[1] : xm[2];
        const float o_xn = (g == 0) ? xn[0] : (g == 1) ? xn[1] : xn[2];
        if (A.move) A.move[3 * s + g] = o_move;
        if (A.x_move) A.x_move[3 * s + g] = o_xm;
        if (A.x_norm) A.x_norm[3 * s + g] = o_xn;
    }
}

// ---- ced_field_move, ced_field_move_rays --------------------------------------------------------------------------------
struct MoveOp : SampleOp {
    using Args = MoveArgs;

    // eval frames: one timestamp for every sample, its two Frequency features of this lane computed once per workgroup
    // (field_kernel.hpp); only the fp32 chain asks for features
    struct Shared {
        bool on;
        float feat[2];
    };
    template <typename W> __device__ __forceinline__ static Shared prologue(const MoveArgs &A, int lane)
    {
        Shared sh{ A.src.rays_mode && !A.src.t_per_ray, { 0.0f, 0.0f } };
        if constexpr (!W::kHalf) {
            if (sh.on) {
                const int g = lane >> 4;
                const float t_all = A.src.timestamps[0];
#pragma unroll
                for (int S = 6; S < 8; ++S) sh.feat[S - 6] = det_sinpi_phase(t_all * (float)(1 << (2 * (S & 1) + (g >> 1))), g & 1);
            }
        }
        return sh;
    }
    // RowTime, except that the shared timestamp's features are taken as they are: the shortcut stays a branch inside the
    // encoding
    template <int NT> struct Time {
        const float (&tq)[NT];
        const Shared &sh;
        __device__ __forceinline__ float value(int j) const { return tq[j]; }
        __device__ __forceinline__ void features(int j, int g, float &f0, float &f1) const
        {
            if (sh.on) {
                f0 = sh.feat[0]; f1 = sh.feat[1];
            } else {
                time_features(tq[j], g, f0, f1);
            }
        }
    };

    template <typename W, int NT>
    __device__ __forceinline__ static void tile(const MoveArgs &A, const Shared &sh, const typename W::Elem *w, int64_t tile_base,
                                                int64_t n_eff, int lane)
    {
        const int g = lane >> 4, c = lane & 15;
        float px[NT][3], tq[NT], mv[NT][3];
        load_samples<NT>(A.src, tile_base, n_eff, c, px, tq);
        motion_move<W, NT>(w, lane, px, Time<NT>{ tq, sh }, A.moving_step, A.use_div, mv);
        move_store<NT>(A, mv, px, tile_base, n_eff, g, c);
    }
};

// ---- ced_field_move_inverse, ced_field_track: the fixed point on TrackRows (field_move_device.hpp) -----------------------
struct TrackOp : TileOp {
    using Args = TrackArgs;
    template <typename W, int NT>
    __device__ __forceinline__ static void tile(const TrackArgs &A, const Shared &, const typename W::Elem *w, int64_t tile_base,
                                                int64_t, int lane)
    {
        const int g = lane >> 4, c = lane & 15;
        TrackRows<NT> R;
        track_load<NT>(A, tile_base, c, R);
        const HeldTime<NT> time = hold_time<W, NT>(R.tq, g);
        for (int it = 0; it < A.max_iters; ++it) {
            float mv[NT][3];
            motion_move<W, NT>(opaque(w), lane, R.px, time, A.moving_step, A.use_div, mv);
            if (__ballot(track_update<NT>(mv, A.tol, R)) == 0) break;    // wave-uniform
        }
        track_store<NT>(A, R, tile_base, g, c);
    }
};

// SH coefficient g of the head's input (model.py:447-459), as the fused kernels evaluate it: lane group g normalises
// only the direction component it needs (Y00 const, Y1-1 ~ -y, Y10 ~ z, Y11 ~ -x; tcnn maps the unit vector to [0,1]
// and back).
__device__ __forceinline__ float sh_component(const float *__restrict__ dir, int64_t s, int g)
{
    float dv[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) dv[a] = dir[3 * s + a];
    const float nrm = __builtin_sqrtf((dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2]);
    const float comp = (g == 1) ? dv[1] : (g == 2) ? dv[2] : dv[0];
    const float u = (comp / nrm + 1.0f) / 2.0f;
    const float vv = u * 2.0f - 1.0f;
    const float coef = (g == 2) ? 0.48860251190291987f : -0.48860251190291987f;
    return (g == 0) ? 0.28209479177387814f : coef * vv;
}

// the rows of `dir` and `geo` that output row s reads
template <bool BCAST> __device__ __forceinline__ void rgb_rows(const RgbArgs &A, int64_t s, int64_t &sd, int64_t &se)
{
    if constexpr (BCAST) {
        se = s / A.n_dirs;
        sd = s - se * A.n_dirs;
    } else {
        sd = se = s;
    }
}

// colour channel a sits on accumulator row 4a = (lane group a, register 0): one sigmoid per lane
template <int NT>
__device__ __forceinline__ void rgb_store(const RgbArgs &A, const f4 (&D)[NT][4], int64_t tile_base, int g, int c)
{
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int64_t s = tile_base + 16 * j + c;
        const float raw = D[j][0][0];
        const float o1 = A.apply_act ? 1.0f / (1.0f + det_expf(-raw)) : raw;
        if (g < 3 && s < A.n) A.rgb[3 * s + g] = o1;
    }
}

// ---- ced_field_rgb, ced_field_rgb_bcast: the colour head on rows given one by one, or as embedding x direction -------------
template <bool BCAST> struct RgbOp : TileOp {
    using Args = RgbArgs;

    // fp32 MFMA chain (CED_MLP_F32)
    template <int NT>
    __device__ __forceinline__ static void head(const RgbArgs &A, const float *lw, int64_t tile_base, int lane, f4 (&D)[NT][4])
    {
        constexpr int H0 = 0, H1 = H0 + layer_floats(4, 5), H2 = H1 + layer_floats(4, 16);
        static_assert(H2 + layer_floats(1, 16) == kHeadFloats, "head layers");
        const int g = lane >> 4, c = lane & 15;
        float B[NT][16];
        // head input [SH(4), geo(15)], k = 4S + g: k-step 0 is SH_g, k-steps 1..3 geometry feature 4S + g - 4, k-step 4
        // features 12 + g (g < 3) -- what the fused kernel's mlp_base leaves in those registers (base_out_neuron)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            int64_t s = tile_base + 16 * j + c;
            s = s < A.n ? s : A.n - 1;
            int64_t sd, se;
            rgb_rows<BCAST>(A, s, sd, se);
            B[j][0] = sh_component(A.dir, sd, g);
#pragma unroll
            for (int S = 1; S < 4; ++S) B[j][S] = A.geo[se * 15 + 4 * S + g - 4];
            const float tail = A.geo[se * 15 + (g < 3 ? 12 + g : 14)];
            B[j][4] = (g == 3) ? 0.0f : tail;
        }
        mlp_layer<5, 4, NT>(lw + H0, lane, B, D);
        to_operand<4, true, NT>(D, B);
        mlp_layer<16, 4, NT>(lw + H1, lane, B, D);
        to_operand<4, true, NT>(D, B);
        mlp_layer<16, 1, NT>(lw + H2, lane, B, D);
    }

    // fp16 MFMAs (CED_MLP_F16, CED_MLP_F16X2, CED_MLP_F32_HEAD16X2)
    template <bool SPLIT, bool K32, int NT>
    __device__ __forceinline__ static void head_half(const RgbArgs &A, const _Float16 *whi, const _Float16 *wlo, int64_t tile_base,
                                                     int lane, f4 (&D)[NT][4])
    {
        using BL = Blob<false>;
        const int g = lane >> 4, c = lane & 15;
        h8 Bh[NT][2], Bl[NT][2];
        // operand element 0 = SH_g, 1..4 = geometry features 4g .. 4g + 3 (feature 15 does not exist), saturated to the
        // fp16 range as the fused kernels saturate their mlp_base outputs
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            int64_t s = tile_base + 16 * j + c;
            s = s < A.n ? s : A.n - 1;
            int64_t sd, se;
            rgb_rows<BCAST>(A, s, sd, se);
            float hin[8];
            hin[0] = sh_component(A.dir, sd, g);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = 4 * g + r < 15 ? 4 * g + r : 14;
                hin[1 + r] = __builtin_amdgcn_fmed3f(A.geo[se * 15 + f], -kHalfMax, kHalfMax);
            }
            hin[4] = (g == 3) ? 0.0f : hin[4];
            hin[5] = hin[6] = hin[7] = 0.0f;
            to_half8<SPLIT>(hin, Bh[j][0], Bl[j][0]);
        }
        mlp_layer_h<1, 4, NT, SPLIT>(whi + BL::HF_H0 * kFragHalves, wlo + BL::HF_H0 * kFragHalves, lane, Bh, Bl, D);
        to_operand_h<NT, SPLIT>(D, Bh, Bl);
        hidden_fed_layer<2, 4, NT, SPLIT, K32>(whi + BL::HF_H1 * kFragHalves, wlo + BL::HF_H1 * kFragHalves, lane, Bh, Bl, D);
        to_operand_h<NT, SPLIT>(D, Bh, Bl);
        hidden_fed_layer<2, 1, NT, SPLIT, K32>(whi + BL::HF_H2 * kFragHalves, wlo + BL::HF_H2 * kFragHalves, lane, Bh, Bl, D);
    }

    template <typename W, int NT>
    __device__ __forceinline__ static void tile(const RgbArgs &A, const Shared &, const typename W::Elem *w, int64_t tile_base, int64_t,
                                                int lane)
    {
        f4 D[NT][4];
        if constexpr (W::kHalf) head_half<W::kSplit, W::kK32, NT>(A, w, w + W::kPlane, tile_base, lane, D);
        else head<NT>(A, w, tile_base, lane, D);
        rgb_store<NT>(A, D, tile_base, lane >> 4, lane & 15);
    }
};

static int launch_move(const ced_field_desc *d, MoveArgs &A, const char *who, void *stream)
{
    for (int i = 0; i < 6; ++i) A.aabb[i] = d->aabb[i];
    return launch_motion<MoveOp, 2>(d, A, who, stream);
}

// the head in the descriptor's arithmetic; its layers sit behind the other networks' at an offset the time encoding moves
template <bool BCAST> static int launch_rgb(const ced_field_desc *desc, RgbArgs &A, const char *who, void *stream)
{
    using Op = RgbOp<BCAST>;
    const bool te = desc->time_mode != 0;
    const int mw = desc->max_workgroups;
    if (desc->mlp_precision == CED_MLP_F32) {
        A.weights = reinterpret_cast<const float *>(desc->packed_weights) + (te ? Blob<true>::H0 : Blob<false>::H0);
        launch_tiles<Op, F32Weights<kHeadFloats>, 2>(A, mw, stream);
    } else if (desc->mlp_precision == CED_MLP_F32_HEAD16X2) {
        // the mixed blob: fp16 fragments in the fp32 head's region, high parts then remainders, pair-form placements
        A.weights = reinterpret_cast<const float *>(desc->packed_weights) + (te ? Blob<true>::H0 : Blob<false>::H0);
        A.lo_halves = kHeadHalves;
        launch_tiles<Op, HalfWeights<kHeadHalves, true, false>, 2>(A, mw, stream);
    } else {
        A.weights = reinterpret_cast<const _Float16 *>(desc->packed_weights) +
                    (int64_t)(te ? HalfBlob<true>::H0 : HalfBlob<false>::H0) * kFragHalves;
        A.lo_halves = (int64_t)(te ? HalfBlob<true>::FRAGS : HalfBlob<false>::FRAGS) * kFragHalves;
        if (desc->mlp_precision == CED_MLP_F16)
            launch_tiles<Op, HalfWeights<kHeadHalves, false, false>, 2>(A, mw, stream);
        else if (half_layout_k32(desc->time_mode, desc->mlp_precision, desc->hash.temporal))
            launch_tiles<Op, HalfWeights<kHeadHalves, true, true>, 2>(A, mw, stream);
        else
            launch_tiles<Op, HalfWeights<kHeadHalves, true, false>, 2>(A, mw, stream);
    }
    return check_launch(who);
}

}  // namespace ced

extern "C" int ced_field_move(const ced_field_desc *desc, int64_t n, const float *positions, const float *t, float *x_move,
                              float *move, float *x_norm, uint8_t *selector, void *stream)
{
    ced::MoveArgs A{};
    const int rc = ced::point_samples(desc, n, positions, t, x_move || move || x_norm || selector, "field_move", A.src);
    if (rc || n == 0) return rc;
    A.x_move = x_move; A.move = move; A.x_norm = x_norm; A.selector = selector;
    return ced::launch_move(desc, A, "field_move", stream);
}

extern "C" int ced_field_move_rays(const ced_field_desc *desc, int64_t n, const int64_t *n_dev, const float *rays_o,
                                   const float *rays_d, const int64_t *ray_indices, const float *t_starts,
                                   const float *t_ends, const float *timestamps, int32_t t_per_ray, float *move,
                                   float *x_norm, void *stream)
{
    ced::MoveArgs A{};
    const int rc = ced::ray_samples(desc, n, n_dev, rays_o, rays_d, ray_indices, t_starts, t_ends, timestamps, t_per_ray,
                                    move || x_norm, "field_move_rays", A.src);
    if (rc || n == 0) return rc;
    A.move = move; A.x_norm = x_norm;
    return ced::launch_move(desc, A, "field_move_rays", stream);
}

extern "C" int ced_field_move_inverse(const ced_field_desc *desc, int64_t n, const float *target, const float *t,
                                      const float *init, int32_t max_iters, float tol, float *x, float *step,
                                      int32_t *evals, void *stream)
{
    return ced::solve_rows(desc, n, target, t, init, max_iters, tol, x, step, evals, "field_move_inverse",
                           ced::launch_motion<ced::TrackOp, 2>, stream);
}

extern "C" int ced_field_track(const ced_field_desc *desc, int64_t n_points, int64_t n_times, const float *target,
                               const float *times, const float *init, int32_t max_iters, float tol, float *x,
                               float *step, int32_t *evals, void *stream)
{
    return ced::solve_track(desc, n_points, n_times, target, times, init, max_iters, tol, x, step, evals, "field_track",
                            ced::launch_motion<ced::TrackOp, 2>, stream);
}

extern "C" int ced_field_rgb(const ced_field_desc *desc, int64_t n, const float *dirs, const float *embedding,
                             int32_t apply_act, float *rgb, void *stream)
{
    using namespace ced;
    int rc = validate_desc(desc, "field_rgb");
    if (rc) return rc;
    CED_REQUIRE(n >= 0, "field_rgb: n < 0");
    if (n == 0) return CED_OK;
    CED_REQUIRE(dirs && embedding && rgb, "field_rgb: null pointer");
    RgbArgs A{};
    A.n = n;
    A.dir = dirs; A.geo = embedding; A.apply_act = apply_act ? 1 : 0; A.rgb = rgb;
    return launch_rgb<false>(desc, A, "field_rgb", stream);
}

extern "C" int ced_field_rgb_bcast(const ced_field_desc *desc, int64_t m, int32_t n_dirs, const float *dirs,
                                   const float *embedding, int32_t apply_act, float *rgb, void *stream)
{
    using namespace ced;
    int rc = validate_desc(desc, "field_rgb_bcast");
    if (rc) return rc;
    CED_REQUIRE(m >= 0 && n_dirs >= 0, "field_rgb_bcast: m=%lld n_dirs=%d", (long long)m, n_dirs);
    CED_REQUIRE(m <= INT64_MAX / 3 / (n_dirs > 0 ? n_dirs : 1), "field_rgb_bcast: m * n_dirs overflows");
    if (m == 0 || n_dirs == 0) return CED_OK;
    CED_REQUIRE(dirs && embedding && rgb, "field_rgb_bcast: null pointer");
    RgbArgs A{};
    A.n = m * n_dirs;
    A.n_dirs = n_dirs;
    A.dir = dirs; A.geo = embedding; A.apply_act = apply_act ? 1 : 0; A.rgb = rgb;
    return launch_rgb<true>(desc, A, "field_rgb_bcast", stream);
}
