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
// v_mfma_f32_16x16x16_f16 (mlp_layer_k32_blocks below): the K-doubled instruction stays confined to the two fused kernels
// that hold their SIMDs alone, and these short kernels need no residency rule.
//
// Shape: one network per 32-sample wave tile, workgroups persistent over tiles (wave w of workgroup b takes tiles
// b * WAVES + w, + gridDim.x * WAVES, ...).  Only that network's layers are staged into LDS (motion: 44 KB fp32 or split
// fp16, 22 KB fp16; head: 28 KB / 14 KB), not the fused kernel's 86 KB, so two 512-thread workgroups share a CU.
#include "ced_common.hpp"
#include "field_device.hpp"
#include "field_half_device.hpp"
#include "field_kernel.hpp"
#include "field_move_device.hpp"

namespace ced {

struct MoveArgs {
    int64_t n;
    const int64_t *n_dev;                             // optional device-side sample count (<= n)
    const float *pos, *t;                             // explicit mode
    const float *rays_o, *rays_d;                     // rays mode
    const int64_t *ray_idx;
    const float *t0, *t1, *timestamps;
    int rays_mode, t_per_ray;
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

__device__ __forceinline__ int64_t sample_count(int64_t n, const int64_t *n_dev)
{
    if (!n_dev) return n;
    const int64_t nd = *n_dev;
    return nd < n ? nd : n;
}

// Position and time of sample c of each 16-sample column tile: the expressions of field_kernel.hpp / field_half.hip
// (rays mode: o + (d * (t0 + t1)) / 2 in fp32; a negative ray index is evaluated on ray 0 at distance 0).  A ragged last
// tile repeats the last sample (never stored).
template <int NT>
__device__ __forceinline__ void load_samples(const MoveArgs &A, int64_t tile_base, int64_t n_eff, int c, float (&px)[NT][3],
                                             float (&tq)[NT])
{
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        int64_t s = tile_base + 16 * j + c;
        s = s < n_eff ? s : n_eff - 1;
        if (A.rays_mode) {
            const int64_t r_in = A.ray_idx[s];
            const bool used = r_in >= 0;
            const int64_t r = used ? r_in : 0;
            const float tm2 = used ? A.t0[s] + A.t1[s] : 0.0f;
#pragma unroll
            for (int a = 0; a < 3; ++a) px[j][a] = A.rays_o[3 * r + a] + (A.rays_d[3 * r + a] * tm2) / 2.0f;
            tq[j] = A.t_per_ray ? A.timestamps[r] : A.timestamps[0];
        } else {
#pragma unroll
            for (int a = 0; a < 3; ++a) px[j][a] = A.pos[3 * s + a];
            tq[j] = A.t[s];
        }
    }
}

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

// ---- motion network, fp32 MFMA chain (CED_MLP_F32, CED_MLP_F32_HEAD16X2) ------------------------------------------
template <int NT, int THREADS>
__global__ __launch_bounds__(THREADS) void move_kernel(MoveArgs A)
{
    constexpr int WAVES = THREADS / kWave;
    constexpr int TILE = 16 * NT;
    __shared__ __attribute__((aligned(16))) float lds[kMotionFloats];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int g = lane >> 4, c = lane & 15;
    const int64_t n_eff = sample_count(A.n, A.n_dev);
    const int64_t n_tiles = (n_eff + TILE - 1) / TILE;
    if ((int64_t)blockIdx.x * WAVES >= n_tiles) return;                 // workgroup-uniform

    stage<THREADS>(lds, A.weights, kMotionFloats / 4, tid);
    __syncthreads();

    // eval frames: one timestamp for every sample, its two Frequency features of this lane computed once (field_kernel.hpp)
    const bool shared_time = A.rays_mode && !A.t_per_ray;
    float t_feat[2] = { 0.0f, 0.0f };
    if (shared_time) {
        const float t_all = A.timestamps[0];
#pragma unroll
        for (int S = 6; S < 8; ++S) t_feat[S - 6] = det_sinpi_phase(t_all * (float)(1 << (2 * (S & 1) + (g >> 1))), g & 1);
    }

    for (int64_t tile = (int64_t)blockIdx.x * WAVES + (tid >> 6); tile < n_tiles; tile += (int64_t)gridDim.x * WAVES) {
        // opaque LDS base per tile: keeps the A-fragment reads inside the loop (see field_kernel.hpp)
        int lds_off = 0;
        asm volatile("" : "+v"(lds_off));
        const float *const lw = lds + lds_off;
        float px[NT][3], tq[NT], mv[NT][3];
        load_samples<NT>(A, tile * TILE, n_eff, c, px, tq);
        const auto time = [&](int j, float &f0, float &f1) {
            if (shared_time) {
                f0 = t_feat[0]; f1 = t_feat[1];
            } else {
                time_features(tq[j], g, f0, f1);
            }
        };
        motion_move<NT>(lw, lane, px, time, A.moving_step, A.use_div, mv);
        move_store<NT>(A, mv, px, tile * TILE, n_eff, g, c);
    }
}

// ---- motion network on fp16 MFMAs (CED_MLP_F16, CED_MLP_F16X2; K32: the blob has half_kernel_k32's placements) ----
template <bool SPLIT, bool K32, int NT, int THREADS>
__global__ __launch_bounds__(THREADS) void move_half_kernel(MoveArgs A)
{
    static_assert(!K32 || SPLIT, "only the f16x2 blob has K = 32 placements");
    constexpr int WAVES = THREADS / kWave;
    constexpr int TILE = 16 * NT;
    __shared__ __attribute__((aligned(16))) _Float16 lds[kMotionHalves * (SPLIT ? 2 : 1)];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int g = lane >> 4, c = lane & 15;
    const int64_t n_eff = sample_count(A.n, A.n_dev);
    const int64_t n_tiles = (n_eff + TILE - 1) / TILE;
    if ((int64_t)blockIdx.x * WAVES >= n_tiles) return;                 // workgroup-uniform

    stage<THREADS>(lds, A.weights, kMotionHalves / 8, tid);
    if constexpr (SPLIT)
        stage<THREADS>(lds + kMotionHalves, reinterpret_cast<const _Float16 *>(A.weights) + A.lo_halves, kMotionHalves / 8, tid);
    __syncthreads();

    for (int64_t tile = (int64_t)blockIdx.x * WAVES + (tid >> 6); tile < n_tiles; tile += (int64_t)gridDim.x * WAVES) {
        int lds_off = 0;
        asm volatile("" : "+v"(lds_off));
        const _Float16 *const whi = lds + lds_off;
        const _Float16 *const wlo = whi + kMotionHalves;
        float px[NT][3], tq[NT], mv[NT][3];
        load_samples<NT>(A, tile * TILE, n_eff, c, px, tq);
        motion_move_half<SPLIT, K32, NT>(whi, wlo, lane, px, tq, A.moving_step, A.use_div, mv);
        move_store<NT>(A, mv, px, tile * TILE, n_eff, g, c);
    }
}

template <int NT, int THREADS>
__global__ __launch_bounds__(THREADS) void track_kernel(TrackArgs A)
{
    constexpr int WAVES = THREADS / kWave;
    constexpr int TILE = 16 * NT;
    __shared__ __attribute__((aligned(16))) float lds[kMotionFloats];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int g = lane >> 4, c = lane & 15;
    const int64_t n_tiles = (A.n + TILE - 1) / TILE;
    if ((int64_t)blockIdx.x * WAVES >= n_tiles) return;                 // workgroup-uniform

    stage<THREADS>(lds, A.weights, kMotionFloats / 4, tid);
    __syncthreads();

    for (int64_t tile = (int64_t)blockIdx.x * WAVES + (tid >> 6); tile < n_tiles; tile += (int64_t)gridDim.x * WAVES) {
        TrackRows<NT> R;
        track_load<NT>(A, tile * TILE, c, R);
        float tf[NT][2];
#pragma unroll
        for (int j = 0; j < NT; ++j) time_features(R.tq[j], g, tf[j][0], tf[j][1]);   // the time does not move: once per tile
        const auto time = [&](int j, float &f0, float &f1) { f0 = tf[j][0]; f1 = tf[j][1]; };
        for (int it = 0; it < A.max_iters; ++it) {
            // opaque LDS base per round: keeps the A-fragment reads inside the loop (see field_kernel.hpp)
            int lds_off = 0;
            asm volatile("" : "+v"(lds_off));
            float mv[NT][3];
            motion_move<NT>(lds + lds_off, lane, R.px, time, A.moving_step, A.use_div, mv);
            if (__ballot(track_update<NT>(mv, A.tol, R)) == 0) break;    // wave-uniform
        }
        track_store<NT>(A, R, tile * TILE, g, c);
    }
}

template <bool SPLIT, bool K32, int NT, int THREADS>
__global__ __launch_bounds__(THREADS) void track_half_kernel(TrackArgs A)
{
    static_assert(!K32 || SPLIT, "only the f16x2 blob has K = 32 placements");
    constexpr int WAVES = THREADS / kWave;
    constexpr int TILE = 16 * NT;
    __shared__ __attribute__((aligned(16))) _Float16 lds[kMotionHalves * (SPLIT ? 2 : 1)];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int g = lane >> 4, c = lane & 15;
    const int64_t n_tiles = (A.n + TILE - 1) / TILE;
    if ((int64_t)blockIdx.x * WAVES >= n_tiles) return;                 // workgroup-uniform

    stage<THREADS>(lds, A.weights, kMotionHalves / 8, tid);
    if constexpr (SPLIT)
        stage<THREADS>(lds + kMotionHalves, reinterpret_cast<const _Float16 *>(A.weights) + A.lo_halves, kMotionHalves / 8, tid);
    __syncthreads();

    for (int64_t tile = (int64_t)blockIdx.x * WAVES + (tid >> 6); tile < n_tiles; tile += (int64_t)gridDim.x * WAVES) {
        TrackRows<NT> R;
        track_load<NT>(A, tile * TILE, c, R);
        for (int it = 0; it < A.max_iters; ++it) {
            int lds_off = 0;
            asm volatile("" : "+v"(lds_off));
            const _Float16 *const whi = lds + lds_off;
            float mv[NT][3];
            motion_move_half<SPLIT, K32, NT>(whi, whi + kMotionHalves, lane, R.px, R.tq, A.moving_step, A.use_div, mv);
            if (__ballot(track_update<NT>(mv, A.tol, R)) == 0) break;    // wave-uniform
        }
        track_store<NT>(A, R, tile * TILE, g, c);
    }
}

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

// ---- colour head, fp32 MFMA chain (CED_MLP_F32) --------------------------------------------------------------------
template <int NT, int THREADS, bool BCAST = false>
__global__ __launch_bounds__(THREADS) void rgb_kernel(RgbArgs A)
{
    constexpr int WAVES = THREADS / kWave;
    constexpr int TILE = 16 * NT;
    constexpr int H0 = 0, H1 = H0 + layer_floats(4, 5), H2 = H1 + layer_floats(4, 16);
    static_assert(H2 + layer_floats(1, 16) == kHeadFloats, "head layers");
    __shared__ __attribute__((aligned(16))) float lds[kHeadFloats];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int g = lane >> 4, c = lane & 15;
    const int64_t n_tiles = (A.n + TILE - 1) / TILE;
    if ((int64_t)blockIdx.x * WAVES >= n_tiles) return;

    stage<THREADS>(lds, A.weights, kHeadFloats / 4, tid);
    __syncthreads();

    for (int64_t tile = (int64_t)blockIdx.x * WAVES + (tid >> 6); tile < n_tiles; tile += (int64_t)gridDim.x * WAVES) {
        int lds_off = 0;
        asm volatile("" : "+v"(lds_off));
        const float *const lw = lds + lds_off;
        float B[NT][16];
        f4 D[NT][4];
        // head input [SH(4), geo(15)], k = 4S + g: k-step 0 is SH_g, k-steps 1..3 geometry feature 4S + g - 4, k-step 4
        // features 12 + g (g < 3) -- what the fused kernel's mlp_base leaves in those registers (base_out_neuron)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            int64_t s = tile * TILE + 16 * j + c;
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
        rgb_store<NT>(A, D, tile * TILE, g, c);
    }
}

// ---- colour head on fp16 MFMAs (CED_MLP_F16, CED_MLP_F16X2, CED_MLP_F32_HEAD16X2) -------------------------------------
template <bool SPLIT, bool K32, int NT, int THREADS, bool BCAST = false>
__global__ __launch_bounds__(THREADS) void rgb_half_kernel(RgbArgs A)
{
    static_assert(!K32 || SPLIT, "only the f16x2 blob has K = 32 placements");
    constexpr int WAVES = THREADS / kWave;
    constexpr int TILE = 16 * NT;
    using BL = Blob<false>;
    __shared__ __attribute__((aligned(16))) _Float16 lds[kHeadHalves * (SPLIT ? 2 : 1)];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int g = lane >> 4, c = lane & 15;
    const int64_t n_tiles = (A.n + TILE - 1) / TILE;
    if ((int64_t)blockIdx.x * WAVES >= n_tiles) return;                 // workgroup-uniform

    stage<THREADS>(lds, A.weights, kHeadHalves / 8, tid);
    if constexpr (SPLIT)
        stage<THREADS>(lds + kHeadHalves, reinterpret_cast<const _Float16 *>(A.weights) + A.lo_halves, kHeadHalves / 8, tid);
    __syncthreads();

    for (int64_t tile = (int64_t)blockIdx.x * WAVES + (tid >> 6); tile < n_tiles; tile += (int64_t)gridDim.x * WAVES) {
        int lds_off = 0;
        asm volatile("" : "+v"(lds_off));
        const _Float16 *const whi = lds + lds_off;
        const _Float16 *const wlo = whi + kHeadHalves;
        h8 Bh[NT][2], Bl[NT][2];
        f4 D[NT][4];
        // operand element 0 = SH_g, 1..4 = geometry features 4g .. 4g + 3 (feature 15 does not exist), saturated to the
        // fp16 range as the fused kernels saturate their mlp_base outputs
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            int64_t s = tile * TILE + 16 * j + c;
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
        rgb_store<NT>(A, D, tile * TILE, g, c);
    }
}

static int launch_move(const ced_field_desc *d, MoveArgs &A, const char *who, void *stream)
{
    for (int i = 0; i < 6; ++i) A.aabb[i] = d->aabb[i];
    A.moving_step = d->moving_step;
    A.use_div = d->use_div_offsets ? 1 : 0;
    A.weights = d->packed_weights;                    // every blob starts with the motion network
    A.lo_halves = (int64_t)(d->time_mode ? HalfBlob<true>::FRAGS : HalfBlob<false>::FRAGS) * kFragHalves;
    const int mw = d->max_workgroups;
    if (d->mlp_precision == CED_MLP_F32 || d->mlp_precision == CED_MLP_F32_HEAD16X2)
        launch_tiles<2, 512>(move_kernel<2, 512>, A, A.n, 2, mw, stream);
    else if (d->mlp_precision == CED_MLP_F16)
        launch_tiles<2, 512>(move_half_kernel<false, false, 2, 512>, A, A.n, 2, mw, stream);
    else if (half_layout_k32(d->time_mode, d->mlp_precision, d->hash.temporal))
        launch_tiles<2, 512>(move_half_kernel<true, true, 2, 512>, A, A.n, 2, mw, stream);
    else
        launch_tiles<2, 512>(move_half_kernel<true, false, 2, 512>, A, A.n, 2, mw, stream);
    return check_launch(who);
}

// the fixed-point kernel for the descriptor's arithmetic: launch_move's four variants, the same launch geometry
static int launch_track(const ced_field_desc *d, TrackArgs &A, const char *who, void *stream)
{
    A.moving_step = d->moving_step;
    A.use_div = d->use_div_offsets ? 1 : 0;
    A.weights = d->packed_weights;
    A.lo_halves = (int64_t)(d->time_mode ? HalfBlob<true>::FRAGS : HalfBlob<false>::FRAGS) * kFragHalves;
    const int mw = d->max_workgroups;
    if (d->mlp_precision == CED_MLP_F32 || d->mlp_precision == CED_MLP_F32_HEAD16X2)
        launch_tiles<2, 512>(track_kernel<2, 512>, A, A.n, 2, mw, stream);
    else if (d->mlp_precision == CED_MLP_F16)
        launch_tiles<2, 512>(track_half_kernel<false, false, 2, 512>, A, A.n, 2, mw, stream);
    else if (half_layout_k32(d->time_mode, d->mlp_precision, d->hash.temporal))
        launch_tiles<2, 512>(track_half_kernel<true, true, 2, 512>, A, A.n, 2, mw, stream);
    else
        launch_tiles<2, 512>(track_half_kernel<true, false, 2, 512>, A, A.n, 2, mw, stream);
    return check_launch(who);
}

// the head's kernel for the descriptor's arithmetic, on rows given one by one (ced_field_rgb) or as embedding x direction
template <bool BCAST> static int launch_rgb(const ced_field_desc *desc, RgbArgs &A, const char *who, void *stream)
{
    const int64_t n = A.n;
    const bool te = desc->time_mode != 0;
    const int mw = desc->max_workgroups;
    if (desc->mlp_precision == CED_MLP_F32) {
        A.weights = reinterpret_cast<const float *>(desc->packed_weights) + (te ? Blob<true>::H0 : Blob<false>::H0);
        launch_tiles<2, 512>(rgb_kernel<2, 512, BCAST>, A, n, 2, mw, stream);
    } else if (desc->mlp_precision == CED_MLP_F32_HEAD16X2) {
        // the mixed blob: fp16 fragments in the fp32 head's region, high parts then remainders, pair-form placements
        A.weights = reinterpret_cast<const float *>(desc->packed_weights) + (te ? Blob<true>::H0 : Blob<false>::H0);
        A.lo_halves = kHeadHalves;
        launch_tiles<2, 512>(rgb_half_kernel<true, false, 2, 512, BCAST>, A, n, 2, mw, stream);
    } else {
        A.weights = reinterpret_cast<const _Float16 *>(desc->packed_weights) +
                    (int64_t)(te ? HalfBlob<true>::H0 : HalfBlob<false>::H0) * kFragHalves;
        A.lo_halves = (int64_t)(te ? HalfBlob<true>::FRAGS : HalfBlob<false>::FRAGS) * kFragHalves;
        if (desc->mlp_precision == CED_MLP_F16)
            launch_tiles<2, 512>(rgb_half_kernel<false, false, 2, 512, BCAST>, A, n, 2, mw, stream);
        else if (half_layout_k32(desc->time_mode, desc->mlp_precision, desc->hash.temporal))
            launch_tiles<2, 512>(rgb_half_kernel<true, true, 2, 512, BCAST>, A, n, 2, mw, stream);
        else
            launch_tiles<2, 512>(rgb_half_kernel<true, false, 2, 512, BCAST>, A, n, 2, mw, stream);
    }
    return check_launch(who);
}

}  // namespace ced

extern "C" int ced_field_move(const ced_field_desc *desc, int64_t n, const float *positions, const float *t, float *x_move,
                              float *move, float *x_norm, uint8_t *selector, void *stream)
{
    int rc = ced::validate_desc(desc, "field_move");
    if (rc) return rc;
    CED_REQUIRE(n >= 0, "field_move: n < 0");
    if (n == 0) return CED_OK;
    CED_REQUIRE(positions && t, "field_move: null positions/t");
    CED_REQUIRE(x_move || move || x_norm || selector, "field_move: no output requested");
    ced::MoveArgs A{};
    A.n = n;
    A.pos = positions; A.t = t;
    A.x_move = x_move; A.move = move; A.x_norm = x_norm; A.selector = selector;
    return ced::launch_move(desc, A, "field_move", stream);
}

extern "C" int ced_field_move_rays(const ced_field_desc *desc, int64_t n, const int64_t *n_dev, const float *rays_o,
                                   const float *rays_d, const int64_t *ray_indices, const float *t_starts,
                                   const float *t_ends, const float *timestamps, int32_t t_per_ray, float *move,
                                   float *x_norm, void *stream)
{
    int rc = ced::validate_desc(desc, "field_move_rays");
    if (rc) return rc;
    CED_REQUIRE(n >= 0, "field_move_rays: n < 0");
    if (n == 0) return CED_OK;
    CED_REQUIRE(rays_o && rays_d && ray_indices && t_starts && t_ends && timestamps, "field_move_rays: null pointer");
    CED_REQUIRE(move || x_norm, "field_move_rays: no output requested");
    ced::MoveArgs A{};
    A.n = n;
    A.n_dev = n_dev;
    A.rays_o = rays_o; A.rays_d = rays_d; A.ray_idx = ray_indices;
    A.t0 = t_starts; A.t1 = t_ends; A.timestamps = timestamps;
    A.rays_mode = 1; A.t_per_ray = t_per_ray ? 1 : 0;
    A.move = move; A.x_norm = x_norm;
    return ced::launch_move(desc, A, "field_move_rays", stream);
}

extern "C" int ced_field_move_inverse(const ced_field_desc *desc, int64_t n, const float *target, const float *t,
                                      const float *init, int32_t max_iters, float tol, float *x, float *step,
                                      int32_t *evals, void *stream)
{
    int rc = ced::validate_desc(desc, "field_move_inverse");
    if (rc) return rc;
    CED_REQUIRE(n >= 0, "field_move_inverse: n < 0");
    rc = ced::validate_solve(max_iters, tol, "field_move_inverse");
    if (rc) return rc;
    if (n == 0) return CED_OK;
    CED_REQUIRE(target && t, "field_move_inverse: null target/t");
    CED_REQUIRE(x || step || evals, "field_move_inverse: no output requested");
    ced::TrackArgs A{};
    A.n = n;
    A.target = target; A.t = t; A.init = init;
    A.max_iters = max_iters; A.tol = tol;
    A.x = x; A.step = step; A.evals = evals;
    return ced::launch_track(desc, A, "field_move_inverse", stream);
}

extern "C" int ced_field_track(const ced_field_desc *desc, int64_t n_points, int64_t n_times, const float *target,
                               const float *times, const float *init, int32_t max_iters, float tol, float *x,
                               float *step, int32_t *evals, void *stream)
{
    int rc = ced::validate_desc(desc, "field_track");
    if (rc) return rc;
    CED_REQUIRE(n_points >= 0 && n_times >= 0, "field_track: n_points=%lld n_times=%lld", (long long)n_points,
                (long long)n_times);
    CED_REQUIRE(n_points <= INT64_MAX / 3 / (n_times > 0 ? n_times : 1), "field_track: n_points * n_times overflows");
    rc = ced::validate_solve(max_iters, tol, "field_track");
    if (rc) return rc;
    if (n_points == 0 || n_times == 0) return CED_OK;
    CED_REQUIRE(target && times, "field_track: null target/times");
    CED_REQUIRE(x || step || evals, "field_track: no output requested");
    ced::TrackArgs A{};
    A.n = n_points * n_times;
    A.n_points = n_points;
    A.bcast = 1;
    A.target = target; A.t = times; A.init = init;
    A.max_iters = max_iters; A.tol = tol;
    A.x = x; A.step = step; A.evals = evals;
    return ced::launch_track(desc, A, "field_track", stream);
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
