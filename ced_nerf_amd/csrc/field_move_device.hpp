// Device code of the motion network and of the colour head on their own, shared by field_move.hip (ced_field_move,
// ced_field_move_inverse, ced_field_track, ced_field_rgb), field_jacobian.hip (ced_field_move_jacobian, the Newton
// inverse, ced_field_velocity) and field_density_gradient.hip (ced_field_density_gradient).
//
// Every kernel of the three files is tile_kernel<Op, W, NT, THREADS>.  The skeleton fixes, once: the wave's tiles of
// 16 * NT rows (wave w of workgroup b takes tiles b * WAVES + w, + gridDim.x * WAVES, ...), the workgroup-uniform early
// return, the staging of the layers into LDS and its barrier, and the opaque LDS base of each tile.
//   W, the weights (F32Weights, HalfWeights): the LDS element type, the size of one plane, whether a plane of remainders
//      follows it (in LDS directly behind, in the blob A.lo_halves after A.weights), whether the blob has the K = 32
//      placements.  A tile body gets the base of the first plane.
//   Op, what one tile does: its Args (the kernel's argument; weights and lo_halves are read here), tile(), and -- where
//      TileOp's defaults do not fit -- the row count, what else the workgroup puts into LDS before the barrier, a
//      once-per-workgroup prologue whose result every tile receives, and how many workgroups share a CU.
// The per-sample entries (move, velocity, density gradient; each with a rays twin) read their rows from one SampleSrc, the
// first member of their Args: sample_count / load_samples on the device, point_samples / ray_samples -- the entries'
// argument checks, stated once -- on the host.
// Below them: the encode -> four layers -> move chain in the three arithmetics (motion_move), the K = 32 blocks on the
// K = 16 instruction, the rows a solver keeps in registers, and the launch / validation helpers of the entries.  One
// statement of the arithmetic, so every kernel built on it computes ced_field_move's bits.
#pragma once
#include "ced_common.hpp"
#include "field_device.hpp"
#include "field_half_device.hpp"
#include "field_kernel.hpp"

namespace ced {

// Where a per-sample entry takes its rows from: positions and times given one by one, or the samples of a ray batch as
// ced_field_forward_rays reads them.  The first member of MoveArgs, VelArgs and GradArgs.
struct SampleSrc {
    int64_t n;
    const int64_t *n_dev;                             // optional device-side sample count (<= n)
    const float *pos, *t;                             // explicit mode
    const float *rays_o, *rays_d;                     // rays mode
    const int64_t *ray_idx;
    const float *t0, *t1, *timestamps;
    int rays_mode, t_per_ray;
};

// the inverse of the warp by fixed-point iteration (ced_field_move_inverse, ced_field_track)
struct TrackArgs {
    int64_t n;                                        // rows
    int64_t n_points;                                 // broadcast: row r reads target / start r % n_points, time r / n_points
    int bcast;
    const float *target, *t, *init;                   // [n,3], [n], [n,3] or null; broadcast: [P,3], [T], [P,3] or null
    int max_iters;
    float tol;
    float *x, *step;                                  // [n,3], [n], either may be null
    int32_t *evals;                                   // [n], may be null
    float moving_step;
    int use_div;
    const void *weights;
    int64_t lo_halves;
};

static_assert(HalfBlob<true>::B0 == HalfBlob<false>::B0 && Blob<true>::B0 == Blob<false>::B0,
              "the motion network sits at the start of the blob with or without a time encoding");
constexpr int kMotionFloats = Blob<false>::B0;                                  // fp32 layers M0..M3
constexpr int kMotionHalves = HalfBlob<false>::B0 * kFragHalves;                // the same as fp16 fragments, one plane

// `count` 16-byte words of weights into LDS
template <int THREADS> __device__ __forceinline__ void stage(void *dst, const void *src, int count, int tid)
{
    const f4 *s = reinterpret_cast<const f4 *>(src);
    f4 *d = reinterpret_cast<f4 *>(dst);
    for (int i = tid; i < count; i += THREADS) d[i] = s[i];
}

// ---- what a kernel stages ------------------------------------------------------------------------------------------
template <int FLOATS> struct F32Weights {             // fp32 layers for the fp32 MFMA chain
    using Elem = float;
    static constexpr int kPlane = FLOATS;
    static constexpr bool kHalf = false, kSplit = false, kK32 = false;
};
template <int HALVES, bool SPLIT, bool K32> struct HalfWeights {   // fp16 fragments; SPLIT: high parts, then remainders
    static_assert(!K32 || SPLIT, "only the f16x2 blob has K = 32 placements");
    using Elem = _Float16;
    static constexpr int kPlane = HALVES;
    static constexpr bool kHalf = true, kSplit = SPLIT, kK32 = K32;
};

// what an op leaves to the skeleton unless it says otherwise: A.n rows, nothing but the weights in LDS, nothing computed
// once per workgroup, two workgroups per CU
struct TileOp {
    struct Shared {};
    static constexpr int kPerCu = 2;
    template <typename Args> static int64_t capacity(const Args &A) { return A.n; }       // the rows the grid is sized for
    template <typename Args> __device__ __forceinline__ static int64_t rows(const Args &A) { return A.n; }
    template <typename Args> __device__ __forceinline__ static void fill_lds(const Args &, int) {}    // before the barrier
    template <typename W, typename Args> __device__ __forceinline__ static Shared prologue(const Args &, int) { return {}; }
};

// An LDS base the compiler cannot see through: keeps the A-fragment reads inside the loop it is taken in (see
// field_kernel.hpp).  The skeleton takes it per tile; a solver, which evaluates the network up to max_iters times per
// tile, takes it again per round.
template <typename T> __device__ __forceinline__ const T *opaque(const T *lds)
{
    int lds_off = 0;
    asm volatile("" : "+v"(lds_off));
    return lds + lds_off;
}

template <typename Op, typename W, int NT, int THREADS>
__global__ __launch_bounds__(THREADS) void tile_kernel(typename Op::Args A)
{
    using Elem = typename W::Elem;
    constexpr int WAVES = THREADS / kWave;
    constexpr int TILE = 16 * NT;
    constexpr int kPlaneWords = W::kPlane * (int)sizeof(Elem) / 16;
    __shared__ __attribute__((aligned(16))) Elem lds[W::kPlane * (W::kSplit ? 2 : 1)];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int64_t n = Op::rows(A);
    const int64_t n_tiles = (n + TILE - 1) / TILE;
    if ((int64_t)blockIdx.x * WAVES >= n_tiles) return;                 // workgroup-uniform

    const Elem *const blob = reinterpret_cast<const Elem *>(A.weights);
    stage<THREADS>(lds, blob, kPlaneWords, tid);
    if constexpr (W::kSplit) stage<THREADS>(lds + W::kPlane, blob + A.lo_halves, kPlaneWords, tid);
    Op::fill_lds(A, tid);
    __syncthreads();

    const typename Op::Shared shared = Op::template prologue<W>(A, lane);
    for (int64_t tile = (int64_t)blockIdx.x * WAVES + (tid >> 6); tile < n_tiles; tile += (int64_t)gridDim.x * WAVES)
        Op::template tile<W, NT>(A, shared, opaque(lds), tile * TILE, n, lane);
}

// position and time of sample c of each 16-sample column tile, rows given one by one; a ragged last tile repeats the last
// sample (never stored)
template <int NT>
__device__ __forceinline__ void load_points(const float *pos, const float *t, int64_t n, int64_t tile_base, int c,
                                            float (&px)[NT][3], float (&tq)[NT])
{
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        int64_t s = tile_base + 16 * j + c;
        s = s < n ? s : n - 1;
#pragma unroll
        for (int a = 0; a < 3; ++a) px[j][a] = pos[3 * s + a];
        tq[j] = t[s];
    }
}

// the rows of a per-sample entry: n, or the device-side count where one is given and smaller
__device__ __forceinline__ int64_t sample_count(const SampleSrc &A)
{
    if (!A.n_dev) return A.n;
    const int64_t nd = *A.n_dev;
    return nd < A.n ? nd : A.n;
}

// an op on the rows of a SampleSrc, the member `src` of its Args
struct SampleOp : TileOp {
    template <typename Args> static int64_t capacity(const Args &A) { return A.src.n; }
    template <typename Args> __device__ __forceinline__ static int64_t rows(const Args &A) { return sample_count(A.src); }
};

// Position and time of sample c of each 16-sample column tile: load_points, or the expressions of field_kernel.hpp /
// field_half.hip (rays mode: o + (d * (t0 + t1)) / 2 in fp32; a negative ray index is evaluated on ray 0 at distance 0).
// A ragged last tile repeats the last sample (never stored).
template <int NT>
__device__ __forceinline__ void load_samples(const SampleSrc &A, int64_t tile_base, int64_t n_eff, int c, float (&px)[NT][3],
                                             float (&tq)[NT])
{
    if (!A.rays_mode) return load_points<NT>(A.pos, A.t, n_eff, tile_base, c, px, tq);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        int64_t s = tile_base + 16 * j + c;
        s = s < n_eff ? s : n_eff - 1;
        const int64_t r_in = A.ray_idx[s];
        const bool used = r_in >= 0;
        const int64_t r = used ? r_in : 0;
        const float tm2 = used ? A.t0[s] + A.t1[s] : 0.0f;
#pragma unroll
        for (int a = 0; a < 3; ++a) px[j][a] = A.rays_o[3 * r + a] + (A.rays_d[3 * r + a] * tm2) / 2.0f;
        tq[j] = A.t_per_ray ? A.timestamps[r] : A.timestamps[0];
    }
}

// The last layer's accumulators hold the output rows naturally: offset a on (lane group 0, register a), fine offset a
// (row 3 + a) on (g0,r3), (g1,r0), (g1,r1).  fine_row: that row's value of column c; fine_tanh: the tanh the fused
// kernels take of it.
__device__ __forceinline__ float fine_row(const f4 &D0, int a, int c)
{
    constexpr int kFineReg[3] = { 3, 0, 1 };
    return __shfl(D0[kFineReg[a]], (a == 0) ? c : 16 + c, 64);
}

__device__ __forceinline__ float fine_tanh(float fine)
{
    const float e = det_expf(2.0f * fine);
    return 1.0f - 2.0f / (e + 1.0f);
}

// query_move's `move` (model.py:354-365) from the motion network's accumulators, as the fused kernels state it.  Every
// lane gets all three components of its column's samples.
template <int NT>
__device__ __forceinline__ void move_vector(const f4 (&D)[NT][4], float moving_step, int use_div, int c, float (&mv)[NT][3])
{
#pragma unroll
    for (int j = 0; j < NT; ++j) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float off = __shfl(D[j][0][a], c, 64);
            float m = off * moving_step;
            if (use_div) m = m + fine_tanh(fine_row(D[j][0], a, c)) * moving_step;
            mv[j][a] = m;
        }
    }
}

// ---- a K = 32 layer without the K-doubled instruction --------------------------------------------------------------
// v_mfma_f32_16x16x32_f16 consumes lane group q's eight operand elements as block q of eight products, q = 0..3, each
// block rounded once onto the accumulator; v_mfma_f32_16x16x16_f16 consumes lane groups {0,1}, then {2,3}, four elements
// each, as two such blocks; the order of the products inside a block is irrelevant (oracle/mfma_f16_model.h).  So one
// K = 32 instruction on operands (a, b) IS two K = 16 instructions on regrouped operands: the first takes from lane group
// G the elements 4(G&1) .. 4(G&1)+3 of K = 32 lane group G>>1 (its blocks: K = 32 blocks 0, 1), the second the same of lane
// group 2 + (G>>1) (blocks 2, 3).  The weights are read from LDS at the regrouped address, the activations are regrouped
// across lanes once per layer.  Same blocks, same order, same bits as mlp_layer_h<..., K32 = true> on the K = 32 blob.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void regroup_k32(const h8 &b, int src_lane, bool upper, h4 &b01, h4 &b23)
{
    const u32x4 w = __builtin_bit_cast(u32x4, b);
    uint32_t x01[4], x23[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        x01[k] = (uint32_t)__shfl((int)w[k], src_lane, 64);
        x23[k] = (uint32_t)__shfl((int)w[k], src_lane + 32, 64);
    }
    b01 = __builtin_bit_cast(h4, u32x2{ upper ? x01[2] : x01[0], upper ? x01[3] : x01[1] });
    b23 = __builtin_bit_cast(h4, u32x2{ upper ? x23[2] : x23[0], upper ? x23[3] : x23[1] });
}

template <int KS, int NB, int NT>
__device__ __forceinline__ void mlp_layer_k32_blocks(const _Float16 *__restrict__ whi, const _Float16 *__restrict__ wlo, int lane,
                                                     const h8 (&Bh)[NT][2], const h8 (&Bl)[NT][2], f4 (&D)[NT][4])
{
    const int g = lane >> 4, c = lane & 15;
    const int src_lane = 16 * (g >> 1) + c;               // the K = 32 lane whose elements this lane feeds to blocks 0 / 1
    const bool upper = (g & 1) != 0;
    const int a01 = src_lane * 8 + (upper ? 4 : 0), a23 = a01 + 32 * 8;
    h4 bh01[NT][KS], bh23[NT][KS], bl01[NT][KS], bl23[NT][KS];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            regroup_k32(Bh[j][ks], src_lane, upper, bh01[j][ks], bh23[j][ks]);
            regroup_k32(Bl[j][ks], src_lane, upper, bl01[j][ks], bl23[j][ks]);
        }
    }
    f4 acc[NT];
#pragma unroll
    for (int grp = 0; grp < NB * KS; ++grp) {
        const int nb = grp / KS, ks = grp % KS;
        if (ks == 0) {
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j] = f4{ 0.0f, 0.0f, 0.0f, 0.0f };
        }
        const h4 ah01 = *reinterpret_cast<const h4 *>(whi + grp * kFragHalves + a01);
        const h4 ah23 = *reinterpret_cast<const h4 *>(whi + grp * kFragHalves + a23);
        const h4 al01 = *reinterpret_cast<const h4 *>(wlo + grp * kFragHalves + a01);
        const h4 al23 = *reinterpret_cast<const h4 *>(wlo + grp * kFragHalves + a23);
        // the three products of the split, in mlp_layer_h's order: lo * hi, hi * lo, hi * hi
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x16f16(al01, bh01[j][ks], acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x16f16(al23, bh23[j][ks], acc[j], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x16f16(ah01, bl01[j][ks], acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x16f16(ah23, bl23[j][ks], acc[j], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x16f16(ah01, bh01[j][ks], acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x16f16(ah23, bh23[j][ks], acc[j], 0, 0, 0);
        }
        if (ks == KS - 1) {
#pragma unroll
            for (int j = 0; j < NT; ++j) D[j][nb] = acc[j];
        }
    }
}

// a layer fed by a hidden layer: on the pair form, or (K32L: the blob has the K = 32 placements) on that form's blocks
template <int KS, int NB, int NT, bool SPLIT, bool K32L>
__device__ __forceinline__ void hidden_fed_layer(const _Float16 *__restrict__ whi, const _Float16 *__restrict__ wlo, int lane,
                                                 const h8 (&Bh)[NT][2], const h8 (&Bl)[NT][2], f4 (&D)[NT][4])
{
    if constexpr (K32L) mlp_layer_k32_blocks<KS, NB, NT>(whi, wlo, lane, Bh, Bl, D);
    else mlp_layer_h<KS, NB, NT, SPLIT>(whi, wlo, lane, Bh, Bl, D);
}

// ---- the motion network on one wave tile: encode -> four layers -> move -------------------------------------------------
// Shared by the ops that hand `move` out once and by the solvers that evaluate it up to max_iters times on a position
// held in registers: one statement of the arithmetic, so every evaluation has ced_field_move's bits.

// fp32 chain: the two Frequency features of time tq that lane group g feeds (field_kernel.hpp: k = 4S + g, S = 6, 7)
__device__ __forceinline__ void time_features(float tq, int g, float &f0, float &f1)
{
    const float sc0 = (float)(1 << (g >> 1)), sc1 = 4.0f * sc0;
    const float scz = (g & 1) != 0 ? sc1 : sc0;
    float p0, p1;
    det_sinpi_both(tq * scz, p0, p1);
    const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(p0), __float_as_uint(p1), false, false);
    f0 = __uint_as_float(sw[0]); f1 = __uint_as_float(sw[1]);
}

// Where a chain takes the time of column tile j from: the fp16 encodings ask for its value, the fp32 encoding for the two
// features of it that the lane feeds.  RowTime: each row's own time, the features made where the encoding wants them, so
// no feature array is live beside the operands.  HeldTime (hold_time): a solver's rows, whose time does not move -- the
// features are made once per tile.
template <int NT> struct RowTime {
    const float (&tq)[NT];
    __device__ __forceinline__ float value(int j) const { return tq[j]; }
    __device__ __forceinline__ void features(int j, int g, float &f0, float &f1) const { time_features(tq[j], g, f0, f1); }
};

template <int NT> struct HeldTime {
    const float (&tq)[NT];
    float tf[NT][2];
    __device__ __forceinline__ float value(int j) const { return tq[j]; }
    __device__ __forceinline__ void features(int j, int, float &f0, float &f1) const { f0 = tf[j][0]; f1 = tf[j][1]; }
};

template <typename W, int NT> __device__ __forceinline__ HeldTime<NT> hold_time(const float (&tq)[NT], int g)
{
    HeldTime<NT> held{ tq, {} };
    if constexpr (!W::kHalf) {
#pragma unroll
        for (int j = 0; j < NT; ++j) time_features(tq[j], g, held.tf[j][0], held.tf[j][1]);
    }
    return held;
}

// fp32 chain: tcnn Frequency(4) on (x,y,z,t) in the fused kernel's operand order (field_kernel.hpp: k = 4S + g): B[j][0 .. 7]
template <int NT, typename Time>
__device__ __forceinline__ void motion_encode(const float (&px)[NT][3], const Time &time, int g, float (&B)[NT][16])
{
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const bool odd = (g & 1) != 0;
        const float sc0 = (float)(1 << (g >> 1)), sc1 = 4.0f * sc0;
        const float vxy = odd ? px[j][1] : px[j][0];
        float p0, p1;
        det_sinpi_both(vxy * sc0, p0, p1);
        auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(p0), __float_as_uint(p1), false, false);
        B[j][0] = __uint_as_float(sw[0]); B[j][2] = __uint_as_float(sw[1]);
        det_sinpi_both(vxy * sc1, p0, p1);
        sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(p0), __float_as_uint(p1), false, false);
        B[j][1] = __uint_as_float(sw[0]); B[j][3] = __uint_as_float(sw[1]);
        const float scz = odd ? sc1 : sc0;
        det_sinpi_both(px[j][2] * scz, p0, p1);
        sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(p0), __float_as_uint(p1), false, false);
        B[j][4] = __uint_as_float(sw[0]); B[j][5] = __uint_as_float(sw[1]);
        time.features(j, g, B[j][6], B[j][7]);
    }
}

// fp16 operands: tcnn Frequency(4), lane group g owns dimension g; e = 2 * freq + phase (field_half.hip)
__device__ __forceinline__ void motion_features_half(const float (&px)[3], float tq, int g, float (&f)[8])
{
    float v = tq;
    v = (g == 0) ? px[0] : v;
    v = (g == 1) ? px[1] : v;
    v = (g == 2) ? px[2] : v;
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = det_sinpi_phase(v * (float)(1 << (e >> 1)), e & 1);
}

// fp32 MFMA chain (CED_MLP_F32, CED_MLP_F32_HEAD16X2): lw = the staged layers M0..M3
template <int NT, typename Time>
__device__ __forceinline__ void motion_move_f32(const float *lw, int lane, const float (&px)[NT][3], const Time &time,
                                                float moving_step, int use_div, float (&mv)[NT][3])
{
    using BL = Blob<false>;
    const int g = lane >> 4, c = lane & 15;
    float B[NT][16];
    f4 D[NT][4];
    motion_encode<NT>(px, time, g, B);
    mlp_layer<8, 4, NT>(lw + BL::M0, lane, B, D);
    to_operand<4, true, NT>(D, B);
    mlp_layer<16, 4, NT>(lw + BL::M1, lane, B, D);
    to_operand<4, true, NT>(D, B);
    mlp_layer<16, 4, NT>(lw + BL::M2, lane, B, D);
    to_operand<4, true, NT>(D, B);
    mlp_layer<16, 1, NT>(lw + BL::M3, lane, B, D);
    move_vector<NT>(D, moving_step, use_div, c, mv);
}

// fp16 MFMAs (CED_MLP_F16, CED_MLP_F16X2; K32: the blob has half_kernel_k32's placements): whi / wlo = the staged planes
template <bool SPLIT, bool K32, int NT, typename Time>
__device__ __forceinline__ void motion_move_half(const _Float16 *whi, const _Float16 *wlo, int lane, const float (&px)[NT][3],
                                                 const Time &time, float moving_step, int use_div, float (&mv)[NT][3])
{
    using BL = HalfBlob<false>;
    const int g = lane >> 4, c = lane & 15;
    h8 Bh[NT][2], Bl[NT][2];
    f4 D[NT][4];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        float f[8];
        motion_features_half(px[j], time.value(j), g, f);
        to_half8<SPLIT>(f, Bh[j][0], Bl[j][0]);
    }
    mlp_layer_h<1, 4, NT, SPLIT>(whi + BL::M0 * kFragHalves, wlo + BL::M0 * kFragHalves, lane, Bh, Bl, D);
    to_operand_h<NT, SPLIT>(D, Bh, Bl);
    hidden_fed_layer<2, 4, NT, SPLIT, K32>(whi + BL::M1 * kFragHalves, wlo + BL::M1 * kFragHalves, lane, Bh, Bl, D);
    to_operand_h<NT, SPLIT>(D, Bh, Bl);
    hidden_fed_layer<2, 4, NT, SPLIT, K32>(whi + BL::M2 * kFragHalves, wlo + BL::M2 * kFragHalves, lane, Bh, Bl, D);
    to_operand_h<NT, SPLIT>(D, Bh, Bl);
    hidden_fed_layer<2, 1, NT, SPLIT, K32>(whi + BL::M3 * kFragHalves, wlo + BL::M3 * kFragHalves, lane, Bh, Bl, D);
    move_vector<NT>(D, moving_step, use_div, c, mv);
}

// the chain in the arithmetic of the staged weights W; w = the tile's LDS base
template <typename W, int NT, typename Time>
__device__ __forceinline__ void motion_move(const typename W::Elem *w, int lane, const float (&px)[NT][3], const Time &time,
                                            float moving_step, int use_div, float (&mv)[NT][3])
{
    if constexpr (W::kHalf) motion_move_half<W::kSplit, W::kK32, NT>(w, w + W::kPlane, lane, px, time, moving_step, use_div, mv);
    else motion_move_f32<NT>(w, lane, px, time, moving_step, use_div, mv);
}

// ---- the warp's inverse: x + move(x, t) = target by fixed-point iteration (include/cednerf_hip.h states it) -----------
// A wave tile keeps target, time and the iterate of its 32 rows in registers (every lane group holds the same copy of
// column c's rows) and calls the motion network's device function once per round.  A row that has met `step <= tol`
// is frozen: its registers no longer take the round's result, so its outputs are those of the round it stopped at
// whatever the other rows of the tile do (and MFMA columns do not mix).  The loop leaves early only when the ballot
// finds no active row in the wave; rows past n are never active.
template <int NT> struct TrackRows {
    float target[NT][3], px[NT][3], tq[NT], step[NT];
    int evals[NT];
    bool active[NT];
};

template <int NT>
__device__ __forceinline__ void track_load(const TrackArgs &A, int64_t tile_base, int c, TrackRows<NT> &R)
{
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int64_t row = tile_base + 16 * j + c;
        const int64_t s = row < A.n ? row : A.n - 1;                     // a ragged last tile repeats the last row
        int64_t sp = s, st = s;
        if (A.bcast) {
            st = s / A.n_points;
            sp = s - st * A.n_points;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            R.target[j][a] = A.target[3 * sp + a];
            R.px[j][a] = A.init ? A.init[3 * sp + a] : R.target[j][a];
        }
        R.tq[j] = A.t[st];
        R.step[j] = __builtin_inff();
        R.evals[j] = 0;
        R.active[j] = row < A.n;
    }
}

// one round on the rows still active: x_new = target - move, step = max_a |x_new[a] - x[a]|, freeze at step <= tol.
// Returns whether any row of this lane is still active.
template <int NT>
__device__ __forceinline__ bool track_update(const float (&mv)[NT][3], float tol, TrackRows<NT> &R)
{
    bool any = false;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        float xn[3], d[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            xn[a] = R.target[j][a] - mv[j][a];
            d[a] = __builtin_fabsf(xn[a] - R.px[j][a]);
        }
        const float step = fmaxf(fmaxf(d[0], d[1]), d[2]);
        const bool on = R.active[j];                                     // a frozen row keeps what it has
#pragma unroll
        for (int a = 0; a < 3; ++a) R.px[j][a] = on ? xn[a] : R.px[j][a];
        R.step[j] = on ? step : R.step[j];
        R.evals[j] += on ? 1 : 0;
        R.active[j] = on && !(step <= tol);                              // a NaN step stays active
        any = any || R.active[j];
    }
    return any;
}

// lane group a < 3 stores component a of x, lane group 3 step and evals
template <int NT>
__device__ __forceinline__ void track_store(const TrackArgs &A, const TrackRows<NT> &R, int64_t tile_base, int g, int c)
{
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int64_t s = tile_base + 16 * j + c;
        const float x0 = R.px[j][0], x1 = R.px[j][1], x2 = R.px[j][2];
        const float o = (g == 0) ? x0 : (g == 1) ? x1 : x2;
        if (s >= A.n) continue;
        if (g == 3) {
            if (A.step) A.step[s] = R.step[j];
            if (A.evals) A.evals[s] = R.evals[j];
            continue;
        }
        if (A.x) A.x[3 * s + g] = o;
    }
}

// Persistent launch of Op on the weights W, NT 16-row tiles per wave: workgroups of 512 threads, enough for the tiles, at
// most Op::kPerCu per CU (the descriptor's max_workgroups caps it).
template <typename Op, typename W, int NT>
static void launch_tiles(const typename Op::Args &A, int max_workgroups, void *stream)
{
    constexpr int THREADS = 512;
    const int64_t n_tiles = (Op::capacity(A) + 16 * NT - 1) / (16 * NT);
    constexpr int waves = THREADS / 64;
    int64_t blocks = (n_tiles + waves - 1) / waves;
    const int64_t cap = max_workgroups > 0 ? max_workgroups : (int64_t)kFieldBlocksDefault * Op::kPerCu;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL((tile_kernel<Op, W, NT, THREADS>), dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, A);
}

// what every op on the motion network reads from the descriptor
template <typename Args> static void motion_args(const ced_field_desc *d, Args &A)
{
    A.moving_step = d->moving_step;
    A.use_div = d->use_div_offsets ? 1 : 0;
    A.weights = d->packed_weights;                    // every blob starts with the motion network
    A.lo_halves = (int64_t)(d->time_mode ? HalfBlob<true>::FRAGS : HalfBlob<false>::FRAGS) * kFragHalves;
}

// Op on the motion network in the descriptor's arithmetic: the fp32 chain, fp16 operands, or split fp16 on the blob's
// K = 32 placements or on the pair form
template <typename Op, int NT> static int launch_motion(const ced_field_desc *d, typename Op::Args &A, const char *who, void *stream)
{
    motion_args(d, A);
    const int mw = d->max_workgroups;
    if (d->mlp_precision == CED_MLP_F32 || d->mlp_precision == CED_MLP_F32_HEAD16X2)
        launch_tiles<Op, F32Weights<kMotionFloats>, NT>(A, mw, stream);
    else if (d->mlp_precision == CED_MLP_F16)
        launch_tiles<Op, HalfWeights<kMotionHalves, false, false>, NT>(A, mw, stream);
    else if (half_layout_k32(d->time_mode, d->mlp_precision, d->hash.temporal))
        launch_tiles<Op, HalfWeights<kMotionHalves, true, true>, NT>(A, mw, stream);
    else
        launch_tiles<Op, HalfWeights<kMotionHalves, true, false>, NT>(A, mw, stream);
    return check_launch(who);
}

// the descriptor fields these entries read; the hash table is not touched, but its kind selects the blob's layout
static int validate_desc(const ced_field_desc *d, const char *who)
{
    CED_REQUIRE(d != nullptr, "%s: null descriptor", who);
    CED_REQUIRE(d->time_mode >= 0 && d->time_mode <= 2, "%s: time_mode=%d", who, d->time_mode);
    CED_REQUIRE(d->packed_weights != nullptr, "%s: null packed_weights", who);
    CED_REQUIRE(d->mlp_precision >= CED_MLP_F32 && d->mlp_precision <= CED_MLP_F32_HEAD16X2, "%s: mlp_precision=%d", who,
                d->mlp_precision);
    CED_REQUIRE((int64_t)d->packed_floats == ced_packed_weight_words(d->use_div_offsets, d->time_mode, d->mlp_precision),
                "%s: packed_floats=%llu does not match this configuration (mlp_precision %d)", who,
                (unsigned long long)d->packed_floats, d->mlp_precision);
    CED_REQUIRE(d->max_workgroups >= 0 && d->max_workgroups <= 65536, "%s: max_workgroups=%d", who, d->max_workgroups);
    return CED_OK;
}

// What the per-sample entries check before they look at their outputs, in this order: the descriptor, n < 0, n == 0 -- the
// caller returns CED_OK on it before any pointer is looked at --, null inputs, no output requested.  They fill S.
static int point_samples(const ced_field_desc *d, int64_t n, const float *positions, const float *t, bool any_output,
                         const char *who, SampleSrc &S)
{
    int rc = validate_desc(d, who);
    if (rc) return rc;
    CED_REQUIRE(n >= 0, "%s: n < 0", who);
    if (n == 0) return CED_OK;
    CED_REQUIRE(positions && t, "%s: null positions/t", who);
    CED_REQUIRE(any_output, "%s: no output requested", who);
    S.n = n;
    S.pos = positions; S.t = t;
    return CED_OK;
}

static int ray_samples(const ced_field_desc *d, int64_t n, const int64_t *n_dev, const float *rays_o, const float *rays_d,
                       const int64_t *ray_indices, const float *t_starts, const float *t_ends, const float *timestamps,
                       int32_t t_per_ray, bool any_output, const char *who, SampleSrc &S)
{
    int rc = validate_desc(d, who);
    if (rc) return rc;
    CED_REQUIRE(n >= 0, "%s: n < 0", who);
    if (n == 0) return CED_OK;
    CED_REQUIRE(rays_o && rays_d && ray_indices && t_starts && t_ends && timestamps, "%s: null pointer", who);
    CED_REQUIRE(any_output, "%s: no output requested", who);
    S.n = n;
    S.n_dev = n_dev;
    S.rays_o = rays_o; S.rays_d = rays_d; S.ray_idx = ray_indices;
    S.t0 = t_starts; S.t1 = t_ends; S.timestamps = timestamps;
    S.rays_mode = 1; S.t_per_ray = t_per_ray ? 1 : 0;
    return CED_OK;
}

static int validate_solve(int32_t max_iters, float tol, const char *who)
{
    CED_REQUIRE(max_iters >= 1 && max_iters <= 1024, "%s: max_iters=%d outside 1 .. 1024", who, max_iters);
    CED_REQUIRE(tol >= 0.0f, "%s: tol=%g must be >= 0 (and not a NaN)", who, (double)tol);
    return CED_OK;
}

// ---- the bodies of the solver entries: `launch` is the fixed-point or the Newton op on the motion network ------------------
typedef int (*SolveLaunch)(const ced_field_desc *, TrackArgs &, const char *, void *);

// ced_field_move_inverse, ced_field_move_inverse_newton: rows given one by one
static int solve_rows(const ced_field_desc *desc, int64_t n, const float *target, const float *t, const float *init,
                      int32_t max_iters, float tol, float *x, float *step, int32_t *evals, const char *who, SolveLaunch launch,
                      void *stream)
{
    int rc = validate_desc(desc, who);
    if (rc) return rc;
    CED_REQUIRE(n >= 0, "%s: n < 0", who);
    rc = validate_solve(max_iters, tol, who);
    if (rc) return rc;
    if (n == 0) return CED_OK;
    CED_REQUIRE(target && t, "%s: null target/t", who);
    CED_REQUIRE(x || step || evals, "%s: no output requested", who);
    TrackArgs A{};
    A.n = n;
    A.target = target; A.t = t; A.init = init;
    A.max_iters = max_iters; A.tol = tol;
    A.x = x; A.step = step; A.evals = evals;
    return launch(desc, A, who, stream);
}

// ced_field_track, ced_field_track_newton: every (time, point) pair
static int solve_track(const ced_field_desc *desc, int64_t n_points, int64_t n_times, const float *target, const float *times,
                       const float *init, int32_t max_iters, float tol, float *x, float *step, int32_t *evals, const char *who,
                       SolveLaunch launch, void *stream)
{
    int rc = validate_desc(desc, who);
    if (rc) return rc;
    CED_REQUIRE(n_points >= 0 && n_times >= 0, "%s: n_points=%lld n_times=%lld", who, (long long)n_points, (long long)n_times);
    CED_REQUIRE(n_points <= INT64_MAX / 3 / (n_times > 0 ? n_times : 1), "%s: n_points * n_times overflows", who);
    rc = validate_solve(max_iters, tol, who);
    if (rc) return rc;
    if (n_points == 0 || n_times == 0) return CED_OK;
    CED_REQUIRE(target && times, "%s: null target/times", who);
    CED_REQUIRE(x || step || evals, "%s: no output requested", who);
    TrackArgs A{};
    A.n = n_points * n_times;
    A.n_points = n_points;
    A.bcast = 1;
    A.target = target; A.t = times; A.init = init;
    A.max_iters = max_iters; A.tol = tol;
    A.x = x; A.step = step; A.evals = evals;
    return launch(desc, A, who, stream);
}

}  // namespace ced
