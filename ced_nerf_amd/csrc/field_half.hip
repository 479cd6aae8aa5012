// Half-precision-MFMA variants of the fused dynamic-NGP field (same fusion and same interface as
// field_kernel.hpp; selected by ced_field_desc.mlp_precision):
//
//   CED_MLP_F16X2 (1): every MLP operand is split into two fp16 numbers, x = hi + lo (22 significant
//       bits), and each product block is three fp16 MFMA blocks (hi*hi + hi*lo + lo*hi) with
//       fp32 accumulation -- fp32-grade results (~1e-6 relative) at a fraction of the fp32-MFMA time.
//   CED_MLP_F16   (2): operands rounded to fp16, fp32 accumulation: the precision class of the
//       reference's tiny-cuda-nn FullyFusedMLP (cednerf/model.py:200-222,280-309) and of
//       BASELINE config 5 ("fp16 hash features + fp16 MFMA MLP").
//
// Outside the GEMMs everything is the same deterministic fp32 code as the exact kernel (field_device.hpp, det_expf,
// IEEE division / square root): encodings (Frequency / SH / time), hash-grid gather and interpolation, position
// normalisation, trunc_exp, tanh, sigmoid.  Together with the CPU model of the matrix instruction
// (oracle/mfma_f16_model.h: two blocks of eight products per v_mfma_f32_16x16x16_f16, each cut below
// 2^(Emax - 24) and rounded once) every output of these kernels is reproducible on the CPU bit for bit.
//
// Geometry: D^T = W * X^T as in field_kernel.hpp, but K = 32 per product block (mfma_k32, field_half_device.hpp): lane (g = lane>>4, c = lane&15) supplies
// inputs 32ks + 8g + e (e = 0..7, four packed VGPRs) of sample c, and receives accumulator rows 4g + r.
// The host packs the weight rows of every 64-wide hidden layer so that accumulator row 16nb + 4g + r
// holds neuron 32(nb>>1) + 8g + 4(nb&1) + r: the eight values a lane needs as operand of k-step ks are
// then its own registers D[2ks][0..3], D[2ks+1][0..3] -- activations never move between lanes.  The
// inputs are laid out likewise: lane group g computes the eight Frequency features of dimension g,
// gathers hash levels {g, 4+g, 8+g, 12+g} (input columns are permuted on the host to match), and the
// last layer of mlp_base is packed so that a lane's four outputs are its own mlp_head inputs.
#include <cstring>

#include "ced_common.hpp"
#include "field_args.hpp"
#include "field_device.hpp"
#include "field_half_device.hpp"
#include "hash_device.hpp"

namespace ced {

// Rays-mode front end of a tile: two batches of loads, each issued together and waited for once.  The forms of a call
// must not put a branch between the loads of a batch -- the compiler moves no load across one, and each block then
// waits for its own: the 32- or 64-bit ray indices are the one branch, around the index loads alone and after the
// loads that do not depend on it; an unused slot's values are dropped by a select; shared time is entry 0 of the array.
//
// First batch, addressed by the slot alone: t0, t1 and the ray index of every j.  Every slot below n_eff is valid
// memory, so an unused slot (negative ray index) loads its t0 / t1 too; what they hold is discarded (a select, not a
// product: the memory may hold NaN) and the slot is evaluated on ray 0 at t = 0.  Returns whether the lane has a used slot.
template <int NT>
__device__ __forceinline__ bool load_tile_slots(const FieldArgs &A, int64_t first, const int (&sofs)[NT], int64_t (&ridx)[NT],
                                                float (&tm2)[NT])
{
    int64_t r_in[NT];
    float t0[NT], t1[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        t0[j] = A.t0[first + sofs[j]];
        t1[j] = A.t1[first + sofs[j]];
    }
    if (A.ray_idx32) {
#pragma unroll
        for (int j = 0; j < NT; ++j) r_in[j] = (int64_t)A.ray_idx32[first + sofs[j]];
    } else {
#pragma unroll
        for (int j = 0; j < NT; ++j) r_in[j] = A.ray_idx[first + sofs[j]];
    }
    bool any_used = false;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const bool used = r_in[j] >= 0;
        any_used = any_used || used;
        ridx[j] = used ? r_in[j] : 0;
        const float sum = t0[j] + t1[j];
        tm2[j] = used ? sum : 0.0f;
    }
    return any_used;
}

// Second batch, addressed by the ray: origin, direction and timestamp of every j, then the sample positions.
template <int NT>
__device__ __forceinline__ void load_tile_rays(const FieldArgs &A, const int64_t (&ridx)[NT], const float (&tm2)[NT],
                                               float (&px)[NT][3], float (&tq)[NT])
{
    float o[NT][3], d[NT][3];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            o[j][a] = A.rays_o[3 * ridx[j] + a];
            d[j][a] = A.rays_d[3 * ridx[j] + a];
        }
        tq[j] = A.timestamps[A.t_per_ray ? ridx[j] : 0];
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
#pragma unroll
        for (int a = 0; a < 3; ++a) px[j][a] = o[j][a] + (d[j][a] * tm2[j]) / 2.0f;
    }
    // the timestamps are this batch's: without a use here the compiler merges their loads with the explicit mode's
    // loads of t into one after the two modes join, a round trip of its own
#pragma unroll
    for (int j = 0; j < NT; ++j) asm volatile("" : "+v"(tq[j]));
}

template <bool TE, bool F16, bool TEMPORAL, bool SPLIT, int NT, int THREADS>
__global__ __launch_bounds__(THREADS) void field_half_kernel(FieldArgs A)
{
    constexpr int WAVES = THREADS / kWave;
    constexpr bool K32 = half_kernel_k32(TE, TEMPORAL, SPLIT, THREADS);
    static_assert(!K32 || (WAVES & (WAVES - 1)) == 0, "field_tile_seq needs a power-of-two wave count");
    constexpr int TILE = 16 * NT;
    using BL = HalfBlob<TE>;
    constexpr int PLANE = BL::FRAGS * kFragHalves;
    constexpr int WHALVES = PLANE * (SPLIT ? 2 : 1);
    __shared__ __attribute__((aligned(16))) _Float16 lds[WHALVES + 16 * CED_MAX_LEVELS];
    __shared__ int next_elem;                 // K32: the workgroup's next unclaimed element of its tile sequence
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    // the wave's number as a SCALAR: everything derived from it (the wave's tiles, their sample ranges, the bases of the
    // per-sample arrays) then lives in scalar registers and the per-lane part of an index is a 32-bit offset
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, c = lane & 15;

    int64_t n_eff = A.n;
    if (A.n_dev) {
        const int64_t nd = *A.n_dev;
        n_eff = nd < n_eff ? nd : n_eff;
    }
    // the call's window of persistent per-sample arrays (render_image, image.hip): ray_idx / t0 / t1 / sigma / rgb
    // entry s of the call is entry sbase + s of the arrays.  (Kept as an index offset: adding it to the pointers of
    // the by-value argument block would make the compiler keep the whole block in scratch.)
    const int64_t sbase = A.base_dev ? *A.base_dev : 0;
    const int64_t n_tiles = (n_eff + TILE - 1) / TILE;
    // a workgroup without a tile leaves before staging anything (field_device.hpp: field_tile_range); workgroup-uniform,
    // before any MFMA.  K32: the waves' first tiles are the static ones, every further tile is claimed from next_elem --
    // the waves then run out of tiles within one tile of each other and the barrier before the exit costs little.
    TileRange tiles;
    TileSeq seq;
    if constexpr (K32) {
        if (!field_tile_seq(A.spread_tiles, n_tiles, WAVES, seq)) return;
        tiles.first = field_tile_at(seq, wave);
        tiles.end = seq.end;
        tiles.stride = 0;
        if (tid == 0) next_elem = WAVES;
    } else {
        if (!field_tile_range(A.spread_tiles, n_tiles, WAVES, wave, tiles)) return;
    }
    if (A.stamp && tid == 0) atomicMin(A.stamp, (unsigned long long)wall_clock64());

    {
        const f4 *src = reinterpret_cast<const f4 *>(A.weights);
        f4 *dst = reinterpret_cast<f4 *>(lds);
        for (int i = tid; i < WHALVES / 8; i += THREADS) dst[i] = src[i];
        if (tid < CED_MAX_LEVELS) {
            uint32_t *lt = reinterpret_cast<uint32_t *>(lds + WHALVES);
            // the five reads spelled out: A is this kernel's by-value argument block (hash_device.hpp: make_level)
            const HashLevels &lv = A.levels;
            const LevelConst L = make_level(lv.scale[tid], lv.res[tid], lv.offset[tid], lv.size[tid], lv.hashed[tid],
                                            EntryBytes<F16, TEMPORAL>::value);
            store_level(lt + tid * 8, L);
        }
    }
    __syncthreads();

    const float extent[3] = { A.aabb[3] - A.aabb[0], A.aabb[4] - A.aabb[1], A.aabb[5] - A.aabb[2] };

    auto next_tile = [&](int64_t tile) -> int64_t {
        if constexpr (K32) {
            int i = 0;
            if (lane == 0) i = atomicAdd(&next_elem, 1);
            return field_tile_at(seq, __builtin_amdgcn_readfirstlane(i));
        } else {
            return tile + tiles.stride;
        }
    };
    for (int64_t tile = tiles.first; tile < tiles.end; tile = next_tile(tile)) {
        // opaque LDS base per tile: keeps the A-fragment reads inside the loop (see field_kernel.hpp)
        int lds_off = 0;
        asm volatile("" : "+v"(lds_off));
        const _Float16 *const whi = lds + lds_off;
        const _Float16 *const wlo = whi + PLANE;
        // sample s of the call = tile_base + lane offset; a ragged last tile repeats its last sample (never stored)
        const int64_t tile_base = tile * TILE;
        const int64_t left = n_eff - tile_base;
        const int in_tile = left < TILE ? (int)left : TILE;                  // 1 .. TILE, scalar
        int sofs[NT];
        int64_t ridx[NT];
        float px[NT][3], tq[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) sofs[j] = 16 * j + c < in_tile ? 16 * j + c : in_tile - 1;
        if (A.rays_mode) {
            // negative ray index = unused sample slot (see field_kernel.hpp); two batches of loads (load_tile_slots)
            float tm2[NT];
            const bool any_used = load_tile_slots(A, sbase + tile_base, sofs, ridx, tm2);
            if (__ballot(any_used) == 0ull) continue;        // a tile of unused slots only (wave-uniform)
            load_tile_rays(A, ridx, tm2, px, tq);
        } else {
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int64_t s = tile_base + sofs[j];
                ridx[j] = s;
#pragma unroll
                for (int a = 0; a < 3; ++a) px[j][a] = A.pos[3 * s + a];
                tq[j] = A.t[s];
            }
        }

        h8 Bh[NT][2], Bl[NT][2];
        f4 D[NT][4];

        // --- tcnn Frequency(4) on (x,y,z,t): lane group g owns dimension g; e = 2*freq + phase ---
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            float v = tq[j];
            v = (g == 0) ? px[j][0] : v;
            v = (g == 1) ? px[j][1] : v;
            v = (g == 2) ? px[j][2] : v;
            float f[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = det_sinpi_phase(v * (float)(1 << (e >> 1)), e & 1);
            to_half8<SPLIT>(f, Bh[j][0], Bl[j][0]);
        }
        // --- motion MLP 32-64-64-64-(3|6) ---
        mlp_layer_h<1, 4, NT, SPLIT>(whi + BL::M0 * kFragHalves, wlo + BL::M0 * kFragHalves, lane, Bh, Bl, D);
        to_operand_h<NT, SPLIT>(D, Bh, Bl);
        mlp_layer_h<2, 4, NT, SPLIT, K32>(whi + BL::M1 * kFragHalves, wlo + BL::M1 * kFragHalves, lane, Bh, Bl, D);
        to_operand_h<NT, SPLIT>(D, Bh, Bl);
        mlp_layer_h<2, 4, NT, SPLIT, K32>(whi + BL::M2 * kFragHalves, wlo + BL::M2 * kFragHalves, lane, Bh, Bl, D);
        to_operand_h<NT, SPLIT>(D, Bh, Bl);
        mlp_layer_h<2, 1, NT, SPLIT, K32>(whi + BL::M3 * kFragHalves, wlo + BL::M3 * kFragHalves, lane, Bh, Bl, D);

        // --- query_move / normalise / selector (model.py:354-383); motion rows are natural ---
        float xn[NT][3], mnorm[NT];
        bool sel[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            float mv[3];
            bool inside = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float off = __shfl(D[j][0][a], c, 64);          // row a: lane group 0, reg a
                float m = off * A.moving_step;
                if (A.use_div) {
                    constexpr int kFineReg[3] = { 3, 0, 1 };          // rows 3,4,5: (g0,r3), (g1,r0), (g1,r1)
                    const float fine = __shfl(D[j][0][kFineReg[a]], (a == 0) ? c : 16 + c, 64);
                    const float e = det_expf(2.0f * fine);
                    const float th = 1.0f - 2.0f / (e + 1.0f);
                    m = m + th * A.moving_step;
                }
                mv[a] = m;
                const float xm = px[j][a] + m;
                const float x = (xm - A.aabb[a]) / extent[a];      // IEEE division: 1 ulp here is amplified by the fine hash levels
                inside = inside && (x > 0.0f && x < 1.0f);
                xn[j][a] = __builtin_fminf(__builtin_fmaxf(x, 0.0f), 1.0f);
            }
            sel[j] = inside;
            mnorm[j] = TE ? __builtin_sqrtf((mv[0] * mv[0] + mv[1] * mv[1]) + mv[2] * mv[2]) : 0.0f;
        }

        // --- hash gather: slot i of lane group g is level 4i + g (slot i spans levels 4i..4i+3 across the
        // wave: one index form when they are all dense or all hashed); features land at operand elements
        // 2i, 2i+1.  Level constants are fetched from LDS per use. ---
        float R[NT][8];
        int k_lo[NT];
        float t_frac[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            k_lo[j] = 0;
            t_frac[j] = 0.0f;
            if constexpr (TEMPORAL) temporal_keyframe(tq[j], k_lo[j], t_frac[j]);
        }
        const uint32_t *const ltab = reinterpret_cast<const uint32_t *>(whi + WHALVES);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const LevelConst L = load_level(ltab + (4 * i + g) * 8);
            const int mode = (A.level_mode >> (2 * i)) & 3;
            if (mode == 1) {
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    hash_level<F16, TEMPORAL, 1>(L, A.table, xn[j], k_lo[j], t_frac[j], R[j][2 * i], R[j][2 * i + 1]);
            } else if (mode == 2) {
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    hash_level<F16, TEMPORAL, 2>(L, A.table, xn[j], k_lo[j], t_frac[j], R[j][2 * i], R[j][2 * i + 1]);
            } else if (mode == 3) {
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    hash_level<F16, TEMPORAL, 3>(L, A.table, xn[j], k_lo[j], t_frac[j], R[j][2 * i], R[j][2 * i + 1]);
            } else {
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    hash_level<F16, TEMPORAL, 0>(L, A.table, xn[j], k_lo[j], t_frac[j], R[j][2 * i], R[j][2 * i + 1]);
            }
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
#pragma unroll
            for (int e = 0; e < 8; ++e) R[j][e] = __builtin_amdgcn_fmed3f(R[j][e], -kHalfMax, kHalfMax);
            to_half8<SPLIT>(R[j], Bh[j][0], Bl[j][0]);
            if constexpr (TE) {
                // second k-step: time feature 4e + g at element e < 3 (feature 8 on lane group 0 only)
                float tf[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) tf[e] = (e < 3) ? time_feature(4 * e + g, A.time_mode, tq[j], mnorm[j]) : 0.0f;
                to_half8<SPLIT>(tf, Bh[j][1], Bl[j][1]);
            }
        }

        // --- mlp_base (32|41)-64-16 ---
        mlp_layer_h<BL::KS_B0, 4, NT, SPLIT>(whi + BL::B0 * kFragHalves, wlo + BL::B0 * kFragHalves, lane, Bh, Bl, D);
        to_operand_h<NT, SPLIT>(D, Bh, Bl);
        mlp_layer_h<2, 1, NT, SPLIT, K32>(whi + BL::B1 * kFragHalves, wlo + BL::B1 * kFragHalves, lane, Bh, Bl, D);

        // accumulator row 4g + r: geometry feature 4g + r; row 15 (g = 3, r = 3): raw density
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const bool stored = 16 * j + c < in_tile;
            const int64_t s = tile_base + (16 * j + c);
            float sg = det_expf(D[j][0][3] - 1.0f);            // trunc_exp(raw - 1) * selector
            sg = sel[j] ? sg : 0.0f;
            if (g == 3 && stored) A.sigma[sbase + s] = sg;
            if (A.geo && stored) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (4 * g + r < 15) A.geo[s * 15 + 4 * g + r] = D[j][0][r];
            }
        }

        if (A.want_rgb) {
            // --- head input [SH(4), geo(15)] (model.py:447-459): element 0 = SH_g, 1..4 = this lane's geo ---
            // lane group g feeds SH coefficient g (field_device.hpp: sh_head_input): one load where the caller computed it per
            // ray (frame renderers), else from the direction (wave-uniform choice)
            const bool sh_per_ray = A.rays_mode && A.sh_ray;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                float hin[8];
                if (sh_per_ray) {
                    hin[0] = sh_ray_load(A.sh_ray, ridx[j], g);
                } else {
                    float dv[3];
#pragma unroll
                    for (int a = 0; a < 3; ++a)
                        dv[a] = A.rays_mode ? A.rays_d[3 * ridx[j] + a] : A.dir[3 * (tile_base + sofs[j]) + a];
                    hin[0] = sh_head_input(dv, g);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) hin[1 + r] = __builtin_amdgcn_fmed3f(D[j][0][r], -kHalfMax, kHalfMax);
                hin[4] = (g == 3) ? 0.0f : hin[4];
                hin[5] = hin[6] = hin[7] = 0.0f;
                to_half8<SPLIT>(hin, Bh[j][0], Bl[j][0]);
            }
            mlp_layer_h<1, 4, NT, SPLIT>(whi + BL::H0 * kFragHalves, wlo + BL::H0 * kFragHalves, lane, Bh, Bl, D);
            to_operand_h<NT, SPLIT>(D, Bh, Bl);
            mlp_layer_h<2, 4, NT, SPLIT, K32>(whi + BL::H1 * kFragHalves, wlo + BL::H1 * kFragHalves, lane, Bh, Bl, D);
            to_operand_h<NT, SPLIT>(D, Bh, Bl);
            mlp_layer_h<2, 1, NT, SPLIT, K32>(whi + BL::H2 * kFragHalves, wlo + BL::H2 * kFragHalves, lane, Bh, Bl, D);
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int64_t s = tile_base + (16 * j + c);
                // the packer put colour channel a on accumulator row 4a = (lane group a, register 0): one sigmoid per lane
                const float o1 = 1.0f / (1.0f + det_expf(-D[j][0][0]));
                if (g < 3 && 16 * j + c < in_tile) A.rgb[3 * (sbase + s) + g] = o1;
            }
        }
    }
    // K32: no wave frees its registers while a sibling can still issue a 16x16x32 MFMA (field_half_device.hpp: mfma_k32).
    // Other kernels: no barrier -- under the static mapping waves finish up to a tile apart, and holding the early ones'
    // registers cost 3 % of throughput.
    if constexpr (K32) {
        __syncthreads();
        // the allocation's floor: 128 registers per wave, all of them (the residency argument at mfma_k32 needs it exact;
        // here, after the last MFMA, the clobber costs the allocator nothing)
        asm volatile("" ::: "v127");
    }
    // tracing only: every wave stamps its own end
    if (A.stamp && lane == 0) atomicMax(A.stamp + 1, (unsigned long long)wall_clock64());
}

// Host: one layer into 16x16x32 A-fragment order.  Element (accumulator row p, operand position k) goes to
// fragment [frag + (p/16)*ks + k/32], lane 16*((k%32)/8) + p%16, half k%8; row_map says which neuron row p
// computes, col_map which input of the layer sits at position k (header comment of this file).
void pack_half_layer(const float *w, int n_out, int n_in, int nb, int ks, int frag, int row_map, int col_map,
                     _Float16 *hi, _Float16 *lo)
{
    for (int p = 0; p < nb * 16; ++p) {
        int neuron = p;
        if (row_map == HALF_ROW_HIDDEN) neuron = half_hidden_neuron(p);
        else if (row_map == HALF_ROW_HIDDEN_K32) neuron = half_hidden_neuron_k32(p);
        else if (row_map == HALF_ROW_BASE_OUT) neuron = half_base_out_neuron(p);
        else if (row_map == HALF_ROW_RGB) neuron = (p % 4 == 0) ? p / 4 : n_out;
        if (neuron >= n_out) continue;
        for (int k = 0; k < ks * 32; ++k) {
            const int g = (k % 32) / 8, e = k % 8;
            int in = k;
            if (col_map == HALF_COL_HASH) {
                if (k < 32) in = 2 * (4 * (e >> 1) + g) + (e & 1);          // level 4i + g, feature f at e = 2i + f
                else in = (e < 3 && 4 * e + g <= 8) ? 32 + 4 * e + g : -1;   // time feature 4e + g
            } else if (col_map == HALF_COL_K32) {
                in = half_hidden_neuron_k32(16 * (2 * (k / 32) + (e >> 2)) + 4 * g + (e & 3));
            } else if (col_map == HALF_COL_HEAD) {
                if (e == 0) in = g;                                          // SH component g
                else if (e <= 4 && 4 * g + e - 1 < 15) in = 4 + 4 * g + e - 1;   // geometry feature 4g + e - 1
                else in = -1;
            }
            if (in < 0 || in >= n_in) continue;
            const float v = w[(int64_t)neuron * n_in + in];
            const _Float16 h = (_Float16)v;
            const int64_t idx = ((int64_t)(frag + (p / 16) * ks + k / 32) * 64 + 16 * g + (p % 16)) * 8 + e;
            hi[idx] = h;
            if (lo) lo[idx] = (_Float16)(v - (float)h);
        }
    }
}

int launch_field_half(FieldArgs &A, int time_mode, int precision, void *stream)
{
    // Launch geometry (which kernels fit which register cap without scratch: tools/kernel_schedule.py; the choice follows
    // the round-4 measurements, profiles/r04_ab_half_geometry.txt): temporal tables 2 x 512 threads (228-248 registers,
    // scratch above 512 threads); f16x2 2 x 768 with a time encoding, else 2 x 1024; f16 2 x 768.
    const int sel = (time_mode ? 1 : 0) | (A.table_dtype ? 2 : 0) | (A.temporal ? 4 : 0);
    if (precision == CED_MLP_F16X2) {
        switch (sel) {
        case 0: launch_field_grid<2, 1024>(field_half_kernel<false, false, false, true, 2, 1024>, A, stream); break;
        case 1: launch_field_grid<2, 768>(field_half_kernel<true, false, false, true, 2, 768>, A, stream); break;
        case 2: launch_field_grid<2, 1024>(field_half_kernel<false, true, false, true, 2, 1024>, A, stream); break;
        case 3: launch_field_grid<2, 768>(field_half_kernel<true, true, false, true, 2, 768>, A, stream); break;
        case 4: launch_field_grid<2, 512>(field_half_kernel<false, false, true, true, 2, 512>, A, stream); break;
        case 5: launch_field_grid<2, 512>(field_half_kernel<true, false, true, true, 2, 512>, A, stream); break;
        case 6: launch_field_grid<2, 512>(field_half_kernel<false, true, true, true, 2, 512>, A, stream); break;
        default: launch_field_grid<2, 512>(field_half_kernel<true, true, true, true, 2, 512>, A, stream); break;
        }
    } else {
        switch (sel) {
        case 0: launch_field_grid<2, 768>(field_half_kernel<false, false, false, false, 2, 768>, A, stream); break;
        case 1: launch_field_grid<2, 768>(field_half_kernel<true, false, false, false, 2, 768>, A, stream); break;
        case 2: launch_field_grid<2, 768>(field_half_kernel<false, true, false, false, 2, 768>, A, stream); break;
        case 3: launch_field_grid<2, 768>(field_half_kernel<true, true, false, false, 2, 768>, A, stream); break;
        case 4: launch_field_grid<2, 512>(field_half_kernel<false, false, true, false, 2, 512>, A, stream); break;
        case 5: launch_field_grid<2, 512>(field_half_kernel<true, false, true, false, 2, 512>, A, stream); break;
        case 6: launch_field_grid<2, 512>(field_half_kernel<false, true, true, false, 2, 512>, A, stream); break;
        default: launch_field_grid<2, 512>(field_half_kernel<true, true, true, false, 2, 512>, A, stream); break;
        }
    }
    return check_launch("field_forward (half-precision MLP)");
}

}  // namespace ced

extern "C" int64_t ced_packed_weight_words(int use_div_offsets, int time_mode, int mlp_precision)
{
    if (mlp_precision == CED_MLP_F32 || mlp_precision == CED_MLP_F32_HEAD16X2) return ced_packed_weight_floats(use_div_offsets, time_mode);
    if (mlp_precision != CED_MLP_F16X2 && mlp_precision != CED_MLP_F16) return -1;
    const int64_t frags = time_mode ? ced::HalfBlob<true>::FRAGS : ced::HalfBlob<false>::FRAGS;
    return frags * (ced::kFragHalves / 2) * (mlp_precision == CED_MLP_F16X2 ? 2 : 1);
}

// Host-side reorder into 16x16x32 A-fragment order: element (accumulator row p, operand position k) of a
// layer goes to fragment [nb = p/16][ks = k/32], lane 16*((k%32)/8) + p%16, half k%8.  Which neuron row p
// computes and which input sits at position k are the layer's placements (header comment of this file).  k32: the
// placements of the K = 32 kernels (half_kernel_k32): the hidden layers feeding a 16x16x32 layer are packed with
// half_hidden_neuron_k32 and those layers read their inputs from there; the output rows other code reads (motion
// offsets, mlp_base outputs, colour) and the three input layers' columns stay as they are.  Same size either way.
static int pack_half(int use_div_offsets, int time_mode, int mlp_precision, bool k32, const float *m_w0, const float *m_w1,
                     const float *m_w2, const float *m_w3, const float *b_w0, const float *b_w1, const float *h_w0,
                     const float *h_w1, const float *h_w2, void *out)
{
    CED_REQUIRE(m_w0 && m_w1 && m_w2 && m_w3 && b_w0 && b_w1 && h_w0 && h_w1 && h_w2 && out,
                "pack_field_weights_half: null pointer");
    CED_REQUIRE(time_mode >= 0 && time_mode <= 2, "pack_field_weights_half: time_mode=%d", time_mode);
    CED_REQUIRE(mlp_precision == CED_MLP_F16X2 || mlp_precision == CED_MLP_F16,
                "pack_field_weights_half: mlp_precision=%d (1 = f16x2, 2 = f16)", mlp_precision);
    const bool te = time_mode != 0, split = mlp_precision == CED_MLP_F16X2;
    const int64_t words = ced_packed_weight_words(use_div_offsets, time_mode, mlp_precision);
    memset(out, 0, (size_t)words * 4);
    _Float16 *hi = reinterpret_cast<_Float16 *>(out);
    _Float16 *lo = hi + (te ? ced::HalfBlob<true>::FRAGS : ced::HalfBlob<false>::FRAGS) * ced::kFragHalves;
    using namespace ced;
    struct L { const float *w; int n_out, n_in, nb, ks, frag, row, col; };
    const int base_in = te ? 41 : 32, n_mo = use_div_offsets ? 6 : 3, ksb0 = te ? 2 : 1;
    int fr[9];
    if (te) {
        using B = HalfBlob<true>;
        const int o[9] = { B::M0, B::M1, B::M2, B::M3, B::B0, B::B1, B::H0, B::H1, B::H2 };
        for (int i = 0; i < 9; ++i) fr[i] = o[i];
    } else {
        using B = HalfBlob<false>;
        const int o[9] = { B::M0, B::M1, B::M2, B::M3, B::B0, B::B1, B::H0, B::H1, B::H2 };
        for (int i = 0; i < 9; ++i) fr[i] = o[i];
    }
    const int HR = k32 ? HALF_ROW_HIDDEN_K32 : HALF_ROW_HIDDEN, HC = k32 ? HALF_COL_K32 : HALF_COL_NATURAL;
    const L layers[9] = {
        { m_w0, 64, 32, 4, 1, fr[0], HR, HALF_COL_NATURAL },         { m_w1, 64, 64, 4, 2, fr[1], HR, HC },
        { m_w2, 64, 64, 4, 2, fr[2], HR, HC },                       { m_w3, n_mo, 64, 1, 2, fr[3], HALF_ROW_NATURAL, HC },
        { b_w0, 64, base_in, 4, ksb0, fr[4], HR, HALF_COL_HASH },    { b_w1, 16, 64, 1, 2, fr[5], HALF_ROW_BASE_OUT, HC },
        { h_w0, 64, 19, 4, 1, fr[6], HR, HALF_COL_HEAD },            { h_w1, 64, 64, 4, 2, fr[7], HR, HC },
        { h_w2, 3, 64, 1, 2, fr[8], HALF_ROW_RGB, HC },
    };
    for (const L &l : layers) pack_half_layer(l.w, l.n_out, l.n_in, l.nb, l.ks, l.frag, l.row, l.col, hi, split ? lo : nullptr);
    return CED_OK;
}

// The pair-form placements, whatever kernel the blob is for (the layout of rounds 1-4; the tests pin it).
extern "C" int ced_pack_field_weights_half(int use_div_offsets, int time_mode, int mlp_precision, const float *m_w0,
                                           const float *m_w1, const float *m_w2, const float *m_w3, const float *b_w0,
                                           const float *b_w1, const float *h_w0, const float *h_w1, const float *h_w2,
                                           void *out)
{
    return pack_half(use_div_offsets, time_mode, mlp_precision, false, m_w0, m_w1, m_w2, m_w3, b_w0, b_w1, h_w0, h_w1,
                     h_w2, out);
}

// The placements the kernel launched for this configuration needs (half_layout_k32): what a field descriptor with
// these time_mode / mlp_precision / hash table must carry.
extern "C" int ced_pack_field_weights_half_for(int use_div_offsets, int time_mode, int mlp_precision, int table_dtype,
                                               int temporal, const float *m_w0, const float *m_w1, const float *m_w2,
                                               const float *m_w3, const float *b_w0, const float *b_w1, const float *h_w0,
                                               const float *h_w1, const float *h_w2, void *out)
{
    CED_REQUIRE(table_dtype == 0 || table_dtype == 1, "pack_field_weights_half_for: table_dtype=%d (0 = fp32, 1 = fp16)",
                table_dtype);
    return pack_half(use_div_offsets, time_mode, mlp_precision, ced::half_layout_k32(time_mode, mlp_precision, temporal),
                     m_w0, m_w1, m_w2, m_w3, b_w0, b_w1, h_w0, h_w1, h_w2, out);
}
