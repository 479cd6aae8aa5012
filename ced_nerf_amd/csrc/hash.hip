// The hash grid on its own: ced_hash_encode (the multi-resolution gather the fused field kernels contain, one lane per
// point) and its backward, ced_hash_encode_backward / ced_hash_encode_backward_temporal (table gradient by hardware
// atomics, position gradient without), with validate_hash, the check of a ced_hash_desc that every entry reading the
// table makes.  The level table travels as HashLevels (field_args.hpp); the gather is hash_level (field_device.hpp), the
// backward kernels' cell walk is in hash_device.hpp.
#include "ced_common.hpp"
#include "field_args.hpp"
#include "hash_device.hpp"

namespace ced {

// ---- standalone hash-grid encode (one lane per point, all levels) ------------------------------
struct HashArgs {
    int64_t n;
    const float *x, *t;
    float *out;
    int n_levels, table_dtype, temporal;
    const void *table;
    HashLevels levels;
};

template <bool F16, bool TEMPORAL>
__global__ __launch_bounds__(256) void hash_encode_kernel(HashArgs A)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    float x[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) x[a] = __builtin_fminf(__builtin_fmaxf(A.x[3 * i + a], 0.0f), 1.0f);
    int k_lo = 0;
    float t_frac = 0.0f;
    if constexpr (TEMPORAL) temporal_keyframe(A.t ? A.t[i] : 0.0f, k_lo, t_frac);
    float *o = A.out + i * 2 * A.n_levels;
    // a lane owns one 8 * n_levels-byte output row: two levels' features leave as one 16-byte store when the row is
    // aligned (8-byte stores of 64 lanes in 64 rows wrote five times the bytes: 32-byte sectors written a quarter full)
    const bool vec = (A.n_levels & 1) == 0 && (reinterpret_cast<uintptr_t>(A.out) & 15) == 0;
    float p0 = 0.0f, p1 = 0.0f;
#pragma unroll
    for (int l = 0; l < CED_MAX_LEVELS; ++l) {
        if (l < A.n_levels) {
            const LevelConst L = make_level(A.levels, l, EntryBytes<F16, TEMPORAL>::value);
            float f0, f1;
            if (A.levels.hashed[l]) hash_level<F16, TEMPORAL, 2>(L, A.table, x, k_lo, t_frac, f0, f1);      // level-uniform
            else hash_level<F16, TEMPORAL, 1>(L, A.table, x, k_lo, t_frac, f0, f1);
            if (!vec) {
                o[2 * l] = f0;
                o[2 * l + 1] = f1;
            } else if ((l & 1) == 0) {
                p0 = f0; p1 = f1;
            } else {
                typedef float of4 __attribute__((ext_vector_type(4)));
                *reinterpret_cast<of4 *>(o + 2 * (l - 1)) = of4{ p0, p1, f0, f1 };
            }
        }
    }
}

// ---- backward of the hash encode: next row f2, training path ---------------------------
// One lane per (sample, level) as in hash_encoder_half.py:164-226.  Table gradient: one hardware fp32 atomic add
// per corner and feature (the reference's `hash_grad[index] += w * dL/dy`).  As in the reference the position
// gradient is w.r.t. the scaled position (no `scale` factor), and levels whose dL/dy is all zero are skipped.
struct HashBwdArgs {
    int64_t n;
    const float *x, *dy;
    const float *t;              // temporal tables: the sample times (hash_table_grad_kernel<true>)
    float *grad_table, *dx;
    int n_levels, table_dtype, dx_scaled;
    const void *table;
    HashLevels levels;
};

// Table gradient: FOUR adjacent lanes share one sample and one level (blockIdx.y) and add into 16 contiguous bytes, one
// request to the memory side.  The atomics are what bounds this kernel (requests, not bytes).
//   plain table (entry = 2 features): the lanes are (x corner, feature) of one of the four (y, z) corners; the two x
//     corners are adjacent entries whenever the cell's x index is even (dense levels: always adjacent; hashed levels:
//     (x ^ h) and ((x + 1) ^ h) differ in bit 0 only).  Slot = the entry.
//   TEMPORAL table (entry = 4 key-frames x 2 features, hash_encoder_inter.py:202-275): a sample at time t interpolates
//     the key-frames k and k + 1 (k = min(floor(3 t), 2), weight t_frac = 3 t - floor(3 t): the reference's own
//     arithmetic, t = 1 included), so each of the eight corners' entries gets [2k + f] += w dy_f (1 - t_frac) and
//     [2k + 2 + f] += w dy_f t_frac.  The lanes are (key-frame, feature); slot = the float index entry * 8 + 2 (k + up)
//     + feat, so a run needs the same entry AND the same key-frame pair.
// Runs of consecutive samples (lanes 4 apart) with the same slot are summed across the wave first (segmented scan) and
// the run's last lane issues the one atomic.
template <bool TEMPORAL>
__global__ __launch_bounds__(256) void hash_table_grad_kernel(HashBwdArgs A)
{
  constexpr int NC = TEMPORAL ? 8 : 4;          // corners per lane
  // grid-stride over the samples: the launch may be capped to a few workgroups per CU (ced_set_option
  // "hash_grad_blocks"), so that a caller can run it beside compute-bound kernels of another stream -- the atomics
  // are fire-and-forget and a handful of waves per CU keep the memory side's atomic units busy
  for (int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gid - threadIdx.x < 4 * A.n;
       gid += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = gid >> 2;
    const int feat = (int)(gid & 1), up = (int)((gid >> 1) & 1);      // up: the x corner, TEMPORAL: the key-frame
    const int l = (int)blockIdx.y;
    const int lane = threadIdx.x & 63;
    uint32_t pend_slot[NC];
    float pend_val[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) { pend_slot[c] = 0xffffffffu; pend_val[c] = 0.0f; }
    if (i < A.n) {
        const float g0 = A.dy[(i * A.n_levels + l) * 2], g1 = A.dy[(i * A.n_levels + l) * 2 + 1];
        if (g0 != 0.0f || g1 != 0.0f) {
            int k_lo = 0;
            float tw = 1.0f;
            if constexpr (TEMPORAL) {
                float t_frac;
                temporal_keyframe(A.t[i], k_lo, t_frac);
                tw = up ? t_frac : 1.0f - t_frac;
            }
            uint32_t g[3];
            float fr[3], om[3];
            hash_cell(A.x + 3 * i, A.levels.scale[l], g, fr, om);
            const uint32_t res = A.levels.res[l], size = A.levels.size[l], off = A.levels.offset[l];
            const bool hashed = A.levels.hashed[l] != 0;
            const float gv = feat ? g1 : g0;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int cx = TEMPORAL ? (c & 1) : up, cy = TEMPORAL ? ((c >> 1) & 1) : (c & 1), cz = TEMPORAL ? (c >> 2) : (c >> 1);
                const float w = ((cx ? fr[0] : om[0]) * (cy ? fr[1] : om[1])) * (cz ? fr[2] : om[2]);   // the forward's weight
                const uint32_t entry = hash_corner_entry(g[0] + cx, g[1] + cy, g[2] + cz, res, off, size, hashed);
                if constexpr (TEMPORAL) {
                    pend_slot[c] = entry * 8u + 2u * (uint32_t)(k_lo + up) + (uint32_t)feat;
                    pend_val[c] = (w * gv) * tw;                         // (w * dy) * (1 - t_frac | t_frac), :264-267
                } else {
                    pend_slot[c] = entry;
                    pend_val[c] = w * gv;
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const uint32_t slot = pend_slot[c];
        float v = pend_val[c];
        const uint32_t prev = __shfl_up(slot, 4, 64);
        int head = (lane < 4 || prev != slot) ? 1 : 0;
#pragma unroll
        for (int d = 4; d < 64; d <<= 1) {
            const float v_up = __shfl_up(v, d, 64);
            const int h_up = __shfl_up(head, d, 64);
            if (lane >= d && !head) { v += v_up; head |= h_up; }
        }
        const uint32_t next = __shfl_down(slot, 4, 64);
        const bool last = lane >= 60 || next != slot;
        if (last && slot != 0xffffffffu && v != 0.0f)
            unsafeAtomicAdd(TEMPORAL ? A.grad_table + (size_t)slot : A.grad_table + (size_t)slot * 2 + feat, v);
    }
  }
}

// Position gradient: 16 consecutive lanes = the 16 levels of one sample, whose contributions are summed inside the
// 16-lane group in a fixed order and stored without atomics.
template <bool F16>
__global__ __launch_bounds__(256) void hash_backward_kernel(HashBwdArgs A)
{
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = gid >> 4;
    const int l = (int)(gid & 15);
    float gx[3] = { 0.0f, 0.0f, 0.0f };
    if (i < A.n && l < A.n_levels) {
        const float g0 = A.dy[(i * A.n_levels + l) * 2], g1 = A.dy[(i * A.n_levels + l) * 2 + 1];
        if (g0 != 0.0f || g1 != 0.0f) {
            const float sc = A.levels.scale[l];
            uint32_t g[3];
            float fr[3], om[3];
            hash_cell(A.x + 3 * i, sc, g, fr, om);
            const uint32_t res = A.levels.res[l], size = A.levels.size[l], off = A.levels.offset[l];
            const bool hashed = A.levels.hashed[l] != 0;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float wx = (c & 1) ? fr[0] : om[0], wy = (c & 2) ? fr[1] : om[1], wz = (c & 4) ? fr[2] : om[2];
                const float wxy = wx * wy;
                const uint32_t idx = hash_corner_entry(g[0] + (c & 1), g[1] + ((c >> 1) & 1), g[2] + ((c >> 2) & 1), res, off, size, hashed);
                float f0, f1;
                if constexpr (!F16) {
                    const float2 v = reinterpret_cast<const float2 *>(A.table)[idx];
                    f0 = v.x; f1 = v.y;
                } else {
                    const uint32_t u = reinterpret_cast<const uint32_t *>(A.table)[idx];
                    f0 = half_bits_to_float((uint16_t)(u & 0xffffu)); f1 = half_bits_to_float((uint16_t)(u >> 16));
                }
                // d w / d pos_a = +-(product of the other two factors)
                const float dot = (f0 * g0 + f1 * g1) * (A.dx_scaled ? sc : 1.0f);
                gx[0] += dot * ((c & 1) ? (wy * wz) : -(wy * wz));
                gx[1] += dot * ((c & 2) ? (wx * wz) : -(wx * wz));
                gx[2] += dot * ((c & 4) ? wxy : -wxy);
            }
        }
    }
    // sum over the 16 levels of the sample (lanes 16k..16k+15), fixed order
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) gx[a] += __shfl_down(gx[a], off, 16);
    }
    if (l == 0 && i < A.n) {
        A.dx[3 * i] = gx[0]; A.dx[3 * i + 1] = gx[1]; A.dx[3 * i + 2] = gx[2];
    }
}

std::atomic<int> g_hash_grad_blocks{ 0 };       // ced_set_option: table-gradient workgroups per level (0: one per 64 samples)

// grid of a table-gradient launch: four lanes per sample, one level per blockIdx.y, capped to hash_grad_blocks
static dim3 table_grad_grid(int64_t n, int n_levels)
{
    int64_t gx = (4 * n + 255) / 256;
    const int cap = g_hash_grad_blocks;
    if (cap > 0 && gx > cap) gx = cap;
    return dim3((unsigned)gx, (unsigned)n_levels);
}

int validate_hash(const ced_hash_desc *h, const char *who)
{
    CED_REQUIRE(h != nullptr, "%s: null hash descriptor", who);
    CED_REQUIRE(h->n_levels >= 1 && h->n_levels <= CED_MAX_LEVELS, "%s: n_levels=%d out of range", who, h->n_levels);
    CED_REQUIRE(h->table_dtype == 0 || h->table_dtype == 1, "%s: table_dtype must be 0 (f32) or 1 (f16)", who);
    CED_REQUIRE(h->table != nullptr, "%s: null hash table", who);
    for (int l = 0; l < h->n_levels; ++l) {
        CED_REQUIRE(h->size[l] > 0, "%s: level %d has zero entries", who, l);
        if (h->hashed[l])
            CED_REQUIRE((h->size[l] & (h->size[l] - 1)) == 0, "%s: hashed level %d size %u is not a power of two", who, l,
                        h->size[l]);
        else
            CED_REQUIRE((uint64_t)h->res[l] * h->res[l] * h->res[l] <= h->size[l],
                        "%s: dense level %d smaller than res^3", who, l);
        CED_REQUIRE((uint64_t)h->offset[l] + h->size[l] <= h->total_entries, "%s: level %d exceeds the table", who, l);
    }
    return CED_OK;
}

}  // namespace ced

extern "C" int ced_hash_encode(const ced_hash_desc *desc, int64_t n, const float *x, const float *t, float *out,
                               void *stream)
{
    int rc = ced::validate_hash(desc, "hash_encode");
    if (rc) return rc;
    CED_REQUIRE(n >= 0, "hash_encode: n < 0");
    if (n == 0) return CED_OK;
    CED_REQUIRE(x && out, "hash_encode: null pointer");
    ced::HashArgs A{};
    A.n = n; A.x = x; A.t = t; A.out = out;
    A.n_levels = desc->n_levels; A.table_dtype = desc->table_dtype; A.temporal = desc->temporal ? 1 : 0;
    A.table = desc->table;
    ced::fill_levels(A.levels, *desc);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    switch ((A.table_dtype ? 1 : 0) | (A.temporal ? 2 : 0)) {
    case 0: hipLaunchKernelGGL((ced::hash_encode_kernel<false, false>), grid, block, 0, (hipStream_t)stream, A); break;
    case 1: hipLaunchKernelGGL((ced::hash_encode_kernel<true, false>), grid, block, 0, (hipStream_t)stream, A); break;
    case 2: hipLaunchKernelGGL((ced::hash_encode_kernel<false, true>), grid, block, 0, (hipStream_t)stream, A); break;
    default: hipLaunchKernelGGL((ced::hash_encode_kernel<true, true>), grid, block, 0, (hipStream_t)stream, A); break;
    }
    return ced::check_launch("hash_encode");
}

extern "C" int ced_hash_encode_backward(const ced_hash_desc *desc, int64_t n, const float *x, const float *dy,
                                        float *grad_table, float *dx, int32_t dx_scaled, void *stream)
{
    int rc = ced::validate_hash(desc, "hash_encode_backward");
    if (rc) return rc;
    CED_REQUIRE(n >= 0, "hash_encode_backward: n < 0");
    CED_REQUIRE(!desc->temporal, "hash_encode_backward: the temporal table has no backward yet");
    CED_REQUIRE(desc->n_levels <= 16, "hash_encode_backward: n_levels > 16");
    if (n == 0) return CED_OK;
    CED_REQUIRE(x && dy && (grad_table || dx), "hash_encode_backward: null pointer");
    ced::HashBwdArgs A{};
    A.n = n; A.x = x; A.dy = dy; A.grad_table = grad_table; A.dx = dx;
    A.n_levels = desc->n_levels; A.table_dtype = desc->table_dtype; A.table = desc->table;
    A.dx_scaled = dx_scaled ? 1 : 0;
    ced::fill_levels(A.levels, *desc);
    // table gradient: level-major; position gradient (optional): sample-major, no atomics.  Without grad_table only the
    // position gradient runs (the caller runs the table gradient elsewhere, e.g. on another stream).
    if (grad_table)
        hipLaunchKernelGGL(ced::hash_table_grad_kernel<false>, ced::table_grad_grid(n, desc->n_levels), dim3(256), 0,
                           (hipStream_t)stream, A);
    if (dx) {
        const dim3 grid_x((unsigned)((n * 16 + 255) / 256));
        if (A.table_dtype) hipLaunchKernelGGL(ced::hash_backward_kernel<true>, grid_x, dim3(256), 0, (hipStream_t)stream, A);
        else hipLaunchKernelGGL(ced::hash_backward_kernel<false>, grid_x, dim3(256), 0, (hipStream_t)stream, A);
    }
    return ced::check_launch("hash_encode_backward");
}

extern "C" int ced_hash_encode_backward_temporal(const ced_hash_desc *desc, int64_t n, const float *x, const float *t,
                                                 const float *dy, float *grad_table, void *stream)
{
    int rc = ced::validate_hash(desc, "hash_encode_backward_temporal");
    if (rc) return rc;
    CED_REQUIRE(n >= 0, "hash_encode_backward_temporal: n < 0");
    CED_REQUIRE(desc->temporal, "hash_encode_backward_temporal: the table is not temporal (use ced_hash_encode_backward)");
    CED_REQUIRE(desc->n_levels <= 16, "hash_encode_backward_temporal: n_levels > 16");
    CED_REQUIRE(desc->total_entries * 8ull < (1ull << 32), "hash_encode_backward_temporal: table too large for 32-bit slots");
    if (n == 0) return CED_OK;
    CED_REQUIRE(x && t && dy && grad_table, "hash_encode_backward_temporal: null pointer");
    ced::HashBwdArgs A{};
    A.n = n; A.x = x; A.t = t; A.dy = dy; A.grad_table = grad_table;
    A.n_levels = desc->n_levels; A.table_dtype = desc->table_dtype; A.table = desc->table;
    ced::fill_levels(A.levels, *desc);
    hipLaunchKernelGGL(ced::hash_table_grad_kernel<true>, ced::table_grad_grid(n, desc->n_levels), dim3(256), 0,
                       (hipStream_t)stream, A);
    return ced::check_launch("hash_encode_backward_temporal");
}
