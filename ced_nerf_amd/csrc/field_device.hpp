// Device-side pieces shared by the fp32 (field_kernel.hpp) and half-precision (field_half.hip) fused field
// kernels: per-level hash-grid constants, the trilinear gather of one level, the temporal key-frame
// split and the 9-wide time encoding.  Everything here computes in fp32 with the deterministic
// transcendentals of ced_common.hpp, whatever precision the MLPs run in.
#pragma once
#include <cstdint>

#include "ced_common.hpp"

namespace ced {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

// Tile -> wave mapping of the persistent field kernels (one workgroup per CU, WAVES waves, tiles of 16 * NT samples).
// mode 0: wave w of workgroup b takes tiles b * WAVES + w, + gridDim.x * WAVES, ...
// mode 1: a round of gridDim.x * WAVES tiles is dealt in groups of four consecutive tiles (the four SIMDs of a CU) across
//         ALL workgroups before any workgroup gets a second group.  The last, partial round of a launch (a frame's
//         launches are 4-5 rounds long) then leaves every CU with about one wave per SIMD -- which runs ~2.5x faster than
//         three sharing the MFMA pipe -- instead of a third of the CUs fully loaded and the rest idle.
// mode 2 (default; needs gridDim.x % 8 == 0, else mode 1): the same dealing inside each XCD.  Workgroup b runs on XCD
//         b % 8; the eight XCDs take eight CONTIGUOUS parts of the sample stream, so a table line wanted by
//         neighbouring samples (adjacent samples of a ray, adjacent rays of a pixel tile) is fetched into ONE L2
//         instead of up to eight (round 4: +2 % f16x2, +9 % f16 on a 15 M-sample launch).
// Returns false when the workgroup has no tile at all (it leaves before staging anything).
struct TileRange { int64_t first, end, stride; };
__device__ __forceinline__ bool field_tile_range(int mode, int64_t n_tiles, int waves, int wave, TileRange &r)
{
    const int64_t grid = gridDim.x, b = blockIdx.x;
    if (mode == 2 && (grid & 7) == 0) {
        const int64_t n_groups = (n_tiles + 3) >> 2, per_xcd = grid >> 3, region = (n_groups + 7) >> 3;
        const int64_t start = (b & 7) * region;
        const int64_t g_end = start + region < n_groups ? start + region : n_groups;
        if (start + (b >> 3) >= g_end) return false;
        r.first = (start + (int64_t)(wave >> 2) * per_xcd + (b >> 3)) * 4 + (wave & 3);
        r.end = 4 * g_end < n_tiles ? 4 * g_end : n_tiles;
        r.stride = (int64_t)(waves / 4) * per_xcd * 4;
        return true;
    }
    if ((mode ? b * 4 : b * waves) >= n_tiles) return false;
    r.first = mode ? ((int64_t)(wave >> 2) * grid + b) * 4 + (wave & 3) : b * waves + wave;
    r.end = n_tiles;
    r.stride = grid * waves;
    return true;
}

// The same tiles as ONE sequence per workgroup, for kernels whose waves take their tiles from a workgroup counter
// (field_half.hip, the K = 32 kernels): element i = t * waves + w is the t-th tile field_tile_range gives wave w,
// tile (base + (i >> shift) * gstride) << shift | (i & ((1 << shift) - 1)), increasing in i; the sequence ends at the
// first element >= end.  waves must be a power of two (mode 0).
struct TileSeq { int64_t base, gstride, end; int shift; };
__device__ __forceinline__ int64_t field_tile_at(const TileSeq &q, int i)
{
    return ((q.base + (int64_t)(i >> q.shift) * q.gstride) << q.shift) + (i & ((1 << q.shift) - 1));
}
__device__ __forceinline__ bool field_tile_seq(int mode, int64_t n_tiles, int waves, TileSeq &q)
{
    const int64_t grid = gridDim.x, b = blockIdx.x;
    if (mode == 2 && (grid & 7) == 0) {
        const int64_t n_groups = (n_tiles + 3) >> 2, per_xcd = grid >> 3, region = (n_groups + 7) >> 3;
        const int64_t start = (b & 7) * region;
        const int64_t g_end = start + region < n_groups ? start + region : n_groups;
        if (start + (b >> 3) >= g_end) return false;
        q.base = start + (b >> 3);
        q.gstride = per_xcd;
        q.end = 4 * g_end < n_tiles ? 4 * g_end : n_tiles;
        q.shift = 2;
        return true;
    }
    if ((mode ? b * 4 : b * waves) >= n_tiles) return false;
    q.base = b;
    q.gstride = grid;
    q.end = n_tiles;
    q.shift = mode ? 2 : __builtin_ctz((unsigned)waves);
    return true;
}

// Per-level constants, pre-multiplied by the table's bytes per entry (a power of two), so the
// corner arithmetic below produces byte offsets directly: the xor-hash commutes with the shift
// ((a^b) << s == (a<<s) ^ (b<<s)) and the dense index is linear.
struct LevelConst {
    float scale;
    uint32_t sxb, syb, szb;   // per-axis multipliers in bytes: (1, p1, p2) * EB when hashed, (1, res, res^2) * EB when dense
    uint32_t offb;            // first byte of the level
    uint32_t sizeb;           // level size in bytes (dense wrap-around)
    uint32_t maskb;           // (size - 1) * EB (hashed levels: size is a power of two)
    uint32_t hashed;
};

template <bool F16, bool TEMPORAL> struct EntryBytes { static constexpr uint32_t value = (F16 ? 4u : 8u) * (TEMPORAL ? 4u : 1u); };

// the spatial hash of a hashed level: x ^ y * kHashPrimeY ^ z * kHashPrimeZ (hash_encoder_half.py:112-161)
constexpr uint32_t kHashPrimeY = 2654435761u, kHashPrimeZ = 805459861u;

__device__ __forceinline__ LevelConst make_level(float scale, uint32_t res, uint32_t offset, uint32_t size, uint32_t hashed,
                                                 uint32_t eb)
{
    LevelConst L;
    L.scale = scale;
    L.sxb = eb;
    L.syb = (hashed ? kHashPrimeY : res) * eb;
    L.szb = (hashed ? kHashPrimeZ : res * res) * eb;
    L.offb = offset * eb;
    L.sizeb = size * eb;
    L.maskb = (size - 1u) * eb;
    L.hashed = hashed;
    return L;
}

// The kernels keep the 16 levels' constants in LDS as 8 words each and fetch them where they are used
// (two ds_read_b128 per level per wave tile) instead of holding 32 registers across the whole tile.
__device__ __forceinline__ void store_level(uint32_t *lt, const LevelConst &L)
{
    lt[0] = __float_as_uint(L.scale);
    lt[1] = L.sxb;
    lt[2] = L.syb;
    lt[3] = L.szb;
    lt[4] = L.offb;
    lt[5] = L.sizeb;
    lt[6] = L.maskb;
    lt[7] = L.hashed;
}
__device__ __forceinline__ LevelConst load_level(const uint32_t *lt)
{
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const u4 a = *reinterpret_cast<const u4 *>(lt), b = *reinterpret_cast<const u4 *>(lt + 4);
    LevelConst L;
    L.scale = __uint_as_float(a[0]);
    L.sxb = a[1];
    L.syb = a[2];
    L.szb = a[3];
    L.offb = b[0];
    L.sizeb = b[1];
    L.maskb = b[2];
    L.hashed = b[3];
    return L;
}

// The eight corner values of hash_level at byte offsets off[c] (c = cx + 2 cy + 4 cz), both features of a corner as one
// register pair; a temporal table's key-frames k_lo and k_lo + 1 are interpolated here.  PAIRS (non-temporal): the two x
// corners of a (y, z) corner come from ONE 16-byte (fp16 table: 8-byte) load at off[2q]; ADJACENT says the caller knows
// off[2q + 1] == off[2q] + entry size on every lane, otherwise a lane where that fails re-reads its second corner.
template <bool F16, bool TEMPORAL, bool PAIRS, bool ADJACENT>
__device__ __forceinline__ void load_corners(const char *__restrict__ tb, const uint32_t (&off)[8], int k_lo, float t_frac,
                                             f2 (&v)[8])
{
    if constexpr (!TEMPORAL) {
        if constexpr (PAIRS) {
            // dense level (not the table's last: field_args.hpp, hash_level_modes): the two x corners of a (y, z) corner are adjacent entries -- ONE
            // 16-byte (fp16 table: 8-byte) load instead of two on the same cache line.  The one exception is the reference's
            // `% size` acting between the two (the +x corner is the level's entry 0): that lane re-reads its second corner.
            constexpr uint32_t EBp = EntryBytes<F16, TEMPORAL>::value;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if constexpr (!F16) {
                    const f4 pr = *reinterpret_cast<const f4 *>(tb + off[2 * q]);
                    v[2 * q] = f2{ pr[0], pr[1] };
                    v[2 * q + 1] = f2{ pr[2], pr[3] };
                    if constexpr (!ADJACENT)
                        if (off[2 * q + 1] != off[2 * q] + EBp) v[2 * q + 1] = *reinterpret_cast<const f2 *>(tb + off[2 * q + 1]);
                } else {
                    typedef uint32_t u2v __attribute__((ext_vector_type(2)));
                    const u2v u = *reinterpret_cast<const u2v *>(tb + off[2 * q]);
                    uint32_t u1 = u[1];
                    if constexpr (!ADJACENT)
                        if (off[2 * q + 1] != off[2 * q] + EBp) u1 = *reinterpret_cast<const uint32_t *>(tb + off[2 * q + 1]);
                    v[2 * q] = f2{ half_bits_to_float((uint16_t)(u[0] & 0xffffu)), half_bits_to_float((uint16_t)(u[0] >> 16)) };
                    v[2 * q + 1] = f2{ half_bits_to_float((uint16_t)(u1 & 0xffffu)), half_bits_to_float((uint16_t)(u1 >> 16)) };
                }
            }
        } else if constexpr (!F16) {
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = *reinterpret_cast<const f2 *>(tb + off[c]);
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const uint32_t u = *reinterpret_cast<const uint32_t *>(tb + off[c]);
                v[c] = f2{ half_bits_to_float((uint16_t)(u & 0xffffu)), half_bits_to_float((uint16_t)(u >> 16)) };
            }
        }
    } else {
        const float omt = 1.0f - t_frac;
        const f2 omt2 = { omt, omt }, tf2 = { t_frac, t_frac };
        const uint32_t kb = (uint32_t)k_lo * (F16 ? 4u : 8u);      // byte offset of key-frame k_lo inside the entry
        if constexpr (!F16) {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                // key-frames k and k + 1 of an entry are adjacent: ONE 16-byte load (rounds 1-4: two 8-byte loads)
                const f4 pr = *reinterpret_cast<const f4 *>(tb + off[c] + kb);
                const f2 lo = { pr[0], pr[1] }, hi = { pr[2], pr[3] };
                v[c] = lo * omt2 + hi * tf2;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                typedef uint32_t u2t __attribute__((ext_vector_type(2)));
                const u2t pr = *reinterpret_cast<const u2t *>(tb + off[c] + kb);
                const uint32_t lo = pr[0], hi = pr[1];
                const f2 a = { half_bits_to_float((uint16_t)(lo & 0xffffu)), half_bits_to_float((uint16_t)(lo >> 16)) };
                const f2 b = { half_bits_to_float((uint16_t)(hi & 0xffffu)), half_bits_to_float((uint16_t)(hi >> 16)) };
                v[c] = a * omt2 + b * tf2;
            }
        }
    }
}

// Trilinear gather of one level for one point (hash_encoder_half.py:112-161; temporal variant
// hash_encoder_inter.py:148-197).  x already clamped to [0,1].  MODE: 0 = this lane's level may be
// dense or hashed (both index forms computed, selected per lane), 1 = dense, 2 = hashed, 3 = dense with the x-corner
// pairs fetched by one load each (non-temporal tables, levels followed by another level).
template <bool F16, bool TEMPORAL, int MODE>
__device__ __forceinline__ void hash_level(const LevelConst &L, const void *__restrict__ table, const float (&x)[3],
                                           int k_lo, float t_frac, float &f0, float &f1)
{
    uint32_t g[3];
    float fr[3], om[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        // p >= 0.5: the conversion truncates = floor, and p - floor(p) is exact, which is what v_fract_f32 returns
        const float p = x[a] * L.scale + 0.5f;
        g[a] = (uint32_t)p;
        fr[a] = __builtin_amdgcn_fractf(p);
        om[a] = 1.0f - fr[a];
    }
    // byte strides: x is the entry size (a power of two: a shift); dense levels have res^2 * EB < 2^24, so
    // their products are single full-rate 24-bit multiplies; hashed levels need the 32-bit wrap-around product
    constexpr uint32_t EB = EntryBytes<F16, TEMPORAL>::value;
    const uint32_t x0 = g[0] * EB;
    const uint32_t y0 = (MODE == 1 || MODE == 3) ? __umul24(g[1], L.syb) : g[1] * L.syb;
    const uint32_t z0 = (MODE == 1 || MODE == 3) ? __umul24(g[2], L.szb) : g[2] * L.szb;
    const uint32_t xs[2] = { x0, x0 + EB };
    const uint32_t ys[2] = { y0, y0 + L.syb };
    const uint32_t zs[2] = { z0, z0 + L.szb };
    const bool hashed = L.hashed != 0;
    // y/z combinations are shared by the two x corners
    uint32_t yz_x[4], yz_a[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if constexpr (MODE != 1 && MODE != 3) yz_x[q] = ys[q & 1] ^ zs[q >> 1];
        if constexpr (MODE != 2) yz_a[q] = ys[q & 1] + zs[q >> 1];
    }
    const float wxy[4] = { om[0] * om[1], fr[0] * om[1], om[0] * fr[1], fr[0] * fr[1] };   // index cx + 2*cy
    float w[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) w[c] = wxy[c & 3] * ((c >> 2) ? fr[2] : om[2]);
    const char *tb = reinterpret_cast<const char *>(table);
    uint32_t off[8];
    f2 v[8];
    if constexpr (MODE == 1 || MODE == 3) {
        // Dense level: the reference's `% size` acts only on a corner index >= size, and size >= res^3 while the corner
        // coordinates reach res -- only cells on the level's far y / z boundary get there.  All strides are positive and
        // the largest index, corner (1, 1, 1), is below 2 * size (no 32-bit carry), so when xs[1] + yz_a[3] < sizeb
        // every corner's dx is below sizeb: dx - sizeb wraps to dx + (2^32 - sizeb) > dx and the min below returns dx
        // itself.  ONE wave-uniform test per call then takes the wrap (add / subtract / min per corner) off the common
        // path; without it the x corners are xs[0] and xs[0] + EB, adjacent entries, so the pair load needs no re-read
        // test either, and the level's first byte goes into the four (y, z) sums instead of the eight corners (integer
        // sums, re-associated: the same byte offsets).
        if (__ballot(xs[1] + yz_a[3] >= L.sizeb) == 0ull) {
            uint32_t yz_o[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) yz_o[q] = yz_a[q] + L.offb;
#pragma unroll
            for (int c = 0; c < 8; ++c) off[c] = xs[c & 1] + yz_o[c >> 1];
            load_corners<F16, TEMPORAL, MODE == 3, true>(tb, off, k_lo, t_frac, v);
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                // idx % size with idx < 2 * size: the unsigned difference wraps to a huge value when idx < size
                const uint32_t dx = xs[c & 1] + yz_a[c >> 1];
                const uint32_t dw = dx - L.sizeb;
                off[c] = L.offb + (dx < dw ? dx : dw);
            }
            load_corners<F16, TEMPORAL, MODE == 3, false>(tb, off, k_lo, t_frac, v);
        }
    } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const uint32_t hb = (xs[c & 1] ^ yz_x[c >> 1]) & L.maskb;
            uint32_t idxb = hb;
            if constexpr (MODE == 0) {
                const uint32_t dx = xs[c & 1] + yz_a[c >> 1];
                const uint32_t dw = dx - L.sizeb;
                const uint32_t db = dx < dw ? dx : dw;
                idxb = hashed ? hb : db;
            }
            off[c] = L.offb + idxb;
        }
        load_corners<F16, TEMPORAL, false, false>(tb, off, k_lo, t_frac, v);
    }
    f2 acc = { 0.0f, 0.0f };
#pragma unroll
    for (int c = 0; c < 8; ++c) acc = __builtin_elementwise_fma(f2{ w[c], w[c] }, v[c], acc);
    f0 = acc[0];
    f1 = acc[1];
}

// hash_level with the derivative of both features with respect to the normalised position (field_density_gradient.hip).
// The features are hash_level's bits: the same corner weights, the same eight fused multiply-adds in the same order, on
// the same corner values (MODE 0 or 2; a dense level goes through MODE 0, which reads what MODE 1 and 3 read).  Inside
// the cell the fp32 floor above selects, the fraction's derivative is the level's scale exactly, so with v[c] the
// (time-interpolated) corner values and (wx, wy, wz)[0 / 1] = 1 - frac / frac per axis
//     d f / d x_a = (scale * dscale) * sum over the four corner pairs along axis a of  (weight of the other two axes) * (v[upper] - v[lower])
// each difference, weight product and fused multiply-add rounded once, pairs in ascending corner order.  dscale is an
// exact power of two the caller carries its tangents by.
template <bool F16, bool TEMPORAL, int MODE>
__device__ __forceinline__ void hash_level_dx(const LevelConst &L, const void *__restrict__ table, const float (&x)[3],
                                              int k_lo, float t_frac, float dscale, float &f0, float &f1, float (&d0)[3],
                                              float (&d1)[3])
{
    static_assert(MODE == 0 || MODE == 2, "hash_level_dx: mixed (0) or hashed (2) index form");
    uint32_t g[3];
    float fr[3], om[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = x[a] * L.scale + 0.5f;
        g[a] = (uint32_t)p;
        fr[a] = __builtin_amdgcn_fractf(p);
        om[a] = 1.0f - fr[a];
    }
    constexpr uint32_t EB = EntryBytes<F16, TEMPORAL>::value;
    const uint32_t x0 = g[0] * EB;
    const uint32_t y0 = g[1] * L.syb;
    const uint32_t z0 = g[2] * L.szb;
    const uint32_t xs[2] = { x0, x0 + EB };
    const uint32_t ys[2] = { y0, y0 + L.syb };
    const uint32_t zs[2] = { z0, z0 + L.szb };
    const bool hashed = L.hashed != 0;
    const float wxy[4] = { om[0] * om[1], fr[0] * om[1], om[0] * fr[1], fr[0] * fr[1] };   // index cx + 2*cy
    const char *tb = reinterpret_cast<const char *>(table);
    const float omt = 1.0f - t_frac;
    const f2 omt2 = { omt, omt }, tf2 = { t_frac, t_frac };
    const uint32_t kb = TEMPORAL ? (uint32_t)k_lo * (F16 ? 4u : 8u) : 0u;
    f2 v[8];
    float w[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int cx = c & 1, cy = (c >> 1) & 1, cz = (c >> 2) & 1;
        const uint32_t hb = (xs[cx] ^ (ys[cy] ^ zs[cz])) & L.maskb;
        uint32_t idxb = hb;
        if constexpr (MODE == 0) {
            const uint32_t dx = xs[cx] + (ys[cy] + zs[cz]);
            const uint32_t dw = dx - L.sizeb;
            const uint32_t db = dx < dw ? dx : dw;
            idxb = hashed ? hb : db;
        }
        const char *entry = tb + (L.offb + idxb) + kb;
        w[c] = wxy[cx + 2 * cy] * (cz ? fr[2] : om[2]);
        if constexpr (!TEMPORAL && !F16) {
            v[c] = *reinterpret_cast<const f2 *>(entry);
        } else if constexpr (!TEMPORAL) {
            const uint32_t u = *reinterpret_cast<const uint32_t *>(entry);
            v[c] = f2{ half_bits_to_float((uint16_t)(u & 0xffffu)), half_bits_to_float((uint16_t)(u >> 16)) };
        } else if constexpr (!F16) {
            const f4 pr = *reinterpret_cast<const f4 *>(entry);
            const f2 lo = { pr[0], pr[1] }, hi = { pr[2], pr[3] };
            v[c] = lo * omt2 + hi * tf2;
        } else {
            typedef uint32_t u2t __attribute__((ext_vector_type(2)));
            const u2t pr = *reinterpret_cast<const u2t *>(entry);
            const f2 a = { half_bits_to_float((uint16_t)(pr[0] & 0xffffu)), half_bits_to_float((uint16_t)(pr[0] >> 16)) };
            const f2 b = { half_bits_to_float((uint16_t)(pr[1] & 0xffffu)), half_bits_to_float((uint16_t)(pr[1] >> 16)) };
            v[c] = a * omt2 + b * tf2;
        }
    }
    f2 acc = { 0.0f, 0.0f };
#pragma unroll
    for (int c = 0; c < 8; ++c) acc = __builtin_elementwise_fma(f2{ w[c], w[c] }, v[c], acc);
    f0 = acc[0];
    f1 = acc[1];

    f2 gx = { 0.0f, 0.0f }, gy = { 0.0f, 0.0f }, gz = { 0.0f, 0.0f };
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int lo = q & 1, hi = q >> 1;
        const float wyz = (lo ? fr[1] : om[1]) * (hi ? fr[2] : om[2]);       // x pairs: cy = lo, cz = hi
        const float wxz = (lo ? fr[0] : om[0]) * (hi ? fr[2] : om[2]);       // y pairs: cx = lo, cz = hi
        gx = __builtin_elementwise_fma(f2{ wyz, wyz }, v[1 + 2 * lo + 4 * hi] - v[2 * lo + 4 * hi], gx);
        gy = __builtin_elementwise_fma(f2{ wxz, wxz }, v[lo + 2 + 4 * hi] - v[lo + 4 * hi], gy);
        gz = __builtin_elementwise_fma(f2{ wxy[q], wxy[q] }, v[q + 4] - v[q], gz);
    }
    const float s = L.scale * dscale;
    d0[0] = gx[0] * s; d0[1] = gy[0] * s; d0[2] = gz[0] * s;
    d1[0] = gx[1] * s; d1[1] = gy[1] * s; d1[2] = gz[1] * s;
}

// The colour head's SH(4) input of lane group g from the view direction (model.py:447-459; Y00 const, Y1-1 ~ -y,
// Y10 ~ z, Y11 ~ -x; tcnn maps the unit vector to [0,1] and back): only component g is normalised.  Group 0's constant
// aside, it depends on the ray alone: the frame renderers compute groups 1..3 once per ray (FieldArgs::sh_ray, entry
// 3 r + g - 1, written by sh_ray_store) with these very operations, and the field kernels then load instead of recompute.
__device__ __forceinline__ float sh_head_input(const float (&dv)[3], int g)
{
    const float nrm = __builtin_sqrtf((dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2]);
    const float comp = (g == 1) ? dv[1] : (g == 2) ? dv[2] : dv[0];
    const float u = (comp / nrm + 1.0f) / 2.0f;
    const float vv = u * 2.0f - 1.0f;
    const float coef = (g == 2) ? 0.48860251190291987f : -0.48860251190291987f;
    return (g == 0) ? 0.28209479177387814f : coef * vv;
}
__device__ __forceinline__ void sh_ray_store(const float *__restrict__ rays_d, int64_t r, float *__restrict__ sh_ray)
{
    const float dv[3] = { rays_d[3 * r], rays_d[3 * r + 1], rays_d[3 * r + 2] };
#pragma unroll
    for (int g = 1; g < 4; ++g) sh_ray[3 * r + g - 1] = sh_head_input(dv, g);
}
// lane group g's SH input of ray r from that array (group 0 reads entry 0 of the ray and keeps the constant)
__device__ __forceinline__ float sh_ray_load(const float *__restrict__ sh_ray, int64_t r, int g)
{
    const float v = sh_ray[3 * r + (g ? g - 1 : 0)];
    return (g == 0) ? 0.28209479177387814f : v;
}

__device__ __forceinline__ void temporal_keyframe(float tq, int &k_lo, float &t_frac)
{
    float ts = tq * 3.0f;
    float fl = __builtin_floorf(ts);
    t_frac = ts - fl;
    fl = __builtin_fminf(fl, 2.0f);
    k_lo = (int)fl;
}

// feature idx (0..8, >8 -> 0) of the 9-wide time encoding (cednerf/encoder.py:6-44 / :46-90)
__device__ __forceinline__ float time_feature(int idx, int time_mode, float t, float mn)
{
    const float HALF_PI = 1.57079637050628662f;
    if (idx == 0) return t;
    if (idx > 8) return 0.0f;
    int k, ph;
    if (time_mode == 1) { k = (idx - 1) & 3; ph = (idx - 1) >> 2; }
    else { k = (idx - 1) >> 1; ph = (idx - 1) & 1; }
    float xb = t * (float)(1 << k);
    float arg = ph ? (xb + HALF_PI) : xb;
    float s = det_sinf(arg);
    if (time_mode == 2) {
        float att = det_expf(-1.0f * (mn * (float)(k * (1 << k))));
        s = s * att;
    }
    return s;
}

}  // namespace ced
