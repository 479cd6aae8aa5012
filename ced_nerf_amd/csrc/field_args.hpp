// Kernel-argument block of the fused field kernel (field_kernel.hpp; launched by field.hip), shared with the frame
// renderer, and the per-level table of the hash grid as every kernel that reads the grid receives it.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>

#include "../../include/cednerf_hip.h"
#include "ced_common.hpp"

namespace ced {

// The per-level table of a ced_hash_desc, by value inside a kernel's argument block (hash_device.hpp: make_level).
struct HashLevels {
    float scale[CED_MAX_LEVELS];
    uint32_t res[CED_MAX_LEVELS], offset[CED_MAX_LEVELS], size[CED_MAX_LEVELS], hashed[CED_MAX_LEVELS];
};

inline void fill_levels(HashLevels &lv, const ced_hash_desc &h)
{
    for (int l = 0; l < CED_MAX_LEVELS; ++l) {
        lv.scale[l] = h.scale[l]; lv.res[l] = h.res[l]; lv.offset[l] = h.offset[l];
        lv.size[l] = h.size[l]; lv.hashed[l] = h.hashed[l];
    }
}

// the fused kernels address the table by 32-bit byte offsets
inline int require_32bit_byte_offsets(const ced_hash_desc &h, const char *who)
{
    CED_REQUIRE(h.total_entries * (uint64_t)((h.table_dtype ? 4 : 8) * (h.temporal ? 4 : 1)) < (1ull << 32),
                "%s: hash table larger than 4 GiB", who);
    return CED_OK;
}

// The level_mode word of a sixteen-level table, 2 bits per gather slot i = levels 4i..4i+3: 2 = all hashed, 0 = mixed.
// With dense_modes a slot of four dense levels is 1, or 3 = all dense with the x-corner pairs as one load (hash_level
// MODE 3): non-temporal tables, and every level of the slot followed by another level of the table -- the pair load of
// a level's last entry reads one entry past the level.  Without it such a slot is 0.
inline int hash_level_modes(const ced_hash_desc &h, bool dense_modes)
{
    int word = 0;
    for (int i = 0; i < 4; ++i) {
        int n_hashed = 0;
        bool pairs = !h.temporal;
        for (int g = 0; g < 4; ++g) {
            const int l = 4 * i + g;
            n_hashed += h.hashed[l] ? 1 : 0;
            pairs = pairs && l + 1 < h.n_levels && (uint64_t)h.offset[l] + h.size[l] < h.total_entries;
        }
        const int dense = dense_modes ? (pairs ? 3 : 1) : 0;
        word |= (n_hashed == 0 ? dense : (n_hashed == 4 ? 2 : 0)) << (2 * i);
    }
    return word;
}

struct FieldArgs {
    int64_t n;
    const int64_t *n_dev;                             // optional device-side sample count (<= n)
    unsigned long long *stamp;                        // optional device {min start, max end} of the launch on the constant
                                                      // wall clock (wall_clock64): first workgroup in, last workgroup out
    const int64_t *base_dev;                          // optional device-side first sample: the per-sample arrays of a
                                                      // rays-mode call (ray_idx32, t0, t1, rgb, sigma) start there
    const float *pos, *t, *dir;                       // explicit mode
    const float *rays_o, *rays_d;                     // rays mode
    const float *sh_ray;                              // optional (rays mode): [n_rays, 3] colour-head SH inputs of lane groups
                                                      // 1..3, computed once per ray (field_device.hpp: sh_ray_store); NULL:
                                                      // the kernel computes them per sample from rays_d
    const int64_t *ray_idx;
    const int32_t *ray_idx32;                         // alternative 32-bit ray indices (frame renderer)
    const float *t0, *t1, *timestamps;
    int rays_mode, t_per_ray, want_rgb;
    float *rgb, *sigma, *geo;
    float aabb[6];
    float moving_step;
    int use_div, time_mode;
    const void *weights;                              // packed blob of the descriptor's mlp_precision
    int table_dtype, temporal;
    int spread_tiles;                                 // tile -> wave mapping (field_device.hpp); ced_set_option("field_spread_tiles")
    int level_mode;                                   // 2 bits per gather slot: 0 mixed, 1 all dense, 2 all hashed, 3 all dense and cannot wrap
    int max_blocks;                                   // workgroups of the launch (ced_field_desc.max_workgroups; <= 0: one per CU)
    const void *table;
    HashLevels levels;
};

// options of ced_set_option (field.hip)
extern std::atomic<int> g_march_two_pass;
extern std::atomic<int> g_field_spread_tiles;
extern std::atomic<int> g_frame_sh_per_ray;
extern std::atomic<int> g_hash_grad_blocks;           // hash.hip
constexpr int kFieldBlocksDefault = 256;      // one persistent workgroup per CU

// Launches a persistent field kernel of NT 16-sample tiles per wave and THREADS threads per workgroup: enough
// workgroups for the tiles under A.spread_tiles, at most A.max_blocks (<= 0: one resident workgroup per CU).
template <int NT, int THREADS, typename Kernel>
void launch_field_grid(Kernel kernel, const FieldArgs &A, void *stream)
{
    const int64_t n_tiles = (A.n + 16 * NT - 1) / (16 * NT);
    constexpr int waves = THREADS / 64;
    int64_t blocks = A.spread_tiles ? (n_tiles + 3) / 4 : (n_tiles + waves - 1) / waves;
    const int cap = A.max_blocks > 0 ? A.max_blocks : kFieldBlocksDefault;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, A);
}

// hash.hip: what every entry that reads the hash table checks of its descriptor
int validate_hash(const ced_hash_desc *h, const char *who);
// Fills the field/hash parts of A from the descriptor, validates, and launches on `stream`.
int launch_field(const ced_field_desc *d, FieldArgs &A, void *stream);
// field_half.hip: the f16x2 / f16 MLP variants (A already filled by launch_field)
int launch_field_half(FieldArgs &A, int time_mode, int precision, void *stream);
// field_mixed.hip: exact sigma chain + split-fp16 colour head (CED_MLP_F32_HEAD16X2)
int launch_field_mixed(FieldArgs &A, int time_mode, void *stream);

}  // namespace ced
