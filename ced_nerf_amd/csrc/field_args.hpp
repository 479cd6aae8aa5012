// Kernel-argument block of the fused field kernel (field.hip), shared with the frame renderer.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>

#include "../../include/cednerf_hip.h"

namespace ced {

struct FieldArgs {
    int64_t n;
    const int64_t *n_dev;                             // optional device-side sample count (<= n)
    unsigned long long *stamp;                        // optional device {min start, max end} of the launch on the constant
                                                      // wall clock (wall_clock64): first workgroup in, last workgroup out
    const int64_t *base_dev;                          // optional device-side first sample: the per-sample arrays of a
                                                      // rays-mode call (ray_idx32, t0, t1, rgb, sigma) start there
    const float *pos, *t, *dir;                       // explicit mode
    const float *rays_o, *rays_d;                     // rays mode
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
    int spread_tiles;                                 // tile -> wave mapping (field.hip); ced_set_option("field_spread_tiles")
    int level_mode;                                   // 2 bits per gather slot: 0 mixed, 1 all dense, 2 all hashed, 3 all dense and cannot wrap
    int max_blocks;                                   // workgroups of the launch (ced_field_desc.max_workgroups; <= 0: one per CU)
    const void *table;
    float scale[CED_MAX_LEVELS];
    uint32_t res[CED_MAX_LEVELS], offset[CED_MAX_LEVELS], size[CED_MAX_LEVELS], hashed[CED_MAX_LEVELS];
};

extern std::atomic<int> g_march_two_pass;
extern std::atomic<int> g_field_spread_tiles;
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

// field.hip: what every entry that reads the hash table checks of its descriptor
int validate_hash(const ced_hash_desc *h, const char *who);
// Fills the field/hash parts of A from the descriptor, validates, and launches on `stream`.
int launch_field(const ced_field_desc *d, FieldArgs &A, void *stream);
// field_half.hip: the f16x2 / f16 MLP variants (A already filled by launch_field)
int launch_field_half(FieldArgs &A, int time_mode, int precision, void *stream);
// field_mixed.hip: exact sigma chain + split-fp16 colour head (CED_MLP_F32_HEAD16X2)
int launch_field_mixed(FieldArgs &A, int time_mode, void *stream);

}  // namespace ced
