#include "ced_common.hpp"
#include "march_accel.hpp"
#include "march_pack.hpp"

namespace ced {

AccelSpec accel_view(const void *accel, int n_grids, int res, bool with_cells);

// One-shot march of every ray to the far plane (nerfacc traverse_grids without a step limit: the marching half of
// OccGridEstimator.sampling, call sites cednerf/utils.py:115-125 and train_real.py:339-350) on the frame renderer's
// accelerated walk: sphere tracing over the brick / cell distance fields through empty space, closed-form DDA re-entry,
// the emitted samples those of the cell-by-cell walk bit for bit (march_accel.hpp).  Count pass -> caller's scan ->
// fill pass, as ced_traverse_grids; one grid level (the multi-level case stays on ced_traverse_grids).
struct MarchAllArgs {
    int64_t n_rays;
    const float *rays_o, *rays_d;
    GridSpec grid;
    AccelSpec accel;
    const float *near_planes;
    float far_plane;
    const float *t_sorted;         // several grid levels: the rays' sorted entry / exit events (cednerf/utils.py:215-225)
    const int64_t *t_indices;
    const uint8_t *hits;
    int64_t *packed;               // [n_rays, 2]: FILL reads the first sample, COUNT writes the count
    float *t_starts, *t_ends;
    int64_t *ray_indices;          // optional
};

template <bool SINGLE, bool FILL>
__global__ __launch_bounds__(kMarchThreads, SINGLE ? 4 : 3) void march_all_kernel(MarchAllArgs A)
{
    const int64_t r = (int64_t)blockIdx.x * kMarchThreads + threadIdx.x;
    if (r >= A.n_rays) return;
    float o[3], d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { o[a] = A.rays_o[3 * r + a]; d[a] = A.rays_d[3 * r + a]; }
    const int m = A.grid.n_grids;
    const float *const ts_row = SINGLE ? nullptr : A.t_sorted + r * 2 * m;
    const int64_t *const ti_row = SINGLE ? nullptr : A.t_indices + r * 2 * m;
    const uint8_t *const hit_row = SINGLE ? nullptr : A.hits + r * m;
    float t_term;
    if constexpr (!FILL) {
        const int n = traverse_ray_frame<kFrameLook, SINGLE, false>(A.grid, A.accel, true, o, d, A.near_planes[r], A.far_plane, ts_row,
                                                             ti_row, hit_row, [](int, float, float) {}, t_term);
        A.packed[2 * r + 1] = n;
    } else {
        const int64_t start = A.packed[2 * r];
        if (A.packed[2 * r + 1] == 0) return;
        float *const p0 = A.t_starts + start, *const p1 = A.t_ends + start;
        int64_t *const pr = A.ray_indices ? A.ray_indices + start : nullptr;
        (void)traverse_ray_frame<kFrameLook, SINGLE, false>(A.grid, A.accel, true, o, d, A.near_planes[r], A.far_plane, ts_row, ti_row,
                                                     hit_row,
                                                     [&](int i, float t0, float t1) {
                                                         p0[i] = t0; p1[i] = t1;
                                                         if (pr) pr[i] = r;
                                                     },
                                                     t_term);
    }
}

// The same march in ONE pass, for callers that can bound the total (a video's frames: the previous frame's count):
// pack_ray_samples (march_pack.hpp, as march_frame_kernel) on a device counter over the caller's arrays.  Rays land in
// workgroup arrival order (packed_info says where); a ray whose range would pass `capacity` stores nothing -- the
// counter then exceeds the capacity and the caller falls back to the two-pass form.
template <bool SINGLE>
__global__ __launch_bounds__(kMarchThreads, SINGLE ? 4 : 3) void march_all_onepass_kernel(MarchAllArgs A, int64_t capacity,
                                                                                         unsigned long long *total)
{
    const int64_t r = (int64_t)blockIdx.x * kMarchThreads + threadIdx.x;
    const bool active = r < A.n_rays;
    const int m = A.grid.n_grids;
    float o[3] = { 0.0f, 0.0f, 0.0f }, d[3] = { 0.0f, 0.0f, 1.0f };
    float near = 0.0f;
    const float *const ts_row = (SINGLE || !active) ? nullptr : A.t_sorted + r * 2 * m;
    const int64_t *const ti_row = (SINGLE || !active) ? nullptr : A.t_indices + r * 2 * m;
    const uint8_t *const hit_row = (SINGLE || !active) ? nullptr : A.hits + r * m;
    const auto walk = [&](auto first, auto &&emit) {
        if constexpr (decltype(first)::value) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { o[a] = A.rays_o[3 * r + a]; d[a] = A.rays_d[3 * r + a]; }
            near = A.near_planes[r];
        }
        float t_term = 0.0f;
        return traverse_ray_frame<kFrameLook, SINGLE, false>(A.grid, A.accel, true, o, d, near, A.far_plane, ts_row, ti_row,
                                                             hit_row, emit, t_term);
    };
    float *p0 = nullptr, *p1 = nullptr;
    pack_ray_samples<kMarchThreads / 64>(
        active, A.grid, walk,
        [&](int run) { return (long long)atomicAdd(total, (unsigned long long)run); },
        [&](int64_t start, int n) {
            A.packed[2 * r] = start;
            A.packed[2 * r + 1] = n;
            p0 = A.t_starts + start; p1 = A.t_ends + start;
            return n > 0 && start + n <= capacity;
        },
        [&](int i, float t0, float t1) { p0[i] = t0; p1[i] = t1; });
}

}  // namespace ced

extern "C" int ced_march_all(int64_t n_rays, const float *rays_o, const float *rays_d, const uint8_t *binaries,
                             int32_t n_grids, int32_t res, const float *aabbs, const void *accel, const float *near_planes,
                             float far_plane, float step_size, float cone_angle, const float *t_sorted,
                             const int64_t *t_indices, const uint8_t *hits, int32_t fill, int64_t *packed_info,
                             float *t_starts, float *t_ends, int64_t *ray_indices, int64_t capacity, int64_t *total,
                             void *stream)
{
    CED_REQUIRE(n_rays >= 0 && res >= 1 && res <= 1024 && n_grids >= 1 && n_grids <= ced::kMaxGrids, "march_all: bad sizes");
    if (n_rays == 0) return CED_OK;
    CED_REQUIRE(rays_o && rays_d && binaries && aabbs && accel && near_planes && packed_info, "march_all: null pointer");
    CED_REQUIRE(n_grids == 1 || (t_sorted && t_indices && hits), "march_all: %d grid levels need the sorted intersections", n_grids);
    CED_REQUIRE(!fill || (t_starts && t_ends), "march_all: fill pass without sample arrays");
    ced::MarchAllArgs A{ n_rays, rays_o, rays_d,
                         ced::GridSpec{ binaries, aabbs, n_grids, res, step_size, cone_angle, 0x7fffffff, nullptr },
                         ced::accel_view(accel, n_grids, res, true), near_planes, far_plane, t_sorted, t_indices, hits,
                         packed_info, t_starts, t_ends, ray_indices };
    const dim3 grid((unsigned)((n_rays + ced::kMarchThreads - 1) / ced::kMarchThreads)), blk(ced::kMarchThreads);
    hipStream_t st = (hipStream_t)stream;
    if (fill == 2) {
        CED_REQUIRE(capacity >= 0 && total != nullptr, "march_all: the one-pass form needs a capacity and a device counter");
        ced::with_bool(n_grids == 1, [&](auto single) {
            hipLaunchKernelGGL((ced::march_all_onepass_kernel<decltype(single)::value>), grid, blk, 0, st, A, capacity,
                               reinterpret_cast<unsigned long long *>(total));
        });
        return ced::check_launch("march_all (one pass)");
    }
    ced::with_bool(n_grids == 1, [&](auto single) {
        ced::with_bool(fill != 0, [&](auto filling) {
            hipLaunchKernelGGL((ced::march_all_kernel<decltype(single)::value, decltype(filling)::value>), grid, blk, 0, st, A);
        });
    });
    return ced::check_launch("march_all");
}
