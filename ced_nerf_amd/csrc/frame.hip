// Frame renderer: the whole of render_image_test (cednerf/utils.py:153-318) behind one C call.
//
// Same algorithm and the same per-ray sample sets as the reference's host loop (image-global schedule
// N_samples = clamp(N_rays // N_alive, min, 64), termination checked between iterations), but
//   * an iteration is four launches instead of ~15 kernels + torch glue:
//       march     : one lane per ALIVE ray (march_accel.hpp: distance fields through empty space, exact DDA where it
//                   matters), the samples ray-packed and dense without a count pass (march_pack.hpp);
//       field     : the fused field kernel (field.hip / field_half.hip) on those samples (count read from device memory);
//       composite : per-ray front-to-back compositing over the alive list; survivors are appended to the next
//                   iteration's list, one range reservation per workgroup;
//       schedule  : one wave turns the survivor counts into the NEXT iteration's plan on the device -- rays alive,
//                   N_samples, slot and sample bases per frame -- and publishes (alive, done) to pinned host memory
//                   (frame_loop.hip);
//   * THE HOST NEVER WAITS FOR AN ITERATION (the reference syncs at utils.py:231 every time): the loop driver of
//     frame_loop.hpp, shared with render_image in eval mode (image.hip).
// Pixels, per-iteration schedule and sample counts are bit-identical to the reference loop.
#include "ced_common.hpp"
#include "composite_core.hpp"
#include "field_args.hpp"
#include "frame_loop.hpp"
#include "march_accel.hpp"
#include "march_diag.hpp"
#include "march_pack.hpp"

namespace ced {

int build_brick_accel(const uint8_t *binaries, int n_grids, int res, uint8_t *dist, uint8_t *scratch, hipStream_t stream);
AccelSpec accel_view(const void *accel, int n_grids, int res, bool with_cells);

__global__ __launch_bounds__(256) void frame_times_kernel(int64_t n_rays, int rays_per_frame,
                                                          const float *__restrict__ frame_times, float *__restrict__ ts_ray)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_rays) ts_ray[r] = frame_times[r / rays_per_frame];
}

// Per-ray setup of cednerf/utils.py:197-225: ray/AABB intersection per grid level and the stably sorted entry/exit event
// list, near planes, and the ray's reset (reset_ray: SH inputs of the colour head, zeroed pixel accumulators).
__global__ __launch_bounds__(256) void frame_prep_kernel(int64_t n_rays, const float *__restrict__ rays_o,
                                                         const float *__restrict__ rays_d, int m,
                                                         const float *__restrict__ aabbs, float near_plane,
                                                         float *__restrict__ t_sorted, uint8_t *__restrict__ t_indices,
                                                         uint8_t *__restrict__ hits, float *__restrict__ near_planes,
                                                         float *__restrict__ sh_ray, float *__restrict__ rgb,
                                                         float *__restrict__ opacity, float *__restrict__ depth)
{
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rays) return;
    const float o[3] = { rays_o[3 * r], rays_o[3 * r + 1], rays_o[3 * r + 2] };
    const float inv_d[3] = { 1.0f / rays_d[3 * r], 1.0f / rays_d[3 * r + 1], 1.0f / rays_d[3 * r + 2] };
    float ev[2 * kMaxGrids];
    int id[2 * kMaxGrids];
    for (int a = 0; a < m; ++a) {
        float t0 = __builtin_inff(), t1 = __builtin_inff();
        bool hit = slab_test(o, inv_d, aabbs + 6 * a, t0, t1);
        if (!hit) { t0 = __builtin_inff(); t1 = __builtin_inff(); }
        hits[r * m + a] = hit ? 1 : 0;
        ev[a] = t0; id[a] = a;
        ev[m + a] = t1; id[m + a] = m + a;
    }
    if (m > 1) {            // stable insertion sort of the 2m events (torch.sort(..., stable=True))
        for (int i = 1; i < 2 * m; ++i) {
            float v = ev[i];
            int k = id[i], j = i - 1;
            while (j >= 0 && ev[j] > v) { ev[j + 1] = ev[j]; id[j + 1] = id[j]; --j; }
            ev[j + 1] = v; id[j + 1] = k;
        }
    }
    for (int i = 0; i < 2 * m; ++i) {
        t_sorted[r * 2 * m + i] = ev[i];
        t_indices[r * 2 * m + i] = (uint8_t)id[i];
    }
    near_planes[r] = near_plane;
    reset_ray(rays_d, r, sh_ray, rgb, opacity, depth);
}

// One grid level: the marching recomputes the ray/box interval itself (march_accel.hpp, SINGLE), so the set-up is only
// the near planes and the ray's reset.
__global__ __launch_bounds__(256) void frame_prep_single_kernel(int64_t n_rays, const float *__restrict__ rays_d,
                                                                float near_plane, float *__restrict__ near_planes,
                                                                float *__restrict__ sh_ray, float *__restrict__ rgb,
                                                                float *__restrict__ opacity, float *__restrict__ depth)
{
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rays) return;
    near_planes[r] = near_plane;
    reset_ray(rays_d, r, sh_ray, rgb, opacity, depth);
}

struct MarchArgs {
    const float *rays_o, *rays_d;
    GridSpec grid;                 // limit is per frame (plan)
    AccelSpec accel;
    float *near_planes;            // in: near plane, out: termination plane (cednerf/utils.py:301)
    float far_plane;
    const int32_t *alive;          // per-frame lists of the rays still alive (NULL: all rays, first iteration)
    int n_frames, rays_per_frame;
    const float *t_sorted;
    const uint8_t *t_indices;      // event ids as bytes (nerfacc's int64 layout would be 64 B per ray at four levels)
    const uint8_t *hits;
    float *t_starts, *t_ends;      // ray-packed samples of the iteration
    int32_t *ray_idx;              // ray of every sample
    int32_t *packed;               // [n_rays, 2] (first sample, count) of the ray in this iteration
    int32_t *cand;                 // first iteration in two passes: the rays march_cull_kernel could not rule out
    const float *t_clear;          // first iteration: [n_frames, groups_per_frame] group clearances (march_accel.hpp)
    int groups_per_frame;
};

// Group clearance, phase A: one wave per group of kGroupRays consecutive rays of a frame (its last group may be
// partial; the padding rays of a sharded frame, local_rays, are no members).  Every lane folds its ray against the
// group's reference ray (group_member) into NV maxima -- 6 deviations and 2 limits per level, padded to a power of
// two -- and the wave reduces them with a halving butterfly: at the step with lane distance 2^s a lane keeps one half of
// its values and trades the other half with its partner, so the first log2(NV) steps take NV - 1 shuffles in all
// instead of NV each, and lane j < NV ends with one value (`mine`), which it stores itself.
constexpr int kGroupThreads = 256;
static_assert(kGroupMaxLevels == kMaxGrids, "group_member's per-level limits");
static_assert(kSlotAlign % kGroupRays == 0 && kGroupRays == 64, "a wave's slots of the first iteration are one group");
template <int NV>
__global__ __launch_bounds__(kGroupThreads) void ray_group_bounds_kernel(
    int n_frames, int rays_per_frame, int groups_per_frame, const int32_t *__restrict__ local_rays,
    const float *__restrict__ rays_o, const float *__restrict__ rays_d, int m, const float *__restrict__ aabbs,
    RayGroupBounds *__restrict__ bounds, float *__restrict__ limits)
{
    static_assert(NV == 8 || NV == 16 || NV == 32, "6 + 2 m values, padded");
    const int lane = threadIdx.x & 63;
    const int64_t n_groups = (int64_t)n_frames * groups_per_frame;
    const float inf = __builtin_inff();
    int mine = 0;                                            // the value lane j < NV ends up with
#pragma unroll
    for (int s = 0; (NV >> s) > 1; ++s) mine += ((lane >> s) & 1) * (NV >> (s + 1));
    for (int64_t g = (int64_t)blockIdx.x * (kGroupThreads / 64) + (threadIdx.x >> 6); g < n_groups;
         g += (int64_t)gridDim.x * (kGroupThreads / 64)) {
        const int f = (int)(g / groups_per_frame);
        const int k0 = (int)(g % groups_per_frame) * kGroupRays;
        const int count = local_rays ? local_rays[f] : rays_per_frame;
        const int members = count - k0 < kGroupRays ? count - k0 : kGroupRays;
        if (members <= 0) continue;                          // no member (the whole wave): phase B writes +inf
        const int64_t r = (int64_t)f * rays_per_frame + k0 + (lane < members ? lane : 0);
        const float o[3] = { rays_o[3 * r], rays_o[3 * r + 1], rays_o[3 * r + 2] };
        const float d[3] = { rays_d[3 * r], rays_d[3 * r + 1], rays_d[3 * r + 2] };
        const int ref = group_reference(members);
        const float oc[3] = { __shfl(o[0], ref, 64), __shfl(o[1], ref, 64), __shfl(o[2], ref, 64) };
        const float dc[3] = { __shfl(d[0], ref, 64), __shfl(d[1], ref, 64), __shfl(d[2], ref, 64) };
        float v[6 + 2 * kMaxGrids > NV ? 6 + 2 * kMaxGrids : NV];
#pragma unroll
        for (float &x : v) x = -inf;
        bool bad = false;
        if (lane < members) group_member(o, d, oc, dc, m, aabbs, v, bad);
#pragma unroll
        for (int s = 0; (NV >> s) > 1; ++s) {
            const int half = NV >> (s + 1);
            const bool up = (lane >> s) & 1;
#pragma unroll
            for (int k = 0; k < half; ++k) {
                const float keep = up ? v[k + half] : v[k], send = up ? v[k] : v[k + half];
                v[k] = fmaxf(keep, __shfl_xor(send, 1 << s, 64));
            }
        }
#pragma unroll
        for (int off = NV; off < 64; off <<= 1) v[0] = fmaxf(v[0], __shfl_xor(v[0], off, 64));
        bad = __any(bad);
        float *B = reinterpret_cast<float *>(bounds + g);    // oc[3], dc[3], dev_o[3], dev_d[3]
        if (lane == ref) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { B[a] = oc[a]; B[3 + a] = dc[a]; }
        }
        if (lane < NV) {
            if (mine < 6) B[6 + mine] = (bad && mine == 0) ? inf : v[0];          // bad: group_clear then claims nothing
            else if (mine < 6 + 2 * m) limits[g * 2 * m + (mine - 6)] = (mine & 1) ? v[0] : -v[0];
        }
    }
}

// Phase B: one LANE per group traces the group's cone (group_clear) -- 64 times fewer wave-instructions than the per-ray
// traces of the groups it clears.  A group without members gets +inf (nobody reads it).
__global__ __launch_bounds__(kGroupThreads) void ray_group_clear_kernel(
    int n_frames, int rays_per_frame, int groups_per_frame, const int32_t *__restrict__ local_rays, AccelSpec S, int m, int res,
    const float *__restrict__ aabbs, const RayGroupBounds *__restrict__ bounds, const float *__restrict__ limits,
    float near_plane, float far_plane, float *__restrict__ t_clear)
{
    const int64_t g = (int64_t)blockIdx.x * kGroupThreads + threadIdx.x;
    if (g >= (int64_t)n_frames * groups_per_frame) return;
    const int count = local_rays ? local_rays[g / groups_per_frame] : rays_per_frame;
    const bool empty = (int)(g % groups_per_frame) * kGroupRays >= count;
    const RayGroupBounds B = bounds[g];
    t_clear[g] = empty ? __builtin_inff() : group_clear(S, m, res, aabbs, B, limits + g * 2 * m, near_plane, far_plane);
}

// First iteration, the groups of the workgroup whose first slot is s0 (kWaves groups: a frame's slots start at a
// multiple of kSlotAlign, so a wave's 64 slots are one group): the clearance of wave `wave`'s own group, and whether
// every group of the workgroup is cleared to the far plane -- from wave-uniform loads, so the answer is the same in
// every thread of the workgroup.
template <int kWaves>
__device__ __forceinline__ bool workgroup_clearance(const MarchArgs &A, const IterPlan &P, int f, int64_t s0, int wave, float &t_own)
{
    const int idx0 = (int)(s0 - P.slot_base[f]);
    const float *row = A.t_clear + (int64_t)f * A.groups_per_frame + (idx0 >> 6);
    bool all_clear = true;
    t_own = 0.0f;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const float tc = idx0 + 64 * w < P.count[f] ? row[w] : __builtin_inff();       // no member in this wave's slots
        all_clear = all_clear && tc == __builtin_inff();
        t_own = w == wave ? tc : t_own;
    }
    return all_clear;
}

// First iteration of a frame, pass one of two.  Nine rays in ten see nothing (the scene fills a few percent of the
// grid), and what decides that is only the sphere trace through the distance field: this pass runs the trace of every
// segment of every ray -- traverse_ray_frame's own first step, the same function on the same arguments -- on a lean
// kernel (no DDA state, twice the waves per SIMD of the marching kernel to hide the probes' latency).  A ray whose
// segments are all traced to their ends marches no sample (packed = {0, 0}); the others are compacted into a list
// that the marching kernel then walks with full waves.
constexpr int kCullThreads = 256;
static_assert(kSlotAlign % kCullThreads == 0, "a culling workgroup's slots belong to one frame");
template <bool SINGLE>
__global__ __launch_bounds__(kCullThreads) void march_cull_kernel(MarchArgs A, IterPlan *__restrict__ plan)
{
    const IterPlan &P = *plan;
    const int64_t total = P.total_slots;
    const int m = SINGLE ? 1 : A.grid.n_grids, res = A.grid.res;
    for (int64_t s0 = (int64_t)blockIdx.x * kCullThreads; s0 < total; s0 += (int64_t)gridDim.x * kCullThreads) {
        // kSlotAlign == kCullThreads: a workgroup's slots belong to one frame
        const int f = frame_of_slot(P, A.n_frames, s0);
        if (f < 0) continue;
        const int64_t idx = s0 + threadIdx.x - P.slot_base[f];
        const bool active = idx < P.count[f];
        const int64_t r = (int64_t)f * A.rays_per_frame + (active ? idx : 0);
        // group clearance: a workgroup of cleared groups is done before it loads a ray (the same decision in all its
        // threads: no barrier below is skipped by a part of it); a cleared group among others takes no trace
        float t_hint = 0.0f;
        if (A.t_clear) {
            const bool all_clear = workgroup_clearance<kCullThreads / 64>(A, P, f, s0, __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), t_hint);
            if (all_clear) {
                if (active) { A.packed[2 * r] = 0; A.packed[2 * r + 1] = 0; }
                continue;
            }
        }
        bool cand = false;
        if (active && t_hint == __builtin_inff()) {
            A.packed[2 * r] = 0; A.packed[2 * r + 1] = 0;
        } else if (active) {
            float o[3], d[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) { o[a] = A.rays_o[3 * r + a]; d[a] = A.rays_d[3 * r + a]; }
            const float near = A.near_planes[r];
            const float inv_d[3] = { 1.0f / d[0], 1.0f / d[1], 1.0f / d[2] };
            // the segments traverse_ray_frame visits, in its order (decode_segment)
            const float *ts_row = SINGLE ? nullptr : A.t_sorted + r * 2 * m;
            const uint8_t *ti_row = SINGLE ? nullptr : A.t_indices + r * 2 * m;
            const uint8_t *hit_row = SINGLE ? nullptr : A.hits + r * m;
            for (int i = 0; i < 2 * m - 1 && !cand; ++i) {
                int lvl;
                float seg_a, seg_b;
                if (!decode_segment<SINGLE>(A.grid, o, inv_d, ts_row, ti_row, hit_row, i, lvl, seg_a, seg_b)) continue;
                const float t0 = fmaxf(seg_a, near), t1 = fminf(seg_b, A.far_plane);
                if (t0 >= t1) continue;
                float t_stop, cells;
                cand = !coarse_advance(A.accel, lvl, res, A.grid.aabbs + 6 * lvl, o, d, t0, t1, t_stop, cells, t_hint);
            }
            if (!cand) { A.packed[2 * r] = 0; A.packed[2 * r + 1] = 0; }
        }
        const int slot = workgroup_append<kCullThreads / 64, 0>(
            cand, nullptr, [&](int run, const int *) { return run > 0 ? atomicAdd(&plan->n_cand, run) : 0; });
        if (cand) A.cand[slot] = (int32_t)r;
        __syncthreads();
    }
}

// One lane per alive ray, its samples into the iteration's arrays by pack_ray_samples (march_pack.hpp).
// FIRST: a frame's first iteration (every segment starts with a sphere trace; the walk in its looking-loop form,
// march_accel.hpp).  CAND: the rays are those of the culling pass's list, any frame's in any order, kCandLanes of them
// per wave (64; measured with 32 and 16 -- more, emptier waves in case a wave alone on its SIMD were bound by the latency
// of its own instruction stream: 118 and 164 us against 91, the kernel is bound by instruction issue, not by that).
constexpr int kCandLanes = 64;
template <bool SINGLE, bool CAND, bool FIRST>
__global__ __launch_bounds__(kMarchThreads, (SINGLE && !CAND) ? 4 : 3) void march_frame_kernel(MarchArgs A, IterPlan *__restrict__ plan)
{
    static_assert(!CAND || FIRST, "the candidate list belongs to the first iteration");
    constexpr int kWaves = kMarchThreads / 64;
    constexpr int kPerGroup = CAND ? kWaves * kCandLanes : kMarchThreads;        // rays of one workgroup pass
    const IterPlan &P = *plan;
    const int64_t total = CAND ? (int64_t)P.n_cand : (int64_t)P.total_slots;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t s0 = (int64_t)blockIdx.x * kPerGroup; s0 < total; s0 += (int64_t)gridDim.x * kPerGroup) {
        int f = 0;
        bool active;
        int64_t r = 0;
        float t_hint = 0.0f;                                 // FIRST: the group clearance of the lane's ray
        if constexpr (CAND) {
            const int64_t slot = s0 + wave * kCandLanes + lane;
            active = lane < kCandLanes && slot < total;
            if (active) {
                r = A.cand[slot]; f = (int)(r / A.rays_per_frame);
                if (A.t_clear) t_hint = A.t_clear[(int64_t)f * A.groups_per_frame + (r - (int64_t)f * A.rays_per_frame) / kGroupRays];
            }
        } else {
            f = frame_of_slot(P, A.n_frames, s0);
            if (f < 0) continue;                             // padding between two frames' slot ranges (whole workgroup)
            const int64_t idx = s0 + threadIdx.x - P.slot_base[f];
            active = idx < P.count[f];
            const int64_t first = (int64_t)f * A.rays_per_frame;
            r = active ? (A.alive ? (int64_t)A.alive[first + idx] : first + idx) : 0;
            if constexpr (FIRST) {
                // group clearance (all rays alive, slot order = ray order): a workgroup of cleared groups is done before
                // it loads a ray -- the same decision in all its threads, so no barrier below is skipped by a part of
                // it; a cleared group among others goes through the pack step as inactive lanes do, with no samples
                if (A.t_clear) {
                    const bool all_clear = workgroup_clearance<kWaves>(A, P, f, s0, __builtin_amdgcn_readfirstlane(wave), t_hint);
                    if (all_clear) {
                        if (active) { A.packed[2 * r] = 0; A.packed[2 * r + 1] = 0; }
                        continue;
                    }
                    if (t_hint == __builtin_inff()) {        // the wave's group is cleared: its lanes are inactive lanes
                        if (active) { A.packed[2 * r] = 0; A.packed[2 * r + 1] = 0; }
                        active = false;
                    }
                }
            }
        }
        const int limit = P.limit[f];
        GridSpec grid = A.grid;
        grid.limit = limit;
        const int m = grid.n_grids;
        float o[3] = { 0.0f, 0.0f, 0.0f }, d[3] = { 0.0f, 0.0f, 1.0f };
        float near = 0.0f;
        const auto walk = [&](auto first, auto &&emit) {
            if constexpr (decltype(first)::value) {
#pragma unroll
                for (int a = 0; a < 3; ++a) { o[a] = A.rays_o[3 * r + a]; d[a] = A.rays_d[3 * r + a]; }
                near = A.near_planes[r];
            }
            float t_term = 0.0f;
            const int n = traverse_ray_frame<kFrameLook, SINGLE, FIRST>(
                grid, A.accel, FIRST, o, d, near, A.far_plane,
                SINGLE ? nullptr : A.t_sorted + r * 2 * m, SINGLE ? (const uint8_t *)nullptr : A.t_indices + r * 2 * m,
                SINGLE ? nullptr : A.hits + r * m, emit, t_term, t_hint);
            if constexpr (decltype(first)::value) A.near_planes[r] = t_term;
            return n;
        };
        float *p0 = nullptr, *p1 = nullptr;
        int32_t *pr = nullptr;
        CED_DIAG_TICK(0);
        pack_ray_samples<kWaves>(
            active, grid, walk,
            [&](int run) {
                return (long long)atomicAdd(reinterpret_cast<unsigned long long *>(&plan->total_samples), (unsigned long long)run);
            },
            [&](int64_t start, int n) {
                A.packed[2 * r] = (int32_t)start;
                A.packed[2 * r + 1] = n;
                p0 = A.t_starts + start; p1 = A.t_ends + start; pr = A.ray_idx + start;
                return true;
            },
            [&](int i, float t0, float t1) { p0[i] = t0; p1[i] = t1; pr[i] = (int32_t)r; });
        CED_DIAG_TICK(7);
        __syncthreads();                                     // wave_tot / block_base are reused by the next chunk
    }
#ifdef CED_MARCH_DIAG
    ced_diag_flush();
#endif
}

// composite_prefix (cednerf/utils.py:274-299) + ray bookkeeping (utils.py:301-307) over the list of alive rays;
// survivors (opacity <= threshold and a full sample budget) are appended to the next iteration's list, one range
// reservation per workgroup; the frame's sample count of the iteration rides in the high word of the same atomic.
__global__ __launch_bounds__(kCompositeThreads) void frame_composite_kernel(
    IterPlan *plan, int n_frames, int rays_per_frame, const int32_t *__restrict__ alive_list,
    int32_t *__restrict__ next_list, const int32_t *__restrict__ packed, const float *__restrict__ t0,
    const float *__restrict__ t1, const float *__restrict__ sig, const float *__restrict__ rgbs, float *__restrict__ rgb,
    float *__restrict__ opacity, float *__restrict__ depth, float opc_thres)
{
    const IterPlan &P = *plan;
    const int64_t total = P.total_slots;
    for (int64_t s0 = (int64_t)blockIdx.x * kCompositeThreads; s0 < total; s0 += (int64_t)gridDim.x * kCompositeThreads) {
        const int f = frame_of_slot(P, n_frames, s0);
        if (f < 0) continue;                                 // padding between two frames' slot ranges (whole workgroup)
        const int limit = P.limit[f];
        const int64_t idx = s0 + threadIdx.x - P.slot_base[f];
        const bool active = idx < P.count[f];
        const int64_t first = (int64_t)f * rays_per_frame;
        const int64_t r = active ? (alive_list ? (int64_t)alive_list[first + idx] : first + idx) : 0;
        int cnt = 0;
        bool alive = false;
        if (active) {
            cnt = packed[2 * r + 1];
            const float op = composite_ray(r, packed[2 * r], cnt, t0, t1, sig, rgbs, rgb, opacity, depth);
            alive = !P.last[f] && survives(op, cnt, limit, opc_thres);
        }
        const int slot = workgroup_append<kCompositeThreads / 64, 1>(alive, &cnt, [&](int run, const int *samples) {
            const unsigned long long add = (unsigned long long)run + ((unsigned long long)samples[0] << 32);
            return add != 0 ? (int)(atomicAdd(&plan->next[f], add) & 0xffffffffull) : 0;
        });
        if (alive) next_list[first + slot] = (int32_t)r;
        __syncthreads();                                     // the append's LDS is reused by the next chunk
    }
}

// Sharded frames: this process's survivors of iteration `it`, per frame, as the int64 row the exchange step sums over
// the processes (ced_shard_exchange.reduce) before frame_schedule_kernel reads it.
__global__ __launch_bounds__(64) void frame_pack_counts_kernel(const IterPlan *__restrict__ plan, int n_frames,
                                                               int64_t *__restrict__ row)
{
    const int f = threadIdx.x;
    if (f >= n_frames) return;
    const unsigned long long nx = __hip_atomic_load(&plan->next[f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool finished = plan->last[f] || plan->gcount[f] == 0 || plan->count[f] == 0;
    row[f] = finished ? 0 : (int64_t)(nx & 0xffffffffull);
}

struct FrameWorkspace {
    float *t_sorted; uint8_t *t_indices; uint8_t *hits; float *near; int32_t *packed;
    int32_t *alive_a, *alive_b;     // double-buffered list of alive ray ids
    IterPlan *plans;                // [max_iters + 1]
    float *lattice;                 // [256] first lattice point per binade (cone_angle == 0)
    float *ts_ray;                  // per-ray time of a multi-frame call
    float *t0, *t1; int32_t *ridx; float *sigma, *rgbs;
    uint8_t *accel;                 // brick distance field when the caller did not bring one
    float *sh_ray;                  // [n, 3] colour-head SH inputs per ray (FieldArgs::sh_ray)
    float *group_clear;             // [groups] clearance per group of kGroupRays rays (march_accel.hpp: group_clear), from
    RayGroupBounds *group_bounds;   // [groups] the group's reference ray and deviations and
    float *group_limits;            // [groups, 2 m] its per-level entry / exit limits
    size_t bytes;
};

static inline int min_samples_of(float cone_angle) { return cone_angle == 0.0f ? 1 : 4; }
// iterations the reference loop can take: each one uses at least min_samples of the max_samples budget
static inline int max_iterations(int max_samples, int min_samples) { return (max_samples + min_samples - 1) / min_samples; }

// Samples one iteration can march, over all frames of a call.  A frame alone: alive * N_samples with N_samples =
// clamp(N // alive, min, 64), i.e. at most N * min_samples.  A SHARE of a frame whose loop is the whole image's
// (ced_shard_exchange): N_samples = N_image // alive_image, and this process's alive rays may be any part of
// alive_image -- at most min(local rays * 64, N_image) samples (or local rays * min_samples when that clamp binds).
static inline int64_t sample_capacity(int n_frames, int64_t rays_per_frame, int min_samples, int64_t global_rays)
{
    int64_t per = rays_per_frame * min_samples;
    if (global_rays > rays_per_frame) {
        const int64_t worst = rays_per_frame * 64 < global_rays ? rays_per_frame * 64 : global_rays;
        if (worst > per) per = worst;
    }
    return per * n_frames;
}

static inline int64_t groups_of(int64_t rays_per_frame) { return (rays_per_frame + kGroupRays - 1) / kGroupRays; }

static FrameWorkspace carve(void *base, int n_frames, int64_t rays_per_frame, int m, int64_t cap, int max_iters, int res,
                            bool per_ray_times = false)
{
    const int64_t n = (int64_t)n_frames * rays_per_frame, groups = (int64_t)n_frames * groups_of(rays_per_frame);
    FrameWorkspace w{};
    Carver c{ (char *)base };
    w.t_sorted = c.take<float>((size_t)n * 2 * m);
    w.t_indices = c.take<uint8_t>((size_t)n * 2 * m);
    w.hits = c.take<uint8_t>((size_t)n * m);
    w.near = c.take<float>((size_t)n);
    w.packed = c.take<int32_t>((size_t)n * 2);
    w.alive_a = c.take<int32_t>((size_t)n);
    w.alive_b = c.take<int32_t>((size_t)n);
    w.plans = c.take<IterPlan>((size_t)max_iters + 2);
    w.lattice = c.take<float>(256);
    w.ts_ray = c.take<float>(per_ray_times ? (size_t)n : 0);
    w.t0 = c.take<float>((size_t)cap);
    w.t1 = c.take<float>((size_t)cap);
    w.ridx = c.take<int32_t>((size_t)cap);
    w.sigma = c.take<float>((size_t)cap);
    w.rgbs = c.take<float>((size_t)cap * 3);
    const int64_t nbk = (res + kBrick - 1) / kBrick;
    w.accel = c.take<uint8_t>((size_t)(2 * m * nbk * nbk * nbk));       // brick field + scratch (no accel from the caller)
    w.sh_ray = c.take<float>((size_t)n * 3);
    w.group_clear = c.take<float>((size_t)groups);
    w.group_bounds = c.take<RayGroupBounds>((size_t)groups);
    w.group_limits = c.take<float>((size_t)groups * 2 * m);
    w.bytes = c.off;
    return w;
}

// What a call of the frame loop takes: `n_frames` frames of `rays_per_frame` rays each (ced_render_image_test: one frame).
// frame_times == nullptr: `timestamps` is what the field kernel gets ([1] shared or [n_rays] per ray, t_per_ray);
// otherwise frame_times [n_frames] holds one time per frame and is expanded to a per-ray array.  The other fields are
// the entry points' arguments of the same names (include/cednerf_hip.h).
struct FrameCall {
    const char *who;
    const ced_field_desc *field;
    int n_frames;
    int64_t rays_per_frame, workspace_bytes;
    const float *rays_o, *rays_d, *aabbs, *timestamps, *frame_times, *bkgd;
    const uint8_t *binaries;
    const void *accel;
    int32_t n_grids, res, max_samples, t_per_ray;
    float near_plane, far_plane, step_size, cone_angle, early_stop_eps;
    float *rgb, *opacity, *depth;
    void *workspace, *field_stream, *stream;
    int64_t *host_stats, *total_samples_out;
    ced_frame_trace *trace;
    const ced_shard_exchange *xch;
};

static int render_frames_impl(const FrameCall &c)
{
    hipStream_t stream = (hipStream_t)c.stream;
    // Optional separate stream for the field kernel: callers that keep several frames in flight may hand every frame
    // the same field stream, so that the field launches of different frames queue behind each other.
    hipStream_t fstream = c.field_stream ? (hipStream_t)c.field_stream : stream;
    const bool split = fstream != stream;
    constexpr int kMaxDevices = 64;
    static thread_local hipEvent_t ev_to_field[kMaxDevices] = {}, ev_from_field[kMaxDevices] = {};
    int dev = 0;
    if (split) {                // events belong to the device they were created on
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return check_launch("render_image_test (device)");
        if (!ev_to_field[dev] &&
            (hipEventCreateWithFlags(&ev_to_field[dev], hipEventDisableTiming) != hipSuccess ||
             hipEventCreateWithFlags(&ev_from_field[dev], hipEventDisableTiming) != hipSuccess))
            return check_launch("render_image_test (event create)");
    }
    const int64_t n_rays = (int64_t)c.n_frames * c.rays_per_frame;
    CED_REQUIRE(c.field != nullptr, "%s: null field descriptor", c.who);
    CED_REQUIRE(c.n_frames >= 1 && c.n_frames <= kMaxFrames, "%s: n_frames must be 1..%d", c.who, kMaxFrames);
    CED_REQUIRE(c.rays_per_frame >= 0 && c.n_grids >= 1 && c.n_grids <= kMaxGrids && c.res >= 1 && c.res <= 1024, "%s: bad sizes", c.who);
    CED_REQUIRE(n_rays < (1ll << 31) / 4, "%s: too many rays for 32-bit sample indices", c.who);
    CED_REQUIRE(c.max_samples >= 0, "%s: max_samples < 0", c.who);
    if (c.total_samples_out)
        for (int f = 0; f < c.n_frames; ++f) c.total_samples_out[f] = 0;
    if (c.trace) c.trace->n_iters = 0;
    if (n_rays == 0) return CED_OK;
    CED_REQUIRE(c.rays_o && c.rays_d && c.binaries && c.aabbs && (c.timestamps || c.frame_times) && c.rgb && c.opacity && c.depth &&
                    c.workspace && c.host_stats,
                "%s: null pointer", c.who);
    const int min_samples = min_samples_of(c.cone_angle);
    const int64_t cap = sample_capacity(c.n_frames, c.rays_per_frame, min_samples, c.xch ? c.xch->global_rays_per_frame : 0);
    CED_REQUIRE(cap < (1ll << 31) - 64, "%s: too many samples per iteration for 32-bit sample indices", c.who);
    const int max_iters = max_iterations(c.max_samples, min_samples);
    FrameWorkspace W = carve(c.workspace, c.n_frames, c.rays_per_frame, c.n_grids, cap, max_iters, c.res, c.frame_times != nullptr);
    CED_REQUIRE((int64_t)W.bytes <= c.workspace_bytes, "%s: workspace too small (%lld < %lld bytes)", c.who,
                (long long)c.workspace_bytes, (long long)W.bytes);
    if (c.xch) {
        CED_REQUIRE(c.xch->reduce && c.xch->counts && c.xch->global_rays_per_frame >= c.rays_per_frame &&
                        c.xch->global_rays_per_frame < (1ll << 31),
                    "%s: bad ced_shard_exchange (reduce / counts NULL, or global_rays_per_frame < rays_per_frame)", c.who);
        CED_REQUIRE(!c.field_stream || c.field_stream == c.stream, "%s: a sharded call takes no separate field stream", c.who);
    }
    const dim3 blk(256), grd((unsigned)((n_rays + 255) / 256));

    if (c.n_grids == 1)
        hipLaunchKernelGGL(frame_prep_single_kernel, grd, blk, 0, stream, n_rays, c.rays_d, c.near_plane, W.near, W.sh_ray, c.rgb,
                           c.opacity, c.depth);
    else
        hipLaunchKernelGGL(frame_prep_kernel, grd, blk, 0, stream, n_rays, c.rays_o, c.rays_d, (int)c.n_grids, c.aabbs, c.near_plane,
                           W.t_sorted, W.t_indices, W.hits, W.near, W.sh_ray, c.rgb, c.opacity, c.depth);
    if (c.frame_times)
        hipLaunchKernelGGL(frame_times_kernel, grd, blk, 0, stream, n_rays, (int)c.rays_per_frame, c.frame_times, W.ts_ray);
    const int nb = (c.res + kBrick - 1) / kBrick;
    AccelSpec acc;
    if (c.accel) {
        acc = accel_view(c.accel, c.n_grids, c.res, true);           // the caller's: brick and cell fields
    } else {                                                         // none brought: the cheap brick field, per call
        int rc = build_brick_accel(c.binaries, c.n_grids, c.res, W.accel, W.accel + (size_t)c.n_grids * nb * nb * nb, stream);
        if (rc) return rc;
        acc = AccelSpec{ W.accel, nb, nullptr };
    }
    // group clearances of the rays passed in, once per call: the first iteration skips the groups that see nothing and
    // starts the others' traces where their group's ends (march_accel.hpp)
    // (near plane >= 0 is the bound's precondition: with a negative one nothing is computed and the walks take no hint)
    const int gpf = (int)groups_of(c.rays_per_frame);
    const bool clear_groups = acc.bdist && c.near_plane >= 0.0f;
    if (clear_groups) {
        const int64_t n_groups = (int64_t)c.n_frames * gpf;
        const int32_t *local = c.xch ? c.xch->local_rays : nullptr;
        int64_t agrid = (n_groups + kGroupThreads / 64 - 1) / (kGroupThreads / 64);
        if (agrid > 16384) agrid = 16384;
        const auto bounds_kernel = c.n_grids == 1 ? ray_group_bounds_kernel<8>
                                   : (c.n_grids <= 5 ? ray_group_bounds_kernel<16> : ray_group_bounds_kernel<32>);
        hipLaunchKernelGGL(bounds_kernel, dim3((unsigned)agrid), dim3(kGroupThreads), 0, stream, c.n_frames,
                           (int)c.rays_per_frame, gpf, local, c.rays_o, c.rays_d, (int)c.n_grids, c.aabbs, W.group_bounds, W.group_limits);
        hipLaunchKernelGGL(ray_group_clear_kernel, dim3((unsigned)((n_groups + kGroupThreads - 1) / kGroupThreads)), dim3(kGroupThreads),
                           0, stream, c.n_frames, (int)c.rays_per_frame, gpf, local, acc, (int)c.n_grids, (int)c.res, c.aabbs,
                           W.group_bounds, W.group_limits, c.near_plane, c.far_plane, W.group_clear);
    }
    const bool use_lattice = c.cone_angle == 0.0f && c.step_size > 0.0f && c.near_plane >= 0.0f;
    if (use_lattice) build_lattice(c.near_plane, c.step_size, reinterpret_cast<float *>(c.host_stats + kHostLatticeWord));
    FrameLoop L{ ScheduleArgs{ W.plans, -1, c.n_frames, (int)c.rays_per_frame, min_samples, (int)c.max_samples,
                               (long long *)c.host_stats, 0, c.xch ? c.xch->local_rays : nullptr,
                               c.xch ? c.xch->counts : nullptr, c.xch ? c.xch->global_rays_per_frame : 0,
                               c.xch ? (long long *)c.host_stats + kHostIterWord : nullptr },
                 W.alive_a, W.alive_b, max_iters, c.who };
    L.begin(stream, use_lattice ? W.lattice : nullptr, (unsigned long long *)(c.trace ? c.trace->field_stamps : nullptr),
            (c.trace && c.trace->field_stamps) ? (int)c.trace->capacity : 0);
    int rc = check_launch("render_image_test (prep)");
    if (rc) return rc;

    const float opc_thres = (float)(1.0 - (double)c.early_stop_eps);
    for (; L.it < L.max_iters; ++L.it) {
        bool stop = false;
        rc = L.next(stop);
        if (rc) return rc;
        if (stop) break;
        const int it = L.it;
        IterPlan *plan = L.plan();
        const int32_t *cur_list = L.cur_list();
        int32_t *next_list = L.next_list();

        // slots <= alive rays + padding between frames; the kernels stride over what the plan really holds
        const int64_t slot_bound = L.alive_bound + (int64_t)c.n_frames * kSlotAlign;
        MarchArgs M{ c.rays_o, c.rays_d,
                     GridSpec{ c.binaries, c.aabbs, c.n_grids, c.res, c.step_size, c.cone_angle, 0, use_lattice ? W.lattice : nullptr },
                     acc, W.near, c.far_plane, cur_list, c.n_frames, (int)c.rays_per_frame, W.t_sorted, W.t_indices, W.hits,
                     W.t0, W.t1, W.ridx, W.packed, W.alive_b, (it == 0 && clear_groups) ? W.group_clear : nullptr, gpf };
        int64_t mgrid = (slot_bound + kMarchThreads - 1) / kMarchThreads;
        if (mgrid > 8192) mgrid = 8192;
        const dim3 mblk(kMarchThreads);
        // Two passes pay where the marching kernel is heavy (several grid levels: sorted event lists, 160 registers,
        // three waves per SIMD): C4 +3 % pipelined, first iteration 370 -> 335 us; one level: 103 us in one pass
        // against 29 + 91 in two.
        const int two_pass_opt = g_march_two_pass;
        const bool two_pass = two_pass_opt < 0 ? c.n_grids > 1 : two_pass_opt != 0;
        with_bool(c.n_grids == 1, [&](auto single) {
            constexpr bool kSingle = decltype(single)::value;
            if (it == 0 && acc.bdist && two_pass) {
                // first iteration in two passes: cull by the sphere trace alone, then march the rays that are left
                int64_t kgrid = (slot_bound + kCullThreads - 1) / kCullThreads;
                if (kgrid > 8192) kgrid = 8192;
                if (mgrid > 4096) mgrid = 4096;                  // the list's length is only known on the device
                hipLaunchKernelGGL(march_cull_kernel<kSingle>, dim3((unsigned)kgrid), dim3(kCullThreads), 0, stream, M, plan);
                hipLaunchKernelGGL((march_frame_kernel<kSingle, true, true>), dim3((unsigned)mgrid), mblk, 0, stream, M, plan);
            } else if (it == 0) {
                hipLaunchKernelGGL((march_frame_kernel<kSingle, false, true>), dim3((unsigned)mgrid), mblk, 0, stream, M, plan);
            } else {
                hipLaunchKernelGGL((march_frame_kernel<kSingle, false, false>), dim3((unsigned)mgrid), mblk, 0, stream, M, plan);
            }
        });
        rc = check_launch("render_image_test (march)");
        if (rc) return rc;

        FieldArgs F{};
        F.n = cap;                          // host-side upper bound; the kernel reads the exact count from the plan
        F.n_dev = &plan->total_samples;
        F.rays_o = c.rays_o; F.rays_d = c.rays_d; F.ray_idx32 = W.ridx;
        F.sh_ray = g_frame_sh_per_ray ? W.sh_ray : nullptr;
        F.t0 = W.t0; F.t1 = W.t1;
        F.timestamps = c.frame_times ? W.ts_ray : c.timestamps;
        F.rays_mode = 1; F.t_per_ray = (c.frame_times || c.t_per_ray) ? 1 : 0; F.want_rgb = 1;
        F.rgb = W.rgbs; F.sigma = W.sigma; F.geo = nullptr;
        if (c.trace && c.trace->field_stamps && it < c.trace->capacity)
            F.stamp = reinterpret_cast<unsigned long long *>(c.trace->field_stamps) + 2 * it;
        if (split) {
            (void)hipEventRecord(ev_to_field[dev], stream);
            (void)hipStreamWaitEvent(fstream, ev_to_field[dev], 0);
        }
        if (c.trace && it < c.trace->capacity && c.trace->field_begin)
            (void)hipEventRecord((hipEvent_t)c.trace->field_begin[it], fstream);
        rc = launch_field(c.field, F, (void *)fstream);
        if (rc) return rc;
        if (c.trace && it < c.trace->capacity && c.trace->field_end)
            (void)hipEventRecord((hipEvent_t)c.trace->field_end[it], fstream);
        if (split) {
            (void)hipEventRecord(ev_from_field[dev], fstream);
            (void)hipStreamWaitEvent(stream, ev_from_field[dev], 0);
        }

        int64_t cgrid = (slot_bound + kCompositeThreads - 1) / kCompositeThreads;
        if (cgrid > 4096) cgrid = 4096;
        hipLaunchKernelGGL(frame_composite_kernel, dim3((unsigned)cgrid), dim3(kCompositeThreads), 0, stream,
                           plan, c.n_frames, (int)c.rays_per_frame, cur_list, next_list, W.packed, W.t0, W.t1, W.sigma, W.rgbs,
                           c.rgb, c.opacity, c.depth, opc_thres);
        int64_t *xrow = nullptr;
        if (c.xch) {
            // the exchange step: this process's survivors per frame -> summed over the processes, on the stream
            xrow = c.xch->counts + (int64_t)it * c.n_frames;
            hipLaunchKernelGGL(frame_pack_counts_kernel, dim3(1), dim3(64), 0, stream, plan, c.n_frames, xrow);
            rc = check_launch("render_image_test (pack counts)");
            if (rc) return rc;
            const int xrc = c.xch->reduce(c.xch->user, xrow, c.n_frames, it, (void *)stream);
            if (xrc != 0) {
                set_error("%s: the exchange step of iteration %d failed (code %d)", c.who, it, xrc);
                (void)hipStreamSynchronize(stream);
                return CED_E_LAUNCH;
            }
        }
        L.schedule(stream);
        rc = check_launch("render_image_test (composite / schedule)");
        if (rc) return rc;
    }
    rc = ced_finalize_pixels(n_rays, c.bkgd, c.rgb, c.opacity, c.depth, stream);
    if (rc) return rc;
    std::vector<IterPlan> plans;
    int n_iters = 0;
    rc = L.finish(stream, "render_image_test (read-back)", plans, n_iters);
    if (rc) return rc;
    int64_t total[kMaxFrames] = { 0 };
    for (int k = 0; k < n_iters; ++k) {
        const IterPlan &P = plans[k];
        int64_t alive_total = 0, samples_it = 0;
        int max_limit = 0;
        for (int f = 0; f < c.n_frames; ++f) {
            alive_total += P.count[f];
            samples_it += (int64_t)(P.next[f] >> 32);
            total[f] += (int64_t)(P.next[f] >> 32);
            if (P.count[f] > 0 && P.limit[f] > max_limit) max_limit = P.limit[f];
        }
        if (c.trace && k < c.trace->capacity) {
            if (c.trace->iter_alive) c.trace->iter_alive[k] = alive_total;
            if (c.trace->iter_n_samples) c.trace->iter_n_samples[k] = max_limit;
            if (c.trace->iter_samples) c.trace->iter_samples[k] = samples_it;
        }
    }
    if (c.trace) c.trace->n_iters = n_iters;
    if (c.total_samples_out)
        for (int f = 0; f < c.n_frames; ++f) c.total_samples_out[f] = total[f];
    return CED_OK;
}

}  // namespace ced

extern "C" int64_t ced_render_image_test_workspace_bytes(int64_t n_rays, int32_t n_grids, int32_t res,
                                                         float cone_angle, int32_t max_samples)
{
    if (n_rays < 0 || n_grids < 1 || n_grids > ced::kMaxGrids || res < 1 || res > 1024 || max_samples < 0) return -1;
    const int ms = ced::min_samples_of(cone_angle);
    return (int64_t)ced::carve(nullptr, 1, n_rays, n_grids, n_rays * ms, ced::max_iterations(max_samples, ms), res).bytes;
}

extern "C" int ced_render_image_test(const ced_field_desc *field, int64_t n_rays, const float *rays_o,
                                     const float *rays_d, const uint8_t *binaries, int32_t n_grids, int32_t res,
                                     const float *aabbs, const void *accel, float near_plane, float far_plane,
                                     float step_size, float cone_angle, float early_stop_eps, int32_t max_samples,
                                     const float *timestamps, int32_t t_per_ray, const float *bkgd, float *rgb,
                                     float *opacity, float *depth, void *workspace, int64_t workspace_bytes,
                                     int64_t *host_stats, int64_t *total_samples_out, ced_frame_trace *trace,
                                     void *field_stream_, void *stream_)
{
    ced::FrameCall c{};
    c.who = "render_image_test"; c.field = field; c.n_frames = 1; c.rays_per_frame = n_rays; c.rays_o = rays_o; c.rays_d = rays_d;
    c.binaries = binaries; c.n_grids = n_grids; c.res = res; c.aabbs = aabbs; c.accel = accel; c.near_plane = near_plane;
    c.far_plane = far_plane; c.step_size = step_size; c.cone_angle = cone_angle; c.early_stop_eps = early_stop_eps;
    c.max_samples = max_samples; c.timestamps = timestamps; c.t_per_ray = t_per_ray; c.frame_times = nullptr; c.bkgd = bkgd;
    c.rgb = rgb; c.opacity = opacity; c.depth = depth; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    c.host_stats = host_stats; c.total_samples_out = total_samples_out; c.trace = trace; c.field_stream = field_stream_;
    c.stream = stream_; c.xch = nullptr;
    return ced::render_frames_impl(c);
}

extern "C" int64_t ced_render_frames_test_workspace_bytes(int32_t n_frames, int64_t rays_per_frame, int32_t n_grids,
                                                          int32_t res, float cone_angle, int32_t max_samples)
{
    // not sharded: the image's rays are the frame's own
    return ced_render_frames_test_sharded_workspace_bytes(n_frames, rays_per_frame, rays_per_frame, n_grids, res, cone_angle,
                                                          max_samples);
}

extern "C" int ced_render_frames_test(const ced_field_desc *field, int32_t n_frames, int64_t rays_per_frame,
                                      const float *rays_o, const float *rays_d, const uint8_t *binaries, int32_t n_grids,
                                      int32_t res, const float *aabbs, const void *accel, float near_plane,
                                      float far_plane, float step_size, float cone_angle, float early_stop_eps,
                                      int32_t max_samples, const float *frame_times, const float *bkgd, float *rgb,
                                      float *opacity, float *depth, void *workspace, int64_t workspace_bytes,
                                      int64_t *host_stats, int64_t *total_samples_out, ced_frame_trace *trace,
                                      void *field_stream_, void *stream_)
{
    CED_REQUIRE(frame_times != nullptr, "render_frames_test: null frame_times");
    ced::FrameCall c{};
    c.who = "render_frames_test"; c.field = field; c.n_frames = n_frames; c.rays_per_frame = rays_per_frame; c.rays_o = rays_o; c.rays_d = rays_d;
    c.binaries = binaries; c.n_grids = n_grids; c.res = res; c.aabbs = aabbs; c.accel = accel; c.near_plane = near_plane;
    c.far_plane = far_plane; c.step_size = step_size; c.cone_angle = cone_angle; c.early_stop_eps = early_stop_eps;
    c.max_samples = max_samples; c.timestamps = nullptr; c.t_per_ray = 0; c.frame_times = frame_times; c.bkgd = bkgd;
    c.rgb = rgb; c.opacity = opacity; c.depth = depth; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    c.host_stats = host_stats; c.total_samples_out = total_samples_out; c.trace = trace; c.field_stream = field_stream_;
    c.stream = stream_; c.xch = nullptr;
    return ced::render_frames_impl(c);
}

extern "C" int64_t ced_render_frames_test_sharded_workspace_bytes(int32_t n_frames, int64_t rays_per_frame,
                                                                  int64_t global_rays_per_frame, int32_t n_grids,
                                                                  int32_t res, float cone_angle, int32_t max_samples)
{
    if (n_frames < 1 || n_frames > ced::kMaxFrames || rays_per_frame < 0 || global_rays_per_frame < rays_per_frame ||
        n_grids < 1 || n_grids > ced::kMaxGrids || res < 1 || res > 1024 || max_samples < 0)
        return -1;
    const int ms = ced::min_samples_of(cone_angle);
    return (int64_t)ced::carve(nullptr, n_frames, rays_per_frame, n_grids, ced::sample_capacity(n_frames, rays_per_frame, ms, global_rays_per_frame),
                               ced::max_iterations(max_samples, ms), res, true).bytes;
}

extern "C" int32_t ced_render_frames_test_iterations(float cone_angle, int32_t max_samples)
{
    if (max_samples < 0) return -1;
    return ced::max_iterations(max_samples, ced::min_samples_of(cone_angle));
}

extern "C" int64_t ced_render_frames_test_host_bytes(float cone_angle, int32_t max_samples)
{
    if (max_samples < 0) return -1;
    const int64_t iters = ced::max_iterations(max_samples, ced::min_samples_of(cone_angle));
    return (ced::kHostIterWord + 3 * (iters + 2)) * (int64_t)sizeof(int64_t);
}

extern "C" int ced_render_frames_test_sharded(const ced_field_desc *field, int32_t n_frames, int64_t rays_per_frame,
                                              const float *rays_o, const float *rays_d, const uint8_t *binaries,
                                              int32_t n_grids, int32_t res, const float *aabbs, const void *accel,
                                              float near_plane, float far_plane, float step_size, float cone_angle,
                                              float early_stop_eps, int32_t max_samples, const float *frame_times,
                                              const float *bkgd, float *rgb, float *opacity, float *depth, void *workspace,
                                              int64_t workspace_bytes, int64_t *host_stats, int64_t *total_samples_out,
                                              ced_frame_trace *trace, void *field_stream_, void *stream_,
                                              const ced_shard_exchange *exchange)
{
    CED_REQUIRE(frame_times != nullptr, "render_frames_test_sharded: null frame_times");
    ced::FrameCall c{};
    c.who = "render_frames_test_sharded"; c.field = field; c.n_frames = n_frames; c.rays_per_frame = rays_per_frame; c.rays_o = rays_o; c.rays_d = rays_d;
    c.binaries = binaries; c.n_grids = n_grids; c.res = res; c.aabbs = aabbs; c.accel = accel; c.near_plane = near_plane;
    c.far_plane = far_plane; c.step_size = step_size; c.cone_angle = cone_angle; c.early_stop_eps = early_stop_eps;
    c.max_samples = max_samples; c.timestamps = nullptr; c.t_per_ray = 0; c.frame_times = frame_times; c.bkgd = bkgd;
    c.rgb = rgb; c.opacity = opacity; c.depth = depth; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    c.host_stats = host_stats; c.total_samples_out = total_samples_out; c.trace = trace; c.field_stream = field_stream_;
    c.stream = stream_; c.xch = exchange;
    return ced::render_frames_impl(c);
}
