// What the iterating renderers share (frame.hip: render_image_test and its multi-frame / sharded forms; image.hip:
// render_image in eval mode; march_all.hip borrows the workgroup reservation): the plan of an iteration in device
// memory, the workgroup-wide slot reservations, the per-ray reset, the workspace carver, and the host's loop driver.
//
// THE HOST NEVER WAITS FOR AN ITERATION: every kernel reads its sizes from the plan in device memory, grids are sized by
// the last PUBLISHED alive count (an upper bound: the count only falls) and the host enqueues up to kRunAhead (1)
// iteration beyond the last one it has seen published; iterations enqueued after the loop has finished are empty launches.
#pragma once
#include <type_traits>
#include <vector>

#include "ced_common.hpp"
#include "field_device.hpp"

namespace ced {

constexpr int kMaxGrids = 8;
constexpr int kMaxFrames = 64;      // frames rendered by one call (ced_render_frames_test); one lane of the scheduling wave each
constexpr int kSlotAlign = 256;     // a frame's ray slots start at a multiple of this: no workgroup straddles two frames
constexpr int kRunAhead = 1;       // iterations the host enqueues beyond the last plan it has seen published
constexpr int kMarchThreads = 128;
constexpr int kCompositeThreads = 256;
constexpr int kHostLatticeWord = 8;    // host_stats: words 0..2 publish {alive, done, seq}; the lattice table from word 8 on
constexpr int kHostIterWord = 8 + 128; // sharded calls: {alive here, done, seq} of plan k at word kHostIterWord + 3k

// The plan of ONE iteration, in device memory (written by make_next_plan, read by that iteration's launches).
// Several frames in one call: the rays of all frames are one array (frame f owns ray ids [f*rays_per_frame,
// (f+1)*rays_per_frame)); every frame keeps its OWN reference loop (N_samples on its own counts, its own end) and its
// own alive list; a launch covers the frames' alive rays back to back.
struct IterPlan {
    int32_t count[kMaxFrames];       // rays of frame f alive entering the iteration, in THIS process (0: none left here)
    int32_t gcount[kMaxFrames];      // the same over all processes that share the frame (= count unless the frame's rays
                                     // are sharded, ced_shard_exchange); 0: the frame has finished
    int32_t limit[kMaxFrames];       // the frame's N_samples in this iteration (cednerf/utils.py:235)
    int32_t last[kMaxFrames];        // the frame's loop ends after this iteration (max_samples reached, utils.py:229)
    int32_t used[kMaxFrames];        // the frame's iter_samples, this iteration included (utils.py:236)
    int32_t slot_base[kMaxFrames];   // first ray slot of the frame in this iteration's launches (multiple of kSlotAlign)
    int32_t samp_bound[kMaxFrames];  // count * limit: the frame's samples of the iteration are at most this many
    int32_t total_slots;             // end of the last frame's ray-slot range
    int32_t done;                    // nothing left: this and every later iteration is an empty launch
    int32_t n_cand;                  // first iteration: rays the culling pass could not rule out (march_cull_kernel)
    int32_t cursor;                  // first iteration, candidate list: next entry the persistent marching waves take
    int64_t sample_base;             // render_image: first entry of the iteration in the call's persistent sample arrays
    int64_t total_samples;           // samples RESERVED in the iteration so far: the marching workgroups add their totals
                                     // (ray-packed allocation); the field kernel's n once the marching launch is over
    // filled in DURING the iteration by the compositing kernel: low word = survivors appended to the frame's next
    // alive list, high word = samples the frame marched in this iteration
    unsigned long long next[kMaxFrames];
};

// frame of the workgroup whose first ray slot is s0 (block-uniform), -1 for the padding between two frames
__device__ __forceinline__ int frame_of_slot(const IterPlan &P, int n_frames, int64_t s0)
{
    // slot_base is non-decreasing and a frame without rays shares its base with the next one: the LAST frame whose
    // base is <= s0 is the only candidate (binary search; n_frames <= 64)
    int lo = 0, hi = n_frames - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int64_t)P.slot_base[mid] <= s0) lo = mid; else hi = mid - 1;
    }
    return (P.count[lo] > 0 && s0 >= P.slot_base[lo] && s0 < (int64_t)P.slot_base[lo] + P.count[lo]) ? lo : -1;
}

// Workgroup range reservation: every lane asks for n slots (wave-inclusive prefix sums, an exclusive scan of the wave
// totals in LDS); thread 0 hands the workgroup's total, when there is one, to reserve(total), which makes the site's
// single atomic and returns the range's first slot.  Returns the lane's first slot.  Two barriers: a persistent loop
// that calls this again puts a third one behind its last use of the result.
template <int kWaves, class Reserve>
__device__ __forceinline__ int64_t workgroup_reserve(int n, Reserve reserve)
{
    __shared__ int wave_tot[kWaves];
    __shared__ long long block_base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = n;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int w = 0; w < kWaves; ++w) { const int t = wave_tot[w]; wave_tot[w] = run; run += t; }
        block_base = run > 0 ? reserve(run) : 0;
    }
    __syncthreads();
    return (int64_t)block_base + wave_tot[wave] + (incl - n);
}

// Ballot append: every lane that takes one slot gets its own, in lane order (ballot and popcount per wave, an exclusive
// scan of the wave counts in LDS).  kSums per-lane values sums[k] are summed over the workgroup on the way; thread 0
// calls reserve(count, totals) with the workgroup's slot count and those totals, which makes the site's atomics and
// returns the first slot.  Returns the lane's slot (meaningful where take).  Barriers as workgroup_reserve.
template <int kWaves, int kSums, class Reserve>
__device__ __forceinline__ int workgroup_append(bool take, const int *sums, Reserve reserve)
{
    __shared__ int wave_cnt[kWaves], wave_sum[kSums > 0 ? kSums : 1][kWaves];
    __shared__ int block_base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long ballot = __ballot(take);
    int tot[kSums > 0 ? kSums : 1];
#pragma unroll
    for (int k = 0; k < kSums; ++k) tot[k] = sums[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int k = 0; k < kSums; ++k) tot[k] += __shfl_xor(tot[k], off, 64);
    if (lane == 0) {
        wave_cnt[wave] = __builtin_popcountll(ballot);
#pragma unroll
        for (int k = 0; k < kSums; ++k) wave_sum[k][wave] = tot[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
#pragma unroll
        for (int k = 0; k < kSums; ++k) tot[k] = 0;
        for (int w = 0; w < kWaves; ++w) {
            const int t = wave_cnt[w]; wave_cnt[w] = run; run += t;
#pragma unroll
            for (int k = 0; k < kSums; ++k) tot[k] += wave_sum[k][w];
        }
        block_base = reserve(run, tot);
    }
    __syncthreads();
    return block_base + wave_cnt[wave] + __builtin_popcountll(ballot & ((1ull << lane) - 1ull));
}

// A ray before its first iteration: the colour head's per-ray SH inputs (FieldArgs::sh_ray) and zeroed pixel sums.
__device__ __forceinline__ void reset_ray(const float *__restrict__ rays_d, int64_t r, float *__restrict__ sh_ray,
                                          float *__restrict__ rgb, float *__restrict__ opacity, float *__restrict__ depth)
{
    sh_ray_store(rays_d, r, sh_ray);
    rgb[3 * r] = 0.0f; rgb[3 * r + 1] = 0.0f; rgb[3 * r + 2] = 0.0f;
    opacity[r] = 0.0f;
    depth[r] = 0.0f;
}

// What frame_init_kernel (it = -1: the plan of iteration 0) and frame_schedule_kernel (the plan of iteration it + 1 from
// the survivor counts of iteration it) get; see make_next_plan, frame_loop.hip.
struct ScheduleArgs {
    IterPlan *plans;
    int it, n_frames, rays_per_frame, min_samples, max_samples;
    long long *host;
    long long seq;
    const int32_t *local_rays;      // device [n_frames] or NULL: rays of frame f that are real (the rest of its
                                    // rays_per_frame slots is padding and never alive)
    const int64_t *xcounts;         // device [(max_iters + 1) * n_frames] or NULL: survivors over all processes
    int64_t global_rays;            // N_rays of the whole image when sharded, else 0 (= rays_per_frame)
    long long *host_iter;           // pinned, or NULL: {alive here, done, seq} of EVERY plan, plan k at word 3k
};

// A bump allocator over a call's workspace: every array starts 256-byte aligned; `off` ends as the bytes taken (base may
// be NULL to size a workspace).
struct Carver {
    char *base;
    size_t off = 0;
    template <class T> T *take(size_t count)
    {
        T *p = (T *)(base + off);
        off = (off + count * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
};

// f(std::bool_constant<b>{}): a runtime flag as a template argument of what a generic lambda launches
template <class F> inline void with_bool(bool b, F f)
{
    if (b) f(std::true_type{}); else f(std::false_type{});
}

// The host's side of the loop, for one call.  A renderer's loop reads
//     L.begin(...);  for (; L.it < L.max_iters; ++L.it) { L.next(stop) -> break;  its own launches on L.plan(),
//     L.cur_list(), L.next_list() and grids sized from L.alive_bound;  L.schedule(stream); }  L.finish(...);
// sched.it and sched.seq are filled in per launch; the rest of `sched` is the call's.
struct FrameLoop {
    ScheduleArgs sched;             // plans, sizes, publish words (host: {alive, done, seq}) and the sharded call's extras
    int32_t *alive_a, *alive_b;     // the two alive lists, ping-pong
    int max_iters;
    const char *who;
    long long alive_bound = 0;      // rays alive in the iteration being enqueued: never more than this
    int it = 0;
    std::vector<long long> plan_seq = {};       // publication of plan k
    hipStream_t stream = nullptr;

    // the plan of iteration 0 (frame_init_kernel): every ray alive; lattice / stamps as that kernel takes them
    void begin(hipStream_t stream, float *lattice, unsigned long long *stamps, int n_stamps);
    // run-ahead control before iteration `it` is enqueued: `stop` when the loop is over, else alive_bound tightened
    int next(bool &stop);
    IterPlan *plan() const { return sched.plans + it; }
    const int32_t *cur_list() const { return it == 0 ? nullptr : ((it & 1) ? alive_a : alive_b); }     // NULL: all rays
    int32_t *next_list() const { return (it & 1) ? alive_b : alive_a; }
    // takes the sequence number of plan it + 1 and launches frame_schedule_kernel, which publishes it
    void schedule(hipStream_t stream);
    // the plans of the enqueued iterations in one copy (the call blocks here, once); n_iters: the iterations that ran
    int finish(hipStream_t stream, const char *what, std::vector<IterPlan> &plans, int &n_iters);
};

}  // namespace ced
