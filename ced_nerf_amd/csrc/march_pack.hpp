// Ray-packed samples without a count pass: a lane walks its ray once remembering the samples as runs in registers, the
// workgroup reserves ONE contiguous range of the sample array (wave prefix sums + a single returning atomic: the samples
// stay ray-packed and dense, no scan, no staging) and every lane regenerates its samples there.  Used by the frame
// loop's marching kernel (frame.hip) and the one-pass form of the one-shot march (march_all.hip).
#pragma once
#include "frame_loop.hpp"
#include "march_accel.hpp"

namespace ced {

constexpr int kMaxRuns = 4;        // runs of consecutive samples a ray's walk is remembered by (more: the ray walks twice)

// A ray's walk remembered as (first t, length) of up to kMaxRuns runs of consecutive samples, in registers: within a
// run t_start[j+1] == t_end[j] and t_end[j] = t_start[j] + dt(t_start[j]), so replay() regenerates the same floats.
struct SampleRuns {
    float t[kMaxRuns] = {};
    int n[kMaxRuns] = {};
    int count = 0;
    float prev_end = 0.0f;

    __device__ __forceinline__ void record(int i, float t0, float t1)
    {
        const bool fresh = i == 0 || t0 != prev_end;
        if (fresh) ++count;
        prev_end = t1;
        // run slots as a chain of selects (t / n stay in registers)
#pragma unroll
        for (int k = 0; k < kMaxRuns; ++k) {
            const bool here = count == k + 1;
            t[k] = (here && fresh) ? t0 : t[k];
            n[k] += here ? 1 : 0;
        }
    }
    // false: more runs than fit (alternating single occupied cells) or a walk without a step size -- walk again instead
    __device__ __forceinline__ bool replayable(const GridSpec &grid) const { return count <= kMaxRuns && grid.step_size > 0.0f; }
    // store(i, t0, t1) for every sample, in the walk's order
    template <class Store>
    __device__ __forceinline__ void replay(const GridSpec &grid, Store store) const
    {
        int pos = 0;
#pragma unroll
        for (int k = 0; k < kMaxRuns; ++k) {
            float ts = t[k];
            for (int j = 0; j < n[k]; ++j) {
                const float te = ts + calc_dt(ts, grid.cone_angle, grid.step_size, 1e10f);
                store(pos++, ts, te);
                ts = te;
            }
        }
    }
};

// Record -> reserve -> replay or walk again, for one lane; every lane of the workgroup (kWaves waves) calls it (the two
// barriers of workgroup_reserve).  What differs between the callers comes in as callables:
//   walk(first, emit) -> n    the ray's walk, emit(i, t0, t1) per sample.  first (std::true_type): the walk that is
//                             recorded -- the site loads its ray before it and keeps what it wants of the walk's end;
//                             std::false_type: the same walk again, storing directly (runs that are not replayable)
//   reserve(total) -> first   thread 0: the site's one atomic on its sample counter
//   place(start, n) -> bool   active lanes: the lane's range is known (packed_info; where store() will write);
//                             false: store nothing (no samples, or none that fit)
//   store(i, t0, t1)          sample i of the lane
template <int kWaves, class Walk, class Reserve, class Place, class Store>
__device__ __forceinline__ void pack_ray_samples(bool active, const GridSpec &grid, Walk walk, Reserve reserve, Place place,
                                                 Store store)
{
    SampleRuns runs;
    int n = 0;
    if (active) n = walk(std::true_type{}, [&](int i, float t0, float t1) { runs.record(i, t0, t1); });
    CED_DIAG_TICK(6);
    const int64_t start = workgroup_reserve<kWaves>(n, reserve);
    if (!active || !place(start, n)) return;
    if (n > 0 && !runs.replayable(grid)) (void)walk(std::false_type{}, store);
    else runs.replay(grid, store);
}

}  // namespace ced
