// The first sample of each ray at which the density reaches a threshold, and the bracket that holds the crossing:
// ced_surface_first_crossing (include/cednerf_hip.h states the definition).  What utils.render_surface runs between the
// density of every marched sample and the bisection on the field (field_level_set.hip): the bracket's upper end is the
// crossing sample's midpoint, its lower end the midpoint of the sample before it where the two touch, else the crossing
// sample's own start.
// One lane owns one ray and walks its samples in order through composite_core.hpp's walk_samples, as the compositing
// kernels do; a ray's outputs are written by its lane alone (no atomics).  Streams 12 B per sample.
#include "ced_common.hpp"
#include "composite_core.hpp"

namespace ced {

__global__ __launch_bounds__(256) void first_crossing_kernel(int64_t n_rays, const int64_t *__restrict__ packed,
                                                             const float *__restrict__ t0, const float *__restrict__ t1,
                                                             const float *__restrict__ sig, float thresh,
                                                             int64_t *__restrict__ k_out, float *__restrict__ lo_out,
                                                             float *__restrict__ hi_out)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rays) return;
    const int64_t s0 = packed[2 * r], cnt = packed[2 * r + 1];
    int64_t k = -1;
    float lo = 0.0f, hi = 0.0f;
    float prev_end = 0.0f, prev_mid = 0.0f;
    bool have_prev = false;
    walk_samples<4, false>(s0, s0 + (cnt > 0 ? cnt : 0), t0, t1, sig, nullptr,
                           [&](float ts, float te, float sg, float, float, float, int64_t i) __attribute__((always_inline)) {
                               if (k >= 0) return;                      // the first crossing stands
                               const float mid = (ts + te) / 2.0f;
                               if (sg >= thresh) {                      // false for a NaN
                                   k = i;
                                   hi = mid;
                                   lo = (have_prev && prev_end == ts) ? prev_mid : ts;
                               }
                               prev_end = te;
                               prev_mid = mid;
                               have_prev = true;
                           });
    if (k_out) k_out[r] = k;
    if (lo_out) lo_out[r] = lo;
    if (hi_out) hi_out[r] = hi;
}

}  // namespace ced

extern "C" int ced_surface_first_crossing(int64_t n_rays, const int64_t *packed_info, const float *t_starts,
                                          const float *t_ends, const float *sigmas, float thresh, int64_t *k, float *lo,
                                          float *hi, void *stream)
{
    CED_REQUIRE(n_rays >= 0, "surface_first_crossing: n_rays < 0");
    if (n_rays == 0) return CED_OK;
    CED_REQUIRE(packed_info && k && lo && hi, "surface_first_crossing: null pointer");
    CED_REQUIRE(!(thresh != thresh), "surface_first_crossing: thresh is a NaN");
    CED_REQUIRE(n_rays <= (int64_t)INT32_MAX * 256, "surface_first_crossing: n_rays=%lld too large", (long long)n_rays);
    hipLaunchKernelGGL(ced::first_crossing_kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_rays,
                       packed_info, t_starts, t_ends, sigmas, thresh, k, lo, hi);
    return ced::check_launch("surface_first_crossing");
}
