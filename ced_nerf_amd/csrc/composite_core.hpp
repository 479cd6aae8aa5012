// The front-to-back compositing recurrence, once, for every kernel that walks a ray's samples: composite.hip (the
// nerfacc-shaped entries), frame.hip (frame renderer), image.hip (eval renderer) and losses.hip (the fused distortion loss).
// Per sample, in this order and each a single float32 operation (-ffp-contract=off; det_expf is ced_common.hpp's):
//   sd = sigma * (t1 - t0);  a = 1 - exp(-sd);  T = exp(-acc) [* the ray's prefix];  w = T * a;
//   c += w * rgb;  op += w;  dp += w * ((t0 + t1) / 2);  acc += sd.
// The kernels' contract is that they all give the same bits as the C oracle: do not "simplify" the arithmetic.
#pragma once
#include <cfloat>

#include "ced_common.hpp"

namespace ced {

__device__ __forceinline__ float alpha_of(float sd) { return 1.0f - det_expf(-sd); }
__device__ __forceinline__ float trans_of(float acc) { return det_expf(-acc); }

// One sample in front of which the transmittance is T.  The caller says what T is: trans_of(acc), that times the ray's
// prefix (ONE multiply, composite_ray), or the value a forward sweep stored (the backward sweeps).
struct Sample {
    float sd, a, T, w;
};
__device__ __forceinline__ Sample sample_step(float sg, float ts, float te, float T)
{
    Sample s;
    s.sd = sg * (te - ts);
    s.a = alpha_of(s.sd);
    s.T = T;
    s.w = T * s.a;
    return s;
}

// nerfacc render_visibility_from_density: exp(-sum so far) >= early_stop_eps, and alpha >= alpha_thre where there is a
// threshold (a NaN alpha fails it)
__device__ __forceinline__ bool visible(float T, float a, float eps, float alpha_thre)
{
    return T >= eps && !(alpha_thre > 0.0f && !(a >= alpha_thre));
}

// cednerf/utils.py:301-303: a ray goes on to the next iteration while it is not opaque and used its whole sample budget
__device__ __forceinline__ bool survives(float op, int64_t cnt, int64_t limit, float opc_thres)
{
    return op <= opc_thres && cnt == limit;
}

// The three per-ray sums of cednerf/render.py:158-169, carried in the ray's pixel between iterations.
struct RaySums {
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, op = 0.0f, dp = 0.0f;
    __device__ __forceinline__ void load(const float *rgb, const float *opacity, const float *depth, int64_t r)
    {
        c0 = rgb[3 * r]; c1 = rgb[3 * r + 1]; c2 = rgb[3 * r + 2];
        op = opacity[r];
        dp = depth[r];
    }
    __device__ __forceinline__ void store(float *rgb, float *opacity, float *depth, int64_t r) const
    {
        rgb[3 * r] = c0; rgb[3 * r + 1] = c1; rgb[3 * r + 2] = c2;
        opacity[r] = op;
        depth[r] = dp;
    }
    __device__ __forceinline__ void add(float w, float r, float g, float b, float ts, float te)
    {
        c0 = c0 + w * r;
        c1 = c1 + w * g;
        c2 = c2 + w * b;
        op = op + w;
        dp = dp + w * ((ts + te) / 2.0f);
    }
};

// cednerf/utils.py:309-314: background behind what is left of the ray, depth normalised by the opacity
__device__ __forceinline__ void finalize_pixel(int64_t r, const float *__restrict__ bkgd, float *__restrict__ rgb,
                                               const float *__restrict__ opacity, float *__restrict__ depth)
{
    const float op = opacity[r];
    if (bkgd) {
        const float rem = 1.0f - op;
        rgb[3 * r] = rgb[3 * r] + bkgd[0] * rem;
        rgb[3 * r + 1] = rgb[3 * r + 1] + bkgd[1] * rem;
        rgb[3 * r + 2] = rgb[3 * r + 2] + bkgd[2] * rem;
    }
    depth[r] = depth[r] / __builtin_fmaxf(op, FLT_EPSILON);
}

// THE loop over samples [begin, end) of one ray: body(ts, te, sigma, r, g, b, i) is called strictly in sample order (the
// per-ray sums are sequential by contract), but the loads of kU samples are issued before the first of them is
// consumed, so one memory round trip feeds kU samples.  What is left after the full batches goes one sample at a time.
// RGB = false: no colour loads (body gets zeros).  body is a force-inlined callable; it may store, but not to these arrays.
template <int kN, bool RGB, class Body>
__device__ __forceinline__ void walk_batch(int64_t i, const float *__restrict__ t0, const float *__restrict__ t1,
                                           const float *__restrict__ sig, const float *__restrict__ rgbs, Body &body)
{
    float ts[kN], te[kN], sg[kN], cr[kN], cg[kN], cb[kN];
#pragma unroll
    for (int u = 0; u < kN; ++u) {
        ts[u] = t0[i + u]; te[u] = t1[i + u]; sg[u] = sig[i + u];
        if constexpr (RGB) { cr[u] = rgbs[3 * (i + u)]; cg[u] = rgbs[3 * (i + u) + 1]; cb[u] = rgbs[3 * (i + u) + 2]; }
        else { cr[u] = 0.0f; cg[u] = 0.0f; cb[u] = 0.0f; }
    }
#pragma unroll
    for (int u = 0; u < kN; ++u) body(ts[u], te[u], sg[u], cr[u], cg[u], cb[u], i + u);
}

template <int kU, bool RGB, class Body>
__device__ __forceinline__ void walk_samples(int64_t begin, int64_t end, const float *__restrict__ t0,
                                             const float *__restrict__ t1, const float *__restrict__ sig,
                                             const float *__restrict__ rgbs, Body body)
{
    int64_t i = begin;
    for (; i + kU <= end; i += kU) walk_batch<kU, RGB>(i, t0, t1, sig, rgbs, body);
    for (; i < end; ++i) walk_batch<1, RGB>(i, t0, t1, sig, rgbs, body);
}

// composite_prefix (cednerf/utils.py:274-299) for one ray: weights with prefix_trans = 1 - opacity[ray], then the three
// sums, same operation order as the unfused sequence.  Returns the ray's opacity afterwards.
__device__ __forceinline__ float composite_ray(int64_t r, int64_t begin, int64_t cnt, const float *__restrict__ t0,
                                               const float *__restrict__ t1, const float *__restrict__ sig,
                                               const float *__restrict__ rgbs, float *__restrict__ rgb,
                                               float *__restrict__ opacity, float *__restrict__ depth)
{
    if (cnt <= 0) return opacity[r];
    RaySums sums;
    sums.load(rgb, opacity, depth, r);
    const float prefix = 1.0f - sums.op;
    float acc = 0.0f;
    walk_samples<4, true>(begin, begin + cnt, t0, t1, sig, rgbs,
                          [&](float ts, float te, float sg, float cr, float cg, float cb, int64_t) __attribute__((always_inline)) {
                              const Sample s = sample_step(sg, ts, te, trans_of(acc) * prefix);
                              sums.add(s.w, cr, cg, cb, ts, te);
                              acc = acc + s.sd;
                          });
    sums.store(rgb, opacity, depth, r);
    return sums.op;
}

}  // namespace ced
