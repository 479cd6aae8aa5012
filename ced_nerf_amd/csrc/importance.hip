// DyNeRF's importance-sampling weight maps on the device (datasets/dnerf_3d_video_IS.py:13-76, 187): the per-camera
// temporal median, the ISG weights (squared difference from the median through a Geman-McClure kernel) and the IST
// weights (largest change against the frames up to frame_shift away).  Images are the uint8 [C, T, H, W, 3] of
// trainset.TrainViews, camera-major.  Pure streaming kernels: a thread per output element, consecutive threads on
// consecutive bytes of a frame, no atomics, no LDS, no scratch.  ced_nerf_amd/importance.py restates the three formulas
// on the CPU and the tests compare every bit.
#include "ced_common.hpp"

namespace ced {

// Median over T of one (pixel, channel) of one camera, torch.median's rule: the element of rank (T - 1) / 2 of the
// sorted values (the lower middle for even T).  Bisection on the byte value: the median is the smallest v with
// #(values <= v) > rank; eight passes over T, each a coalesced read of one byte per thread per frame.
__global__ __launch_bounds__(256) void temporal_median_kernel(int64_t n_frames, int64_t frame_bytes, int64_t total,
                                                              const uint8_t *__restrict__ images,
                                                              uint8_t *__restrict__ median)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;       // camera * frame_bytes + element
    if (i >= total) return;
    const int64_t cam = i / frame_bytes, e = i - cam * frame_bytes;
    const uint8_t *p = images + cam * n_frames * frame_bytes + e;
    const int32_t rank = (int32_t)((n_frames - 1) / 2);
    int32_t lo = 0, hi = 255;
#pragma unroll 1
    for (int step = 0; step < 8; ++step) {
        const int32_t mid = (lo + hi) >> 1;
        int32_t below = 0;
#pragma unroll 4
        for (int64_t t = 0; t < n_frames; ++t) below += (int32_t)p[t * frame_bytes] <= mid ? 1 : 0;
        if (below > rank) hi = mid; else lo = mid + 1;
    }
    median[i] = (uint8_t)lo;
}

// dynerf_isg_weight in its order of roundings: a = u8 / 255, m = med / 255, d = a - m, q = d * d, p = q / (q + gamma^2),
// (p0 + p1 + p2) * (1/3).
__global__ __launch_bounds__(256) void isg_weights_kernel(int64_t n_frames, int64_t frame_pixels, int64_t total,
                                                          const uint8_t *__restrict__ images,
                                                          const uint8_t *__restrict__ median, float gamma2,
                                                          float *__restrict__ weights)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;       // (camera * T + t) * frame_pixels + pixel
    if (i >= total) return;
    const int64_t frame = i / frame_pixels, pix = i - frame * frame_pixels;
    const int64_t cam = frame / n_frames;
    const uint8_t *a8 = images + 3 * i, *m8 = median + 3 * (cam * frame_pixels + pix);
    float p[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = (float)a8[c] / 255.0f, m = (float)m8[c] / 255.0f;
        const float d = a - m;
        const float q = d * d;
        p[c] = q / (q + gamma2);
    }
    weights[i] = ((p[0] + p[1]) + p[2]) * 0.3333333432674407958984375f;
}

// dynerf_ist_weight_nice: per channel the largest |f[t +- s] - f[t]| over s = 1..frame_shift, a neighbour outside the
// clip being a zero frame; then (m0 + m1 + m2) / 3 and max(., alpha).  The values are the integers 0..255, so the
// largest absolute difference is max(window max - f[t], f[t] - window min) exactly, the window running over the
// neighbours and, where the clip ends inside it, a zero.
__global__ __launch_bounds__(256) void ist_weights_kernel(int64_t n_frames, int64_t frame_pixels, int64_t total,
                                                          const uint8_t *__restrict__ images, float alpha,
                                                          int32_t frame_shift, float *__restrict__ weights)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;       // (camera * T + t) * frame_pixels + pixel
    if (i >= total) return;
    const int64_t frame = i / frame_pixels;
    const int64_t t = frame % n_frames;
    const uint8_t *p = images + 3 * i;
    const int64_t stride = 3 * frame_pixels;
    int32_t v[3], lo[3], hi[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = lo[c] = hi[c] = (int32_t)p[c];
    const int64_t first = t - frame_shift > 0 ? t - frame_shift : 0;
    const int64_t last = t + frame_shift < n_frames - 1 ? t + frame_shift : n_frames - 1;
    if (frame_shift > 0 && (t - frame_shift < 0 || t + frame_shift > n_frames - 1)) {
#pragma unroll
        for (int c = 0; c < 3; ++c) lo[c] = 0;                               // a zero frame is among the neighbours
    }
#pragma unroll 2
    for (int64_t u = first; u <= last; ++u) {
        const uint8_t *q = p + (u - t) * stride;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int32_t w = (int32_t)q[c];
            lo[c] = w < lo[c] ? w : lo[c];
            hi[c] = w > hi[c] ? w : hi[c];
        }
    }
    float m[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int32_t up = hi[c] - v[c], down = v[c] - lo[c];
        m[c] = (float)(up > down ? up : down);
    }
    const float mean = ((m[0] + m[1]) + m[2]) / 3.0f;
    weights[i] = mean > alpha ? mean : alpha;
}

// Every launch is one thread per output element in workgroups of 256: frames * pixels (* 3 bytes for the median, whose
// frames are the cameras) stays below 2^38, so the grid stays below 2^30 workgroups.
static int check_clip(const char *what, int32_t n_cameras, int32_t n_frames, int32_t height, int32_t width,
                      int64_t elements_per_pixel = 1)
{
    CED_REQUIRE(n_cameras > 0 && n_frames > 0 && height > 0 && width > 0, "%s: bad clip shape [%d, %d, %d, %d, 3]", what,
                n_cameras, n_frames, height, width);
    const int64_t frames = (int64_t)n_cameras * n_frames, pixels = (int64_t)height * width;
    CED_REQUIRE(pixels <= ((int64_t)1 << 38) / frames / elements_per_pixel, "%s: clip too large", what);
    return CED_OK;
}

}  // namespace ced

extern "C" int ced_temporal_median_u8(int32_t n_cameras, int32_t n_frames, int32_t height, int32_t width,
                                      const uint8_t *images, uint8_t *median, void *stream)
{
    if (int rc = ced::check_clip("temporal_median_u8", n_cameras, n_frames, height, width, 3)) return rc;
    CED_REQUIRE(images && median, "temporal_median_u8: null pointer");
    const int64_t frame_bytes = (int64_t)height * width * 3, total = frame_bytes * n_cameras;
    hipLaunchKernelGGL(ced::temporal_median_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, (int64_t)n_frames, frame_bytes, total, images, median);
    return ced::check_launch("temporal_median_u8");
}

extern "C" int ced_isg_weights(int32_t n_cameras, int32_t n_frames, int32_t height, int32_t width,
                               const uint8_t *images, const uint8_t *median, float gamma, float *weights, void *stream)
{
    if (int rc = ced::check_clip("isg_weights", n_cameras, n_frames, height, width)) return rc;
    CED_REQUIRE(images && median && weights, "isg_weights: null pointer");
    CED_REQUIRE(gamma == gamma, "isg_weights: gamma is not a number");
    const int64_t frame_pixels = (int64_t)height * width, total = frame_pixels * n_cameras * n_frames;
    hipLaunchKernelGGL(ced::isg_weights_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (int64_t)n_frames, frame_pixels, total, images, median, gamma * gamma, weights);
    return ced::check_launch("isg_weights");
}

extern "C" int ced_ist_weights(int32_t n_cameras, int32_t n_frames, int32_t height, int32_t width,
                               const uint8_t *images, float alpha, int32_t frame_shift, float *weights, void *stream)
{
    if (int rc = ced::check_clip("ist_weights", n_cameras, n_frames, height, width)) return rc;
    CED_REQUIRE(images && weights, "ist_weights: null pointer");
    CED_REQUIRE(frame_shift >= 0, "ist_weights: frame_shift must be >= 0, got %d", frame_shift);
    CED_REQUIRE(alpha == alpha, "ist_weights: alpha is not a number");
    const int64_t frame_pixels = (int64_t)height * width, total = frame_pixels * n_cameras * n_frames;
    hipLaunchKernelGGL(ced::ist_weights_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (int64_t)n_frames, frame_pixels, total, images, alpha, frame_shift, weights);
    return ced::check_launch("ist_weights");
}
