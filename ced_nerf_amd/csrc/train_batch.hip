// The training batch in one launch: view / pixel draws, the pixel's ray, its colour and its timestamp, for every ray of
// a step.  Replaces the per-step data fetch of the reference's datasets:
//   D-NeRF   : datasets/dnerf_synthetic.py:142-242 (fetch_data + preprocess, batch_over_images=True): a view per ray,
//              RGBA / 255 composited on the batch's background;
//   HyperNeRF: datasets/hypernerf.py:443-541: one view per batch, RGB / 255, rays by Camera.pixels_to_rays at the pixel
//              centre (a host-side numpy Newton undistortion there, uploaded every step).
// Rays come from the per-pixel bodies that the full-frame kernels use (camera_models.hpp): the same bits for the same
// pixel.  The random numbers are a pure function of (seed, step, ray, draw) ("Training batches"):
//   key        = h(h(h(h(seed_lo ^ 0x243f6a88) ^ seed_hi) ^ step_lo) ^ step_hi)
//   draw(r, k) = h(h(h(key ^ r_lo) ^ r_hi) ^ (0x9e3779b9 * (k + 1)))             (32-bit wrap-around arithmetic)
// with h the "lowbias32" integer hash.  Per ray r: k = 0 view (per-ray mode), 1 x, 2 y.  The batch's own draws use
// r = 2^64 - 1: k = 0 the view (one-per-step mode), k = 1..3 the random background.  An integer in [0, n) is
// (u * n) >> 32 (64-bit product), a float in [0, 1) is (u >> 8) * 2^-24.
#include "ced_common.hpp"
#include "camera_models.hpp"

namespace ced {

__host__ __device__ __forceinline__ uint32_t lowbias32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__host__ __device__ __forceinline__ uint32_t batch_key(uint64_t seed, uint64_t step)
{
    uint32_t h = lowbias32((uint32_t)seed ^ 0x243f6a88u);
    h = lowbias32(h ^ (uint32_t)(seed >> 32));
    h = lowbias32(h ^ (uint32_t)step);
    return lowbias32(h ^ (uint32_t)(step >> 32));
}

__host__ __device__ __forceinline__ uint32_t batch_draw(uint32_t key, uint64_t ray, uint32_t k)
{
    const uint32_t h = lowbias32(lowbias32(key ^ (uint32_t)ray) ^ (uint32_t)(ray >> 32));
    return lowbias32(h ^ (0x9e3779b9u * (k + 1u)));
}

__host__ __device__ __forceinline__ int32_t draw_below(uint32_t u, int32_t n)
{
    return (int32_t)(((uint64_t)u * (uint64_t)(uint32_t)n) >> 32);
}

__host__ __device__ __forceinline__ float draw_unit(uint32_t u) { return (float)(u >> 8) * 5.9604644775390625e-8f; }

struct BatchArgs {
    int64_t n;
    int32_t model, n_views, width, height, channels, per_ray, view0;
    uint32_t key;
    float bkgd[3];
    const uint8_t *images;
    const float *cameras, *view_ts;
    float *origins, *viewdirs, *pixels, *timestamps, *color_bkgd;
    int32_t *indices;
};

__global__ __launch_bounds__(256) void training_batch_kernel(BatchArgs A)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    if (i == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) A.color_bkgd[c] = A.bkgd[c];
    }
    const int32_t v = A.per_ray ? draw_below(batch_draw(A.key, (uint64_t)i, 0u), A.n_views) : A.view0;
    const int32_t x = draw_below(batch_draw(A.key, (uint64_t)i, 1u), A.width);
    const int32_t y = draw_below(batch_draw(A.key, (uint64_t)i, 2u), A.height);
    float o[3], d[3];
    if (A.model == CED_CAMERA_PINHOLE) {
        const float *p = A.cameras + (int64_t)v * CED_PINHOLE_FLOATS;
        PinholeCam C;
        C.fx = p[0]; C.fy = p[1]; C.cx = p[2]; C.cy = p[3];
#pragma unroll
        for (int k = 0; k < 12; ++k) C.c2w[k] = p[4 + k];
        C.sign = p[16];
        float unnormalised[3];
        pinhole_pixel_ray(C, (float)x, (float)y, o, d, unnormalised);
    } else {
        const float *p = A.cameras + (int64_t)v * CED_HYPERCAM_FLOATS;
        HyperCam C;
#pragma unroll
        for (int k = 0; k < 9; ++k) C.orientation[k] = p[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) C.position[k] = p[9 + k];
        C.focal = p[12]; C.ppx = p[13]; C.ppy = p[14]; C.skew = p[15]; C.aspect = p[16];
        C.k1 = p[17]; C.k2 = p[18]; C.k3 = p[19]; C.p1 = p[20]; C.p2 = p[21];
        C.distorted = hypercam_is_distorted(C.k1, C.k2, C.k3, C.p1, C.p2);
        hypercam_pixel_ray(C, (float)x + 0.5f, (float)y + 0.5f, o, d);      // hypernerf.py:514-521
    }
    const uint8_t *px = A.images + (((int64_t)v * A.height + y) * A.width + x) * A.channels;
    float rgb[3];
    if (A.channels == 4) {                     // dnerf_synthetic.py:145-158: rgba / 255, then rgb * a + bkgd * (1 - a)
        const float a = (float)px[3] / 255.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] = ((float)px[c] / 255.0f) * a + A.bkgd[c] * (1.0f - a);
    } else {                                   // hypernerf.py:490
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] = (float)px[c] / 255.0f;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        A.origins[3 * i + c] = o[c];
        A.viewdirs[3 * i + c] = d[c];
        A.pixels[3 * i + c] = rgb[c];
    }
    A.timestamps[i] = A.view_ts[v];
    if (A.indices) {
        A.indices[3 * i] = v;
        A.indices[3 * i + 1] = x;
        A.indices[3 * i + 2] = y;
    }
}

}  // namespace ced

extern "C" int ced_sample_training_batch(int32_t camera_model, int32_t n_views, int32_t width, int32_t height,
                                         int32_t channels, const uint8_t *images, const float *cameras,
                                         const float *view_timestamps, int64_t num_rays, uint64_t seed, int64_t step,
                                         int32_t view_mode, int32_t bkgd_mode, float *origins, float *viewdirs,
                                         float *pixels, float *timestamps, float *color_bkgd, int32_t *indices,
                                         void *stream)
{
    CED_REQUIRE(camera_model == CED_CAMERA_PINHOLE || camera_model == CED_CAMERA_HYPERCAM,
                "sample_training_batch: unknown camera model %d", camera_model);
    CED_REQUIRE(n_views > 0 && width > 0 && height > 0, "sample_training_batch: bad view count or image size");
    CED_REQUIRE(channels == 3 || channels == 4, "sample_training_batch: channels must be 3 (RGB) or 4 (RGBA), got %d",
                channels);
    CED_REQUIRE(num_rays >= 1 && (num_rays + 255) / 256 <= 0x7fffffff, "sample_training_batch: bad ray count %lld",
                (long long)num_rays);
    CED_REQUIRE(view_mode == CED_VIEW_PER_RAY || view_mode == CED_VIEW_PER_STEP, "sample_training_batch: bad view mode %d",
                view_mode);
    CED_REQUIRE(bkgd_mode == CED_BKGD_WHITE || bkgd_mode == CED_BKGD_BLACK || bkgd_mode == CED_BKGD_RANDOM,
                "sample_training_batch: bad background mode %d", bkgd_mode);
    CED_REQUIRE(images && cameras && view_timestamps && origins && viewdirs && pixels && timestamps && color_bkgd,
                "sample_training_batch: null pointer");
    ced::BatchArgs A{};
    A.n = num_rays;
    A.model = camera_model; A.n_views = n_views; A.width = width; A.height = height; A.channels = channels;
    A.per_ray = view_mode == CED_VIEW_PER_RAY ? 1 : 0;
    // the batch's own draws (ray 2^64 - 1) are pure functions of (seed, step): made here, no device round trip
    A.key = ced::batch_key(seed, (uint64_t)step);
    const uint64_t batch_ray = ~(uint64_t)0;
    A.view0 = ced::draw_below(ced::batch_draw(A.key, batch_ray, 0u), n_views);
    for (int c = 0; c < 3; ++c)
        A.bkgd[c] = bkgd_mode == CED_BKGD_WHITE ? 1.0f : bkgd_mode == CED_BKGD_BLACK ? 0.0f
                  : ced::draw_unit(ced::batch_draw(A.key, batch_ray, 1u + (uint32_t)c));
    A.images = images; A.cameras = cameras; A.view_ts = view_timestamps;
    A.origins = origins; A.viewdirs = viewdirs; A.pixels = pixels; A.timestamps = timestamps; A.color_bkgd = color_bkgd;
    A.indices = indices;
    hipLaunchKernelGGL(ced::training_batch_kernel, dim3((unsigned)((num_rays + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, A);
    return ced::check_launch("sample_training_batch");
}
