// The per-pixel bodies of the two camera models, shared by the full-frame ray kernels
// (raygen.hip) and the training-batch sampler (train_batch.hip), so that a pixel's ray is the same code, hence the
// same bits, on both paths.
//   pinhole  : datasets/dnerf_synthetic.py:191-221 and gui.py:43-86 (OpenGL or OpenCV convention);
//   hypercam : datasets/hyper_cam.py:210-252 (Camera.pixels_to_rays at a pixel centre), including the 10-step Newton
//              undistortion of :22-91.
// float32 throughout, operations in the reference's order (the build's -ffp-contract=off keeps every rounding).
#pragma once
#include <hip/hip_runtime.h>

namespace ced {

struct PinholeCam {
    float fx, fy, cx, cy;
    float c2w[12];          // row-major [3][4]
    float sign;             // -1 OpenGL (y up, looking down -z), +1 OpenCV
};

// Pixel (x, y) (integer coordinates): origin, unit view direction and the unnormalised direction.
__device__ __forceinline__ void pinhole_pixel_ray(const PinholeCam &C, float x, float y, float o[3], float v[3], float d[3])
{
    const float cam[3] = { (x - C.cx + 0.5f) / C.fx, ((y - C.cy + 0.5f) / C.fy) * C.sign, C.sign };
#pragma unroll
    for (int r = 0; r < 3; ++r) d[r] = (cam[0] * C.c2w[4 * r] + cam[1] * C.c2w[4 * r + 1]) + cam[2] * C.c2w[4 * r + 2];
    const float nrm = __builtin_sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        o[r] = C.c2w[4 * r + 3];
        v[r] = d[r] / nrm;
    }
}

struct HyperCam {
    float orientation[9];   // row-major world->camera rotation
    float position[3];
    float focal, ppx, ppy, skew, aspect;
    float k1, k2, k3, p1, p2;
    int distorted;          // 0: no distortion coefficient is set, the Newton steps are skipped
};

// The point (px, py) in pixel units (the centre of pixel (x, y) is (x + 0.5, y + 0.5)): origin and unit direction.
__device__ __forceinline__ void hypercam_pixel_ray(const HyperCam &A, float px, float py, float o[3], float v[3])
{
    float y = (py - A.ppy) / (A.focal * A.aspect);
    float x = (px - A.ppx - y * A.skew) / A.focal;
    if (A.distorted) {
        const float xd = x, yd = y;
        for (int it = 0; it < 10; ++it) {
            const float r = x * x + y * y;
            const float d = 1.0f + r * (A.k1 + r * (A.k2 + A.k3 * r));
            const float fx = d * x + 2.0f * A.p1 * x * y + A.p2 * (r + 2.0f * x * x) - xd;
            const float fy = d * y + 2.0f * A.p2 * x * y + A.p1 * (r + 2.0f * y * y) - yd;
            const float d_r = A.k1 + r * (2.0f * A.k2 + 3.0f * A.k3 * r);
            const float d_x = 2.0f * x * d_r, d_y = 2.0f * y * d_r;
            const float fx_x = d + d_x * x + 2.0f * A.p1 * y + 6.0f * A.p2 * x;
            const float fx_y = d_y * x + 2.0f * A.p1 * x + 2.0f * A.p2 * y;
            const float fy_x = d_x * y + 2.0f * A.p2 * y + 2.0f * A.p1 * x;
            const float fy_y = d + d_y * y + 2.0f * A.p2 * x + 6.0f * A.p1 * y;
            const float den = fy_x * fx_y - fx_x * fy_y;
            const float xn = fx * fy_y - fy * fx_y, yn = fy * fx_x - fx * fy_x;
            const bool ok = __builtin_fabsf(den) > 1e-9f;
            x = x + (ok ? xn / den : 0.0f);
            y = y + (ok ? yn / den : 0.0f);
        }
    }
    float l[3] = { x, y, 1.0f };
    const float ln = __builtin_sqrtf((l[0] * l[0] + l[1] * l[1]) + l[2] * l[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) l[r] = l[r] / ln;
    float w[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)      // orientation^T @ local
        w[r] = (A.orientation[r] * l[0] + A.orientation[3 + r] * l[1]) + A.orientation[6 + r] * l[2];
    const float wn = __builtin_sqrtf((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        o[r] = A.position[r];
        v[r] = w[r] / wn;          // rays_dir (hyper_cam.py:249); already unit, so viewdirs = rays_dir / |rays_dir|
    }
}

__host__ __device__ __forceinline__ int hypercam_is_distorted(float k1, float k2, float k3, float p1, float p2)
{
    return (k1 != 0.0f || k2 != 0.0f || k3 != 0.0f || p1 != 0.0f || p2 != 0.0f) ? 1 : 0;
}

}  // namespace ced
