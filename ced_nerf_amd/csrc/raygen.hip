// On-device ray generation for full frames: the camera models whose rays the
// reference builds on the host and uploads every frame (15 MB at 800x800).
//   pinhole  : datasets/dnerf_synthetic.py:191-221 and gui.py:43-86 (OpenGL or OpenCV convention);
//   hypercam : datasets/hyper_cam.py:210-252 (Camera.pixels_to_rays on get_pixel_centers(), :299-303),
//              including the 10-step Newton undistortion of :22-91, as used at datasets/hypernerf.py:172-173.
// float32 throughout, operations in the reference's order.  The per-pixel bodies live in camera_models.hpp, shared with
// the training-batch sampler (train_batch.hip).
#include "ced_common.hpp"
#include "camera_models.hpp"

namespace ced {

struct PinholeArgs {
    int width, height;
    PinholeCam cam;
    float *origins, *viewdirs, *directions;   // [H*W,3]; directions may be NULL
};

__global__ __launch_bounds__(256) void pinhole_rays_kernel(PinholeArgs A)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)A.width * A.height) return;
    float o[3], v[3], d[3];
    pinhole_pixel_ray(A.cam, (float)(i % A.width), (float)(i / A.width), o, v, d);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        A.origins[3 * i + r] = o[r];
        A.viewdirs[3 * i + r] = v[r];
        if (A.directions) A.directions[3 * i + r] = d[r];
    }
}

struct HyperCamArgs {
    int width, height;
    HyperCam cam;
    float *origins, *viewdirs;
};

__global__ __launch_bounds__(256) void hypercam_rays_kernel(HyperCamArgs A)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)A.width * A.height) return;
    float o[3], v[3];
    hypercam_pixel_ray(A.cam, (float)(i % A.width) + 0.5f, (float)(i / A.width) + 0.5f, o, v);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        A.origins[3 * i + r] = o[r];
        A.viewdirs[3 * i + r] = v[r];
    }
}

}  // namespace ced

extern "C" int ced_generate_rays_pinhole(int32_t width, int32_t height, float fx, float fy, float cx, float cy,
                                         const float *c2w_host, int32_t opengl, float *origins, float *viewdirs,
                                         float *directions, void *stream)
{
    CED_REQUIRE(width > 0 && height > 0, "generate_rays_pinhole: bad image size");
    CED_REQUIRE(c2w_host && origins && viewdirs, "generate_rays_pinhole: null pointer");
    ced::PinholeArgs A{};
    A.width = width; A.height = height; A.cam.fx = fx; A.cam.fy = fy; A.cam.cx = cx; A.cam.cy = cy;
    for (int i = 0; i < 12; ++i) A.cam.c2w[i] = c2w_host[i];
    A.cam.sign = opengl ? -1.0f : 1.0f;
    A.origins = origins; A.viewdirs = viewdirs; A.directions = directions;
    const int64_t n = (int64_t)width * height;
    hipLaunchKernelGGL(ced::pinhole_rays_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A);
    return ced::check_launch("generate_rays_pinhole");
}

extern "C" int ced_generate_rays_hypercam(int32_t width, int32_t height, const float *orientation_host,
                                          const float *position_host, float focal_length, float principal_x,
                                          float principal_y, float skew, float pixel_aspect_ratio,
                                          const float *radial3_host, const float *tangential2_host, float *origins,
                                          float *viewdirs, void *stream)
{
    CED_REQUIRE(width > 0 && height > 0, "generate_rays_hypercam: bad image size");
    CED_REQUIRE(orientation_host && position_host && origins && viewdirs, "generate_rays_hypercam: null pointer");
    ced::HyperCamArgs A{};
    A.width = width; A.height = height;
    ced::HyperCam &c = A.cam;
    for (int i = 0; i < 9; ++i) c.orientation[i] = orientation_host[i];
    for (int i = 0; i < 3; ++i) c.position[i] = position_host[i];
    c.focal = focal_length; c.ppx = principal_x; c.ppy = principal_y; c.skew = skew; c.aspect = pixel_aspect_ratio;
    c.k1 = radial3_host ? radial3_host[0] : 0.0f; c.k2 = radial3_host ? radial3_host[1] : 0.0f;
    c.k3 = radial3_host ? radial3_host[2] : 0.0f;
    c.p1 = tangential2_host ? tangential2_host[0] : 0.0f; c.p2 = tangential2_host ? tangential2_host[1] : 0.0f;
    c.distorted = ced::hypercam_is_distorted(c.k1, c.k2, c.k3, c.p1, c.p2);
    A.origins = origins; A.viewdirs = viewdirs;
    const int64_t n = (int64_t)width * height;
    hipLaunchKernelGGL(ced::hypercam_rays_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A);
    return ced::check_launch("generate_rays_hypercam");
}
