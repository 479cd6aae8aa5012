// Distortion loss of the reference's `-d` regulariser (train_real.py:379-386 -> cednerf/losses.py:4-11 ->
// torch_efficient_distloss.flatten_eff_distloss), forward and gradient in one pass per ray.
//
// For one ray with samples i in marching order, s_i = t_end - t_start, m_i = (t_start + t_end) / 2:
//   L_ray = sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i s_i w_i^2 = 2 sum_i w_i D_i + 1/3 sum_i s_i w_i^2
//   dL_ray/dw_i = 2 (D_i + E_i) + 2/3 s_i w_i
// with D_i = sum_{j<i} w_j (m_i - m_j) and E_i = sum_{j>i} w_j (m_j - m_i).  The package writes these as
// m_i W_<i - WM_<i and WM_>i - m_i W_>i; here they run as their own recurrences
//   D_i = D_{i-1} + W_<i (m_i - m_{i-1}),   E_i = E_{i+1} + W_>i (m_{i+1} - m_i),
// whose terms are all >= 0 for samples in marching order: no cancellation of m W against WM, and the midpoint steps
// come from differences of neighbouring t values (exact in fp32), not from rounded midpoints.  The running sums (W, D,
// E, the loss, the suffix of the density gradient) are fp64: in fp32 the recurrences drift by ~sqrt(n) ulps over a ray
// of n samples (1e-6 of the largest gradient at 1.6 M samples), in fp64 the results are the fp32 rounding of the sums.
//
// One lane owns one ray (like composite_backward_kernel): a forward sweep for W_<, D and the loss, then a reverse sweep
// for W_>, E and the gradient.  Each workgroup sums its rays' losses in a fixed tree into a partial, one more workgroup
// sums the partials in a fixed order: no float atomics, two calls give the same bits.  Precondition (met by every producer in this package): samples are grouped by ray, in the order of
// packed_info, and t_starts does not decrease within a ray.
#include "ced_common.hpp"
#include "composite_core.hpp"

namespace ced {

// the midpoint step m_b - m_a from the neighbouring sample bounds
__device__ __forceinline__ float mid_step(float ta0, float ta1, float tb0, float tb1)
{
    return ((tb0 - ta0) + (tb1 - ta1)) * 0.5f;
}

// per-sample term of the loss: 2 w D + 1/3 s w^2
__device__ __forceinline__ double dist_term(double w, double D, double s)
{
    return 2.0 * (w * D) + (s * (w * w)) * (1.0 / 3.0);
}

// weights route, one ray: L_ray; grad (may be NULL) [S] = dL_ray/dw (unscaled), the scratch of D_i in between
__device__ __forceinline__ double ray_weights(int64_t s0, int64_t cnt, const float *__restrict__ w, const float *__restrict__ t0,
                                              const float *__restrict__ t1, float *__restrict__ grad)
{
    double W = 0.0, D = 0.0, L = 0.0;
    float p0 = 0.0f, p1 = 0.0f;
    for (int64_t i = s0; i < s0 + cnt; ++i) {
        const float ts = t0[i], te = t1[i], wi = w[i];
        if (i > s0) D = D + W * (double)mid_step(p0, p1, ts, te);
        L = L + dist_term(wi, D, te - ts);
        if (grad) grad[i] = (float)D;
        W = W + wi;
        p0 = ts; p1 = te;
    }
    if (!grad) return L;
    double Wg = 0.0, E = 0.0;
    for (int64_t i = s0 + cnt - 1; i >= s0; --i) {
        const float ts = t0[i], te = t1[i], wi = w[i];
        if (i < s0 + cnt - 1) E = E + Wg * (double)mid_step(ts, te, p0, p1);
        grad[i] = (float)(2.0 * ((double)grad[i] + E) + (2.0 / 3.0) * ((double)(te - ts) * wi));
        Wg = Wg + wi;
        p0 = ts; p1 = te;
    }
    return L;
}

// fused route, one ray: the weights of render_weights_kernel (the same sample_step, composite_core.hpp), L_ray, and the gradient through
// the weights to the densities, d sigma_i = s_i (g_i (T_i - w_i) - sum_{k>i} g_k w_k), g = dL_ray/dw (the composite
// backward's formula).  d_sig holds D_i and trans T_i between the two sweeps, so the reverse sweep sees the forward's
// weights bit for bit.  d_sig and trans are both NULL (loss only) or both set.
__device__ __forceinline__ double ray_density(int64_t s0, int64_t cnt, const float *__restrict__ sig, const float *__restrict__ t0,
                                              const float *__restrict__ t1, float *__restrict__ d_sig, float *__restrict__ trans)
{
    float acc = 0.0f, p0 = 0.0f, p1 = 0.0f;
    double W = 0.0, D = 0.0, L = 0.0;
    for (int64_t i = s0; i < s0 + cnt; ++i) {
        const float ts = t0[i], te = t1[i];
        const Sample s = sample_step(sig[i], ts, te, trans_of(acc));
        const float t = s.T, wi = s.w;
        acc = acc + s.sd;
        if (i > s0) D = D + W * (double)mid_step(p0, p1, ts, te);
        L = L + dist_term(wi, D, te - ts);
        if (d_sig) { d_sig[i] = (float)D; trans[i] = t; }
        W = W + wi;
        p0 = ts; p1 = te;
    }
    if (!d_sig) return L;
    double Wg = 0.0, E = 0.0, suffix = 0.0;
    for (int64_t i = s0 + cnt - 1; i >= s0; --i) {
        const float ts = t0[i], te = t1[i];
        const float dt = te - ts;
        const Sample s = sample_step(sig[i], ts, te, trans[i]);
        const float t = s.T, wi = s.w;
        if (i < s0 + cnt - 1) E = E + Wg * (double)mid_step(ts, te, p0, p1);
        const double g = 2.0 * ((double)d_sig[i] + E) + (2.0 / 3.0) * ((double)dt * wi);
        d_sig[i] = (float)(dt * (g * ((double)t - (double)wi) - suffix));
        suffix = suffix + g * wi;
        Wg = Wg + wi;
        p0 = ts; p1 = te;
    }
    return L;
}

constexpr int kRayThreads = 256;          // rays per workgroup = partials per workgroup
constexpr int kReduceThreads = 1024;

// fixed-order tree over the workgroup: the sum of the losses and the largest ray index that has a sample
template <int N>
__device__ __forceinline__ void block_reduce(double &sum, int64_t &last, double *s_sum, int64_t *s_last)
{
    const int k = threadIdx.x;
    s_sum[k] = sum;
    s_last[k] = last;
    __syncthreads();
    for (int h = N / 2; h > 0; h >>= 1) {
        if (k < h) {
            s_sum[k] = s_sum[k] + s_sum[k + h];
            s_last[k] = s_last[k] > s_last[k + h] ? s_last[k] : s_last[k + h];
        }
        __syncthreads();
    }
    sum = s_sum[0];
    last = s_last[0];
}

// one lane per ray: ray_loss [n_rays] and the workgroup's partial (sum of its rays' losses, largest ray with a sample)
template <bool kDensity>
__global__ __launch_bounds__(kRayThreads) void distortion_kernel(int64_t n_rays, const int64_t *__restrict__ packed,
                                                                 const float *__restrict__ in, const float *__restrict__ t0,
                                                                 const float *__restrict__ t1, float *__restrict__ ray_loss,
                                                                 float *__restrict__ grad, float *__restrict__ trans,
                                                                 double *__restrict__ part_sum, int64_t *__restrict__ part_last)
{
    __shared__ double s_sum[kRayThreads];
    __shared__ int64_t s_last[kRayThreads];
    const int64_t r = (int64_t)blockIdx.x * kRayThreads + threadIdx.x;
    double L = 0.0;
    int64_t last = -1;
    if (r < n_rays) {
        const int64_t s0 = packed[2 * r], cnt = packed[2 * r + 1];
        L = kDensity ? ray_density(s0, cnt, in, t0, t1, grad, trans) : ray_weights(s0, cnt, in, t0, t1, grad);
        ray_loss[r] = (float)L;
        if (cnt > 0) last = r;
    }
    block_reduce<kRayThreads>(L, last, s_sum, s_last);
    if (threadIdx.x == 0) {
        part_sum[blockIdx.x] = L;
        part_last[blockIdx.x] = last;
    }
}

// loss = sum of the partials / n_norm and inv_norm = 1 / n_norm, n_norm = 1 + the largest ray index with a sample (none:
// both 0).  One workgroup: lane k sums partials k, k + 1024, ... in order (fp64), then the fixed tree.
__global__ __launch_bounds__(kReduceThreads) void distortion_finish_kernel(int64_t n_parts, const double *__restrict__ part_sum,
                                                                           const int64_t *__restrict__ part_last,
                                                                           float *__restrict__ loss, float *__restrict__ inv_norm)
{
    __shared__ double s_sum[kReduceThreads];
    __shared__ int64_t s_last[kReduceThreads];
    double sum = 0.0;
    int64_t last = -1;
    for (int64_t p = threadIdx.x; p < n_parts; p += kReduceThreads) {
        sum = sum + part_sum[p];
        last = part_last[p] > last ? part_last[p] : last;
    }
    block_reduce<kReduceThreads>(sum, last, s_sum, s_last);
    if (threadIdx.x == 0) {
        const double n = (double)(last + 1);
        loss[0] = last >= 0 ? (float)(sum / n) : 0.0f;
        inv_norm[0] = last >= 0 ? (float)(1.0 / n) : 0.0f;
    }
}

static inline int64_t n_parts(int64_t n_rays) { return (n_rays + kRayThreads - 1) / kRayThreads; }

// workspace: [partial sums: n_parts doubles][partial last rays: n_parts int64][trans: n_samples floats (density route)]
static inline int64_t workspace_bytes(int64_t n_rays, int64_t n_samples, bool density)
{
    return n_parts(n_rays) * 16 + (density ? n_samples * 4 : 0);
}

// the empty cases: zero outputs without a kernel launch
static int distortion_zero(int64_t n_rays, int64_t n_samples, float *ray_loss, float *grad, float *loss, float *inv_norm,
                           hipStream_t st)
{
    if (hipMemsetAsync(loss, 0, 4, st) != hipSuccess || hipMemsetAsync(inv_norm, 0, 4, st) != hipSuccess ||
        (n_rays > 0 && hipMemsetAsync(ray_loss, 0, (size_t)n_rays * 4, st) != hipSuccess) ||
        (grad && n_samples > 0 && hipMemsetAsync(grad, 0, (size_t)n_samples * 4, st) != hipSuccess))
        return check_launch("distortion_loss (memset)");
    return CED_OK;
}

template <bool kDensity>
static int distortion(const char *what, int64_t n_rays, int64_t n_samples, const int64_t *packed, const float *in,
                      const float *t0, const float *t1, float *ray_loss, float *grad, void *workspace, float *loss,
                      float *inv_norm, hipStream_t st)
{
    if (n_rays == 0 || n_samples == 0) return distortion_zero(n_rays, n_samples, ray_loss, grad, loss, inv_norm, st);
    CED_REQUIRE(packed && in && t0 && t1 && workspace, "%s: null pointer", what);
    const int64_t parts = n_parts(n_rays);
    double *part_sum = (double *)workspace;
    int64_t *part_last = (int64_t *)(part_sum + parts);
    float *trans = (kDensity && grad) ? (float *)(part_last + parts) : nullptr;
    hipLaunchKernelGGL(distortion_kernel<kDensity>, dim3((unsigned)parts), dim3(kRayThreads), 0, st, n_rays, packed, in, t0, t1,
                       ray_loss, grad, trans, part_sum, part_last);
    hipLaunchKernelGGL(distortion_finish_kernel, dim3(1), dim3(kReduceThreads), 0, st, parts, part_sum, part_last, loss, inv_norm);
    return check_launch(what);
}

}  // namespace ced

extern "C" int64_t ced_distortion_workspace_bytes(int64_t n_rays, int64_t n_samples, int32_t density)
{
    CED_REQUIRE(n_rays >= 0 && n_samples >= 0, "distortion_workspace_bytes: negative size");
    return ced::workspace_bytes(n_rays, n_samples, density != 0);
}

extern "C" int ced_distortion_loss(int64_t n_rays, int64_t n_samples, const int64_t *packed_info, const float *weights,
                                   const float *t_starts, const float *t_ends, float *ray_loss, float *grad_weights,
                                   void *workspace, float *loss, float *inv_norm, void *stream)
{
    CED_REQUIRE(n_rays >= 0 && n_samples >= 0, "distortion_loss: negative size");
    CED_REQUIRE(loss && inv_norm && (ray_loss || n_rays == 0), "distortion_loss: null output");
    return ced::distortion<false>("distortion_loss", n_rays, n_samples, packed_info, weights, t_starts, t_ends, ray_loss,
                                  grad_weights, workspace, loss, inv_norm, (hipStream_t)stream);
}

extern "C" int ced_distortion_loss_density(int64_t n_rays, int64_t n_samples, const int64_t *packed_info, const float *sigmas,
                                           const float *t_starts, const float *t_ends, float *ray_loss, float *d_sigmas,
                                           void *workspace, float *loss, float *inv_norm, void *stream)
{
    CED_REQUIRE(n_rays >= 0 && n_samples >= 0, "distortion_loss_density: negative size");
    CED_REQUIRE(loss && inv_norm && (ray_loss || n_rays == 0), "distortion_loss_density: null output");
    return ced::distortion<true>("distortion_loss_density", n_rays, n_samples, packed_info, sigmas, t_starts, t_ends, ray_loss,
                                 d_sigmas, workspace, loss, inv_norm, (hipStream_t)stream);
}
