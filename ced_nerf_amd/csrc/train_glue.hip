// Element-wise pieces of the DIFFERENTIABLE field (training path; cednerf/model.py:354-466 as the
// reference trains it, train_real.py:339-420) that sit between its MLPs and its hash grid, one launch each instead of
// the ~35 torch element-wise / gather / cat kernels per direction they replace:
//   ced_train_inputs        sample positions from the rays, Frequency(4) of (x, t) for the motion MLP, SH(2) of the
//                           direction for the colour head                              (model.py:354-356, 447-455)
//   ced_train_inputs_backward  its gradient at the rays (or positions / directions / times), summed per ray
//   ced_train_warp[_bwd]    x' = x + move, normalised into the box, clamped; selector   (model.py:356-383)
//   ced_train_head_in[_bwd] density = exp(raw - 1) * selector (trunc_exp, utils.py:27-43), colour-head input
//                           [SH(4), geo(15)]                                             (model.py:414-417, 455)
// Same operation order as the torch statements of ced_nerf_amd/train.py they replace (the Frequency terms use the
// inference kernel's exact-reduction sin(pi y + phase), ced_common.hpp).  No parameters: nothing here is atomic.
#include "ced_common.hpp"

namespace ced {

struct TrainInputsArgs {
    int64_t n;
    const float *rays_o, *rays_d;        // rays mode: [n_rays, 3]
    const int64_t *ray_idx;              // [n] or NULL (explicit mode: positions / dirs / t per sample)
    const float *t0, *t1;                // rays mode: sample interval
    const float *ts;                     // rays mode: [n_rays] time per ray; explicit mode: [n] time per sample
    const float *pos_in, *dir_in;        // explicit mode: [n, 3]
    float *pos, *enc, *sh, *t_out;       // [n,3], [n,32], [n,4], [n]
};

__global__ __launch_bounds__(256) void train_inputs_kernel(TrainInputsArgs A)
{
    // four lanes per sample: lane q computes the Frequency features of input dimension q (x, y, z, t) -- 8 floats,
    // two 16-byte stores -- and one SH coefficient
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = gid >> 2;
    const int q = (int)(gid & 3);
    if (i >= A.n) return;
    float p[3], d[3], t;
    if (A.ray_idx) {
        const int64_t r = A.ray_idx[i];
        const float tm = (A.t0[i] + A.t1[i]) / 2.0f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            d[a] = A.rays_d[3 * r + a];
            p[a] = A.rays_o[3 * r + a] + d[a] * tm;
        }
        t = A.ts[r];
    } else {
#pragma unroll
        for (int a = 0; a < 3; ++a) { p[a] = A.pos_in[3 * i + a]; d[a] = A.dir_in[3 * i + a]; }
        t = A.ts[i];
    }
    const float v = q == 0 ? p[0] : (q == 1 ? p[1] : (q == 2 ? p[2] : t));
    typedef float f4 __attribute__((ext_vector_type(4)));
    f4 e0, e1;
    // tcnn Frequency: [dim][freq k][sin, cos] of pi * 2^k * v
    float s, c;
    det_sinpi_both(v * 1.0f, s, c); e0[0] = s; e0[1] = c;
    det_sinpi_both(v * 2.0f, s, c); e0[2] = s; e0[3] = c;
    det_sinpi_both(v * 4.0f, s, c); e1[0] = s; e1[1] = c;
    det_sinpi_both(v * 8.0f, s, c); e1[2] = s; e1[3] = c;
    f4 *eo = reinterpret_cast<f4 *>(A.enc + i * 32 + 8 * q);
    eo[0] = e0;
    eo[1] = e1;
    // SH degree 2 of w = ((d / |d| + 1) / 2) * 2 - 1   (the reference maps to [0, 1] and tcnn maps back)
    const float nrm = __builtin_sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    const int a = q == 1 ? 1 : (q == 2 ? 2 : 0);                 // coefficient q uses component y, z, x for q = 1, 2, 3
    const float w = ((d[a] / nrm + 1.0f) / 2.0f) * 2.0f - 1.0f;
    const float coef = q == 0 ? 0.28209479177387814f : (q == 2 ? 0.48860251190291987f * w : -0.48860251190291987f * w);
    A.sh[4 * i + q] = coef;
    if (q < 3) A.pos[3 * i + q] = p[q];
    else A.t_out[i] = t;
}

// ---------------------------------------------------------------------------------------------------------------
// Backward of train_inputs_kernel: the gradient at (positions, directions, time) per sample, and in rays mode its
// sum over each ray's samples.  The lane layout is the forward's: lane q of a sample's four owns input dimension q
// (x, y, z, t), reads that dimension's eight d_enc floats with two 16-byte loads and recomputes their sin / cos.
// ---------------------------------------------------------------------------------------------------------------
struct TrainInputsBwdArgs {
    int64_t n, n_rays;
    const float *rays_o, *rays_d;        // rays mode: [n_rays, 3]
    const int64_t *ray_idx;              // [n], non-decreasing, or NULL (explicit mode)
    const float *t0, *t1, *ts;
    const float *pos_in, *dir_in;        // explicit mode: [n, 3]
    const int64_t *packed;               // rays mode: [n_rays, 2] (first sample, count)
    const float *d_pos, *d_enc, *d_sh, *d_t;     // [n,3], [n,32], [n,4], [n]; each may be NULL (= zero)
    float *g_o, *g_d, *g_t;              // rays mode: [n_rays,3], [n_rays,3], [n_rays]; explicit mode: [n,3], [n,3], [n]
};

// Lane q of sample i, v its Frequency input (p[q] or t), d the direction:
//   ga = d_pos[i, q] (q < 3) or d_t[i] (q = 3), plus sum_k pi 2^k (d_enc[i, 8q + 2k] cos_k - d_enc[i, 8q + 2k + 1] sin_k)
//   gb = component q of the direction's gradient (g_w - w (w . g_w)) / |d|, w as the forward forms it (q < 3; else 0)
__device__ __forceinline__ void train_inputs_bwd_lane(const TrainInputsBwdArgs &A, int64_t i, int q, float v,
                                                      const float (&d)[3], float &ga, float &gb)
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    float g = 0.0f;
    if (A.d_enc) {
        const f4 *e = reinterpret_cast<const f4 *>(A.d_enc + i * 32 + 8 * q);
        const f4 e0 = e[0], e1 = e[1];
        float s, c;
        det_sinpi_both(v * 1.0f, s, c); const float a0 = 3.14159274101257324f * (e0[0] * c - e0[1] * s);
        det_sinpi_both(v * 2.0f, s, c); const float a1 = 6.28318548202514648f * (e0[2] * c - e0[3] * s);
        det_sinpi_both(v * 4.0f, s, c); const float a2 = 12.5663709640502930f * (e1[0] * c - e1[1] * s);
        det_sinpi_both(v * 8.0f, s, c); const float a3 = 25.1327419281005859f * (e1[2] * c - e1[3] * s);
        g = ((a0 + a1) + a2) + a3;
    }
    float up = 0.0f;
    if (q < 3) { if (A.d_pos) up = A.d_pos[3 * i + q]; }
    else if (A.d_t) up = A.d_t[i];
    ga = up + g;
    gb = 0.0f;
    if (A.d_sh && q < 3) {
        const f4 ds = *reinterpret_cast<const f4 *>(A.d_sh + 4 * i);
        const float K = 0.48860251190291987f;
        const float gw[3] = { -K * ds[3], -K * ds[1], K * ds[2] };
        const float nrm = __builtin_sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        float w[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) w[a] = ((d[a] / nrm + 1.0f) / 2.0f) * 2.0f - 1.0f;
        const float dot = (w[0] * gw[0] + w[1] * gw[1]) + w[2] * gw[2];
        const float wq = q == 0 ? w[0] : (q == 1 ? w[1] : w[2]);
        const float gq = q == 0 ? gw[0] : (q == 1 ? gw[1] : gw[2]);
        gb = (gq - wq * dot) / nrm;
    }
}

__global__ __launch_bounds__(256) void train_inputs_bwd_kernel(TrainInputsBwdArgs A)
{
    // explicit mode: one row of each output per sample
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = gid >> 2;
    const int q = (int)(gid & 3);
    if (i >= A.n) return;
    float d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) d[a] = A.dir_in[3 * i + a];
    const float v = q < 3 ? A.pos_in[3 * i + q] : A.ts[i];
    float ga, gb;
    train_inputs_bwd_lane(A, i, q, v, d, ga, gb);
    if (q < 3) { A.g_o[3 * i + q] = ga; A.g_d[3 * i + q] = gb; }
    else A.g_t[i] = ga;
}

constexpr int kInputsBwdChunk = 64;      // samples a wave answers for: it sums every ray that STARTS among them

// Rays mode.  The samples of a ray are consecutive (ray_idx is non-decreasing), so a ray's gradient is a segmented sum
// over the sample stream.  Each wave takes 64 consecutive samples and owns the rays whose first sample is among them: it
// skips the head samples of a ray that began earlier (that ray's owner runs on into this chunk) and runs on past its
// chunk to the end of its last ray.  It walks its samples 16 at a time (four lanes each, as above); a pass is a segmented
// inclusive scan over the 16 samples (shuffles at lane distances 4, 8, 16, 32, joined where the ray index agrees), the
// open ray's partial sum is carried into the next pass in registers, and the lanes of a ray's last sample store its
// rows.  No atomics, no LDS, no barrier, no workspace; the order of every sum is fixed by the inputs.  Blocks past the
// sample blocks write the zero rows of the rays without samples.
__global__ __launch_bounds__(256) void train_inputs_bwd_rays_kernel(TrainInputsBwdArgs A, unsigned sample_blocks)
{
    if (blockIdx.x >= sample_blocks) {
        const int64_t r = (int64_t)(blockIdx.x - sample_blocks) * blockDim.x + threadIdx.x;
        if (r < A.n_rays && A.packed[2 * r + 1] == 0) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { A.g_o[3 * r + a] = 0.0f; A.g_d[3 * r + a] = 0.0f; }
            A.g_t[r] = 0.0f;
        }
        return;
    }
    const int lane = threadIdx.x & 63;
    const int q = lane & 3, s = lane >> 2;
    const int64_t c0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kInputsBwdChunk;
    if (c0 >= A.n) return;
    const int64_t c1 = c0 + kInputsBwdChunk < A.n ? c0 + kInputsBwdChunk : A.n;
    int64_t first = c0;
    if (c0 > 0) {
        const int64_t r0 = A.ray_idx[c0];
        if ((uint64_t)r0 >= (uint64_t)A.n_rays) return;
        if (A.ray_idx[c0 - 1] == r0) first = A.packed[2 * r0] + A.packed[2 * r0 + 1];     // where the ray before ends
        if (first < c0) first = c0;
    }
    if (first >= c1) return;                       // one earlier ray covers the whole chunk
    const int64_t rl = A.ray_idx[c1 - 1];
    if ((uint64_t)rl >= (uint64_t)A.n_rays) return;
    int64_t end = A.packed[2 * rl] + A.packed[2 * rl + 1];
    if (end > A.n) end = A.n;
    float carry_a = 0.0f, carry_b = 0.0f;
    int carry_ray = -1;
    for (int64_t base = first; base < end; base += 16) {
        const int64_t i = base + s;
        const bool valid = i < end;
        int ray = -2;                              // the low word of the ray index; -2: no sample
        int64_t r = 0;
        bool last = false;
        float va = 0.0f, vb = 0.0f;
        if (valid) {
            r = A.ray_idx[i];
            ray = (int)r;
            last = i + 1 >= A.n || A.ray_idx[i + 1] != r;
            if ((uint64_t)r >= (uint64_t)A.n_rays) { r = 0; last = false; }
            const float tm = (A.t0[i] + A.t1[i]) / 2.0f;
            float d[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) d[a] = A.rays_d[3 * r + a];
            const float dq = q == 0 ? d[0] : (q == 1 ? d[1] : d[2]);
            const float v = q < 3 ? A.rays_o[3 * r + q] + dq * tm : A.ts[r];
            float gb;
            train_inputs_bwd_lane(A, i, q, v, d, va, gb);
            vb = va * tm + gb;                     // d_rays_d's term: g_pos t_mid + g_dir (unused by lane 3)
            if (s == 0 && ray == carry_ray) { va = carry_a + va; vb = carry_b + vb; }
        }
#pragma unroll
        for (int off = 4; off < 64; off <<= 1) {
            const float ua = __shfl_up(va, off, 64), ub = __shfl_up(vb, off, 64);
            const int ur = __shfl_up(ray, off, 64);
            if (lane >= off && ur == ray) { va = ua + va; vb = ub + vb; }
        }
        if (valid && last) {
            if (q < 3) { A.g_o[3 * r + q] = va; A.g_d[3 * r + q] = vb; }
            else A.g_t[r] = va;
        }
        carry_a = __shfl(va, 60 + q, 64);
        carry_b = __shfl(vb, 60 + q, 64);
        carry_ray = __shfl(ray, 63, 64);
    }
}

struct TrainWarpArgs {
    int64_t n;
    const float *pos, *mo;               // [n,3], [n,mo_w]
    int mo_w, use_div;
    float moving_step, lo[3], ext[3];
    float *xn, *move, *selector;         // forward outputs: clamped normalised position, move, selector (0 / 1)
    const float *d_xn, *d_move;          // backward inputs (d_move may be NULL)
    float *d_mo;                         // backward output [n, mo_w]
    const float *xn_raw_sel;             // unused
    float *d_pos;                        // backward output [n, 3] (train_warp_bwd_pos_kernel)
};

__device__ __forceinline__ float det_tanhf(float x)
{
    // tanh(x) = 1 - 2 / (exp(2x) + 1), exp from the contract's polynomial kernel
    const float e = det_expf(2.0f * x);
    return 1.0f - 2.0f / (e + 1.0f);
}

__global__ __launch_bounds__(256) void train_warp_kernel(TrainWarpArgs A)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float mv = A.mo[i * A.mo_w + a] * A.moving_step;
        if (A.use_div) mv = mv + det_tanhf(A.mo[i * A.mo_w + 3 + a]) * A.moving_step;
        const float xn = ((A.pos[3 * i + a] + mv) - A.lo[a]) / A.ext[a];
        inside = inside && (xn > 0.0f) && (xn < 1.0f);
        A.move[3 * i + a] = mv;
        A.xn[3 * i + a] = __builtin_fminf(__builtin_fmaxf(xn, 0.0f), 1.0f);
    }
    A.selector[i] = inside ? 1.0f : 0.0f;
}

// d_mo from d_xn (gradient at the CLAMPED normalised position: passes where 0 <= xn <= 1, torch.clamp's rule) and
// d_move (the `move` output's own consumers: the attenuated time encoder's norm, the internal outputs)
__global__ __launch_bounds__(256) void train_warp_bwd_kernel(TrainWarpArgs A)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float mv = A.mo[i * A.mo_w + a] * A.moving_step;
        float th = 0.0f;
        if (A.use_div) { th = det_tanhf(A.mo[i * A.mo_w + 3 + a]); mv = mv + th * A.moving_step; }
        const float xn = ((A.pos[3 * i + a] + mv) - A.lo[a]) / A.ext[a];
        const bool pass = xn >= 0.0f && xn <= 1.0f;
        float g = pass ? A.d_xn[3 * i + a] / A.ext[a] : 0.0f;
        if (A.d_move) g = g + A.d_move[3 * i + a];
        A.d_mo[i * A.mo_w + a] = g * A.moving_step;
        if (A.use_div) A.d_mo[i * A.mo_w + 3 + a] = (g * A.moving_step) * (1.0f - th * th);
    }
    for (int k = A.use_div ? 6 : 3; k < A.mo_w; ++k) A.d_mo[i * A.mo_w + k] = 0.0f;
}

// d_pos from d_xn: the same clamp rule, and d xn / d pos = 1 / (aabb_hi - aabb_lo); `move` does not depend on pos
__global__ __launch_bounds__(256) void train_warp_bwd_pos_kernel(TrainWarpArgs A)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float mv = A.mo[i * A.mo_w + a] * A.moving_step;
        if (A.use_div) mv = mv + det_tanhf(A.mo[i * A.mo_w + 3 + a]) * A.moving_step;
        const float xn = ((A.pos[3 * i + a] + mv) - A.lo[a]) / A.ext[a];
        const bool pass = xn >= 0.0f && xn <= 1.0f;
        A.d_pos[3 * i + a] = pass ? A.d_xn[3 * i + a] / A.ext[a] : 0.0f;
    }
}

struct TrainHeadArgs {
    int64_t n;
    const float *bout, *sh, *selector;   // [n,16], [n,4], [n]
    float *head_in, *sigma;              // [n,19], [n]
    const float *d_head_in, *d_sigma;    // backward inputs
    float *d_bout;                       // backward output [n,16]
};

__global__ __launch_bounds__(256) void train_head_in_kernel(TrainHeadArgs A)
{
    // 4 lanes per sample: lane q moves geo features 4q .. 4q + 3 (and, for q = 0, the density; SH by all four)
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = gid >> 2;
    const int q = (int)(gid & 3);
    if (i >= A.n) return;
    const float *b = A.bout + 16 * i;
    float *h = A.head_in + 19 * i;
    h[q] = A.sh[4 * i + q];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = 4 * q + k;               // bout column 1 + j -> head_in column 4 + j, j = 0..14
        if (j < 15) h[4 + j] = b[1 + j];
    }
    if (q == 0) A.sigma[i] = det_expf(b[0] - 1.0f) * A.selector[i];
}

__global__ __launch_bounds__(256) void train_head_in_bwd_kernel(TrainHeadArgs A)
{
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = gid >> 2;
    const int q = (int)(gid & 3);
    if (i >= A.n) return;
    float *db = A.d_bout + 16 * i;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = 4 * q + k;
        if (j < 15) db[1 + j] = A.d_head_in ? A.d_head_in[19 * i + 4 + j] : 0.0f;
    }
    if (q == 0) {
        // trunc_exp backward: g * exp(clamp(x, max = 15)), x = raw - 1; the selector factor of the product
        const float x = A.bout[16 * i] - 1.0f;
        const float g = A.d_sigma ? A.d_sigma[i] * A.selector[i] : 0.0f;
        db[0] = g * det_expf(__builtin_fminf(x, 15.0f));
    }
}

}  // namespace ced

extern "C" int ced_train_inputs(int64_t n, const float *rays_o, const float *rays_d, const int64_t *ray_indices,
                                const float *t_starts, const float *t_ends, const float *timestamps,
                                const float *positions, const float *directions, float *pos_out, float *enc_out,
                                float *sh_out, float *t_out, void *stream)
{
    CED_REQUIRE(n >= 0, "train_inputs: n < 0");
    if (n == 0) return CED_OK;
    CED_REQUIRE(timestamps && pos_out && enc_out && sh_out && t_out, "train_inputs: null pointer");
    if (ray_indices) CED_REQUIRE(rays_o && rays_d && t_starts && t_ends, "train_inputs: rays mode needs rays and sample intervals");
    else CED_REQUIRE(positions && directions, "train_inputs: explicit mode needs positions and directions");
    CED_REQUIRE((reinterpret_cast<uintptr_t>(enc_out) & 15) == 0, "train_inputs: enc_out must be 16-byte aligned");
    ced::TrainInputsArgs A{ n, rays_o, rays_d, ray_indices, t_starts, t_ends, timestamps, positions, directions,
                            pos_out, enc_out, sh_out, t_out };
    hipLaunchKernelGGL(ced::train_inputs_kernel, dim3((unsigned)((4 * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A);
    return ced::check_launch("train_inputs");
}

extern "C" int ced_train_inputs_backward(int64_t n, int64_t n_rays, const float *rays_o, const float *rays_d,
                                         const int64_t *ray_indices, const float *t_starts, const float *t_ends,
                                         const float *timestamps, const float *positions, const float *directions,
                                         const int64_t *packed_info, const float *d_pos, const float *d_enc,
                                         const float *d_sh, const float *d_t, float *d_origins, float *d_directions,
                                         float *d_times, void *stream)
{
    CED_REQUIRE(n >= 0 && n_rays >= 0, "train_inputs_backward: n < 0 or n_rays < 0");
    if (ray_indices ? n_rays == 0 : n == 0) return CED_OK;
    CED_REQUIRE(timestamps && d_origins && d_directions && d_times, "train_inputs_backward: null pointer");
    CED_REQUIRE(!d_enc || (reinterpret_cast<uintptr_t>(d_enc) & 15) == 0, "train_inputs_backward: d_enc must be 16-byte aligned");
    CED_REQUIRE(!d_sh || (reinterpret_cast<uintptr_t>(d_sh) & 15) == 0, "train_inputs_backward: d_sh must be 16-byte aligned");
    ced::TrainInputsBwdArgs A{ n, n_rays, rays_o, rays_d, ray_indices, t_starts, t_ends, timestamps, positions, directions,
                               packed_info, d_pos, d_enc, d_sh, d_t, d_origins, d_directions, d_times };
    if (!ray_indices) {
        CED_REQUIRE(positions && directions, "train_inputs_backward: explicit mode needs positions and directions");
        hipLaunchKernelGGL(ced::train_inputs_bwd_kernel, dim3((unsigned)((4 * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A);
        return ced::check_launch("train_inputs_backward");
    }
    CED_REQUIRE(n == 0 || (rays_o && rays_d && t_starts && t_ends), "train_inputs_backward: rays mode needs rays and sample intervals");
    CED_REQUIRE(packed_info, "train_inputs_backward: rays mode needs packed_info");
    CED_REQUIRE(n_rays < (int64_t)1 << 31, "train_inputs_backward: n_rays %lld", (long long)n_rays);
    const int64_t per_block = 4 * ced::kInputsBwdChunk;
    const unsigned sample_blocks = (unsigned)((n + per_block - 1) / per_block);
    const unsigned ray_blocks = (unsigned)((n_rays + 255) / 256);
    hipLaunchKernelGGL(ced::train_inputs_bwd_rays_kernel, dim3(sample_blocks + ray_blocks), dim3(256), 0, (hipStream_t)stream, A,
                       sample_blocks);
    return ced::check_launch("train_inputs_backward");
}

static int fill_warp(ced::TrainWarpArgs &A, int64_t n, const float *pos, const float *mo, int32_t mo_width,
                     int32_t use_div_offsets, float moving_step, const float *aabb_host, const char *who)
{
    CED_REQUIRE(n >= 0 && pos && mo && aabb_host, "%s: null pointer", who);
    CED_REQUIRE(mo_width >= (use_div_offsets ? 6 : 3) && mo_width <= 64, "%s: mo_width %d", who, mo_width);
    A.n = n; A.pos = pos; A.mo = mo; A.mo_w = mo_width; A.use_div = use_div_offsets ? 1 : 0; A.moving_step = moving_step;
    for (int a = 0; a < 3; ++a) { A.lo[a] = aabb_host[a]; A.ext[a] = aabb_host[3 + a] - aabb_host[a]; }
    return CED_OK;
}

extern "C" int ced_train_warp(int64_t n, const float *pos, const float *mo, int32_t mo_width, int32_t use_div_offsets,
                              float moving_step, const float *aabb_host, float *xn, float *move, float *selector,
                              void *stream)
{
    ced::TrainWarpArgs A{};
    int rc = fill_warp(A, n, pos, mo, mo_width, use_div_offsets, moving_step, aabb_host, "train_warp");
    if (rc) return rc;
    if (n == 0) return CED_OK;
    CED_REQUIRE(xn && move && selector, "train_warp: null output");
    A.xn = xn; A.move = move; A.selector = selector;
    hipLaunchKernelGGL(ced::train_warp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A);
    return ced::check_launch("train_warp");
}

extern "C" int ced_train_warp_backward(int64_t n, const float *pos, const float *mo, int32_t mo_width,
                                       int32_t use_div_offsets, float moving_step, const float *aabb_host,
                                       const float *d_xn, const float *d_move, float *d_mo, void *stream)
{
    ced::TrainWarpArgs A{};
    int rc = fill_warp(A, n, pos, mo, mo_width, use_div_offsets, moving_step, aabb_host, "train_warp_backward");
    if (rc) return rc;
    if (n == 0) return CED_OK;
    CED_REQUIRE(d_xn && d_mo, "train_warp_backward: null pointer");
    A.d_xn = d_xn; A.d_move = d_move; A.d_mo = d_mo;
    hipLaunchKernelGGL(ced::train_warp_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A);
    return ced::check_launch("train_warp_backward");
}

extern "C" int ced_train_warp_backward_pos(int64_t n, const float *pos, const float *mo, int32_t mo_width,
                                           int32_t use_div_offsets, float moving_step, const float *aabb_host,
                                           const float *d_xn, float *d_pos, void *stream)
{
    ced::TrainWarpArgs A{};
    int rc = fill_warp(A, n, pos, mo, mo_width, use_div_offsets, moving_step, aabb_host, "train_warp_backward_pos");
    if (rc) return rc;
    if (n == 0) return CED_OK;
    CED_REQUIRE(d_xn && d_pos, "train_warp_backward_pos: null pointer");
    A.d_xn = d_xn; A.d_pos = d_pos;
    hipLaunchKernelGGL(ced::train_warp_bwd_pos_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A);
    return ced::check_launch("train_warp_backward_pos");
}

extern "C" int ced_train_head_in(int64_t n, const float *bout, const float *sh, const float *selector, float *head_in,
                                 float *sigma, void *stream)
{
    CED_REQUIRE(n >= 0, "train_head_in: n < 0");
    if (n == 0) return CED_OK;
    CED_REQUIRE(bout && sh && selector && head_in && sigma, "train_head_in: null pointer");
    ced::TrainHeadArgs A{ n, bout, sh, selector, head_in, sigma, nullptr, nullptr, nullptr };
    hipLaunchKernelGGL(ced::train_head_in_kernel, dim3((unsigned)((4 * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A);
    return ced::check_launch("train_head_in");
}

extern "C" int ced_train_head_in_backward(int64_t n, const float *bout, const float *selector, const float *d_head_in,
                                          const float *d_sigma, float *d_bout, void *stream)
{
    CED_REQUIRE(n >= 0, "train_head_in_backward: n < 0");
    if (n == 0) return CED_OK;
    CED_REQUIRE(bout && selector && d_bout, "train_head_in_backward: null pointer");
    ced::TrainHeadArgs A{ n, bout, nullptr, selector, nullptr, nullptr, d_head_in, d_sigma, d_bout };
    hipLaunchKernelGGL(ced::train_head_in_bwd_kernel, dim3((unsigned)((4 * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A);
    return ced::check_launch("train_head_in_backward");
}
