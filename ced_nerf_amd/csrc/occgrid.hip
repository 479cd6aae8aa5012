// Occupancy-grid maintenance: the device side of
// nerfacc.OccGridEstimator._update / update_every_n_steps as driven at train_real.py:324-336.
// nerfacc itself does these steps with torch ops; here the two per-sample pieces around the density
// query are native: cell index + jitter -> world position (one launch), and the EMA-max write-back (three
// small ones, so that a cell listed several times decays once and takes the largest of its samples).
#include "ced_common.hpp"

namespace ced {

// x = (grid_coord(idx) + noise) / res  ->  aabb_min + x * (aabb_max - aabb_min); idx = (ix*res + iy)*res + iz
__global__ __launch_bounds__(256) void occ_points_kernel(int64_t n, const int64_t *__restrict__ cell_idx,
                                                         const float *__restrict__ noise, int res, float a0, float a1,
                                                         float a2, float e0, float e1, float e2,
                                                         float *__restrict__ pos)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t c = cell_idx[i];
    const int iz = (int)(c % res), iy = (int)((c / res) % res), ix = (int)(c / ((int64_t)res * res));
    const float resf = (float)res;
    const float x = ((float)ix + noise[3 * i]) / resf;
    const float y = ((float)iy + noise[3 * i + 1]) / resf;
    const float z = ((float)iz + noise[3 * i + 2]) / resf;
    pos[3 * i] = a0 + x * e0;
    pos[3 * i + 1] = a1 + y * e1;
    pos[3 * i + 2] = a2 + z * e2;
}

// EMA write-back, occs[c] = fmax(occs[c] * decay, max over the samples of c of density * step), for a list that may name
// a cell any number of times (the sampled draw is with replacement and then appends the occupied cells).  Three launches,
// none of which reads a cell after a write to it:
//   gather : decayed[i] = occs[id_i] * decay               reads occs, writes the workspace
//   spread : occs[id_i] = decayed[i]                        the writers of one cell all store the same bits
//   max    : occs[id_i] = max(occs[id_i], density_i * step) an integer atomic on the float's bits, so any order of the
//                                                           writers leaves the largest; a NaN sample is skipped (fmaxf)
__global__ __launch_bounds__(256) void occ_ema_gather_kernel(int64_t n, const int64_t *__restrict__ cell_ids, float decay,
                                                             const float *__restrict__ occs, float *__restrict__ decayed)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = __fmul_rn(occs[cell_ids[i]], decay);
    // a NaN loses against every sample (fmaxf): the pattern below is under both atomics of the max kernel, and still a NaN
    decayed[i] = v == v ? v : __uint_as_float(0xffffffffu);
}

__global__ __launch_bounds__(256) void occ_ema_spread_kernel(int64_t n, const int64_t *__restrict__ cell_ids,
                                                             const float *__restrict__ decayed, float *__restrict__ occs)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    occs[cell_ids[i]] = decayed[i];
}

// Floats without the sign bit order like their bits as signed integers (and above every pattern with the sign bit);
// floats with it order opposite to their bits as unsigned integers (and below every pattern without it).  -0 < +0.
__global__ __launch_bounds__(256) void occ_ema_max_kernel(int64_t n, const int64_t *__restrict__ cell_ids,
                                                          const float *__restrict__ density, float step_size,
                                                          float *__restrict__ occs)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float occ = __fmul_rn(density[i], step_size);
    if (occ != occ) return;
    const unsigned int b = __float_as_uint(occ);
    float *cell = occs + cell_ids[i];
    if (b >> 31) atomicMin(reinterpret_cast<unsigned int *>(cell), b);
    else atomicMax(reinterpret_cast<int *>(cell), (int)b);
}

// Time slices (ced_occ_time_slices), first kernel: hit[b, cell_ids[p]] = max_sigma[b, p] * step_size > thre.  One thread per
// (bin, row); a listed cell's byte is written by its row alone (or by several rows with one value), unlisted cells keep
// the 0 the caller cleared them to.  An id outside the grid is skipped.
__global__ __launch_bounds__(256) void occ_slice_mark_kernel(int64_t n, int64_t total, const int64_t *__restrict__ cell_ids,
                                                             const float *__restrict__ max_sigma, float step_size, float thre,
                                                             int64_t cells, uint8_t *__restrict__ hit)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t b = i / n, p = i - b * n;
    const int64_t id = cell_ids[p];
    if (id < 0 || id >= cells) return;
    hit[b * cells + id] = __fmul_rn(max_sigma[i], step_size) > thre ? 1 : 0;      // false for a NaN
}

// second kernel: out[b, l, c] = (hit[b, l, c], or the OR of hit over c's 3x3x3 neighbourhood inside level l) AND union[l, c]
__global__ __launch_bounds__(256) void occ_slice_finish_kernel(int64_t total, int64_t cells, int res, int dilate,
                                                               const uint8_t *__restrict__ hit, const uint8_t *__restrict__ uni,
                                                               uint8_t *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t id = i % cells;                                        // level * R^3 + cell
    uint8_t v = hit[i];
    if (dilate && !v) {
        const int64_t per = (int64_t)res * res * res;
        const int64_t c = id % per;
        const int iz = (int)(c % res), iy = (int)((c / res) % res), ix = (int)(c / ((int64_t)res * res));
        for (int dx = -1; dx <= 1; ++dx) {
            for (int dy = -1; dy <= 1; ++dy) {
                for (int dz = -1; dz <= 1; ++dz) {
                    const int x = ix + dx, y = iy + dy, z = iz + dz;
                    if (x < 0 || x >= res || y < 0 || y >= res || z < 0 || z >= res) continue;
                    v |= hit[i + ((int64_t)dx * res + dy) * res + dz];
                }
            }
        }
    }
    if (uni) v = v && uni[id];
    out[i] = v ? 1 : 0;
}

}  // namespace ced

extern "C" int64_t ced_occ_time_slices_workspace_bytes(int32_t n_bins, int32_t levels, int32_t res)
{
    if (n_bins < 1 || n_bins > CED_TIME_MAX_BINS || levels < 1 || levels > 64 || res < 1 || res > 1024) return -1;
    return (int64_t)n_bins * levels * res * res * res;
}

extern "C" int ced_occ_time_slices(int64_t n, const int64_t *cell_ids, const float *max_sigma, int32_t n_bins, float step_size,
                                   float thre, int32_t levels, int32_t res, const uint8_t *union_binaries, int32_t dilate,
                                   uint8_t *out, void *workspace, int64_t workspace_bytes, void *stream)
{
    CED_REQUIRE(n >= 0, "occ_time_slices: n < 0");
    CED_REQUIRE(n_bins >= 1 && n_bins <= CED_TIME_MAX_BINS, "occ_time_slices: n_bins=%d outside 1 .. %d", n_bins, CED_TIME_MAX_BINS);
    CED_REQUIRE(levels >= 1 && levels <= 64 && res >= 1 && res <= 1024, "occ_time_slices: levels=%d res=%d", levels, res);
    CED_REQUIRE(dilate == 0 || dilate == 1, "occ_time_slices: dilate=%d must be 0 or 1", dilate);
    const int64_t need = ced_occ_time_slices_workspace_bytes(n_bins, levels, res);
    CED_REQUIRE(need / 256 < 2147483647 && n <= INT64_MAX / n_bins && (n * n_bins) / 256 < 2147483647,
                "occ_time_slices: too many cells for one launch");
    CED_REQUIRE(workspace && workspace_bytes >= need, "occ_time_slices: workspace too small (%lld < %lld bytes)",
                (long long)workspace_bytes, (long long)need);
    CED_REQUIRE(n == 0 || (cell_ids && max_sigma), "occ_time_slices: null cell_ids/max_sigma");
    const int64_t cells = need / n_bins;
    uint8_t *hit = reinterpret_cast<uint8_t *>(workspace);
    if (n > 0) {
        const int64_t total = n * n_bins;
        hipLaunchKernelGGL(ced::occ_slice_mark_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                           total, cell_ids, max_sigma, step_size, thre, cells, hit);
    }
    if (out)
        hipLaunchKernelGGL(ced::occ_slice_finish_kernel, dim3((unsigned)((need + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           need, cells, (int)res, (int)dilate, hit, union_binaries, out);
    return ced::check_launch("occ_time_slices");
}

extern "C" int ced_occ_cell_points(int64_t n, const int64_t *cell_indices, const float *noise, int32_t res,
                                   const float *aabb_host, float *positions, void *stream)
{
    CED_REQUIRE(n >= 0 && res >= 1, "occ_cell_points: bad sizes");
    if (n == 0) return CED_OK;
    CED_REQUIRE(cell_indices && noise && aabb_host && positions, "occ_cell_points: null pointer");
    hipLaunchKernelGGL(ced::occ_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                       cell_indices, noise, (int)res, aabb_host[0], aabb_host[1], aabb_host[2],
                       aabb_host[3] - aabb_host[0], aabb_host[4] - aabb_host[1], aabb_host[5] - aabb_host[2], positions);
    return ced::check_launch("occ_cell_points");
}

extern "C" int ced_occ_ema_update(int64_t n, const int64_t *cell_ids, const float *density, float step_size,
                                  float ema_decay, float *occs, void *workspace, int64_t workspace_bytes, void *stream)
{
    CED_REQUIRE(n >= 0 && n / 256 < 2147483647, "occ_ema_update: n=%lld outside one launch", (long long)n);
    if (n == 0) return CED_OK;
    CED_REQUIRE(cell_ids && density && occs, "occ_ema_update: null pointer");
    CED_REQUIRE(workspace && workspace_bytes >= n * (int64_t)sizeof(float), "occ_ema_update: workspace too small (%lld < %lld bytes)",
                (long long)workspace_bytes, (long long)(n * (int64_t)sizeof(float)));
    float *decayed = reinterpret_cast<float *>(workspace);
    const dim3 grd((unsigned)((n + 255) / 256)), blk(256);
    hipLaunchKernelGGL(ced::occ_ema_gather_kernel, grd, blk, 0, (hipStream_t)stream, n, cell_ids, ema_decay, occs, decayed);
    hipLaunchKernelGGL(ced::occ_ema_spread_kernel, grd, blk, 0, (hipStream_t)stream, n, cell_ids, decayed, occs);
    hipLaunchKernelGGL(ced::occ_ema_max_kernel, grd, blk, 0, (hipStream_t)stream, n, cell_ids, density, step_size, occs);
    return ced::check_launch("occ_ema_update");
}
