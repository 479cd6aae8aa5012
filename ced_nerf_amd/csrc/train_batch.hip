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
//
// The importance sampler (datasets/dnerf_3d_video_IS.py:401-440, ced_sample_importance_batch) draws k cells of a weight
// map without replacement, as torch.multinomial does: the weight divided by an Exp(1) variate, the k largest.  Per
// candidate j: k = 3 its cell (pool path), k = 4 its variate, unit = ((u >> 9) * 2 + 1) * 2^-24, e = -det_logf(unit),
// key = w / e.  The k largest keys (unsigned bit patterns, ties to the lower j) are found by a three-pass radix select
// and compacted in ascending j; trainset.importance_draws restates it in numpy.
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

// Ray i of the batch is pixel (x, y) of view v: its ray, colour and timestamp.
__device__ __forceinline__ void write_batch_ray(const BatchArgs &A, int64_t i, int32_t v, int32_t x, int32_t y)
{
    if (i == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) A.color_bkgd[c] = A.bkgd[c];
    }
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

__global__ __launch_bounds__(256) void training_batch_kernel(BatchArgs A)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const int32_t v = A.per_ray ? draw_below(batch_draw(A.key, (uint64_t)i, 0u), A.n_views) : A.view0;
    const int32_t x = draw_below(batch_draw(A.key, (uint64_t)i, 1u), A.width);
    const int32_t y = draw_below(batch_draw(A.key, (uint64_t)i, 2u), A.height);
    write_batch_ray(A, i, v, x, y);
}

// ---------------------------------------------------------------------------------------------------------------------
// Importance sampling: k of M candidate cells by the largest key = weight / Exp(1) variate
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kSelectBits[3] = {11, 11, 10};      // the key pattern's digits, most significant first
constexpr int kSelectShift[3] = {21, 10, 0};
constexpr int kSelectBins = 2048;
constexpr int kHistItems = 8;                     // candidates per thread of the key / histogram kernels
constexpr int kTile = 1024;                       // candidates per workgroup of the compaction (4 rounds of 256)

// Workspace header.  threshold: the k-th largest key pattern (its digits are filled in pass by pass); take: how many
// candidates of the current prefix are still to be taken, after the last pass the number of ties at the threshold.
struct SelectState {
    uint32_t hist[3][kSelectBins];
    uint32_t threshold, take, pad[2];
};

struct ImportanceArgs {
    int64_t n_cells, n_cand, k;
    int32_t pooled, sub, wsub, hsub;
    uint32_t key;
    const float *weights;
    SelectState *state;
    uint32_t *keys, *tile_counts;     // keys [n_cand]; tile_counts [2][n_tiles]: above the threshold, at the threshold
    int32_t *selected;                // [k] cells in ascending candidate order
    uint32_t *min_key;                // out: the smallest selected key's pattern (the threshold after the last pass)
    int64_t n_tiles;
};

__device__ __forceinline__ int64_t candidate_cell(const ImportanceArgs &I, int64_t j)
{
    return I.pooled ? (int64_t)draw_below(batch_draw(I.key, (uint64_t)j, 3u), (int32_t)I.n_cells) : j;
}

__device__ __forceinline__ uint32_t candidate_key(const ImportanceArgs &I, int64_t j)
{
    const float w = I.weights[candidate_cell(I, j)];
    if (!(w > 0.0f) || w == __builtin_inff()) return 0u;
    const uint32_t u = batch_draw(I.key, (uint64_t)j, 4u);
    const float unit = (float)((u >> 9) * 2u + 1u) * 5.9604644775390625e-8f;      // odd * 2^-24: exact, in (0, 1)
    const float e = -det_logf(unit);
    return __builtin_bit_cast(uint32_t, w / e);
}

// Pass p of the radix select over the stored keys (pass 0 also makes and stores them): the histogram of digit p among
// the keys whose higher digits equal the threshold's.  LDS counters, flushed with one global atomic per used bin.
template <int PASS>
__global__ __launch_bounds__(256) void select_histogram_kernel(ImportanceArgs I)
{
    __shared__ uint32_t bins[kSelectBins];
    for (int b = threadIdx.x; b < kSelectBins; b += 256) bins[b] = 0u;
    __syncthreads();
    const uint32_t prefix = PASS == 0 ? 0u : I.state->threshold;
    const int64_t base = (int64_t)blockIdx.x * (256 * kHistItems);
#pragma unroll
    for (int r = 0; r < kHistItems; ++r) {
        const int64_t j = base + r * 256 + threadIdx.x;
        if (j >= I.n_cand) break;
        uint32_t key;
        if (PASS == 0) {
            key = candidate_key(I, j);
            I.keys[j] = key;
        } else {
            key = I.keys[j];
        }
        const bool in_prefix = PASS == 0 || (key >> (kSelectShift[PASS] + kSelectBits[PASS])) ==
                                                (prefix >> (kSelectShift[PASS] + kSelectBits[PASS]));
        if (in_prefix) atomicAdd(&bins[(key >> kSelectShift[PASS]) & ((1u << kSelectBits[PASS]) - 1u)], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kSelectBins; b += 256)
        if (bins[b]) atomicAdd(&I.state->hist[PASS][b], bins[b]);
}

// One workgroup: the digit of pass p in which the take-th largest remaining key lies, and how many are left to take in it.
// Each thread adds up the partial sums of the threads before it, a serial loop of at most 255 LDS reads: 2048 bins once
// per pass do not pay for a parallel scan.
template <int PASS>
__global__ __launch_bounds__(256) void select_digit_kernel(ImportanceArgs I)
{
    __shared__ uint32_t part[256];
    constexpr int kPer = kSelectBins / 256;       // bins per thread, thread 0 holding the highest
    const uint32_t *hist = I.state->hist[PASS];
    const uint32_t take = PASS == 0 ? (uint32_t)I.k : I.state->take;
    uint32_t mine[kPer], sum = 0u;
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        mine[q] = hist[kSelectBins - 1 - ((int)threadIdx.x * kPer + q)];
        sum += mine[q];
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    uint32_t above = 0u;                          // keys in the bins of the threads before this one (higher digits)
    for (int t = 0; t < (int)threadIdx.x; ++t) above += part[t];
    __syncthreads();
    if (above < take && above + sum >= take) {    // exactly one thread, when the histogram holds at least `take` keys
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            if (above < take && above + mine[q] >= take) {
                const uint32_t digit = (uint32_t)(kSelectBins - 1 - ((int)threadIdx.x * kPer + q));
                const uint32_t prefix = PASS == 0 ? 0u : I.state->threshold;
                I.state->threshold = prefix | (digit << kSelectShift[PASS]);
                I.state->take = take - above;
                if (PASS == 2) *I.min_key = prefix | digit;
            }
            above += mine[q];
        }
    }
}

__device__ __forceinline__ uint32_t wave_exclusive(bool flag, uint32_t &wave_total)
{
    const unsigned long long ballot = __ballot(flag);
    wave_total = (uint32_t)__popcll(ballot);
    return (uint32_t)__popcll(ballot & ((1ull << (threadIdx.x & 63)) - 1ull));
}

// Per tile of kTile candidates: how many keys lie above the threshold and how many at it.
__global__ __launch_bounds__(256) void select_count_kernel(ImportanceArgs I)
{
    __shared__ uint32_t counts[2];
    if (threadIdx.x < 2) counts[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t threshold = I.state->threshold;
    const int64_t base = (int64_t)blockIdx.x * kTile;
    uint32_t above = 0u, at = 0u;
#pragma unroll
    for (int r = 0; r < kTile / 256; ++r) {
        const int64_t j = base + r * 256 + threadIdx.x;
        const uint32_t key = j < I.n_cand ? I.keys[j] : 0u;
        above += (j < I.n_cand && key > threshold) ? 1u : 0u;
        at += (j < I.n_cand && key == threshold) ? 1u : 0u;
    }
    uint32_t total;
    for (int bit = 0; bit < 3; ++bit) {           // a tile holds at most 4 per thread: three ballots count them
        wave_exclusive((above >> bit) & 1u, total);
        if ((threadIdx.x & 63) == 0 && total) atomicAdd(&counts[0], total << bit);
        wave_exclusive((at >> bit) & 1u, total);
        if ((threadIdx.x & 63) == 0 && total) atomicAdd(&counts[1], total << bit);
    }
    __syncthreads();
    if (threadIdx.x < 2) I.tile_counts[threadIdx.x * I.n_tiles + blockIdx.x] = counts[threadIdx.x];
}

// One workgroup: tile_counts becomes its exclusive prefix sums, in tile order.  Serial per thread over n_tiles / 256
// tiles: 8 per thread for the default pool of 2 000 000 candidates, 8192 for a pool near 2^31 (slow there, still right).
__global__ __launch_bounds__(256) void select_scan_kernel(ImportanceArgs I)
{
    __shared__ uint32_t part[2][256];
    const int64_t per = (I.n_tiles + 255) / 256;
    const int64_t first = (int64_t)threadIdx.x * per, last = first + per < I.n_tiles ? first + per : I.n_tiles;
    for (int w = 0; w < 2; ++w) {
        uint32_t sum = 0u;
        for (int64_t t = first; t < last; ++t) sum += I.tile_counts[w * I.n_tiles + t];
        part[w][threadIdx.x] = sum;
    }
    __syncthreads();
    for (int w = 0; w < 2; ++w) {
        uint32_t run = 0u;
        for (int t = 0; t < (int)threadIdx.x; ++t) run += part[w][t];
        for (int64_t t = first; t < last; ++t) {
            const uint32_t c = I.tile_counts[w * I.n_tiles + t];
            I.tile_counts[w * I.n_tiles + t] = run;
            run += c;
        }
    }
}

// The selected candidates (key above the threshold, or at it among the first `take` such) in ascending j: each one's
// place is the number of selected candidates before it.
__global__ __launch_bounds__(256) void select_compact_kernel(ImportanceArgs I)
{
    __shared__ uint32_t wave_sum[2][4];
    const uint32_t threshold = I.state->threshold, take = I.state->take;
    const uint32_t ties_before_tile = I.tile_counts[I.n_tiles + blockIdx.x];
    uint32_t ties = ties_before_tile;                                        // ties at the threshold before this round
    uint32_t place = I.tile_counts[blockIdx.x] + (ties_before_tile < take ? ties_before_tile : take);
    const int wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * kTile;
    for (int r = 0; r < kTile / 256; ++r) {
        const int64_t j = base + r * 256 + threadIdx.x;
        const uint32_t key = j < I.n_cand ? I.keys[j] : 0u;
        const bool tie = j < I.n_cand && key == threshold;
        uint32_t total;
        const uint32_t tie_lane = wave_exclusive(tie, total);
        if ((threadIdx.x & 63) == 0) wave_sum[0][wave] = total;
        __syncthreads();
        uint32_t tie_rank = ties + tie_lane, ties_round = 0u;
        for (int w = 0; w < 4; ++w) {
            tie_rank += w < wave ? wave_sum[0][w] : 0u;
            ties_round += wave_sum[0][w];
        }
        const bool chosen = j < I.n_cand && (key > threshold || (tie && tie_rank < take));
        const uint32_t lane_place = wave_exclusive(chosen, total);
        if ((threadIdx.x & 63) == 0) wave_sum[1][wave] = total;
        __syncthreads();
        uint32_t at = place + lane_place, chosen_round = 0u;
        for (int w = 0; w < 4; ++w) {
            at += w < wave ? wave_sum[1][w] : 0u;
            chosen_round += wave_sum[1][w];
        }
        if (chosen && (int64_t)at < I.k) I.selected[at] = (int32_t)candidate_cell(I, j);
        ties += ties_round;
        place += chosen_round;
    }
}

// Ray (ah * s + aw) * k + i is pixel (xsub * s + aw, ysub * s + ah) of the i-th selected cell's view
// (dnerf_3d_video_IS.py:426-440).
__global__ __launch_bounds__(256) void importance_batch_kernel(BatchArgs A, ImportanceArgs I)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= A.n) return;
    const int64_t a = r / I.k, i = r - a * I.k;
    const int32_t ah = (int32_t)(a / I.sub), aw = (int32_t)(a - (int64_t)ah * I.sub);
    int32_t cell = I.selected[i];
    cell = cell < 0 ? 0 : cell < (int32_t)I.n_cells ? cell : (int32_t)I.n_cells - 1;      // in bounds whatever was selected
    const int32_t per_view = I.hsub * I.wsub;
    const int32_t v = cell / per_view;
    const int32_t rem = cell - v * per_view;
    const int32_t ysub = rem / I.wsub, xsub = rem - ysub * I.wsub;
    write_batch_ray(A, r, v, xsub * I.sub + aw, ysub * I.sub + ah);
}

static int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

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

static int importance_sizes(const char *what, int64_t n_cells, int64_t pool_size, int64_t k, int64_t *n_cand)
{
    CED_REQUIRE(n_cells >= 1 && n_cells < ((int64_t)1 << 31), "%s: the weight map must have 1 .. 2^31 - 1 cells, got %lld",
                what, (long long)n_cells);
    CED_REQUIRE(pool_size >= 1 && pool_size < ((int64_t)1 << 31), "%s: bad pool size %lld", what, (long long)pool_size);
    *n_cand = n_cells <= pool_size ? n_cells : pool_size;
    CED_REQUIRE(k >= 1 && k <= *n_cand, "%s: cannot draw %lld cells from %lld candidates", what, (long long)k,
                (long long)*n_cand);
    return CED_OK;
}

extern "C" int64_t ced_importance_batch_workspace_bytes(int64_t n_cells, int64_t pool_size, int64_t k)
{
    int64_t n_cand = 0;
    if (importance_sizes("importance_batch_workspace_bytes", n_cells, pool_size, k, &n_cand) != CED_OK) return -1;
    const int64_t n_tiles = (n_cand + ced::kTile - 1) / ced::kTile;
    return ced::align256((int64_t)sizeof(ced::SelectState)) + ced::align256(4 * n_cand) + ced::align256(8 * n_tiles) +
           ced::align256(4 * k);
}

extern "C" int ced_sample_importance_batch(int32_t camera_model, int32_t n_views, int32_t width, int32_t height,
                                           int32_t channels, const uint8_t *images, const float *cameras,
                                           const float *view_timestamps, const float *weights, int32_t weights_subsampled,
                                           int64_t pool_size, int64_t num_cells, uint64_t seed, int64_t step,
                                           int32_t bkgd_mode, float *origins, float *viewdirs, float *pixels,
                                           float *timestamps, float *color_bkgd, int32_t *indices, uint32_t *min_key,
                                           void *workspace, int64_t workspace_bytes, void *stream)
{
    CED_REQUIRE(camera_model == CED_CAMERA_PINHOLE || camera_model == CED_CAMERA_HYPERCAM,
                "sample_importance_batch: unknown camera model %d", camera_model);
    CED_REQUIRE(n_views > 0 && width > 0 && height > 0, "sample_importance_batch: bad view count or image size");
    CED_REQUIRE(channels == 3, "sample_importance_batch: channels must be 3 (RGB), got %d", channels);
    CED_REQUIRE(weights_subsampled >= 1 && weights_subsampled <= width && weights_subsampled <= height,
                "sample_importance_batch: bad weights_subsampled %d for %d x %d images", weights_subsampled, width, height);
    CED_REQUIRE(bkgd_mode == CED_BKGD_WHITE || bkgd_mode == CED_BKGD_BLACK || bkgd_mode == CED_BKGD_RANDOM,
                "sample_importance_batch: bad background mode %d", bkgd_mode);
    const int32_t s = weights_subsampled, hsub = height / s, wsub = width / s;
    const int64_t n_cells = (int64_t)n_views * hsub * wsub;
    int64_t n_cand = 0;
    if (int rc = importance_sizes("sample_importance_batch", n_cells, pool_size, num_cells, &n_cand)) return rc;
    const int64_t num_rays = num_cells * s * s;
    CED_REQUIRE((num_rays + 255) / 256 <= 0x7fffffff, "sample_importance_batch: bad ray count %lld", (long long)num_rays);
    CED_REQUIRE(images && cameras && view_timestamps && weights && origins && viewdirs && pixels && timestamps &&
                    color_bkgd && min_key && workspace,
                "sample_importance_batch: null pointer");
    CED_REQUIRE(((uintptr_t)workspace & 15) == 0, "sample_importance_batch: workspace must be 16-byte aligned");
    CED_REQUIRE(workspace_bytes >= ced_importance_batch_workspace_bytes(n_cells, pool_size, num_cells),
                "sample_importance_batch: workspace of %lld bytes is too small", (long long)workspace_bytes);
    ced::BatchArgs A{};
    A.n = num_rays;
    A.model = camera_model; A.n_views = n_views; A.width = width; A.height = height; A.channels = channels;
    A.key = ced::batch_key(seed, (uint64_t)step);
    const uint64_t batch_ray = ~(uint64_t)0;
    for (int c = 0; c < 3; ++c)
        A.bkgd[c] = bkgd_mode == CED_BKGD_WHITE ? 1.0f : bkgd_mode == CED_BKGD_BLACK ? 0.0f
                  : ced::draw_unit(ced::batch_draw(A.key, batch_ray, 1u + (uint32_t)c));
    A.images = images; A.cameras = cameras; A.view_ts = view_timestamps;
    A.origins = origins; A.viewdirs = viewdirs; A.pixels = pixels; A.timestamps = timestamps; A.color_bkgd = color_bkgd;
    A.indices = indices;
    ced::ImportanceArgs I{};
    I.n_cells = n_cells; I.n_cand = n_cand; I.k = num_cells;
    I.pooled = n_cells > pool_size ? 1 : 0;
    I.sub = s; I.wsub = wsub; I.hsub = hsub;
    I.key = A.key;
    I.weights = weights;
    I.min_key = min_key;
    I.n_tiles = (n_cand + ced::kTile - 1) / ced::kTile;
    char *ws = (char *)workspace;
    I.state = (ced::SelectState *)ws;            ws += ced::align256((int64_t)sizeof(ced::SelectState));
    I.keys = (uint32_t *)ws;                     ws += ced::align256(4 * n_cand);
    I.tile_counts = (uint32_t *)ws;              ws += ced::align256(8 * I.n_tiles);
    I.selected = (int32_t *)ws;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(I.state, 0, sizeof(ced::SelectState), st) != hipSuccess)
        return ced::check_launch("sample_importance_batch (workspace reset)");
    const dim3 hist_grid((unsigned)((n_cand + 256 * ced::kHistItems - 1) / (256 * ced::kHistItems)));
    const dim3 tile_grid((unsigned)I.n_tiles);
    hipLaunchKernelGGL(ced::select_histogram_kernel<0>, hist_grid, dim3(256), 0, st, I);
    hipLaunchKernelGGL(ced::select_digit_kernel<0>, dim3(1), dim3(256), 0, st, I);
    hipLaunchKernelGGL(ced::select_histogram_kernel<1>, hist_grid, dim3(256), 0, st, I);
    hipLaunchKernelGGL(ced::select_digit_kernel<1>, dim3(1), dim3(256), 0, st, I);
    hipLaunchKernelGGL(ced::select_histogram_kernel<2>, hist_grid, dim3(256), 0, st, I);
    hipLaunchKernelGGL(ced::select_digit_kernel<2>, dim3(1), dim3(256), 0, st, I);
    hipLaunchKernelGGL(ced::select_count_kernel, tile_grid, dim3(256), 0, st, I);
    hipLaunchKernelGGL(ced::select_scan_kernel, dim3(1), dim3(256), 0, st, I);
    hipLaunchKernelGGL(ced::select_compact_kernel, tile_grid, dim3(256), 0, st, I);
    hipLaunchKernelGGL(ced::importance_batch_kernel, dim3((unsigned)((num_rays + 255) / 256)), dim3(256), 0, st, A, I);
    return ced::check_launch("sample_importance_batch");
}
