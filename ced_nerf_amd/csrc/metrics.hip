// Image metrics of the reference's evaluation step (train_real.py:494-500): SSIM / MS-SSIM as pytorch_msssim 1.0.0
// computes them (ssim, ms_ssim with the package defaults), and the per-image MSE of the PSNR, over a batch of N images
// of C channels.
//
// One level of the pyramid is one launch, a workgroup per (image, channel, tile of TH x TW valid outputs).  The workgroup
// stages its input tile plus a halo of X and Y in LDS (win - 1 rows and columns, at least 1: see the pooling below), runs
// the separable Gaussian (valid convolution: along W for the staged rows, then along H) over the five moments X, Y, X^2, Y^2, XY in fp64, forms the cs and
// ssim maps and reduces them to one fp64 partial per workgroup.  Before the last level it also writes the 2x2 average
// pool of its inputs (torch's avg_pool2d(2, stride 2, padding (H%2, W%2)), count_include_pad: the zero row / column of
// an odd side enters the division by 4) into the next level's buffer in the workspace.  Ownership of the pooled outputs:
// the tile of rows [y0, y0 + TH) owns the pooled rows whose first input row 2i - pad_h lies in its rows, tile 0 also the
// one that starts at the padding row -1, the last tile every row down to H (the last tile's staged rows reach H - 1 because
// the tiles cover the valid outputs).  The same for columns.  Every pooled pixel thus has exactly one writer, and the
// rows it reads (f, f + 1 <= y0 + TH) are staged: the halo is at least one row and column, also for win == 1.  Level 0's pass also sums (x - y)^2 over the input pixels the tile
// owns (the same ownership, without the pooling's pairing), in fp64: the MSE of the PSNR.
//
// Level 0 reads X and Y (fp32) through element strides (n, c, h, w): an [H,W,3] render permuted to [1,3,H,W] is read in
// place.  Levels 1+ are contiguous [N,C,H_l,W_l] fp64 in the workspace: rounding the pooled images to fp32 moved the
// deeper levels' cs by up to 6e-6 on random images (a 13x15 level of 16x16-pixel averages has sigma^2 ~ C2).
//
// Precision: the tiles are staged as fp64 and the filtered moments are fp64 sums (fused multiply-adds) of exact fp64
// products, so sigma^2 = E[x^2] - mu^2 keeps ~1e-16 beside C2 = 9e-4 in flat regions.
// Determinism: no atomics; every partial is summed in a fixed order (per-wave butterfly, then the waves in order), and
// the finishing launches sum the partials of one (image, level, channel) in a fixed order that depends only on that
// image's sizes: image i's bits do not depend on the rest of the batch, and two calls give the same bits.
#include "ced_common.hpp"

#include <cmath>

namespace ced {

constexpr int kTileW = 32, kTileH = 16;
constexpr int kLevelThreads = 256;         // 4 waves; a tile is 512 outputs, two per lane
constexpr int kFinishThreads = 256;
constexpr int kMaxWin = 15;                // LDS: (kTileH + 14) x kTileW x 5 + 2 x (kTileH + 14) x (kTileW + 14) fp64 = 59 KiB
constexpr int kMaxLevels = 5;

// rows / columns staged beyond the tile: the window's win - 1, at least 1 in a pyramid pass (a tile's last pooled row
// reads row y0 + TH), none in the MSE-only pass (no window, no pooling)
__host__ __device__ constexpr int stage_halo(bool ssim, int win) { return ssim ? (win > 2 ? win - 1 : 1) : 0; }

struct LevelArgs {
    int64_t n, c;                          // images, channels
    int32_t h, w;                          // this level's sides
    int32_t win;                           // window size (odd); 1 for the MSE-only pass
    int32_t tiles_x, tiles_y;
    int32_t nh, nw, pad_h, pad_w;          // next level's sides and this level's pooling pads (nh == 0: no pooling)
    const void *x, *y;                     // level 0: float, levels 1+: double
    int64_t sx[4], sy[4];                  // element strides (n, c, h, w)
    double *nx, *ny;                       // next level, [N,C,nh,nw]
    double c1, c2;
    double g[kMaxWin];                     // the float32 window, exactly
    double *part;                          // [N][C][tiles][2]: sums of the cs and ssim maps (NULL: MSE only)
    double *mse_part;                      // [N][C][tiles]: sums of (x - y)^2 (NULL: not this level)
};

__device__ __forceinline__ double wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, kWave);
    return v;
}

// fixed-order workgroup sum of kLevelThreads lanes (lane 0 of wave 0 holds the result)
__device__ __forceinline__ double block_sum(double v, double *s_red)
{
    v = wave_sum(v);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) s_red[wave] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int k = 0; k < kLevelThreads / kWave; ++k) s = s + s_red[k];
    __syncthreads();
    return s;
}

// one pyramid level (kSsim) or the plain MSE pass (!kSsim, win == 1: a tile is its own input rows and columns)
template <bool kSsim, typename TIn>
__global__ __launch_bounds__(kLevelThreads) void ssim_level_kernel(const LevelArgs a)
{
    extern __shared__ double smem[];
    __shared__ double s_red[kLevelThreads / kWave];
    const int win = a.win;
    const int RH = kTileH + stage_halo(kSsim, win), RW = kTileW + stage_halo(kSsim, win);
    double *s_h = smem;                                                  // [5][RH][kTileW] (kSsim)
    double *s_x = smem + (kSsim ? 5 * RH * kTileW : 0);                  // [RH][RW]
    double *s_y = s_x + RH * RW;

    const int tile = blockIdx.x;
    const int64_t ci = blockIdx.y, ni = blockIdx.z;
    const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
    const int x0 = tx * kTileW, y0 = ty * kTileH;
    const TIn *X = (const TIn *)a.x + ni * a.sx[0] + ci * a.sx[1];
    const TIn *Y = (const TIn *)a.y + ni * a.sy[0] + ci * a.sy[1];

    for (int i = threadIdx.x; i < RH * RW; i += kLevelThreads) {
        const int r = i / RW, q = i - r * RW;
        const int yy = y0 + r, xx = x0 + q;
        double vx = 0.0, vy = 0.0;
        if (yy < a.h && xx < a.w) {
            vx = (double)X[yy * a.sx[2] + xx * a.sx[3]];
            vy = (double)Y[yy * a.sy[2] + xx * a.sy[3]];
        }
        s_x[i] = vx;
        s_y[i] = vy;
    }
    __syncthreads();

    // the input rows / columns this tile owns: [y0, y_end) x [x0, x_end)
    const int y_end = ty == a.tiles_y - 1 ? a.h : y0 + kTileH;
    const int x_end = tx == a.tiles_x - 1 ? a.w : x0 + kTileW;
    const size_t plane = (size_t)(ni * a.c + ci);
    const size_t n_tiles = (size_t)a.tiles_x * a.tiles_y;

    if (a.mse_part) {
        const int oh = y_end - y0, ow = x_end - x0;
        double sse = 0.0;
        for (int i = threadIdx.x; i < oh * ow; i += kLevelThreads) {
            const int r = i / ow, q = i - r * ow;
            const double d = s_x[r * RW + q] - s_y[r * RW + q];
            sse = sse + d * d;
        }
        sse = block_sum(sse, s_red);
        if (threadIdx.x == 0) a.mse_part[plane * n_tiles + tile] = sse;
    }
    if (!kSsim) return;

    // horizontal pass: RH staged rows x kTileW output columns, five moments
    for (int i = threadIdx.x; i < RH * kTileW; i += kLevelThreads) {
        const int r = i / kTileW, j = i - r * kTileW;
        const double *px = s_x + r * RW + j, *py = s_y + r * RW + j;
        double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
        for (int k = 0; k < win; ++k) {
            const double g = a.g[k], xv = px[k], yv = py[k];
            m0 = __builtin_fma(g, xv, m0);
            m1 = __builtin_fma(g, yv, m1);
            m2 = __builtin_fma(g, xv * xv, m2);
            m3 = __builtin_fma(g, yv * yv, m3);
            m4 = __builtin_fma(g, xv * yv, m4);
        }
        s_h[(0 * RH + r) * kTileW + j] = m0;
        s_h[(1 * RH + r) * kTileW + j] = m1;
        s_h[(2 * RH + r) * kTileW + j] = m2;
        s_h[(3 * RH + r) * kTileW + j] = m3;
        s_h[(4 * RH + r) * kTileW + j] = m4;
    }
    __syncthreads();

    // vertical pass and the two maps over the valid outputs of the tile
    const int ho = a.h - win + 1, wo = a.w - win + 1;
    double cs_sum = 0.0, ss_sum = 0.0;
    for (int i = threadIdx.x; i < kTileH * kTileW; i += kLevelThreads) {
        const int r = i / kTileW, j = i - r * kTileW;
        if (y0 + r >= ho || x0 + j >= wo) continue;
        double v[5];
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            const double *col = s_h + (m * RH + r) * kTileW + j;
            double s = 0.0;
            for (int k = 0; k < win; ++k) s = __builtin_fma(a.g[k], col[k * kTileW], s);
            v[m] = s;
        }
        const double mu_xy = v[0] * v[1], mu_xx = v[0] * v[0], mu_yy = v[1] * v[1];
        const double s_xx = v[2] - mu_xx, s_yy = v[3] - mu_yy, s_xy = v[4] - mu_xy;
        const double cs = (2.0 * s_xy + a.c2) / (s_xx + s_yy + a.c2);
        const double ss = ((2.0 * mu_xy + a.c1) / (mu_xx + mu_yy + a.c1)) * cs;
        cs_sum = cs_sum + cs;
        ss_sum = ss_sum + ss;
    }
    cs_sum = block_sum(cs_sum, s_red);
    ss_sum = block_sum(ss_sum, s_red);
    if (threadIdx.x == 0) {
        a.part[(plane * n_tiles + tile) * 2 + 0] = cs_sum;
        a.part[(plane * n_tiles + tile) * 2 + 1] = ss_sum;
    }

    // 2x2 average pool of the owned inputs into the next level
    if (a.nh == 0) return;
    const int i_lo = ty == 0 ? 0 : (y0 + a.pad_h + 1) / 2, i_hi = (y_end + a.pad_h + 1) / 2;
    const int k_lo = tx == 0 ? 0 : (x0 + a.pad_w + 1) / 2, k_hi = (x_end + a.pad_w + 1) / 2;
    const int pw = k_hi - k_lo;
    double *NX = a.nx + plane * a.nh * a.nw, *NY = a.ny + plane * a.nh * a.nw;
    for (int i = threadIdx.x; i < (i_hi - i_lo) * pw; i += kLevelThreads) {
        const int pi = i_lo + i / pw, pk = k_lo + i % pw;
        const int r = 2 * pi - a.pad_h - y0, q = 2 * pk - a.pad_w - x0;   // >= -1 (the padding row / column of tile 0)
        double sx = 0.0, sy = 0.0;
#pragma unroll
        for (int dr = 0; dr < 2; ++dr)
#pragma unroll
            for (int dq = 0; dq < 2; ++dq) {
                if (r + dr < 0 || q + dq < 0) continue;
                sx = sx + s_x[(r + dr) * RW + q + dq];
                sy = sy + s_y[(r + dr) * RW + q + dq];
            }
        NX[(size_t)pi * a.nw + pk] = sx * 0.25;
        NY[(size_t)pi * a.nw + pk] = sy * 0.25;
    }
}

struct FinishArgs {
    int64_t c;
    int32_t levels;                        // 0: MSE only
    int32_t ms;                            // 1: the MS-SSIM product, 0: single-scale SSIM
    int32_t nonnegative;
    int64_t tiles[kMaxLevels];
    int64_t part_off[kMaxLevels];          // offset of each level's partials (doubles)
    int64_t mse_tiles;
    double weights[kMaxLevels];
    double inv_valid[kMaxLevels];          // 1 / the valid outputs of a level, (h - win + 1)(w - win + 1)
    double inv_count;                      // 1 / (C H W)
    const double *part, *mse_part;
    double *lvl;                           // [N][levels][C][2]: the means of cs and ssim
    double *img;                           // [N] fp64 per-image result
    float *per_image;
    double *mse, *level_means;             // [N]; [levels][N][C][2]
};

// one workgroup per (task, image), all lanes on one sum in a fixed order: task t < levels C sums the cs and ssim
// partials of (level t / C, channel t % C), task levels C the squared errors of the image
__global__ __launch_bounds__(kFinishThreads) void ssim_sum_kernel(const FinishArgs a)
{
    __shared__ double s_red[kFinishThreads / kWave];
    const int64_t t = blockIdx.x, ni = blockIdx.y, n = gridDim.y;
    if (t == (int64_t)a.levels * a.c) {
        const double *p = a.mse_part + ni * a.c * a.mse_tiles;
        double s = 0.0;
        for (int64_t k = threadIdx.x; k < a.c * a.mse_tiles; k += kFinishThreads) s = s + p[k];
        s = block_sum(s, s_red);
        if (threadIdx.x == 0 && a.mse) a.mse[ni] = s * a.inv_count;
        return;
    }
    const int l = (int)(t / a.c);
    const int64_t ci = t - (int64_t)l * a.c;
    const double *p = a.part + a.part_off[l] + (ni * a.c + ci) * a.tiles[l] * 2;
    double cs = 0.0, ss = 0.0;
    for (int64_t k = threadIdx.x; k < a.tiles[l]; k += kFinishThreads) {
        cs = cs + p[2 * k];
        ss = ss + p[2 * k + 1];
    }
    cs = block_sum(cs, s_red);
    ss = block_sum(ss, s_red);
    if (threadIdx.x == 0) {
        double *o = a.lvl + ((ni * a.levels + l) * a.c + ci) * 2;
        o[0] = cs * a.inv_valid[l];
        o[1] = ss * a.inv_valid[l];
        if (a.level_means) {
            a.level_means[((l * n + ni) * a.c + ci) * 2 + 0] = o[0];
            a.level_means[((l * n + ni) * a.c + ci) * 2 + 1] = o[1];
        }
    }
}

// one workgroup: lane k forms the result of images k, k + 256, ... (the product over the levels, the mean over the
// channels), then lane 0 sums the images in order for the mean (mean may be NULL)
__global__ __launch_bounds__(kFinishThreads) void ssim_product_kernel(const FinishArgs a, int64_t n, float *__restrict__ mean)
{
    for (int64_t ni = threadIdx.x; ni < n; ni += kFinishThreads) {
        double acc = 0.0;
        for (int64_t ci = 0; ci < a.c; ++ci) {
            double v;
            if (a.ms) {
                v = 1.0;
                for (int l = 0; l < a.levels; ++l) {
                    const double *o = a.lvl + ((ni * a.levels + l) * a.c + ci) * 2;
                    const double x = l < a.levels - 1 ? o[0] : o[1];
                    v = v * pow(x > 0.0 ? x : 0.0, a.weights[l]);
                }
            } else {
                v = a.lvl[(ni * a.levels * a.c + ci) * 2 + 1];
                if (a.nonnegative) v = v > 0.0 ? v : 0.0;
            }
            acc = acc + v;
        }
        acc = acc / (double)a.c;
        a.img[ni] = acc;
        a.per_image[ni] = (float)acc;
    }
    if (!mean) return;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) s = s + a.img[i];
    mean[0] = (float)(s / (double)n);
}

// sizes of the pyramid and the workspace
struct Plan {
    int levels;                            // levels of SSIM (0: MSE only)
    int win;                               // window of the level passes (1 in the MSE-only pass)
    int64_t h[kMaxLevels], w[kMaxLevels], tiles_x[kMaxLevels], tiles_y[kMaxLevels];
    int64_t part_off[kMaxLevels], part_doubles, mse_off, lvl_off, img_off, doubles;
    int64_t pyr_off[kMaxLevels];           // byte offsets of the pooled levels 1.. (X then Y)
    int64_t bytes;
};

static int make_plan(const char *what, int64_t n, int64_t c, int64_t h, int64_t w, int32_t win, int32_t levels, Plan &p)
{
    CED_REQUIRE(n >= 1 && c >= 1 && h >= 1 && w >= 1, "%s: empty or negative size (n %lld, c %lld, h %lld, w %lld)", what,
                (long long)n, (long long)c, (long long)h, (long long)w);
    CED_REQUIRE(n <= 65535 && c <= 65535, "%s: at most 65535 images and 65535 channels", what);
    CED_REQUIRE(h < (1ll << 31) && w < (1ll << 31), "%s: a side of 2^31 or more (h %lld, w %lld)", what, (long long)h,
                (long long)w);
    CED_REQUIRE(levels >= 0 && levels <= kMaxLevels, "%s: levels must be 0..%d, got %d", what, kMaxLevels, levels);
    p.levels = levels;
    p.win = levels == 0 ? 1 : win;
    if (levels > 0)
        CED_REQUIRE(win >= 1 && win <= kMaxWin && win % 2 == 1, "%s: win_size must be odd and at most %d, got %d", what, kMaxWin,
                    win);
    int64_t hh = h, ww = w;
    const int passes = levels == 0 ? 1 : levels;
    int64_t off = 0;
    for (int l = 0; l < passes; ++l) {
        CED_REQUIRE(hh >= p.win && ww >= p.win, "%s: level %d is %lldx%lld, smaller than the %d-wide window", what, l,
                    (long long)hh, (long long)ww, p.win);
        p.h[l] = hh;
        p.w[l] = ww;
        p.tiles_y[l] = (hh - p.win + 1 + kTileH - 1) / kTileH;
        p.tiles_x[l] = (ww - p.win + 1 + kTileW - 1) / kTileW;
        CED_REQUIRE(p.tiles_x[l] * p.tiles_y[l] < (1ll << 31), "%s: image too large", what);
        p.part_off[l] = off;
        if (levels > 0) off += n * c * p.tiles_x[l] * p.tiles_y[l] * 2;
        hh = (hh + 1) / 2;                 // avg_pool2d(2, 2, padding = side % 2): ceil(side / 2)
        ww = (ww + 1) / 2;
    }
    p.part_doubles = off;
    p.mse_off = off;
    off += n * c * p.tiles_x[0] * p.tiles_y[0];
    p.lvl_off = off;
    off += n * (levels > 0 ? levels : 1) * c * 2;
    p.img_off = off;
    off += n;
    p.doubles = off;
    int64_t bytes = off * 8;
    for (int l = 1; l < levels; ++l) {
        p.pyr_off[l] = bytes;
        bytes += 2 * n * c * p.h[l] * p.w[l] * 8;
        bytes = (bytes + 255) & ~(int64_t)255;
    }
    p.bytes = bytes;
    return CED_OK;
}

static size_t level_lds_bytes(bool ssim, int win)
{
    const int RH = kTileH + stage_halo(ssim, win), RW = kTileW + stage_halo(ssim, win);
    return (ssim ? (size_t)5 * RH * kTileW * 8 : 0) + (size_t)2 * RH * RW * 8;
}

}  // namespace ced

extern "C" int64_t ced_ssim_workspace_bytes(int64_t n, int64_t c, int64_t h, int64_t w, int32_t win_size, int32_t levels)
{
    ced::Plan p;
    const int rc = ced::make_plan("ssim_workspace_bytes", n, c, h, w, win_size, levels, p);
    return rc != CED_OK ? rc : p.bytes;
}

extern "C" int ced_ssim(int64_t n, int64_t c, int64_t h, int64_t w, const float *x, const int64_t *x_strides, const float *y,
                        const int64_t *y_strides, double data_range, double k1, double k2, int32_t win_size, const float *win,
                        int32_t levels, const float *weights, int32_t nonnegative, float *per_image, float *mean, double *mse,
                        double *level_means, void *workspace, void *stream)
{
    using namespace ced;
    Plan p;
    const int rc = make_plan("ssim", n, c, h, w, win_size, levels, p);
    if (rc != CED_OK) return rc;
    CED_REQUIRE(x && y && x_strides && y_strides && workspace, "ssim: null pointer");
    CED_REQUIRE(levels > 0 ? (per_image && win) : (mse && !mean && !level_means), "ssim: null pointer (levels %d)", levels);
    CED_REQUIRE(levels <= 1 || weights, "ssim: null pointer (weights of %d levels)", levels);
    CED_REQUIRE(((uintptr_t)workspace & 7) == 0, "ssim: workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double *ws = (double *)workspace;

    LevelArgs a{};
    a.n = n;
    a.c = c;
    a.win = p.win;
    a.c1 = (k1 * data_range) * (k1 * data_range);
    a.c2 = (k2 * data_range) * (k2 * data_range);
    for (int k = 0; k < p.win && levels > 0; ++k) a.g[k] = (double)win[k];
    if (levels == 0) a.g[0] = 1.0;
    const void *cx = x, *cy = y;
    for (int k = 0; k < 4; ++k) {
        a.sx[k] = x_strides[k];
        a.sy[k] = y_strides[k];
    }
    const int passes = levels == 0 ? 1 : levels;
    for (int l = 0; l < passes; ++l) {
        a.h = (int32_t)p.h[l];
        a.w = (int32_t)p.w[l];
        a.tiles_x = (int32_t)p.tiles_x[l];
        a.tiles_y = (int32_t)p.tiles_y[l];
        a.x = cx;
        a.y = cy;
        a.part = levels > 0 ? ws + p.part_off[l] : nullptr;
        a.mse_part = l == 0 ? ws + p.mse_off : nullptr;
        if (l + 1 < levels) {
            a.nh = (int32_t)p.h[l + 1];
            a.nw = (int32_t)p.w[l + 1];
            a.pad_h = (int32_t)(p.h[l] % 2);
            a.pad_w = (int32_t)(p.w[l] % 2);
            a.nx = (double *)((char *)workspace + p.pyr_off[l + 1]);
            a.ny = a.nx + n * c * p.h[l + 1] * p.w[l + 1];
        } else {
            a.nh = a.nw = a.pad_h = a.pad_w = 0;
            a.nx = a.ny = nullptr;
        }
        const dim3 grid((unsigned)(p.tiles_x[l] * p.tiles_y[l]), (unsigned)c, (unsigned)n);
        if (levels == 0)
            hipLaunchKernelGGL((ssim_level_kernel<false, float>), grid, dim3(kLevelThreads), level_lds_bytes(false, 1), st, a);
        else if (l == 0)
            hipLaunchKernelGGL((ssim_level_kernel<true, float>), grid, dim3(kLevelThreads), level_lds_bytes(true, p.win), st, a);
        else
            hipLaunchKernelGGL((ssim_level_kernel<true, double>), grid, dim3(kLevelThreads), level_lds_bytes(true, p.win), st,
                               a);
        if (a.nh == 0) continue;
        // the next level: contiguous [N,C,nh,nw]
        cx = a.nx;
        cy = a.ny;
        a.sx[0] = a.sy[0] = c * p.h[l + 1] * p.w[l + 1];
        a.sx[1] = a.sy[1] = p.h[l + 1] * p.w[l + 1];
        a.sx[2] = a.sy[2] = p.w[l + 1];
        a.sx[3] = a.sy[3] = 1;
    }

    FinishArgs f{};
    f.c = c;
    f.levels = levels;
    f.ms = weights != nullptr;
    f.nonnegative = nonnegative;
    for (int l = 0; l < levels; ++l) {
        f.tiles[l] = p.tiles_x[l] * p.tiles_y[l];
        f.part_off[l] = p.part_off[l];
        f.weights[l] = weights ? (double)weights[l] : 0.0;
        f.inv_valid[l] = 1.0 / ((double)(p.h[l] - p.win + 1) * (double)(p.w[l] - p.win + 1));
    }
    f.mse_tiles = p.tiles_x[0] * p.tiles_y[0];
    f.inv_count = 1.0 / ((double)c * (double)h * (double)w);
    f.part = ws;
    f.mse_part = ws + p.mse_off;
    f.lvl = ws + p.lvl_off;
    f.img = ws + p.img_off;
    f.per_image = per_image;
    f.mse = mse;
    f.level_means = level_means;
    hipLaunchKernelGGL(ssim_sum_kernel, dim3((unsigned)(levels * c + 1), (unsigned)n), dim3(kFinishThreads), 0, st, f);
    if (levels > 0) hipLaunchKernelGGL(ssim_product_kernel, dim3(1), dim3(kFinishThreads), 0, st, f, n, mean);
    return check_launch("ssim");
}
