// Volume export (vis.py:13-46): the cells of a reso^3 grid over the field's bounding cube that are worth evaluating
// (ced_bake_candidates) and, of those, the ones whose density reaches the threshold (ced_bake_select).  The density in
// between is the existing ced_field_forward on the candidates' centres, so every arithmetic mode gives query_density's
// bits.  The colour afterwards is ced_field_rgb_bcast (field_move.hip).
//
// Both entries are stream compactions whose output order is the input order -- the flat cell index ascends -- so no
// output slot is claimed atomically.  Three launches: every workgroup counts its kKeepItems items; one workgroup turns the
// counts into exclusive offsets and the total; every workgroup evaluates its items again and writes each kept one at
// offset + rank, the rank from a wavefront ballot (lanes below) plus the workgroup's earlier waves and rounds.  The
// predicate is one byte or one float per item, evaluating it twice costs less than keeping it.
#include "ced_common.hpp"
#include "march_core.hpp"

namespace ced {

constexpr int kKeepThreads = 256;
constexpr int kKeepRounds = 4;
constexpr int kKeepItems = kKeepThreads * kKeepRounds;          // items per workgroup, in rounds of consecutive items
constexpr int kScanThreads = 1024;

// Op: bool keep(int64_t k) and void write(int64_t k, int64_t slot) over items k = 0 .. n-1.  WRITE = false: blocks[b] =
// kept items of workgroup b.  WRITE = true: blocks[b] is the number kept before workgroup b; slots >= capacity are dropped.
template <class Op, bool WRITE>
__global__ __launch_bounds__(kKeepThreads) void keep_kernel(Op op, int64_t n, int64_t *__restrict__ blocks, int64_t capacity)
{
    constexpr int WAVES = kKeepThreads / kWave;
    __shared__ int wave_kept[2][WAVES];                             // two buffers: one barrier per round
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t base = (int64_t)blockIdx.x * kKeepItems;
    const int64_t first_slot = WRITE ? blocks[blockIdx.x] : 0;
    int kept_so_far = 0;
    for (int r = 0; r < kKeepRounds; ++r) {
        const int64_t k = base + r * kKeepThreads + tid;
        const bool keep = k < n && op.keep(k);
        const unsigned long long mask = __ballot(keep);
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        if (lane == 0) wave_kept[r & 1][wave] = __popcll(mask);
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const int v = wave_kept[r & 1][w];
            before += w < wave ? v : 0;
            all += v;
        }
        if (WRITE && keep) {
            const int64_t slot = first_slot + kept_so_far + before + rank;
            if (slot < capacity) op.write(k, slot);
        }
        kept_so_far += all;
    }
    if (!WRITE && tid == 0) blocks[blockIdx.x] = kept_so_far;
}

// counts -> exclusive offsets in place, total -> *count.  One workgroup: thread i owns a run of consecutive entries.
__global__ __launch_bounds__(kScanThreads) void keep_scan_kernel(int64_t n_blocks, int64_t *__restrict__ blocks,
                                                                 int64_t *__restrict__ count)
{
    constexpr int WAVES = kScanThreads / kWave;
    __shared__ long long wave_sum[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t per = (n_blocks + kScanThreads - 1) / kScanThreads;
    int64_t b0 = (int64_t)tid * per;
    b0 = b0 < n_blocks ? b0 : n_blocks;
    const int64_t b1 = b0 + per < n_blocks ? b0 + per : n_blocks;
    long long own = 0;
    for (int64_t b = b0; b < b1; ++b) own += blocks[b];
    long long incl = own;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const long long v = __shfl_up(incl, d, kWave);
        incl += lane >= d ? v : 0;
    }
    if (lane == kWave - 1) wave_sum[wave] = incl;
    __syncthreads();
    long long before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const long long v = wave_sum[w];
        before += w < wave ? v : 0;
        total += v;
    }
    long long run = before + incl - own;
    for (int64_t b = b0; b < b1; ++b) {
        const long long v = blocks[b];
        blocks[b] = run;
        run += v;
    }
    if (tid == 0) *count = total;
}

// Cell i = (ix * reso + iy) * reso + iz of the cube [lo, lo + reso * h]^3 (OccGridEstimator.grid_indices' order); centre
// p_a = lo_a + (i_a + 0.5) * h, fp32, multiply then add.
struct CandidateOp {
    int64_t first_cell;
    int reso;
    float lo[3], h;
    const uint8_t *binaries;          // [levels, res, res, res] or null: every cell is a candidate
    const float *aabbs;               // [levels, 6]
    int levels, res;
    int64_t *index;
    float *xyz;

    __device__ __forceinline__ void centre(int64_t i, float (&p)[3]) const
    {
        const int iz = (int)(i % reso), iy = (int)((i / reso) % reso), ix = (int)(i / ((int64_t)reso * reso));
        p[0] = lo[0] + ((float)ix + 0.5f) * h;
        p[1] = lo[1] + ((float)iy + 0.5f) * h;
        p[2] = lo[2] + ((float)iz + 0.5f) * h;
    }

    // The smallest level whose box contains the centre (faces included) decides, with the marcher's point-to-cell
    // expression (march_core.hpp traverse_ray: clamp((int)(((p - min) / extent) * res), 0, res - 1)).
    __device__ __forceinline__ bool keep(int64_t k) const
    {
        if (!binaries) return true;
        float p[3];
        centre(first_cell + k, p);
        const float resf = (float)res;
        for (int lvl = 0; lvl < levels; ++lvl) {
            const float *ab = aabbs + 6 * lvl;
            bool inside = true;
            int cell[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                inside = inside && p[a] >= ab[a] && p[a] <= ab[3 + a];
                const float ext = ab[3 + a] - ab[a];
                cell[a] = clampi((int)(((p[a] - ab[a]) / ext) * resf), 0, res - 1);
            }
            if (inside) return binaries[((int64_t)lvl * res + cell[0]) * res * res + (int64_t)cell[1] * res + cell[2]] != 0;
        }
        return false;
    }

    __device__ __forceinline__ void write(int64_t k, int64_t slot) const
    {
        float p[3];
        centre(first_cell + k, p);
        index[slot] = first_cell + k;
#pragma unroll
        for (int a = 0; a < 3; ++a) xyz[3 * slot + a] = p[a];
    }
};

// rows with sigma >= thresh (false for NaN), copied with what belongs to them
struct SelectOp {
    const int64_t *index_in;
    const float *xyz_in, *sigma_in, *emb_in;
    float thresh;
    int64_t *index;
    float *xyz, *sigma, *emb;

    __device__ __forceinline__ bool keep(int64_t k) const { return sigma_in[k] >= thresh; }

    __device__ __forceinline__ void write(int64_t k, int64_t slot) const
    {
        index[slot] = index_in[k];
#pragma unroll
        for (int a = 0; a < 3; ++a) xyz[3 * slot + a] = xyz_in[3 * k + a];
        sigma[slot] = sigma_in[k];
#pragma unroll
        for (int f = 0; f < 15; ++f) emb[15 * slot + f] = emb_in[15 * k + f];
    }
};

static int64_t keep_blocks(int64_t n) { return (n + kKeepItems - 1) / kKeepItems; }

template <class Op>
static int run_keep(const Op &op, int64_t n, int64_t capacity, int64_t *count, void *workspace, const char *who, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        if (hipMemsetAsync(count, 0, sizeof(int64_t), s) != hipSuccess) return check_launch(who);
        return CED_OK;
    }
    const int64_t nb = keep_blocks(n);
    int64_t *blocks = reinterpret_cast<int64_t *>(workspace);
    hipLaunchKernelGGL((keep_kernel<Op, false>), dim3((unsigned)nb), dim3(kKeepThreads), 0, s, op, n, blocks, (int64_t)0);
    hipLaunchKernelGGL(keep_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, nb, blocks, count);
    if (capacity > 0)
        hipLaunchKernelGGL((keep_kernel<Op, true>), dim3((unsigned)nb), dim3(kKeepThreads), 0, s, op, n, blocks, capacity);
    return check_launch(who);
}

constexpr int kBakeMaxReso = 2048;                                 // reso^3 = 2^33 cells; (i + 0.5f) exact far beyond

}  // namespace ced

extern "C" int64_t ced_bake_workspace_bytes(int64_t n)
{
    if (n < 0) return -1;
    const int64_t nb = ced::keep_blocks(n);
    return (nb > 0 ? nb : 1) * (int64_t)sizeof(int64_t);
}

extern "C" int ced_bake_candidates(int32_t reso, const float *center_host, float radius, int64_t first_cell, int64_t n_cells,
                                   const uint8_t *binaries, const float *aabbs, int32_t levels, int32_t grid_res,
                                   int64_t capacity, int64_t *index, float *xyz, int64_t *count, void *workspace,
                                   int64_t workspace_bytes, void *stream)
{
    using namespace ced;
    CED_REQUIRE(reso >= 1 && reso <= kBakeMaxReso, "bake_candidates: reso=%d (1 .. %d)", reso, kBakeMaxReso);
    CED_REQUIRE(center_host != nullptr, "bake_candidates: null center");
    CED_REQUIRE(radius > 0.0f && radius < __builtin_inff(), "bake_candidates: radius=%g", (double)radius);
    const int64_t total = (int64_t)reso * reso * reso;
    CED_REQUIRE(first_cell >= 0 && n_cells >= 0 && first_cell <= total && n_cells <= total - first_cell,
                "bake_candidates: cells [%lld, +%lld) of %lld", (long long)first_cell, (long long)n_cells, (long long)total);
    CED_REQUIRE(capacity >= 0 && count != nullptr, "bake_candidates: capacity < 0 or null count");
    CED_REQUIRE(capacity == 0 || (index && xyz), "bake_candidates: null output");
    CED_REQUIRE(workspace && workspace_bytes >= ced_bake_workspace_bytes(n_cells), "bake_candidates: workspace too small");
    if (binaries)
        CED_REQUIRE(aabbs && levels >= 1 && grid_res >= 1 && grid_res <= 1024, "bake_candidates: grid levels=%d res=%d",
                    levels, grid_res);
    CandidateOp op{};
    op.first_cell = first_cell;
    op.reso = reso;
    for (int a = 0; a < 3; ++a) op.lo[a] = center_host[a] - radius;
    op.h = (2.0f * radius) / (float)reso;
    op.binaries = binaries; op.aabbs = aabbs; op.levels = levels; op.res = grid_res;
    op.index = index; op.xyz = xyz;
    return run_keep(op, n_cells, capacity, count, workspace, "bake_candidates", stream);
}

extern "C" int ced_bake_select(int64_t n, const int64_t *index_in, const float *xyz_in, const float *sigma_in,
                               const float *embedding_in, float sigma_thresh, int64_t capacity, int64_t *index, float *xyz,
                               float *sigma, float *embedding, int64_t *count, void *workspace, int64_t workspace_bytes,
                               void *stream)
{
    using namespace ced;
    CED_REQUIRE(n >= 0, "bake_select: n < 0");
    CED_REQUIRE(capacity >= 0 && count != nullptr, "bake_select: capacity < 0 or null count");
    CED_REQUIRE(n == 0 || sigma_in, "bake_select: null sigma");
    CED_REQUIRE(capacity == 0 || n == 0 || (index_in && xyz_in && embedding_in && index && xyz && sigma && embedding),
                "bake_select: null pointer");
    CED_REQUIRE(workspace && workspace_bytes >= ced_bake_workspace_bytes(n), "bake_select: workspace too small");
    SelectOp op{};
    op.index_in = index_in; op.xyz_in = xyz_in; op.sigma_in = sigma_in; op.emb_in = embedding_in;
    op.thresh = sigma_thresh;
    op.index = index; op.xyz = xyz; op.sigma = sigma; op.emb = embedding;
    return run_keep(op, n, capacity, count, workspace, "bake_select", stream);
}
