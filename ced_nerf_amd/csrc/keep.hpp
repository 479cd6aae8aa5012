// Order-preserving stream compaction shared by bake.hip and mesh.hip: the kept items of 0 .. n-1 land in ascending item
// order, so no output slot is claimed atomically and the output is the same on every run.  Three launches: every workgroup
// counts its kKeepItems items; one workgroup turns the counts into exclusive offsets and the total; every workgroup
// evaluates its items again and writes each kept one at offset + rank, the rank from a wavefront ballot (lanes below) plus
// the workgroup's earlier waves and rounds.  The predicates are a few bytes or floats per item: evaluating one twice costs
// less than keeping it.
#pragma once
#include "ced_common.hpp"

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
// static: every source that includes this header carries its own copy.
static __global__ __launch_bounds__(kScanThreads) void keep_scan_kernel(int64_t n_blocks, int64_t *__restrict__ blocks,
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

static inline int64_t keep_blocks(int64_t n) { return (n + kKeepItems - 1) / kKeepItems; }

// workspace: keep_blocks(n) int64 (at least one).  capacity = 0 only counts.
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

}  // namespace ced
