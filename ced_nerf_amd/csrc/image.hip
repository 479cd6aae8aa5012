#include "ced_common.hpp"
#include "composite_core.hpp"
#include "field_args.hpp"
#include "frame_loop.hpp"

namespace ced {

// render_image in eval mode (cednerf/utils.py:46-150): `sampling` (march every ray to the far plane, evaluate the
// density of EVERY sample, keep those whose transmittance so far is >= early_stop_eps) followed by `rendering` (evaluate
// the field again on the survivors, weights, per-ray sums).  The kept samples of a ray are a prefix of its march (the
// transmittance only falls), so the same result comes from walking each ray's samples front to back in chunks, the field
// evaluated ONCE per sample (colour and density together), and stopping a ray at the first sample that fails the test:
// identical floats in the identical order => bit-identical outputs, with 3.9 M instead of 15 M + 3.9 M field
// evaluations on the 800x800 frame.  The chunk sizes follow the N_samples rule of the test loop (any would do).
// Per sample the call keeps (persistent arrays in the workspace, iteration after iteration, entry = sample_base + i):
// t0, t1, ray, sigma, rgb, weight, transmittance, alpha, and the sample's rank among the ray's kept ones (-1: dropped);
// ced_render_image_gather moves the kept ones into the reference's ray-major order.
struct ImageState {
    int32_t *cursor;     // samples of the ray consumed so far
    float *acc_all;      // sum of sigma * dt over ALL consumed samples      (visibility: render_visibility_from_density)
    float *acc_kept;     // sum of sigma * dt over the KEPT samples           (weights:    render_weight_from_density)
    int32_t *kept;       // kept samples of the ray so far
};

__global__ __launch_bounds__(256) void image_prep_kernel(int64_t n_rays, ImageState st, const float *__restrict__ rays_d,
                                                         float *__restrict__ sh_ray, float *__restrict__ rgb,
                                                         float *__restrict__ opacity, float *__restrict__ depth)
{
    int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rays) return;
    st.cursor[r] = 0; st.acc_all[r] = 0.0f; st.acc_kept[r] = 0.0f; st.kept[r] = 0;
    if (rgb) reset_ray(rays_d, r, sh_ray, rgb, opacity, depth);
}

// The iteration's samples: the next `limit` samples of every alive ray, copied from the one-shot march into the
// iteration's window of the persistent arrays (ray-packed, one range reservation per workgroup as in march_frame_kernel).
// samples of ray r in the one-shot march; a range that passes the end of the arrays (a one-pass march that overflowed
// its capacity: the caller redoes the frame) counts as empty, so that nothing out of bounds is ever read
__device__ __forceinline__ int64_t ray_count(const int64_t *__restrict__ packed_all, int64_t r, int64_t n_all)
{
    const int64_t start = packed_all[2 * r], cnt = packed_all[2 * r + 1];
    return (start < 0 || cnt < 0 || start + cnt > n_all) ? 0 : cnt;
}

__global__ __launch_bounds__(kMarchThreads) void image_chunk_kernel(
    IterPlan *__restrict__ plan, int64_t n_all, const int32_t *__restrict__ alive, const int64_t *__restrict__ packed_all,
    const float *__restrict__ t0_all, const float *__restrict__ t1_all, const int32_t *__restrict__ cursor,
    float *__restrict__ t0s, float *__restrict__ t1s, int32_t *__restrict__ ridx, int32_t *__restrict__ packed)
{
    const IterPlan &P = *plan;
    const int64_t total = P.count[0];
    const int limit = P.limit[0];
    const int64_t base = P.sample_base;
    for (int64_t s0 = (int64_t)blockIdx.x * kMarchThreads; s0 < total; s0 += (int64_t)gridDim.x * kMarchThreads) {
        const int64_t idx = s0 + threadIdx.x;
        const bool active = idx < total;
        const int64_t r = active ? (alive ? (int64_t)alive[idx] : idx) : 0;
        int n = 0;
        int64_t src = 0;
        if (active) {
            const int cur = cursor[r];
            const int64_t left = ray_count(packed_all, r, n_all) - cur;
            n = (int)(left < limit ? left : limit);
            src = packed_all[2 * r] + cur;
        }
        const int64_t slot = workgroup_reserve<kMarchThreads / 64>(n, [&](int run) {
            return (long long)atomicAdd(reinterpret_cast<unsigned long long *>(&plan->total_samples), (unsigned long long)run);
        });
        if (active) {
            const int64_t start = base + slot;
            packed[2 * r] = (int32_t)start;
            packed[2 * r + 1] = n;
            for (int i = 0; i < n; ++i) {
                t0s[start + i] = t0_all[src + i];
                t1s[start + i] = t1_all[src + i];
                ridx[start + i] = (int32_t)r;
            }
        }
        __syncthreads();
    }
}

// Visibility (nerfacc render_visibility_from_density: exp(-sum so far) >= early_stop_eps, alpha >= alpha_thre), weights
// of the kept samples (render_weight_from_density over the kept ones only) and the three per-ray sums of
// cednerf/render.py:158-169 -- every sum sequential in sample order, carried across iterations in the ray's state.
template <bool FULL>
__global__ __launch_bounds__(kCompositeThreads) void image_composite_kernel(
    IterPlan *plan, const int32_t *__restrict__ alive_list, int32_t *__restrict__ next_list,
    const int32_t *__restrict__ packed, const int64_t *__restrict__ packed_all, const float *__restrict__ t0,
    const float *__restrict__ t1, const float *__restrict__ sig, const float *__restrict__ rgbs, ImageState st,
    float *__restrict__ w_out, float *__restrict__ tr_out, float *__restrict__ al_out, int32_t *__restrict__ rank_out,
    float *__restrict__ rgb, float *__restrict__ opacity, float *__restrict__ depth, float eps, float alpha_thre,
    int64_t n_all)
{
    const IterPlan &P = *plan;
    const int64_t total = P.count[0];
    for (int64_t s0 = (int64_t)blockIdx.x * kCompositeThreads; s0 < total; s0 += (int64_t)gridDim.x * kCompositeThreads) {
        const int64_t idx = s0 + threadIdx.x;
        const bool active = idx < total;
        const int64_t r = active ? (alive_list ? (int64_t)alive_list[idx] : idx) : 0;
        int cnt = 0, kept_new = 0;
        bool alive = false;
        if (active) {
            const int64_t sb = packed[2 * r];
            cnt = packed[2 * r + 1];
            if (cnt > 0) {
                RaySums sums;
                if constexpr (FULL) sums.load(rgb, opacity, depth, r);
                float acc = st.acc_all[r], acck = st.acc_kept[r];
                int kept = st.kept[r];
                const int kept_before = kept;
                bool open = true;                   // false once a sample failed the transmittance test: the rest fail too
                walk_samples<4, FULL>(sb, sb + cnt, t0, t1, sig, rgbs,
                                      [&](float ts, float te, float sg, float cr, float cg, float cb, int64_t i) __attribute__((always_inline)) {
                    const Sample all = sample_step(sg, ts, te, trans_of(acc));
                    open = open && (all.T >= eps);          // visible()'s transmittance half, kept for the rest of the ray
                    const bool vis = open && visible(all.T, all.a, eps, alpha_thre);
                    acc = acc + all.sd;
                    int rank = -1;
                    if (vis) {
                        if constexpr (FULL) {
                            // the weight's transmittance is over the KEPT samples; no alpha test: the two sums coincide
                            const Sample k = alpha_thre > 0.0f ? sample_step(sg, ts, te, trans_of(acck)) : all;
                            sums.add(k.w, cr, cg, cb, ts, te);
                            acck = acck + k.sd;
                            w_out[i] = k.w; tr_out[i] = k.T; al_out[i] = k.a;
                        }
                        rank = kept++;
                    }
                    rank_out[i] = rank;
                });
                if constexpr (FULL) sums.store(rgb, opacity, depth, r);
                const int cur = st.cursor[r] + cnt;
                st.cursor[r] = cur;
                st.acc_all[r] = acc; st.acc_kept[r] = acck; st.kept[r] = kept;
                kept_new = kept - kept_before;
                // alive: samples left, and the next one would pass the transmittance test
                alive = open && (int64_t)cur < ray_count(packed_all, r, n_all) && (trans_of(acc) >= eps);
            }
        }
        const int sums[2] = { cnt, kept_new };
        const int slot = workgroup_append<kCompositeThreads / 64, 2>(alive, sums, [&](int run, const int *tot) {
            const unsigned long long add = (unsigned long long)run + ((unsigned long long)tot[0] << 32);
            const int base = add != 0 ? (int)(atomicAdd(&plan->next[0], add) & 0xffffffffull) : 0;
            if (tot[1]) atomicAdd(&plan->next[1], (unsigned long long)tot[1]);        // kept samples of the iteration
            return base;
        });
        if (alive) next_list[slot] = (int32_t)r;
        __syncthreads();
    }
}

// Kept samples -> the reference's order (by ray, then along the ray): entry i of the persistent arrays goes to
// ray_offset[ray] + rank.  chunk_rays > 0: ray indices relative to the ray's chunk of that many rays (the `extras` of
// the reference's chunked eval loop, cednerf/utils.py:108-133).
struct ImageOut {
    int64_t *ray_indices;
    float *t_starts, *t_ends, *sigmas, *rgbs, *weights, *trans, *alphas;
};

__global__ __launch_bounds__(256) void image_gather_kernel(int64_t n, const int32_t *__restrict__ rank,
                                                           const int32_t *__restrict__ ridx, const float *__restrict__ t0,
                                                           const float *__restrict__ t1, const float *__restrict__ sig,
                                                           const float *__restrict__ rgbs, const float *__restrict__ w,
                                                           const float *__restrict__ tr, const float *__restrict__ al,
                                                           const int64_t *__restrict__ ray_offset, int64_t chunk_rays,
                                                           ImageOut out)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int k = rank[i];
        if (k < 0) continue;
        const int64_t r = ridx[i];
        const int64_t d = ray_offset[r] + k;
        out.ray_indices[d] = chunk_rays > 0 ? r % chunk_rays : r;
        out.t_starts[d] = t0[i]; out.t_ends[d] = t1[i];
        if (out.sigmas) out.sigmas[d] = sig[i];
        if (out.rgbs) {                       // (NULL after a sampling-only call: those arrays were never written)
            out.rgbs[3 * d] = rgbs[3 * i]; out.rgbs[3 * d + 1] = rgbs[3 * i + 1]; out.rgbs[3 * d + 2] = rgbs[3 * i + 2];
            out.weights[d] = w[i]; out.trans[d] = tr[i]; out.alphas[d] = al[i];
        }
    }
}

struct ImageWorkspace {
    ImageState st;
    int32_t *packed, *alive_a, *alive_b;
    IterPlan *plans;
    float *t0, *t1; int32_t *ridx; float *sigma, *rgbs, *w, *tr, *al; int32_t *rank;
    float *sh_ray;                  // [n, 3] colour-head SH inputs per ray (FieldArgs::sh_ray)
    size_t bytes;
};

constexpr int kImageMaxIters = 1024;

static ImageWorkspace carve_image(void *base, int64_t n, int64_t cap)
{
    ImageWorkspace w{};
    Carver c{ (char *)base };
    w.st.cursor = c.take<int32_t>((size_t)n);
    w.st.acc_all = c.take<float>((size_t)n);
    w.st.acc_kept = c.take<float>((size_t)n);
    w.packed = c.take<int32_t>((size_t)n * 2);
    w.alive_a = c.take<int32_t>((size_t)n);
    w.alive_b = c.take<int32_t>((size_t)n);
    w.plans = c.take<IterPlan>((size_t)kImageMaxIters + 2);
    w.t0 = c.take<float>((size_t)cap);
    w.t1 = c.take<float>((size_t)cap);
    w.ridx = c.take<int32_t>((size_t)cap);
    w.sigma = c.take<float>((size_t)cap);
    w.rgbs = c.take<float>((size_t)cap * 3);
    w.w = c.take<float>((size_t)cap);
    w.tr = c.take<float>((size_t)cap);
    w.al = c.take<float>((size_t)cap);
    w.rank = c.take<int32_t>((size_t)cap);
    w.sh_ray = c.take<float>((size_t)n * 3);
    w.bytes = c.off;
    return w;
}

// a ray consumes at most its whole march; an iteration at most n_rays samples (N_samples <= n_rays // alive) plus the
// field kernel's tile padding
static inline int64_t image_capacity(int64_t n_rays, int64_t n_all) { return n_all + 64; }

}  // namespace ced

extern "C" int64_t ced_render_image_workspace_bytes(int64_t n_rays, int64_t n_all)
{
    if (n_rays < 0 || n_all < 0) return -1;
    return (int64_t)ced::carve_image(nullptr, n_rays, ced::image_capacity(n_rays, n_all)).bytes;
}

extern "C" int ced_render_image(const ced_field_desc *field, int64_t n_rays, const float *rays_o, const float *rays_d,
                                int64_t n_all, const int64_t *packed_all, const float *t0_all, const float *t1_all,
                                float early_stop_eps, float alpha_thre, const float *timestamps, int32_t t_per_ray,
                                const float *bkgd, float *rgb, float *opacity, float *depth, int32_t *kept,
                                void *workspace, int64_t workspace_bytes, int64_t *host_stats, int64_t *stats_out,
                                void *field_stream_, void *stream_)
{
    using namespace ced;
    const char *who = "render_image";
    hipStream_t stream = (hipStream_t)stream_;
    hipStream_t fstream = field_stream_ ? (hipStream_t)field_stream_ : stream;
    CED_REQUIRE(fstream == stream, "%s: a separate field stream is not supported", who);
    CED_REQUIRE(field != nullptr, "%s: null field descriptor", who);
    CED_REQUIRE(n_rays >= 0 && n_all >= 0, "%s: bad sizes", who);
    CED_REQUIRE(n_rays < (1ll << 31) / 4 && n_all < (1ll << 31) - 128, "%s: too many rays / samples for 32-bit indices", who);
    if (stats_out) { stats_out[0] = 0; stats_out[1] = 0; stats_out[2] = 0; }
    if (n_rays == 0) return CED_OK;
    const bool full = rgb != nullptr;               // rgb == NULL: sampling only (density-only field, no pixel sums)
    CED_REQUIRE(rays_o && rays_d && packed_all && (n_all == 0 || (t0_all && t1_all)) && timestamps && kept && workspace &&
                    host_stats && (!full || (opacity && depth)),
                "%s: null pointer", who);
    const int64_t cap = image_capacity(n_rays, n_all);
    ImageWorkspace W = carve_image(workspace, n_rays, cap);
    W.st.kept = kept;
    CED_REQUIRE((int64_t)W.bytes <= workspace_bytes, "%s: workspace too small (%lld < %lld bytes)", who,
                (long long)workspace_bytes, (long long)W.bytes);
    const dim3 blk(256), grd((unsigned)((n_rays + 255) / 256));
    hipLaunchKernelGGL(image_prep_kernel, grd, blk, 0, stream, n_rays, W.st, rays_d, W.sh_ray, rgb, opacity, depth);
    const int big = 1 << 30;                               // no sample budget: the loop ends when no ray is alive
    // smallest chunk of an iteration (any chunking gives the same result; fewer, larger iterations against samples
    // evaluated behind a ray's end): measured on the 800x800 frame / the 262 k-ray batch, 4 for the full pass (4.26 ->
    // 4.03 ms against chunks from 1) and 8 for the density-only sampling pass
    const int min_chunk = full ? 4 : 8;
    FrameLoop L{ ScheduleArgs{ W.plans, -1, 1, (int)n_rays, min_chunk, big, (long long *)host_stats, 0 }, W.alive_a, W.alive_b,
                 kImageMaxIters, who };
    L.begin(stream, nullptr, nullptr, 0);
    int rc = check_launch("render_image (prep)");
    if (rc) return rc;
    for (; L.it < L.max_iters; ++L.it) {
        bool stop = false;
        rc = L.next(stop);
        if (rc) return rc;
        if (stop) break;
        IterPlan *plan = L.plan();
        const int32_t *cur_list = L.cur_list();
        int32_t *next_list = L.next_list();
        int64_t mgrid = (L.alive_bound + kMarchThreads - 1) / kMarchThreads;
        if (mgrid > 8192) mgrid = 8192;
        if (mgrid < 1) mgrid = 1;
        hipLaunchKernelGGL(image_chunk_kernel, dim3((unsigned)mgrid), dim3(kMarchThreads), 0, stream, plan, n_all, cur_list,
                           packed_all, t0_all, t1_all, W.st.cursor, W.t0, W.t1, W.ridx, W.packed);
        FieldArgs F{};
        F.n = n_rays * (int64_t)min_chunk;  // an iteration's samples: alive * N_samples <= n_rays * min_chunk; exact count from the plan
        F.n_dev = &plan->total_samples;
        F.base_dev = &plan->sample_base;
        F.rays_o = rays_o; F.rays_d = rays_d; F.ray_idx32 = W.ridx;
        F.sh_ray = (full && g_frame_sh_per_ray) ? W.sh_ray : nullptr;
        F.t0 = W.t0; F.t1 = W.t1;
        F.timestamps = timestamps;
        F.rays_mode = 1; F.t_per_ray = t_per_ray ? 1 : 0; F.want_rgb = full ? 1 : 0;
        F.rgb = full ? W.rgbs : nullptr; F.sigma = W.sigma; F.geo = nullptr;
        rc = launch_field(field, F, (void *)stream);
        if (rc) return rc;
        int64_t cgrid = (L.alive_bound + kCompositeThreads - 1) / kCompositeThreads;
        if (cgrid > 4096) cgrid = 4096;
        if (cgrid < 1) cgrid = 1;
        if (full)
            hipLaunchKernelGGL(image_composite_kernel<true>, dim3((unsigned)cgrid), dim3(kCompositeThreads), 0, stream, plan,
                               cur_list, next_list, W.packed, packed_all, W.t0, W.t1, W.sigma, W.rgbs, W.st, W.w, W.tr, W.al,
                               W.rank, rgb, opacity, depth, early_stop_eps, alpha_thre, n_all);
        else
            hipLaunchKernelGGL(image_composite_kernel<false>, dim3((unsigned)cgrid), dim3(kCompositeThreads), 0, stream, plan,
                               cur_list, next_list, W.packed, packed_all, W.t0, W.t1, W.sigma, (const float *)nullptr, W.st,
                               (float *)nullptr, (float *)nullptr, (float *)nullptr, W.rank, (float *)nullptr,
                               (float *)nullptr, (float *)nullptr, early_stop_eps, alpha_thre, n_all);
        L.schedule(stream);
        rc = check_launch("render_image (iteration)");
        if (rc) return rc;
    }
    if (full) {
        rc = ced_finalize_pixels(n_rays, bkgd, rgb, opacity, depth, stream);
        if (rc) return rc;
    }
    std::vector<IterPlan> plans;
    int n_iters = 0;
    rc = L.finish(stream, "render_image (read-back)", plans, n_iters);
    if (rc) return rc;
    int64_t processed = 0, kept_total = 0;
    for (int k = 0; k < n_iters; ++k) {
        processed = plans[k].sample_base + plans[k].total_samples;
        kept_total += (int64_t)plans[k].next[1];
    }
    CED_REQUIRE(processed <= cap, "%s: internal: %lld samples processed, capacity %lld", who, (long long)processed, (long long)cap);
    if (stats_out) { stats_out[0] = processed; stats_out[1] = n_iters; stats_out[2] = kept_total; }
    return CED_OK;
}

extern "C" int ced_render_image_gather(int64_t n_rays, int64_t n_all, int64_t processed, const void *workspace,
                                       int64_t workspace_bytes, const int64_t *ray_offsets, int64_t chunk_rays,
                                       int64_t *ray_indices, float *t_starts, float *t_ends, float *sigmas, float *rgbs,
                                       float *weights, float *trans, float *alphas, void *stream)
{
    CED_REQUIRE(n_rays >= 0 && n_all >= 0 && processed >= 0, "render_image_gather: bad sizes");
    if (processed == 0) return CED_OK;
    CED_REQUIRE(workspace && ray_offsets && ray_indices && t_starts && t_ends, "render_image_gather: null pointer");
    CED_REQUIRE((rgbs && weights && trans && alphas) || (!rgbs && !weights && !trans && !alphas),
                "render_image_gather: rgbs / weights / trans / alphas go together");
    const ced::ImageWorkspace W = ced::carve_image(const_cast<void *>(workspace), n_rays, ced::image_capacity(n_rays, n_all));
    CED_REQUIRE((int64_t)W.bytes <= workspace_bytes && processed <= ced::image_capacity(n_rays, n_all),
                "render_image_gather: workspace does not match");
    int64_t grid = (processed + 255) / 256;
    if (grid > 16384) grid = 16384;
    hipLaunchKernelGGL(ced::image_gather_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, processed, W.rank,
                       W.ridx, W.t0, W.t1, W.sigma, W.rgbs, W.w, W.tr, W.al, ray_offsets, chunk_rays,
                       ced::ImageOut{ ray_indices, t_starts, t_ends, sigmas, rgbs, weights, trans, alphas });
    return ced::check_launch("render_image_gather");
}

