// The loop driver of frame_loop.hpp: the two scheduling kernels (defined here and nowhere else; the renderers reach them
// through FrameLoop) and the host's publish / run-ahead / read-back code.
#include <atomic>
#include <chrono>

#include "frame_loop.hpp"

namespace ced {

// Every frame advances its own reference loop (cednerf/utils.py:227-238): while iter_samples < max_samples and rays
// are alive, N_samples = clamp(N_rays // N_alive, min, 64), iter_samples += N_samples.  it = -1 writes the plan of
// iteration 0 (all rays alive); otherwise the plan of iteration it + 1 from the survivor counts of iteration it.
// Then (alive rays, done) of the new plan go to pinned host memory behind a sequence number.
// ONE WAVE: lane f works out frame f, the frames' slot ranges are an exclusive prefix sum across the lanes.
//
// Sharded frames (ced_shard_exchange): the rays of frame f are dealt over several processes and the reference's loop is
// ONE loop per image -- N_rays and N_alive in utils.py:235 are the whole image's.  `xcounts` then holds, for every
// iteration and frame, the survivors summed over the processes (the exchange step between the compositing and this
// launch), `global_rays` the image's ray count: every process computes the same N_samples, the same last-iteration flag
// and the same end of the loop, so each ray gets exactly the samples it gets when one process renders the image.
__device__ __forceinline__ void make_next_plan(const ScheduleArgs &S)
{
    const int f = threadIdx.x & 63;
    IterPlan &N = S.plans[S.it + 1];
    int local = 0, used = 0;
    long long global = 0;
    if (f < S.n_frames) {
        if (S.it < 0) {
            local = S.local_rays ? S.local_rays[f] : S.rays_per_frame;
            global = S.global_rays > 0 ? S.global_rays : local;
        } else {
            const IterPlan &P = S.plans[S.it];
            // the survivor counts were accumulated by device-scope atomics of other workgroups
            const unsigned long long nx = __hip_atomic_load(&P.next[f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const bool finished = P.last[f] || P.gcount[f] == 0;
            local = (finished || P.count[f] == 0) ? 0 : (int)(nx & 0xffffffffull);
            global = finished ? 0 : (S.xcounts ? S.xcounts[(int64_t)S.it * S.n_frames + f] : local);
            used = P.used[f];
        }
    }
    int count = 0, gcount = 0, limit = 0, last = 0;
    if (global > 0 && used < S.max_samples) {
        const long long n_total = S.global_rays > 0 ? S.global_rays : S.rays_per_frame;
        const long long q = n_total / global;
        limit = q < 64 ? (int)q : 64;
        if (limit < S.min_samples) limit = S.min_samples;
        used += limit;
        last = used >= S.max_samples ? 1 : 0;
        count = local;
        gcount = (int)(global < 0x7fffffffll ? global : 0x7fffffffll);
    }
    // slot ranges: exclusive prefix sum of the counts rounded up to kSlotAlign
    const int padded = (count + kSlotAlign - 1) & ~(kSlotAlign - 1);
    int incl = padded;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off, 64);
        if (f >= off) incl += v;
    }
    long long alive_here = count, alive_all = gcount;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        alive_here += __shfl_xor(alive_here, off, 64);
        alive_all += __shfl_xor(alive_all, off, 64);
    }
    const int total_slots = __shfl(incl, 63, 64);
    N.count[f] = count; N.gcount[f] = gcount; N.limit[f] = limit; N.last[f] = last; N.used[f] = used;
    N.slot_base[f] = incl - padded; N.samp_bound[f] = count * limit;
    N.next[f] = 0;
    if (f == 0) {
        N.total_slots = total_slots;
        N.sample_base = S.it < 0 ? 0 : S.plans[S.it].sample_base + S.plans[S.it].total_samples;
        N.total_samples = 0;
        N.n_cand = 0;
        N.cursor = 0;
        N.done = alive_all == 0 ? 1 : 0;
        S.host[0] = alive_here;                 // rays alive entering iteration it + 1: an upper bound for every later one
        S.host[1] = N.done;
        if (S.host_iter) {
            S.host_iter[3 * (S.it + 1)] = alive_here;
            S.host_iter[3 * (S.it + 1) + 1] = N.done;
        }
        __threadfence_system();
        __hip_atomic_store(&S.host[2], S.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        if (S.host_iter) __hip_atomic_store(&S.host_iter[3 * (S.it + 1) + 2], S.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The plan of iteration 0.  The launch also brings the call's lattice table (256 floats the host wrote behind the
// publish words of the pinned buffer, march_accel.hpp: build_lattice) into device memory.
__global__ void frame_init_kernel(ScheduleArgs S, float *__restrict__ lattice_dev, unsigned long long *stamps = nullptr,
                                  int n_stamps = 0)
{
    for (int i = threadIdx.x; i < n_stamps; i += blockDim.x) {      // {min start, max end} per iteration
        stamps[2 * i] = ~0ull;
        stamps[2 * i + 1] = 0ull;
    }
    if (lattice_dev) {
        const float *src = reinterpret_cast<const float *>(S.host + kHostLatticeWord);
        for (int i = threadIdx.x; i < 256; i += blockDim.x) lattice_dev[i] = src[i];
    }
    if (threadIdx.x < 64) make_next_plan(S);        // the first wave (launched with exactly one)
}

// One wave turns the survivor counts of iteration `it` into the plan of iteration it + 1.  (Folding this into the
// compositing kernel's last workgroup was tried: the system-scope publish inside that kernel cost more than this
// launch -- 24 us instead of 14 + 5 per iteration.)
__global__ __launch_bounds__(64) void frame_schedule_kernel(ScheduleArgs S)
{
    make_next_plan(S);
}

static std::atomic<long long> g_publish_seq{ 0 };

#if defined(__HIP_DEVICE_COMPILE__)
#define CED_CPU_PAUSE()
#else
#define CED_CPU_PAUSE() __builtin_ia32_pause()
#endif

// Waits until the sequence number in pinned host memory has reached `seq` (spin; after 200 ms a stream synchronise,
// after which the number must be there -- otherwise a launch of the chain has failed).
static int wait_published(volatile long long *flag, long long seq, hipStream_t stream, const char *who)
{
    const auto t_start = std::chrono::steady_clock::now();
    long spins = 0;
    while (__atomic_load_n(flag, __ATOMIC_ACQUIRE) < seq) {
        if ((++spins & 0x3ff) == 0) {
            if (std::chrono::steady_clock::now() - t_start > std::chrono::milliseconds(200)) {
                if (hipStreamSynchronize(stream) != hipSuccess) return check_launch("render_image_test (sync)");
                if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) < seq) {
                    set_error("%s: iteration %lld was not published although the stream has drained", who, seq);
                    return CED_E_LAUNCH;
                }
                break;
            }
        } else {
            CED_CPU_PAUSE();
        }
    }
    return CED_OK;
}

void FrameLoop::begin(hipStream_t stream_, float *lattice, unsigned long long *stamps, int n_stamps)
{
    stream = stream_;
    alive_bound = (long long)sched.n_frames * sched.rays_per_frame;
    it = 0;
    plan_seq.assign((size_t)max_iters + 1, 0);
    plan_seq[0] = ++g_publish_seq;
    ScheduleArgs S = sched;
    S.it = -1;
    S.seq = plan_seq[0];
    hipLaunchKernelGGL(frame_init_kernel, dim3(1), dim3(64), 0, stream, S, lattice, stamps, n_stamps);
}

// Run-ahead control, before iteration `it` is enqueued: the plan of iteration it - kRunAhead must have been published
// (by the schedule launch of the iteration before it, or by the initial one; plan_seq[k]: the publication of plan k).
// Then `stop` when the loop is over, else alive_bound tightened to the published alive count.  pub: the words
// {alive, done, seq} the latest plan is published to.  host_iter (sharded frames, else NULL): those of every plan --
// every process must enqueue the same number of iterations (each holds a collective), so the loop ends on the plan of
// iteration it - kRunAhead, identical on all processes, and on nothing later that happens to have been published already.
int FrameLoop::next(bool &stop)
{
    volatile long long *const pub = sched.host, *const host_iter = sched.host_iter;
    stop = false;
    const int need = it - kRunAhead;
    if (need < 0 && host_iter) return CED_OK;
    volatile long long *const rec = host_iter ? host_iter + 3 * need : pub;
    if (need >= 0) {
        const int rc = wait_published(rec + 2, plan_seq[need], stream, who);
        if (rc) return rc;
    }
    if (host_iter || __atomic_load_n(pub + 2, __ATOMIC_ACQUIRE) >= plan_seq[0]) {   // something of THIS call is published
        if (rec[1]) {                                                               // nothing left: stop enqueueing
            stop = true;
            return CED_OK;
        }
        const long long a = rec[0];
        if (a >= 0 && a < alive_bound) alive_bound = a;
    }
    return CED_OK;
}

void FrameLoop::schedule(hipStream_t stream_)
{
    plan_seq[it + 1] = ++g_publish_seq;
    ScheduleArgs S = sched;
    S.it = it;
    S.seq = plan_seq[it + 1];
    hipLaunchKernelGGL(frame_schedule_kernel, dim3(1), dim3(64), 0, stream_, S);
}

// The per-iteration record of a call: the plans of its enqueued iterations and the one after come back in one copy
// (the call blocks here, once).  n_iters: the iterations that ran, up to the first plan with nothing left; a loop that
// was not stopped by such a plan left rays alive.
int FrameLoop::finish(hipStream_t stream_, const char *what, std::vector<IterPlan> &plans, int &n_iters)
{
    const int enqueued = it;
    plans.resize((size_t)enqueued + 1);
    if (hipMemcpyAsync(plans.data(), sched.plans, plans.size() * sizeof(IterPlan), hipMemcpyDeviceToHost, stream_) != hipSuccess ||
        hipStreamSynchronize(stream_) != hipSuccess)
        return check_launch(what);
    n_iters = 0;
    while (n_iters < enqueued && !plans[n_iters].done && plans[n_iters].total_slots != 0) ++n_iters;
    if (n_iters == enqueued && !plans[enqueued].done) {
        set_error("%s: the loop stopped after %d iterations with rays still alive", who, enqueued);
        return CED_E_LAUNCH;
    }
    return CED_OK;
}

}  // namespace ced
