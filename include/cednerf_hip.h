/*
 * cednerf_hip.h -- C ABI of libcednerf_hip.so, the MI355X (gfx950) rendering hot path behind
 * Ced-NeRF's Python API.
 *
 * The reference has no FFI of its own for this path: its native entry points are the Python
 * bindings of two un-vendored CUDA packages (nerfacc's `nerfacc.cuda._C` ops and tiny-cuda-nn's
 * torch modules) plus Taichi kernels called with torch tensors.  Each function below names the
 * reference interface it replaces (file:line relative to /root/reference).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter is documented "host";
 *   - tensors are dense, row-major, float32 unless stated; index tensors are int64 as in nerfacc;
 *     boolean tensors are one byte per element (torch.bool storage);
 *   - the library never allocates or frees user-visible memory and never synchronises the device:
 *     outputs and scratch are caller-allocated, work is enqueued on `stream` (a hipStream_t passed
 *     as void*, NULL = default stream);
 *   - return value 0 = success, negative = error (CED_E_*); ced_last_error_string() describes the
 *     last failure of the calling thread.  Nothing throws or aborts.
 *   - arithmetic contract: IEEE binary32, no FMA contraction except where the algorithm states
 *     one; dot products are ascending-k fused-multiply-add chains (the fp32 MFMA's native
 *     behaviour); per-ray sums run in sample order.  See DESIGN.md, "Arithmetic contract".
 */
#ifndef CEDNERF_HIP_H
#define CEDNERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CED_MAX_LEVELS 16

#define CED_OK 0
#define CED_E_INVALID (-1)      /* bad argument (null pointer, negative size, unsupported option) */
#define CED_E_LAUNCH (-2)       /* HIP launch / runtime error */
#define CED_E_UNSUPPORTED (-3)  /* configuration outside what the kernels implement */

/* Multi-resolution hash grid description (host struct, copied at launch).
 * Replaces the tcnn `HashGrid` encoding built at cednerf/model.py:242-252; arithmetic spec
 * cednerf/taichi_kernel/hash_encoder_half.py:67-161 (and hash_encoder_inter.py:121-199 when
 * `temporal` != 0).  Level tables are computed by the host in float64. */
typedef struct ced_hash_desc {
    int32_t n_levels;            /* 1..16; the fused field kernel requires 16 */
    int32_t table_dtype;         /* 0 = float32 entries, 1 = float16 entries */
    int32_t temporal;            /* 0: entry = 2 features; 1: entry = 4 key-frames x 2 features */
    int32_t reserved;
    float scale[CED_MAX_LEVELS];
    uint32_t res[CED_MAX_LEVELS];
    uint32_t offset[CED_MAX_LEVELS];   /* first entry of the level */
    uint32_t size[CED_MAX_LEVELS];     /* entries in the level */
    uint32_t hashed[CED_MAX_LEVELS];   /* 1: xor-prime hash, 0: dense x + y*res + z*res^2 */
    const void *table;           /* device: [total_entries][2 or 8] */
    uint64_t total_entries;
} ced_hash_desc;

/* DNGPradianceField description (host struct).  Replaces the module built at
 * cednerf/model.py:100-344 (xyz_wrap :200-222, direction_encoding :225-239, hash_encoder :242-252,
 * mlp_base :280-290, mlp_head :291-309). */
typedef struct ced_field_desc {
    float aabb[6];
    float moving_step;           /* model.py:151, train_real.py:104,136,169 */
    int32_t use_div_offsets;     /* model.py:356-358 */
    int32_t time_mode;           /* 0 none, 1 SinusoidalEncoder, 2 SinusoidalEncoderWithExp (model.py:386-396) */
    int32_t mlp_precision;       /* CED_MLP_*: arithmetic of the three MLPs (below) */
    int32_t max_workgroups;      /* workgroups of a field launch: 0 = one per CU (256); callers that keep several
                                    frames in flight pass 128 so that two frames' field kernels run side by side.
                                    A per-call launch property (copy the descriptor to vary it), not process state. */
    const void *packed_weights;  /* device: blob written by ced_pack_field_weights[_half] for that precision */
    uint64_t packed_floats;      /* its size in 32-bit words: ced_packed_weight_words() */
    ced_hash_desc hash;
} ced_field_desc;

int ced_version(void);
const char *ced_last_error_string(void);

/* Process-wide options; results are identical for every setting (launch properties that callers vary per call, such
 * as the workgroup count of a field launch, are descriptor fields instead).  Four keys; any other key returns -1:
 * "field_spread_tiles": 1 deals the sample tiles of a launch across all CUs in groups of four before any CU takes
 * more (shorter last round, lower frame latency); 2 (default) does the same inside each XCD, the eight XCDs taking eight
 * contiguous parts of the sample stream (one L2 per table line instead of up to eight); 0 = contiguous tiles per workgroup;
 * "march_two_pass": the frame renderer's first iteration as a culling pass (the sphere trace alone, every ray) and a
 * marching pass over the rays it could not rule out: 1 / 0, -1 (default) = when there are several grid levels;
 * "hash_grad_blocks": cap on the workgroups per level of the hash-table gradient (ced_hash_encode_backward[_temporal]),
 * 0 (default) = no cap, one per 64 samples; a small cap lets the atomics run beside compute-bound kernels of another
 * stream;
 * "frame_sh_per_ray": 1 (default) = the frame renderers (ced_render_image_test / _frames_test / _sharded,
 * ced_render_image) hand the field kernel the colour head's direction inputs computed once per ray in their set-up launch;
 * 0 = the field kernel computes them per sample from rays_d, as it does for ced_field_forward_rays (the same operations:
 * the tests compare the two).
 * (Round 3's "march_sm" -- that pass on persistent waves with lane-level ray fetch -- was bit-exact and 3x slower; removed
 * in round 4, HISTORY 4.2 keeps the measurements.) */
int ced_set_option(const char *key, int value);

/* Arithmetic of xyz_wrap / mlp_base / mlp_head (everything else is fp32 in every mode):
 *   CED_MLP_F32    v_mfma_f32_16x16x4_f32, an ascending-k fp32 FMA chain: bit-identical to the CPU oracle.
 *   CED_MLP_F16X2  every operand split into two fp16 numbers (22 significant bits), three fp16 MFMA
 *                  blocks per product block, fp32 accumulation: fp32-grade results.
 *   CED_MLP_F16    operands rounded to fp16, fp32 accumulation: the precision class of the reference's
 *                  tiny-cuda-nn FullyFusedMLP (cednerf/model.py:200-222,280-309).
 * The half modes assume |weights|, |activations| <= 65504 (activations saturate there), like tcnn. */
#define CED_MLP_F32 0
#define CED_MLP_F16X2 1
#define CED_MLP_F16 2
/*   CED_MLP_F32_HEAD16X2  the chain that decides sample counts, opacity and depth -- xyz_wrap, the hash features,
 *                  mlp_base, trunc_exp (cednerf/model.py:354-445) -- exactly as CED_MLP_F32, bit-identical to the CPU
 *                  oracle; only mlp_head (model.py:447-466), which feeds rgb alone, on split-fp16 operands as
 *                  CED_MLP_F16X2.  sigma, counts, opacity and depth equal the exact mode's bits; rgb within 1e-4. */
#define CED_MLP_F32_HEAD16X2 3

/* Number of floats in the packed (MFMA-fragment-order) fp32 weight blob. */
int64_t ced_packed_weight_floats(int use_div_offsets, int time_mode);

/* HOST function: reorders natural-layout weights W[out][in] (row-major, host pointers) into the
 * fragment-order blob the fused kernel stages into LDS.  Layer dims: xyz_wrap 32-64-64-64-(3|6),
 * mlp_base (32|41)-64-16, mlp_head 19-64-64-3 (model.py:200-222,280-309).  `out` is host memory
 * of ced_packed_weight_floats() floats; upload it and put the device address in
 * ced_field_desc.packed_weights.  Replaces tcnn's flat `params` tensor layout. */
int ced_pack_field_weights(int use_div_offsets, int time_mode,
                           const float *m_w0, const float *m_w1, const float *m_w2, const float *m_w3,
                           const float *b_w0, const float *b_w1,
                           const float *h_w0, const float *h_w1, const float *h_w2,
                           float *out);

/* The same for the half-precision MLP modes: size of the blob in 32-bit words for any mlp_precision, and
 * the HOST packer for CED_MLP_F16X2 / CED_MLP_F16 (weights are rounded to fp16 here; F16X2 also stores the
 * fp16 remainders). */
int64_t ced_packed_weight_words(int use_div_offsets, int time_mode, int mlp_precision);
int ced_pack_field_weights_half(int use_div_offsets, int time_mode, int mlp_precision,
                                const float *m_w0, const float *m_w1, const float *m_w2, const float *m_w3,
                                const float *b_w0, const float *b_w1,
                                const float *h_w0, const float *h_w1, const float *h_w2,
                                void *out);
/* The blob the field kernel for this configuration reads (table_dtype / temporal as in ced_hash_desc): the f16x2 kernels
 * without a time encoding on a plain table run their hidden layers on v_mfma_f32_16x16x32_f16 and need other row / column
 * placements than ced_pack_field_weights_half's; every other configuration gets the same blob as there.  Same size. */
int ced_pack_field_weights_half_for(int use_div_offsets, int time_mode, int mlp_precision, int table_dtype, int temporal,
                                    const float *m_w0, const float *m_w1, const float *m_w2, const float *m_w3,
                                    const float *b_w0, const float *b_w1,
                                    const float *h_w0, const float *h_w1, const float *h_w2,
                                    void *out);
/* HOST packer for CED_MLP_F32_HEAD16X2: `out` holds ced_packed_weight_floats() floats (the head's region carries fp16
 * fragments). */
int ced_pack_field_weights_mixed(int use_div_offsets, int time_mode,
                                 const float *m_w0, const float *m_w1, const float *m_w2, const float *m_w3,
                                 const float *b_w0, const float *b_w1,
                                 const float *h_w0, const float *h_w1, const float *h_w2,
                                 float *out);

/* nerfacc.ray_aabb_intersect(rays_o, rays_d, aabbs, near_plane, far_plane, miss_value)
 * -- call site cednerf/utils.py:215.  Outputs [n_rays, n_aabbs]. */
int ced_ray_aabb_intersect(int64_t n_rays, const float *rays_o, const float *rays_d,
                           int32_t n_aabbs, const float *aabbs,
                           float near_plane, float far_plane, float miss_value,
                           float *t_mins, float *t_maxs, uint8_t *hits, void *stream);

/* The sorted entry / exit events of cednerf/utils.py:219-225: per ray, torch.sort(cat([t_mins, t_maxs], -1), stable=True).
 * t_mins / t_maxs [n_rays, n_grids] (ced_ray_aabb_intersect's) -> t_sorted [n_rays, 2 n_grids], t_indices [n_rays,
 * 2 n_grids] int64 (event id: level for an entry, n_grids + level for an exit), n_grids <= 8.  Equal keys keep their
 * order, NaN keys sort last (torch's rules). */
int ced_sort_intersections(int64_t n_rays, int32_t n_grids, const float *t_mins, const float *t_maxs, float *t_sorted,
                           int64_t *t_indices, void *stream);

/* nerfacc.traverse_grids(...) -- call sites cednerf/utils.py:241-264 and, via
 * OccGridEstimator.sampling, cednerf/utils.py:115-125.  The caller allocates, so the op is split:
 *   mode 0  count: writes counts[n_rays] and termination_planes (t_starts/t_ends/ray_indices unused);
 *   mode 1  fill : writes samples of ray r at base[r] + i (base = exclusive scan of counts);
 *   mode 2  over-allocate (nerfacc `over_allocate=True`): ray r owns slots [r*limit, (r+1)*limit),
 *           counts[r] tells how many are valid; `base` unused; requires limit > 0;
 *   mode 3  fill, with `base` = INCLUSIVE scan of the counts of a preceding mode-0 call and
 *           `counts` still holding those counts (start of ray r = base[r] - counts[r]).
 * packed_info_out (may be NULL): [n_rays,2] = (start, count) written by the same launch.
 * near_planes and termination_planes may alias (each ray reads its near plane before writing).
 * rays_mask may be NULL (all rays).  ray_indices may be NULL.  binaries: [n_grids,res,res,res]
 * bytes; t_sorted/t_indices: [n_rays, 2*n_grids]; hits: [n_rays, n_grids].  limit <= 0: no limit.
 * Implemented in csrc/march.hip on traverse_ray of csrc/march_accel.hpp (the frame renderer's helpers, no distance
 * fields); ced_host_march_frame(walk = 3) runs the same function on the host. */
int ced_traverse_grids(int64_t n_rays, const float *rays_o, const float *rays_d,
                       const uint8_t *binaries, int32_t n_grids, int32_t res, const float *aabbs,
                       const float *near_planes, const float *far_planes,
                       float step_size, float cone_angle, int32_t limit, const uint8_t *rays_mask,
                       const float *t_sorted, const int64_t *t_indices, const uint8_t *hits,
                       int32_t mode, const int64_t *base,
                       int64_t *counts, float *t_starts, float *t_ends, int64_t *ray_indices,
                       float *termination_planes, int64_t *packed_info_out, void *stream);

/* ---- occupancy acceleration structure of the frame renderer ----
 * Chebyshev distance fields over `binaries` (per 8^3-cell brick and per cell): the frame renderer's marching
 * sphere-traces them through empty space and re-enters the exact cell walk in closed form (csrc/march_accel.hpp), so
 * the emitted samples are those of nerfacc.traverse_grids (cednerf/utils.py:241-264) bit for bit.  Build it once per
 * occupancy-grid update (train_real.py:332-336) and hand it to ced_render_image_test / ced_render_frames_test; with
 * NULL there only the brick-level field is built, inside every call.
 * accel: device memory of ced_occupancy_accel_bytes(n_grids, res) bytes. */
int64_t ced_occupancy_accel_bytes(int32_t n_grids, int32_t res);
int ced_build_occupancy_accel(const uint8_t *binaries, int32_t n_grids, int32_t res, void *accel, int64_t accel_bytes,
                              void *stream);

/* HOST functions (validation aids, no GPU needed): the acceleration structure built on the host (accel_host:
 * ced_occupancy_accel_bytes() bytes of host memory, same layout as the device one); the closed-form DDA re-entry  k = 0; while (k < kcap && *x < tau) { *prev = *x; *x += d; ++k; }
 * and the frame renderer's marching of n_rays rays with the SAME code the device runs (march_accel.hpp is host +
 * device): counts[r] samples (<= limit) at t_starts/t_ends[r * limit + i]; t_term[r] is the termination plane when
 * counts[r] == limit (unspecified otherwise: such a ray is dead, cednerf/utils.py:303-306).  accel_mode: 0 = plain
 * cell-by-cell walk, 1 = brick field only (what a render call builds for itself), 2 = brick + cell fields (what
 * ced_build_occupancy_accel provides).  use_lattice: far skips start from the table of first lattice points per
 * binade, as in a frame with cone_angle == 0 (every near plane must then be a point of the lattice t_0 = near_planes[0],
 * t_{k+1} = t_k + step: the frame's near plane or an earlier termination plane).  walk selects what runs: the
 * instantiations of the walker traverse_ray_frame -- 0 = a frame's later iterations (no trace at a segment's start,
 * emission inline), 1 = a frame's first iteration (trace first, looking loop + emission phase), 2 = the one-shot march
 * (trace first, emission inline) -- or 3 = traverse_ray, the walk of ced_traverse_grids' kernel (the same helpers,
 * look-ahead of 8 cells, events always read from t_sorted / t_indices; t_term[r] is then the termination plane of EVERY
 * ray; it has neither distance fields nor a lattice: pass accel_mode 0 and use_lattice 0, other values are ignored).
 * All pointers are host pointers. */
int ced_host_build_occupancy_accel(const uint8_t *binaries_host, int32_t n_grids, int32_t res, uint8_t *accel_host);
int32_t ced_host_count_steps(float *x, float d, float tau, int32_t kcap, float *prev);
int ced_host_march_frame(int64_t n_rays, const float *rays_o, const float *rays_d, const uint8_t *binaries,
                         int32_t n_grids, int32_t res, const float *aabbs, const float *near_planes, float far_plane,
                         float step_size, float cone_angle, int32_t limit, const float *t_sorted,
                         const int64_t *t_indices, const uint8_t *hits, const uint8_t *accel_host, int32_t accel_mode,
                         int32_t use_lattice, int32_t walk, int32_t *counts, float *t_starts, float *t_ends,
                         float *t_term);

/* HOST functions (validation aids): the group clearance of the frame renderer's first iteration (csrc/march_accel.hpp,
 * group_clear), with the code the device runs.  ced_host_ray_group_clear: for every frame and every group of 64
 * consecutive rays of it (the last group may be partial; with local_rays [n_frames], host, only the first local_rays[f]
 * rays of frame f are members) one float t_clear[f * ceil(rays_per_frame / 64) + k]: no member ray meets an occupied
 * cell of any level at a parameter t < t_clear (+inf: nowhere between the planes; 0: nothing is claimed, e.g. a
 * non-finite ray component).  Precondition near_plane >= 0 (the cone bound holds for t >= 0): with a negative near plane
 * every group gets 0, and the renderers compute nothing and pass no hint.  accel_mode 1 = brick field only, 2 = brick +
 * cell fields.
 * ced_host_march_frame_hinted: ced_host_march_frame with a hint per ray, t_hint [n_rays] -- nothing occupied is met
 * before it (a ray's group clearance); a hint of 0 or less claims nothing and never moves the start of a segment, so
 * segments below 0 (negative near planes) walk as without hints.  The trace at a segment's start probes from there.  Same samples, counts
 * and termination planes as without hints (walks 0..2; walk 3 takes no hint). */
int ced_host_ray_group_clear(int32_t n_frames, int64_t rays_per_frame, const int32_t *local_rays, const float *rays_o,
                             const float *rays_d, int32_t n_grids, int32_t res, const float *aabbs,
                             const uint8_t *accel_host, int32_t accel_mode, float near_plane, float far_plane,
                             float *t_clear);
int ced_host_march_frame_hinted(int64_t n_rays, const float *rays_o, const float *rays_d, const uint8_t *binaries,
                                int32_t n_grids, int32_t res, const float *aabbs, const float *near_planes,
                                float far_plane, float step_size, float cone_angle, int32_t limit, const float *t_sorted,
                                const int64_t *t_indices, const uint8_t *hits, const uint8_t *accel_host,
                                int32_t accel_mode, int32_t use_lattice, int32_t walk, const float *t_hint,
                                int32_t *counts, float *t_starts, float *t_ends, float *t_term);

/* HOST function (validation aid): the kernels' empty-space skip -- advance t_last by whole steps
 * dt = clamp(t*cone_angle, step_size, 1e10) until t_last + dt/2 >= target -- evaluated on the host
 * with the same code the device runs (closed form when cone_angle == 0). */
float ced_host_skip_march(float t_last, float target, float step_size, float cone_angle);

/* hash_encoder(x): the tcnn HashGrid forward at cednerf/model.py:384 (spec
 * hash_encoder_half.py:112-161).  x [n,3] in [0,1] (clamped), t [n] or NULL (temporal only),
 * out [n, 2*n_levels] level-major (hash_encoder_half.py:339-345,385). */
int ced_hash_encode(const ced_hash_desc *desc, int64_t n, const float *x, const float *t,
                    float *out, void *stream);

/* Backward of ced_hash_encode (non-temporal tables): the training-path row of SURVEY 8f, restating
 * hash_encoder_backward_kernel, taichi_kernel/hash_encoder_half.py:164-226.  dy [n, 2*n_levels] is the gradient
 * w.r.t. the encoder output; grad_table [total_entries, 2] fp32 is ACCUMULATED into (one hardware atomic add per
 * corner and feature; zero it first for a fresh gradient, as HashEncoder.backward does at :362-364); dx [n, 3]
 * (optional) receives the position gradient: dx_scaled = 0 as the reference computes it (per level w.r.t. the
 * scaled position, i.e. without the `scale` factor), dx_scaled = 1 the gradient w.r.t. x itself.  grad_table may be
 * NULL when dx is given (position gradient only): the two halves are independent launches and a caller may run them on
 * different streams. */
int ced_hash_encode_backward(const ced_hash_desc *desc, int64_t n, const float *x, const float *dy,
                             float *grad_table, float *dx, int32_t dx_scaled, void *stream);

/* Backward of ced_hash_encode for TEMPORAL tables (desc->temporal: entry = 4 key-frames x 2 features), restating
 * hash_encoder_backward_kernel of taichi_kernel/hash_encoder_inter.py:202-275: t [n] the sample times; grad_table
 * [total_entries, 8] fp32 is ACCUMULATED into -- per corner the key-frames k and k + 1 of the sample's time receive
 * w * dy * (1 - t_frac) and w * dy * t_frac (k, t_frac as in the forward, :228-240).  Like the reference's autograd
 * function (:403-420) it yields the table gradient only: positions and times get none through this encoder. */
int ced_hash_encode_backward_temporal(const ced_hash_desc *desc, int64_t n, const float *x, const float *t,
                                      const float *dy, float *grad_table, void *stream);

/* DNGPradianceField.forward(positions, t, directions) -- cednerf/model.py:468-488 (query_move
 * :354-365, query_density :367-445, _query_rgb :447-466), fused into one kernel.
 * dir/rgb may both be NULL (density only = query_density, model.py:367); geo [n,15] may be NULL
 * (= results['base_mlp_out']). */
int ced_field_forward(const ced_field_desc *desc, int64_t n, const float *positions, const float *t,
                      const float *directions, float *rgb, float *sigma, float *geo, void *stream);

/* The sigma_fn / rgb_sigma_fn closures of the render drivers (cednerf/utils.py:74-104,181-195)
 * fused with the field: positions = o[ray] + d[ray]*(t0+t1)/2, t = timestamps[t_per_ray ? ray : 0].
 * want_rgb == 0 evaluates the density only (sigma_fn).
 * n_dev (may be NULL): device scalar; the kernel evaluates min(n, *n_dev) samples, so a caller
 * that only knows an upper bound of the sample count on the host needs no device->host sync. */
int ced_field_forward_rays(const ced_field_desc *desc, int64_t n, const int64_t *n_dev,
                           const float *rays_o, const float *rays_d,
                           const int64_t *ray_indices, const float *t_starts, const float *t_ends,
                           const float *timestamps, int32_t t_per_ray, int32_t want_rgb,
                           float *rgb, float *sigma, void *stream);

/* ---- the deformation field on its own ----
 * DNGPradianceField.query_move(x, t) -- cednerf/model.py:354-365 -- with the normalisation that follows it in
 * query_density (:378-383): tcnn Frequency encoding of (x, y, z, t), xyz_wrap, move = out * moving_step (with
 * use_div_offsets: out[:3] * step + tanh(out[3:]) * step), x_move = x + move, x_norm = (x_move - aabb_min) /
 * (aabb_max - aabb_min) (NOT clamped), selector = all(0 < x_norm < 1).  The motion network runs in the arithmetic
 * desc->mlp_precision gives it inside ced_field_forward, on the same packed blob: the values are the ones the fused
 * kernel computes internally, bit for bit.  The hash table is not read (desc->hash.temporal still says which blob layout
 * the f16x2 mode uses).  x_move, move, x_norm [n,3] and selector [n] (uint8, 0 / 1) may each be NULL, not all of them. */
int ced_field_move(const ced_field_desc *desc, int64_t n, const float *positions, const float *t,
                   float *x_move, float *move, float *x_norm, uint8_t *selector, void *stream);

/* The same at the sample positions of the sigma_fn / rgb_sigma_fn closures: positions, timestamps, t_per_ray and n_dev
 * as in ced_field_forward_rays (samples past min(n, *n_dev) are left untouched).  move, x_norm [n,3]: either may be
 * NULL, not both. */
int ced_field_move_rays(const ced_field_desc *desc, int64_t n, const int64_t *n_dev,
                        const float *rays_o, const float *rays_d,
                        const int64_t *ray_indices, const float *t_starts, const float *t_ends,
                        const float *timestamps, int32_t t_per_ray, float *move, float *x_norm, void *stream);

/* ---- the warp's inverse: where a material point sits at time t ----
 * The density at (x, t) is the canonical density at c = x + move(x, t), `move` being ced_field_move's.  A material point
 * with canonical coordinate c therefore sits at time t at the solution x of  x + move(x, t) = c.  These entries solve it
 * by fixed-point iteration.  Per row, with target c, time t, a start (init's row, or c when init is NULL),
 * max_iters = K (1 .. 1024) and tol (>= 0), every operation in fp32 with one rounding:
 *     x = start; evals = 0; step = +inf
 *     repeat while evals < K:
 *         m = move(x, t)                      -- ced_field_move's `move` at (x, t) in desc->mlp_precision, bit for bit
 *         x_new[a] = c[a] - m[a]              -- one subtraction per component
 *         step = fmaxf(fmaxf(|x_new[0] - x[0]|, |x_new[1] - x[1]|), |x_new[2] - x[2]|)
 *         x = x_new; evals += 1
 *         if step <= tol: stop                -- false for a NaN step: such a row runs all K rounds
 * Outputs: x [n,3], step [n] (the size of the last update), evals [n] int32; each may be NULL, not all.  A row has
 * converged iff step <= tol.  There is no damping, no Newton step and no Jacobian: the iteration converges where
 * move(., t) is a contraction (its Lipschitz constant scales with moving_step) and reports the rows where it did not
 * through step and evals == K.  A row's result does not depend on n or on the other rows: a finished row is frozen while
 * its wave goes on, and a wave stops early only when all of its rows are frozen. */
int ced_field_move_inverse(const ced_field_desc *desc, int64_t n, const float *target, const float *t,
                           const float *init, int32_t max_iters, float tol, float *x, float *step,
                           int32_t *evals, void *stream);

/* The same for every (time, point) pair without expanding either input: row r = k * n_points + p takes times[k]
 * ([n_times]), target[p] and init[p] ([n_points,3]; init may be NULL); x [n_times, n_points, 3], step and evals
 * [n_times, n_points].  Each row has the bits of ced_field_move_inverse on the expanded rows. */
int ced_field_track(const ced_field_desc *desc, int64_t n_points, int64_t n_times, const float *target,
                    const float *times, const float *init, int32_t max_iters, float tol, float *x,
                    float *step, int32_t *evals, void *stream);

/* ---- the derivative of the warp ----
 * move [n,3] and jac [n,12], jac[r, 4a + b] = d move_a / d (x, y, z, t)_b, from one launch; either may be NULL, not
 * both.  `move` is ced_field_move's `move`, bit for bit, in desc->mlp_precision.  The Jacobian is computed in forward
 * mode: four tangent vectors per sample (directions b = x, y, z, t) pushed through the four layers beside the primal,
 * as four more matrix-instruction columns on the same weights, in this order:
 *   encoding   the feature sin(2^k pi v_d + phase) of dimension d has the tangent, for direction b == d,
 *                  w * q   with w = fp32(pi) * 2^k (exact) and q the primal feature of the OTHER phase of that frequency,
 *              negated when the feature itself is the cosine; for b != d it is 0.  fp32 chain: q is the fp32 feature.
 *              f16 / f16x2: the product is formed in fp32 from the fp32 features, then rounded to fp16 / split into
 *              hi + lo like the primal features.
 *   layers     every layer multiplies the tangents by the layer's weights in the mode's own layer arithmetic (fp32
 *              MFMA chain in ascending k; fp16 or split-fp16 blocks with fp32 accumulation, the f16x2 blob's two
 *              layouts included), exactly as it multiplies the primal.
 *   ReLU       a hidden layer's tangent is set to 0 wherever the PRIMAL pre-activation is not > 0; f16 / f16x2: it is
 *              then clamped to +-65504 and rounded / split like the primal activation.
 *   output     with (off, fine) the last layer's rows and (d off, d fine) their tangents, step = moving_step:
 *                  use_div_offsets == 0:   jac = (d off_a) * step
 *                  otherwise:              s = 1 - th_a * th_a;   jac = (d off_a + s * d fine_a) * step
 *              th_a being the tanh value ced_field_move computes for `move`; every operation one fp32 rounding. */
int ced_field_move_jacobian(const ced_field_desc *desc, int64_t n, const float *positions, const float *t,
                            float *move, float *jac, void *stream);

/* The warp's inverse by Newton's method on that Jacobian: arguments, outputs and refusals of ced_field_move_inverse.
 * Per row, with target c, time t, a start (init's row, or c when init is NULL), max_iters = K and tol, every line in
 * fp32, every product, sum, difference and quotient rounded on its own (no fused multiply-add):
 *     x = start
 *     for k = 1 .. K:
 *         (m, J) = ced_field_move_jacobian at (x, t)           -- its bits, in desc->mlp_precision
 *         r[a] = (x[a] + m[a]) - c[a]
 *         step = fmaxf(fmaxf(|r[0]|, |r[1]|), |r[2]|);  evals = k
 *         if step <= tol or k == K: stop                      -- `step <= tol` is false for a NaN
 *         A = I + J[:, :3]                                      -- A[a][a] = 1.0f + J[a][a], A[a][b] = J[a][b]
 *         C[a][b] = A[a+1][b+1] * A[a+2][b+2] - A[a+1][b+2] * A[a+2][b+1]      -- cofactors, indices mod 3
 *         det = (A[0][0] * C[0][0] + A[0][1] * C[0][1]) + A[0][2] * C[0][2]
 *         d[a] = ((C[0][a] * r[0] + C[1][a] * r[1]) + C[2][a] * r[2]) / det    -- the adjugate is C transposed
 *         if !(|det| >= 2^-20) or some d[a] is not finite: d = r               -- the fixed-point step
 *         x[a] = x[a] - d[a]
 * Outputs: x [n,3], step [n], evals [n] int32.  `step` is the max-norm residual |x + move(x, t) - c| of the RETURNED x,
 * and a row has converged iff step <= tol.  There is no line search and no damping: rows that do not converge are
 * reported through step and evals == K, as by the fixed-point entries.  Where the warp folds (det(I + J_x) <= 0
 * somewhere between the start and a solution) the equation has several solutions and Newton may land on another
 * preimage of c than the fixed-point iteration, or on none.  A row's result does not depend on n or on the other rows
 * (finished rows are frozen, a wave leaves the loop when all of its rows are). */
int ced_field_move_inverse_newton(const ced_field_desc *desc, int64_t n, const float *target, const float *t,
                                  const float *init, int32_t max_iters, float tol, float *x, float *step,
                                  int32_t *evals, void *stream);

/* ced_field_track's broadcast (row r = k * n_points + p) on the Newton iteration: each row has the bits of
 * ced_field_move_inverse_newton on the expanded rows. */
int ced_field_track_newton(const ced_field_desc *desc, int64_t n_points, int64_t n_times, const float *target,
                           const float *times, const float *init, int32_t max_iters, float tol, float *x,
                           float *step, int32_t *evals, void *stream);

/* ---- the velocity of the warp ----
 * Where the material point that sits at x at time t is going: differentiating x(t) + move(x(t), t) = c in t gives
 *     v = -(I + J_x)^-1 d move / dt
 * with J = ced_field_move_jacobian's jac of the row (its bits, in desc->mlp_precision), from the same launch: the
 * Jacobian is not written out.  Per row, r = J[:, 3] (the time column), every line in fp32, every product, sum, difference
 * and quotient rounded on its own (no fused multiply-add) -- the Newton step's arithmetic on another right-hand side:
 *     A = I + J[:, :3]                                          -- A[a][a] = 1.0f + J[a][a], A[a][b] = J[a][b]
 *     C[a][b] = A[a+1][b+1] * A[a+2][b+2] - A[a+1][b+2] * A[a+2][b+1]      -- cofactors, indices mod 3
 *     det = (A[0][0] * C[0][0] + A[0][1] * C[0][1]) + A[0][2] * C[0][2]
 *     d[a] = ((C[0][a] * r[0] + C[1][a] * r[1]) + C[2][a] * r[2]) / det
 *     valid = det >= 2^-20 and every |d[a]| < infinity           -- false for a NaN
 *     v[a] = valid ? -d[a] : 0
 * A determinant that is not positive is a fold of the warp (several material points share x, none has "the" velocity) and
 * is not valid, unlike in the Newton step, which only asks for |det| >= 2^-20.  A row that is not valid has velocity 0
 * exactly, so that a sum of w_i * v_i along a ray stays finite; `det` is stored as computed, whatever `valid` says.
 * Outputs: velocity [n,3], det [n], valid [n] uint8 (1 / 0); each may be NULL, not all three.  A row's outputs do not
 * depend on n or on the other rows. */
int ced_field_velocity(const ced_field_desc *desc, int64_t n, const float *positions, const float *t,
                       float *velocity, float *det, uint8_t *valid, void *stream);

/* The same at the sample positions of the sigma_fn / rgb_sigma_fn closures: positions, timestamps, t_per_ray and n_dev
 * as in ced_field_move_rays (rows past min(n, *n_dev) are left untouched; a negative ray index is evaluated on ray 0 at
 * distance 0). */
int ced_field_velocity_rays(const ced_field_desc *desc, int64_t n, const int64_t *n_dev,
                            const float *rays_o, const float *rays_d,
                            const int64_t *ray_indices, const float *t_starts, const float *t_ends,
                            const float *timestamps, int32_t t_per_ray, float *velocity, float *det, uint8_t *valid,
                            void *stream);

/* ---- the derivative of the density ----
 * sigma [n] and three gradients [n,3] per row (x, t), all in world units, from one launch; each output may be NULL, not
 * all.  sigma is ced_field_forward's, bit for bit, in desc->mlp_precision.  `grad` is what torch.autograd.grad(
 * density.sum(), x) returns on the reference's graph (cednerf/model.py:354-445), under four rules:
 *   time encoding  a constant (model.py:386-396 runs it under no_grad), its attenuation by |move| included;
 *   activation     trunc_exp's backward (cednerf/utils.py:27-43), exp(min(raw - 1, 15)): slope = fminf(s, kExp15) with s the
 *                  forward's exp(raw - 1), its own bits, and kExp15 = 3269017.25f, the float32 nearest e^15;
 *   hash grid      piecewise trilinear: inside the cell the encode's own fp32 floor selects, d frac / d x_norm = scale_l
 *                  exactly; the temporal table's derivative is the same formula on the time-interpolated corner values;
 *   outside        where the selector is false, sigma and every gradient output are 0.
 * Forward mode: three tangent vectors per row (the axes of x_norm) through mlp_base beside the primal, as three more
 * matrix-instruction columns on the same weights:
 *   encoding   with v[c] corner c's two values (temporal table: v_k * (1 - t_frac) + v_(k+1) * t_frac, as the encode forms
 *              them), frac / 1 - frac the encode's own fp32 fractions and K = ceil(log2(the largest level scale)):
 *                  g_a = sum over the four corner pairs along axis a, ascending, of
 *                        fma(w, v[upper] - v[lower], g_a),  w = the product of the other two axes' weights
 *                  d feature / d x_norm[a] = g_a * (scale_l * 2^-K)
 *              The tangents are carried scaled by the exact 2^-K so that they stay inside the fp16 range; f16 / f16x2:
 *              clamped to +-65504, then rounded to fp16 / split into hi + lo like the primal features.  The tangents of
 *              the nine time features are 0.
 *   layers     mlp_base's two layers multiply the tangents in the mode's own layer arithmetic, exactly as the primal.
 *   ReLU       the hidden tangent is set to 0 wherever the PRIMAL pre-activation is not > 0; f16 / f16x2: then clamped
 *              to +-65504 and rounded / split like the primal activation.
 * Then, with d[a] the raw density's three tangents, extent[a] = aabb[3 + a] - aabb[a] and J = ced_field_move_jacobian's
 * jac of the row (its bits), every line in fp32, every product, sum and quotient rounded on its own (no fused
 * multiply-add):
 *     dlog_canonical[a] = (d[a] * 2^K) / extent[a]
 *     dlog[b] = dlog_canonical[b] + ((J[0][b] * dlog_canonical[0] + J[1][b] * dlog_canonical[1]) + J[2][b] * dlog_canonical[2])
 *     grad[b] = slope * dlog[b]
 * dlog_canonical is the gradient of the pre-activation density with respect to the canonical point c = x + move(x, t)
 * (the gradient of log sigma below the clamp), dlog = (I + J_x)^T dlog_canonical the same with respect to the observed
 * point x.  A row's outputs do not depend on n or on the other rows. */
int ced_field_density_gradient(const ced_field_desc *desc, int64_t n, const float *positions, const float *t,
                               float *sigma, float *grad, float *dlog, float *dlog_canonical, void *stream);

/* The same at the sample positions of the sigma_fn / rgb_sigma_fn closures: positions, timestamps, t_per_ray and n_dev
 * as in ced_field_move_rays (rows past min(n, *n_dev) are left untouched). */
int ced_field_density_gradient_rays(const ced_field_desc *desc, int64_t n, const int64_t *n_dev,
                                    const float *rays_o, const float *rays_d,
                                    const int64_t *ray_indices, const float *t_starts, const float *t_ends,
                                    const float *timestamps, int32_t t_per_ray, float *sigma, float *grad, float *dlog,
                                    float *dlog_canonical, void *stream);

/* ---- the density's maximum over windows of time, and occupancy slices made from it ----
 * What a time-sliced occupancy grid is built from: n positions, B windows ("bins") of S probe times each, one launch.
 *     out[b, p] = fmaxf over s = 0 .. S-1 of sigma(positions[p], times[b * S + s])
 * The maximum starts from 0.0f.  sigma has ced_field_forward's bits in the descriptor's arithmetic (desc->mlp_precision,
 * either f16x2 layout, time_mode 0 / 1 / 2, use_div_offsets on and off, fp32 / fp16 / temporal tables), 0 outside the box.
 * fmaxf ignores a NaN density: a cell whose density is NaN at every probe keeps 0, as `occs > thre` is false for a NaN.
 * times [B * S] floats on the device (each in [0, 1], as for ced_field_forward), out [B, n] floats.  A wave keeps its rows'
 * positions and running maxima in registers across the whole loop: besides positions, times and out only the hash table's
 * gathers touch device memory; a probe time that equals the one before it bit for bit is not evaluated twice.  Limits: 1 <= B <= CED_TIME_MAX_BINS, 1 <= S <= CED_TIME_MAX_TIMES, n >= 0; n == 0 launches
 * nothing.  A row's outputs do not depend on n or on the other rows. */
#define CED_TIME_MAX_BINS 256
#define CED_TIME_MAX_TIMES 64
int ced_field_density_time_max(const ced_field_desc *desc, int64_t n, const float *positions, int32_t n_bins,
                               int32_t n_times, const float *times, float *out, void *stream);

/* B occupancy grids [levels, R, R, R] from those maxima.  cell_ids [n] int64 lists the probed cells as level * R^3 + cell
 * (cell = (ix * R + iy) * R + iz), max_sigma [B, n] their maxima.  With M = levels * R^3:
 *     hit[b, id]    = __fmul_rn(max_sigma[b, p], step_size) > thre   for id = cell_ids[p], 0 for a cell that is not listed
 *                     (false for a NaN; an id outside 0 .. M-1 is skipped)
 *     out[b, l, c]  = (dilate == 0 ? hit[b, l, c] : OR of hit[b, l, c'] over the 3x3x3 neighbourhood c' of c inside level l)
 *                     AND (union_binaries == NULL or union_binaries[l, c] != 0)
 * out [B, levels, R, R, R] bytes (1 / 0), union_binaries [levels, R, R, R] bytes or NULL.  Two plain kernels (mark, then
 * dilate / AND), no atomics: a cell's byte is written by the one row that lists it; listing a cell twice is allowed only
 * with equal maxima.  workspace holds hit: ced_occ_time_slices_workspace_bytes(B, levels, R) bytes of device memory
 * (negative for sizes outside 1 <= B <= CED_TIME_MAX_BINS, 1 <= levels <= 64, 1 <= R <= 1024), ZEROED BY THE CALLER before
 * the first call of a build.  out == NULL marks only: a build may hand its rows over in several calls (max_sigma is then
 * [B, n] of that call's rows) and passes out with the last, which marks its rows and then writes every slice.  dilate is
 * 0 or 1. */
int64_t ced_occ_time_slices_workspace_bytes(int32_t n_bins, int32_t levels, int32_t res);
int ced_occ_time_slices(int64_t n, const int64_t *cell_ids, const float *max_sigma, int32_t n_bins, float step_size,
                        float thre, int32_t levels, int32_t res, const uint8_t *union_binaries, int32_t dilate,
                        uint8_t *out, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- the density's level set along rays: the first crossing per ray, then bisection on the field ----
 * ced_surface_first_crossing: per ray of packed_info [n_rays, 2] int64 (first sample, count) over the samples t_starts /
 * t_ends / sigmas [S]:
 *     k  = the index (into the S samples) of the ray's first sample with sigma >= thresh; a NaN never qualifies;
 *          -1 if there is none or the ray has no samples
 *     hi = (t_starts[k] + t_ends[k]) / 2
 *     lo = (t_starts[k-1] + t_ends[k-1]) / 2 if sample k-1 belongs to the same ray and t_ends[k-1] == t_starts[k]
 *          (contiguous), else t_starts[k]
 *     lo = hi = 0 for k = -1
 * each a single float32 operation.  k [n_rays] int64, lo / hi [n_rays] floats.  One lane per ray on the compositing
 * kernels' sample walk, no atomics: deterministic.
 *
 * ced_field_level_set: per row a ray o + d * t, a bracket [lo, hi] and a time (times [n], or [1] with t_per_row == 0).
 * With every line one float32 operation, no contraction,
 *     p(t) = o + d * t                       (multiply, then add, per axis)
 *     f(t) = sigma(p(t), time)               (ced_field_forward's bits in the descriptor's arithmetic, 0 outside the box)
 *     s_lo = f(lo); s_hi = f(hi); evals = 2
 *     status 1 if s_lo >= thresh:            t = lo, sigma = s_lo, width = 0
 *     status 2 else if !(s_hi >= thresh):    t = hi, sigma = s_hi, width = hi - lo
 *     status 0 otherwise; then at most max_iters rounds:
 *         if hi - lo <= tol: stop
 *         m = (lo + hi) / 2;  if m == lo or m == hi: stop
 *         s = f(m); evals += 1
 *         if s >= thresh: hi = m, s_hi = s   else: lo = m        (a NaN goes to lo)
 *       t = hi, sigma = s_hi, width = hi - lo
 * so that a status-0 row holds f(t - width) < thresh <= f(t).  Outputs, any of which may be NULL (not all): t [n],
 * x [n,3] = p(t), sigma [n], width [n], status [n] int32, evals [n] int32.  A wave keeps its rows and their brackets in
 * registers across the rounds; a row's outputs do not depend on n or on the other rows.  Limits: thresh > 0,
 * 0 <= max_iters <= CED_LEVEL_SET_MAX_ITERS, tol >= 0, n >= 0; n == 0 launches nothing. */
#define CED_LEVEL_SET_MAX_ITERS 64
int ced_surface_first_crossing(int64_t n_rays, const int64_t *packed_info, const float *t_starts, const float *t_ends,
                               const float *sigmas, float thresh, int64_t *k, float *lo, float *hi, void *stream);
int ced_field_level_set(const ced_field_desc *desc, int64_t n, const float *origins, const float *dirs, const float *lo,
                        const float *hi, const float *times, int32_t t_per_row, float thresh, int32_t max_iters, float tol,
                        float *t, float *x, float *sigma, float *width, int32_t *status, int32_t *evals, void *stream);

/* DNGPradianceField._query_rgb(dir, embedding, apply_act) -- cednerf/model.py:447-466: dirs [n,3] are normalised,
 * mapped to [0,1], SH degree 2; mlp_head on [SH(4), embedding(15)]; the sigmoid iff apply_act.  embedding [n,15] is what
 * ced_field_forward writes to `geo`; rgb [n,3].  The head runs in the arithmetic of desc->mlp_precision. */
int ced_field_rgb(const ced_field_desc *desc, int64_t n, const float *dirs, const float *embedding,
                  int32_t apply_act, float *rgb, void *stream);

/* The same head on m * n_dirs rows without expanding either input: row r = e * n_dirs + d reads embedding[e] ([m,15]) and
 * dirs[d] ([n_dirs,3]); rgb [m, n_dirs, 3].  Each row's arithmetic is ced_field_rgb's: the bits are those of
 * ced_field_rgb on the expanded inputs. */
int ced_field_rgb_bcast(const ced_field_desc *desc, int64_t m, int32_t n_dirs, const float *dirs,
                        const float *embedding, int32_t apply_act, float *rgb, void *stream);

/* ---- volume export (vis.py:13-46: nerfvis.add_nerf's grid of the field, without nerfvis) ----
 * The reso^3 cells of the cube [center - radius, center + radius]^3, flat index i = (ix * reso + iy) * reso + iz, centre
 * p_a = lo_a + (i_a + 0.5f) * h with lo_a = center_a - radius and h = (2 * radius) / reso, all fp32, multiply then add.
 * Both entries compact in input order (ascending cell index; no atomically claimed slots), write the first
 * min(*count, capacity) kept rows and the number of kept rows to the device scalar *count; capacity = 0 only counts
 * (outputs may be NULL).  workspace: ced_bake_workspace_bytes(n) bytes of device memory, n = n_cells resp. n. */
int64_t ced_bake_workspace_bytes(int64_t n);

/* Cells [first_cell, first_cell + n_cells) worth evaluating.  binaries [levels, R, R, R] (bytes) with aabbs [levels, 6]
 * on the device: a cell is kept iff some level's box contains its centre (faces included) and, in the first such level,
 * the grid cell clamp((int)(((p - min) / extent) * R), 0, R - 1) -- the marcher's expression -- is set.  binaries NULL:
 * every cell is kept.  The levels must be ordered from the smallest box to the largest (OccGridEstimator's nested
 * levels are): "smallest containing level" is the first in array order.  center_host: 3 floats on the host.  index [capacity] int64, xyz [capacity, 3]. */
int ced_bake_candidates(int32_t reso, const float *center_host, float radius, int64_t first_cell, int64_t n_cells,
                        const uint8_t *binaries, const float *aabbs, int32_t levels, int32_t grid_res,
                        int64_t capacity, int64_t *index, float *xyz, int64_t *count, void *workspace,
                        int64_t workspace_bytes, void *stream);

/* Of n candidate rows (index_in [n], xyz_in [n,3]) with ced_field_forward's sigma_in [n] and geo as embedding_in [n,15],
 * the rows with sigma >= sigma_thresh (a NaN does not pass), copied to index / xyz / sigma / embedding. */
int ced_bake_select(int64_t n, const int64_t *index_in, const float *xyz_in, const float *sigma_in,
                    const float *embedding_in, float sigma_thresh, int64_t capacity, int64_t *index, float *xyz,
                    float *sigma, float *embedding, int64_t *count, void *workspace, int64_t workspace_bytes,
                    void *stream);

/* ---- mesh export: naive surface nets on the lattice of cell centres ----
 * Definition (issue "Extract a triangle mesh of the field per time step, in HIP"; tests/mesh_reference.py restates it in
 * numpy).  All arithmetic is fp32, one rounding per operation.
 * Lattice: reso nodes per axis (1 .. 512), node (ix,iy,iz) has id (ix * reso + iy) * reso + iz and the position of the
 *   volume export's cell centre, lo_a + (i_a + 0.5f) * h.  S[n] = lattice[n]; in(n) = S[n] >= thresh (false for a NaN).
 * Vertices: a cube is named by its lowest corner c (every coordinate < reso - 1) and is active when its 8 corners are
 *   neither all inside nor all outside; the active cubes in ascending id are the vertices.  Its 12 edges are walked in the
 *   order: (a,b,c') in (x,y,z),(y,z,x),(z,x,y); ob in 0,1; oc in 0,1; from corner p0 (p0[a] = 0, p0[b] = ob, p0[c'] = oc)
 *   to p1 = p0 + e_a, s0 = S[p0], s1 = S[p1].  Always g[a] += (s1 - s0); if in(p0) != in(p1): mu = (thresh - s0) / (s1 - s0),
 *   a non-finite mu becomes 0.5, mu is clamped to [0,1], acc += (p0 with its a-th component replaced by mu), cnt += 1.
 *   u = acc / (float)cnt; vertex_a = lo_a + (((float)c_a + 0.5f) + u_a) * h; normal = -g / |g| with
 *   |g| = sqrtf((g_x^2 + g_y^2) + g_z^2), the zero vector when |g| is 0 or not finite.
 * Faces: lattice edge (n, a), n_a < reso - 1, has key 3 * id(n) + a and is active when in(n) != in(n + e_a) and
 *   1 <= n_b, n_c' <= reso - 2 (all four cubes around it exist).  Its quad is the vertex ids of the cubes q0 = n - e_b - e_c',
 *   q1 = n - e_c', q2 = n, q3 = n - e_b, as the triangles (q0,q1,q2),(q0,q2,q3) if in(n), else (q0,q2,q1),(q0,q3,q2):
 *   outward-facing.  Faces ascend with the edge key; sign-changing edges on the lattice border emit none (the mesh is open
 *   there) and vertices no face references are kept.
 * Both entries compact in ascending item order (no atomically claimed slots), write the first min(*count, capacity) kept
 * items and the number of kept items to the device scalar *count; capacity = 0 only counts (outputs may be NULL).
 * workspace: ced_mesh_workspace_bytes(reso) bytes of device memory (-1 for a reso outside 1 .. 512). */
int64_t ced_mesh_workspace_bytes(int32_t reso);

/* lattice [reso^3] on the device, center_host: 3 floats on the host.  *count = V active cubes; vertices, normals
 * [capacity, 3], cube [capacity] int64 (the cube ids, ascending). */
int ced_mesh_vertices(int32_t reso, const float *center_host, float radius, const float *lattice, float thresh,
                      int64_t capacity, float *vertices, float *normals, int64_t *cube, int64_t *count,
                      void *workspace, int64_t workspace_bytes, void *stream);

/* cube [n_vertices]: ALL of ced_mesh_vertices' cube ids for the same lattice and thresh (a face looks its four vertex
 * ids up in it by binary search; an id that is absent gives -1).  *count = active edges (quads); faces [2 * capacity, 3]
 * int32, the two triangles of a quad adjacent. */
int ced_mesh_faces(int32_t reso, const float *lattice, float thresh, const int64_t *cube, int64_t n_vertices,
                   int64_t capacity, int32_t *faces, int64_t *count, void *workspace, int64_t workspace_bytes,
                   void *stream);

/* nerfacc.render_weight_from_density / render_transmittance_from_density with packed_info
 * [n_rays,2] = (start,count) -- call sites cednerf/render.py:52-54,81-87, cednerf/utils.py:274-281.
 * prefix_trans is per sample (NULL = 1); weights/trans/alphas may each be NULL. */
int ced_render_weights(int64_t n_rays, const int64_t *packed_info, const float *t_starts,
                       const float *t_ends, const float *sigmas, const float *prefix_trans,
                       float *weights, float *trans, float *alphas, void *stream);

/* nerfacc.accumulate_along_rays(_): out[ray, :] += sum_i w_i * values[i, :] (values NULL: C must
 * be 1 and the weights are summed) -- cednerf/render.py:158-169, cednerf/utils.py:282-299. */
int ced_accumulate_along_rays(int64_t n_rays, const int64_t *packed_info, const float *weights,
                              const float *values, int32_t n_channels, float *out, void *stream);

/* reduce_along_rays(ray_indices, values, n_rays, weights, reduce) -- cednerf/render.py:8-39 (the training extras of
 * rendering(), render.py:101-124): out [n_rays, C] = scatter_reduce_ of weights * values into zeros, reduce "sum"
 * (mean == 0) or "mean" (mean == 1, with the initial zero counted as an element, torch's include_self default).
 * values [S, C]; weights NULL or [S, weight_channels] with weight_channels 1 (broadcast) or C; ray indices outside
 * [0, n_rays) are ignored; counts_workspace: n_rays int32 of device scratch (mean only).  Float atomics, as in torch:
 * sums of unsorted indices depend on arrival order in the last bits. */
int ced_reduce_along_rays(int64_t n_samples, const int64_t *ray_indices, const float *values, int32_t n_channels,
                          const float *weights, int32_t weight_channels, int64_t n_rays, int32_t mean, float *out,
                          int32_t *counts_workspace, void *stream);

/* nerfacc.render_visibility_from_density inside OccGridEstimator.sampling (cednerf/utils.py:115-125):
 * mask[i] = trans_i >= early_stop_eps && (alpha_thre <= 0 || alpha_i >= alpha_thre). */
int ced_visibility_mask(int64_t n_rays, const int64_t *packed_info, const float *t_starts,
                        const float *t_ends, const float *sigmas, float early_stop_eps, float alpha_thre,
                        uint8_t *mask, void *stream);

/* One pass of cednerf/utils.py:274-299 (render_weight_from_density with
 * prefix_trans = 1 - opacity[ray], then the three accumulate_along_rays_) fused per ray, in place.
 * packed_info [n_rays,2] indexes the sample arrays; rgbs [S,3]. */
int ced_composite_prefix(int64_t n_rays, const int64_t *packed_info, const float *t_starts,
                         const float *t_ends, const float *sigmas, const float *rgbs,
                         float *rgb, float *opacity, float *depth, void *stream);

/* Backward of the training-time compositing: the derivative of the un-normalised
 * (colors, opacities, depths) = accumulate_along_rays(render_weight_from_density(...), {rgbs, 1, t_mid}) of
 * cednerf/render.py:158-169 w.r.t. the per-sample sigmas [S] and rgbs [S,3], given d_color [n_rays,3],
 * d_opacity [n_rays] and d_depth [n_rays] (the last two may be NULL = zero).  Replaces the backward of nerfacc's
 * render_weight_from_density / accumulate_along_rays autograd functions.  d_sigmas doubles as the kernel's scratch (it
 * holds each sample's transmittance between the two sweeps), so it must not alias an input; the weights the backward
 * uses are ced_render_weights' bit for bit, and only the slots [start, start + count) of each ray are written. */
int ced_composite_backward(int64_t n_rays, const int64_t *packed_info, const float *t_starts,
                           const float *t_ends, const float *sigmas, const float *rgbs,
                           const float *d_color, const float *d_opacity, const float *d_depth,
                           float *d_sigmas, float *d_rgbs, void *stream);

/* Distortion loss of the reference's `-d` flag (train_real.py:379-386, cednerf/losses.py:4-11, i.e.
 * torch_efficient_distloss.flatten_eff_distloss).  Per ray, with s_i = t_end - t_start, m_i = (t_start + t_end) / 2:
 *   L_ray = sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i s_i w_i^2,
 *   loss = sum_rays L_ray / n_norm,  n_norm = 1 + the largest ray index that has at least one sample.
 * packed_info [n_rays,2] (start, count), int64; samples grouped by ray and t_starts non-decreasing within a ray.
 * Outputs: ray_loss [n_rays] (L_ray), *loss (device scalar) and *inv_norm (device scalar, 1 / n_norm, 0 when no ray has a
 * sample), so that a backward scales the unscaled gradient by grad_out * inv_norm without reading anything on the host.
 * Deterministic: no float atomics, the per-ray losses summed in a fixed order (fp64).  n_rays == 0 or n_samples == 0:
 * every output zeroed, no kernel launched.  workspace: ced_distortion_workspace_bytes(n_rays, n_samples, density) bytes
 * of device scratch, 8-byte aligned (density = 1 for ced_distortion_loss_density with d_sigmas, else 0).
 * ced_distortion_loss: weights [S] in; grad_weights [S] (may be NULL) = dL_ray/dw, unscaled.
 * ced_distortion_loss_density: sigmas [S] in; the weights are recomputed with the arithmetic of ced_render_weights (same
 * bits, hence the same loss as ced_distortion_loss fed by ced_render_weights); d_sigmas [S] (may be NULL) =
 * dL_ray/dsigma, unscaled, through the weights.  Samples outside every ray are not written. */
int64_t ced_distortion_workspace_bytes(int64_t n_rays, int64_t n_samples, int32_t density);
int ced_distortion_loss(int64_t n_rays, int64_t n_samples, const int64_t *packed_info, const float *weights,
                        const float *t_starts, const float *t_ends, float *ray_loss, float *grad_weights,
                        void *workspace, float *loss, float *inv_norm, void *stream);
int ced_distortion_loss_density(int64_t n_rays, int64_t n_samples, const int64_t *packed_info, const float *sigmas,
                                const float *t_starts, const float *t_ends, float *ray_loss, float *d_sigmas,
                                void *workspace, float *loss, float *inv_norm, void *stream);

/* Image metrics of the reference's evaluation (train_real.py:494-500): single-scale SSIM and MS-SSIM as pytorch_msssim
 * 1.0.0 computes ssim / ms_ssim, and the per-image MSE of the PSNR, over N images of C channels, H x W, fp32 in.
 * x, y: level-0 images read through the element strides x_strides / y_strides [4] = (n, c, h, w) (host arrays; an
 * [H,W,3] frame permuted to [1,3,H,W] is read in place).  win [win_size]: the normalised Gaussian window (host, fp32,
 * win_size odd, <= 15), applied as a separable valid convolution.  Per level: mu, sigma^2 = E[x^2] - mu^2, ...,
 *   cs = (2 sigma_xy + C2) / (sigma_x^2 + sigma_y^2 + C2),  ssim = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1) * cs,
 * C1 = (k1 data_range)^2, C2 = (k2 data_range)^2, each map averaged over the valid region per (image, channel); between
 * levels both images go through avg_pool2d(2, stride 2, padding (H%2, W%2)) with count_include_pad.
 * levels: 1..5 pyramid levels; 0 = the MSE alone (any size; per_image, mean, level_means must be NULL, mse required).
 * weights [levels] (host, fp32): NULL = single-scale SSIM (levels must be 1), the mean of the ssim map, relu'd when
 * nonnegative != 0; else MS-SSIM = prod_{l<levels-1} relu(cs_l)^w_l * relu(ssim_last)^w_last.  Every level must be at
 * least win_size on each side (pytorch_msssim's stricter min side > (win_size - 1) * 16 is the caller's check).
 * Outputs (device): per_image [N] fp32 (the mean over the channels), mean (may be NULL) the mean over the images,
 * mse [N] fp64 (may be NULL) = sum (x - y)^2 / (C H W) of level 0, level_means [levels][N][C][2] fp64 (may be NULL) =
 * the means of the cs and ssim maps of every level before any relu.
 * Precision: the filtered moments and the pooled levels are fp64 (no cancellation of E[x^2] against mu^2 beside C2).
 * Deterministic: fp64 partials summed in a fixed order, no float atomics; image i's results do not depend on the other
 * images of the batch.  workspace: ced_ssim_workspace_bytes(n, c, h, w, win_size, levels) bytes, 8-byte aligned.  No
 * host synchronisation, no allocation; levels + 2 launches on the stream (2 for the MSE alone). */
int64_t ced_ssim_workspace_bytes(int64_t n, int64_t c, int64_t h, int64_t w, int32_t win_size, int32_t levels);
int ced_ssim(int64_t n, int64_t c, int64_t h, int64_t w, const float *x, const int64_t *x_strides, const float *y,
             const int64_t *y_strides, double data_range, double k1, double k2, int32_t win_size, const float *win,
             int32_t levels, const float *weights, int32_t nonnegative, float *per_image, float *mean, double *mse,
             double *level_means, void *workspace, void *stream);

/* Weight gradient of a bias-free dense layer over the sample stream:
 *   dw[o][i] = sum_s dy[s][o] * x[s][i],   x [n, n_in], dy [n, n_out], dw [n_out, n_in], widths 1..64, all fp32,
 * x and dy contiguous and 16-byte aligned.  Replaces the weight-gradient GEMM of tiny-cuda-nn's Network backward
 * (modules of cednerf/model.py:200-222,280-309 under loss.backward(), train_real.py:414-419).  fp32 MFMA
 * accumulation, two deterministic stages (per-workgroup partial tiles in `workspace`, then a fixed-order sum):
 * reproducible run to run.  ced_weight_grad_workspace_bytes gives the scratch size for n samples. */
/* The 8-bit frames of the reference's video step, on the device:
 * ced_frame_to_rgb8: out[y][x'][c] = uint8(rgb[y][x][c] * 255), x' = width-1-x when flip_w
 *   (np.flip(rgb * 255, axis=1).astype(np.uint8), train_real.py:556); rgb [H,W,3] f32, out [H,W,3] u8.
 * ced_depth_to_u8: out = uint8((depth - min) / (max - min) * 255) over the image (depth2img before the colour-map
 *   lookup, train_real.py:38-41), same flip; depth [H,W] f32, out [H,W] u8, workspace = 8 bytes of device memory. */
int ced_frame_to_rgb8(int32_t height, int32_t width, const float *rgb, int32_t flip_w, uint8_t *out, void *stream);
int ced_depth_to_u8(int32_t height, int32_t width, const float *depth, int32_t flip_w, uint8_t *out,
                    void *workspace, void *stream);

/* A flow image as colour, on the device: flow [H,W,2] f32 (x, y components), max_mag > 0, out [H,W,3] u8, the flip of
 * ced_frame_to_rgb8.  The HSV wheel in closed form, every line in fp32, no fused multiply-add:
 *     h = atan2f(fy, fx) * fp32(1 / (2 pi));  if h < 0: h = h + 1;  if h >= 1: h = 0              -- hue in [0, 1)
 *     s = fminf(sqrtf(fx * fx + fy * fy) / max_mag, 1)                                            -- saturation; value = 1
 *     for (channel, n) in (R, 5), (G, 3), (B, 1):
 *         k = n + h * 6;  if k >= 6: k = k - 6
 *         channel = 1 - s * fmaxf(fminf(fminf(k, 4 - k), 1), 0)
 *     out = uint8(channel * 255)                          -- ced_frame_to_rgb8's conversion: clamped, truncated toward zero
 * so no flow is white, flow along +x pure red, +y (down the image) yellow-green, -x cyan, and a magnitude of max_mag or
 * more is fully saturated.  A pixel either of whose components is not finite is black (0, 0, 0). */
int ced_flow_to_rgb8(int32_t height, int32_t width, const float *flow, float max_mag, int32_t flip_w, uint8_t *out,
                     void *stream);

/* The exchange's consumer ("a local un-permute fused into the consumer"): rendered pixels arrive in marching
 * order (8x8-tile order; with several GPUs every rank's shard of it, all-gathered as [rows, 5] = rgb, opacity, depth);
 * row i goes to raster pixel dest[i] (rows with dest outside [0, n_pixels) are padding).  One pass writes the raster
 * rgb [n_pixels,3] / opacity [n_pixels] / depth [n_pixels] (each may be NULL) and, when rgb8 != NULL, the 8-bit
 * colour frame of ced_frame_to_rgb8 directly ([n_pixels,3] uint8, flipped inside rows of `width` pixels when flip_w).
 * Sources are given with their row strides in floats (5, 5, 5 for the gathered payload; 3, 1, 1 for separate arrays). */
int ced_scatter_pixels(int64_t n_rows, const float *src_rgb, int32_t stride_rgb, const float *src_opacity,
                       int32_t stride_opacity, const float *src_depth, int32_t stride_depth, const int64_t *dest,
                       int64_t n_pixels, float *rgb, float *opacity, float *depth, uint8_t *rgb8, int32_t width,
                       int32_t flip_w, void *stream);

/* Bias-free dense layer over the sample stream, hand-written (csrc/linear.hip) in place of a library GEMM -- the
 * forward and the input gradient of the tiny-cuda-nn Networks the reference trains through (cednerf/model.py:200-222,
 * 280-344; loss.backward(), train_real.py:412-420):
 *   transpose_w == 0:  y[s][o] = sum_i x[s][i] * w[o][i]     w [n_out, n_in]   (forward; relu != 0: y = max(y, 0))
 *   transpose_w != 0:  y[s][o] = sum_i x[s][i] * w[i][o]     w [n_in, n_out]   (input gradient dz W of a layer W)
 * then, when mask != NULL ([n, n_out]):  y[s][o] = mask[s][o] > 0 ? y[s][o] : 0  (the ReLU derivative of the layer
 * below, fused).  x [n, n_in], y [n, n_out], widths 1..64, fp32 MFMA with fp32 accumulation.  w_rows / w_cols are
 * checked against n_in / n_out.  The weight gradient of the same layer is ced_weight_grad. */
int ced_linear(int64_t n, const float *x, int32_t n_in, const float *w, int32_t w_rows, int32_t w_cols,
               int32_t transpose_w, int32_t n_out, int32_t relu, const float *mask, float *y, void *stream);

int64_t ced_weight_grad_workspace_bytes(int64_t n, int32_t n_out, int32_t n_in);
int ced_weight_grad(int64_t n, const float *x, int32_t n_in, const float *dy, int32_t n_out, float *dw,
                    void *workspace, int64_t workspace_bytes, void *stream);

/* ced_composite_prefix plus the per-iteration bookkeeping of cednerf/utils.py:301-307 in the same
 * launch: ray_mask[r] = opacity[r] <= opc_thres && count[r] == n_samples_iter, and
 * stats[0] += number of rays still alive, stats[1] += samples composited (device int64[2], the
 * caller zeroes it).  Lets the host loop read both numbers with a single 16-byte copy. */
int ced_composite_step(int64_t n_rays, const int64_t *packed_info, const float *t_starts,
                       const float *t_ends, const float *sigmas, const float *rgbs,
                       float *rgb, float *opacity, float *depth,
                       float opc_thres, int32_t n_samples_iter, uint8_t *ray_mask, int64_t *stats,
                       void *stream);

/* composite_test -- cednerf/taichi_kernel/volume_render_test.py:4-59 (same arguments, same
 * in-place semantics; alive_indices entries are set to -1 when a ray finishes).  The four sample arrays may be NULL
 * when no entry has a step (an empty sample set): every entry then only becomes -1. */
int ced_composite_test(int64_t n_alive, const float *sigmas, const float *rgbs, const float *t_start,
                       const float *t_end, const int64_t *pack_info, int64_t *alive_indices,
                       float T_threshold, float alpha_threshold,
                       float *opacity, float *depth, float *rgb, void *stream);

/* Tail of render_image_test / rendering (cednerf/utils.py:310-311, cednerf/render.py:170-174):
 * rgb += bkgd * (1 - opacity); depth /= max(opacity, FLT_EPSILON).  bkgd: device [3] or NULL. */
int ced_finalize_pixels(int64_t n_rays, const float *bkgd, float *rgb, const float *opacity,
                        float *depth, void *stream);

/* ---- occupancy-grid maintenance (nerfacc OccGridEstimator._update as driven at
 * train_real.py:324-336).  The density query in between is ced_field_forward with directions == NULL. ---- */

/* World positions of jittered cell samples: cell index c = (ix*res + iy)*res + iz of one grid level,
 * x = aabb_min + ((ix,iy,iz) + noise) / res * (aabb_max - aabb_min).  aabb_host: HOST float[6] of that
 * level; noise [n,3] in [0,1); positions [n,3] out. */
int ced_occ_cell_points(int64_t n, const int64_t *cell_indices, const float *noise, int32_t res,
                        const float *aabb_host, float *positions, void *stream);

/* The EMA write-back of _update, for any cell_ids (the sampled draw lists cells several times): every listed cell c
 * becomes  fmax(occs[c] * ema_decay, max over i with cell_ids[i] == c of density[i] * step_size)  -- it decays once and
 * takes the largest of its samples, whatever the order of the list; a NaN sample contributes nothing (fmaxf), unlisted
 * cells keep their bits.  Of the outcomes the index assignment it replaces can have with duplicates, this is the one
 * that does not depend on the order of the writers, so a call is reproducible.  cell_ids must lie inside occs.
 * workspace: n floats of device memory (workspace_bytes >= 4 * n), overwritten. */
int ced_occ_ema_update(int64_t n, const int64_t *cell_ids, const float *density, float step_size,
                       float ema_decay, float *occs, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- on-device ray generation: full-frame rays from camera parameters, so no
 * [H,W,3] x 2 upload per frame.  Outputs [height*width, 3] row-major (pixel x fastest), i.e. Rays of
 * shape [H,W,3]. ---- */

/* Pinhole camera of datasets/dnerf_synthetic.py:191-221 / gui.py:43-86: pixel (x,y) ->
 * [(x-cx+.5)/fx, (y-cy+.5)/fy * s, s] (s = -1 OpenGL, +1 OpenCV) rotated by c2w[:3,:3]; origins = c2w[:3,3];
 * viewdirs = normalised directions.  c2w_host: HOST float[12] ([3][4] row-major); directions may be NULL. */
int ced_generate_rays_pinhole(int32_t width, int32_t height, float fx, float fy, float cx, float cy,
                              const float *c2w_host, int32_t opengl, float *origins, float *viewdirs,
                              float *directions, void *stream);

/* HyperNeRF camera, datasets/hyper_cam.py:210-252 on get_pixel_centers() (:299-303), as used at
 * datasets/hypernerf.py:172-176: skew / aspect / principal point, radial (k1,k2,k3) + tangential (p1,p2)
 * undistortion by 10 Newton steps (:22-91), rotation by orientation^T.  orientation_host float[9]
 * (row-major), position_host float[3], radial3_host / tangential2_host HOST arrays (NULL = none). */
int ced_generate_rays_hypercam(int32_t width, int32_t height, const float *orientation_host,
                               const float *position_host, float focal_length, float principal_x, float principal_y,
                               float skew, float pixel_aspect_ratio, const float *radial3_host,
                               const float *tangential2_host, float *origins, float *viewdirs, void *stream);

/* Training batch in one launch: replaces the per-step fetch_data + preprocess of datasets/dnerf_synthetic.py:142-242
 * (D-NeRF, a view per ray, RGBA composited on the batch's background) and datasets/hypernerf.py:443-541 (HyperNeRF,
 * one view per batch, RGB, rays at the pixel centre).  Views are device-resident:
 *   images          uint8 [n_views, height, width, channels], channels 4 (RGBA) or 3 (RGB);
 *   cameras         float [n_views, CED_PINHOLE_FLOATS] or [n_views, CED_HYPERCAM_FLOATS] (layouts below);
 *   view_timestamps float [n_views].
 * Every ray r draws (view, x, y) uniformly (view_mode CED_VIEW_PER_RAY), or the batch draws one view
 * (CED_VIEW_PER_STEP); its ray is the full-frame kernels' ray of that pixel, bit for bit (pinhole: pixel (x, y) as in
 * ced_generate_rays_pinhole; hypercam: centre (x + .5, y + .5) as in ced_generate_rays_hypercam).  Pixels: RGBA
 * rgb / 255 * (a / 255) + bkgd * (1 - a / 255), RGB u8 / 255.  Background: white, black or one random colour per batch.
 * The random numbers are a pure function of (seed, step, ray, draw) (train_batch.hip, DESIGN.md "Training batches").
 * Writes origins [n,3], viewdirs [n,3], pixels [n,3], timestamps [n] (the view's), color_bkgd [3] and, if `indices` is
 * not NULL, the drawn (view, x, y) as int32 [n,3].  One launch, no host synchronisation. */
#define CED_CAMERA_PINHOLE 0
#define CED_CAMERA_HYPERCAM 1
#define CED_PINHOLE_FLOATS 17    /* fx, fy, cx, cy, c2w[3][4] row-major, sign (-1 OpenGL, +1 OpenCV) */
#define CED_HYPERCAM_FLOATS 22   /* orientation[3][3] row-major, position[3], focal, principal x, principal y, skew,
                                    pixel aspect ratio, k1, k2, k3, p1, p2 */
#define CED_VIEW_PER_RAY 0
#define CED_VIEW_PER_STEP 1
#define CED_BKGD_WHITE 0
#define CED_BKGD_BLACK 1
#define CED_BKGD_RANDOM 2
int ced_sample_training_batch(int32_t camera_model, int32_t n_views, int32_t width, int32_t height, int32_t channels,
                              const uint8_t *images, const float *cameras, const float *view_timestamps,
                              int64_t num_rays, uint64_t seed, int64_t step, int32_t view_mode, int32_t bkgd_mode,
                              float *origins, float *viewdirs, float *pixels, float *timestamps, float *color_bkgd,
                              int32_t *indices, void *stream);

/* Importance-sampled training batch (datasets/dnerf_3d_video_IS.py:401-440): num_cells cells of a weight map drawn
 * without replacement, as torch.multinomial draws them (weight / Exp(1) variate, the num_cells largest), each cell
 * expanded to its s x s pixels, s = weights_subsampled.
 *   weights  float [n_views * (height / s) * (width / s)] (device), non-negative, any positive scale; cell index
 *            (view * (height / s) + ysub) * (width / s) + xsub.  n_cells = that count, below 2^31.
 *   Candidates: all n_cells cells (candidate j = cell j) when n_cells <= pool_size, else pool_size cells drawn uniformly
 *            with replacement, c_j = (draw(j, 3) * n_cells) >> 32 (the draws of ced_sample_training_batch).
 *   Key:     u = draw(j, 4), unit = ((u >> 9) * 2 + 1) * 2^-24, e = -det_logf(unit) (ced_common.hpp: every operation one
 *            float32 rounding), key_j = weights[c_j] / e; a weight that is not a positive finite number gives key 0.
 *   Select:  the num_cells largest keys as unsigned bit patterns, equal keys to the lower j; the selected candidates in
 *            ascending j are i = 0 .. num_cells - 1.
 *   Rays:    ray (ah * s + aw) * num_cells + i is pixel (xsub * s + aw, ysub * s + ah) of the cell's view; its ray,
 *            colour (u8 / 255; channels must be 3), timestamp and the batch's background as ced_sample_training_batch.
 * Writes num_cells * s * s rays to origins, viewdirs, pixels [n,3], timestamps [n], color_bkgd [3] and, if not NULL,
 * indices int32 [n,3] = (view, x, y), and to min_key (device, one uint32) the bit pattern of the smallest selected key:
 * 0 means that fewer than num_cells candidates had a positive key and the batch is not a valid draw (the caller's check;
 * every write stays in bounds).  workspace: ced_importance_batch_workspace_bytes(n_cells, pool_size, num_cells) bytes of
 * device scratch (-1 for sizes the sampler rejects), 16-byte aligned, contents unspecified.  Ten launches and a memset on
 * the stream, no host synchronisation, no state kept between calls. */
int64_t ced_importance_batch_workspace_bytes(int64_t n_cells, int64_t pool_size, int64_t num_cells);
int ced_sample_importance_batch(int32_t camera_model, int32_t n_views, int32_t width, int32_t height, int32_t channels,
                                const uint8_t *images, const float *cameras, const float *view_timestamps,
                                const float *weights, int32_t weights_subsampled, int64_t pool_size, int64_t num_cells,
                                uint64_t seed, int64_t step, int32_t bkgd_mode, float *origins, float *viewdirs,
                                float *pixels, float *timestamps, float *color_bkgd, int32_t *indices, uint32_t *min_key,
                                void *workspace, int64_t workspace_bytes, void *stream);

/* DyNeRF's sampling-weight maps (datasets/dnerf_3d_video_IS.py:13-76, 187) from device-resident uint8 images
 * [n_cameras, n_frames, height, width, 3], camera-major.  One launch each, no workspace, no host synchronisation.
 * ced_temporal_median_u8: median uint8 [n_cameras, height, width, 3], per camera, pixel and channel the median over the
 *   frames with torch.median's rule (the lower middle value for an even count).
 * ced_isg_weights: weights float [n_cameras, n_frames, height, width] = dynerf_isg_weight in its order of roundings:
 *   a = u8 / 255, m = median / 255, d = a - m, q = d * d, p = q / (q + gamma * gamma), (p0 + p1 + p2) * (1/3 in float).
 * ced_ist_weights: dynerf_ist_weight_nice: per channel max over s = 1 .. frame_shift of |f[t + s] - f[t]| and
 *   |f[t - s] - f[t]| on the 0 .. 255 values, a neighbour outside the clip being zero; (m0 + m1 + m2) / 3; max(., alpha). */
int ced_temporal_median_u8(int32_t n_cameras, int32_t n_frames, int32_t height, int32_t width, const uint8_t *images,
                           uint8_t *median, void *stream);
int ced_isg_weights(int32_t n_cameras, int32_t n_frames, int32_t height, int32_t width, const uint8_t *images,
                    const uint8_t *median, float gamma, float *weights, void *stream);
int ced_ist_weights(int32_t n_cameras, int32_t n_frames, int32_t height, int32_t width, const uint8_t *images,
                    float alpha, int32_t frame_shift, float *weights, void *stream);

/* Optional per-iteration trace of ced_render_image_test (host struct, host arrays of `capacity`
 * entries, each may be NULL).  field_begin/field_end are caller-created hipEvent_t handles that the
 * renderer records on `stream` around the field-kernel launch of iteration i, so a benchmark can
 * time that kernel live without perturbing the launch sequence.  Events of iterations >= n_iters may have been
 * recorded around empty launches (the host enqueues ahead of the device-side schedule). */
typedef struct ced_frame_trace {
    int32_t capacity;        /* in  */
    int32_t n_iters;         /* out: iterations executed */
    void **field_begin;      /* in  */
    void **field_end;        /* in  */
    int64_t *iter_alive;     /* out: rays alive entering iteration i (N_alive, cednerf/utils.py:231) */
    int64_t *iter_n_samples; /* out: samples per ray requested in iteration i (N_samples, utils.py:235) */
    int64_t *iter_samples;   /* out: samples marched and composited in iteration i */
    uint64_t *field_stamps;  /* in: DEVICE memory [2 * capacity] or NULL.  Out (device): for iteration i the ticks
                                {first workgroup of the field launch started, its last workgroup finished} on the
                                device's constant wall clock (ced_wall_clock_khz ticks per ms): the interval the kernel
                                was EXECUTING, where the event pair also counts its wait for free CUs */
} ced_frame_trace;

/* Rate of the device wall clock the field_stamps are taken on (hipDeviceAttributeWallClockRate), in kHz; < 0 on error. */
int64_t ced_wall_clock_khz(void);

/* Device bytes ced_render_image_test needs in `workspace` (negative on bad arguments).  Besides the per-ray marching
 * state and the per-sample arrays of one iteration this holds 3 floats per ray (each array rounded up to 256 bytes): the
 * colour head's direction inputs, computed once per ray in the call's set-up launch and read by the field kernel.  The
 * same holds for the workspaces of ced_render_frames_test(_sharded) and ced_render_image below: always ask the entry. */
int64_t ced_render_image_test_workspace_bytes(int64_t n_rays, int32_t n_grids, int32_t res, float cone_angle,
                                              int32_t max_samples);

/* render_image_test(max_samples, radiance_field, estimator, rays, near_plane, far_plane,
 * render_step_size, render_bkgd, cone_angle, alpha_thre, early_stop_eps, timestamps)
 * -- cednerf/utils.py:153-318, the eval / GUI frame renderer (callers train_real.py:481-493,
 * :541-553, gui.py:215-228), as ONE call: ray/AABB setup, then per iteration one marching launch,
 * one fused field launch, one compositing launch and a one-wave scheduling launch that computes the next
 * iteration's N_samples = clamp(N_rays // N_alive, min, 64) ON THE DEVICE, and the background / depth
 * normalisation at the end.  Same schedule and per-ray sample sets as the reference loop; unlike it
 * (utils.py:231: one device->host sync per iteration) the host never waits for an iteration: it enqueues up to
 * one iteration beyond the last one whose plan it has seen published in `host_stats`.
 * `alpha_thre` is not a parameter because the reference ignores it in this function.
 *   rays_o, rays_d [n_rays,3]; binaries [n_grids,res,res,res] bytes; aabbs [n_grids,6];
 *   accel: device, from ced_build_occupancy_accel for these binaries, or NULL (built inside the call);
 *   timestamps: device [1] (t_per_ray = 0, eval) or [n_rays] (t_per_ray = 1); bkgd: device [3] or NULL;
 *   outputs rgb [n_rays,3], opacity [n_rays], depth [n_rays] (overwritten);
 *   workspace: device scratch of ced_render_image_test_workspace_bytes() bytes;
 *   host_stats: PINNED host memory, >= 2048 bytes, private to this call while it runs (the scheduling launches
 *   publish {rays alive, done, sequence number} there; the call's table of lattice points travels through it);
 *   total_samples_out: host, receives the number of field evaluations (utils.py:307,317).
 *   field_stream: NULL, or a second stream on which the field kernel is launched (event-ordered with `stream`).
 * The call returns when the frame is complete (it ends with one stream synchronise to read the sample count and
 * the per-iteration record back). */
int ced_render_image_test(const ced_field_desc *field, int64_t n_rays, const float *rays_o, const float *rays_d,
                          const uint8_t *binaries, int32_t n_grids, int32_t res, const float *aabbs, const void *accel,
                          float near_plane, float far_plane, float render_step_size, float cone_angle,
                          float early_stop_eps, int32_t max_samples,
                          const float *timestamps, int32_t t_per_ray, const float *bkgd,
                          float *rgb, float *opacity, float *depth,
                          void *workspace, int64_t workspace_bytes, int64_t *host_stats,
                          int64_t *total_samples_out, ced_frame_trace *trace, void *field_stream, void *stream);

/* Several frames of a video in ONE call: the reference renders them one after another with
 * render_image_test (train_real.py:531-558); here `n_frames` (1..64) frames of `rays_per_frame` rays each share the
 * launches of an iteration -- one marching, one field and one compositing launch cover the alive rays of all the
 * frames -- while EVERY FRAME KEEPS ITS OWN reference loop: N_samples = clamp(N_rays // N_alive, min, 64) on its own
 * counts, its own `iteration < max_samples` end.  Each frame's pixels and sample count are therefore exactly those of
 * ced_render_image_test on that frame alone; what changes is that the launches are n_frames times larger.
 *   rays_o, rays_d [n_frames * rays_per_frame, 3] (frame-major); frame_times: device [n_frames], one time per frame;
 *   outputs rgb [n_frames * rays_per_frame, 3], opacity, depth; workspace of
 *   ced_render_frames_test_workspace_bytes() bytes; total_samples_out: host [n_frames].
 *   Everything else as ced_render_image_test. */
int64_t ced_render_frames_test_workspace_bytes(int32_t n_frames, int64_t rays_per_frame, int32_t n_grids, int32_t res,
                                               float cone_angle, int32_t max_samples);
int ced_render_frames_test(const ced_field_desc *field, int32_t n_frames, int64_t rays_per_frame,
                           const float *rays_o, const float *rays_d, const uint8_t *binaries, int32_t n_grids,
                           int32_t res, const float *aabbs, const void *accel, float near_plane, float far_plane,
                           float render_step_size, float cone_angle, float early_stop_eps, int32_t max_samples,
                           const float *frame_times, const float *bkgd, float *rgb, float *opacity, float *depth,
                           void *workspace, int64_t workspace_bytes, int64_t *host_stats,
                           int64_t *total_samples_out, ced_frame_trace *trace, void *field_stream, void *stream);

/* ---- frames whose rays are sharded over several processes (one process per GPU) ----
 * The loop of render_image_test is ONE loop per image: N_samples = clamp(N_rays // N_alive, min, 64)
 * (cednerf/utils.py:231-235) counts the rays of the whole image, and a ray stays alive on `packed_info[:, 1] ==
 * N_samples` (utils.py:301-306).  When frame f's rays are dealt over several processes, every process must therefore
 * run the IMAGE's schedule, not one of its own shard: per iteration the processes exchange, per frame, the number of
 * their rays that survived (one int64 per frame), and the scheduling launch computes N_samples, the last-iteration
 * flag and the end of the loop from the sums.  Each ray then receives exactly the samples, termination planes and
 * pixel values it receives when a single process renders the whole image (bit for bit), whatever the sharding.
 *
 * The exchange is the caller's (the library links no communication library): `reduce` is called by the rendering
 * thread once per enqueued iteration, between that iteration's compositing launch and its scheduling launch, and must
 * ENQUEUE on `stream` an in-place sum over the processes of counts[0 .. n_counts) (device memory, int64; e.g.
 * ncclAllReduce / torch.distributed.all_reduce on that stream) and return 0, or non-zero to abort the call.  It must
 * not block on the device.  Every process makes the same number of calls in the same order: the host loop ends on the
 * plan of a fixed earlier iteration (one iteration behind), which is identical on all processes, never on
 * timing.  No kernel of this library waits for another process.
 *   global_rays_per_frame: N_rays of the whole image; local_rays: DEVICE int32 [n_frames] or NULL -- how many of the
 *   frame's `rays_per_frame` local slots hold real rays (shards are padded to a common size; padding is never alive);
 *   counts: DEVICE int64 [(iterations + 1) * n_frames] scratch, iterations = ced_render_frames_test_iterations();
 *   host_stats must then hold ced_render_frames_test_host_bytes() bytes of pinned memory. */
typedef int (*ced_exchange_fn)(void *user, int64_t *counts, int32_t n_counts, int32_t iteration, void *stream);
typedef struct ced_shard_exchange {
    int64_t global_rays_per_frame;
    const int32_t *local_rays;
    int64_t *counts;
    ced_exchange_fn reduce;
    void *user;
} ced_shard_exchange;
/* device bytes of `workspace` for a sharded call: a share's rays may hold any part of the image's alive rays, so its
 * sample arrays are sized for min(rays_per_frame * 64, global_rays_per_frame) samples per frame and iteration */
int64_t ced_render_frames_test_sharded_workspace_bytes(int32_t n_frames, int64_t rays_per_frame,
                                                       int64_t global_rays_per_frame, int32_t n_grids, int32_t res,
                                                       float cone_angle, int32_t max_samples);
/* most iterations the loop can take (each uses at least min_samples of the max_samples budget) */
int32_t ced_render_frames_test_iterations(float cone_angle, int32_t max_samples);
/* pinned bytes `host_stats` needs for a sharded call (per-iteration publication records) */
int64_t ced_render_frames_test_host_bytes(float cone_angle, int32_t max_samples);
/* ced_render_frames_test with `exchange` (NULL: identical to ced_render_frames_test). */
int ced_render_frames_test_sharded(const ced_field_desc *field, int32_t n_frames, int64_t rays_per_frame,
                                   const float *rays_o, const float *rays_d, const uint8_t *binaries, int32_t n_grids,
                                   int32_t res, const float *aabbs, const void *accel, float near_plane, float far_plane,
                                   float render_step_size, float cone_angle, float early_stop_eps, int32_t max_samples,
                                   const float *frame_times, const float *bkgd, float *rgb, float *opacity, float *depth,
                                   void *workspace, int64_t workspace_bytes, int64_t *host_stats,
                                   int64_t *total_samples_out, ced_frame_trace *trace, void *field_stream, void *stream,
                                   const ced_shard_exchange *exchange);

/* ---- render_image in eval mode: cednerf/utils.py:46-150 (`estimator.sampling` with sigma_fn, then `rendering`) ----
 * The reference evaluates the density of EVERY marched sample (nerfacc OccGridEstimator.sampling ->
 * render_visibility_from_density, call site cednerf/utils.py:115-125) and then the whole field again on the survivors
 * (cednerf/render.py:81-87).  This entry returns the same arrays, bit for bit, from ONE field evaluation per sample:
 * each ray's samples are walked front to back in chunks and a ray stops at the first sample whose transmittance so
 * far is below early_stop_eps (the kept samples of a ray are a prefix of its march, so the rest can never be kept).
 * Inputs: the one-shot march of all rays -- packed_info [n_rays, 2] (first sample, count), t_starts / t_ends [n_all],
 * as ced_traverse_grids produces them (samples sorted by ray).  timestamps as in ced_field_forward_rays.
 * Outputs per ray: rgb [n_rays, 3], opacity, depth (finalised as cednerf/render.py:158-176: background blend, depth /
 * max(opacity, eps)), kept [n_rays] = kept samples of the ray.  stats_out (host int64 [3]): [0] samples evaluated
 * (entries of the workspace's sample arrays), [1] iterations, [2] kept samples (= sum of `kept`).  host_stats: PINNED host memory, >= 64 bytes (the
 * iteration schedule is computed on the device and published there, as in ced_render_image_test).  The call returns
 * after one stream synchronisation (the sample total is needed to size the outputs of the gather).
 * ced_render_image_gather then writes the per-sample `extras` of the kept samples in the reference's order (by ray,
 * then along the ray): ray_offsets [n_rays] = exclusive prefix sum of `kept` (int64), outputs of sum(kept) entries;
 * chunk_rays > 0 makes ray_indices relative to the ray's chunk of that many rays (the reference's chunked eval loop,
 * cednerf/utils.py:108-133), 0 keeps them absolute.
 * Sampling only (rgb == opacity == depth == NULL; the training step's `estimator.sampling(sigma_fn=...)`,
 * train_real.py:339-350, per-ray timestamps): the field kernel evaluates the density alone and no pixel sums are formed;
 * the gather then takes sigmas optional and rgbs == weights == trans == alphas == NULL and returns the surviving
 * (ray_indices, t_starts, t_ends) of nerfacc's sampling, bit for bit. */
int64_t ced_render_image_workspace_bytes(int64_t n_rays, int64_t n_all);
int ced_render_image(const ced_field_desc *field, int64_t n_rays, const float *rays_o, const float *rays_d,
                     int64_t n_all, const int64_t *packed_info, const float *t_starts, const float *t_ends,
                     float early_stop_eps, float alpha_thre, const float *timestamps, int32_t t_per_ray,
                     const float *bkgd, float *rgb, float *opacity, float *depth, int32_t *kept, void *workspace,
                     int64_t workspace_bytes, int64_t *host_stats, int64_t *stats_out, void *field_stream, void *stream);
int ced_render_image_gather(int64_t n_rays, int64_t n_all, int64_t processed, const void *workspace,
                            int64_t workspace_bytes, const int64_t *ray_offsets, int64_t chunk_rays,
                            int64_t *ray_indices, float *t_starts, float *t_ends, float *sigmas, float *rgbs,
                            float *weights, float *trans, float *alphas, void *stream);

/* One-shot march of every ray to the far plane on the accelerated walk of the frame renderer: the samples of
 * nerfacc.traverse_grids without a step limit (the marching half of OccGridEstimator.sampling, call sites
 * cednerf/utils.py:115-125, train_real.py:339-350), bit for bit, faster than ced_traverse_grids through empty space.
 * accel: ced_build_occupancy_accel's structure.  t_sorted [n_rays, 2 n_grids], t_indices (int64), hits [n_rays, n_grids]:
 * the sorted ray / box events of cednerf/utils.py:215-225 (ced_ray_aabb_intersect + stable sort); NULL for one level.
 * fill = 0: packed_info[r][1] = samples of ray r.  The caller scans the counts into packed_info[r][0].
 * fill = 1: writes t_starts / t_ends (and ray_indices, optional) of ray r from packed_info[r][0] on.
 * fill = 2: ONE pass for callers that can bound the total: `total` (device int64, zero on entry) counts the samples,
 *   every ray gets a range [packed_info[r][0], + packed_info[r][1]) of t_starts / t_ends [capacity] in workgroup
 *   arrival order (NOT sorted by ray; ray_indices unused) and stores its samples there if the range ends within
 *   `capacity`; *total > capacity afterwards means some rays stored nothing (redo with the two-pass form).
 *   ced_render_image accepts such a march (it treats a range beyond n_all as empty and never reads past the arrays). */
int ced_march_all(int64_t n_rays, const float *rays_o, const float *rays_d, const uint8_t *binaries, int32_t n_grids,
                  int32_t res, const float *aabbs, const void *accel, const float *near_planes, float far_plane,
                  float render_step_size, float cone_angle, const float *t_sorted, const int64_t *t_indices,
                  const uint8_t *hits, int32_t fill, int64_t *packed_info, float *t_starts, float *t_ends,
                  int64_t *ray_indices, int64_t capacity, int64_t *total, void *stream);

/* A whole bias-free ReLU MLP (widths <= 64, <= 6 layers) in one launch per direction: the fused forward / backward of
 * the tiny-cuda-nn FullyFusedMLP networks the reference trains through (cednerf/model.py:200-222,280-344 under
 * train_real.py:339-420).  Same per-output MFMA order as ced_linear: the results are those of the layer-by-layer calls.
 * widths (host) [n_layers + 1]: input width, then each layer's output width; weights (host array of device pointers):
 * W_l [widths[l+1], widths[l]] row-major.
 * backward = 0: x [n, widths[0]]; outs[l] (device, [n, widths[l+1]]) receives layer l's output -- ReLU applied on all but
 *   the last layer (on the last too with relu_last); masks unused.
 * backward = 1: x = dy [n, widths[n_layers]]; going down from the last layer, outs[l] ([n, widths[l]], may be NULL)
 *   receives the gradient with respect to layer l's INPUT, multiplied by [masks[l] > 0] where masks[l] (that input, i.e.
 *   the forward's outs[l-1]) is given -- masks[0] is normally NULL (the network input has no ReLU). */
int ced_mlp_chain(int64_t n, int32_t n_layers, int32_t backward, const float *x, const int32_t *widths,
                  const float *const *weights, float *const *outs, const float *const *masks, int32_t relu_last,
                  void *stream);

/* Backward of a whole MLP WITH its weight gradients, one launch (+ a fixed-order reduction): the walk of ced_mlp_chain's
 * backward direction, with dW_l = dz_l^T a_l accumulated at every layer from the registers the walk holds (instead of
 * ced_weight_grad re-reading every dz_l and a_l).  Shapes: input width <= 48, 1..3 hidden layers of width 64, output
 * width <= 32 (n_layers = hidden layers + 1); CED_E_INVALID otherwise (callers fall back to ced_mlp_chain +
 * ced_weight_grad).  widths as ced_mlp_chain; acts (host array of device pointers) [n_layers]: acts[0] = the network
 * input x [n, widths[0]], acts[l] = the forward's (post-ReLU) output of layer l-1 [n, 64]; dy [n, widths[n_layers]].
 * Outputs: dws (device, sum of widths[l] * widths[l+1] floats): dW_0, dW_1, ... back to back, each row-major
 * [widths[l+1], widths[l]]; g0 [n, widths[0]] (gradient w.r.t. x) or NULL.  Deterministic (no float atomics). */
int64_t ced_mlp_backward_dw_workspace_bytes(int64_t n, int32_t n_layers, const int32_t *widths);
int ced_mlp_backward_dw(int64_t n, int32_t n_layers, const float *dy, const int32_t *widths,
                        const float *const *weights, const float *const *acts, float *g0, float *dws, void *workspace,
                        int64_t workspace_bytes, void *stream);

/* Element-wise pieces of the DIFFERENTIABLE field between its MLPs and its hash grid (training path; the statements of
 * cednerf/model.py:354-383,414-417,447-455 as train_real.py:339-420 differentiates them), one launch each.  fp32, device
 * pointers, row-major.
 * ced_train_inputs: per sample the position (rays mode, ray_indices != NULL: rays_o[r] + rays_d[r] * ((t_start + t_end) / 2),
 *   time timestamps[r]; explicit mode: positions / directions / timestamps per sample), enc_out [n, 32] = tcnn
 *   Frequency(4) of (x, y, z, t) ([dim][freq][sin, cos] of pi 2^k v), sh_out [n, 4] = SH degree 2 of the normalised
 *   direction, t_out [n].  Its backward is ced_train_inputs_backward. */
int ced_train_inputs(int64_t n, const float *rays_o, const float *rays_d, const int64_t *ray_indices,
                     const float *t_starts, const float *t_ends, const float *timestamps, const float *positions,
                     const float *directions, float *pos_out, float *enc_out, float *sh_out, float *t_out, void *stream);
/* ced_train_inputs_backward: the gradient of ced_train_inputs at its inputs (a camera pose, a time offset), from the
 *   gradients d_pos [n, 3], d_enc [n, 32], d_sh [n, 4], d_t [n] at its four outputs; each may be NULL (= zero).  The
 *   forward's own inputs are passed again: sin / cos are recomputed as the forward computes them.  Per sample i, with
 *   v_q the q-th of (x, y, z, t), s_k / c_k = sin / cos(pi 2^k v_q):
 *     g_v[q] = ((a_0 + a_1) + a_2) + a_3,  a_k = fl(pi 2^k) * (d_enc[i, 8q + 2k] * c_k - d_enc[i, 8q + 2k + 1] * s_k)
 *     g_pos  = d_pos[i] + g_v[0..2],   g_t = d_t[i] + g_v[3]
 *     g_dir  = (g_w - w * ((w_x g_wx + w_y g_wy) + w_z g_wz)) / |d|,  w = ((d / |d| + 1) / 2) * 2 - 1 as in the forward,
 *              g_w = (-K d_sh[i, 3], -K d_sh[i, 1], K d_sh[i, 2]),  K = 0.48860251190291987
 *   Explicit mode (ray_indices == NULL; n_rays ignored): d_origins [n, 3] = g_pos, d_directions [n, 3] = g_dir,
 *   d_times [n] = g_t.
 *   Rays mode: per ray r the sums over its samples, t_mid = (t_start + t_end) / 2 as the forward rounds it and
 *   t_starts / t_ends constants:  d_origins [n_rays, 3] = sum g_pos,  d_directions [n_rays, 3] = sum (g_pos * t_mid + g_dir),
 *   d_times [n_rays] = sum g_t.  PRECONDITION: ray_indices is non-decreasing (what sampling produces) and packed_info
 *   [n_rays, 2] int64 holds each ray's (first sample, count) -- nerfacc's packed_info of the same ray_indices.  Every
 *   one of the n_rays rows is written (exact zeros for a ray without samples): the caller does not clear the outputs.
 *   A segmented sum in a fixed order, no float atomics: the same bits on every launch.  n_rays < 2^31; d_enc and d_sh
 *   16-byte aligned.  Explicit mode with n == 0 and rays mode with n_rays == 0 return CED_OK without a launch. */
int ced_train_inputs_backward(int64_t n, int64_t n_rays, const float *rays_o, const float *rays_d,
                              const int64_t *ray_indices, const float *t_starts, const float *t_ends,
                              const float *timestamps, const float *positions, const float *directions,
                              const int64_t *packed_info, const float *d_pos, const float *d_enc, const float *d_sh,
                              const float *d_t, float *d_origins, float *d_directions, float *d_times, void *stream);
/* ced_train_warp: move = mo[:, :3] * moving_step (+ tanh(mo[:, 3:6]) * moving_step with use_div_offsets),
 *   xn = clamp((pos + move - aabb_lo) / (aabb_hi - aabb_lo), 0, 1), selector = 1 where the unclamped xn lies strictly
 *   inside (0, 1) on all axes, else 0.  aabb_host: six floats on the HOST.
 * ced_train_warp_backward: d_mo [n, mo_width] from d_xn (passes where 0 <= unclamped xn <= 1, torch.clamp's rule) and
 *   d_move (may be NULL).
 * ced_train_warp_backward_pos: d_pos [n, 3] = d_xn / (aabb_hi - aabb_lo) where 0 <= unclamped xn <= 1 (the same rule),
 *   else 0; `move` does not depend on pos. */
int ced_train_warp(int64_t n, const float *pos, const float *mo, int32_t mo_width, int32_t use_div_offsets,
                   float moving_step, const float *aabb_host, float *xn, float *move, float *selector, void *stream);
int ced_train_warp_backward(int64_t n, const float *pos, const float *mo, int32_t mo_width, int32_t use_div_offsets,
                            float moving_step, const float *aabb_host, const float *d_xn, const float *d_move,
                            float *d_mo, void *stream);
int ced_train_warp_backward_pos(int64_t n, const float *pos, const float *mo, int32_t mo_width, int32_t use_div_offsets,
                                float moving_step, const float *aabb_host, const float *d_xn, float *d_pos, void *stream);
/* ced_train_head_in: sigma = exp(bout[:, 0] - 1) * selector (trunc_exp, cednerf/utils.py:27-43), head_in [n, 19] =
 *   [sh (4), bout[:, 1:16]].  ced_train_head_in_backward: d_bout [n, 16] from d_head_in [n, 19] and d_sigma [n] (either may
 *   be NULL = zero); the density's derivative is exp(min(raw - 1, 15)) as in the reference's _TruncExp.backward. */
int ced_train_head_in(int64_t n, const float *bout, const float *sh, const float *selector, float *head_in,
                      float *sigma, void *stream);
int ced_train_head_in_backward(int64_t n, const float *bout, const float *selector, const float *d_head_in,
                               const float *d_sigma, float *d_bout, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CEDNERF_HIP_H */
