// The derivative of the motion network: ced_field_move_jacobian hands out move(x, t) and its 3 x 4 Jacobian with respect
// to (x, y, z, t) from one launch, and ced_field_move_inverse_newton / ced_field_track_newton solve x + move(x, t) = c by
// Newton's method on that Jacobian, the iterate held in registers (include/cednerf_hip.h states every operation).
// ced_field_velocity / ced_field_velocity_rays turn the same Jacobian into the velocity of the material point that sits at
// x, v = -(I + J_x)^-1 d move / dt, inside the launch: 17 bytes per row leave instead of the Jacobian's 60.
//
// Forward mode: the Jacobian of a sample is four tangent vectors pushed through the four layers beside the primal.  A
// tangent is one more MFMA column, so the tangents of a 16-sample primal tile are four 16-column operand tiles that go
// through the SAME layer functions on the same staged weights (mlp_layer; mlp_layer_h / hidden_fed_layer), in the
// arithmetic the descriptor selects: MFMA columns do not mix, so the primal tile computes ced_field_move's bits whatever
// stands beside it.  The encoding's tangent is built from the primal features the lane already holds (the derivative of
// sin(2^k pi v + phase) is 2^k pi times the other phase of the same frequency, negated for a cosine), a hidden layer's
// tangent is zeroed wherever the PRIMAL pre-activation is not > 0, and the output applies the tanh's derivative
// 1 - th^2 to the fine offsets.
//
// Shape: field_move.hip's (tile_kernel of field_move_device.hpp with the ops JacobianOp, NewtonOp and VelocityOp:
// persistent workgroups of 512 threads, the motion network's layers staged into LDS once), with ONE 16-sample primal tile
// per wave iteration instead of two: primal + four tangents are five operand tiles and five accumulator tiles (80 + 80
// registers on the fp32 chain), which fit the 256 registers of a wave at two waves per SIMD without scratch; two primal
// tiles would not.  VelocityOp reads its rows from that header's SampleSrc, as MoveOp does; the two velocity entries fill it
// through point_samples / ray_samples.
#include "field_jacobian_device.hpp"

namespace ced {

struct JacArgs {
    int64_t n;
    const float *pos, *t;                             // [n,3], [n]
    float *move, *jac;                                // [n,3], [n,12]; either may be null
    float moving_step;
    int use_div;
    const void *weights;
    int64_t lo_halves;
};

// ---- ced_field_move_jacobian ---------------------------------------------------------------------------------------------
// lane group a < 3 stores component a of move and row a of the Jacobian
template <int NP>
__device__ __forceinline__ void jac_store(const JacArgs &A, const float (&mv)[NP][3], const float (&J)[NP][12], int64_t tile_base,
                                          int g, int c)
{
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int64_t s = tile_base + 16 * j + c;
        const bool stores = s < A.n && g < 3;
        // named values first: a select between array elements would become a load at a selected address
        const float m0 = mv[j][0], m1 = mv[j][1], m2 = mv[j][2];
        const float o_move = (g == 0) ? m0 : (g == 1) ? m1 : m2;
        if (stores && A.move) A.move[3 * s + g] = o_move;
#pragma unroll
        for (int b = 0; b < kDirs; ++b) {
            const float j0 = J[j][b], j1 = J[j][4 + b], j2 = J[j][8 + b];
            const float o_jac = (g == 0) ? j0 : (g == 1) ? j1 : j2;
            if (stores && A.jac) A.jac[12 * s + 4 * g + b] = o_jac;
        }
    }
}

struct JacobianOp : TileOp {
    using Args = JacArgs;
    template <typename W, int NP>
    __device__ __forceinline__ static void tile(const JacArgs &A, const Shared &, const typename W::Elem *w, int64_t tile_base, int64_t,
                                                int lane)
    {
        const int g = lane >> 4, c = lane & 15;
        float px[NP][3], tq[NP], mv[NP][3], J[NP][12];
        load_points<NP>(A.pos, A.t, A.n, tile_base, c, px, tq);
        motion_move_jacobian<W, NP>(w, lane, px, RowTime<NP>{ tq }, A.moving_step, A.use_div, mv, J);
        jac_store<NP>(A, mv, J, tile_base, g, c);
    }
};

// ---- the 3 x 3 solve both the Newton step and the velocity take (include/cednerf_hip.h states it) ------------------------
// A = I + J_x, its cofactors Cf (adj = Cf^T), det by the first row, d = adj r / det; every fp32 operation rounded on its own.
__device__ __forceinline__ void adjugate_solve(const float (&J)[12], const float (&r)[3], float &det, float (&d)[3])
{
    float Am[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) Am[a][b] = (a == b) ? __fadd_rn(1.0f, J[4 * a + b]) : J[4 * a + b];
    }
    float Cf[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const int a1 = (a + 1) % 3, a2 = (a + 2) % 3, b1 = (b + 1) % 3, b2 = (b + 2) % 3;
            Cf[a][b] = __fsub_rn(__fmul_rn(Am[a1][b1], Am[a2][b2]), __fmul_rn(Am[a1][b2], Am[a2][b1]));
        }
    }
    det = __fadd_rn(__fadd_rn(__fmul_rn(Am[0][0], Cf[0][0]), __fmul_rn(Am[0][1], Cf[0][1])), __fmul_rn(Am[0][2], Cf[0][2]));
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float num = __fadd_rn(__fadd_rn(__fmul_rn(Cf[0][a], r[0]), __fmul_rn(Cf[1][a], r[1])), __fmul_rn(Cf[2][a], r[2]));
        d[a] = __fdiv_rn(num, det);
    }
}

constexpr float kDetFloor = 9.5367431640625e-07f;     // 2^-20: below it (in magnitude) neither op divides by the determinant

// ---- the warp's inverse by Newton's method (include/cednerf_hip.h states it) ----------------------------------------------
// The rows, their load and their store are the fixed-point kernels' (TrackRows: target, time and iterate of a wave tile
// in registers, every lane group the same copy of column c's rows); `step` holds the residual.  One round on the rows
// still active: r = (x + m) - c, res = max |r_a|, freeze at res <= tol; a row that goes on takes the Newton step
// x <- x - (I + J_x)^-1 r by the adjugate, or the fixed-point step x <- x - r where the determinant is too small or the
// step not finite.  `last`: round max_iters evaluates the residual of the x it was given and moves nothing.  Returns
// whether any row of this lane is still active.
template <int NT>
__device__ __forceinline__ bool newton_update(const float (&mv)[NT][3], const float (&J)[NT][12], float tol, bool last, TrackRows<NT> &R)
{
    bool any = false;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        float r[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) r[a] = __fsub_rn(__fadd_rn(R.px[j][a], mv[j][a]), R.target[j][a]);
        const float res = fmaxf(fmaxf(__builtin_fabsf(r[0]), __builtin_fabsf(r[1])), __builtin_fabsf(r[2]));
        const bool on = R.active[j];                                     // a frozen row keeps what it has
        R.step[j] = on ? res : R.step[j];
        R.evals[j] += on ? 1 : 0;
        R.active[j] = on && !(res <= tol);                               // a NaN residual stays active
        any = any || R.active[j];

        float det, d[3];
        adjugate_solve(J[j], r, det, d);
        bool fine = __builtin_fabsf(det) >= kDetFloor;                   // false for a NaN
#pragma unroll
        for (int a = 0; a < 3; ++a) fine = fine && __builtin_fabsf(d[a]) < __builtin_inff();   // finite: false for an infinity and for a NaN
        const bool go = R.active[j] && !last;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float xn = __fsub_rn(R.px[j][a], fine ? d[a] : r[a]);
            R.px[j][a] = go ? xn : R.px[j][a];
        }
    }
    return any;
}

struct NewtonOp : TileOp {
    using Args = TrackArgs;
    template <typename W, int NT>
    __device__ __forceinline__ static void tile(const TrackArgs &A, const Shared &, const typename W::Elem *w, int64_t tile_base,
                                                int64_t, int lane)
    {
        const int g = lane >> 4, c = lane & 15;
        TrackRows<NT> R;
        track_load<NT>(A, tile_base, c, R);
        const HeldTime<NT> time = hold_time<W, NT>(R.tq, g);
        for (int it = 0; it < A.max_iters; ++it) {
            float mv[NT][3], J[NT][12];
            motion_move_jacobian<W, NT>(opaque(w), lane, R.px, time, A.moving_step, A.use_div, mv, J);
            if (__ballot(newton_update<NT>(mv, J, A.tol, it + 1 == A.max_iters, R)) == 0) break;   // wave-uniform
        }
        track_store<NT>(A, R, tile_base, g, c);
    }
};

// ---- ced_field_velocity, ced_field_velocity_rays: v = -(I + J_x)^-1 d move / dt (include/cednerf_hip.h states it) ----------
struct VelArgs {
    SampleSrc src;
    float *velocity, *det;                            // [n,3], [n]; any may be null
    uint8_t *valid;                                   // [n], may be null
    float moving_step;
    int use_div;
    const void *weights;
    int64_t lo_halves;
};

// The solve with r = the Jacobian's time column.  valid: the determinant at least 2^-20 -- a fold (det <= 0) and a NaN are
// not -- and a finite quotient; a row that is not valid has velocity 0, so that it composites to nothing.  Lane group
// a < 3 stores component a, lane group 3 det and valid.
template <int NP>
__device__ __forceinline__ void velocity_store(const VelArgs &A, const float (&J)[NP][12], int64_t tile_base, int64_t n_eff, int g, int c)
{
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const float r[3] = { J[j][3], J[j][7], J[j][11] };
        float det, d[3];
        adjugate_solve(J[j], r, det, d);
        bool valid = det >= kDetFloor;
#pragma unroll
        for (int a = 0; a < 3; ++a) valid = valid && __builtin_fabsf(d[a]) < __builtin_inff();
        const float v0 = valid ? -d[0] : 0.0f, v1 = valid ? -d[1] : 0.0f, v2 = valid ? -d[2] : 0.0f;
        const float o = (g == 0) ? v0 : (g == 1) ? v1 : v2;
        const int64_t s = tile_base + 16 * j + c;
        if (s >= n_eff) continue;
        if (g == 3) {
            if (A.det) A.det[s] = det;
            if (A.valid) A.valid[s] = valid ? 1 : 0;
            continue;
        }
        if (A.velocity) A.velocity[3 * s + g] = o;
    }
}

struct VelocityOp : SampleOp {
    using Args = VelArgs;
    template <typename W, int NP>
    __device__ __forceinline__ static void tile(const VelArgs &A, const Shared &, const typename W::Elem *w, int64_t tile_base,
                                                int64_t n_eff, int lane)
    {
        const int g = lane >> 4, c = lane & 15;
        float px[NP][3], tq[NP], mv[NP][3], J[NP][12];
        load_samples<NP>(A.src, tile_base, n_eff, c, px, tq);
        motion_move_jacobian<W, NP>(w, lane, px, RowTime<NP>{ tq }, A.moving_step, A.use_div, mv, J);
        velocity_store<NP>(A, J, tile_base, n_eff, g, c);
    }
};

}  // namespace ced

extern "C" int ced_field_move_jacobian(const ced_field_desc *desc, int64_t n, const float *positions, const float *t, float *move,
                                       float *jac, void *stream)
{
    int rc = ced::validate_desc(desc, "field_move_jacobian");
    if (rc) return rc;
    CED_REQUIRE(n >= 0, "field_move_jacobian: n < 0");
    if (n == 0) return CED_OK;
    CED_REQUIRE(positions && t, "field_move_jacobian: null positions/t");
    CED_REQUIRE(move || jac, "field_move_jacobian: no output requested");
    ced::JacArgs A{};
    A.n = n;
    A.pos = positions; A.t = t;
    A.move = move; A.jac = jac;
    return ced::launch_motion<ced::JacobianOp, 1>(desc, A, "field_move_jacobian", stream);
}

extern "C" int ced_field_move_inverse_newton(const ced_field_desc *desc, int64_t n, const float *target, const float *t,
                                             const float *init, int32_t max_iters, float tol, float *x, float *step,
                                             int32_t *evals, void *stream)
{
    return ced::solve_rows(desc, n, target, t, init, max_iters, tol, x, step, evals, "field_move_inverse_newton",
                           ced::launch_motion<ced::NewtonOp, 1>, stream);
}

extern "C" int ced_field_track_newton(const ced_field_desc *desc, int64_t n_points, int64_t n_times, const float *target,
                                      const float *times, const float *init, int32_t max_iters, float tol, float *x,
                                      float *step, int32_t *evals, void *stream)
{
    return ced::solve_track(desc, n_points, n_times, target, times, init, max_iters, tol, x, step, evals, "field_track_newton",
                            ced::launch_motion<ced::NewtonOp, 1>, stream);
}

extern "C" int ced_field_velocity(const ced_field_desc *desc, int64_t n, const float *positions, const float *t, float *velocity,
                                  float *det, uint8_t *valid, void *stream)
{
    ced::VelArgs A{};
    const int rc = ced::point_samples(desc, n, positions, t, velocity || det || valid, "field_velocity", A.src);
    if (rc || n == 0) return rc;
    A.velocity = velocity; A.det = det; A.valid = valid;
    return ced::launch_motion<ced::VelocityOp, 1>(desc, A, "field_velocity", stream);
}

extern "C" int ced_field_velocity_rays(const ced_field_desc *desc, int64_t n, const int64_t *n_dev, const float *rays_o,
                                       const float *rays_d, const int64_t *ray_indices, const float *t_starts,
                                       const float *t_ends, const float *timestamps, int32_t t_per_ray, float *velocity,
                                       float *det, uint8_t *valid, void *stream)
{
    ced::VelArgs A{};
    const int rc = ced::ray_samples(desc, n, n_dev, rays_o, rays_d, ray_indices, t_starts, t_ends, timestamps, t_per_ray,
                                    velocity || det || valid, "field_velocity_rays", A.src);
    if (rc || n == 0) return rc;
    A.velocity = velocity; A.det = det; A.valid = valid;
    return ced::launch_motion<ced::VelocityOp, 1>(desc, A, "field_velocity_rays", stream);
}
