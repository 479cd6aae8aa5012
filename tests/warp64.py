"""numpy models of the warp's derivative, for tests/test_warp_jacobian_cpu.py and tests/test_gpu_warp_jacobian.py.

* `move_jacobian`: the motion network and its forward-mode Jacobian with respect to (x, y, z, t), in float64 or float32,
  optionally with the weights and every layer's inputs (features, activations and tangents alike) rounded as an
  mlp_precision rounds them: "f32" to float32, "f16" to one float16, "f16x2" to hi + lo float16.
* `complex_step`: the derivative of the float64 `move` model by a complex step, which pins `move_jacobian` itself.
* `newton_f32`: include/cednerf_hip.h's Newton iteration line by line in numpy float32 (IEEE single, no contraction), on
  any (x, t) -> (move, jac) callable.
* `solve64`, `velocity`, `carried_normals`: what the accuracy tests compare against.
"""
import math

import numpy as np

MOTION_MODES = {"f32": "f32", "f32+h16x2": "f32", "f16": "f16", "f16x2": "f16x2"}     # mlp_precision -> the motion network's


def rounder(mode, dtype):
    """v -> v as `mode` holds a matrix operand, returned in `dtype`"""
    if mode is None:
        return lambda v: v
    if mode == "f32":
        return lambda v: v.astype(np.float32).astype(dtype)
    if mode == "f16":
        return lambda v: v.astype(np.float16).astype(dtype)
    if mode == "f16x2":
        def split(v):
            hi = v.astype(np.float16).astype(dtype)
            return hi + (v - hi).astype(np.float16).astype(dtype)
        return split
    raise ValueError(mode)


def features(x4, dtype):
    """tcnn Frequency(4) of [n,4] -> [n,32] in the order of xyz_wrap's input: dimension, frequency, (sin, cos)"""
    enc = []
    for d in range(4):
        for k in range(4):
            ang = dtype((2 ** k) * math.pi) * x4[:, d]
            enc += [np.sin(ang), np.sin(ang + dtype(0.5 * math.pi))]
    return np.stack(enc, -1)


def move_jacobian(params, x, t, dtype=np.float64, mode=None):
    """(move [n,3], jac [n,3,4], pre) -- pre: the three hidden layers' primal pre-activations [n,64]"""
    rnd = rounder(mode, dtype)
    x4 = np.concatenate([x, t[:, None]], -1).astype(dtype)
    n = x4.shape[0]
    h = features(x4, dtype)
    dh = np.zeros((n, 32, 4), dtype)                                     # tangents: [n, feature, direction]
    for d in range(4):
        for k in range(4):
            w = dtype((2 ** k) * math.pi)
            dh[:, 8 * d + 2 * k, d] = w * h[:, 8 * d + 2 * k + 1]
            dh[:, 8 * d + 2 * k + 1, d] = -w * h[:, 8 * d + 2 * k]
    ws = [rnd(np.asarray(w, dtype)) for w in params["xyz_wrap"]]
    pre = []
    for i, w in enumerate(ws):
        z = rnd(h) @ w.T
        dz = np.einsum("of,nfb->nob", w, rnd(dh))
        if i < len(ws) - 1:
            pre.append(z)
            on = z > 0
            h, dh = np.where(on, z, 0), np.where(on[:, :, None], dz, 0)
        else:
            h, dh = z, dz
    step = dtype(np.float32(params["moving_step"]))
    if params["use_div_offsets"]:
        th = np.tanh(h[:, 3:])
        move = (h[:, :3] + th) * step
        jac = (dh[:, :3] + (1 - th * th)[:, :, None] * dh[:, 3:]) * step
    else:
        move, jac = h * step, dh * step
    return move, jac, pre


def move64(params, x, t):
    return move_jacobian(params, x, t)[0]


def complex_step(params, x, t, h=1e-30):
    """jac [n,3,4] of the float64 move model: Im move(p + i h e_b) / h, the ReLU deciding on the real part"""
    out = []
    for b in range(4):
        x4 = np.concatenate([x, t[:, None]], -1).astype(np.complex128)
        x4[:, b] += 1j * h
        a = features(x4, np.float64)
        ws = [np.asarray(w, np.float64) for w in params["xyz_wrap"]]
        for i, w in enumerate(ws):
            a = a @ w.T
            if i < len(ws) - 1:
                a = np.where(a.real > 0, a, 0)
        mv = (a[:, :3] + np.tanh(a[:, 3:]) if params["use_div_offsets"] else a) * np.float64(np.float32(params["moving_step"]))
        out.append(mv.imag / h)
    return np.stack(out, -1)


def kept_rows(pre, rel=1e-5):
    """rows none of whose hidden pre-activations lies within rel * (the layer's largest magnitude) of zero"""
    keep = np.ones(pre[0].shape[0], bool)
    for z in pre:
        keep &= (np.abs(z) > rel * np.abs(z).max()).all(-1)
    return keep


# ---- 3 x 3 algebra ----------------------------------------------------------------------------------------------------
def cofactors(A):
    """C[..., a, b] = A[a+1][b+1] * A[a+2][b+2] - A[a+1][b+2] * A[a+2][b+1], indices mod 3, in A's dtype"""
    C = np.empty_like(A)
    for a in range(3):
        for b in range(3):
            a1, a2, b1, b2 = (a + 1) % 3, (a + 2) % 3, (b + 1) % 3, (b + 2) % 3
            C[..., a, b] = A[..., a1, b1] * A[..., a2, b2] - A[..., a1, b2] * A[..., a2, b1]
    return C


def gradient_inverse(jac):
    """(A = I + jac[..., :3], A^-1 by the adjugate, det A) in jac's dtype"""
    A = jac[..., :3] + np.eye(3, dtype=jac.dtype)
    C = cofactors(A)
    det = (A[..., 0, 0] * C[..., 0, 0] + A[..., 0, 1] * C[..., 0, 1]) + A[..., 0, 2] * C[..., 0, 2]
    return A, np.swapaxes(C, -1, -2) / det[..., None, None], det


# ---- the Newton iteration of include/cednerf_hip.h ------------------------------------------------------------------------
def newton_step_f32(J, r):
    """d [n,3] from J [n,3,4], r [n,3], all float32: the adjugate solve, or r where it is refused"""
    assert J.dtype == np.float32 and r.dtype == np.float32
    A = J[:, :, :3].copy()
    for a in range(3):
        A[:, a, a] = np.float32(1.0) + J[:, a, a]
    C = cofactors(A)
    with np.errstate(all="ignore"):
        det = (A[:, 0, 0] * C[:, 0, 0] + A[:, 0, 1] * C[:, 0, 1]) + A[:, 0, 2] * C[:, 0, 2]
        d = np.stack([((C[:, 0, a] * r[:, 0] + C[:, 1, a] * r[:, 1]) + C[:, 2, a] * r[:, 2]) / det for a in range(3)], -1)
        fine = (np.abs(det) >= np.float32(2.0 ** -20)) & np.isfinite(d).all(-1)
    assert det.dtype == np.float32 and d.dtype == np.float32
    return np.where(fine[:, None], d, r)


def newton_f32(move_jac, c, t, K, tol, init=None):
    """(x, step, evals) of ced_field_move_inverse_newton; move_jac(x, t) -> (move [n,3], jac [n,3,4]) float32"""
    c = np.ascontiguousarray(c, np.float32)
    x = (c if init is None else np.asarray(init, np.float32)).copy()
    n = c.shape[0]
    step = np.full(n, np.inf, np.float32)
    evals = np.zeros(n, np.int32)
    active = np.ones(n, bool)
    tol = np.float32(tol)
    for k in range(1, K + 1):
        m, J = move_jac(x, t)
        assert m.dtype == np.float32 and J.dtype == np.float32
        r = (x + m) - c
        with np.errstate(invalid="ignore"):
            res = np.fmax(np.fmax(np.abs(r[:, 0]), np.abs(r[:, 1])), np.abs(r[:, 2]))
            step = np.where(active, res, step)
            evals += active
            active &= ~(res <= tol)
            if k == K or not active.any():
                break
            x = np.where(active[:, None], x - newton_step_f32(J, r), x)
    return x, step, evals


def model_move_jac(params, dtype=np.float32, mode=None):
    def fn(x, t):
        m, J, _ = move_jacobian(params, x, t, dtype, mode)
        return m.astype(dtype), J.astype(dtype)
    return fn


# ---- float64 references -----------------------------------------------------------------------------------------------
def solve64(params, c, t, start=None, rounds=60):
    """x with x + move(x, t) = c in float64 by Newton's method, to a standstill; rows that do not get there are NaN"""
    c = c.astype(np.float64)
    t = t.astype(np.float64)
    x = c.copy() if start is None else start.astype(np.float64).copy()
    for _ in range(rounds):
        m, J, _ = move_jacobian(params, x, t)
        r = x + m - c
        if np.abs(r).max() <= 1e-15:
            break
        x = x - np.einsum("nab,nb->na", gradient_inverse(J)[1], r)
    m = move64(params, x, t)
    x[~(np.abs(x + m - c).max(-1) <= 1e-13)] = np.nan
    return x


def velocity(jac):
    """v = -(I + J_x)^-1 d move / dt [n,3] and det(I + J_x) [n], in jac's dtype"""
    _, inv, det = gradient_inverse(jac)
    return -np.einsum("...ab,...b->...a", inv, jac[..., 3]), det


def carried_normals(jac_t, jac_ref, n_ref):
    """(I + J_t)^T (I + J_ref)^-T n_ref, normalised, in the inputs' dtype"""
    A_t = gradient_inverse(jac_t)[0]
    inv_ref = gradient_inverse(jac_ref)[1]
    g = np.einsum("...ba,...b->...a", inv_ref, n_ref)
    n_t = np.einsum("...ba,...b->...a", A_t, g)
    return n_t / np.linalg.norm(n_t, axis=-1, keepdims=True)
