"""numpy models of the flow outputs, for tests/test_scene_flow_cpu.py and tests/test_gpu_scene_flow.py.

* `velocity_f32`: include/cednerf_hip.h's guarded velocity line by line in numpy float32 (IEEE single, no contraction), on a
  float32 Jacobian [n,3,4] -- the adjugate solve of warp64.newton_step_f32 with r = the time column and the guard
  det >= 2^-20 and a finite quotient.
* `velocity_rounding_bound`: what float32 rounding of those lines can cost against the same lines in exact arithmetic.
* `flow_rgb8`: the header's colour wheel in numpy float32.
* `pinhole_rays` / `pinhole_project`: the reference's pixel-centre rays and their inverse, in any dtype.
* `inputs`: the rows of tests/test_gpu_track.py as numpy arrays (no device needed).
"""
import numpy as np

import warp64 as W

DET_FLOOR = np.float32(2.0 ** -20)


def inputs(n=4099):
    """tests/test_gpu_track.py's `_inputs` without the device: default_rng(7), positions in +-1.6, times in [0, 1]"""
    rng = np.random.default_rng(7)
    pos = rng.uniform(-1.6, 1.6, size=(n, 3)).astype(np.float32)
    t = rng.uniform(0.0, 1.0, size=(n,)).astype(np.float32)
    return pos, t


def velocity_f32(J):
    """(v [n,3], det [n], valid [n] bool) from J [n,3,4] float32"""
    assert J.dtype == np.float32
    one, zero = np.float32(1.0), np.float32(0.0)
    r = J[:, :, 3]
    A = J[:, :, :3].copy()
    for a in range(3):
        A[:, a, a] = one + J[:, a, a]
    C = W.cofactors(A)
    with np.errstate(all="ignore"):
        det = A[:, 0, 0] * C[:, 0, 0]
        det = det + A[:, 0, 1] * C[:, 0, 1]
        det = det + A[:, 0, 2] * C[:, 0, 2]
        d = []
        for a in range(3):
            num = C[:, 0, a] * r[:, 0]
            num = num + C[:, 1, a] * r[:, 1]
            num = num + C[:, 2, a] * r[:, 2]
            d.append(num / det)
        d = np.stack(d, -1)
        valid = det >= DET_FLOOR                                        # false for a NaN and for a fold
        valid = valid & (np.abs(d) < np.float32(np.inf)).all(-1)
    v = np.where(valid[:, None], -d, zero)
    assert det.dtype == np.float32 and v.dtype == np.float32
    return v, det, valid


def velocity_rounding_bound(J):
    """(bound on |v_f32 - v_exact| [n,3], bound on |det_f32 - det_exact| [n]) for the header's lines on the float32 J, in
    float64: every line is a sum of products; each product and each sum rounds once (u = 2^-24), so a line of depth k
    errs by at most ~k u times the sum of the ABSOLUTE values of its terms.  A cofactor has depth 3 (diagonal 1 + J,
    product, difference), det and the numerators depth 3 more, the quotient one: 8 u covers each, to first order."""
    u = 2.0 ** -24
    J = J.astype(np.float64)
    A = J[..., :3] + np.eye(3)
    r = np.abs(J[..., 3])
    C = W.cofactors(A)
    absA = np.abs(A)
    Cabs = np.empty_like(A)
    for a in range(3):
        for b in range(3):
            a1, a2, b1, b2 = (a + 1) % 3, (a + 2) % 3, (b + 1) % 3, (b + 2) % 3
            Cabs[..., a, b] = absA[..., a1, b1] * absA[..., a2, b2] + absA[..., a1, b2] * absA[..., a2, b1]
    det = (A[..., 0, :] * C[..., 0, :]).sum(-1)
    det_abs = (absA[..., 0, :] * Cabs[..., 0, :]).sum(-1)
    num = np.einsum("...ba,...b->...a", C, J[..., 3])
    num_abs = np.einsum("...ba,...b->...a", Cabs, r)
    e_det = 8 * u * det_abs
    e_v = 8 * u * num_abs / np.abs(det)[..., None] + np.abs(num) * e_det[..., None] / (det * det)[..., None]
    return e_v, e_det


# ---- the colour wheel of ced_flow_to_rgb8 ------------------------------------------------------------------------------
def flow_rgb8(flow, max_mag, flip_w=True):
    """uint8 [H,W,3] from flow [H,W,2] float32, the header's lines in numpy float32"""
    f32 = np.float32
    flow = np.asarray(flow, f32)
    fx, fy = flow[..., 0], flow[..., 1]
    with np.errstate(all="ignore"):
        finite = np.isfinite(fx) & np.isfinite(fy)
        h = np.arctan2(fy, fx).astype(f32) * f32(0.15915494309189535)
        h = np.where(h < 0, h + f32(1.0), h)
        h = np.where(h >= 1, f32(0.0), h).astype(f32)
        h6 = h * f32(6.0)
        sat = np.minimum(np.sqrt(fx * fx + fy * fy) / f32(max_mag), f32(1.0)).astype(f32)
        out = np.zeros(flow.shape[:-1] + (3,), np.uint8)
        for c, n in enumerate((5.0, 3.0, 1.0)):
            k = f32(n) + h6
            k = np.where(k >= 6, k - f32(6.0), k).astype(f32)
            m = np.minimum(np.minimum(k, f32(4.0) - k), f32(1.0))
            ch = f32(1.0) - sat * np.maximum(m, f32(0.0))
            v = np.clip(ch * f32(255.0), 0, 255)
            out[..., c] = np.where(finite, np.nan_to_num(v), 0).astype(np.uint8)      # the cast truncates toward zero
    return out[:, ::-1].copy() if flip_w else out


# ---- the pinhole camera -------------------------------------------------------------------------------------------------
def pinhole_rays(K, c2w, width, height, opengl, dtype=np.float64):
    """The reference's pixel-centre rays (datasets/dnerf_synthetic.py:191-221), restated: for pixel (x, y) the camera-space
    direction ((x - cx + 0.5) / fx, (y - cy + 0.5) / fy * s, s), s = -1 for OpenGL (y up, looking down -z) and +1 for
    OpenCV; rotated by c2w[:3,:3]; the origin is c2w[:3,3].  Returns (origins, UNNORMALISED directions, x, y) flat [H*W]."""
    K, c2w = np.asarray(K, dtype), np.asarray(c2w, dtype)[:3, :4]
    x, y = np.meshgrid(np.arange(width, dtype=dtype), np.arange(height, dtype=dtype), indexing="xy")
    x, y = x.reshape(-1), y.reshape(-1)
    s = dtype(-1.0 if opengl else 1.0)
    half = dtype(0.5)
    cam = np.stack([(x - K[0, 2] + half) / K[0, 0], (y - K[1, 2] + half) / K[1, 1] * s, np.full_like(x, s)], -1)
    d = (cam[:, None, :] * c2w[None, :, :3]).sum(-1)
    o = np.broadcast_to(c2w[:, 3], d.shape).copy()
    return o, d, x, y


def pinhole_project(K, c2w, opengl, points, dtype):
    """cameras.pinhole_projector's formula in numpy, every operation in `dtype`"""
    K, c2w = np.asarray(K, np.float64), np.asarray(c2w, np.float64)[:3, :4]
    inv_t = np.linalg.inv(c2w[:, :3]).T.astype(dtype)
    origin = c2w[:, 3].astype(dtype)
    s = -1.0 if opengl else 1.0
    pc = (points.astype(dtype) - origin) @ inv_t
    z = pc[:, 2]
    px = dtype(s * K[0, 0]) * (pc[:, 0] / z) + dtype(K[0, 2] - 0.5)
    py = dtype(K[1, 1]) * (pc[:, 1] / z) + dtype(K[1, 2] - 0.5)
    return np.stack([px, py], -1), (z * dtype(s)) > 0
