"""Naive surface nets in numpy float32: the test reference of csrc/mesh.hip, restated from the definition in
include/cednerf_hip.h (not from the kernel), vectorised over cubes and edges so reso 48 takes seconds.  Every float32
operation below is one rounding, in the definition's order, so the kernel's output is expected bit for bit.

Also here: the analytic lattices the mesh tests share and four mesh checkers (directed-edge balance, 2-manifoldness, Euler
characteristic, signed volume)."""
import numpy as np

F32 = np.float32


def origin_and_step(reso, center, radius):
    r = F32(radius)
    return np.asarray(center, F32) - r, (F32(2.0) * r) / F32(reso)


def node_positions(reso, center=(0.0, 0.0, 0.0), radius=1.5):
    """[reso, reso, reso, 3] float32: lo_a + (i_a + 0.5) * h"""
    lo, h = origin_and_step(reso, center, radius)
    i = np.arange(reso, dtype=F32) + F32(0.5)
    axes = [lo[a] + i * h for a in range(3)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), -1).astype(F32)


def surface_nets(S, thresh, center, radius):
    """S [reso,reso,reso] -> vertices [V,3] f32, normals [V,3] f32, cube [V] int64, faces [F,3] int32"""
    S = np.ascontiguousarray(S, F32)
    reso = S.shape[0]
    assert S.shape == (reso, reso, reso)
    thresh = F32(thresh)
    lo, h = origin_and_step(reso, center, radius)
    with np.errstate(all="ignore"):
        inside = S >= thresh                                                     # False for a NaN
        m = reso - 1                                                             # cubes per axis
        corner = lambda x, y, z, A: A[x:x + m, y:y + m, z:z + m]
        n_in = np.zeros((m, m, m), np.int32)
        for x in (0, 1):
            for y in (0, 1):
                for z in (0, 1):
                    n_in += corner(x, y, z, inside)
        ijk = np.argwhere((n_in > 0) & (n_in < 8))                               # C order: the cube id ascends
        V = ijk.shape[0]
        cube = (ijk[:, 0].astype(np.int64) * reso + ijk[:, 1]) * reso + ijk[:, 2]
        s = np.empty((V, 2, 2, 2), F32)
        for x in (0, 1):
            for y in (0, 1):
                for z in (0, 1):
                    s[:, x, y, z] = S[ijk[:, 0] + x, ijk[:, 1] + y, ijk[:, 2] + z]
        acc, g, cnt = np.zeros((V, 3), F32), np.zeros((V, 3), F32), np.zeros(V, np.int32)
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            for ob in (0, 1):
                for oc in (0, 1):
                    p0 = [0, 0, 0]
                    p0[b], p0[c] = ob, oc
                    p1 = list(p0)
                    p1[a] = 1
                    s0, s1 = s[:, p0[0], p0[1], p0[2]], s[:, p1[0], p1[1], p1[2]]
                    d = s1 - s0
                    g[:, a] = g[:, a] + d
                    cross = (s0 >= thresh) != (s1 >= thresh)
                    mu = (thresh - s0) / d
                    mu = np.where(np.isfinite(mu), mu, F32(0.5)).astype(F32)
                    mu = np.minimum(np.maximum(mu, F32(0.0)), F32(1.0))
                    for k in range(3):
                        q = mu if k == a else np.full(V, F32(p0[k]), F32)
                        acc[:, k] = np.where(cross, acc[:, k] + q, acc[:, k])
                    cnt += cross
        u = acc / cnt.astype(F32)[:, None]
        vertices = np.empty((V, 3), F32)
        for a in range(3):
            vertices[:, a] = lo[a] + ((ijk[:, a].astype(F32) + F32(0.5)) + u[:, a]) * h
        length = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        ok = (length > 0) & np.isfinite(length)
        normals = np.where(ok[:, None], -(g / length[:, None]), F32(0.0)).astype(F32)

    rank = np.full(reso ** 3, -1, np.int64)
    rank[cube] = np.arange(V)
    node = np.arange(reso ** 3, dtype=np.int64).reshape(reso, reso, reso)
    idx = np.indices((reso, reso, reso))
    stride = (reso * reso, reso, 1)
    keys = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        nxt = np.roll(inside, -1, axis=a)                                        # the wrapped plane is masked out below
        act = (idx[a] < reso - 1) & (inside != nxt)
        for o in (b, c):
            act &= (idx[o] >= 1) & (idx[o] <= reso - 2)
        keys.append(3 * node[act] + a)
    keys = np.sort(np.concatenate(keys)) if keys else np.zeros(0, np.int64)
    n, a = keys // 3, keys % 3
    eb, ec = np.take(stride, (a + 1) % 3), np.take(stride, (a + 2) % 3)
    q0, q1, q2, q3 = rank[n - eb - ec], rank[n - ec], rank[n], rank[n - eb]
    n_inside = inside.reshape(-1)[n]
    first = np.where(n_inside[:, None], np.stack([q0, q1, q2], -1), np.stack([q0, q2, q1], -1))
    second = np.where(n_inside[:, None], np.stack([q0, q2, q3], -1), np.stack([q0, q3, q2], -1))
    faces = np.stack([first, second], 1).reshape(-1, 3).astype(np.int32)
    return vertices, normals, cube, faces


# ---- lattices (cube centre 0, radius 1.5, iso-value 1.0) -------------------------------------------------------------
CENTER, RADIUS, THRESH = (0.0, 0.0, 0.0), 1.5, 1.0
SPHERE_CENTER, SPHERE_RADIUS = (0.13, -0.07, 0.21), 0.9


def sphere_lattice(reso):
    """S = exp(8 (0.9 - |p - c|))"""
    p = node_positions(reso).astype(np.float64)
    return np.exp(8.0 * (SPHERE_RADIUS - np.linalg.norm(p - np.asarray(SPHERE_CENTER), axis=-1))).astype(F32)


def torus_lattice(reso):
    """S = exp(8 (0.4 - sqrt((sqrt(x^2 + y^2) - 0.85)^2 + z^2)))"""
    p = node_positions(reso).astype(np.float64)
    ring = np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - 0.85
    return np.exp(8.0 * (0.4 - np.sqrt(ring ** 2 + p[..., 2] ** 2))).astype(F32)


def noise_lattice(reso, closed=True):
    """uniform noise in [0, 2), default_rng(5); closed: the six border slabs zeroed, so no sign change touches the border"""
    S = np.random.default_rng(5).uniform(0.0, 2.0, size=(reso, reso, reso)).astype(F32)
    if closed:
        for a in range(3):
            sl = [slice(None)] * 3
            for i in (0, -1):
                sl[a] = i
                S[tuple(sl)] = 0.0
    return S


def special_lattice(reso):
    """the open noise lattice with NaN, +inf and -inf nodes scattered through it"""
    S = noise_lattice(reso, closed=False).reshape(-1)
    S[::37] = np.nan
    S[3::41] = np.inf
    S[5::43] = -np.inf
    return S.reshape(reso, reso, reso)


# ---- checkers ----------------------------------------------------------------------------------------------------------
def _directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def directed_edges_balance(faces):
    """every directed edge u -> v occurs as often as v -> u (the surface is closed and consistently oriented)"""
    e = _directed_edges(faces)
    if e.shape[0] == 0:
        return True
    base = int(e.max()) + 1
    fwd, n_fwd = np.unique(e[:, 0] * base + e[:, 1], return_counts=True)
    rev, n_rev = np.unique(e[:, 1] * base + e[:, 0], return_counts=True)
    return bool(np.array_equal(fwd, rev) and np.array_equal(n_fwd, n_rev))


def is_two_manifold(faces):
    """closed oriented 2-manifold: every directed edge occurs once and so does its reverse, no degenerate triangle, and
    the triangles round every vertex form one cycle (its link is connected)"""
    f = np.asarray(faces, np.int64)
    if f.shape[0] == 0:
        return True
    if (f[:, 0] == f[:, 1]).any() or (f[:, 1] == f[:, 2]).any() or (f[:, 0] == f[:, 2]).any():
        return False
    e = _directed_edges(f)
    base = int(e.max()) + 1
    _, counts = np.unique(e[:, 0] * base + e[:, 1], return_counts=True)
    if (counts != 1).any() or not directed_edges_balance(f):
        return False
    link = {}                                              # vertex -> {u: w} for each triangle (vertex, u, w)
    for tri in f:
        for k in range(3):
            link.setdefault(int(tri[k]), {})[int(tri[(k + 1) % 3])] = int(tri[(k + 2) % 3])
    for nxt in link.values():
        start = next(iter(nxt))
        at, steps = nxt.get(start), 1
        while at is not None and at != start and steps <= len(nxt):
            at, steps = nxt.get(at), steps + 1
        if at != start or steps != len(nxt):
            return False
    return True


def euler_characteristic(faces):
    """V - E + F over the vertices the faces reference"""
    f = np.asarray(faces, np.int64)
    e = np.sort(_directed_edges(f), axis=1)
    return int(np.unique(f).size - np.unique(e, axis=0).shape[0] + f.shape[0])


def signed_volume(vertices, faces):
    """sum of v0 . (v1 x v2) / 6 in float64: positive for a closed surface whose triangles are counter-clockwise from
    outside"""
    v = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)
