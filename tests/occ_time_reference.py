"""Numpy restatements for the time-sliced occupancy grid tests (no GPU, nothing of the package's kernels):

  time_slices      ced_occ_time_slices' definition (include/cednerf_hip.h): the float32 multiply, the `>`, the 27-neighbour
                   OR inside a level, the AND with the union;
  probe_times      TimeSlicedOccGrid.probe_times' float32 lines;
  cell_centres     ops.occ_cell_points with noise 0.5, in float32, operation by operation;
  ball_*           the hand-made "moving ball" field of tests/test_gpu_time_slices.py and its slices from a density function.
"""
import numpy as np


def time_slices(cell_ids, max_sigma, step_size, thre, levels, res, union=None, dilate=1):
    """cell_ids [n] int64, max_sigma [B,n] float32 -> bool [B, levels, R, R, R]"""
    max_sigma = np.asarray(max_sigma, np.float32)
    B = max_sigma.shape[0]
    hit = np.zeros((B, levels * res ** 3), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = max_sigma * np.float32(step_size)                         # float32 x float32 -> float32, rounded once
        hit[:, np.asarray(cell_ids, np.int64)] = prod > np.float32(thre)  # false for a NaN
    hit = hit.reshape(B, levels, res, res, res)
    out = hit
    if dilate:
        pad = np.zeros((B, levels, res + 2, res + 2, res + 2), bool)
        pad[:, :, 1:-1, 1:-1, 1:-1] = hit
        out = np.zeros_like(hit)
        for dx in range(3):
            for dy in range(3):
                for dz in range(3):
                    out |= pad[:, :, dx:dx + res, dy:dy + res, dz:dz + res]
    if union is not None:
        out = out & np.asarray(union, bool)[None]
    return out


def probe_times(n_bins, times_per_bin):
    """[B, S] float32: (b + s / (S - 1)) / B, every operation in float32; S = 1: the midpoint"""
    b = np.arange(n_bins, dtype=np.float32)[:, None]
    s = np.arange(times_per_bin, dtype=np.float32)[None, :]
    frac = s / np.float32(times_per_bin - 1) if times_per_bin >= 2 else np.full_like(s, 0.5)
    return ((b + frac) / np.float32(n_bins)).astype(np.float32)


def cell_centres(cells, res, aabb):
    """world centres [n,3] of the cells (ix * R + iy) * R + iz of a level with box aabb: occ_points_kernel's float32 lines"""
    cells = np.asarray(cells, np.int64)
    aabb = np.asarray(aabb, np.float32)
    idx = np.stack([cells // (res * res), (cells // res) % res, cells % res], axis=-1).astype(np.float32)
    x = (idx + np.float32(0.5)) / np.float32(res)
    return (aabb[:3] + x * (aabb[3:] - aabb[:3])).astype(np.float32)


# ---- the moving ball ---------------------------------------------------------------------------------------------------
BALL_AABB = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
BALL_CENTRE, BALL_RADIUS = (0.4, 0.0, 0.0), 0.4
BALL_GRID = dict(resolution=32, levels=1, n_bins=8, times_per_bin=3, dilate=1, render_step_size=5e-3, occ_thre=0.01)


def ball_params():
    """Parameters (synthetic.init_field_params' layout, log2 table 15, hash_max_res 256) of a field whose geometry is known:
    the table is zero except level 0's feature 0, 1.0 at the lattice vertices within 0.4 of (0.4, 0, 0); mlp_base is zero
    except W0[0, 0] = 1 and W1[0, 0] = 8, so sigma = exp(8 f0 - 1); xyz_wrap is zero except one chain that carries the
    encoding's sin(pi t) input (Frequency(4) on (x, y, z, t): input 8 * 3 + 0) through the three hidden layers to output x
    with weight 1; moving_step = 1: the canonical point is x + (sin(pi t), 0, 0), the ball slides by -sin(pi t) along x."""
    from ced_nerf_amd.hashgrid import level_tables
    lv = level_tables(16, 256, 16, 15)
    table = np.zeros((int(lv["total"]), 2), np.float32)
    assert not lv["hashed"][0]
    r, scale = int(lv["res"][0]), float(lv["scale"][0])
    i = np.arange(r, dtype=np.float64)
    world = BALL_AABB[0] + ((i - 0.5) / scale) * (BALL_AABB[3] - BALL_AABB[0])     # vertex i of an axis: x_norm * scale + 0.5 = i
    X, Y, Z = np.meshgrid(world, world, world, indexing="ij")
    inside = (X - BALL_CENTRE[0]) ** 2 + (Y - BALL_CENTRE[1]) ** 2 + (Z - BALL_CENTRE[2]) ** 2 <= BALL_RADIUS ** 2
    ix, iy, iz = np.nonzero(inside)
    table[int(lv["offset"][0]) + ix + iy * r + iz * r * r, 0] = 1.0        # dense level: x + y * res + z * res^2
    z = lambda *shape: np.zeros(shape, np.float32)
    m = [z(64, 32), z(64, 64), z(64, 64), z(3, 64)]
    m[0][0, 24] = m[1][0, 0] = m[2][0, 0] = m[3][0, 0] = 1.0
    b = [z(64, 32), z(16, 64)]
    b[0][0, 0], b[1][0, 0] = 1.0, 8.0
    return dict(aabb=np.asarray(BALL_AABB, np.float32), moving_step=1.0, use_div_offsets=False, time_mode=0,
                hash=dict(base_res=16, max_res=256, n_levels=16, log2_hashmap_size=15, table=table, temporal=False),
                xyz_wrap=m, mlp_base=b, mlp_head=[z(64, 19), z(64, 64), z(3, 64)])


def nan_inf_params():
    """The ball's field with another density: level 0's feature 0 is 3e38 on the vertices of the lower half in x, feature 1
    on those of the lower half in y; mlp_base has W0[0, 0] = W0[1, 1] = 8 (the hidden units overflow to inf there) and
    W1[0, 0] = 1, W1[0, 1] = 0.  On the fp32 chain the raw density is inf where only feature 0 is large, 0 x inf = NaN where
    feature 1 is, 0 elsewhere; the fp16 modes clamp to 65504 and give inf without NaN.  The motion slides rows between the
    regions from probe to probe."""
    from ced_nerf_amd.hashgrid import level_tables
    lv = level_tables(16, 256, 16, 15)
    r, off = int(lv["res"][0]), int(lv["offset"][0])
    p = ball_params()
    b = p["mlp_base"]
    b[0][0, 0] = b[0][1, 1] = 8.0
    b[1][0, 0], b[1][0, 1] = 1.0, 0.0
    table = p["hash"]["table"]
    table[:] = 0.0
    ix, iy, iz = np.meshgrid(np.arange(r), np.arange(r), np.arange(r), indexing="ij")
    idx = off + ix + iy * r + iz * r * r
    table[idx[ix < r // 2], 0] = 3e38
    table[idx[iy < r // 2], 1] = 3e38
    return p


def ball_slices(density_fn):
    """The slices of BALL_GRID by the composition, candidates = all cells: density_fn(pos [n,3], t [n]) -> sigma [n]."""
    g = BALL_GRID
    res, B, S = g["resolution"], g["n_bins"], g["times_per_bin"]
    cells = np.arange(res ** 3, dtype=np.int64)
    pos = cell_centres(cells, res, BALL_AABB)
    times = probe_times(B, S)
    mx = np.zeros((B, len(cells)), np.float32)
    for b in range(B):
        for s in range(S):
            mx[b] = np.fmax(mx[b], density_fn(pos, np.full(len(cells), times[b, s], np.float32)))
    return time_slices(cells, mx, g["render_step_size"], g["occ_thre"], 1, res, None, g["dilate"])
