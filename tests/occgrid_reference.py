"""Plain-numpy references of the occupancy grid's two device-built pieces (no project code):

  ema_update        the contract of ced_occ_ema_update (include/cednerf_hip.h) for ANY index list, duplicates included
  chebyshev_fields  the brick and cell distance fields of ced_build_occupancy_accel, from their definition

and what the CPU and GPU tests of the distance fields share: the (levels, res) shapes, the occupancy patterns, the
layout of the accel buffer and the true (uncapped) distances the device field must never exceed."""
import numpy as np

BRICK = 8                   # cells per brick and axis
CAP = 15                    # distances are exact up to CAP; farther elements read CAP + 1 in the reference
FAR = 1 << 20               # "no occupied cell at all" in the uncapped distances

_I32_MIN = np.int32(-2 ** 31)


def _flip(b):
    """int32 bits of non-NaN floats <-> keys that order like the floats (-0 below +0).  Its own inverse."""
    return np.where(b >= 0, b, b ^ np.int32(0x7fffffff)).astype(np.int32)


def _key(x):
    return _flip(np.ascontiguousarray(x, np.float32).view(np.int32))


def ema_update(occs, ids, occ, decay):
    """new[c] = fmax(fl32(old[c] * decay), max over j with ids[j] == c of occ[j]) for every listed cell c; a NaN occ[j]
    contributes nothing (fmaxf's rule); unlisted cells keep their bits.  Of the outcomes the index assignment
    occs[ids] = maximum(occs[ids] * decay, occ) can have with duplicates -- max(old * decay, occ[j]) for some j -- this
    is the only one that does not depend on the order of the writers.  The maximum runs on order-preserving integer
    keys (np.maximum.at), so that +0 beats -0 whichever comes first."""
    occs = np.ascontiguousarray(occs, np.float32)
    ids = np.asarray(ids, np.int64).reshape(-1)
    occ = np.ascontiguousarray(occ, np.float32).reshape(-1)
    assert ids.shape == occ.shape and (ids.size == 0 or (ids.min() >= 0 and ids.max() < occs.size))
    listed = np.unique(ids)
    decayed = (occs[listed] * np.float32(decay)).astype(np.float32)
    keys = np.full(occs.shape, _I32_MIN, np.int32)                  # below the key of every number
    keys[listed] = np.where(np.isnan(decayed), _I32_MIN, _key(decayed))
    ok = ~np.isnan(occ)
    np.maximum.at(keys, ids[ok], _key(occ[ok]))
    new = occs.copy()
    won = keys[listed]
    new[listed] = np.where(won == _I32_MIN, decayed, _flip(won).view(np.float32))   # nothing but NaNs: fmax(NaN, -) = NaN
    return new


def brick_occupancy(binaries):
    """[m, nb, nb, nb] bool: any occupied cell in the brick (the last brick of an axis may be partial)."""
    b = np.asarray(binaries).astype(bool)
    m, res = b.shape[0], b.shape[1]
    nb = -(-res // BRICK)
    pad = nb * BRICK - res
    b = np.pad(b, ((0, 0), (0, pad), (0, pad), (0, pad)))
    return b.reshape(m, nb, BRICK, nb, BRICK, nb, BRICK).any(axis=(2, 4, 6))


def _dilate(a):
    """3 x 3 x 3 box dilation inside the array: one shift-or per axis and direction."""
    for ax in range(3):
        lo = [slice(None)] * 3; hi = [slice(None)] * 3
        lo[ax] = slice(None, -1); hi[ax] = slice(1, None)
        out = a.copy()
        out[tuple(hi)] |= a[tuple(lo)]
        out[tuple(lo)] |= a[tuple(hi)]
        a = out
    return a


def _capped_distance(occ):
    """Chebyshev distance of every element of one 3-D bool array to the nearest True one, CAP + 1 beyond CAP: an
    element first reached by round r of dilation has distance r.  Only the occupied elements' bounding box grown by
    CAP can hold a distance <= CAP, so the rounds run there."""
    dist = np.full(occ.shape, CAP + 1, np.uint8)
    if not occ.any():
        return dist
    box = []
    for ax in range(3):
        hit = np.flatnonzero(occ.any(axis=tuple(a for a in range(3) if a != ax)))
        box.append(slice(max(int(hit[0]) - CAP, 0), min(int(hit[-1]) + CAP + 1, occ.shape[ax])))
    box = tuple(box)
    reached = occ[box].copy()
    d = dist[box]                                                   # a view
    d[reached] = 0
    for r in range(1, CAP + 1):
        grown = _dilate(reached)
        new = grown & ~reached
        if not new.any():
            break
        d[new] = r
        reached = grown
    return dist


def chebyshev_fields(binaries):
    """(bdist [m, nb, nb, nb], cdist_exact [m, res, res, res]) uint8: per level, the Chebyshev distance of every brick
    to the nearest brick holding an occupied cell and of every cell to the nearest occupied cell -- exact up to CAP,
    CAP + 1 beyond.  Levels are independent."""
    b = np.asarray(binaries).astype(bool)
    assert b.ndim == 4 and b.shape[1] == b.shape[2] == b.shape[3]
    bricks = brick_occupancy(b)
    return (np.stack([_capped_distance(lv) for lv in bricks]), np.stack([_capped_distance(lv) for lv in b]))


def brute_force_distance(level):
    """Uncapped Chebyshev distance [res, res, res] (int32, FAR without any occupied cell) of one level by pairs: every
    unoccupied cell against every occupied one (an occupied cell is its own nearest, at distance 0)."""
    level = np.asarray(level).astype(bool)
    out = np.zeros(level.shape, np.int32)
    pts = np.argwhere(level)
    free = np.argwhere(~level)
    if pts.size == 0:
        out[:] = FAR
        return out
    if free.size == 0:
        return out
    best = np.full(len(free), FAR, np.int32)
    for p in pts:
        np.minimum(best, np.abs(free - p).max(axis=1).astype(np.int32), out=best)
    out[tuple(free.T)] = best
    return out


def single_cell_distance(res, p):
    """Uncapped distance field of one occupied cell p, in closed form."""
    ax = [np.abs(np.arange(res) - int(c)) for c in p]
    return np.maximum(np.maximum(ax[0][:, None, None], ax[1][None, :, None]), ax[2][None, None, :]).astype(np.int32)


# ---- the cases of the distance-field tests ---------------------------------------------------------------------------
SHAPES = [
    (1, 1),        # smallest grid
    (1, 7),        # less than one brick
    (1, 8),        # exactly one brick
    (2, 9),        # just over one brick, two levels
    (1, 21),       # size of the brute-force check of test_march_accel_cpu.py
    (3, 24),       # three bricks per axis, three levels
    (2, 40),       # size of the brute-force check, two levels
    (4, 128),      # the DyNeRF shape
    (1, 250),      # nb = 32: the one-workgroup brick kernel at its 64 KiB of LDS
    (1, 257),      # nb = 33: the first size on the global-memory rounds
    (2, 264),      # global-memory rounds with two levels
]

SINGLE_CELLS = ["corner%d" % k for k in range(8)] + ["centre"]
PATTERNS = ["empty", "full"] + SINGLE_CELLS + ["random", "last_brick", "empty_level"]


def single_cell(res, name):
    """The occupied cell of a single-cell pattern."""
    if name == "centre":
        return (res // 2,) * 3
    k = int(name[len("corner"):])
    return tuple((res - 1) if (k >> a) & 1 else 0 for a in range(3))


def cases():
    """Every (levels, res, pattern).  "empty_level" needs an empty level BETWEEN occupied ones, so three levels: with
    fewer it cannot be built and is left to the shapes that have them ((3, 24) and (4, 128))."""
    return [(m, res, p) for m, res in SHAPES for p in PATTERNS if p != "empty_level" or m >= 3]


def make_pattern(m, res, name):
    """binaries [m, res, res, res] uint8 of a named pattern, the same on every call."""
    rng = np.random.default_rng(1000 * res + m)
    b = np.zeros((m, res, res, res), np.uint8)
    if name == "empty":
        pass
    elif name == "full":
        b[:] = 1
    elif name in SINGLE_CELLS:
        b[(slice(None),) + single_cell(res, name)] = 1
    elif name == "random":                                          # 0.2 %, at least one cell per level
        b[:] = rng.uniform(size=b.shape) < 0.002
        for lvl in range(m):
            b[(lvl,) + tuple(rng.integers(0, res, size=3))] = 1
    elif name == "last_brick":                                      # per axis: cells whose coordinate on that axis lies in
        first = (-(-res // BRICK) - 1) * BRICK                       # the last (possibly partial) brick, the others anywhere
        for lvl in range(m):
            for ax in range(3):
                for _ in range(3):
                    c = rng.integers(0, res, size=3)
                    c[ax] = rng.integers(first, res)
                    b[(lvl,) + tuple(c)] = 1
    elif name == "empty_level":                                     # level 1 empty, its neighbours sparsely occupied
        b[:] = rng.uniform(size=b.shape) < 0.002
        for lvl in range(m):
            b[(lvl,) + tuple(rng.integers(0, res, size=3))] = 1
        b[1] = 0
    else:
        raise KeyError(name)
    return b


def accel_regions(accel, m, res):
    """The two field regions of an accel buffer (1-D uint8): [bdist m*nb^3][scratch m*nb^3], padded to 256 bytes, then
    [cdist m*res^3][scratch].  Returns (bdist [m,nb,nb,nb], cdist [m,res,res,res]); scratch and padding are left out."""
    nb = -(-res // BRICK)
    off = (2 * m * nb ** 3 + 255) // 256 * 256
    assert accel.ndim == 1 and accel.dtype == np.uint8 and accel.size == off + 2 * m * res ** 3
    return accel[:m * nb ** 3].reshape(m, nb, nb, nb), accel[off:off + m * res ** 3].reshape(m, res, res, res)


def check_fields(bdist, cdist, binaries, pattern):
    """The assertions on a built pair of fields that hold for any builder (host twin or device): bdist is the
    reference; cdist is the reference wherever that is <= CAP and >= CAP + 1 elsewhere; cdist never exceeds the true
    distance -- closed form for the single-cell patterns, pairwise brute force for res <= 40."""
    m, res = binaries.shape[0], binaries.shape[1]
    want_b, want_c = chebyshev_fields(binaries)
    assert bdist.shape == want_b.shape and cdist.shape == want_c.shape
    assert np.array_equal(bdist, want_b), ("bdist", int((bdist != want_b).sum()))
    near = want_c <= CAP
    assert np.array_equal(cdist[near], want_c[near]), ("cdist within the cap", int((cdist[near] != want_c[near]).sum()))
    assert (cdist[~near] >= CAP + 1).all(), "cdist beyond the cap must stay a bound >= CAP + 1"
    if pattern in SINGLE_CELLS:
        true = single_cell_distance(res, single_cell(res, pattern))
        assert (cdist <= true[None]).all(), "cdist above the closed-form distance"
    if res <= 40:
        for lvl in range(m):
            true = brute_force_distance(binaries[lvl])
            assert (cdist[lvl] <= true).all(), ("cdist above the brute-force distance", lvl)
            assert np.array_equal(np.minimum(true, CAP + 1), want_c[lvl]), ("reference against brute force", lvl)
