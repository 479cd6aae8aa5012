"""GPU suite: the inverse of the warp (csrc/field_move.hip: ced_field_move_inverse, ced_field_track) and what stands on it --
DNGPradianceField.query_move_inverse / track_points, export.track_mesh / extract_mesh_tracked.

The reference of the bit-identity tests is the composition the fused kernel replaces: a Python loop of
`field.query_move` with the fp32 lines of include/cednerf_hip.h and the per-row freeze in torch.  The reference of the
accuracy tests is a float64 restatement of the motion network and a float64 solve of the same equation.

Fields: synthetic.init_field_params("trained"), log2_hashmap_size 15, hash_max_res 256, aabb [-1.5, 1.5]^3, moving step
1/32 (the map x -> c - move(x, t) is a contraction on every row: the float32 iteration converges in 3 .. 12 evaluations)
and 1/8 (it is not, on a few per cent of the rows).  Positions are default_rng(7).uniform(-1.6, 1.6), t in [0, 1]."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
AABB = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
STEP = 1.0 / 32
SIZES = (0, 1, 31, 32, 33, 257, 4099)
MODES = ("f32", "f16", "f16x2", "f32+h16x2")
FLAGS = [(False, 0), (True, 2)]                                     # (use_div_offsets, time_mode)
# The issue's bound: a numpy float32 model of the iteration differs from the float64 solve of x + move(x, t) = c by a few
# 1e-7 on these inputs (moving step 1/32, K = 32, tol = 1e-6; stated there as 4.1e-7, restated in test_it_inverts_the_warp
# as 3.4e-7 / 5.5e-7 without / with the fine offsets).  Four times 4.1e-7, for the device's sin and the ulp (1.2e-7) at
# |x| ~ 1.6 -- not derived from the kernel under test.
MARGIN = 4 * 4.1e-7


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _params(div, tm, step=STEP, table="f32"):
    from ced_nerf_amd import synthetic as S
    return S.init_field_params(list(AABB), step, hash_max_res=256, log2_hashmap_size=15, use_div_offsets=div,
                               use_time_embedding=tm != 0, use_time_attenuation=tm == 2, regime="trained",
                               table_dtype=np.float16 if table == "f16" else np.float32, temporal_hash=table == "temporal")


@functools.lru_cache(maxsize=None)
def _field(div, tm, mode, step=STEP, table="f32"):
    from ced_nerf_amd.model import DNGPradianceField
    return DNGPradianceField.from_params(_params(div, tm, step, table), DEV, mlp_precision=mode).eval()


@functools.lru_cache(maxsize=None)
def _inputs():
    rng = np.random.default_rng(7)
    n = max(SIZES)
    pos = rng.uniform(-1.6, 1.6, size=(n, 3)).astype(np.float32)
    t = rng.uniform(0.0, 1.0, size=(n,)).astype(np.float32)
    return T(pos), T(t)


def _composition(f, c, t, K, tol, init=None):
    """The iteration of include/cednerf_hip.h on today's pieces: K launches of query_move, the fp32 lines and the per-row
    freeze in torch.  c [n,3], t [n] -> (x, step, evals)."""
    n = c.shape[0]
    x = (c if init is None else init).clone()
    step = torch.full((n,), float("inf"), device=c.device)
    evals = torch.zeros((n,), device=c.device, dtype=torch.int32)
    active = torch.ones((n,), device=c.device, dtype=torch.bool)
    for _ in range(K):
        m = f.query_move(x, t)[1]
        x_new = c - m
        d = (x_new - x).abs()
        s = torch.fmax(torch.fmax(d[:, 0], d[:, 1]), d[:, 2])
        x = torch.where(active[:, None], x_new, x)
        step = torch.where(active, s, step)
        evals = evals + active.to(torch.int32)
        active = active & ~(s <= tol)
        if not bool(active.any()):
            break
    return x, step, evals


def _assert_same(got, want, what):
    for g, w, name in zip(got, want, ("x", "step", "evals")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert torch.equal(g, w), (what, name, int((g != w).sum()))


def _check_is_the_composition(f, what):
    pos, t = _inputs()
    c = f.query_move(pos, t)[0]                                      # canonical targets; the start is the default (c)
    several = False
    for K in (1, 4, 32):
        for tol in (0.0, 1e-6):
            want = _composition(f, c, t, K, tol)
            for n in SIZES:
                got = f.query_move_inverse(c[:n], t[:n], max_iters=K, tol=tol)
                assert got[0].shape == (n, 3) and got[1].shape == (n,) and got[2].dtype == torch.int32
                _assert_same(got, tuple(w[:n] for w in want), (what, K, tol, n))
            ev = want[2]
            assert int(ev.min()) >= 1 and int(ev.max()) <= K
            # the same with a start of its own: the positions the targets were computed from
            want = _composition(f, c, t, K, tol, init=pos)
            for n in SIZES:
                got = f.query_move_inverse(c[:n], t[:n], max_iters=K, tol=tol, init=pos[:n])
                _assert_same(got, tuple(w[:n] for w in want), (what, K, tol, n, "init"))
            several = several or (tol > 0 and K == 32 and len(torch.unique(ev)) >= 4)
    assert several, "the rows of a tile must stop at different rounds for the freeze to be exercised"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("div,tm", FLAGS)
def test_inverse_is_the_composition_bit_for_bit(div, tm, mode):
    """query_move_inverse == the Python loop of query_move: x, step and evals with torch.equal, for K in 1, 4, 32, tol in
    0, 1e-6 and every n of SIZES (one row, a wave tile of 32 +- 1, several workgroups with a ragged tail), started at the
    target (the default) and at an `init` of its own."""
    _check_is_the_composition(_field(div, tm, mode), (div, tm, mode))


@pytest.mark.parametrize("mode,table", [("f16x2", "f16"), ("f16x2", "temporal"), ("f16", "temporal"), ("f32", "f16")])
def test_inverse_is_the_composition_on_the_other_tables(mode, table):
    """The table's kind selects the packed blob's layout: f16x2 has the K = 32 placements on an fp16 table and the pair
    form on a temporal one -- both of the fixed-point kernel's f16x2 variants are hit."""
    _check_is_the_composition(_field(True, 0, mode, STEP, table), (mode, table))


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
@pytest.mark.parametrize("use_init", [False, True])
def test_broadcast_equals_explicit_rows(mode, use_init):
    """ops.field_track(c [P], times [T]) == ops.field_move_inverse on the expanded rows r = k * P + p."""
    from ced_nerf_amd import ops
    f = _field(True, 2, mode)
    pos, t = _inputs()
    d = f._descriptor()
    for P in (1, 33, 257):
        c = f.query_move(pos[:P], t[:P])[0]
        init = pos[:P].contiguous() if use_init else None
        for n_t in (1, 3):
            times = T(np.asarray([0.8, 0.1, 0.45][:n_t], np.float32))
            x, step, evals = ops.field_track(d, c, times, init, max_iters=32, tol=1e-6)
            assert x.shape == (n_t, P, 3) and step.shape == (n_t, P) and evals.shape == (n_t, P)
            want = ops.field_move_inverse(d, c.repeat(n_t, 1), times.repeat_interleave(P),
                                          None if init is None else init.repeat(n_t, 1), max_iters=32, tol=1e-6)
            _assert_same((x.view(-1, 3), step.view(-1), evals.view(-1)), want, (P, n_t))
            if n_t == 3 and P > 1:
                assert not torch.equal(x[0], x[1])


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
def test_a_row_does_not_depend_on_its_tile(mode):
    """Eight rows that stop at eight different rounds (with the fine offsets a row takes 4 .. 12 evaluations): each one's x,
    step, evals at n = 4099 (inside full tiles, beside rows that go on after it has stopped) are those of the row solved
    alone."""
    f = _field(True, 2, mode)
    pos, t = _inputs()
    c = f.query_move(pos, t)[0]
    x, step, evals = f.query_move_inverse(c, t, max_iters=32, tol=1e-6)
    ev = N(evals)
    values = np.unique(ev)
    assert len(values) >= 8, values
    rows = [int(np.flatnonzero(ev == v)[0]) for v in values[:8]]
    assert len({int(ev[r]) for r in rows}) == 8
    for r in rows:
        alone = f.query_move_inverse(c[r:r + 1], t[r:r + 1], max_iters=32, tol=1e-6)
        _assert_same(alone, (x[r:r + 1], step[r:r + 1], evals[r:r + 1]), (r, int(ev[r])))


# ---- float64 -----------------------------------------------------------------------------------------------------------
def _move_model(params, x, t, dtype=np.float64):
    """query_move's `move` in numpy, after tests/test_gpu_deformation.py::_move_float64"""
    x4 = np.concatenate([x, t[:, None]], -1).astype(dtype)
    enc = []
    for d in range(4):
        for k in range(4):
            ang = dtype((2 ** k) * math.pi) * x4[:, d]
            enc += [np.sin(ang), np.sin(ang + dtype(0.5 * math.pi))]
    h = np.stack(enc, -1)
    ws = [np.asarray(w, dtype) for w in params["xyz_wrap"]]
    for i, w in enumerate(ws):
        h = h @ w.T
        if i < len(ws) - 1:
            h = np.maximum(h, 0)
    out = h[:, :3] + np.tanh(h[:, 3:]) if params["use_div_offsets"] else h
    return out * dtype(np.float32(params["moving_step"]))


def _solve_float64(params, c, t, rounds=400):
    """the solution of x + move(x, t) = c in float64, iterated to a standstill; rows that do not get there are NaN"""
    c = c.astype(np.float64)
    x = c.copy()
    for _ in range(rounds):
        x_new = c - _move_model(params, x, t)
        step = np.abs(x_new - x).max(-1)
        x = x_new
        if step.max() <= 1e-14:
            break
    x[step > 1e-12] = np.nan
    return x


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
@pytest.mark.parametrize("div,tm", FLAGS)
def test_it_inverts_the_warp(div, tm, mode):
    """Moving step 1/32, K = 32, tol = 1e-6; every row must converge.  With c = query_move(x, t)[0]:
    the inverse started at c returns x; positions + move(positions, t) is c; track_points(x, t_src, [t_src]) returns x; and
    the positions are the float64 solve's -- all within MARGIN = 4 * 4.1e-7 = 1.64e-6.
    Measured on an MI355X, max over the 4099 rows, the same for f32 and f16x2 to the digits shown: |x - float64 solve|
    3.6e-7 (fine offsets off) / 5.5e-7 (on), where a numpy float32 model of the iteration gives 3.4e-7 / 5.5e-7 on the CPU;
    |x - x_src| 3.7e-7 / 4.8e-7; |x + move(x) - c| 2.7e-7 / 3.6e-7; track_points back at its source time 1.2e-7 (one ulp);
    3 .. 8 / 4 .. 12 evaluations per row."""
    params = _params(div, tm)
    f = _field(div, tm, mode)
    pos, t = _inputs()
    c = f.query_move(pos, t)[0]
    x, step, evals = f.query_move_inverse(c, t, max_iters=32, tol=1e-6)
    assert bool((step <= 1e-6).all()), int((~(step <= 1e-6)).sum())
    back = float((x - pos).abs().max())
    resid = float((x + f.query_move(x, t)[1] - c).abs().max())
    x64 = _solve_float64(params, N(c), N(t))
    assert np.isfinite(x64).all()
    vs64 = float(np.abs(N(x).astype(np.float64) - x64).max())
    # an independent float32 statement of the same iteration, against the same float64 solve
    c32, t32 = N(c), N(t)
    x32, live = c32.copy(), np.ones(len(c32), bool)
    for _ in range(32):
        x_new = c32 - _move_model(params, x32, t32, np.float32)
        s = np.abs(x_new - x32).max(-1)
        x32 = np.where(live[:, None], x_new, x32)
        live &= ~(s <= np.float32(1e-6))
    cpu = float(np.abs(x32.astype(np.float64) - x64).max())
    # one scalar source time through the public entry
    tr = f.track_points(pos, 0.37, [0.37], max_iters=32, tol=1e-6)
    assert tr["positions"].shape == (1, pos.shape[0], 3) and tr["converged"].dtype == torch.bool
    assert bool(tr["converged"].all()) and torch.equal(tr["converged"], tr["step"] <= 1e-6)
    assert torch.equal(tr["canonical"], f.query_move(pos, torch.full_like(t, 0.37))[0])
    track_back = float((tr["positions"][0] - pos).abs().max())
    print(f"inverse [{mode} div={div} tm={tm}]: evals {int(evals.min())}..{int(evals.max())}, max |x - x_src| = {back:.3e}, "
          f"max |x + move(x) - c| = {resid:.3e}, max |x - float64 solve| = {vs64:.3e} (numpy float32 model: {cpu:.3e}), "
          f"track_points max |x - x_src| = {track_back:.3e}; margin {MARGIN:.3e}")
    assert not live.any()
    assert back <= MARGIN and resid <= MARGIN and vs64 <= MARGIN and track_back <= MARGIN
    # several times at once: every frame satisfies the equation
    tr = f.track_points(pos[:257], t[:257], [0.0, 0.37, 1.0])
    assert bool(tr["converged"].all())
    for k, tk in enumerate((0.0, 0.37, 1.0)):
        p = tr["positions"][k]
        r = float((p + f.query_move(p, torch.full((257,), tk, device=DEV))[1] - tr["canonical"]).abs().max())
        assert r <= MARGIN, (tk, r)


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
@pytest.mark.parametrize("div,tm", FLAGS)
def test_non_convergence_is_reported(div, tm, mode):
    """Moving step 1/8: the same inputs hold rows on which the iteration never settles (a numpy float32 model on the CPU:
    2.8 % without, 9.3 % with the fine offsets by K = 32; an MI355X: 2.8 % / 9.4 %, the converged rows' largest residual
    1.0e-6 / 1.2e-6).  Both kinds are present, converged == (step <= tol), the unconverged rows ran exactly K evaluations,
    and the converged ones satisfy the equation within MARGIN."""
    K, tol = 32, 1e-6
    f = _field(div, tm, mode, 1.0 / 8)
    pos, t = _inputs()
    c = f.query_move(pos, t)[0]
    x, step, evals = f.query_move_inverse(c, t, max_iters=K, tol=tol)
    ok = step <= tol
    share = 1.0 - float(ok.float().mean())
    resid = (x + f.query_move(x, t)[1] - c).abs().max(-1).values
    print(f"step 1/8 [{mode} div={div} tm={tm}]: {100 * share:.2f} % of {len(ok)} rows not converged by K = {K}; converged rows: "
          f"max residual {float(resid[ok].max()):.3e}, evals {int(evals[ok].min())}..{int(evals[ok].max())}")
    assert bool(ok.any()) and bool((~ok).any())
    assert bool((evals[~ok] == K).all()) and bool((evals[ok] <= K).all()) and bool((step[~ok] > tol).all())
    assert float(resid[ok].max()) <= MARGIN
    tr = f.track_points(pos, t, [0.5], max_iters=K, tol=tol)
    assert torch.equal(tr["converged"], tr["step"] <= tol)
    assert bool(tr["converged"].any()) and bool((~tr["converged"]).any())
    assert bool((tr["evals"][~tr["converged"]] == K).all())


# ---- the tracked mesh --------------------------------------------------------------------------------------------------
def _read_ply(path):
    """a minimal reader of save_mesh_ply's two layouts"""
    head, _, body = path.read_bytes().partition(b"end_header\n")
    lines = head.decode("ascii").splitlines()
    v = int(next(l for l in lines if l.startswith("element vertex")).split()[-1])
    n_f = int(next(l for l in lines if l.startswith("element face")).split()[-1])
    normals = "property float nx" in lines
    fields = [("xyz", "<f4", 3)] + ([("normal", "<f4", 3)] if normals else []) + [("rgb", "u1", 3)]
    size = 27 if normals else 15
    assert np.dtype(fields).itemsize == size and len(body) == size * v + 13 * n_f
    vrec = np.frombuffer(body[:size * v], dtype=np.dtype(fields))
    frec = np.frombuffer(body[size * v:], dtype=np.dtype([("n", "u1"), ("ids", "<i4", 3)]))
    assert (frec["n"] == 3).all()
    return vrec, frec, normals


def test_tracked_mesh(tmp_path):
    """extract_mesh_tracked on the volume tests' field (reso 32, three times): the faces are extract_mesh(t_ref)'s, the
    vertices at t_ref are the reference vertices within MARGIN, two runs give equal bits, every frame satisfies the
    equation, and the files read back (PLY with and without normals)."""
    from ced_nerf_amd import export as E
    from test_gpu_export import _density, _field as export_field
    f = export_field(True, 2, "f32")
    t_ref, times = 0.37, [0.0, 0.37, 1.0]
    thresh = float(_density(True, 2, "f32", 32, t_ref)[1].median())
    kw = dict(reso=32, sigma_thresh=thresh, dirs="normal")
    ref = E.extract_mesh(f, t_ref, **kw)
    tracked = E.extract_mesh_tracked(f, t_ref, times, **kw)
    v, n_f = ref["vertices"].shape[0], ref["faces"].shape[0]
    assert v > 100 and n_f > 100
    for k in ("faces", "cube", "sigma", "embedding", "rgb", "normals"):
        assert torch.equal(tracked[k], ref[k]), k
    assert tracked["vertices_t"].shape == (3, v, 3) and tracked["converged"].shape == (3, v)
    assert tracked["step"].shape == (3, v) and tracked["evals"].dtype == torch.int32
    assert tracked["times"] == times and tracked["t_ref"] == t_ref and tracked["reso"] == 32
    assert bool(tracked["converged"].all()) and torch.equal(tracked["converged"], tracked["step"] <= 1e-6)
    at_ref = float((tracked["vertices_t"][1] - ref["vertices"]).abs().max())
    moved = float((tracked["vertices_t"][0] - tracked["vertices_t"][2]).abs().max())
    print(f"tracked mesh: V = {v}, F = {n_f}, max |vertices_t(t_ref) - vertices| = {at_ref:.3e}, moved {moved:.3e}")
    assert at_ref <= MARGIN and moved > 1e-4
    for k, tk in enumerate(times):
        p = tracked["vertices_t"][k]
        r = float((p + f.query_move(p, torch.full((v,), tk, device=DEV))[1] - tracked["canonical"]).abs().max())
        assert r <= MARGIN, (tk, r)
    again = E.track_mesh(f, ref, t_ref, times)
    for k in ("vertices_t", "converged", "step", "evals", "canonical"):
        assert torch.equal(again[k], tracked[k]), k
    # files
    E.save_tracked_npz(str(tmp_path / "tracked.npz"), tracked)
    with np.load(tmp_path / "tracked.npz") as z:
        for k in ("vertices_t", "converged", "step", "evals", "canonical", "faces", "normals", "rgb"):
            assert np.array_equal(z[k], N(tracked[k])), k
        assert np.array_equal(z["times"], np.asarray(times, np.float32)) and float(z["t_ref"]) == np.float32(t_ref)
    E.save_mesh_ply(str(tmp_path / "ref.ply"), ref)
    vrec, frec, normals = _read_ply(tmp_path / "ref.ply")
    assert normals and np.array_equal(vrec["xyz"], N(ref["vertices"])) and np.array_equal(vrec["normal"], N(ref["normals"]))
    assert np.array_equal(frec["ids"], N(ref["faces"]))
    for k in range(3):
        frame = E.tracked_frame(tracked, k)
        assert "normals" not in frame
        E.save_mesh_ply(str(tmp_path / f"tracked_{k}.ply"), frame)
        w, fr, normals = _read_ply(tmp_path / f"tracked_{k}.ply")
        assert not normals and np.array_equal(w["xyz"], N(tracked["vertices_t"][k])) and np.array_equal(fr["ids"], N(ref["faces"]))
        assert np.array_equal(w["rgb"], vrec["rgb"])
