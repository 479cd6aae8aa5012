"""GPU suite: the volume export (ced_nerf_amd/export.py on csrc/bake.hip and ced_field_rgb_bcast) against the composition of
the public calls it replaces -- voxel_centers -> query_density -> torch.nonzero -> expanded _query_rgb.  Every comparison
is torch.equal: the kernels are deterministic and the export changes no row's arithmetic.

Fields: synthetic.init_field_params("trained"), log2_hashmap_size 15, hash_max_res 256.  Grids: reso 12 (1 728 cells: a
partial last wave and workgroup) and reso 20 (8 000 cells: eight compaction workgroups of 1 024, the last one partial);
the compaction alone also at 70 001 and 1 200 003 rows, where the scan of the workgroup counts spans several waves and
several entries per thread."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
AABB = (-1.5, -1.5, -1.5, 1.5, 1.5, 1.5)
FLAT = (-1.5, -1.0, -0.5, 1.5, 1.0, 0.5)                            # non-cubic: most of its bounding cube lies outside
STEP = 1.0 / 256
MODES = ("f32", "f16", "f16x2", "f32+h16x2")
FLAGS = [(False, 0), (True, 0), (False, 2), (True, 2)]              # (use_div_offsets, time_mode)
CASES = [(12, 1, True), (12, 3, False), (20, 3, True), (20, 1, False)]          # (reso, D, apply_act)
KEYS = ("index", "xyz", "sigma", "embedding")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _params(div, tm, aabb=AABB):
    from ced_nerf_amd import synthetic as S
    return S.init_field_params(list(aabb), STEP, hash_max_res=256, log2_hashmap_size=15, use_div_offsets=div,
                               use_time_embedding=tm != 0, use_time_attenuation=tm == 2, regime="trained")


@functools.lru_cache(maxsize=None)
def _field(div, tm, mode, aabb=AABB):
    from ced_nerf_amd.model import DNGPradianceField
    return DNGPradianceField.from_params(_params(div, tm, aabb), DEV, mlp_precision=mode).eval()


@functools.lru_cache(maxsize=None)
def _dirs(d):
    v = np.random.default_rng(11).normal(size=(3, 3)).astype(np.float32) * np.float32(2.5)         # unnormalised
    return T(v[:d])


def _cube(aabb):
    a = torch.tensor(aabb, dtype=torch.float32)
    return ((a[3:] + a[:3]) / 2.0).tolist(), ((a[3:] - a[:3]) / 2.0).max().item()


@functools.lru_cache(maxsize=None)
def _density(div, tm, mode, reso, t, aabb=AABB):
    """query_density on every cell centre, once per (field, grid, time): (sigma [reso^3], embedding [reso^3, 15])"""
    from ced_nerf_amd.export import voxel_centers
    f = _field(div, tm, mode, aabb)
    center, radius = _cube(aabb)
    P = voxel_centers(reso, center, radius, DEV)
    res = f.query_density(P, torch.full((P.shape[0], 1), t, device=DEV), return_feat=True)
    return P, res["density"][:, 0].contiguous(), res["base_mlp_out"]


def _composition(f, P, sig, emb, cand, thresh, dirs, apply_act):
    """the hand composition of the calls that exist without the export, on the candidate cells `cand` (ascending)"""
    keep = cand[torch.nonzero(sig[cand] >= thresh)[:, 0]]
    out = dict(index=keep, xyz=P[keep], sigma=sig[keep], embedding=emb[keep])
    if dirs is not None:
        m, d = keep.shape[0], dirs.shape[0]
        out["rgb"] = f._query_rgb(dirs[None].expand(m, d, 3), emb[keep][:, None].expand(m, d, 15), apply_act)
    return out


def _assert_same(got, want, what=""):
    for k in KEYS + (("rgb",) if "rgb" in want else ()):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert torch.equal(got[k], want[k]), (what, k)
    assert ("rgb" in got) == ("rgb" in want)


def _median(v):
    return float(v.median())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("div,tm", FLAGS)
def test_bake_volume_is_the_composition(div, tm, mode):
    """index == nonzero(sigma >= thresh) with thresh the median density (both outcomes occur); xyz, sigma, embedding, rgb
    equal the composition's, for D = 1 and D = 3 (rows that straddle the head kernel's tiles), the sigmoid on and off."""
    from ced_nerf_amd.export import bake_volume
    f = _field(div, tm, mode)
    for reso, d, act in CASES:
        t = 0.37
        P, sig, emb = _density(div, tm, mode, reso, t)
        n = reso ** 3
        thresh = _median(sig)
        vol = bake_volume(f, t, reso=reso, sigma_thresh=thresh, dirs=_dirs(d), apply_act=act)
        m = vol["index"].shape[0]
        print(f"[{mode} div={div} tm={tm}] reso {reso} D {d}: thresh {thresh:.4g}, M = {m} of {n}")
        assert 0 < m < n
        want = _composition(f, P, sig, emb, torch.arange(n, device=DEV), thresh, _dirs(d), act)
        _assert_same(vol, want, (reso, d, act))
        assert vol["rgb"].shape == (m, d, 3) and vol["index"].dtype == torch.int64
        assert vol["reso"] == reso and vol["t"] == t and vol["radius"] == 1.5 and vol["center"] == [0.0, 0.0, 0.0]
        if not act:
            assert bool((vol["rgb"] < 0).any() | (vol["rgb"] > 1).any())


def _mask_restatement(P, binaries, aabbs):
    """a cell is a candidate iff some level's box contains its centre (faces included) and, in the smallest such level,
    the grid cell clamp(int(((p - min) / extent) * R), 0, R - 1) is set"""
    res = binaries.shape[1]
    keep = torch.zeros(P.shape[0], dtype=torch.bool, device=P.device)
    decided = torch.zeros_like(keep)
    for lvl in range(binaries.shape[0]):
        lo, hi = aabbs[lvl, :3], aabbs[lvl, 3:]
        inside = ((P >= lo) & (P <= hi)).all(-1)
        cell = (((P - lo) / (hi - lo)) * float(res)).to(torch.int32).clamp(0, res - 1).long()
        occ = binaries[lvl][cell[:, 0], cell[:, 1], cell[:, 2]]
        keep |= inside & ~decided & occ
        decided |= inside
    return keep


def _estimator(roi, p_set, seed):
    """2 levels, resolution 16, a seeded random pattern with level 0's first octant empty"""
    from ced_nerf_amd.nerfacc_api import OccGridEstimator
    est = OccGridEstimator(list(roi), 16, 2).to(DEV)
    pattern = np.random.default_rng(seed).uniform(size=(2, 16, 16, 16)) < np.asarray(p_set).reshape(2, 1, 1, 1)
    pattern[0, :8, :8, :8] = False
    est.set_binaries(T(pattern))
    return est


@pytest.mark.parametrize("reso", [12, 20, 48])                # 48: 110 592 cells, 108 workgroup counts
def test_candidates_follow_the_smallest_containing_level(reso):
    """Level 0 covers the inner eighth of the cube, level 1 all of it: the candidates (bake with a threshold every
    density passes) are the restatement's cells, some but not all, in ascending order."""
    from ced_nerf_amd import ops
    from ced_nerf_amd.export import voxel_centers
    est = _estimator((-0.75, -0.75, -0.75, 0.75, 0.75, 0.75), (0.6, 0.4), 5)
    P = voxel_centers(reso, [0.0, 0.0, 0.0], 1.5, DEV)
    want = torch.nonzero(_mask_restatement(P, est.binaries, est.aabbs))[:, 0]
    assert 0 < want.shape[0] < reso ** 3
    inner = (P.abs() <= 0.75).all(-1)
    assert bool(inner[want].any()) and bool((~inner)[want].any())                 # both levels decide somewhere
    assert not bool(((P < 0).all(-1) & inner)[want].any())                        # the empty octant of level 0
    with torch.cuda.device(0):
        index, xyz = ops.bake_candidates(reso, [0.0, 0.0, 0.0], 1.5, 0, reso ** 3, DEV, est.binaries, est.aabbs)
        assert index.dtype == torch.int64 and torch.equal(index, want) and torch.equal(xyz, P[want])
        # without a grid: every cell, the centres voxel_centers states
        index, xyz = ops.bake_candidates(reso, [0.0, 0.0, 0.0], 1.5, 0, reso ** 3, DEV)
        assert torch.equal(index, torch.arange(reso ** 3, device=DEV)) and torch.equal(xyz, P)
        # a slab in the middle, boundaries off every workgroup's
        first, count = 1000, reso ** 3 - 1531
        index, xyz = ops.bake_candidates(reso, [0.0, 0.0, 0.0], 1.5, first, count, DEV, est.binaries, est.aabbs)
        sub = want[(want >= first) & (want < first + count)]
        assert torch.equal(index, sub) and torch.equal(xyz, P[sub])


@pytest.mark.parametrize("mode", MODES)
def test_bake_of_a_flat_box_with_an_occupancy_grid(mode):
    """The field's box is 3 x 2 x 1: most of its bounding cube lies outside it, where the density is exactly 0.  The
    estimator's level 0 is that box, level 1 (twice the box) reaches outside it, so cells of density 0 are candidates
    and the median threshold drops them."""
    from ced_nerf_amd.export import bake_volume
    f = _field(True, 2, mode, FLAT)
    est = _estimator(FLAT, (0.9, 0.2), 9)
    for reso, d, act in ((12, 3, False), (20, 3, True)):
        t = 0.5
        P, sig, emb = _density(True, 2, mode, reso, t, FLAT)
        cand = torch.nonzero(_mask_restatement(P, est.binaries, est.aabbs))[:, 0]
        assert 0 < cand.shape[0] < reso ** 3
        assert bool((sig[cand] == 0).any()) and bool((sig == 0).sum() > reso ** 3 // 2)
        thresh = _median(sig[cand])
        vol = bake_volume(f, torch.tensor([t], device=DEV), reso=reso, sigma_thresh=thresh, dirs=_dirs(d), estimator=est,
                          apply_act=act)
        m = vol["index"].shape[0]
        print(f"[{mode}] flat box, reso {reso}: {cand.shape[0]} candidates, thresh {thresh:.4g}, M = {m}")
        assert thresh > 0 and 0 < m < cand.shape[0]
        _assert_same(vol, _composition(f, P, sig, emb, cand, thresh, _dirs(d), act), reso)
        assert vol["radius"] == 1.5 and bool((vol["sigma"] > 0).all())


def test_a_threshold_above_every_density_gives_empty_outputs():
    from ced_nerf_amd.export import bake_volume
    f = _field(True, 2, "f16x2")
    _, sig, _ = _density(True, 2, "f16x2", 12, 0.0)
    for dirs in (None, _dirs(3)):
        vol = bake_volume(f, 0.0, reso=12, sigma_thresh=float(sig.max()) * 2.0 + 1.0, dirs=dirs)
        assert vol["index"].shape == (0,) and vol["index"].dtype == torch.int64
        assert vol["xyz"].shape == (0, 3) and vol["sigma"].shape == (0,) and vol["embedding"].shape == (0, 15)
        assert all(vol[k].dtype == torch.float32 and vol[k].is_cuda for k in ("xyz", "sigma", "embedding"))
        if dirs is None:
            assert "rgb" not in vol
        else:
            assert vol["rgb"].shape == (0, 3, 3) and vol["rgb"].dtype == torch.float32
    # NaN does not pass, whatever the threshold
    from ced_nerf_amd import ops
    n = 300
    s = torch.linspace(-1.0, 1.0, n, device=DEV)
    s[::7] = float("nan")
    idx = torch.arange(n, device=DEV)
    xyz, emb = torch.rand(n, 3, device=DEV), torch.rand(n, 15, device=DEV)
    with torch.cuda.device(0):
        got = ops.bake_select(idx, xyz, s, emb, -2.0)
    keep = torch.nonzero(~torch.isnan(s))[:, 0]
    assert torch.equal(got[0], keep) and torch.equal(got[1], xyz[keep]) and torch.equal(got[3], emb[keep])


@pytest.mark.parametrize("with_grid", [False, True])
def test_slabs_do_not_change_the_result(with_grid):
    """max_cells_per_launch = 1000 at reso 12 (two slabs; 1000 is no multiple of a workgroup's 1 024 cells) and 577 (three
    slabs) give the single-slab outputs."""
    from ced_nerf_amd.export import bake_volume
    f = _field(True, 2, "f32")
    est = _estimator((-0.75, -0.75, -0.75, 0.75, 0.75, 0.75), (0.6, 0.4), 5) if with_grid else None
    _, sig, _ = _density(True, 2, "f32", 12, 0.25)
    kw = dict(reso=12, sigma_thresh=_median(sig), dirs=_dirs(3), estimator=est)
    one = bake_volume(f, 0.25, **kw)
    assert 0 < one["index"].shape[0] < 12 ** 3
    for cells in (1000, 577):
        _assert_same(bake_volume(f, 0.25, max_cells_per_launch=cells, **kw), one, cells)


def test_bake_sequence_is_bake_volume_per_time():
    from ced_nerf_amd.export import bake_sequence, bake_volume
    f = _field(True, 2, "f16x2")
    est = _estimator((-0.75, -0.75, -0.75, 0.75, 0.75, 0.75), (0.6, 0.4), 5)
    _, sig, _ = _density(True, 2, "f16x2", 12, 0.37)
    kw = dict(reso=12, sigma_thresh=_median(sig), dirs=_dirs(3), estimator=est, apply_act=True)
    times = [0, 0.37, 1]
    seq = bake_sequence(f, times, **kw)
    assert len(seq) == 3 and [v["t"] for v in seq] == [0.0, 0.37, 1.0]
    for t, vol in zip(times, seq):
        _assert_same(vol, bake_volume(f, t, **kw), t)
    assert not torch.equal(seq[0]["sigma"][:50], seq[2]["sigma"][:50])            # the field does move


@pytest.mark.parametrize("mode", MODES)
def test_nerfvis_eval_fn_is_the_reference_closure(mode):
    """x [N,1,3], dirs [1,D,3] -> rgb [N,D,3] before the activation and density [N,1], as the composition vis.py:24-34
    writes out."""
    from ced_nerf_amd.export import nerfvis_eval_fn
    f = _field(True, 2, mode)
    rng = np.random.default_rng(2)
    n, d = 1031, 5
    x = T(rng.uniform(-1.6, 1.6, size=(n, 1, 3)).astype(np.float32))
    dirs = T(rng.normal(size=(1, d, 3)).astype(np.float32))
    for t in (0.0, 0.6):
        rgb, density = nerfvis_eval_fn(f, t)(x, dirs)
        tt = torch.full((n, 1, 1), t, device=DEV)
        res = f.query_density(x, tt, return_feat=True)
        want = f._query_rgb(dirs.expand(n, -1, -1), res["base_mlp_out"].expand(-1, d, -1), apply_act=False)
        assert rgb.shape == (n, d, 3) and torch.equal(rgb, want)
        assert density.shape == (n, 1) and torch.equal(density, res["density"].view(n, 1))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tm", [0, 2])
def test_field_rgb_is_unchanged_and_the_broadcast_entry_agrees(tm, mode):
    """On test_gpu_deformation's inputs: _query_rgb(dirs, geo) is still the fused forward's rgb at every n, and the
    broadcast entry gives the same rows -- D = 1 (one direction under every embedding) and M = 1 (one embedding under
    every direction) against _query_rgb on the expanded inputs, with and without the sigmoid."""
    from ced_nerf_amd import ops
    rng = np.random.default_rng(7)
    sizes = (0, 1, 31, 32, 33, 257, 4099)
    n = max(sizes)
    pos = rng.uniform(-1.6, 1.6, size=(n, 3)).astype(np.float32)
    t = rng.uniform(0.0, 1.0, size=(n,)).astype(np.float32)
    dirs = (rng.normal(size=(n, 3)) * rng.uniform(0.1, 5.0, size=(n, 1))).astype(np.float32)
    dirs[:6] = [[1, 0, 0], [0, 0, -3], [1, 1e-7, 0], [1e-3, 1, 1e-6], [0, -1e-4, 0], [-2, 2e-7, -2e-7]]
    f = _field(True, tm, mode)
    desc = f._descriptor()
    for n in sizes:
        Dn = T(dirs[:n])
        rgb, res = f(T(pos[:n]), T(t[:n, None]), Dn)
        geo = res["base_mlp_out"]
        assert torch.equal(f._query_rgb(Dn, geo), rgb), n
        for act in (True, False):
            one_dir = ops.field_rgb_bcast(desc, T(dirs[3:4]), geo, act)
            assert one_dir.shape == (n, 1, 3)
            assert torch.equal(one_dir[:, 0], f._query_rgb(T(dirs[3:4]).expand(n, 3), geo, act)), (n, act)
            if n:
                one_emb = ops.field_rgb_bcast(desc, Dn, geo[7 % n:7 % n + 1].contiguous(), act)
                assert one_emb.shape == (1, n, 3)
                assert torch.equal(one_emb[0], f._query_rgb(Dn, geo[7 % n:7 % n + 1].expand(n, 15), act)), (n, act)


def test_cli_writes_volumes_of_a_saved_checkpoint(tmp_path):
    """A model.pth in the form trainer.fit saves (the two modules' state dicts) -> volume_%04d.npz / .ply per time, equal
    to bake_volume on the modules the file was saved from."""
    from ced_nerf_amd import export as E, trainer
    cfg = trainer.resolve_config("dnerf", None, log2_hashmap_size=14)
    flags = dict(use_div_offsets=True, use_time_embedding=True)
    field, est = trainer.build_modules(cfg, torch.device(DEV), **flags)
    pattern = np.random.default_rng(4).uniform(size=tuple(est.binaries.shape)) < 0.5
    est.set_binaries(T(pattern))
    path = str(tmp_path / "model.pth")
    torch.save({"radiance_field": field.state_dict(), "occupancy_grid": est.state_dict()}, path)
    out = tmp_path / "vols"
    argv = ["--load_model", path, "--preset", "dnerf", "--log2_hashmap_size", "14", "-df", "-te", "--times", "0,0.5",
            "--reso", "16", "--sigma_thresh", "1e-6", "--n_dirs", "4", "--device", DEV, "--out", str(out)]
    assert E.main(argv) == 0
    dirs = T(E.fibonacci_dirs(4))
    for i, t in enumerate((0.0, 0.5)):
        want = E.bake_volume(field, t, reso=16, sigma_thresh=1e-6, dirs=dirs, estimator=est)
        m = want["index"].shape[0]
        assert 0 < m < 16 ** 3
        with np.load(out / f"volume_{i:04d}.npz") as z:
            for k in KEYS + ("rgb",):
                assert np.array_equal(z[k], want[k].cpu().numpy()), k
            assert int(z["reso"]) == 16 and float(z["t"]) == t
        raw = (out / f"volume_{i:04d}.ply").read_bytes()
        assert raw.startswith(E.ply_header(m)) and len(raw) == len(E.ply_header(m)) + 19 * m


@pytest.mark.parametrize("n", [70_001, 1_200_003])
def test_select_keeps_order_across_many_workgroups(n):
    """70 001 rows are 69 workgroup counts (the scan's second wave takes part), 1 200 003 rows 1 172 (two entries per scan
    thread, the default reso 128's regime): the kept rows are torch.nonzero's, in order, with what belongs to them."""
    from ced_nerf_amd import ops
    g = torch.Generator(device=DEV).manual_seed(n)
    sigma = torch.rand(n, device=DEV, generator=g)
    sigma[::1013] = float("nan")
    index = torch.arange(n, device=DEV) * 3 + 1
    xyz = torch.rand(n, 3, device=DEV, generator=g)
    emb = torch.rand(n, 15, device=DEV, generator=g)
    with torch.cuda.device(0):
        got = ops.bake_select(index, xyz, sigma, emb, 0.7)
    keep = torch.nonzero(sigma >= 0.7)[:, 0]
    assert 0 < keep.shape[0] < n
    for a, b in zip(got, (index[keep], xyz[keep], sigma[keep], emb[keep])):
        assert a.shape == b.shape and torch.equal(a, b)
