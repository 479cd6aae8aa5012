"""GPU suite: the device-side copies of host-visible state follow every writer of their source.

The kernels are tested elsewhere; this module tests the Python layer that decides WHICH BYTES they read.
`DNGPradianceField._descriptor` keeps a packed weight blob and a descriptor (box, python scalars, table pointer) and
decides from `(data_ptr, _version)` keys whether they are still valid; `TrainableField` keeps the box as python floats,
an fp16 copy of the master table and a shared inference module.  A wrong decision faults nothing and trips no
tolerance: the kernel computes the bit-exact answer for the OLD state.

Every test: build the module, launch it once (every cache populated), apply a write, launch again.  The second result
must equal -- torch.equal, no tolerance -- that of a FRESH module built from `export_params()` of the written one, which
has never been launched and so has no cache to be wrong about; in one test per precision mode the fresh module is
itself anchored to the CPU oracle, bit for bit.  And every write must change the answer (asserted), so that a stale
cache cannot pass.  Inputs: a 2^14-entry table, n = 1031 samples (ragged against the 64-sample tile, some outside the
box), a 48 x 36 frame.

What the code BEFORE the fixes of this change did on these tests (run once on an MI355X; every failure a wrong value
on valid memory, 26 of the 75 cases):

  1. fp16-table `TrainableField` after `load_state_dict` (fourth finding) -- FAILED for f16_table and
     temporal_f16: `tf(pos, t, d)`, `forward_rays` and `shared_inference()` all evaluated the previous table ("stale
     after load_state_dict: 3093/3093 forward rgb values differ; 858/1031 forward sigma; 931/1031 forward_rays sigma;
     858/1031 shared density; 15465/15465 shared base_mlp_out").  `hash_table.copy_(other)` on the fp32 master failed
     the same way (856/1031 sigma), and so did a load into a deep copy.  The fp32 table passed.
  2. `w.data = other` on `DNGPradianceField`, the old tensor dropped first -- FAILED in all five packer cases: the
     allocator handed the freed block to the replacement (old address == new address in every case), the key
     `(data_ptr, _version)` was re-issued and the old blob was used (3093/3093 rgb, 861/1031 density, 15465/15465
     base_mlp_out values differ).  PASSED before: `w.copy_` / `w.mul_` under no_grad, `load_state_dict`, both
     checkpoint loaders, `w.data.mul_` + `weights_changed()`, `aabb.copy_`.  `aabb.data = other` FAILED like the weights
     (address reused; 976/1031 densities).
  3. `MOVING_STEP = 1/16` after a launch -- FAILED in all five cases, silently ignored (868/1031 densities differ from
     the fresh module's); `time_mode = 2` -- FAILED (856/1031); `use_div_offsets = False` on a six-row motion network
     -- FAILED: no exception, the old descriptor was used.
  4. `TrainableField._aabb6_key`: `aabb.copy_` PASSED (fused against the torch statements: rgb within 1.1e-6, sigma
     within 2e-5 relative); `aabb.data = other` FAILED (address reused; the fused warp kernel and the shared module
     kept the old box: 976/1031 forward sigma, 1008/1031 forward_rays sigma values differ from the fresh field's).
  5. `shared_inference()` built on the CPU, then `.to("cuda:0")` -- fp32 table: the launch after the move PASSED (the
     shared module still read the old CPU box, which held the same numbers) and the `aabb.copy_` that followed FAILED
     (3093/3093 shared rgb, 929/1031 shared density: the new buffer was never looked at); fp16 table: raised
     NotImplementedError "move the field to a GPU" although the field had been moved.
  6. `train_step` with fused Adam, with and without a GradScaler, fp32 and fp16 tables, f32 and f16x2, then
     `refresh_occupancy` -- PASSED in all eight cases: the explicit `sync_half_table()` / `weights_changed()` after the
     step do their job.  The hazard does not bite; the tests stay.
  Also PASSED before: set_mlp_precision round trips, every hash-table write (the table is read in place; its address
  was reused too, harmlessly), copy.deepcopy of the inference module, two frames with a `copy_` between them, two
  threads asking for the descriptor.
"""
import copy
import threading

import numpy as np
import pytest
import torch

from conftest import assert_bitexact

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BOX = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
MODES = ["f32", "f16", "f16x2", "f32+h16x2"]
# the four packers; f16x2 without a time encoding is the K=32 layout, with one the pair layout
PACKERS = [("f32", {}), ("f16", {}), ("f16x2", {}), ("f32+h16x2", {}), ("f16x2", dict(use_time_embedding=True))]
PACKER_IDS = ["f32", "f16", "f16x2-k32", "f32+h16x2", "f16x2-pair"]
TABLES = {"f32_table": {}, "f16_table": dict(table_dtype=np.float16),
          "temporal": dict(temporal_hash=True, use_time_embedding=True),
          "temporal_f16": dict(temporal_hash=True, use_time_embedding=True, table_dtype=np.float16)}
N = 1031


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def make_params(seed=42, **kw):
    from ced_nerf_amd import synthetic as S
    return S.init_field_params(BOX, 1.0 / 64, 1024, 14, regime="trained", seed=seed, **kw)


_INPUTS = {}


def inputs():
    """pos [N,3] (a few points outside the box), t [N,1] in [0,1], directions [N,3]; ray-packed samples of the same size."""
    if not _INPUTS:
        rng = np.random.default_rng(11)
        pos = rng.uniform(-1.6, 1.6, size=(N, 3)).astype(np.float32)
        pos[0] = [1.5, 0, 0]; pos[1] = [-1.5, -1.5, -1.5]
        t = rng.uniform(0, 1, size=(N, 1)).astype(np.float32); t[2] = 0; t[3] = 1
        d = rng.normal(size=(N, 3)).astype(np.float32)
        n_rays = 64
        ro = rng.uniform(-0.4, 0.4, size=(n_rays, 3)).astype(np.float32)
        rd = rng.normal(size=(n_rays, 3)); rd = (rd / np.linalg.norm(rd, axis=1, keepdims=True)).astype(np.float32)
        ri = np.sort(rng.integers(0, n_rays, size=N)).astype(np.int64)
        t0 = rng.uniform(0.0, 1.9, size=N).astype(np.float32)
        ts = rng.uniform(0, 1, size=(n_rays, 1)).astype(np.float32)
        _INPUTS.update(np=(pos, t, d), dev=(T(pos), T(t), T(d)),
                       rays=(T(ro), T(rd), T(ri), T(t0), T(t0) + 5e-3, T(ts)))
    return _INPUTS


NAMES = ("rgb", "density", "base_mlp_out", "query_density")


def outputs(f):
    """forward -> rgb, density, base_mlp_out; query_density (the density-only launch)."""
    pos, t, d = inputs()["dev"]
    rgb, res = f(pos, t, d)
    dens = f.query_density(pos, t)["density"]
    return rgb, res["density"], res["base_mlp_out"], dens


def describe(got, want, names=NAMES):
    return "; ".join(f"{int((g != w).sum())}/{g.numel()} {nm} values differ" for nm, g, w in zip(names, got, want)
                     if not torch.equal(g, w))


def assert_same(got, want, what, names=NAMES):
    assert len(got) == len(want)
    assert all(torch.equal(g, w) for g, w in zip(got, want)), f"stale after {what}: {describe(got, want, names)}"


def assert_changed(got, before, what, which=(0,), names=NAMES):
    """The write must move the answer, or the comparison with the fresh module proves nothing."""
    for i in which:
        assert not torch.equal(got[i], before[i]), f"{what} did not change {names[i]}: the test would pass on a stale cache"


def make_field(mode, seed=42, **kw):
    from ced_nerf_amd.model import DNGPradianceField
    return DNGPradianceField.from_params(make_params(seed, **kw), DEV, mlp_precision=mode).eval()


def fresh_of(f, mode=None):
    """A module with the written one's parameters that has never been launched: the reference."""
    from ced_nerf_amd.model import DNGPradianceField
    return DNGPradianceField.from_params(f.export_params(), DEV, mlp_precision=mode or f.mlp_precision).eval()


def check_write(f, write, what, which=(0, 1, 3)):
    before = outputs(f)
    write(f)
    got = outputs(f)
    assert_same(got, outputs(fresh_of(f)), what)
    assert_changed(got, before, what, which)
    return got


def replace_data(owner_tensor, make_host_values):
    """`p.data = other` in the order in which the caching allocator re-issues the address: the replacement's values
    are prepared on the host, the parameter lets go of its storage (no other reference exists), and only then is the
    replacement of equal size allocated on the same stream.  Returns (old address, new address)."""
    host = make_host_values(owner_tensor.detach().cpu())
    old = owner_tensor.data_ptr()
    torch.cuda.synchronize()
    owner_tensor.data = torch.empty(0, device=DEV)
    owner_tensor.data = host.to(DEV)
    new = owner_tensor.data_ptr()
    print(f"  .data replaced: old address {old:#x}, new {new:#x} ({'reused' if old == new else 'not reused'})")
    return old, new


# ---- DNGPradianceField: the MLP weights ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,kw", PACKERS, ids=PACKER_IDS)
def test_in_place_writes_to_a_weight_of_each_network(mode, kw):
    f = make_field(mode, **kw)
    donor = make_params(9, **kw)
    for net, which in (("xyz_wrap", (0, 1, 3)), ("mlp_base", (0, 1, 3)), ("mlp_head", (0,))):
        w = getattr(f, net)[0]
        last = getattr(f, net)[-1]

        def mul(_):
            with torch.no_grad():
                w.mul_(0.5)

        def cp(_):
            with torch.no_grad():
                last.copy_(T(donor[net][-1]))
        check_write(f, mul, f"{net}[0].mul_(0.5)", which)
        check_write(f, cp, f"{net}[-1].copy_(other)", which)


@pytest.mark.parametrize("mode,kw", PACKERS, ids=PACKER_IDS)
def test_load_state_dict_of_another_field(oracle, mode, kw):
    f = make_field(mode, **kw)
    other_params = make_params(9, **kw)
    from ced_nerf_amd.model import DNGPradianceField
    other = DNGPradianceField.from_params(other_params, DEV, mlp_precision=mode).eval()
    before = outputs(f)
    f.load_state_dict(other.state_dict())
    got = outputs(f)
    want = outputs(fresh_of(f))
    assert_same(got, want, "load_state_dict")
    assert_changed(got, before, "load_state_dict", (0, 1, 2, 3))
    # the anchor of the reference: the fresh module is the oracle's mode of the same name, bit for bit
    pos, t, d = inputs()["np"]
    o = oracle.OracleField(other_params, mlp_half=mode).forward(pos, t, d, want_geo=True)
    assert_bitexact(want[0].cpu().numpy(), o["rgb"], f"fresh {mode} rgb vs oracle")
    assert_bitexact(want[1].cpu().numpy()[:, 0], o["density"], f"fresh {mode} density vs oracle")
    assert_bitexact(want[2].cpu().numpy(), o["base_mlp_out"], f"fresh {mode} base_mlp_out vs oracle")
    assert_bitexact(want[3].cpu().numpy()[:, 0], o["density"], f"fresh {mode} query_density vs oracle")


@pytest.mark.parametrize("mode,kw", PACKERS, ids=PACKER_IDS)
def test_checkpoint_load_paths(mode, kw):
    from ced_nerf_amd import checkpoint as CK
    f = make_field(mode, **kw)
    second, third = make_field(mode, 9, **kw), make_field(mode, 10, **kw)
    check_write(f, lambda m: CK.load_checkpoint({"radiance_field": second.state_dict()}, m),
                "checkpoint.load_checkpoint (this package's state dict)", (0, 1, 2, 3))
    ref_state = {"radiance_field": CK.reference_state_from_field(third)}
    check_write(f, lambda m: CK.load_checkpoint(ref_state, m, assume_tcnn_layout=CK.TCNN_LAYOUT),
                "checkpoint.load_reference_checkpoint (tiny-cuda-nn layout)", (0, 1, 2, 3))


@pytest.mark.parametrize("mode,kw", PACKERS, ids=PACKER_IDS)
def test_data_assignment_of_a_weight(mode, kw):
    """`w.data = other` advances no version counter: only the address tells the tensors apart, and the allocator is
    free to give the dropped block to the replacement unless the cache entry keeps it."""
    f = make_field(mode, **kw)
    for net, which in (("xyz_wrap", (0, 1, 3)), ("mlp_base", (0, 1, 3)), ("mlp_head", (0,))):
        w = getattr(f, net)[1]
        check_write(f, lambda _: replace_data(w, lambda old: old * 0.5), f"{net}[1].data = other", which)


@pytest.mark.parametrize("mode,kw", PACKERS, ids=PACKER_IDS)
def test_write_through_data_then_weights_changed(mode, kw):
    f = make_field(mode, **kw)
    for net, which in (("xyz_wrap", (0, 1, 3)), ("mlp_base", (0, 1, 3)), ("mlp_head", (0,))):
        def write(m):
            getattr(m, net)[0].data.mul_(0.5)
            m.weights_changed()
        check_write(f, write, f"{net}[0].data.mul_(0.5) and weights_changed()", which)


# ---- DNGPradianceField: the box, the python scalars, the precision -----------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_box_writes(mode):
    f = make_field(mode)

    def cp(m):
        with torch.no_grad():
            m.aabb.copy_(m.aabb + 0.25)

    def through_data(m):
        m.aabb.data.add_(0.25)
        m.weights_changed()
    check_write(f, cp, "aabb.copy_(aabb + 0.25)")
    check_write(f, lambda m: replace_data(m.aabb, lambda old: old - 0.5), "aabb.data = other")
    check_write(f, through_data, "aabb.data.add_(0.25) and weights_changed()")


@pytest.mark.parametrize("mode,kw", PACKERS, ids=PACKER_IDS)
def test_moving_step_assigned_after_a_launch(mode, kw):
    f = make_field(mode, **kw)

    def write(m):
        m.MOVING_STEP = 1.0 / 16
    check_write(f, write, "MOVING_STEP = 1/16")


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
def test_time_mode_assigned_after_a_launch(mode):
    """The constructor stores it as a plain attribute; 1 <-> 2 keeps every shape, so the assignment is followed."""
    f = make_field(mode, use_time_embedding=True)

    def attenuate(m):
        m.time_mode = 2
    check_write(f, attenuate, "time_mode = 2")


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
def test_div_offsets_assigned_after_a_launch(mode):
    """use_div_offsets decides the motion network's output width, so an assignment that no longer fits the weights is
    refused at the next launch -- never silently ignored."""
    g = make_field(mode, use_div_offsets=True)
    first = outputs(g)
    g.use_div_offsets = False
    with pytest.raises(ValueError, match="weight shapes"):
        outputs(g)
    g.use_div_offsets = True
    assert_same(outputs(g), first, "use_div_offsets restored")


def test_precision_round_trips():
    """set_mlp_precision(a) -> launch -> set_mlp_precision(b) -> launch -> back to a: each launch is a fresh module's of
    that mode (one fresh module per mode, shared)."""
    f = make_field("f32")
    want = {m: outputs(fresh_of(f, m)) for m in MODES}
    for a in MODES:
        for b in MODES:
            if a != b:
                assert_changed(want[a], want[b], f"{a} -> {b}")
                for m in (a, b, a):
                    assert_same(outputs(f.set_mlp_precision(m)), want[m], f"set_mlp_precision {a} -> {b} -> {a}, at {m}")


# ---- DNGPradianceField: the hash table (read in place) -------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "f16x2"])
@pytest.mark.parametrize("table", ["f32_table", "f16_table", "temporal", "temporal_f16"])
def test_hash_table_writes_need_no_call(table, mode):
    kw = TABLES[table]
    f = make_field(mode, **kw)
    donor = T(make_params(9, **kw)["hash"]["table"])
    assert donor.dtype == f.hash_table.dtype and donor.shape == f.hash_table.shape

    def cp(m):
        with torch.no_grad():
            m.hash_table.copy_(donor)
    check_write(f, lambda m: m.hash_table.data.mul_(3), "hash_table.data.mul_(3)", (0, 1, 2, 3))
    check_write(f, cp, "hash_table.copy_(other)", (0, 1, 2, 3))
    check_write(f, lambda m: replace_data(m.hash_table, lambda old: (old.float() * 0.5).to(old.dtype)),
                "hash_table.data = new_table", (0, 1, 2, 3))


# ---- DNGPradianceField: copies ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_deepcopy_after_a_launch_follows_its_own_weights(mode):
    f = make_field(mode)
    original = outputs(f)
    c = copy.deepcopy(f)
    assert_same(outputs(c), original, "copy.deepcopy (nothing written yet)")

    def write(m):
        with torch.no_grad():
            m.mlp_base[1].mul_(0.5)
            m.aabb.copy_(m.aabb + 0.25)
    got = check_write(c, write, "a write to the deep copy")
    assert_same(outputs(f), original, "a write to the deep copy, seen from the original")
    assert_changed(got, original, "a write to the deep copy")


# ---- TrainableField ---------------------------------------------------------------------------------------------------------
T_NAMES = ("forward rgb", "forward sigma", "forward_rays rgb", "forward_rays sigma", "shared rgb", "shared density",
           "shared base_mlp_out")


def make_trainable(table, seed=42, device=DEV):
    from ced_nerf_amd.train import TrainableField
    return TrainableField(make_params(seed, **TABLES[table]), device)


def fresh_trainable(tf):
    from ced_nerf_amd.train import TrainableField
    return TrainableField(tf.export_params(), DEV)


def t_outputs(tf, mode="f32"):
    """tf(pos, t, d), tf.forward_rays(...) and tf.shared_inference()(pos, t, d)."""
    pos, t, d = inputs()["dev"]
    rgb, sig = tf(pos, t, d)
    rgb_r, sig_r = tf.forward_rays(*inputs()["rays"])
    s_rgb, s_res = tf.shared_inference().set_mlp_precision(mode)(pos, t, d)
    return (rgb.detach(), sig.detach(), rgb_r.detach(), sig_r.detach(), s_rgb, s_res["density"], s_res["base_mlp_out"])


def check_trainable_write(tf, write, what):
    before = t_outputs(tf)
    write(tf)
    got = t_outputs(tf)
    assert_same(got, t_outputs(fresh_trainable(tf)), what, T_NAMES)
    assert_changed(got, before, what, range(7), T_NAMES)
    return got


@pytest.mark.parametrize("table", ["f32_table", "f16_table", "temporal_f16"])
def test_trainable_field_after_load_state_dict(oracle, table):
    """ADVICE.md's fourth finding: the evaluated fp16 copy of the table is a non-persistent buffer; after a load it must
    follow the loaded master without a manual sync_half_table()."""
    tf, other = make_trainable(table), make_trainable(table, 9)
    before = t_outputs(tf)
    tf.load_state_dict(other.state_dict())
    got = t_outputs(tf)
    want = t_outputs(fresh_trainable(other))
    assert_same(got, want, "load_state_dict", T_NAMES)
    assert_changed(got, before, "load_state_dict", range(7), T_NAMES)
    pos, t, d = inputs()["np"]
    o = oracle.OracleField(other.export_params()).forward(pos, t, d, want_geo=True)      # the reference's anchor
    assert_bitexact(want[4].cpu().numpy(), o["rgb"], "fresh shared rgb vs oracle")
    assert_bitexact(want[5].cpu().numpy()[:, 0], o["density"], "fresh shared density vs oracle")
    assert_bitexact(want[6].cpu().numpy(), o["base_mlp_out"], "fresh shared base_mlp_out vs oracle")


@pytest.mark.parametrize("table", ["f32_table", "f16_table", "temporal_f16"])
def test_trainable_field_master_table_written_in_place(table):
    tf = make_trainable(table)
    donor = T(make_params(9, **TABLES[table])["hash"]["table"]).float()

    def cp(m):
        with torch.no_grad():
            m.hash_table.copy_(donor)
    check_trainable_write(tf, cp, "hash_table.copy_(other)")


def _train_scene():
    from ced_nerf_amd import synthetic as S
    from ced_nerf_amd.nerfacc_api import OccGridEstimator
    cfg = S.CONFIGS["dnerf"]
    o, d = S.make_camera_rays(24, 18, cfg["camera_angle_x"], S.look_at_c2w(cfg["radius"], 30.0, 30.0, cfg["opengl"]), cfg["opengl"])

    def estimator():
        est = OccGridEstimator(BOX, 32, 1).to(DEV)
        est.set_binaries(torch.ones_like(est.binaries))
        return est
    rng = np.random.default_rng(3)
    return (T(o.reshape(-1, 3)), T(d.reshape(-1, 3)), T(np.array([[0.5]], np.float32)),
            T(rng.uniform(0, 1, size=(24 * 18, 3)).astype(np.float32)), estimator)


@pytest.mark.parametrize("scaler", [False, True], ids=["plain", "grad_scaler"])
@pytest.mark.parametrize("mode", ["f32", "f16x2"])
@pytest.mark.parametrize("table", ["f32_table", "f16_table"])
def test_shared_inference_sees_a_fused_adam_step(table, mode, scaler):
    """One train_step with torch.optim.Adam(fused=True) over all parameters: the shared inference module, launched before
    the step, evaluates the stepped weights -- those of `to_inference()`, a fresh copy -- and so does the occupancy
    refresh that follows the step (the order `fit` uses)."""
    from ced_nerf_amd.model import make_occ_eval_fn
    from ced_nerf_amd.train import refresh_occupancy, train_step
    rays_o, rays_d, ts, target, estimator = _train_scene()
    tf = make_trainable(table)
    shared = tf.shared_inference().set_mlp_precision(mode)
    before = outputs(shared)                                   # every cache populated with the weights before the step
    opt = torch.optim.Adam(tf.parameters(), lr=1e-2, eps=1e-15, fused=True)
    gs = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10) if scaler else None
    est = estimator()
    out = train_step(tf, est, opt, rays_o, rays_d, ts, target, 2e-2, render_bkgd=torch.ones(3, device=DEV), grad_scaler=gs)
    assert out["n_samples"] > 0 and np.isfinite(out["loss"])
    got = outputs(tf.shared_inference())
    assert tf.shared_inference() is shared and shared.mlp_precision == mode
    assert_same(got, outputs(tf.to_inference(DEV, mode)), "a fused Adam step")
    assert_changed(got, before, "a fused Adam step", (0, 1, 2, 3))
    # the refresh after the step: the same draws, once through the shared module and once through a fresh copy
    a, b = estimator(), estimator()
    torch.manual_seed(5)
    refresh_occupancy(tf, a, 0, ts, 2e-2)
    torch.manual_seed(5)
    b.train()
    b.update_every_n_steps(step=0, occ_eval_fn=make_occ_eval_fn(tf.to_inference(DEV, mode), ts, 2e-2), occ_thre=1e-2)
    assert torch.equal(a.occs, b.occs) and torch.equal(a.binaries, b.binaries), "stale density in refresh_occupancy"
    assert not torch.equal(a.occs, est.occs)
    assert_same(outputs(tf.shared_inference()), got, "refresh_occupancy")


def _torch_statement_params(seed=21):
    """The recipe of test_trainable_field_fused_elementwise_pieces_match_the_torch_statements, whose tolerance is used."""
    from ced_nerf_amd import synthetic as S
    p = S.init_field_params(BOX, 1e-3, 1024, 14, regime="init", seed=seed)
    p["hash"]["table"] = (p["hash"]["table"] * 3000.0).astype(np.float32)
    return p


def test_trainable_field_box_writes():
    """`_aabb6` (the box as python floats for the fused warp kernel) and the shared module's box follow aabb.copy_ and
    aabb.data = ...: against a fresh field bit for bit, and against the torch statements (`fused_glue = False`), which
    read self.aabb directly."""
    from ced_nerf_amd.train import TrainableField
    tf = TrainableField(_torch_statement_params(), DEV)
    pos, t, d = inputs()["dev"]

    def cp(m):
        with torch.no_grad():
            m.aabb.copy_(m.aabb + 0.25)
    for write, what in ((cp, "aabb.copy_(aabb + 0.25)"),
                        (lambda m: replace_data(m.aabb, lambda old: old - 0.5), "aabb.data = other")):
        got = check_trainable_write(tf, write, what)
        tf.fused_glue = False
        try:
            rgb, sig = tf(pos, t, d)
        finally:
            del tf.fused_glue
        inside = int((sig != 0).sum())
        assert 0 < inside < N                           # some samples inside the box, some outside
        assert torch.equal(got[1] == 0, sig == 0), f"stale box after {what}: the selector differs from the torch statements'"
        err_rgb = (got[0] - rgb).abs().max().item()
        err_sig = ((got[1] - sig).abs() - 2e-5 * sig.abs()).max().item()
        print(f"  {what}: fused vs torch statements, max |rgb diff| {err_rgb:.3e}, max (|sigma diff| - 2e-5 |sigma|) {err_sig:.3e}")
        assert err_rgb <= 2e-6, what
        assert ((got[1] - sig).abs() <= 2e-5 * sig.abs() + 1e-12).all(), what


@pytest.mark.parametrize("table", ["f32_table", "f16_table"])
def test_trainable_field_moved_to_the_gpu_after_shared_inference(table):
    """Module._apply replaces buffer objects: a shared module built before the move must not keep the old ones."""
    tf = make_trainable(table, device="cpu")
    assert tf.shared_inference().aabb.device.type == "cpu"
    tf = tf.to(DEV)
    assert_same(t_outputs(tf), t_outputs(fresh_trainable(tf)), "the move to the GPU", T_NAMES)
    donor = T(make_params(9, **TABLES[table])["hash"]["table"]).float()

    def write(m):
        with torch.no_grad():
            m.aabb.copy_(m.aabb + 0.25)
            m.hash_table.copy_(donor)
    check_trainable_write(tf, write, "aabb.copy_ and hash_table.copy_ after the move")


def test_trainable_field_deepcopy_shares_nothing_with_the_original():
    tf = make_trainable("f16_table")
    original = t_outputs(tf)
    c = copy.deepcopy(tf)
    other = make_trainable("f16_table", 9)
    check_trainable_write(c, lambda m: m.load_state_dict(other.state_dict()), "load_state_dict into the deep copy")
    assert_same(t_outputs(tf), original, "a load into the deep copy, seen from the original", T_NAMES)


# ---- frame level ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_second_frame_after_a_weight_copy(oracle, mode):
    """Two render_image_test calls on the same stream and the same cached workspace, a weight copy_ between them: the
    second frame is a fresh field's, and the fresh field's frame is the oracle's."""
    from ced_nerf_amd import synthetic as S
    from ced_nerf_amd.nerfacc_api import OccGridEstimator
    from ced_nerf_amd.utils import Rays, render_image_test
    cfg = S.CONFIGS["dnerf"]
    w, h, res = 48, 36, 64
    o, d = S.make_camera_rays(w, h, cfg["camera_angle_x"], S.look_at_c2w(cfg["radius"], 30.0, 30.0, cfg["opengl"]), cfg["opengl"])
    binaries = S.make_occupancy(BOX, res, 1)
    est = OccGridEstimator(BOX, res, 1).to(DEV)
    est.set_binaries(T(binaries))
    ts = np.array([[0.5]], np.float32)
    bk = np.ones(3, np.float32)
    rk = dict(near_plane=0.0, far_plane=1e10, render_step_size=5e-3, cone_angle=0.0)
    rays = Rays(T(o), T(d))

    def frame(field):
        rgb, op, dp, total = render_image_test(1024, field, est, rays, timestamps=T(ts), render_bkgd=T(bk), **rk)
        return rgb, op, dp, torch.tensor(total)
    names = ("rgb", "opacity", "depth", "total samples")
    f = make_field(mode)
    donor = make_params(9)
    first = frame(f)
    with torch.no_grad():
        f.mlp_base[1].copy_(T(donor["mlp_base"][1]))
        f.mlp_head[2].copy_(T(donor["mlp_head"][2]))
    second = frame(f)
    fresh = fresh_of(f)
    want = frame(fresh)
    assert_same(second, want, "a weight copy_ between two frames", names)
    assert_changed(second, first, "a weight copy_ between two frames", (0, 1, 2), names)
    oest = oracle.OracleEstimator(BOX, res, 1, binaries)
    w_rgb, w_op, w_dp, w_total = oracle.render_image_test(1024, oracle.OracleField(fresh.export_params(), mlp_half=mode), oest,
                                                          o, d, timestamps=ts, render_bkgd=bk, **rk)
    assert int(want[3]) == w_total and w_total > 1000
    assert_bitexact(want[0].cpu().numpy(), w_rgb, f"fresh {mode} frame rgb vs oracle")
    assert_bitexact(want[1].cpu().numpy(), w_op, f"fresh {mode} frame opacity vs oracle")
    assert_bitexact(want[2].cpu().numpy(), w_dp, f"fresh {mode} frame depth vs oracle")


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
def test_two_threads_get_the_descriptor_of_the_written_weights(mode):
    """Frames in flight share one field: after a write, two threads ask for the descriptor at once.  Both get the one
    whose blob is the fresh module's.  Only the host-side packing runs in the threads; no kernel is launched there."""
    f = make_field(mode)
    outputs(f)
    bits = lambda blob: blob.view(torch.int32)
    old_blob = bits(f._packed).clone()
    with torch.no_grad():
        f.mlp_base[0].mul_(0.5)
    gate, got, errors = threading.Barrier(2), [None, None], []

    def ask(i):
        try:
            gate.wait(timeout=30)
            got[i] = f._descriptor()
        except Exception as e:          # noqa: BLE001 -- reported below
            errors.append(e)
    threads = [threading.Thread(target=ask, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=60)
    assert not errors and not any(th.is_alive() for th in threads), errors
    torch.cuda.synchronize()
    fresh = fresh_of(f)
    want_desc = fresh._descriptor()
    for d in got:
        assert d is got[0] and d.packed_weights == f._packed.data_ptr() and d.packed_floats == want_desc.packed_floats
    assert torch.equal(bits(f._packed), bits(fresh._packed)), "stale weight blob handed to a thread"
    assert not torch.equal(bits(f._packed), old_blob)
    assert_same(outputs(f), outputs(fresh), "a write seen by two threads")
