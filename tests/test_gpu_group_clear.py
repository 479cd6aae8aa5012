"""GPU suite: the frame renderers with the group clearance of the first iteration (csrc/march_accel.hpp: group_clear;
frame.hip: ray_group_bounds_kernel, ray_group_clear_kernel, the skip and the hint in the first-iteration kernels)
against the CPU oracle, bit for bit: render_image_test and a 2-frame render_frames_test at 50 x 50 rays (groups of 64
that straddle image rows, a partial last group) and 64 x 64 (a group per row), with one grid level (the one-pass first
iteration) and two (culling pass + candidate list), with the caller's distance fields and with none brought (the brick
field alone), with the rays shuffled and in tile order, and sharded with a padded share (local_rays below
rays_per_frame)."""
import threading

import numpy as np
import pytest
import torch

from conftest import assert_bitexact

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAX_SAMPLES = 1024
SCENES = {"dnerf": 1, "hypernerf": 2}            # grid levels: one pass / two passes by default
SIZES = [(50, 50), (64, 64)]
CAMERAS = [(30.0, 10.0, 1.0, 0.25), (55.0, 140.0, 0.8, 0.75)]      # elevation, azimuth, radius factor, time


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def cases(oracle):
    """Per scene and size: the field, the estimator, two frames' rays and the oracle's render of each frame (computed
    once, shared by every test below and left unchanged)."""
    from ced_nerf_amd import synthetic as S
    from ced_nerf_amd.model import DNGPradianceField
    from ced_nerf_amd.nerfacc_api import OccGridEstimator
    out = {}
    for name, levels in SCENES.items():
        for w, h in SIZES:
            sc = S.make_scene(name, w, h, "trained", log2_hashmap_size=15)
            cfg = sc["cfg"]
            assert cfg["grid_levels"] == levels
            of = oracle.OracleField(sc["params"])
            oest = oracle.OracleEstimator(cfg["aabb"], cfg["grid_resolution"], cfg["grid_levels"], sc["binaries"])
            f = DNGPradianceField.from_params(sc["params"], DEV).eval()
            est = OccGridEstimator(cfg["aabb"], cfg["grid_resolution"], cfg["grid_levels"]).to(DEV)
            est.set_binaries(T(sc["binaries"]))
            rk = dict(sc["render"]); rk["render_bkgd"] = T(rk["render_bkgd"])
            frames = []
            for elev, az, radius, t in CAMERAS:
                o, d = S.make_camera_rays(w, h, cfg["camera_angle_x"], S.look_at_c2w(cfg["radius"] * radius, elev, az, cfg["opengl"]),
                                          cfg["opengl"])
                want = oracle.render_image_test(MAX_SAMPLES, of, oest, o, d, timestamps=np.asarray([[t]], np.float32), **sc["render"])
                frames.append(dict(o=o, d=d, t=np.float32(t), want=want))
            assert frames[0]["want"][3] > 500 and (frames[0]["want"][1] == 0).mean() > 0.3       # samples, and empty tiles
            out[(name, w, h)] = dict(f=f, est=est, rk=rk, frames=frames, w=w, h=h)
    return out


def check_frame(got, want, what, perm=None):
    rgb, op, dp, total = got
    assert total == want[3], (what, total, want[3])
    for g, w_, nm in ((rgb, want[0], "rgb"), (op, want[1], "opacity"), (dp, want[2], "depth")):
        w_ = np.ascontiguousarray(w_).reshape(-1, w_.shape[-1])
        assert_bitexact(N(g).reshape(-1, w_.shape[-1]), w_ if perm is None else w_[perm], f"{what}: {nm}")


def native_kwargs(c):
    rk = c["rk"]
    return dict(near_plane=rk.get("near_plane", 0.0), far_plane=rk.get("far_plane", 1e10),
                render_step_size=rk["render_step_size"], cone_angle=rk.get("cone_angle", 0.0),
                early_stop_eps=rk.get("early_stop_eps", 1e-4), bkgd=rk["render_bkgd"].reshape(-1).float().contiguous())


def render_one(c, o, d, t, accel):
    """ced_render_image_test on rays [n, 3]; accel: the estimator's distance fields, or None (the brick field is built
    inside the call)."""
    from ced_nerf_amd import ops
    k = native_kwargs(c)
    est = c["est"]
    return ops.render_image_test_native(c["f"]._descriptor(), T(o), T(d), est.binaries, est.aabbs.contiguous(), k["near_plane"],
                                        k["far_plane"], k["render_step_size"], k["cone_angle"], k["early_stop_eps"], MAX_SAMPLES,
                                        torch.tensor([t], device=DEV), False, k["bkgd"], accel=accel)


def render_two(c, frames, accel):
    from ced_nerf_amd import ops
    k = native_kwargs(c)
    est = c["est"]
    o = torch.cat([T(fr["o"]).reshape(-1, 3) for fr in frames]); d = torch.cat([T(fr["d"]).reshape(-1, 3) for fr in frames])
    return ops.render_frames_test_native(c["f"]._descriptor(), len(frames), o, d, est.binaries, est.aabbs.contiguous(),
                                         k["near_plane"], k["far_plane"], k["render_step_size"], k["cone_angle"],
                                         k["early_stop_eps"], MAX_SAMPLES, torch.tensor([fr["t"] for fr in frames], device=DEV),
                                         k["bkgd"], accel=accel)


@pytest.mark.parametrize("brought", [True, False], ids=["callers_accel", "no_accel"])
@pytest.mark.parametrize("wh", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(SCENES))
def test_frames_with_group_clearance_match_the_oracle(cases, name, wh, brought):
    c = cases[(name, wh[0], wh[1])]
    accel = c["est"].occupancy_accel() if brought else None
    fr = c["frames"]
    n = wh[0] * wh[1]
    check_frame(render_one(c, fr[0]["o"].reshape(-1, 3), fr[0]["d"].reshape(-1, 3), fr[0]["t"], accel), fr[0]["want"], "frame alone")
    rgb, op, dp, totals = render_two(c, fr, accel)
    torch.cuda.synchronize()
    for k in range(2):
        s = slice(k * n, (k + 1) * n)
        check_frame((rgb[s], op[s], dp[s], totals[k]), fr[k]["want"], f"frame {k} of two")


@pytest.mark.parametrize("order", ["shuffled", "tiles"])
@pytest.mark.parametrize("wh", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(SCENES))
def test_reordered_rays_match_the_oracle(cases, name, wh, order):
    """The schedule is image-global, so a frame's rays in another order render the same pixels in that order: shuffled
    (groups of unrelated rays: nothing may be claimed wrongly) and in 8 x 8 tile order (the narrow bundles)."""
    c = cases[(name, wh[0], wh[1])]
    w, h = wh
    if order == "shuffled":
        perm = np.random.default_rng(3).permutation(w * h)
    else:
        idx = np.arange(w * h).reshape(h, w)
        perm = np.concatenate([idx[y:y + 8, x:x + 8].ravel() for y in range(0, h, 8) for x in range(0, w, 8)])
    fr = c["frames"][1]
    o, d = fr["o"].reshape(-1, 3)[perm], fr["d"].reshape(-1, 3)[perm]
    for accel in (c["est"].occupancy_accel(), None):
        check_frame(render_one(c, o, d, fr["t"], accel), fr["want"], order, perm)


@pytest.mark.parametrize("name", list(SCENES))
def test_sharded_frames_with_padded_shares_match_the_oracle(cases, name):
    """Two frames of 50 x 50 dealt in 8 x 8 tiles over two ranks (threads of this process, the exchange a host-side sum):
    the shares are uneven, so a rank's frames carry padding rays (local_rays below rays_per_frame) that belong to no
    group.  The re-assembled frames are the oracle's."""
    from ced_nerf_amd import ops
    from ced_nerf_amd.dist import ShardedRenderer
    c = cases[(name, 50, 50)]
    W = H = 50
    world, n_frames = 2, 2
    fr = c["frames"]
    os_ = torch.stack([T(x["o"]) for x in fr]); ds_ = torch.stack([T(x["d"]) for x in fr])
    times = torch.tensor([x["t"] for x in fr], device=DEV)
    c["est"].occupancy_accel(); c["f"]._descriptor()
    acc, lock, barrier = {}, threading.Lock(), threading.Barrier(world)
    ranks = []
    for r in range(world):
        sr = ShardedRenderer(c["f"], c["est"], world, r, torch.device(DEV), max_samples=MAX_SAMPLES, render_kwargs=c["rk"])
        sr.set_rays(os_, ds_)
        n_calls = [0]

        def reduce_fn(row, n_calls=n_calls):
            torch.cuda.current_stream().synchronize()
            with lock:
                acc[n_calls[0]] = acc.get(n_calls[0], 0) + row.clone()
            barrier.wait(timeout=120)
            row.copy_(acc[n_calls[0]])
            n_calls[0] += 1

        sr.exchange = ops.ScheduleExchange(n_frames, H * W, sr.local_real, torch.device(DEV), MAX_SAMPLES,
                                           float(c["rk"].get("cone_angle", 0.0)), reduce_fn=reduce_fn)
        ranks.append(sr)
    assert any(v < sr.n_unit for sr in ranks for v in sr.local_real)          # a share with padding rays
    outs, errs = [None] * world, []

    def work(r):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                outs[r] = ranks[r].render_local(times)
                torch.cuda.current_stream().synchronize()
        except BaseException as e:
            errs.append(e)
            barrier.abort()

    threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    n_img = H * W
    img = torch.zeros((n_frames * n_img + 1, 5), device=DEV)
    for r, sr in enumerate(ranks):
        rgb, op, dp, _ = outs[r]
        img[sr.gather_index.view(world, -1)[r, :-1]] = torch.cat([rgb, op, dp], dim=1)
    img = img[:-1].view(n_frames, n_img, 5)
    assert sum(o[3] for o in outs) == sum(x["want"][3] for x in fr)
    for k in range(n_frames):
        check_frame((img[k, :, 0:3], img[k, :, 3:4], img[k, :, 4:5], fr[k]["want"][3]), fr[k]["want"], f"sharded frame {k}")


@pytest.mark.parametrize("name", list(SCENES))
def test_negative_near_plane_renders_the_oracles_frame(oracle, cases, name):
    """A camera inside the boxes with a negative near plane: segments start below 0, where the clearance claims nothing
    (it is not computed) and no walk may have its start moved.  One frame and two frames, with and without the caller's
    distance fields, against the oracle on the same rays."""
    from ced_nerf_amd import synthetic as S
    c = dict(cases[(name, 50, 50)])
    sc = S.make_scene(name, 50, 50, "trained", log2_hashmap_size=15)
    fr = c["frames"][0]
    o = np.ascontiguousarray(np.broadcast_to(np.asarray([0.02, -0.03, 0.01], np.float32), fr["o"].shape))
    kw = dict(sc["render"]); kw["near_plane"] = -3.0
    of = oracle.OracleField(sc["params"])
    cfg = sc["cfg"]
    oest = oracle.OracleEstimator(cfg["aabb"], cfg["grid_resolution"], cfg["grid_levels"], sc["binaries"])
    want = oracle.render_image_test(MAX_SAMPLES, of, oest, o, fr["d"], timestamps=np.asarray([[fr["t"]]], np.float32), **kw)
    plain = oracle.render_image_test(MAX_SAMPLES, of, oest, o, fr["d"], timestamps=np.asarray([[fr["t"]]], np.float32), **sc["render"])
    assert want[3] > 500 and want[3] != plain[3] and not np.array_equal(want[2], plain[2])     # the stretch below 0 matters
    c["rk"] = dict(c["rk"]); c["rk"]["near_plane"] = -3.0
    inside = dict(o=o, d=fr["d"], t=fr["t"], want=want)
    for accel in (c["est"].occupancy_accel(), None):
        check_frame(render_one(c, o.reshape(-1, 3), fr["d"].reshape(-1, 3), fr["t"], accel), want, "frame alone, near < 0")
        rgb, op, dp, totals = render_two(c, [inside, inside], accel)
        torch.cuda.synchronize()
        for k in range(2):
            s_ = slice(k * 2500, (k + 1) * 2500)
            check_frame((rgb[s_], op[s_], dp[s_], totals[k]), want, f"frame {k} of two, near < 0")
