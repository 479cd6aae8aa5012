"""The eight table / time variants of the field kernels, named once (no GPU import: the CPU companion imports this too).

Three launchers pick a kernel with the same selector, sel = (time encoding ? 1 : 0) | (fp16 table ? 2 : 0) |
(temporal table ? 4 : 0): launch_field (csrc/field.hip, mode f32), field_mixed.hip (f32+h16x2) and launch_field_half
(csrc/field_half.hip, modes f16x2 and f16).  Eight variants times four arithmetic modes are the 32 kernels; every cell is
launched by the tests named here:

  per-sample mode   tests/test_gpu_field_variants.py::test_per_sample[sel x mode]               all 32
  rays mode         tests/test_gpu_field_variants.py::test_rays_mode[sel 2..7 x mode]           24
                    sel 0, 1: f16x2 / f16 in tests/test_gpu_field_front_end.py (kinds plain, div, te); f32 and
                    f32+h16x2 through the frame loop below, which launches the field kernel in rays mode only
  inside a frame    tests/test_gpu_frame_variants.py::test_render_image_test[sel x mode]        all 32
  loop              and there: render_frames_test (sel 4..7; f32, f16x2), render_image (sel 3, 4, 7), native sampling
                    (sel 7), six fuzz seeds (sel 2..7)

The odd selectors also use the six-wide motion output (use_div_offsets); sel 3 and 7 use time_mode 2
(use_time_attenuation), so both are crossed with the fp16 and the temporal tables.
"""
import numpy as np

MODES = ["f32", "f16x2", "f16", "f32+h16x2"]
SELS = list(range(8))
TEMPORAL_SELS = [4, 5, 6, 7]
AABB = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
F32 = np.float32
T13, T23 = F32(1.0 / 3.0), F32(2.0 / 3.0)        # the key-frame boundaries of the temporal table (t * 3 = 1, 2)


def variant_kw(sel):
    """init_field_params keywords of selector `sel`"""
    kw = dict(table_dtype=np.float16 if sel & 2 else np.float32, temporal_hash=bool(sel & 4),
              use_time_embedding=bool(sel & 1))
    if sel & 1:
        kw["use_div_offsets"] = True
    if sel in (3, 7):
        kw["use_time_attenuation"] = True
    return kw


def selector_of(params):
    """the launchers' selector, from a parameter set"""
    h = params["hash"]
    return (1 if params["time_mode"] else 0) | (2 if h["table"].dtype == np.float16 else 0) | (4 if h["temporal"] else 0)


def field_params(sel):
    """The "trained" regime on the box AABB at max_res 1024, log2_hashmap_size 15"""
    from ced_nerf_amd import synthetic as S
    p = S.init_field_params(AABB, 1.0 / 64, 1024, 15, regime="trained", seed=30 + sel, **variant_kw(sel))
    assert selector_of(p) == sel
    return p


def key_times():
    """0, 1, float32(1/3), float32(2/3) and the float32 neighbours of both on either side"""
    lo, hi = F32(0), F32(1)
    return np.array([0.0, 1.0, T13, T23, np.nextafter(T13, lo), np.nextafter(T13, hi), np.nextafter(T23, lo),
                     np.nextafter(T23, hi)], F32)


def sample_times(n, rng):
    """n times in [0, 1]: key_times() first (cut at n) and, from n = 16 on, again at the end (the ragged last tile);
    the rest uniform, so that a wave's lanes sit in all three key-frame intervals"""
    t = rng.uniform(0, 1, size=n).astype(F32)
    k = key_times()
    if n >= 2 * k.shape[0]:
        t[n - k.shape[0]:] = k
    t[:min(n, k.shape[0])] = k[:n]
    return t


def keyframe_interval(t):
    """index of the key-frame pair the temporal table interpolates at time t: min(floor(3 t), 2)"""
    return np.minimum(np.floor(np.asarray(t, F32) * F32(3)), 2).astype(np.int64)


def sample_points(n):
    """positions in and around the box (faces, a corner, outside on one axis and on all), all key-frame times, directions"""
    rng = np.random.default_rng(11)
    pos = rng.uniform(-1.6, 1.6, size=(n, 3)).astype(F32)
    edge = [[1.5, 0, 0], [-1.5, 0, 0], [0, 1.5, 0], [0, -1.5, 0], [0, 0, 1.5], [0, 0, -1.5], [-1.5, -1.5, -1.5],
            [1.5, 1.5, 1.5], [1.6, 0.2, 0.3], [0.2, -1.7, 0.3], [0.2, 0.3, 1.6], [3.0, 3.0, 3.0]]
    pos[8:8 + len(edge)] = np.asarray(edge, F32)                # after the key-frame times of samples 0..7
    pos[:8] = rng.uniform(-1.4, 1.4, size=(8, 3)).astype(F32)   # the key-frame times inside the box
    pos[n - 8:] = rng.uniform(-1.4, 1.4, size=(8, 3)).astype(F32)
    t = sample_times(n, rng)
    d = rng.normal(size=(n, 3)).astype(F32)
    return pos, t.reshape(n, 1), d


# --- frame scenes --------------------------------------------------------------------------------------------------
# HyperNeRF-shaped marching (two grid levels, cone angle, near plane, alpha threshold) with the variant's flags.  The
# stock "trained" regime ends every hit ray within three iterations and the "init" regime stops none, so the density
# row of mlp_base is scaled down: a frame then runs some twenty iterations, ends a good part of its rays by the early
# stop and leaves another part see-through (tests/test_field_variants_cpu.py asserts it for every scene and mode).
FRAME_W, FRAME_H = 40, 30
FRAME_TIME = T13
FRAME_CFG = dict(aabb=[-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], near_plane=0.2, far_plane=1e10, moving_step=1.0 / 4096,
                 hash_max_res=4096, grid_resolution=128, grid_levels=2, render_step_size=1e-3, alpha_thre=1e-2,
                 cone_angle=0.004, bkgd=[0.0, 0.0, 0.0], opengl=False, camera_angle_x=0.8, radius=1.6)
# The scale per variant: what a scan of the f32 oracle (0.15 .. 0.8) put nearest to equal shares of both kinds of pixel.
DENSITY_ROW_SCALE = {0: 0.8, 1: 0.3, 2: 0.8, 3: 0.45, 4: 0.8, 5: 0.21, 6: 0.8, 7: 0.25}


def with_variant(sc, sel, seed):
    """`sc` (a synthetic.make_scene dict) with its field parameters rebuilt as variant `sel`: same box, moving step,
    table geometry and regime scale, the variant's table type and flags"""
    from ced_nerf_amd import synthetic as S
    cfg, old = sc["cfg"], sc["params"]
    p = S.init_field_params(old["aabb"], cfg["moving_step"], cfg["hash_max_res"], 15, regime="trained",
                            seed=seed, **variant_kw(sel))
    assert selector_of(p) == sel
    out = dict(sc)
    out["params"] = p
    return out


def frame_scene(sel):
    """The 40x30 frame of variant `sel` at float32(1/3), registered as a temporary synthetic.CONFIGS entry whose flags carry the variant"""
    from ced_nerf_amd import synthetic as S
    kw = variant_kw(sel)
    table_dtype = kw.pop("table_dtype")
    name = f"variant{sel}"
    S.CONFIGS[name] = dict(FRAME_CFG, flags=kw)
    try:
        sc = S.make_scene(name, FRAME_W, FRAME_H, "trained", table_dtype=table_dtype, log2_hashmap_size=15,
                          timestamp=float(FRAME_TIME))
    finally:
        del S.CONFIGS[name]
    sc["params"]["mlp_base"][1][0, :] *= F32(DENSITY_ROW_SCALE[sel])
    assert selector_of(sc["params"]) == sel
    return sc


def frame_conditions(trace, opacity):
    """(iterations, samples, share of pixels ended by the early stop, share of see-through pixels) of an oracle frame"""
    op = np.asarray(opacity).reshape(-1)
    return (len(trace), int(sum(t["n_new"] for t in trace)), float((op > 0.99).mean()),
            float(((op > 0) & (op < 0.99)).mean()))
