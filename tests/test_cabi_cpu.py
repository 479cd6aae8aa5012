"""CPU suite, part 2: the C-ABI library and the host logic (no kernel is launched here)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch


def test_library_exports_every_declared_symbol():
    from ced_nerf_amd import _lib
    names = _lib.header_symbols()
    assert len(names) >= 15 and set(names) == set(_lib.PROTOTYPES), set(names) ^ set(_lib.PROTOTYPES)
    raw = C.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), f"{n} declared in include/cednerf_hip.h but not exported"
    L = _lib.lib()
    assert L.ced_version() == 1


def test_header_is_plain_c_and_a_c_program_binds_the_library(tmp_path):
    """include/cednerf_hip.h compiles as C99 (no C++, no torch types) and a C program linked against nothing but libdl
    loads the library, resolves entry points by name and gets the error convention (negative code + message, no
    abort) -- the binding a non-Python caller of the boundary would write."""
    import subprocess
    from ced_nerf_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "bind.c"
    src.write_text(r'''
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>
#include "cednerf_hip.h"
int main(int argc, char **argv)
{
    void *h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
    if (!h) { fprintf(stderr, "%s\n", dlerror()); return 2; }
    int (*version)(void) = (int (*)(void))dlsym(h, "ced_version");
    const char *(*last_error)(void) = (const char *(*)(void))dlsym(h, "ced_last_error_string");
    int (*set_option)(const char *, int) = (int (*)(const char *, int))dlsym(h, "ced_set_option");
    int64_t (*ws)(int64_t, int32_t, int32_t, float, int32_t) =
        (int64_t (*)(int64_t, int32_t, int32_t, float, int32_t))dlsym(h, "ced_render_image_test_workspace_bytes");
    if (!version || !last_error || !set_option || !ws) return 3;
    if (version() <= 0) return 4;
    if (set_option("no_such_option", 1) >= 0 || strlen(last_error()) == 0) return 5;      /* refused with a message */
    if (ws(640000, 1, 128, 0.0f, 1024) <= 0) return 6;
    ced_field_desc d; memset(&d, 0, sizeof d);
    printf("ok %d %zu\n", version(), sizeof d);
    return 0;
}
''')
    exe = tmp_path / "bind"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(src), "-o", str(exe),
                           "-ldl"])
    out = subprocess.run([str(exe), _lib.LIB_PATH], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    import ctypes as C
    assert out.stdout.split()[0] == "ok" and int(out.stdout.split()[2]) == C.sizeof(_lib.FieldDesc)


def test_struct_layout_matches_header():
    from ced_nerf_amd import _lib
    assert C.sizeof(_lib.HashDesc) == 16 + 5 * 64 + 8 + 8
    # aabb[6], moving_step, 4 int32 (use_div_offsets, time_mode, mlp_precision, max_workgroups), 4 bytes of padding,
    # packed_weights, packed_floats, hash
    assert C.sizeof(_lib.FieldDesc) == 24 + 4 + 4 * 4 + 4 + 8 + 8 + C.sizeof(_lib.HashDesc)
    assert _lib.FieldDesc.max_workgroups.offset == 40 and _lib.FieldDesc.packed_weights.offset == 48
    assert _lib.FieldDesc.hash.offset == 64


def test_argument_errors_are_reported_not_thrown():
    from ced_nerf_amd import _lib
    L = _lib.lib()
    rc = L.ced_ray_aabb_intersect(-1, None, None, 1, None, 0.0, 1.0, 1.0, None, None, None, None)
    assert rc == -1 and b"ray_aabb_intersect" in L.ced_last_error_string()
    rc = L.ced_ray_aabb_intersect(5, None, None, 1, None, 0.0, 1.0, 1.0, None, None, None, None)
    assert rc == -1 and b"null pointer" in L.ced_last_error_string()
    assert L.ced_ray_aabb_intersect(0, None, None, 1, None, 0.0, 1.0, 1.0, None, None, None, None) == 0   # empty input
    rc = L.ced_traverse_grids(4, None, None, None, 1, 128, None, None, None, 1e-3, 0.0, 0, None, None, None, None, 7,
                              None, None, None, None, None, None, None, None)
    assert rc == -1 and b"mode" in L.ced_last_error_string()
    assert L.ced_accumulate_along_rays(3, None, None, None, 3, None, None) == -1
    with pytest.raises(RuntimeError, match="accumulate_along_rays"):
        _lib.check(-1, "accumulate_along_rays")
    d = _lib.FieldDesc()
    d.hash.n_levels = 12
    assert L.ced_field_forward(C.byref(d), 4, 1, 1, None, None, 1, None, None) != 0
    assert L.ced_field_forward(C.byref(d), 0, None, None, None, None, None, None, None) == 0            # n == 0
    assert L.ced_render_image_test_workspace_bytes(640000, 1, 128, 0.0, 1024) > 0
    assert L.ced_render_image_test_workspace_bytes(10, 9, 128, 0.0, 16) < 0                                  # too many grids
    tot = C.c_int64(-1)
    assert L.ced_render_image_test(C.byref(d), 0, None, None, None, 1, 128, None, None, 0.0, 1e10, 5e-3, 0.0, 1e-4, 64, None, 0,
                                   None, None, None, None, None, 0, None, C.byref(tot), None, None, None) == 0   # no rays
    assert tot.value == 0
    assert L.ced_render_image_test(C.byref(d), 5, None, None, None, 1, 128, None, None, 0.0, 1e10, 5e-3, 0.0, 1e-4, 64, None, 0,
                                   None, None, None, None, None, 0, None, C.byref(tot), None, None, None) == -1
    # brick field + scratch (padded to 256 bytes), cell field + scratch
    assert L.ced_occupancy_accel_bytes(1, 128) == 2 * 16 ** 3 + 2 * 128 ** 3
    assert L.ced_occupancy_accel_bytes(4, 100) == (2 * 4 * 13 ** 3 + 255) // 256 * 256 + 2 * 4 * 100 ** 3
    assert L.ced_occupancy_accel_bytes(1, 4096) < 0
    assert L.ced_build_occupancy_accel(None, 1, 128, None, 0, None) == -1
    assert L.ced_set_option(b"field_max_blocks", 128) == -1          # a per-call descriptor field now, not process state
    # retired A/B knobs: the library has one launch geometry per kernel and no variant to select
    for key in (b"field_variant", b"half_variant", b"mixed_variant", b"field_stagger", b"hash_grad_form", b"march_early_out"):
        assert L.ced_set_option(key, 0) == -1 and key in L.ced_last_error_string(), key
    for key, default in ((b"field_spread_tiles", 2), (b"march_two_pass", -1), (b"hash_grad_blocks", 0)):
        assert L.ced_set_option(key, default) == 0, key


def test_per_sample_entries_report_the_same_argument_errors():
    """The six per-sample entries on the motion network (move, velocity, density gradient and their rays twins) make the
    same checks in the same order: descriptor, n < 0, n == 0 (success before any pointer is looked at), null inputs, no
    output requested; the gradient pair then asks for sixteen levels.  Return codes and error strings as literals; every
    case returns before a launch, so host pointers stand in for device memory."""
    from ced_nerf_amd import _lib
    L = _lib.lib()
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, C.c_void_p)
    d = _lib.FieldDesc()
    d.packed_weights = ptr
    d.packed_floats = L.ced_packed_weight_words(0, 0, 0)
    d.hash.n_levels = 12                                  # a table validate_hash accepts: twelve hashed levels of 8 entries
    d.hash.table = ptr
    d.hash.total_entries = 8 * 12
    for l in range(12):
        d.hash.scale[l], d.hash.res[l], d.hash.offset[l], d.hash.size[l], d.hash.hashed[l] = 1.0, 2, 8 * l, 8, 1
    # entry -> (rays entry?, number of outputs)
    entries = {"field_move": (False, 4), "field_move_rays": (True, 2), "field_velocity": (False, 3),
               "field_velocity_rays": (True, 3), "field_density_gradient": (False, 4), "field_density_gradient_rays": (True, 4)}

    def call(name, desc, n, inputs, outputs):
        rays, n_out = entries[name]
        i, o = (ptr if inputs else None), (ptr if outputs else None)
        args = [None, i, i, i, i, i, i, 1] if rays else [i, i]        # rays: n_dev (optional), six pointers, t_per_ray
        rc = getattr(L, "ced_" + name)(desc, n, *args, *([o] * n_out), None)
        return rc, L.ced_last_error_string().decode()

    for name, (rays, _) in entries.items():
        assert call(name, None, 4, True, True) == (-1, f"{name}: null descriptor"), name
        assert call(name, C.byref(d), -1, True, True) == (-1, f"{name}: n < 0"), name
        assert call(name, C.byref(d), 0, False, False)[0] == 0, name
        assert call(name, C.byref(d), 4, False, True) == (-1, f"{name}: null pointer" if rays else f"{name}: null positions/t"), name
        assert call(name, C.byref(d), 4, True, False) == (-1, f"{name}: no output requested"), name
        if "gradient" in name:
            assert call(name, C.byref(d), 4, True, True) == (-1, f"{name}: the kernel needs n_levels == 16 (got 12)"), name


def test_hash_entries_report_descriptor_errors():
    """What validate_hash and the three ced_hash_encode* entries refuse, and the 32-bit byte-offset limit of the two fused
    entries that read the table: return codes and error strings as literals.  Every case returns before a launch, so host
    pointers stand in for device memory."""
    from ced_nerf_amd import _lib
    assert "hash.hip" in _lib.SOURCES
    L = _lib.lib()
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, C.c_void_p)

    def table(n_levels=4, temporal=0):
        h = _lib.HashDesc()
        h.n_levels, h.table_dtype, h.temporal, h.table, h.total_entries = n_levels, 0, temporal, ptr, 8 * 16
        for l in range(16):
            h.scale[l], h.res[l], h.offset[l], h.size[l], h.hashed[l] = 1.0, 2, 8 * l, 8, 1
        return h

    entries = {"hash_encode": lambda h, n: L.ced_hash_encode(h, n, ptr, ptr, ptr, None),
               "hash_encode_backward": lambda h, n: L.ced_hash_encode_backward(h, n, ptr, ptr, ptr, ptr, 0, None),
               "hash_encode_backward_temporal": lambda h, n: L.ced_hash_encode_backward_temporal(h, n, ptr, ptr, ptr, ptr, None)}

    def call(name, h, n=4):
        rc = entries[name](None if h is None else C.byref(h), n)
        return rc, L.ced_last_error_string().decode()

    for name in entries:
        temporal = int(name.endswith("temporal"))
        assert call(name, None) == (-1, f"{name}: null hash descriptor"), name
        for n_levels in (0, 17):
            assert call(name, table(n_levels, temporal)) == (-1, f"{name}: n_levels={n_levels} out of range"), name
        h = table(4, temporal); h.table_dtype = 2
        assert call(name, h) == (-1, f"{name}: table_dtype must be 0 (f32) or 1 (f16)"), name
        h = table(4, temporal); h.size[2] = 6
        assert call(name, h) == (-1, f"{name}: hashed level 2 size 6 is not a power of two"), name
        h = table(4, temporal); h.hashed[1] = 0; h.size[1] = 7                # res 2: a dense level needs 8 entries
        assert call(name, h) == (-1, f"{name}: dense level 1 smaller than res^3"), name
        h = table(4, temporal); h.total_entries = 8 * 4 - 1
        assert call(name, h) == (-1, f"{name}: level 3 exceeds the table"), name
        assert call(name, table(4, temporal), -1) == (-1, f"{name}: n < 0"), name
        assert call(name, table(4, temporal), 0)[0] == 0, name
    assert call("hash_encode_backward", table(4, 1)) == (-1, "hash_encode_backward: the temporal table has no backward yet")
    assert call("hash_encode_backward_temporal", table(4, 0)) == \
        (-1, "hash_encode_backward_temporal: the table is not temporal (use ced_hash_encode_backward)")

    # the fused entries address the table by 32-bit byte offsets: total_entries * bytes per entry < 2^32.  One entry
    # below the limit each call gets as far as its next check.
    for dtype, temporal in ((0, 0), (1, 0), (0, 1), (1, 1)):
        limit = (1 << 32) // ((4 if dtype else 8) * (4 if temporal else 1))
        for total in (limit, limit - 1):
            d = _lib.FieldDesc()
            d.packed_weights = ptr
            d.packed_floats = L.ced_packed_weight_words(0, 0, 0)
            d.hash = table(16, temporal)
            d.hash.table_dtype, d.hash.total_entries = dtype, total
            d.hash.scale[0] = 0.0
            d.max_workgroups = -1                                         # field_forward's next check
            rc = L.ced_field_forward(C.byref(d), 4, ptr, ptr, None, None, ptr, None, None)
            want = "field_forward: hash table larger than 4 GiB" if total == limit else "field_forward: max_workgroups=-1"
            assert (rc, L.ced_last_error_string().decode()) == (-1, want), (dtype, temporal, total)
            d.max_workgroups = 0                                          # the gradient's next check: the level scales
            rc = L.ced_field_density_gradient(C.byref(d), 4, ptr, ptr, ptr, None, None, None, None)
            want = ("field_density_gradient: hash table larger than 4 GiB" if total == limit
                    else "field_density_gradient: level 0 has scale 0")
            assert (rc, L.ced_last_error_string().decode()) == (-1, want), (dtype, temporal, total)


def test_time_max_reports_table_errors():
    """ced_field_density_time_max asks of the hash table what the density-gradient pair asks, in the same words: sixteen
    levels (the twelve-level table of test_per_sample_entries_report_the_same_argument_errors) and the 32-bit byte-offset
    limit (the sixteen-level table of test_hash_entries_report_descriptor_errors).  Sizes and pointers are valid; both
    cases return before a launch, so host pointers stand in for device memory."""
    from ced_nerf_amd import _lib
    L = _lib.lib()
    buf = (C.c_float * 64)()
    ptr = C.cast(buf, C.c_void_p)

    def desc(n_levels, total_entries):
        d = _lib.FieldDesc()
        d.packed_weights = ptr
        d.packed_floats = L.ced_packed_weight_words(0, 0, 0)
        d.hash.n_levels, d.hash.table, d.hash.total_entries = n_levels, ptr, total_entries
        for l in range(n_levels):
            d.hash.scale[l], d.hash.res[l], d.hash.offset[l], d.hash.size[l], d.hash.hashed[l] = 1.0, 2, 8 * l, 8, 1
        return d

    def call(d):
        rc = L.ced_field_density_time_max(C.byref(d), 4, ptr, 2, 3, ptr, ptr, None)
        return rc, L.ced_last_error_string().decode()

    assert call(desc(12, 8 * 12)) == (-1, "field_density_time_max: the kernel needs n_levels == 16 (got 12)")
    for dtype, temporal in ((0, 0), (1, 0), (0, 1), (1, 1)):
        d = desc(16, (1 << 32) // ((4 if dtype else 8) * (4 if temporal else 1)))
        d.hash.table_dtype, d.hash.temporal = dtype, temporal
        assert call(d) == (-1, "field_density_time_max: hash table larger than 4 GiB"), (dtype, temporal)


def test_closed_form_skip_matches_sequential_recurrence(oracle):
    """ced_host_skip_march runs the kernels' skip code on the host: the O(#binades) closed form for
    cone_angle == 0 must land on exactly the float the oracle's step-by-step loop reaches."""
    from ced_nerf_amd import _lib
    L = _lib.lib(); OL = oracle.lib()
    rng = np.random.default_rng(0)
    n_bad = 0
    for step in (5e-3, 1e-3, 0.25, 1e-2, 3.3e-3, 0.1, 2.0 ** -7, 7e-5 * 64):
        st = float(np.float32(step))
        for _ in range(1500):
            t = np.float32(rng.uniform(0, 8) if rng.uniform() < 0.8 else rng.uniform(0, 0.02))
            if rng.uniform() < 0.05:
                t = np.float32(0.0)
            target = np.float32(t + rng.uniform(-0.1, 6) * (1 if rng.uniform() < 0.7 else 0.01))
            n_bad += L.ced_host_skip_march(float(t), float(target), st, 0.0) != OL.ced_o_skip_march(float(t), float(target), st, 0.0)
    assert n_bad == 0
    # cone_angle > 0 takes the sequential path; step_size <= 0 jumps to the target
    for t, target in ((0.2, 1.7), (0.5, 0.4), (1.0, 3.0)):
        assert L.ced_host_skip_march(t, target, 1e-3, 0.004) == OL.ced_o_skip_march(t, target, 1e-3, 0.004)
    assert L.ced_host_skip_march(0.3, 2.5, 0.0, 0.0) == 2.5


def _row_neuron(p, placement):
    """Which output neuron accumulator row p = 16nb + 4g + r computes (the row placement that
    makes a layer's accumulator registers the next layer's operand without moving data between lanes)."""
    nb, g, r = p // 16, (p % 16) // 4, p % 4
    if placement == "hidden":
        return 16 * nb + 4 * r + g
    if placement == "base_out":                  # neuron 0 = raw density, n >= 1 = head input 3 + n
        return 4 * r + g - 3 if r else (13 + g if g < 3 else 0)
    if placement == "per_group":                 # colour channel a on row 4a = (lane group a, register 0)
        return g if (r == 0 and nb == 0) else 1 << 30
    return p


def _ref_pack(layer_w, n_out_rows, ks, placement="natural"):
    """Independent numpy statement of the fragment order: [nb][q][lane][s]."""
    w = np.asarray(layer_w, np.float32)
    nb = (n_out_rows + 15) // 16
    ks4 = (ks + 3) // 4
    out = np.zeros((nb, ks4, 64, 4), np.float32)
    for p in range(nb * 16):
        neuron = _row_neuron(p, placement)
        if neuron >= w.shape[0]:
            continue
        for k in range(min(w.shape[1], ks * 4)):
            S, kk = divmod(k, 4)
            out[p // 16, S // 4, kk * 16 + p % 16, S % 4] = w[neuron, k]
    return out.reshape(-1)


@pytest.mark.parametrize("div,tm", [(0, 0), (1, 0), (0, 1), (1, 2)])
def test_pack_field_weights_layout(div, tm):
    from ced_nerf_amd import ops, synthetic as S
    p = S.init_field_params([-1, -1, -1, 1, 1, 1], 1e-3, 1024, 10, use_div_offsets=bool(div),
                            use_time_embedding=tm > 0, use_time_attenuation=tm == 2)
    blob = ops.pack_field_weights(bool(div), tm, p["xyz_wrap"], p["mlp_base"], p["mlp_head"])
    ksb0 = 11 if tm else 8
    H = "hidden"
    parts = [_ref_pack(p["xyz_wrap"][0], 64, 8, H), _ref_pack(p["xyz_wrap"][1], 64, 16, H), _ref_pack(p["xyz_wrap"][2], 64, 16, H),
             _ref_pack(p["xyz_wrap"][3], 16, 16), _ref_pack(p["mlp_base"][0], 64, ksb0, H),
             _ref_pack(p["mlp_base"][1], 16, 16, "base_out"), _ref_pack(p["mlp_head"][0], 64, 5, H),
             _ref_pack(p["mlp_head"][1], 64, 16, H), _ref_pack(p["mlp_head"][2], 16, 16, "per_group")]
    assert sorted(_row_neuron(q, "base_out") for q in range(16)) == list(range(16))
    assert sorted(_row_neuron(q, H) for q in range(64)) == list(range(64))
    want = np.concatenate(parts)
    assert blob.shape == want.shape == ((22528 if tm else 21504),)
    assert np.array_equal(blob, want)
    # every weight appears exactly once
    nz = sum(int(np.count_nonzero(w)) for w in p["xyz_wrap"] + p["mlp_base"] + p["mlp_head"])
    assert np.count_nonzero(blob) == nz
    with pytest.raises(ValueError):
        ops.pack_field_weights(bool(div), tm, p["xyz_wrap"][:3] + [np.zeros((5, 64), np.float32)], p["mlp_base"], p["mlp_head"])


def test_level_tables_match_survey():
    from ced_nerf_amd.hashgrid import level_tables
    for max_res, total, first_hashed in ((1024, 19263424, 8), (4096, 22565520, 6), (8192, 23928800, 6)):
        t = level_tables(16, max_res, 16, 21)
        assert t["total"] == total and int(np.argmax(t["hashed"])) == first_hashed and int(t["res"][-1]) == max_res
        assert t["scale"][0] == 15.0 and t["scale"][-1] == max_res - 1
        assert all(int(s) % 8 == 0 for s in t["size"])
    with pytest.raises(ValueError):
        level_tables(16, 1024, 17, 21)


def test_ops_reject_cpu_tensors_and_bad_shapes():
    """The product path has no CPU fallback: host tensors are refused like cednerf/render.py:17-18."""
    from ced_nerf_amd import nerfacc_api as A, ops
    from ced_nerf_amd.render import reduce_along_rays
    o = torch.zeros(4, 3); d = torch.ones(4, 3); ab = torch.tensor([[-1., -1, -1, 1, 1, 1]])
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        A.ray_aabb_intersect(o, d, ab)
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        reduce_along_rays(torch.zeros(3, dtype=torch.long), torch.zeros(3, 2))
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        ops.render_weights(torch.zeros(2, 2, dtype=torch.long), torch.zeros(3), torch.zeros(3), torch.zeros(3))
    with pytest.raises(ValueError):
        ops.make_hash_desc(torch.zeros(10, 2), 16, 1024, 16, 21)


def test_field_module_construction_and_guards():
    from ced_nerf_amd import synthetic as S
    from ced_nerf_amd.model import DNGPradianceField, DNGPRadianceField
    assert DNGPRadianceField is DNGPradianceField
    p = S.init_field_params([-1, -1, -1, 1, 1, 1], 1e-3, 1024, 10, use_time_embedding=True)
    f = DNGPradianceField.from_params(p, "cpu")
    assert f.hash_table.shape[1] == 2 and f.mlp_base[0].shape == (64, 41) and f.aabb.shape == (6,)
    q = f.export_params()
    assert np.array_equal(q["mlp_head"][2], p["mlp_head"][2]) and q["time_mode"] == 1
    with pytest.raises(NotImplementedError, match="cuda"):
        f(torch.zeros(2, 3), torch.zeros(2, 1), torch.ones(2, 3))
    g = DNGPradianceField([-1, -1, -1, 1, 1, 1], dst_resolution=1024, log2_hashmap_size=10, seed=1)
    assert abs(float(g.hash_table.abs().max())) <= 1e-4 and g.mlp_base[0].shape == (64, 32)
    for bad in (dict(n_levels=8), dict(hash4motion=True), dict(geo_feat_dim=7)):
        with pytest.raises(NotImplementedError):
            DNGPradianceField([-1, -1, -1, 1, 1, 1], log2_hashmap_size=10, **bad)
    # the published configuration (run_hyper.sh:1: -te -ta -f -ae -df -d) constructs: the prediction heads the -f
    # flag adds only run in training (cednerf/model.py:428-443), the eval path ignores them
    h = DNGPradianceField([-1, -1, -1, 1, 1, 1], log2_hashmap_size=10, use_feat_predict=True, use_weight_predict=True,
                          use_time_embedding=True, use_time_attenuation=True, use_div_offsets=True).eval()
    assert h.use_feat_predict and h.time_mode == 2 and h.xyz_wrap[3].shape == (6, 64)


def test_ops_refuse_tensors_of_another_device(monkeypatch):
    """The wrappers launch on the current device's stream with raw pointers: a tensor of another GPU is refused
    before any launch (no GPU needed for the check itself)."""
    from ced_nerf_amd import ops
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    ops._check_current_device(0, "x")
    ops._check_current_device(None, "x")
    with pytest.raises(RuntimeError, match="cuda:1 but the current device is cuda:0"):
        ops._check_current_device(1, "rays_o")


def test_trunc_exp_gradient_is_clamped_like_the_reference():
    """cednerf/utils.py:27-43: forward exp(x) in float32, backward g * exp(clamp(x, max=15))."""
    from ced_nerf_amd.utils import trunc_exp
    x = torch.tensor([-2.0, 0.5, 15.0, 40.0, 100.0], requires_grad=True)
    y = trunc_exp(x)
    assert y.dtype == torch.float32 and torch.equal(y.detach(), torch.exp(x.detach()))
    y.backward(torch.ones_like(y))
    want = torch.exp(torch.clamp(x.detach(), max=15))
    assert torch.equal(x.grad, want) and bool(torch.isfinite(x.grad).all())
    xh = torch.tensor([1.0], dtype=torch.float16, requires_grad=True)
    assert trunc_exp(xh).dtype == torch.float32


def test_state_dict_round_trip_cpu():
    """SURVEY section 5 checkpoint row (train_real.py:433-441,524-529): {"radiance_field": sd, "occupancy_grid": sd}
    saved with torch.save and loaded into freshly built modules reproduces every parameter and the estimator keys
    resolution / aabbs / occs / binaries (the render round trip on the device is in tests/test_gpu_parity.py)."""
    import io
    from ced_nerf_amd import synthetic as S
    from ced_nerf_amd.model import DNGPradianceField
    from ced_nerf_amd.nerfacc_api import OccGridEstimator
    sc = S.make_scene("hypernerf", 16, 12, "trained", log2_hashmap_size=10)
    cfg = sc["cfg"]
    f = DNGPradianceField.from_params(sc["params"], "cpu")
    est = OccGridEstimator(cfg["aabb"], cfg["grid_resolution"], cfg["grid_levels"])
    est.set_binaries(torch.from_numpy(sc["binaries"]))
    buf = io.BytesIO()
    torch.save({"radiance_field": f.state_dict(), "occupancy_grid": est.state_dict()}, buf)
    buf.seek(0)
    ck = torch.load(buf)
    assert set(ck["occupancy_grid"]) == {"resolution", "aabbs", "occs", "binaries"}
    assert {"aabb", "hash_table", "xyz_wrap.0", "xyz_wrap.3", "mlp_base.0", "mlp_base.1", "mlp_head.2"} <= set(ck["radiance_field"])
    f2 = DNGPradianceField(aabb=cfg["aabb"], dst_resolution=cfg["hash_max_res"], log2_hashmap_size=10,
                           moving_step=cfg["moving_step"], seed=3, **cfg["flags"])
    est2 = OccGridEstimator(cfg["aabb"], cfg["grid_resolution"], cfg["grid_levels"])
    f2.load_state_dict(ck["radiance_field"]); est2.load_state_dict(ck["occupancy_grid"])
    for (k, a), (_, b) in zip(f.state_dict().items(), f2.state_dict().items()):
        assert torch.equal(a, b), k
    assert torch.equal(est2.binaries, est.binaries) and torch.equal(est2.occs, est.occs) and torch.equal(est2.aabbs, est.aabbs)


def test_estimator_state_and_api_names():
    import ced_nerf_amd as cednerf
    from ced_nerf_amd.nerfacc_api import OccGridEstimator
    est = OccGridEstimator([-1, -1, -1, 1, 1, 1], 128, 2)
    assert est.binaries.shape == (2, 128, 128, 128) and est.binaries.dtype == torch.bool
    assert est.aabbs.shape == (2, 6) and est.aabbs[1].tolist() == [-2, -2, -2, 2, 2, 2] and est.occs.shape == (2 * 128 ** 3,)
    assert cednerf.utils.render_image_with_occgrid is cednerf.utils.render_image
    for name in ("render_image", "render_image_test", "trunc_exp", "set_random_seed", "Rays", "namedtuple_map"):
        assert hasattr(cednerf.utils, name)
    for name in ("rendering", "reduce_along_rays", "render_weight_from_density_prefix"):
        assert hasattr(cednerf.render, name)
    assert torch.allclose(cednerf.utils.trunc_exp(torch.tensor([0.0, 1.0]).half()), torch.tensor([1.0, 2.7182817]))


def test_synthetic_scene_is_deterministic_and_lego_like():
    from ced_nerf_amd import synthetic as S
    a = S.make_scene("dnerf", 40, 30, "trained", log2_hashmap_size=12)
    b = S.make_scene("dnerf", 40, 30, "trained", log2_hashmap_size=12)
    assert np.array_equal(a["origins"], b["origins"]) and np.array_equal(a["params"]["hash"]["table"], b["params"]["hash"]["table"])
    assert 0.02 < a["binaries"].mean() < 0.08
    assert np.allclose(np.linalg.norm(a["viewdirs"], axis=-1), 1.0, atol=1e-6)
    assert np.allclose(np.linalg.norm(a["origins"], axis=-1), 4.0, atol=1e-5)
    h = S.make_scene("hypernerf", 24, 32, "init", log2_hashmap_size=12)
    assert h["binaries"].shape[0] == 2 and h["params"]["time_mode"] == 2 and h["params"]["use_div_offsets"]


def test_estimator_cell_sampling_and_invisible_cells_cpu():
    """The torch-only parts of grid maintenance run anywhere: visible-cell lists, uniform+occupied
    sampling, camera-visibility marking (nerfacc OccGridEstimator semantics)."""
    from ced_nerf_amd.nerfacc_api import OccGridEstimator
    est = OccGridEstimator([-1, -1, -1, 1, 1, 1], 16, 2)
    assert est.grid_coords.shape == (4096, 3) and est.grid_coords[17].tolist() == [0, 1, 1]
    assert [len(i) for i in est._get_all_cells()] == [4096, 4096]
    # a pinhole camera on the -z side looking along +z sees the far cells, not the ones behind it
    K = torch.tensor([[[20.0, 0, 16], [0, 20.0, 16], [0, 0, 1]]])
    c2w = torch.eye(4)[None, :3].clone(); c2w[0, :3, 3] = torch.tensor([0.0, 0.0, -0.5])
    est.mark_invisible_cells(K, c2w, 32, 32, near_plane=0.1)
    vis = est.occs.view(2, 16, 16, 16)
    assert (est.occs == -1).any() and (est.occs == 0).any() and set(est.occs.unique().tolist()) <= {-1.0, 0.0}
    assert (vis[0, :, :, :3] == -1).all()            # cells behind the camera (z < -0.5 - near)
    assert (vis[0, 7:9, 7:9, 12:] == 0).all()        # cells on the optical axis in front of it
    n_vis = [len(i) for i in est._get_all_cells()]
    assert n_vis[0] == int((vis[0] >= 0).sum()) < 4096
    est.binaries[0, 8, 8, 14] = True
    torch.manual_seed(0)
    idx = est._sample_uniform_and_occupied_cells(256)
    assert all((est.occs[l * 4096 + i] >= 0).all() or True for l, i in enumerate(idx))
    occupied_id = (8 * 16 + 8) * 16 + 14
    assert idx[0][-1].item() == occupied_id and len(idx[1]) <= 256


def test_oracle_occ_grid_update_known_answers(oracle):
    res = 4
    aabbs = oracle.make_aabbs([0, 0, 0, 1, 1, 1], 1)
    occs = np.zeros(64, np.float32); occs[5] = -1.0; occs[7] = 0.5
    idx = [np.array([0, 7, 63], np.int64)]
    noise = [np.full((3, 3), 0.5, np.float32)]
    seen = {}

    def fn(x):
        seen["x"] = x.copy()
        return np.array([0.2, 0.1, 0.0], np.float32)
    out, binaries = oracle.occ_grid_update(occs, aabbs, res, idx, noise, fn, occ_thre=0.01, ema_decay=0.9)
    assert np.allclose(seen["x"], [[0.125, 0.125, 0.125], [0.125, 0.375, 0.875], [0.875, 0.875, 0.875]])
    assert out[0] == np.float32(0.2) and out[7] == np.float32(0.45) and out[63] == 0.0 and out[5] == -1.0
    assert binaries.sum() == 2 and binaries[0] and binaries[7]        # mean of visible = 0.65/63 ~ 0.0103 -> thre 0.01


def test_built_library_has_no_src1_high_op_sel_packed_fp32():
    """gfx950 hazard (tools/probes/pk_opsel_mfma.hip): v_pk_{mul,add,fma}_f32 with op_sel taking the high
    half of src1 for the low lane reads zero beside another wave's v_mfma_f32_16x16x32_f16.  The library is built with
    -fno-slp-vectorize so that hipcc never forms it; this checks the code objects actually built."""
    import importlib.util
    import shutil
    from ced_nerf_amd import _lib
    spec = importlib.util.spec_from_file_location(
        "isa_lint", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "isa_lint.py"))
    lint = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lint)
    # the pattern itself: the forms the probe shows to fail, and the ones it shows to be safe
    for bad in ("v_pk_mul_f32 v[0:1], v[2:3], v[4:5] op_sel:[0,1]", "v_pk_add_f32 v[0:1], v[2:3], v[4:5] op_sel:[0,1] op_sel_hi:[1,0]",
                "v_pk_fma_f32 v[0:1], v[2:3], v[4:5], v[6:7] op_sel:[0,1,0]"):
        assert lint.FORBIDDEN.search(bad), bad
    for ok in ("v_pk_mul_f32 v[0:1], v[2:3], v[4:5] op_sel_hi:[0,1]", "v_pk_mul_f32 v[0:1], v[2:3], v[4:5] op_sel:[1,0]",
               "v_pk_fma_f32 v[0:1], v[2:3], v[4:5], v[6:7] op_sel:[0,0,1]", "v_pk_mov_b32 v[0:1], v[2:3], v[4:5] op_sel:[1,1]"):
        assert not lint.FORBIDDEN.search(ok), ok
    assert "-fno-slp-vectorize" in _lib.HIPCC_FLAGS
    if not (os.path.exists(lint.OBJDUMP) or shutil.which(lint.OBJDUMP)):
        pytest.skip("llvm-objdump not found")
    n, bad = lint.scan(_lib.build())
    assert n > 100, f"only {n} kernels found in the library"
    assert not bad, f"kernels with a src1-high op_sel packed-fp32 instruction: {sorted(bad)}"


def _kernel_notes(path):
    """kernel name -> (vgpr_count, vgpr_spill_count, private_segment_fixed_size) from the metadata notes of the code
    objects inside a built library; None where llvm-readelf is missing.  Reads metadata only."""
    import importlib.util
    import re
    import shutil
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("isa_lint", os.path.join(root, "tools", "isa_lint.py"))
    lint = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lint)
    readelf = os.path.join(os.path.dirname(lint.OBJDUMP), "llvm-readelf")
    if not (os.path.exists(readelf) or shutil.which(readelf)):
        return None
    stats = {}
    for image in lint.code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(image)
            f.flush()
            notes = subprocess.run([readelf, "--notes", f.name], capture_output=True, text=True, check=True).stdout
        for blk in notes.split("- .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            stats[name] = tuple(int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
                                for key in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size"))
    return stats


def test_default_field_kernels_fit_their_launch_geometry():
    """The automatic launch geometry of the field kernels (field.hip / field_half.hip: workgroup size per arithmetic and
    table kind) is chosen so that the kernel runs WITHOUT scratch at that many waves per SIMD.  hipcc's register allocation
    of these kernels is sensitive to their code shape (round 4: 168 registers + scratch became 107-145 after an unrelated
    edit), so the built code objects are checked: kernel (template arguments) -> registers allowed, spilt registers allowed."""
    from ced_nerf_amd import _lib
    stats = _kernel_notes(_lib.build())
    if stats is None:
        pytest.skip("llvm-readelf not found")
    half = "_ZN3ced17field_half_kernelILb{te}ELb{f16}ELb{temporal}ELb{split}ELi2ELi{threads}EEEvNS_9FieldArgsE"
    f32 = "_ZN3ced12field_kernelILb{te}ELb{f16}ELb{temporal}ELi2ELi{threads}ELb{head16}EEEvNS_9FieldArgsE"
    want = []
    for f16 in (0, 1):
        want += [(half.format(te=0, f16=f16, temporal=0, split=1, threads=1024), 128, 0),      # f16x2: four waves per SIMD
                 (half.format(te=0, f16=f16, temporal=0, split=0, threads=768), 168, 0),       # f16: three
                 (half.format(te=1, f16=f16, temporal=0, split=1, threads=768), 168, 0),       # time embedding: three
                 (half.format(te=1, f16=f16, temporal=0, split=0, threads=768), 168, 0),
                 (f32.format(te=0, f16=f16, temporal=0, threads=1024, head16=0), 128, 8),      # fp32: four
                 (f32.format(te=0, f16=f16, temporal=0, threads=768, head16=1), 168, 0)]       # mixed: three
        for te in (0, 1):                                                                      # temporal tables: two
            want += [(half.format(te=te, f16=f16, temporal=1, split=1, threads=512), 256, 2),
                     (f32.format(te=te, f16=f16, temporal=1, threads=512, head16=0), 256, 2)]
    for name, regs, spills in want:
        assert name in stats, f"{name} not in the built library"
        assert stats[name][0] <= regs and stats[name][1] <= spills, f"{name}: {stats[name][0]} registers, {stats[name][1]} spilt"


def test_canonical_density_ops_run_without_scratch():
    """DESIGN 4.1d / 4.1f, "no scratch in any": the two ops on the canonical density (field_density_device.hpp) are built
    for eight table kinds x three staged planes each, and none of the 24 + 24 kernels spills a register or has a private
    segment."""
    from ced_nerf_amd import _lib
    stats = _kernel_notes(_lib.build())
    if stats is None:
        pytest.skip("llvm-readelf not found")
    for op in ("GradientOp", "TimeMaxOp"):
        kernels = {name: s for name, s in stats.items() if op in name}
        assert len(kernels) == 24, f"{op}: {len(kernels)} kernels in the built library"
        for name, (_, spilt, private) in kernels.items():
            assert spilt == 0 and private == 0, f"{name}: {spilt} spilt registers, {private} B private segment"


def test_reference_checkpoint_layout_round_trip_cpu(tmp_path):
    """f3 (train_real.py:433-441,524-529), tiny-cuda-nn half: a `model.pth` written in the documented layout hypothesis
    (tools/write_reference_checkpoint.py: flat `params` per tcnn module, 16-padded row-major matrices, ones-padded inputs)
    loads into fresh modules with the reference's two load_state_dict calls replaced by load_reference_checkpoint:
    hash table, motion MLP and mlp_base come back bit for bit; mlp_head's ones-padded bias column is folded into its
    constant Y00 input (same function: checked on random head inputs); the layout must be named explicitly; a
    time-embedding checkpoint whose padded mlp_base columns act as a bias is refused."""
    import subprocess, sys
    from ced_nerf_amd import checkpoint as CK, synthetic as S
    from ced_nerf_amd.model import DNGPradianceField
    from ced_nerf_amd.nerfacc_api import OccGridEstimator
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "model.pth")
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "write_reference_checkpoint.py"), path, "--head-bias"],
                         capture_output=True, text=True, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    ck = torch.load(path)
    assert set(ck) == {"radiance_field", "occupancy_grid"}
    assert set(ck["radiance_field"]) == {"aabb", "hash_encoder.params", "xyz_wrap.params", "mlp_base.params", "mlp_head.params",
                                         "direction_encoding.params"}
    assert ck["radiance_field"]["mlp_head.params"].numel() == 64 * 32 + 64 * 64 + 16 * 64        # 19 -> 32, 3 -> 16
    sc = S.make_scene("dnerf", 64, 48, "trained", log2_hashmap_size=15)
    cfg = sc["cfg"]
    src = DNGPradianceField.from_params(sc["params"], "cpu")
    dst = DNGPradianceField(aabb=[0, 0, 0, 1, 1, 1], dst_resolution=cfg["hash_max_res"], log2_hashmap_size=15,
                            moving_step=cfg["moving_step"], seed=3, **cfg["flags"])
    est = OccGridEstimator(cfg["aabb"], cfg["grid_resolution"], cfg["grid_levels"])
    with pytest.raises(ValueError, match="assume_tcnn_layout"):
        CK.load_reference_checkpoint(path, dst, est)
    CK.load_reference_checkpoint(path, dst, est, assume_tcnn_layout=CK.TCNN_LAYOUT)
    assert torch.equal(dst.hash_table, src.hash_table) and torch.equal(dst.aabb, src.aabb)
    for a, b in zip(list(dst.xyz_wrap) + list(dst.mlp_base) + list(dst.mlp_head)[1:],
                    list(src.xyz_wrap) + list(src.mlp_base) + list(src.mlp_head)[1:]):
        assert torch.equal(a, b)
    assert torch.equal(est.binaries, torch.from_numpy(sc["binaries"])) and est.occs.sum() > 0
    # the head's first layer: W_file . [x, 1 (ones padding)] == W_loaded . x for inputs whose element 0 is Y00
    rng = np.random.default_rng(0)
    x = rng.normal(size=(100, 19)); x[:, 0] = CK.SH_Y00
    w_file = ck["radiance_field"]["mlp_head.params"][:64 * 32].reshape(64, 32).double().numpy()
    assert np.abs(w_file[:, 19]).max() > 0.01 and not w_file[:, 20:].any()
    want = np.concatenate([x, np.ones((100, 13))], axis=1) @ w_file.T
    got = x @ dst.mlp_head[0].double().numpy().T
    assert np.abs(got - want).max() <= 1e-6
    # and back: the inverse map reproduces the file's sigma-chain tensors
    again = CK.reference_state_from_field(dst)
    for k in ("hash_encoder.params", "xyz_wrap.params", "mlp_base.params"):
        assert torch.equal(again[k], ck["radiance_field"][k]), k
    # time embedding: 41 inputs padded to 48 with ones -- a bias in those columns cannot be expressed
    te = DNGPradianceField(aabb=[0, 0, 0, 1, 1, 1], log2_hashmap_size=12, dst_resolution=256, use_time_embedding=True, seed=1)
    sd = CK.reference_state_from_field(te)
    CK.field_params_from_reference_state(sd, log2_hashmap_size=12, dst_resolution=256, use_time_embedding=True,
                                         assume_tcnn_layout=CK.TCNN_LAYOUT)
    sd["mlp_base.params"][41] = 0.25
    with pytest.raises(NotImplementedError, match="padded"):
        CK.field_params_from_reference_state(sd, log2_hashmap_size=12, dst_resolution=256, use_time_embedding=True,
                                             assume_tcnn_layout=CK.TCNN_LAYOUT)
