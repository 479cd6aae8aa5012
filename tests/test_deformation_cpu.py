"""CPU suite: the deformation-field boundary (csrc/field_move.hip) -- the three entry points are declared, bound and
exported, their argument errors come back as codes, and the Python surface exists and refuses CPU tensors the way the
module's other methods do.  No kernel is launched here."""
import ctypes as C

import pytest
import torch

ENTRIES = ("ced_field_move", "ced_field_move_rays", "ced_field_rgb")


def test_header_declares_and_library_exports_the_entries():
    from ced_nerf_amd import _lib
    names = _lib.header_symbols()
    raw = C.CDLL(_lib.LIB_PATH)
    for n in ENTRIES:
        assert n in names, f"{n} not declared in include/cednerf_hip.h"
        assert n in _lib.PROTOTYPES, f"{n} not bound in _lib.PROTOTYPES"
        assert hasattr(raw, n), f"{n} declared but not exported by the built library"


def _desc(_lib, precision=0, time_mode=0):
    d = _lib.FieldDesc()
    d.mlp_precision = precision
    d.time_mode = time_mode
    d.packed_weights = 64                    # never dereferenced: every call below fails, or returns, before a launch
    d.packed_floats = int(_lib.lib().ced_packed_weight_words(0, time_mode, precision))
    return d


def test_argument_errors_are_codes_and_empty_input_is_a_no_op():
    from ced_nerf_amd import _lib
    L = _lib.lib()
    err = lambda: L.ced_last_error_string()
    for prec in range(4):
        d = _desc(_lib, prec, 2)
        assert L.ced_field_move(C.byref(d), 0, None, None, None, None, None, None, None) == 0
        assert L.ced_field_move_rays(C.byref(d), 0, None, None, None, None, None, None, None, 0, None, None, None) == 0
        assert L.ced_field_rgb(C.byref(d), 0, None, None, 1, None, None) == 0
    d = _desc(_lib)
    assert L.ced_field_move(None, 4, None, None, None, None, None, None, None) == -1 and b"field_move" in err()
    assert L.ced_field_move(C.byref(d), -1, None, None, None, None, None, None, None) == -1 and b"n < 0" in err()
    assert L.ced_field_move(C.byref(d), 4, None, None, None, None, None, None, None) == -1 and b"null" in err()
    # inputs given, no output asked for
    assert L.ced_field_move(C.byref(d), 4, 64, 64, None, None, None, None, None) == -1 and b"no output" in err()
    assert L.ced_field_move_rays(C.byref(d), 4, None, 64, 64, 64, 64, 64, 64, 0, None, None, None) == -1
    assert b"no output" in err()
    assert L.ced_field_move_rays(C.byref(d), 4, None, None, 64, 64, 64, 64, 64, 0, 64, None, None) == -1
    assert b"null pointer" in err()
    assert L.ced_field_rgb(C.byref(d), 4, 64, None, 1, 64, None) == -1 and b"field_rgb" in err()
    # a blob of another configuration is refused before anything is read
    d.packed_floats += 1
    assert L.ced_field_rgb(C.byref(d), 4, 64, 64, 1, 64, None) == -1 and b"packed_floats" in err()
    d = _desc(_lib)
    d.mlp_precision = 7
    assert L.ced_field_move(C.byref(d), 4, 64, 64, 64, None, None, None, None) == -1 and b"mlp_precision" in err()


def test_model_methods_refuse_cpu_tensors():
    from ced_nerf_amd.model import DNGPradianceField
    f = DNGPradianceField(aabb=[-1, -1, -1, 1, 1, 1], log2_hashmap_size=12, dst_resolution=64, seed=0)
    x, t = torch.zeros(5, 3), torch.zeros(5, 1)
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        f.query_move(x, t)
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        f.query_move(x, t, return_normalized=True)
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        f._query_rgb(torch.ones(5, 3), torch.zeros(5, 15))
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        f._query_rgb(torch.ones(5, 3), torch.zeros(5, 15), apply_act=False)
    assert callable(f.query_move_rays)


def test_ops_wrappers_refuse_cpu_tensors():
    from ced_nerf_amd import _lib, ops
    d = _desc(_lib)
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        ops.field_move(d, torch.zeros(3, 3), torch.zeros(3))
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        ops.field_rgb(d, torch.zeros(3, 3), torch.zeros(3, 15))
    with pytest.raises(NotImplementedError, match="Only support cuda inputs"):
        ops.field_move_rays(d, torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(3, dtype=torch.int64), torch.zeros(3),
                            torch.zeros(3), torch.zeros(1), False)


def test_refused_variants_stay_refused():
    from ced_nerf_amd.model import DNGPradianceField
    with pytest.raises(NotImplementedError, match="hash4motion"):
        DNGPradianceField(aabb=[-1, -1, -1, 1, 1, 1], log2_hashmap_size=12, dst_resolution=64, hash4motion=True)
    with pytest.raises(NotImplementedError, match="time_inject_before_sigma"):
        DNGPradianceField(aabb=[-1, -1, -1, 1, 1, 1], log2_hashmap_size=12, dst_resolution=64, time_inject_before_sigma=False)


def test_render_motion_and_the_video_keyword_exist():
    import inspect
    from ced_nerf_amd import utils, video
    sig = inspect.signature(utils.render_motion)
    for name in ("radiance_field", "estimator", "rays", "near_plane", "far_plane", "render_step_size", "cone_angle",
                 "alpha_thre", "test_chunk_size", "timestamps", "return_samples"):
        assert name in sig.parameters, name
    assert sig.parameters["test_chunk_size"].default == 8192 and sig.parameters["return_samples"].default is False
    assert "motion / opacity" in utils.render_motion.__doc__
    assert inspect.signature(video.render_video).parameters["motion"].default is False
