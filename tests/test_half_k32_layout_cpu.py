"""The f16x2 weight blob against the oracle's product blocks (no GPU).

oracle/cednerf_oracle.c: dense_half evaluates, per output, k-step and product term, four blocks of eight products:
block (half h, lane-group pair gp) holds inputs 32ks + 8g + e for g in {2gp, 2gp+1}, e in [4h, 4h + 4).  The pair form of
the kernel (two v_mfma_f32_16x16x16_f16) consumes exactly these for any placement; the single
v_mfma_f32_16x16x32_f16 consumes lane group q as block q, so the layers the f16x2 kernels without a time encoding run on
it (csrc/field_half.hip: half_kernel_k32) must find block (q >> 1, q & 1) in lane group q.  These tests rebuild, from
the packed blob alone, which weight and which activation meet in every product of every instruction.
"""
import numpy as np
import pytest

from ced_nerf_amd import _lib, ops

# HalfBlob<TE> (csrc/field_half.hip): name, first fragment, nb, ks, n_out, n_in, where the input comes from
# ("hidden:<layer>" = that layer's accumulators, else the input layer's column map)


def _layers(te, div):
    ksb0 = 2 if te else 1
    m0, m1, m2, m3 = 0, 4, 12, 20
    b0 = m3 + 2
    b1 = b0 + 4 * ksb0
    h0 = b1 + 2
    h1, h2 = h0 + 4, h0 + 12
    return [("m0", m0, 4, 1, 64, 32, "natural"), ("m1", m1, 4, 2, 64, 64, "hidden:m0"), ("m2", m2, 4, 2, 64, 64, "hidden:m1"),
            ("m3", m3, 1, 2, 6 if div else 3, 64, "hidden:m2"), ("b0", b0, 4, ksb0, 64, 41 if te else 32, "hash"),
            ("b1", b1, 1, 2, 16, 64, "hidden:b0"), ("h0", h0, 4, 1, 64, 19, "head"), ("h1", h1, 4, 2, 64, 64, "hidden:h0"),
            ("h2", h2, 1, 2, 3, 64, "hidden:h1")], h2 + 2


def _half_input_at(col, k, n_in):
    """oracle/cednerf_oracle.c: half_input_at"""
    g, e = (k % 32) // 8, k % 8
    i = k
    if col == "hash":
        i = 2 * (4 * (e >> 1) + g) + (e & 1) if k < 32 else (32 + 4 * e + g if e < 3 and 4 * e + g <= 8 else -1)
    elif col == "head":
        i = g if e == 0 else (4 + 4 * g + e - 1 if e <= 4 and 4 * g + e - 1 < 15 else -1)
    return i if 0 <= i < n_in else -1


def _pack(te, div, fill, table_dtype=0, temporal=False, pair_api=False):
    """blob of weights w[o][i] = fill(o, i) -> (hi plane, lo plane) as [frag][lane][8] float arrays"""
    layers, frags = _layers(te, div)
    mats = [np.fromfunction(fill, (n_out, n_in), dtype=np.float32).astype(np.float32) for _, _, _, _, n_out, n_in, _ in layers]
    if pair_api:
        L = _lib.lib()
        out = np.zeros(L.ced_packed_weight_words(int(div), int(te), _lib.MLP_F16X2), np.uint32)
        import ctypes as C
        _lib.check(L.ced_pack_field_weights_half(int(div), int(te), _lib.MLP_F16X2, *[m.ctypes.data_as(C.c_void_p) for m in mats],
                                                 out.ctypes.data_as(C.c_void_p)))
    else:
        out = ops.pack_field_weights(div, int(te), mats[:4], mats[4:6], mats[6:], _lib.MLP_F16X2, table_dtype, temporal)
    h = out.view(np.float16).astype(np.float32).reshape(2, frags, 64, 8)
    return h[0], h[1]


def _slots(te, div, **kw):
    """per layer: out[p][k] = output neuron, inp[p][k] = input index at (accumulator row p, operand position k); -1 = empty"""
    layers, _ = _layers(te, div)
    o_hi, _ = _pack(te, div, lambda o, i: o + 1, **kw)
    i_hi, i_lo = _pack(te, div, lambda o, i: i + 1 + 2.0 ** -12, **kw)
    res = {}
    for name, frag, nb, ks, n_out, n_in, src in layers:
        out = np.full((nb * 16, ks * 32), -1)
        inp = np.full((nb * 16, ks * 32), -1)
        for p in range(nb * 16):
            for k in range(ks * 32):
                f, lane, e = frag + (p // 16) * ks + k // 32, 16 * ((k % 32) // 8) + p % 16, k % 8
                if o_hi[f, lane, e] != 0:
                    out[p, k] = int(o_hi[f, lane, e]) - 1
                    inp[p, k] = int(i_hi[f, lane, e]) - 1
                    assert i_lo[f, lane, e] == 2.0 ** -12            # the remainder plane sits in the same slot
                else:
                    assert i_hi[f, lane, e] == 0 and i_lo[f, lane, e] == 0
        res[name] = (out, inp)
    return res


def _row_neuron(out):
    """accumulator row -> the neuron it computes (-1: padding row)"""
    rows = []
    for r in out:
        vals = set(r[r >= 0].tolist())
        assert len(vals) <= 1
        rows.append(vals.pop() if vals else -1)
    return rows


def _oracle_block(ks, half, gp, col, n_in):
    return [_half_input_at(col, 32 * ks + 8 * g + e, n_in) for g in (2 * gp, 2 * gp + 1) for e in range(4 * half, 4 * half + 4)]


def _check_blocks(te, div, k32, **kw):
    """every instruction's blocks of the blob the kernel reads are the oracle's blocks, in the oracle's order"""
    layers, _ = _layers(te, div)
    S = _slots(te, div, **kw)
    n_k32 = 0
    for name, frag, nb, ks, n_out, n_in, src in layers:
        out, inp = S[name]
        rows = _row_neuron(out)
        assert sorted(r for r in rows if r >= 0) == list(range(n_out)), name
        hidden = src.startswith("hidden:")
        col = "natural" if hidden else src
        prev_rows = _row_neuron(S[src[7:]][0]) if hidden else None
        single = k32 and hidden
        n_k32 += single
        for p in range(nb * 16):
            if rows[p] < 0:
                continue
            for s in range(ks):
                # what meets in position k: the weight's input index, and the activation the B operand carries there
                # (hidden inputs: lane group g, element e of k-step s is accumulator row 16(2s + e/4) + 4g + e%4 of the
                # previous layer -- to_operand_h; other inputs: the kernel computes input half_input_at(col, k) there)
                def act(k):
                    g, e = (k % 32) // 8, k % 8
                    return prev_rows[16 * (2 * s + (e >> 2)) + 4 * g + (e & 3)] if hidden else _half_input_at(col, k, n_in)
                for k in range(32 * s, 32 * s + 32):
                    if inp[p, k] >= 0:
                        assert inp[p, k] == act(k), (name, p, k)
                if single:
                    blocks = [[act(32 * s + 8 * q + e) for e in range(8)] for q in range(4)]
                else:                                   # (half, pair): the two 16x16x16, groups {0,1} then {2,3}
                    blocks = [[act(32 * s + 8 * g + e) for g in (2 * gp, 2 * gp + 1) for e in range(4 * h, 4 * h + 4)]
                              for h in range(2) for gp in range(2)]
                want = [_oracle_block(s, h, gp, col, n_in) for h in range(2) for gp in range(2)]
                assert blocks == want, (name, p, s, blocks, want)
    return S, n_k32


@pytest.mark.parametrize("div", [0, 1])
@pytest.mark.parametrize("te", [0, 1])
def test_f16x2_blob_blocks_are_the_oracles(te, div):
    k32 = not te                        # half_kernel_k32: the f16x2 kernels without a time encoding on a plain table
    S, n_k32 = _check_blocks(te, div, k32)
    assert n_k32 == (6 if k32 else 0)
    # the output rows other kernel code reads stay where they were: motion offsets (by __shfl), mlp_base outputs, colour
    P = _slots(te, div, pair_api=True)
    for name in ("m3", "b1", "h2"):
        assert np.array_equal(S[name][0], P[name][0]), name
    # and the pair layout of ced_pack_field_weights_half is itself the oracle's, for the pair form
    _check_blocks(te, div, False, pair_api=True)


@pytest.mark.parametrize("table_dtype,temporal", [(1, False), (0, True), (1, True)])
def test_f16x2_blob_of_other_tables(table_dtype, temporal):
    """fp16 tables take the K = 32 kernel too (same geometry); temporal tables keep the pair form and its layout"""
    k32 = not temporal
    _check_blocks(0, 1, k32, table_dtype=table_dtype, temporal=temporal)
    if not k32:
        for te in (0, 1):
            a = _pack(te, 1, lambda o, i: (o * 7 + i) % 13 - 6.3, table_dtype=table_dtype, temporal=temporal)
            b = _pack(te, 1, lambda o, i: (o * 7 + i) % 13 - 6.3, pair_api=True)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_f16_blob_is_the_pair_layout():
    """plain fp16 mode never runs the single instruction: its blob is ced_pack_field_weights_half's"""
    import ctypes as C
    rng = np.random.default_rng(3)
    layers, _ = _layers(False, False)
    mats = [rng.standard_normal((n_out, n_in)).astype(np.float32) for _, _, _, _, n_out, n_in, _ in layers]
    a = ops.pack_field_weights(False, 0, mats[:4], mats[4:6], mats[6:], _lib.MLP_F16)
    L = _lib.lib()
    b = np.zeros_like(a)
    _lib.check(L.ced_pack_field_weights_half(0, 0, _lib.MLP_F16, *[m.ctypes.data_as(C.c_void_p) for m in mats],
                                             b.ctypes.data_as(C.c_void_p)))
    assert np.array_equal(a, b)
