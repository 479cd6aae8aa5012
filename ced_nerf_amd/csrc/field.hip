// Host side of the fused dynamic-NGP radiance field: launch_field (validates a ced_field_desc, fills FieldArgs, picks the
// kernel for the arithmetic and table kind), the two entries on it, ced_field_forward and ced_field_forward_rays, the
// fp32 weight packer ced_pack_field_weights, and ced_set_option.  The kernel itself -- Frequency encoding -> motion MLP ->
// hash gather -> mlp_base -> trunc_exp -> SH(2) -> mlp_head in one launch -- and its execution shape are described in
// field_kernel.hpp; the hash grid's own entries are in hash.hip.
#include <atomic>
#include <cstring>

#include "ced_common.hpp"
#include "field_args.hpp"
#include "field_kernel.hpp"

namespace ced {

// Options of ced_set_option: process-wide, read by concurrently rendering threads -> atomics (relaxed: each is an
// independent launch property; no setting changes a result).
std::atomic<int> g_field_spread_tiles{ 2 };     // field kernels: tile -> wave mapping (field_device.hpp: field_tile_range)
std::atomic<int> g_frame_sh_per_ray{ 1 };       // frame renderers: FieldArgs::sh_ray from the per-ray set-up launch (0: per sample in the field kernel)
std::atomic<int> g_march_two_pass{ -1 };        // frame renderer: first iteration as culling pass + marching of the rest (-1: when there are several grid levels)

int launch_field(const ced_field_desc *d, FieldArgs &A, void *stream)
{
    int rc = validate_hash(&d->hash, "field_forward");
    if (rc) return rc;
    if (d->hash.n_levels != 16) {
        set_error("field_forward: the fused kernel needs n_levels == 16 (got %d)", d->hash.n_levels);
        return CED_E_UNSUPPORTED;
    }
    CED_REQUIRE(d->time_mode >= 0 && d->time_mode <= 2, "field_forward: time_mode=%d", d->time_mode);
    CED_REQUIRE(d->packed_weights != nullptr, "field_forward: null packed_weights");
    CED_REQUIRE(d->mlp_precision >= CED_MLP_F32 && d->mlp_precision <= CED_MLP_F32_HEAD16X2, "field_forward: mlp_precision=%d",
                d->mlp_precision);
    CED_REQUIRE((int64_t)d->packed_floats == ced_packed_weight_words(d->use_div_offsets, d->time_mode, d->mlp_precision),
                "field_forward: packed_floats=%llu does not match this configuration (mlp_precision %d)",
                (unsigned long long)d->packed_floats, d->mlp_precision);
    for (int i = 0; i < 6; ++i) A.aabb[i] = d->aabb[i];
    A.moving_step = d->moving_step;
    A.use_div = d->use_div_offsets ? 1 : 0;
    A.time_mode = d->time_mode;
    A.weights = d->packed_weights;
    A.table_dtype = d->hash.table_dtype;
    A.temporal = d->hash.temporal ? 1 : 0;
    A.table = d->hash.table;
    fill_levels(A.levels, d->hash);
    A.level_mode = hash_level_modes(d->hash, true);
    rc = require_32bit_byte_offsets(d->hash, "field_forward");
    if (rc) return rc;
    CED_REQUIRE(d->max_workgroups >= 0 && d->max_workgroups <= 65536, "field_forward: max_workgroups=%d", d->max_workgroups);
    A.max_blocks = d->max_workgroups;
    A.spread_tiles = g_field_spread_tiles;
    if (d->mlp_precision == CED_MLP_F32_HEAD16X2) return launch_field_mixed(A, d->time_mode, stream);
    if (d->mlp_precision != CED_MLP_F32) {
        // the half kernels gather level 4i + g in slot i: the same slot -> level-range mapping as above
        return launch_field_half(A, d->time_mode, d->mlp_precision, stream);
    }
    // 2 x 1024 threads (four waves per SIMD, 128 registers) since the dense levels' pair loads of round 4 (the kernels
    // fit without scratch: C2 +2.4 %, C3 +2 % over 768 threads); the temporal-table kernels need 250-300 registers and
    // run 2 x 512, two waves per SIMD, without scratch instead.
    switch ((d->time_mode ? 1 : 0) | (A.table_dtype ? 2 : 0) | (A.temporal ? 4 : 0)) {
    case 0: launch_field_grid<2, 1024>(field_kernel<false, false, false, 2, 1024>, A, stream); break;
    case 1: launch_field_grid<2, 1024>(field_kernel<true, false, false, 2, 1024>, A, stream); break;
    case 2: launch_field_grid<2, 1024>(field_kernel<false, true, false, 2, 1024>, A, stream); break;
    case 3: launch_field_grid<2, 1024>(field_kernel<true, true, false, 2, 1024>, A, stream); break;
    case 4: launch_field_grid<2, 512>(field_kernel<false, false, true, 2, 512>, A, stream); break;
    case 5: launch_field_grid<2, 512>(field_kernel<true, false, true, 2, 512>, A, stream); break;
    case 6: launch_field_grid<2, 512>(field_kernel<false, true, true, 2, 512>, A, stream); break;
    default: launch_field_grid<2, 512>(field_kernel<true, true, true, 2, 512>, A, stream); break;
    }
    return check_launch("field_forward");
}

// the nine layers' first words in the fp32 blob (ced_pack_field_weights)
template <bool TE> struct layer_offsets {
    using B = Blob<TE>;
    static constexpr int value[9] = { B::M0, B::M1, B::M2, B::M3, B::B0, B::B1, B::H0, B::H1, B::H2 };
};

}  // namespace ced

extern "C" int ced_set_option(const char *key, int value)
{
    CED_REQUIRE(key != nullptr, "set_option: null key");
    if (strcmp(key, "field_spread_tiles") == 0) {
        CED_REQUIRE(value >= 0 && value <= 2, "set_option: field_spread_tiles must be 0, 1 or 2 (field_tile_range)");
        ced::g_field_spread_tiles = value;
        return CED_OK;
    }
    if (strcmp(key, "march_two_pass") == 0) {
        CED_REQUIRE(value >= -1 && value <= 1, "set_option: march_two_pass must be -1 (automatic), 0 or 1");
        ced::g_march_two_pass = value;
        return CED_OK;
    }
    if (strcmp(key, "frame_sh_per_ray") == 0) {
        CED_REQUIRE(value == 0 || value == 1, "set_option: frame_sh_per_ray must be 0 or 1");
        ced::g_frame_sh_per_ray = value;
        return CED_OK;
    }
    if (strcmp(key, "hash_grad_blocks") == 0) {
        CED_REQUIRE(value >= 0 && value <= (1 << 20), "set_option: hash_grad_blocks must be 0 (no cap) .. 2^20");
        ced::g_hash_grad_blocks = value;
        return CED_OK;
    }
    ced::set_error("set_option: unknown key '%s'", key);
    return CED_E_INVALID;
}

extern "C" int64_t ced_packed_weight_floats(int use_div_offsets, int time_mode)
{
    (void)use_div_offsets;
    return time_mode ? ced::Blob<true>::TOTAL : ced::Blob<false>::TOTAL;
}

// Host-side reorder into MFMA A-fragment order: element (accumulator row p, input k) of a layer goes to
// [nb = p/16][q = (k/4)/4][lane = (k%4)*16 + p%16][s = (k/4)%4]; which neuron row p computes is the
// layer's placement (natural / hidden / base-out, below).
extern "C" int ced_pack_field_weights(int use_div_offsets, int time_mode, const float *m_w0, const float *m_w1,
                                      const float *m_w2, const float *m_w3, const float *b_w0, const float *b_w1,
                                      const float *h_w0, const float *h_w1, const float *h_w2, float *out)
{
    CED_REQUIRE(m_w0 && m_w1 && m_w2 && m_w3 && b_w0 && b_w1 && h_w0 && h_w1 && h_w2 && out,
                "pack_field_weights: null pointer");
    CED_REQUIRE(time_mode >= 0 && time_mode <= 2, "pack_field_weights: time_mode=%d", time_mode);
    const bool te = time_mode != 0;
    const int64_t total = ced_packed_weight_floats(use_div_offsets, time_mode);
    for (int64_t i = 0; i < total; ++i) out[i] = 0.0f;
    // placement: 0 natural, 1 hidden, 2 base-out, 3 one neuron per lane group (row 4a = neuron a)
    struct L { const float *w; int n_out, n_in, nb, ks, off; int placement; };
    const int base_in = te ? 41 : 32;
    const int n_mo = use_div_offsets ? 6 : 3;
    const int ksb0 = te ? 11 : 8;
    const int *offs = te ? ced::layer_offsets<true>::value : ced::layer_offsets<false>::value;
    const L layers[9] = {
        { m_w0, 64, 32, 4, 8, offs[0], 1 },      { m_w1, 64, 64, 4, 16, offs[1], 1 },
        { m_w2, 64, 64, 4, 16, offs[2], 1 },     { m_w3, n_mo, 64, 1, 16, offs[3], 0 },
        { b_w0, 64, base_in, 4, ksb0, offs[4], 1 }, { b_w1, 16, 64, 1, 16, offs[5], 2 },
        { h_w0, 64, 19, 4, 5, offs[6], 1 },      { h_w1, 64, 64, 4, 16, offs[7], 1 },
        { h_w2, 3, 64, 1, 16, offs[8], 3 },
    };
    for (const L &l : layers) {
        const int ks4 = ced::ks4_of(l.ks);
        for (int p = 0; p < l.nb * 16; ++p) {
            // which output neuron accumulator row p computes.  Hidden layers: row 16nb + 4g + r holds neuron
            // 16nb + 4r + g, so that the accumulator registers are the next layer's B operand as they are.
            int neuron = p;
            if (l.placement == 1) neuron = (p & ~15) | ((p & 3) << 2) | ((p >> 2) & 3);
            else if (l.placement == 2) neuron = ced::base_out_neuron(p);
            else if (l.placement == 3) neuron = (p & 3) ? l.n_out : (p >> 2);
            if (neuron >= l.n_out) continue;
            for (int k = 0; k < l.ks * 4; ++k) {
                if (k >= l.n_in) continue;
                const int S = k / 4, kk = k % 4;
                const int lane = kk * 16 + (p % 16);
                const int64_t idx = l.off + (((int64_t)(p / 16) * ks4 + S / 4) * 64 + lane) * 4 + (S % 4);
                out[idx] = l.w[(int64_t)neuron * l.n_in + k];
            }
        }
    }
    return CED_OK;
}

extern "C" int ced_field_forward(const ced_field_desc *desc, int64_t n, const float *positions, const float *t,
                                 const float *directions, float *rgb, float *sigma, float *geo, void *stream)
{
    CED_REQUIRE(desc != nullptr, "field_forward: null descriptor");
    CED_REQUIRE(n >= 0, "field_forward: n < 0");
    if (n == 0) return CED_OK;
    CED_REQUIRE(positions && t && sigma, "field_forward: null positions/t/sigma");
    CED_REQUIRE((directions != nullptr) == (rgb != nullptr), "field_forward: directions and rgb go together");
    ced::FieldArgs A{};
    A.n = n;
    A.pos = positions; A.t = t; A.dir = directions;
    A.rays_mode = 0; A.t_per_ray = 0; A.want_rgb = rgb ? 1 : 0;
    A.rgb = rgb; A.sigma = sigma; A.geo = geo;
    return ced::launch_field(desc, A, stream);
}

extern "C" int ced_field_forward_rays(const ced_field_desc *desc, int64_t n, const int64_t *n_dev,
                                      const float *rays_o, const float *rays_d, const int64_t *ray_indices, const float *t_starts, const float *t_ends,
                                      const float *timestamps, int32_t t_per_ray, int32_t want_rgb, float *rgb,
                                      float *sigma, void *stream)
{
    CED_REQUIRE(desc != nullptr, "field_forward_rays: null descriptor");
    CED_REQUIRE(n >= 0, "field_forward_rays: n < 0");
    if (n == 0) return CED_OK;
    CED_REQUIRE(rays_o && rays_d && ray_indices && t_starts && t_ends && timestamps && sigma,
                "field_forward_rays: null pointer");
    CED_REQUIRE(!want_rgb || rgb, "field_forward_rays: want_rgb without an rgb buffer");
    ced::FieldArgs A{};
    A.n = n;
    A.n_dev = n_dev;
    A.rays_o = rays_o; A.rays_d = rays_d; A.ray_idx = ray_indices;
    A.t0 = t_starts; A.t1 = t_ends; A.timestamps = timestamps;
    A.rays_mode = 1; A.t_per_ray = t_per_ray ? 1 : 0; A.want_rgb = want_rgb ? 1 : 0;
    A.rgb = rgb; A.sigma = sigma; A.geo = nullptr;
    return ced::launch_field(desc, A, stream);
}
