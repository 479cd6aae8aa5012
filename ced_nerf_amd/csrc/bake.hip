// Volume export (vis.py:13-46): the cells of a reso^3 grid over the field's bounding cube that are worth evaluating
// (ced_bake_candidates) and, of those, the ones whose density reaches the threshold (ced_bake_select).  The density in
// between is the existing ced_field_forward on the candidates' centres, so every arithmetic mode gives query_density's
// bits.  The colour afterwards is ced_field_rgb_bcast (field_move.hip).
//
// Both entries are stream compactions whose output order is the input order -- the flat cell index ascends -- by the
// count / scan / write scheme of keep.hpp.
#include "ced_common.hpp"
#include "keep.hpp"
#include "march_core.hpp"

namespace ced {

// Cell i = (ix * reso + iy) * reso + iz of the cube [lo, lo + reso * h]^3 (OccGridEstimator.grid_indices' order); centre
// p_a = lo_a + (i_a + 0.5) * h, fp32, multiply then add.
struct CandidateOp {
    int64_t first_cell;
    int reso;
    float lo[3], h;
    const uint8_t *binaries;          // [levels, res, res, res] or null: every cell is a candidate
    const float *aabbs;               // [levels, 6]
    int levels, res;
    int64_t *index;
    float *xyz;

    __device__ __forceinline__ void centre(int64_t i, float (&p)[3]) const
    {
        const int iz = (int)(i % reso), iy = (int)((i / reso) % reso), ix = (int)(i / ((int64_t)reso * reso));
        p[0] = lo[0] + ((float)ix + 0.5f) * h;
        p[1] = lo[1] + ((float)iy + 0.5f) * h;
        p[2] = lo[2] + ((float)iz + 0.5f) * h;
    }

    // The smallest level whose box contains the centre (faces included) decides, with the marcher's point-to-cell
    // expression (march_accel.hpp dda_setup: clamp((int)(((p - min) / extent) * res), 0, res - 1)).
    __device__ __forceinline__ bool keep(int64_t k) const
    {
        if (!binaries) return true;
        float p[3];
        centre(first_cell + k, p);
        const float resf = (float)res;
        for (int lvl = 0; lvl < levels; ++lvl) {
            const float *ab = aabbs + 6 * lvl;
            bool inside = true;
            int cell[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                inside = inside && p[a] >= ab[a] && p[a] <= ab[3 + a];
                const float ext = ab[3 + a] - ab[a];
                cell[a] = clampi((int)(((p[a] - ab[a]) / ext) * resf), 0, res - 1);
            }
            if (inside) return binaries[((int64_t)lvl * res + cell[0]) * res * res + (int64_t)cell[1] * res + cell[2]] != 0;
        }
        return false;
    }

    __device__ __forceinline__ void write(int64_t k, int64_t slot) const
    {
        float p[3];
        centre(first_cell + k, p);
        index[slot] = first_cell + k;
#pragma unroll
        for (int a = 0; a < 3; ++a) xyz[3 * slot + a] = p[a];
    }
};

// rows with sigma >= thresh (false for NaN), copied with what belongs to them
struct SelectOp {
    const int64_t *index_in;
    const float *xyz_in, *sigma_in, *emb_in;
    float thresh;
    int64_t *index;
    float *xyz, *sigma, *emb;

    __device__ __forceinline__ bool keep(int64_t k) const { return sigma_in[k] >= thresh; }

    __device__ __forceinline__ void write(int64_t k, int64_t slot) const
    {
        index[slot] = index_in[k];
#pragma unroll
        for (int a = 0; a < 3; ++a) xyz[3 * slot + a] = xyz_in[3 * k + a];
        sigma[slot] = sigma_in[k];
#pragma unroll
        for (int f = 0; f < 15; ++f) emb[15 * slot + f] = emb_in[15 * k + f];
    }
};

constexpr int kBakeMaxReso = 2048;                                 // reso^3 = 2^33 cells; (i + 0.5f) exact far beyond

}  // namespace ced

extern "C" int64_t ced_bake_workspace_bytes(int64_t n)
{
    if (n < 0) return -1;
    const int64_t nb = ced::keep_blocks(n);
    return (nb > 0 ? nb : 1) * (int64_t)sizeof(int64_t);
}

extern "C" int ced_bake_candidates(int32_t reso, const float *center_host, float radius, int64_t first_cell, int64_t n_cells,
                                   const uint8_t *binaries, const float *aabbs, int32_t levels, int32_t grid_res,
                                   int64_t capacity, int64_t *index, float *xyz, int64_t *count, void *workspace,
                                   int64_t workspace_bytes, void *stream)
{
    using namespace ced;
    CED_REQUIRE(reso >= 1 && reso <= kBakeMaxReso, "bake_candidates: reso=%d (1 .. %d)", reso, kBakeMaxReso);
    CED_REQUIRE(center_host != nullptr, "bake_candidates: null center");
    CED_REQUIRE(radius > 0.0f && radius < __builtin_inff(), "bake_candidates: radius=%g", (double)radius);
    const int64_t total = (int64_t)reso * reso * reso;
    CED_REQUIRE(first_cell >= 0 && n_cells >= 0 && first_cell <= total && n_cells <= total - first_cell,
                "bake_candidates: cells [%lld, +%lld) of %lld", (long long)first_cell, (long long)n_cells, (long long)total);
    CED_REQUIRE(capacity >= 0 && count != nullptr, "bake_candidates: capacity < 0 or null count");
    CED_REQUIRE(capacity == 0 || (index && xyz), "bake_candidates: null output");
    CED_REQUIRE(workspace && workspace_bytes >= ced_bake_workspace_bytes(n_cells), "bake_candidates: workspace too small");
    if (binaries)
        CED_REQUIRE(aabbs && levels >= 1 && grid_res >= 1 && grid_res <= 1024, "bake_candidates: grid levels=%d res=%d",
                    levels, grid_res);
    CandidateOp op{};
    op.first_cell = first_cell;
    op.reso = reso;
    for (int a = 0; a < 3; ++a) op.lo[a] = center_host[a] - radius;
    op.h = (2.0f * radius) / (float)reso;
    op.binaries = binaries; op.aabbs = aabbs; op.levels = levels; op.res = grid_res;
    op.index = index; op.xyz = xyz;
    return run_keep(op, n_cells, capacity, count, workspace, "bake_candidates", stream);
}

extern "C" int ced_bake_select(int64_t n, const int64_t *index_in, const float *xyz_in, const float *sigma_in,
                               const float *embedding_in, float sigma_thresh, int64_t capacity, int64_t *index, float *xyz,
                               float *sigma, float *embedding, int64_t *count, void *workspace, int64_t workspace_bytes,
                               void *stream)
{
    using namespace ced;
    CED_REQUIRE(n >= 0, "bake_select: n < 0");
    CED_REQUIRE(capacity >= 0 && count != nullptr, "bake_select: capacity < 0 or null count");
    CED_REQUIRE(n == 0 || sigma_in, "bake_select: null sigma");
    CED_REQUIRE(capacity == 0 || n == 0 || (index_in && xyz_in && embedding_in && index && xyz && sigma && embedding),
                "bake_select: null pointer");
    CED_REQUIRE(workspace && workspace_bytes >= ced_bake_workspace_bytes(n), "bake_select: workspace too small");
    SelectOp op{};
    op.index_in = index_in; op.xyz_in = xyz_in; op.sigma_in = sigma_in; op.emb_in = embedding_in;
    op.thresh = sigma_thresh;
    op.index = index; op.xyz = xyz; op.sigma = sigma; op.emb = embedding;
    return run_keep(op, n, capacity, count, workspace, "bake_select", stream);
}
