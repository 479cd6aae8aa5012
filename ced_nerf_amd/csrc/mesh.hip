// Triangle mesh of the density field at one time step: naive surface nets on the reso^3 lattice of cell centres (the
// definition is in include/cednerf_hip.h).  One vertex per cube whose 8 corners are neither all inside nor all outside
// (ced_mesh_vertices), one quad -- two triangles -- per sign-changing lattice edge with all four cubes around it
// (ced_mesh_faces).  No case table; fp32 throughout, one rounding per operation.
//
// Both entries are 0/1 compactions in ascending item order (cube id, edge key 3 * node + axis) by the count / scan / write
// scheme of keep.hpp, so vertex ids and the face order are the definition's and equal on every run; no atomics.  One
// thread per cube reads 8 floats, one thread per edge reads 2: no LDS tiling.
//
// A face finds its four vertex ids by BINARY SEARCH in the ascending `cube` array the vertex pass wrote: no extra
// memory (a dense int32 cube -> rank map would be 4 * reso^3 bytes, 512 MiB at reso 512, beside the 512 MiB lattice) at
// the price of <= 4 * 27 dependent 8-byte loads per ACTIVE edge, and only active edges search.
#include "ced_common.hpp"
#include "keep.hpp"

namespace ced {

constexpr int kMeshMaxReso = 512;                                  // 4 * reso^3 bytes of lattice: 512 MiB

struct MeshGrid {
    int reso;
    const float *S;                   // [reso^3]
    float thresh;

    __device__ __forceinline__ bool inside(float s) const { return s >= thresh; }              // false for a NaN

    __device__ __forceinline__ void coords(int64_t n, int (&i)[3]) const
    {
        i[2] = (int)(n % reso);
        i[1] = (int)((n / reso) % reso);
        i[0] = (int)(n / ((int64_t)reso * reso));
    }

    __device__ __forceinline__ int64_t stride(int a) const { return a == 2 ? 1 : (a == 1 ? (int64_t)reso : (int64_t)reso * reso); }
};

// items: every node as the lowest corner of a cube
struct VertexOp {
    MeshGrid g;
    float lo[3], h;
    float *vertices, *normals;        // [capacity, 3]
    int64_t *cube;                    // [capacity]

    // corners [x][y][z]; false when the node is the lowest corner of no cube
    __device__ __forceinline__ bool load(int64_t n, float (&s)[2][2][2]) const
    {
        int i[3];
        g.coords(n, i);
        if (i[0] >= g.reso - 1 || i[1] >= g.reso - 1 || i[2] >= g.reso - 1) return false;
        const int64_t r = g.reso, r2 = r * r;
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y)
#pragma unroll
                for (int z = 0; z < 2; ++z) s[x][y][z] = g.S[n + x * r2 + y * r + z];
        return true;
    }

    __device__ __forceinline__ bool keep(int64_t n) const
    {
        float s[2][2][2];
        if (!load(n, s)) return false;
        int in = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) in += g.inside(s[c >> 2][(c >> 1) & 1][c & 1]) ? 1 : 0;
        return in != 0 && in != 8;
    }

    __device__ __forceinline__ void write(int64_t n, int64_t slot) const
    {
        float s[2][2][2];
        load(n, s);
        float acc[3] = {0.0f, 0.0f, 0.0f}, grad[3] = {0.0f, 0.0f, 0.0f};
        int cnt = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int b = (a + 1) % 3, c = (a + 2) % 3;
#pragma unroll
            for (int ob = 0; ob < 2; ++ob)
#pragma unroll
                for (int oc = 0; oc < 2; ++oc) {
                    int p0[3], p1[3];
                    p0[a] = 0; p0[b] = ob; p0[c] = oc;
                    p1[a] = 1; p1[b] = ob; p1[c] = oc;
                    const float s0 = s[p0[0]][p0[1]][p0[2]], s1 = s[p1[0]][p1[1]][p1[2]];
                    const float d = s1 - s0;
                    grad[a] += d;
                    if (g.inside(s0) != g.inside(s1)) {
                        float mu = (g.thresh - s0) / d;
                        if (!(__builtin_fabsf(mu) < __builtin_inff())) mu = 0.5f;              // NaN or +-inf
                        mu = mu < 0.0f ? 0.0f : (mu > 1.0f ? 1.0f : mu);
                        float q[3];
                        q[a] = mu; q[b] = (float)ob; q[c] = (float)oc;
                        acc[0] += q[0]; acc[1] += q[1]; acc[2] += q[2];
                        cnt += 1;
                    }
                }
        }
        int i[3];
        g.coords(n, i);
        const float fc = (float)cnt;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float u = acc[a] / fc;
            vertices[3 * slot + a] = lo[a] + (((float)i[a] + 0.5f) + u) * h;
        }
        const float len = __builtin_sqrtf((grad[0] * grad[0] + grad[1] * grad[1]) + grad[2] * grad[2]);
        const bool ok = len > 0.0f && len < __builtin_inff();
#pragma unroll
        for (int a = 0; a < 3; ++a) normals[3 * slot + a] = ok ? -(grad[a] / len) : 0.0f;
        cube[slot] = n;
    }
};

// items: key = 3 * node + axis
struct FaceOp {
    MeshGrid g;
    const int64_t *cube;              // [n_vertices] ascending
    int64_t n_vertices;
    int32_t *faces;                   // [2 * capacity, 3]

    __device__ __forceinline__ bool keep(int64_t key) const
    {
        const int64_t n = key / 3;
        const int a = (int)(key - 3 * n), b = (a + 1) % 3, c = (a + 2) % 3;
        int i[3];
        g.coords(n, i);
        if (i[a] >= g.reso - 1 || i[b] < 1 || i[b] > g.reso - 2 || i[c] < 1 || i[c] > g.reso - 2) return false;
        return g.inside(g.S[n]) != g.inside(g.S[n + g.stride(a)]);
    }

    // rank of cube id `id` in cube[]; -1 if it is absent (a cube array that is not this lattice's)
    __device__ __forceinline__ int32_t rank_of(int64_t id) const
    {
        int64_t lo = 0, hi = n_vertices;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (cube[mid] < id) lo = mid + 1; else hi = mid;
        }
        return lo < n_vertices && cube[lo] == id ? (int32_t)lo : -1;
    }

    __device__ __forceinline__ void write(int64_t key, int64_t slot) const
    {
        const int64_t n = key / 3;
        const int a = (int)(key - 3 * n), b = (a + 1) % 3, c = (a + 2) % 3;
        const int64_t eb = g.stride(b), ec = g.stride(c);
        const int32_t q0 = rank_of(n - eb - ec), q1 = rank_of(n - ec), q2 = rank_of(n), q3 = rank_of(n - eb);
        int32_t *f = faces + 6 * slot;
        f[0] = q0; f[3] = q0;
        if (g.inside(g.S[n])) {
            f[1] = q1; f[2] = q2; f[4] = q2; f[5] = q3;
        } else {
            f[1] = q2; f[2] = q1; f[4] = q3; f[5] = q2;
        }
    }
};

}  // namespace ced

extern "C" int64_t ced_mesh_workspace_bytes(int32_t reso)
{
    if (reso < 1 || reso > ced::kMeshMaxReso) return -1;
    return ced::keep_blocks(3 * (int64_t)reso * reso * reso) * (int64_t)sizeof(int64_t);
}

extern "C" int ced_mesh_vertices(int32_t reso, const float *center_host, float radius, const float *lattice, float thresh,
                                 int64_t capacity, float *vertices, float *normals, int64_t *cube, int64_t *count,
                                 void *workspace, int64_t workspace_bytes, void *stream)
{
    using namespace ced;
    CED_REQUIRE(reso >= 1 && reso <= kMeshMaxReso, "mesh_vertices: reso=%d (1 .. %d)", reso, kMeshMaxReso);
    CED_REQUIRE(center_host != nullptr, "mesh_vertices: null center");
    CED_REQUIRE(radius > 0.0f && radius < __builtin_inff(), "mesh_vertices: radius=%g", (double)radius);
    CED_REQUIRE(lattice != nullptr, "mesh_vertices: null lattice");
    CED_REQUIRE(capacity >= 0 && count != nullptr, "mesh_vertices: capacity < 0 or null count");
    CED_REQUIRE(capacity == 0 || (vertices && normals && cube), "mesh_vertices: null output");
    CED_REQUIRE(workspace && workspace_bytes >= ced_mesh_workspace_bytes(reso), "mesh_vertices: workspace too small");
    VertexOp op{};
    op.g.reso = reso; op.g.S = lattice; op.g.thresh = thresh;
    for (int a = 0; a < 3; ++a) op.lo[a] = center_host[a] - radius;
    op.h = (2.0f * radius) / (float)reso;
    op.vertices = vertices; op.normals = normals; op.cube = cube;
    return run_keep(op, (int64_t)reso * reso * reso, capacity, count, workspace, "mesh_vertices", stream);
}

extern "C" int ced_mesh_faces(int32_t reso, const float *lattice, float thresh, const int64_t *cube, int64_t n_vertices,
                              int64_t capacity, int32_t *faces, int64_t *count, void *workspace, int64_t workspace_bytes,
                              void *stream)
{
    using namespace ced;
    CED_REQUIRE(reso >= 1 && reso <= kMeshMaxReso, "mesh_faces: reso=%d (1 .. %d)", reso, kMeshMaxReso);
    CED_REQUIRE(lattice != nullptr, "mesh_faces: null lattice");
    CED_REQUIRE(n_vertices >= 0 && n_vertices <= (int64_t)reso * reso * reso, "mesh_faces: n_vertices=%lld",
                (long long)n_vertices);
    CED_REQUIRE(capacity >= 0 && count != nullptr, "mesh_faces: capacity < 0 or null count");
    CED_REQUIRE(capacity == 0 || (faces && (cube || n_vertices == 0)), "mesh_faces: null pointer");
    CED_REQUIRE(workspace && workspace_bytes >= ced_mesh_workspace_bytes(reso), "mesh_faces: workspace too small");
    FaceOp op{};
    op.g.reso = reso; op.g.S = lattice; op.g.thresh = thresh;
    op.cube = cube; op.n_vertices = n_vertices; op.faces = faces;
    return run_keep(op, 3 * (int64_t)reso * reso * reso, capacity, count, workspace, "mesh_faces", stream);
}
