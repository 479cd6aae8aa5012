// Device-side reading of the hash grid's level table (field_args.hpp: HashLevels): a level's constants for the forward
// gather (hash_level, field_device.hpp), and the cell walk of the backward kernels (hash.hip).
#pragma once
#include "field_args.hpp"
#include "field_device.hpp"

namespace ced {

// A kernel that takes its argument block BY VALUE and indexes the table with a run-time level must not hand the block (or
// a part of it) to a function by reference: until the function is inlined the block's address has escaped, the compiler
// splits it into scalars one pass later, and the persistent field kernels come out with another register allocation.
// field_kernel / field_half_kernel therefore spell the five reads out; kernels that hold the block by reference
// (tile_kernel's ops) or index with constants (hash_encode_kernel) generate the same code either way and use this.
__device__ __forceinline__ LevelConst make_level(const HashLevels &lv, int l, uint32_t entry_bytes)
{
    return make_level(lv.scale[l], lv.res[l], lv.offset[l], lv.size[l], lv.hashed[l], entry_bytes);
}

// The cell of a level that holds a sample (x: its three raw coordinates): lower corner g, fraction fr, om = 1 - fr.
// floor and subtract, as hash_encoder_half.py:164-226 writes it; hash_level's truncate / fract form gives the same values.
__device__ __forceinline__ void hash_cell(const float *x, float sc, uint32_t (&g)[3], float (&fr)[3], float (&om)[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float xa = __builtin_fminf(__builtin_fmaxf(x[a], 0.0f), 1.0f);
        const float pos = xa * sc + 0.5f;
        const float fl = __builtin_floorf(pos);
        g[a] = (uint32_t)fl;
        fr[a] = pos - fl;
        om[a] = 1.0f - fr[a];
    }
}

// table entry of the corner (px, py, pz) of a level; the level's res / offset / size / hashed by value (see make_level)
__device__ __forceinline__ uint32_t hash_corner_entry(uint32_t px, uint32_t py, uint32_t pz, uint32_t res, uint32_t offset,
                                                      uint32_t size, bool hashed)
{
    const uint32_t idx = hashed ? (px ^ (py * kHashPrimeY) ^ (pz * kHashPrimeZ)) : (px + py * res + pz * res * res);
    return offset + idx % size;
}

}  // namespace ced
