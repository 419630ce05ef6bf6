// Philox4x32-10 (Random123's round function and constants): the one definition behind every dropout mask of a trainable sub-net
// (rc_dropout.hip applies it element-wise; rc_wgrad.hip applies it while an operand tile is staged). Key = (seed low, seed high),
// counter = (row, unit >> 2, site, call); output lane j decides unit 4 (unit >> 2) + j.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += 0x9E3779B9u;
        k.y += 0xBB67AE85u;
    }
    return c;
}
