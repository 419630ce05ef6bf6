// One value into both device packings of a weight matrix; shared by the repack kernels (rc_subnet.hip) and the optimiser step (rc_optim.hip).
#pragma once
#include "rc_internal.h"

// fp32 v = hi + mid + lo exactly, each the top 16 bits of an fp32 (bf16 by truncation): the split of pack_weights_split (rc_api.cpp)
__device__ __forceinline__ void rc_split_bf16(float v, unsigned short& hi, unsigned short& mid, unsigned short& lo) {
    const unsigned uh = __float_as_uint(v) & 0xffff0000u;
    const float r1 = v - __uint_as_float(uh);
    const unsigned um = __float_as_uint(r1) & 0xffff0000u;
    const float r2 = r1 - __uint_as_float(um);
    hi = (unsigned short)(uh >> 16); mid = (unsigned short)(um >> 16); lo = (unsigned short)(__float_as_uint(r2) >> 16);
}

// value v of logical element (column n, k) of a matrix packed with Kp: into the fp32 pack W and the three bf16 planes Ws
__device__ __forceinline__ void rc_pack_store(float* W, unsigned short* Ws, int Kp, int n, int k, float v) {
    const int cb = n >> 4, j = n & 15;
    W[((((long long)cb * (Kp / RC_KC) + (k >> 4)) * 64 + ((k >> 2) & 3) * 16 + j) << 2) + (k & 3)] = v;
    const int kb = k >> 5, r = k & 31, lane = ((r & 15) >> 2) * 16 + j, e = (r >> 4) * 4 + (r & 3);
    const long long base = (((long long)cb * (Kp / 32) + kb) * 3) * 512 + lane * 8 + e;
    rc_split_bf16(v, Ws[base], Ws[base + 512], Ws[base + 1024]);
}
