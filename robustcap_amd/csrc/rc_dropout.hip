// Dropout of a trainable sub-net (articulate/utils/torch/rnn.py:115,130-131: Dropout(p) on relu(linear1); torch.nn.LSTM(dropout=p) on
// layer 0's output as layer 1's input). One element-wise kernel, launched between the launches of rc_subnet_api.cpp.
//
// The mask is a function of (seed, call, site, the frame's row in the CALLER's order, unit) and nothing else: Philox4x32-10 (Random123's
// round function and constants) with key = (seed low, seed high) and counter = (row, unit >> 2, site, call); output lane j decides unit
// 4 (unit >> 2) + j. No mask is stored: the backward regenerates it, and how a call is cut into chunks and groups does not move it.
// A unit is kept iff its 32 bits are >= T = round(p 2^32); kept: x * 1 / (1 - p), dropped: +0.0f stored.
//
// A thread owns the four units of one Philox call, which are 16 contiguous bytes in both layouts (row-major with cols % 4 == 0, and
// rc_pk), and thread q owns bytes [16 q, 16 q + 16) of the matrix: one dwordx4 load and store per lane, 1 KiB contiguous per wave.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "rc_internal.h"
#include "rc_philox.h"

namespace {

// n4: 16-byte pieces of the matrix; c4 = cols / 4 (PK: ld / 4, ld % 16 == 0). PK: piece q of 16-row block q / (16 c4) is
// [k >> 4][(k >> 2) & 3][row & 15] (rc_pk), and rows from `rows` up to the block's end are left as they are.
template <bool PK>
__global__ void rc_dropout_kernel(const float* src, float* dst, long long n4, int c4, long long rows, const int* map, uint32_t site,
                                  uint32_t T, float scale, uint2 key, uint32_t call) {
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < n4; q += (long long)gridDim.x * 256) {
        long long j;
        uint32_t k4;
        if (PK) {
            const long long blk = q / (16ll * c4);
            const uint32_t rem = (uint32_t)(q - blk * 16ll * c4);
            j = blk * 16 + (rem & 15);
            k4 = (rem >> 6) * 4 + ((rem >> 4) & 3);
            if (j >= rows) continue;
        } else {
            j = q / c4;
            k4 = (uint32_t)(q - j * c4);
        }
        const uint32_t row = map ? (uint32_t)map[j] : (uint32_t)j;
        float4 v = reinterpret_cast<const float4*>(src)[q];
        const uint4 u = philox4x32_10(make_uint4(row, k4, site, call), key);
        v.x = u.x >= T ? v.x * scale : 0.0f;
        v.y = u.y >= T ? v.y * scale : 0.0f;
        v.z = u.z >= T ? v.z * scale : 0.0f;
        v.w = u.w >= T ? v.w * scale : 0.0f;
        reinterpret_cast<float4*>(dst)[q] = v;
    }
}

template <bool PK>
void launch(const float* src, float* dst, long long rows, int cols, const int* map, int site, const DropoutKey& k, hipStream_t s) {
    const long long n4 = (PK ? (rows + 15) / 16 * 16 : rows) * (cols / 4);
    if (n4 <= 0) return;
    const uint32_t T = (uint32_t)llrint((double)k.p * 4294967296.0);
    const float scale = (float)(1.0 / (1.0 - (double)k.p));
    const unsigned grid = (unsigned)std::min<long long>((n4 + 255) / 256, 2048);     // memory-bound: 8 blocks per CU, the rest by stride
    hipLaunchKernelGGL(rc_dropout_kernel<PK>, dim3(grid), dim3(256), 0, s, src, dst, n4, cols / 4, rows, map, (uint32_t)site, T, scale,
                       make_uint2((uint32_t)k.seed, (uint32_t)(k.seed >> 32)), k.call);
}

}  // namespace

void rc_launch_dropout_rows(const float* src, float* dst, long long rows, int cols, const int* map, int site, const DropoutKey& k,
                            hipStream_t s) {
    launch<false>(src, dst, rows, cols, map, site, k, s);
}

void rc_launch_dropout_pk(const float* src, float* dst, long long rows, int ld, const int* map, int site, const DropoutKey& k,
                          hipStream_t s) {
    launch<true>(src, dst, rows, ld, map, site, k, s);
}
