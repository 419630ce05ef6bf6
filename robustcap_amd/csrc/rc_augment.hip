// The training batches of one sub-net, built on the device (rc_subnet_batch in rc_subnet_api.cpp): the samples a DataLoader would fetch with
// RNNDataset.__getitem__ (articulate/utils/torch/rnn.py:64-67) are gathered out of a resident corpus and augmented while they pass through
// registers -- the augment_fn of rnn3 / rnn6 / rnn7 / rnn8 (net/sig_mp.py:360-363, 578-581, 701-703, 792-795: torch.normal on the last 69
// columns, or on all of them) and the AMASS __getitem__ of rnn4 / rnn6 (:520-552, :649-679: random camera, random root translation,
// projection, confidence rows drawn from a pool without replacement, confidence-dependent keypoint noise, bounding-box normalisation).
//
// Every draw is Philox4x32-10 (rc_philox.h) with key = (seed low, seed high) and counter = (sample, frame, site | index << 8, call):
// `sample` is the sample's position in the batch, `frame` the frame within the sample, so a draw does not move when another sample's
// length changes or the launch is cut differently. Sites (dropout's are 0 and 1; its third counter word is never above 1):
//   2 NOISE   index = unit >> 2: the normals of augment_fn, unit counted from the first noisy column
//   3 CAMERA  frame 0, index 0: words 0, 1, 2 -> yaw, pitch, roll
//   4 TRAN    frame 0, index 0: words 0, 1, 2 -> the root translation
//   5 PERM    second counter word = the right half of the Feistel state, index = round: word 0 is the round function
//   6 KP      index = keypoint >> 1: the normals of the keypoint noise, unit = 2 keypoint + (0: x, 1: y)
// Uniforms: u = (w >> 8) 2^-24 in [0, 1) (torch.rand's grid); where 0 is excluded u = ((w >> 9) + 0.5) 2^-23. Normals: Box-Muller on the
// four words of one call -- units 4q, 4q + 1 = r cos(t), r sin(t) with r = sqrt(-2 ln u((w0 >> 9) + 0.5)), t = 2 pi u(w1 >> 8); units
// 4q + 2, 4q + 3 the same from (w2, w3). perm(f): a 4-round balanced Feistel network on m bits (m the smallest even number with 2^m >= P),
// (L, R) <- (R, L ^ (word 0 & (2^(m/2) - 1))), cycle-walked from f until the value is < P: a permutation of [0, P) by construction.
//
// A mixed batch (rc_subnet_batch_parts: plain and world samples of several corpora in one batch) runs the same kernels once per kind with
// a table `ext` (rc_internal.h) that gives every sample of the launch its position in the WHOLE batch -- the `sample` word above -- its
// first output frame there and its own corpus buffers; rc_subnet_batch passes none and keeps its bits.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

#include "rc_internal.h"
#include "rc_device.h"
#include "rc_philox.h"

namespace {

enum : uint32_t { SITE_NOISE = 2, SITE_CAMERA = 3, SITE_TRAN = 4, SITE_PERM = 5, SITE_KP = 6 };

struct Key { uint2 key; uint32_t call; };

__device__ __forceinline__ float u_closed0(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }              // [0, 1)
__device__ __forceinline__ float u_open(uint32_t w) { return ((float)(w >> 9) + 0.5f) * 0x1p-23f; }        // (0, 1)

__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float& z0, float& z1) {
    const float r = sqrtf(-2.0f * logf(u_open(wa)));
    float s, c;
    sincosf(6.283185307179586f * u_closed0(wb), &s, &c);
    z0 = r * c;
    z1 = r * s;
}

// the four normals of one call
__device__ __forceinline__ void normals4(uint32_t sample, uint32_t frame, uint32_t site, uint32_t q, const Key& k, float z[4]) {
    const uint4 w = philox4x32_10(make_uint4(sample, frame, site | (q << 8), k.call), k.key);
    box_muller(w.x, w.y, z[0], z[1]);
    box_muller(w.z, w.w, z[2], z[3]);
}

// tab: [n] first corpus frame of every sample | [n + 1] first output frame of every sample (and the total). The sample of output frame f.
__device__ __forceinline__ int find_sample(const long long* __restrict__ out_off, int n, long long f) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (out_off[mid] <= f) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ bool both16(const void* a, const void* b) { return ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0; }

// cnt <= 4 floats: one 16-byte piece where both sides are on the 16-byte grid, else predicated scalars -- nothing past src[cnt], dst[cnt]
__device__ __forceinline__ void copy4(const float* __restrict__ src, float* __restrict__ dst, int cnt) {
    if (cnt == 4 && both16(src, dst)) {
        *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < cnt) dst[k] = src[k];
    }
}

// kind "plain": per output frame nc pieces of copied columns [0, c0), nq Philox calls of noisy columns [c0, W), nl pieces of the label
__global__ __launch_bounds__(256) void rc_batch_plain_kernel(const float* __restrict__ data, const float* __restrict__ label,
                                                             const long long* __restrict__ tab, int n, long long F, int W, int Wl, int c0,
                                                             float sigma, Key key, float* __restrict__ x_out, float* __restrict__ l_out,
                                                             const long long* __restrict__ ext) {
    const long long* out_off = tab + n;
    const int nc = (c0 + 3) >> 2, nq = (W - c0 + 3) >> 2, nl = (Wl + 3) >> 2;
    const int ipr = nc + nq + nl;
    const long long total = F * ipr;
    for (long long item = (long long)blockIdx.x * 256 + threadIdx.x; item < total; item += (long long)gridDim.x * 256) {
        const long long f = item / ipr;
        const int j = (int)(item - f * ipr);
        const int s = find_sample(out_off, n, f);
        const long long t = f - out_off[s];
        const long long sf = tab[s] + t;
        const long long fo = ext ? ext[n + s] + t : f;                       // a mixed batch: the frame, the draws and the corpus of the
        const uint32_t pos = ext ? (uint32_t)ext[s] : (uint32_t)s;          // sample's place in the whole batch
        const float* data_s = ext ? reinterpret_cast<const float*>(ext[2 * (long long)n + s]) : data;
        const float* label_s = ext ? reinterpret_cast<const float*>(ext[3 * (long long)n + s]) : label;
        if (j < nc) {
            copy4(data_s + sf * W + 4 * j, x_out + fo * W + 4 * j, min(4, c0 - 4 * j));
        } else if (j < nc + nq) {
            const int q = j - nc, col = c0 + 4 * q, cnt = min(4, W - col);
            const float* src = data_s + sf * W + col;
            float* dst = x_out + fo * W + col;
            float z[4];
            normals4(pos, (uint32_t)t, SITE_NOISE, (uint32_t)q, key, z);
            if (cnt == 4 && both16(src, dst)) {
                float4 v = *reinterpret_cast<const float4*>(src);
                v.x += sigma * z[0]; v.y += sigma * z[1]; v.z += sigma * z[2]; v.w += sigma * z[3];
                *reinterpret_cast<float4*>(dst) = v;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < cnt) dst[k] = src[k] + sigma * z[k];
            }
        } else {
            const int jl = j - nc - nq;
            copy4(label_s + sf * Wl + 4 * jl, l_out + fo * Wl + 4 * jl, min(4, Wl - 4 * jl));
        }
    }
}

__device__ __forceinline__ void rot(const float* R, float x, float y, float z, float o[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = fmaf(R[3 * r + 2], z, fmaf(R[3 * r + 1], y, R[3 * r] * x));
}

// kind "world", per sample: cam[s] = Rcw [9] | t [3]. Rc0c = Ry(yaw) Rx(pitch) Rz(roll) (angular.py:205-218, 'YXZ' intrinsic) formed in
// double and rounded to fp32 once, Rcw = (diag(-1, -1, 1) Rc0c)^T; t = lerp((-1, -1, 3), (1, 1, 8), u) with t_z lowered by the minimum of
// the camera-frame z over every frame and all 24 joints of the sample (a wave tree, then the four waves in order: min is exact).
__global__ __launch_bounds__(256) void rc_batch_camera_kernel(const float* __restrict__ label, const long long* __restrict__ tab, int n,
                                                              BatchCamera range, Key key, float* __restrict__ cam,
                                                              const long long* __restrict__ ext) {
    __shared__ float Rs[9];
    __shared__ float red[4];
    const int s = blockIdx.x;
    const long long* out_off = tab + n;
    const long long T = out_off[s + 1] - out_off[s];
    const uint32_t pos = ext ? (uint32_t)ext[s] : (uint32_t)s;
    if (threadIdx.x == 0) {
        const uint4 w = philox4x32_10(make_uint4(pos, 0u, SITE_CAMERA, key.call), key.key);
        const double rad = 3.14159265358979323846 / 180.0;
        const double uy = (double)u_closed0(w.x), up = (double)u_closed0(w.y), ur = (double)u_closed0(w.z);
        const double ay = ((double)range.yaw_lo * (1.0 - uy) + (double)range.yaw_hi * uy) * rad;
        const double ap = ((double)range.pitch_lo * (1.0 - up) + (double)range.pitch_hi * up) * rad;
        const double ar = ((double)range.roll_lo * (1.0 - ur) + (double)range.roll_hi * ur) * rad;
        const double cy = cos(ay), sy = sin(ay), cp = cos(ap), sp = sin(ap), cr = cos(ar), sr = sin(ar);
        const float M[9] = {(float)(cy * cr + sy * sp * sr), (float)(-cy * sr + sy * sp * cr), (float)(sy * cp),
                            (float)(cp * sr),                (float)(cp * cr),                 (float)(-sp),
                            (float)(-sy * cr + cy * sp * sr), (float)(sy * sr + cy * sp * cr), (float)(cy * cp)};
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) Rs[3 * i + j] = j < 2 ? -M[3 * j + i] : M[3 * j + i];     // Rcw[i][j] = (D Rc0c)[j][i]
    }
    __syncthreads();
    float R[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = Rs[q];
    const float* joints = (ext ? reinterpret_cast<const float*>(ext[3 * (long long)n + s]) : label) + tab[s] * 72;
    float zmin = __builtin_inff();
    for (long long g = threadIdx.x; g < T * 24; g += 256) {
        float o[3];
        rot(R, joints[3 * g], joints[3 * g + 1], joints[3 * g + 2], o);
        zmin = fminf(zmin, o[2]);
    }
    zmin = wave_min(zmin);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = zmin;
    __syncthreads();
    if (threadIdx.x == 0) {
        zmin = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
        const uint4 w = philox4x32_10(make_uint4(pos, 0u, SITE_TRAN, key.call), key.key);
        const float u0 = u_closed0(w.x), u1 = u_closed0(w.y), u2 = u_closed0(w.z);
        float* c = cam + 12ll * s;
#pragma unroll
        for (int q = 0; q < 9; ++q) c[q] = R[q];
        c[9] = -1.0f * (1.0f - u0) + 1.0f * u0;
        c[10] = -1.0f * (1.0f - u1) + 1.0f * u1;
        c[11] = (3.0f * (1.0f - u2) + 8.0f * u2) - zmin;
    }
}

// perm(f) of sample s: the Feistel network of the header comment on 2 h bits, walked until the value is a row of the pool
__device__ __forceinline__ uint32_t pool_row(uint32_t s, uint32_t f, uint32_t P, int h, const Key& k) {
    const uint32_t mask = (1u << h) - 1u;
    uint32_t x = f;
    do {
        uint32_t L = x >> h, R = x & mask;
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
            const uint32_t fr = philox4x32_10(make_uint4(s, R, SITE_PERM | (r << 8), k.call), k.key).x & mask;
            const uint32_t nr = L ^ fr;
            L = R;
            R = nr;
        }
        x = (L << h) | R;
    } while (x >= P);
    return x;
}

// kind "world", per frame: one wave, lanes 0 .. 32 the landmarks (0 .. 23 also the joints, 0 .. 17 the IMU columns). Four frames per workgroup.
// RNN4: x = accc | oric | bbox-normalised j2dc (171), label = j3dc[1:] - j3dc[:1] (69). Else rnn6: x = accc | oric | raw j2dc |
// (j3dc[1:] - j3dc[:1]) + 0.03 z (240), label = j3dc[:, 0] after the translation (3).
template <bool RNN4>
__global__ __launch_bounds__(256) void rc_batch_world_kernel(const float* __restrict__ data, const float* __restrict__ label,
                                                             const long long* __restrict__ tab, int n, long long F,
                                                             const float* __restrict__ cam, const float* __restrict__ pool, uint32_t P, int h,
                                                             float sigma, Key key, float* __restrict__ x_out, float* __restrict__ l_out,
                                                             const long long* __restrict__ ext) {
    constexpr int WOUT = RNN4 ? 171 : 240, WL = RNN4 ? 69 : 3;
    __shared__ float rel[4][72];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long fq = (long long)blockIdx.x * 4 + wave;
    const bool live = fq < F;                                   // a wave past the end works on the last frame and stores nothing
    const long long f = live ? fq : F - 1;
    const long long* out_off = tab + n;
    const int s = find_sample(out_off, n, f);
    const long long t = f - out_off[s];
    const long long sf = tab[s] + t;
    float R[9], tr[3];
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = cam[12ll * s + q];
#pragma unroll
    for (int q = 0; q < 3; ++q) tr[q] = cam[12ll * s + 9 + q];
    const long long fo = ext ? ext[n + s] + t : f;
    const uint32_t pos = ext ? (uint32_t)ext[s] : (uint32_t)s;
    const float* row = (ext ? reinterpret_cast<const float*>(ext[2 * (long long)n + s]) : data) + sf * 171;
    const float* lab = (ext ? reinterpret_cast<const float*>(ext[3 * (long long)n + s]) : label) + sf * 72;
    float* xo = x_out + fo * WOUT;
    float* lo = l_out + fo * WL;
    float o[3];
    if (lane < 6) {                                             // accc = Rcw acc
        rot(R, row[3 * lane], row[3 * lane + 1], row[3 * lane + 2], o);
        if (live) { xo[3 * lane] = o[0]; xo[3 * lane + 1] = o[1]; xo[3 * lane + 2] = o[2]; }
    }
    if (lane < 18) {                                            // oric = Rcw ori: column c of IMU i
        const int i = lane / 3, c = lane - 3 * i;
        const float* m = row + 18 + 9 * i + c;
        rot(R, m[0], m[3], m[6], o);
        if (live) { xo[18 + 9 * i + c] = o[0]; xo[18 + 9 * i + 3 + c] = o[1]; xo[18 + 9 * i + 6 + c] = o[2]; }
    }
    float j[3] = {0.f, 0.f, 0.f};
    if (lane < 24) {                                            // j3dc = Rcw j3dw + t
        rot(R, lab[3 * lane], lab[3 * lane + 1], lab[3 * lane + 2], j);
        j[0] += tr[0]; j[1] += tr[1]; j[2] += tr[2];
    }
    const float r0 = __shfl(j[0], 0), r1 = __shfl(j[1], 0), r2 = __shfl(j[2], 0);
    float x = 0.f, y = 0.f, p = 0.f;
    const uint32_t prow = pool_row(pos, (uint32_t)t, P, h, key);
    if (lane < 33) {                                            // j2dc = (Rcw j3dw_mp + t) / z, then the confidence row and its noise
        rot(R, row[72 + 3 * lane], row[72 + 3 * lane + 1], row[72 + 3 * lane + 2], o);
        o[0] += tr[0]; o[1] += tr[1]; o[2] += tr[2];
        x = o[0] / o[2];
        y = o[1] / o[2];
        p = pool[(long long)prow * 33 + lane];
        float z[4];
        normals4(pos, (uint32_t)t, SITE_KP, (uint32_t)(lane >> 1), key, z);
        const float sd = 0.003f * (1.0f - p);
        x += sd * ((lane & 1) ? z[2] : z[0]);
        y += sd * ((lane & 1) ? z[3] : z[1]);
    }
    if (RNN4) {
        float xn, yn;
        bbox_normalise(x, y, lane, xn, yn);
        if (live && lane < 33) { xo[72 + 3 * lane] = xn; xo[72 + 3 * lane + 1] = yn; xo[72 + 3 * lane + 2] = p; }
        if (live && lane >= 1 && lane < 24) {
            lo[3 * (lane - 1)] = j[0] - r0; lo[3 * (lane - 1) + 1] = j[1] - r1; lo[3 * (lane - 1) + 2] = j[2] - r2;
        }
    } else {
        if (live && lane < 33) { xo[72 + 3 * lane] = x; xo[72 + 3 * lane + 1] = y; xo[72 + 3 * lane + 2] = p; }
        if (live && lane == 0) { lo[0] = j[0]; lo[1] = j[1]; lo[2] = j[2]; }
        if (lane >= 1 && lane < 24) {
            rel[wave][3 * (lane - 1)] = j[0] - r0; rel[wave][3 * (lane - 1) + 1] = j[1] - r1; rel[wave][3 * (lane - 1) + 2] = j[2] - r2;
        }
        __syncthreads();
        if (lane < 18) {                                        // the ("tail", 69) noise of augment_fn: lane q owns units 4q .. 4q + 3
            float z[4];
            normals4(pos, (uint32_t)t, SITE_NOISE, (uint32_t)lane, key, z);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int u = 4 * lane + k;
                if (live && u < 69) xo[171 + u] = rel[wave][u] + sigma * z[k];
            }
        }
    }
}

}  // namespace

void rc_launch_batch_plain(const float* data, const float* label, const long long* tab, int n, long long F, int W, int Wl, int c0,
                           float sigma, const BatchKey& k, float* x_out, float* l_out, hipStream_t s, const long long* ext) {
    const int ipr = (c0 + 3) / 4 + (W - c0 + 3) / 4 + (Wl + 3) / 4;
    const long long total = F * ipr;
    if (total <= 0) return;
    const unsigned grid = (unsigned)std::min<long long>((total + 255) / 256, 4096);   // 16 blocks per CU, the rest by stride
    const Key key{make_uint2((uint32_t)k.seed, (uint32_t)(k.seed >> 32)), k.call};
    hipLaunchKernelGGL(rc_batch_plain_kernel, dim3(grid), dim3(256), 0, s, data, label, tab, n, F, W, Wl, c0, sigma, key, x_out, l_out,
                       ext);
}

void rc_launch_batch_world(int rnn4, const float* data, const float* label, const long long* tab, int n, long long F,
                           const BatchCamera& range, float* cam, const float* pool, int pool_rows, float sigma, const BatchKey& k,
                           float* x_out, float* l_out, hipStream_t s, const long long* ext) {
    if (F <= 0 || n <= 0) return;
    const Key key{make_uint2((uint32_t)k.seed, (uint32_t)(k.seed >> 32)), k.call};
    int m = 0;
    while ((1ll << m) < pool_rows) m += 2;
    hipLaunchKernelGGL(rc_batch_camera_kernel, dim3((unsigned)n), dim3(256), 0, s, label, tab, n, range, key, cam, ext);
    const unsigned grid = (unsigned)((F + 3) / 4);
    if (rnn4)
        hipLaunchKernelGGL(rc_batch_world_kernel<true>, dim3(grid), dim3(256), 0, s, data, label, tab, n, F, cam, pool, (uint32_t)pool_rows,
                           m / 2, sigma, key, x_out, l_out, ext);
    else
        hipLaunchKernelGGL(rc_batch_world_kernel<false>, dim3(grid), dim3(256), 0, s, data, label, tab, n, F, cam, pool, (uint32_t)pool_rows,
                           m / 2, sigma, key, x_out, l_out, ext);
}
