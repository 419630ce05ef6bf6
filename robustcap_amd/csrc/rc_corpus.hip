// The training corpus of one sub-net, formed on the device (rc_subnet_corpus in rc_subnet_api.cpp): the rows the eleven dataset builders of
// net/sig_mp.py:301-839 compute on the host from the {train,val}.pt dictionaries of preprocess.py -- root-frame or camera-frame IMU readings
// and joints, un-projected and bounding-box-normalised keypoints, root velocity and foot-contact stencils, global r6d poses.
//
// Every builder ends in [1:-1]: a sample of T frames gives T - 2 rows, row r is frame r + 1, and the stencils of rnn3 / rnn8 read frames r
// and r + 2 of the same sample -- the rows the reference pads (zeros, repeated end rows) are exactly the ones [1:-1] crops, so no padding row
// is ever formed. One wave per row, four rows per workgroup; the wave finds its sample by bisection in the table (tab: [n] first field frame
// of the sample's sequence | [n] first keypoint frame of the sample | [n + 1] first output row), forms the row in LDS and writes it out in
// 16-byte pieces where the destination allows (widths 141 and 171 are no multiple of four floats), predicated scalars at both ends:
// nothing is written past a row. No atomics: the same call gives the same bits.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "rc_internal.h"
#include "rc_device.h"

namespace {

enum { MODE_ROOT = 0, MODE_CAM = 1, MODE_WORLD = 2 };
enum { RNN2 = 0, RNN3 = 1, RNN4 = 2, RNN6 = 3, RNN7 = 4, RNN8 = 5 };        // kNets order

// sync_mp3d's overrides (net/sig_mp.py:504-515, :633-644; config.mp_joint_override): landmark row -> joint, -1: the landmark itself
__device__ __forceinline__ int override_joint(int row) {
    if (row >= 11 && row <= 16) return row + 5;
    switch (row) {
        case 23: return 1;
        case 24: return 2;
        case 25: return 4;
        case 26: return 5;
        case 27: return 7;
        case 28: return 8;
        default: return -1;
    }
}

// art.math.axis_angle_to_rotation_matrix (articulate/math/angular.py:221-233), the arithmetic of rc_aa2R_kernel (rc_frame.hip)
__device__ __forceinline__ void aa_to_R(const float* __restrict__ aa, float* R) {
    const float a[3] = {aa[0], aa[1], aa[2]};
    const float th = norm3(a);
    float k[3] = {a[0] / th, a[1] / th, a[2] / th};
#pragma unroll
    for (int q = 0; q < 3; ++q) if (!(fabsf(k[q]) <= 3.0e38f)) k[q] = 0.0f;          // NaN / inf -> 0
    const float c = cosf(th), sn = sinf(th), t = 1.0f - c;
    const float K[9] = {0.f, -k[2], k[1], k[2], 0.f, -k[0], -k[1], k[0], 0.f};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q) R[3 * r + q] = ((r == q ? c : 0.0f) + t * (k[r] * k[q])) + sn * K[3 * r + q];
}

// the sample of output row r
__device__ __forceinline__ int find_sample(const long long* __restrict__ out_off, int n, long long r) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (out_off[mid] <= r) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// a row of W floats out of LDS: scalars up to the destination's next 16-byte line, 16-byte pieces, scalars for what is left
__device__ __forceinline__ void store_row(const float* src, float* __restrict__ dst, int W, int lane) {
    const int head = min((int)(((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u) >> 2), W);
    const int n4 = (W - head) >> 2, done = head + 4 * n4;
    if (lane < head) dst[lane] = src[lane];
    for (int p = lane; p < n4; p += 64) {
        const float* s = src + head + 4 * p;
        *reinterpret_cast<float4*>(dst + head + 4 * p) = make_float4(s[0], s[1], s[2], s[3]);
    }
    if (lane < W - done) dst[done + lane] = src[done + lane];
}

// R^T v
__device__ __forceinline__ void rotT(const float* R, const float* v, float* o) {
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = (R[r] * v[0] + R[3 + r] * v[1]) + R[6 + r] * v[2];
}
// rows 0 .. 2 of a 3 x 4 transform (row stride 4) times (v, w)
__device__ __forceinline__ void rigid(const float* T, const float* v, float w, float* o) {
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = ((T[4 * r] * v[0] + T[4 * r + 1] * v[1]) + T[4 * r + 2] * v[2]) + T[4 * r + 3] * w;
}

template <int MODE>
__global__ __launch_bounds__(256) void rc_corpus_kernel(CorpusArgs a) {
    __shared__ float xs[4][240];
    __shared__ float ys[4][144];
    __shared__ float Gs[4][24][9];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + wave;
    if (r >= a.R) return;                                       // (waves only meet at wave-local barriers)
    const long long* out_off = a.tab + 2 * (long long)a.n;
    const int s = find_sample(out_off, a.n, r);
    const long long t = r - out_off[s];
    const long long f = a.tab[s] + t + 1;                       // the row's frame in the fields: never a sequence's first or last
    float* X = xs[wave];
    float* Y = ys[wave];
    float o[3];
    if (MODE == MODE_ROOT) {
        float Rm[9];
        aa_to_R(a.pose + f * 72, Rm);                           // R(root); Rrw = its transpose
        if (lane < 6) {                                         // accr = Rrw acc
            rotT(Rm, a.acc + (f * 6 + lane) * 3, o);
            X[3 * lane] = o[0]; X[3 * lane + 1] = o[1]; X[3 * lane + 2] = o[2];
        }
        if (lane < 18) {                                        // orir = Rrw ori, column c of IMU i; rnn7 leaves sensor 5 as it is
            const int i = lane / 3, c = lane - 3 * i;
            const float* m = a.ori + (f * 6 + i) * 9 + c;
            const float v[3] = {m[0], m[3], m[6]};
            if (a.net == RNN7 && i == 5) { o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; }
            else rotT(Rm, v, o);
            X[18 + 9 * i + c] = o[0]; X[18 + 9 * i + 3 + c] = o[1]; X[18 + 9 * i + 6 + c] = o[2];
        }
        float j[3] = {0.f, 0.f, 0.f};
        if (lane < 24) {
            const float* p = a.joint + (f * 24 + lane) * 3;
            if (a.amass) {                                      // (j - j0).bmm(R)
                const float* p0 = a.joint + f * 72;
                const float d[3] = {p[0] - p0[0], p[1] - p0[1], p[2] - p0[2]};
                rotT(Rm, d, j);
            } else {                                            // Rrw.matmul(j), the root subtracted afterwards
                rotT(Rm, p, j);
            }
        }
        const float r0 = __shfl(j[0], 0), r1 = __shfl(j[1], 0), r2 = __shfl(j[2], 0);
        if (lane >= 1 && lane < 24) {
            if (!a.amass) { j[0] -= r0; j[1] -= r1; j[2] -= r2; }
            float* d = (a.net == RNN2 ? Y : X + 72) + 3 * (lane - 1);
            d[0] = j[0]; d[1] = j[1]; d[2] = j[2];
        }
        if (a.net == RNN3 && lane == 0) {                       // Rrw ((j0[f + 1] - j0[f - 1]) 30 / vel_scale)
            const float* n = a.joint + (f + 1) * 72;
            const float* p = a.joint + (f - 1) * 72;
            const float v[3] = {(n[0] - p[0]) * 30.0f / 3.0f, (n[1] - p[1]) * 30.0f / 3.0f, (n[2] - p[2]) * 30.0f / 3.0f};
            rotT(Rm, v, o);
            Y[0] = o[0]; Y[1] = o[1]; Y[2] = o[2];
        }
        if (a.net == RNN8 && lane < 2) {                        // |(j[f + 1] - j[f - 1]) 30| < 0.25 of joints 10, 11
            const float* n = a.joint + ((f + 1) * 24 + 10 + lane) * 3;
            const float* p = a.joint + ((f - 1) * 24 + 10 + lane) * 3;
            const float v[3] = {(n[0] - p[0]) * 30.0f, (n[1] - p[1]) * 30.0f, (n[2] - p[2]) * 30.0f};
            Y[lane] = norm3(v) < 0.25f ? 1.0f : 0.0f;
        }
        if (a.net == RNN7) {                                    // r6d of forward_kinematics_R(pose with root := I)
            float Rl[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
            int lvl = -1, par = 0;
            if (lane >= 1 && lane < 24) {
                aa_to_R(a.pose + f * 72 + 3 * lane, Rl);
                lvl = a.body->level[lane];
                par = a.body->parent[lane];
            }
            float g[9];
#pragma unroll
            for (int q = 0; q < 9; ++q) g[q] = Rl[q];
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < 9; ++q) Gs[wave][0][q] = g[q];
            }
            rc_sync<true>();
            for (int l = 1; l < 24; ++l) {
                if (lvl == l) {
                    mat3_mul(Gs[wave][par], Rl, g);
#pragma unroll
                    for (int q = 0; q < 9; ++q) Gs[wave][lane][q] = g[q];
                }
                rc_sync<true>();
            }
            if (lane < 24) {
#pragma unroll
                for (int e = 0; e < 6; ++e) Y[6 * lane + e] = g[3 * (e % 3) + e / 3];
            }
        }
    } else if (MODE == MODE_CAM) {
        const float* cam = a.cams + 22ll * s;                   // K^-1 [9] | rows 0 .. 2 of T_cw [12] | occlusion sample
        const float* T = cam + 9;
        const bool occ = cam[21] != 0.0f;
        if (lane < 6) {                                         // accc = T_cw (acc; 0)
            rigid(T, a.acc + (f * 6 + lane) * 3, 0.0f, o);
            X[3 * lane] = o[0]; X[3 * lane + 1] = o[1]; X[3 * lane + 2] = o[2];
        }
        if (lane < 18) {                                        // oric = R_cw ori
            const int i = lane / 3, c = lane - 3 * i;
            const float* m = a.ori + (f * 6 + i) * 9 + c;
            const float v[3] = {m[0], m[3], m[6]};
            rigid(T, v, 0.0f, o);
            X[18 + 9 * i + c] = o[0]; X[18 + 9 * i + 3 + c] = o[1]; X[18 + 9 * i + 6 + c] = o[2];
        }
        float j[3] = {0.f, 0.f, 0.f};
        if (lane < 24) rigid(T, a.joint + (f * 24 + lane) * 3, 1.0f, j);     // j3dc = T_cw (j; 1)
        const float r0 = __shfl(j[0], 0), r1 = __shfl(j[1], 0), r2 = __shfl(j[2], 0);
        if (lane >= 1 && lane < 24) {
            float* d = (a.net == RNN4 ? Y : X + 171) + 3 * (lane - 1);
            d[0] = j[0] - r0; d[1] = j[1] - r1; d[2] = j[2] - r2;
        }
        if (a.net == RNN6 && lane == 0) {                       // tranc = T_cw (tran; 1)
            rigid(T, a.tran + f * 3, 1.0f, o);
            Y[0] = o[0]; Y[1] = o[1]; Y[2] = o[2];
        }
        const long long kf = a.tab[a.n + s] + t + 1;
        float x = 0.f, y = 0.f, cf = 0.f;
        if (lane < 33) {                                        // K^-1 (u W, v H, 1)
            const float* k = a.kp + (kf * 33 + lane) * 3;
            const float u = k[0] * a.sx, v = k[1] * a.sy;
            x = (cam[0] * u + cam[1] * v) + cam[2];
            y = (cam[3] * u + cam[4] * v) + cam[5];
            cf = k[2];
        }
        if (a.net == RNN4) {
            float xn, yn;
            bbox_normalise(x, y, lane, xn, yn);
            const float hx = __shfl(x, 23), hy = __shfl(y, 23);
            if (occ) {                                          // :480 divides the other tensor: relative to row 23, never scaled
                xn = lane != 23 ? x - hx : x;
                yn = lane != 23 ? y - hy : y;
            }
            x = xn;
            y = yn;
        }
        if (lane < 33) { X[72 + 3 * lane] = x; X[72 + 3 * lane + 1] = y; X[72 + 3 * lane + 2] = cf; }
    } else {
        const float* root = a.joint + a.tab[s] * 72;            // joint3d[0, 0] of the sequence
        const float q0 = root[0], q1 = root[1], q2 = root[2];
        for (int c = lane; c < 72; c += 64) X[c] = c < 18 ? a.acc[f * 18 + c] : a.ori[f * 54 + (c - 18)];
        if (lane < 33) {
            const int oj = override_joint(lane);
            const float* p = oj >= 0 ? a.joint + (f * 24 + oj) * 3 : a.mp + (f * 33 + lane) * 3;
            X[72 + 3 * lane] = p[0] - q0; X[72 + 3 * lane + 1] = p[1] - q1; X[72 + 3 * lane + 2] = p[2] - q2;
        }
        if (lane < 24) {
            const float* p = a.joint + (f * 24 + lane) * 3;
            Y[3 * lane] = p[0] - q0; Y[3 * lane + 1] = p[1] - q1; Y[3 * lane + 2] = p[2] - q2;
        }
    }
    rc_sync<true>();
    store_row(X, a.x + r * a.W, a.W, lane);
    store_row(Y, a.y + r * a.Wl, a.Wl, lane);
}

}  // namespace

void rc_launch_subnet_corpus(int mode, const CorpusArgs& a, hipStream_t s) {
    if (a.R <= 0 || a.n <= 0) return;
    const unsigned grid = (unsigned)((a.R + 3) / 4);
    if (mode == MODE_ROOT) hipLaunchKernelGGL(rc_corpus_kernel<MODE_ROOT>, dim3(grid), dim3(256), 0, s, a);
    else if (mode == MODE_CAM) hipLaunchKernelGGL(rc_corpus_kernel<MODE_CAM>, dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(rc_corpus_kernel<MODE_WORLD>, dim3(grid), dim3(256), 0, s, a);
}
