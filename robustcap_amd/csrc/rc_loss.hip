// The reference's training objectives of the six sub-nets on the device (rc_subnet_loss; articulate/utils/torch/train.py:117,
// `loss = loss_fn(net(d), l)`, with the loss functions of net/sig_mp.py:340,409-418,555,683,749-771,829-831): from x [F, W] (the
// sub-net's output over the concatenated batch) and y [F, W] (the labels) the value as one device float and dx = d value / d x.
// Host side: rc_api.cpp.
//
// Arithmetic: every difference, product and sum that enters the VALUE is formed in double on the fp32 inputs and the value is rounded to
// fp32 once; dx is the closed-form gradient, formed in double from the same quantities and rounded once per element. Every divisor
// (F W, 3 (F // w), 72 F) comes from the host as a double reciprocal, so dx never waits for a sum.
//
// Sums: a workgroup owns units u = blockIdx.x, blockIdx.x + gridDim.x, ... (a unit: RC_LOSS_CHUNK elements | RC_LOSS_WINDOW_FRAMES frames
// counted from the END of the batch | RC_LOSS_POSE_FRAMES frames), every thread adds its terms into one double in a fixed order, the 256
// doubles are added in a fixed tree and stored as one partial; rc_loss_finish_kernel adds the at most RC_LOSS_MAX_PARTIALS partials in
// index order. No atomics: two runs give the same bits.
//
// The validation metric (rc_subnet_eval; train.py:94-101,124-131, `sum([eval_fn(net(d), l) for d, l in vald_dataloader]) / num_vald_step`
// with the eval_fn of net/sig_mp.py:341,431,556,694,784,836): the same sums for every validation BATCH (group) of a concatenated output in
// one launch. What a workgroup does with its units is one __device__ function per kind (rc_loss_*_units), shared by the kernels above and
// by rc_eval_kernel, where workgroup B finds its group and its index within the group in a table; so a group's value has the bits of
// rc_subnet_loss on the group's slice. position_error (articulate/evaluator.py:129, rnn2's and rnn4's eval_fn) exists here only.
#include "../../include/robustcap_hip.h"
#include "rc_internal.h"
#include "rc_device.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// the workgroup's 256 accumulators -> partial[blockIdx.x]
__device__ __forceinline__ void rc_loss_store_partial(double acc, double* s, double* partial) {
    const int tid = threadIdx.x;
    __syncthreads();
    s[tid] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) s[tid] += s[tid + w];
        __syncthreads();
    }
    if (tid == 0) partial[blockIdx.x] = s[0];
}

__global__ __launch_bounds__(256) void rc_loss_finish_kernel(const double* partial, int n, float* value) {
    __shared__ double s[RC_LOSS_MAX_PARTIALS];
    for (int i = threadIdx.x; i < n; i += 256) s[i] = partial[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sum = 0.0;
    for (int i = 0; i < n; ++i) sum += s[i];                              // index order
    *value = (float)sum;
}

// ---- mse, bce_logits: element-wise over the flat array -----------------------------------------------------------------------------------
// one element's term of the sum (before the division by F W) and its gradient; pw: pos_weight of the element's column
template <int KIND>
__device__ __forceinline__ double rc_loss_element(float xf, float yf, double pw, double inv_n, float& g) {
    const double x = (double)xf, y = (double)yf;
    if constexpr (KIND == RC_LOSS_MSE) {
        const double d = x - y;
        g = (float)(2.0 * d * inv_n);
        return d * d;
    } else {                                                              // torch's stable form of BCEWithLogitsLoss(pos_weight)
        const double L = 1.0 + (pw - 1.0) * y, e = exp(-fabs(x));
        const double one_m_sig = x >= 0.0 ? e / (1.0 + e) : 1.0 / (1.0 + e);   // 1 - sigmoid(x), no cancellation at either end
        g = (float)(((1.0 - y) - L * one_m_sig) * inv_n);
        return (1.0 - y) * x + L * (fmax(-x, 0.0) + log1p(e));
    }
}

// Unit u = elements [u RC_LOSS_CHUNK, (u + 1) RC_LOSS_CHUNK): four 16-byte pieces per thread, piece i of thread t at element
// 4 (256 i + t) of the unit -- a wave's load is 1 KiB of consecutive bytes. The piece that crosses n is done element by element.
// al == false (a group of rc_subnet_eval that starts off the 16-byte grid): the piece comes in as four dwords; which element a thread adds
// when is the same.
__device__ __forceinline__ f32x4 rc_loss_piece(const float* p, bool al) {
    if (al) return *reinterpret_cast<const f32x4*>(p);
    f32x4 v;
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
    return v;
}

// the sum of workgroup b of nb over its units b, b + nb, ... of x, y [n] (before the division by n)
template <int KIND>
__device__ __forceinline__ double rc_loss_elem_units(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ pwt,
                                                     long long n, long long units, double inv_n, int b, int nb, bool al, float* dx) {
    const int tid = threadIdx.x;
    double pw0 = 1.0, pw1 = 1.0;
    if constexpr (KIND == RC_LOSS_BCE_LOGITS) { pw0 = (double)pwt[0]; pw1 = (double)pwt[1]; }   // W = 2: an element's column is its parity
    // bce_logits is bound by exp and log1p in double: one copy of their code, not sixteen
    constexpr int UP = KIND == RC_LOSS_MSE ? RC_LOSS_CHUNK / 1024 : 1, UE = KIND == RC_LOSS_MSE ? 4 : 1;
    double acc = 0.0;
    for (long long u = b; u < units; u += nb) {
        const long long e0 = u * RC_LOSS_CHUNK + 4 * tid;
#pragma unroll UP                                                         // (mse: four loads in flight)
        for (int i = 0; i < RC_LOSS_CHUNK / 1024; ++i) {
            const long long e = e0 + 1024 * i;
            if (e + 3 < n) {
                const f32x4 xv = rc_loss_piece(x + e, al), yv = rc_loss_piece(y + e, al);
                f32x4 gv;
#pragma unroll UE
                for (int k = 0; k < 4; ++k) {
                    float g;
                    acc += rc_loss_element<KIND>(xv[k], yv[k], (k & 1) ? pw1 : pw0, inv_n, g);
                    gv[k] = g;
                }
                if (dx) *reinterpret_cast<f32x4*>(dx + e) = gv;
            } else {
                for (long long q = e; q < n; ++q) {
                    float g;
                    acc += rc_loss_element<KIND>(x[q], y[q], (q & 1) ? pw1 : pw0, inv_n, g);
                    if (dx) dx[q] = g;
                }
            }
        }
    }
    return acc * inv_n;
}

template <int KIND>
__global__ __launch_bounds__(256) void rc_loss_elem_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ pwt,
                                                           long long n, long long units, double inv_n, double* partial, float* dx) {
    __shared__ double s[256];
    const double acc = rc_loss_elem_units<KIND>(x, y, pwt, n, units, inv_n, (int)blockIdx.x, (int)gridDim.x, true, dx);
    rc_loss_store_partial(acc, s, partial);
}

// ---- window_mse (W = 3): mse + the mse of the sums over windows of 6, 20 and 60 frames cut from the END of the batch -----------------------
// Counted from the end, frame f is e = F - 1 - f and lies in window e / w; unit u = e in [240 u, 240 u + 240) holds whole windows of every
// width (60 is a multiple of 6 and 20), except those that would start before frame 0: they do not exist (the first F % w frames belong to
// no window). LDS: the unit's differences by (e, component), then the 40 + 12 + 4 window sums per component.
struct LossWindow {
    long long F;
    double c1, c6, c20, c60;       // 1 / (3 F), 1 / (3 (F / 6)), 1 / (3 (F / 20)), 1 / (3 (F / 60))
};
#define RC_LOSS_WINDOW_SUMS (RC_LOSS_WINDOW_FRAMES / 6 + RC_LOSS_WINDOW_FRAMES / 20 + RC_LOSS_WINDOW_FRAMES / 60)

// the sum of workgroup b of nb over its units b, b + nb, ... of x, y [A.F, 3]
__device__ __forceinline__ double rc_loss_window_units(const float* __restrict__ x, const float* __restrict__ y, const LossWindow A,
                                                       long long units, int b, int nb, float* dx) {
    __shared__ double sd[RC_LOSS_WINDOW_FRAMES * 3];
    __shared__ double sS[RC_LOSS_WINDOW_SUMS * 3];
    constexpr int N6 = RC_LOSS_WINDOW_FRAMES / 6, N20 = RC_LOSS_WINDOW_FRAMES / 20;
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (long long u = b; u < units; u += nb) {
        const long long elo = u * RC_LOSS_WINDOW_FRAMES;
        const long long ehi = elo + RC_LOSS_WINDOW_FRAMES < A.F ? elo + RC_LOSS_WINDOW_FRAMES : A.F;
        const int nf = (int)(ehi - elo);                                  // frames of the unit: f0 .. f0 + nf - 1, e descending
        const long long g0 = (A.F - ehi) * 3;
        __syncthreads();                                                  // (the previous unit's readers are done)
        for (int i = tid; i < nf * 3; i += 256) {
            const double d = (double)x[g0 + i] - (double)y[g0 + i];
            const int fl = i / 3, c = i - 3 * fl;
            sd[(nf - 1 - fl) * 3 + c] = d;
            acc += d * d * A.c1;
        }
        __syncthreads();
        if (tid < RC_LOSS_WINDOW_SUMS * 3) {
            const int q = tid / 3, c = tid - 3 * q;
            const int w = q < N6 ? 6 : q < N6 + N20 ? 20 : 60;
            const int k = q < N6 ? q : q < N6 + N20 ? q - N6 : q - N6 - N20;
            const double cw = q < N6 ? A.c6 : q < N6 + N20 ? A.c20 : A.c60;
            double S = 0.0;
            if (elo + (long long)(k + 1) * w <= A.F) {                    // the window exists: (k + 1) w <= nf
                for (int j = w - 1; j >= 0; --j) S += sd[(k * w + j) * 3 + c];     // frame order
                acc += S * S * cw;
            }
            sS[tid] = S;                                                  // 0 where there is no window: adds nothing to dx
        }
        __syncthreads();
        if (dx) {
            for (int i = tid; i < nf * 3; i += 256) {
                const int fl = i / 3, c = i - 3 * fl, le = nf - 1 - fl;
                const double g = sd[le * 3 + c] * A.c1 + sS[(le / 6) * 3 + c] * A.c6 + sS[(N6 + le / 20) * 3 + c] * A.c20 +
                                 sS[(N6 + N20 + le / 60) * 3 + c] * A.c60;
                dx[g0 + i] = (float)(2.0 * g);
            }
        }
    }
    return acc;
}

__global__ __launch_bounds__(256) void rc_loss_window_kernel(const float* __restrict__ x, const float* __restrict__ y, const LossWindow A,
                                                             long long units, double* partial, float* dx) {
    __shared__ double s[256];
    const double acc = rc_loss_window_units(x, y, A, units, (int)blockIdx.x, (int)gridDim.x, dx);
    rc_loss_store_partial(acc, s, partial);
}

// ---- pose_fk (W = 144): mse(x, y) + 100 mse(J(x), J(y)), J = joints of the 24 r6d rotations on the rest bones (sig_mp.py:749-767) ----------
// One wave per frame, a lane per joint: lanes 0-23 the joints of x, lanes 32-55 those of y. The frame's 2 x 576 bytes come in as 16-byte
// pieces (lanes 0-35) and are handed to the joint lanes through the wave's own LDS; R of both sides goes to LDS for the children, the two
// tree sweeps (joints root-to-leaf, subtree sums leaf-to-root) run level by level like rc_fk_r_kernel's, wave-local. The gradient of the six
// numbers of joint p: dR_p = sum over children i of S_i b_i^T, back through the cross product and the two normalisations, with the
// gradient of every entry the reference sets from NaN to 0 (angular.py:263) dropped. A degenerate joint leaves what the formulas give
// (NaN / inf) in its own six entries of dx; R = 0 keeps it out of J, the value and every other entry.
#define RC_LOSS_LEVELS 10
struct alignas(16) LossPoseWave {
    float x[144], y[144];
    double g[144];              // d (FK term) / d x
    double R[2][24][9];
    double J[2][24][3];         // joints of x | of y; the reverse sweep keeps the subtree sums in [1]
};

// the sum of workgroup b of nb over its units b, b + nb, ... of x, y [F, 144]
__device__ __forceinline__ double rc_loss_pose_units(const BodyConst* __restrict__ body, const float* __restrict__ x, const float* __restrict__ y,
                                                     long long F, long long units, double cm, double cj, int b, int nb, float* dx) {
    __shared__ LossPoseWave sw[4];
    __shared__ double sbone[24][3];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, side = lane >> 5;
    const bool joint = j < 24;
    LossPoseWave& W = sw[wave];
    int par = 0, lvl = -1, nch = 0, ch0 = 0, ch1 = 0, ch2 = 0, ch3 = 0;
    double bn[3] = {0.0, 0.0, 0.0};
    if (joint) {
        par = body->parent[j]; lvl = body->level[j]; nch = body->nchild[j];
        ch0 = body->child[j][0]; ch1 = body->child[j][1]; ch2 = body->child[j][2]; ch3 = body->child[j][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) bn[c] = (double)body->bone[j][c];
    }
    if (tid < 72) sbone[tid / 3][tid % 3] = (double)body->bone[tid / 3][tid % 3];
    __syncthreads();
    double acc = 0.0;
    for (long long u = b; u < units; u += nb) {
        for (int k = 0; k < RC_LOSS_POSE_FRAMES / 4; ++k) {
            const long long f = u * RC_LOSS_POSE_FRAMES + 4 * k + wave;
            if (f >= F) break;                                            // (wave-uniform)
            rc_sync<true>();                                              // the previous frame's readers are done
            double dm[4] = {0.0, 0.0, 0.0, 0.0};
            if (lane < 36) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(x + f * 144 + 4 * lane);
                const f32x4 yv = *reinterpret_cast<const f32x4*>(y + f * 144 + 4 * lane);
                *reinterpret_cast<f32x4*>(&W.x[4 * lane]) = xv;
                *reinterpret_cast<f32x4*>(&W.y[4 * lane]) = yv;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double d = (double)xv[e] - (double)yv[e];
                    acc += d * d * cm;
                    dm[e] = 2.0 * d * cm;
                }
            }
            rc_sync<true>();
            double c0[3] = {0, 0, 0}, c1[3] = {0, 0, 0}, c2[3] = {0, 0, 0}, b[3] = {0, 0, 0}, na = 1.0, nt = 1.0, d = 0.0;
            if (joint) {
                const float* v = (side ? W.y : W.x) + 6 * j;
                const double a[3] = {(double)v[0], (double)v[1], (double)v[2]};
                b[0] = (double)v[3]; b[1] = (double)v[4]; b[2] = (double)v[5];
                na = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
#pragma unroll
                for (int r = 0; r < 3; ++r) c0[r] = a[r] / na;
                d = (c0[0] * b[0] + c0[1] * b[1]) + c0[2] * b[2];
                double t[3];
#pragma unroll
                for (int r = 0; r < 3; ++r) t[r] = b[r] - d * c0[r];
                nt = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
#pragma unroll
                for (int r = 0; r < 3; ++r) c1[r] = t[r] / nt;
                c2[0] = c0[1] * c1[2] - c0[2] * c1[1]; c2[1] = c0[2] * c1[0] - c0[0] * c1[2]; c2[2] = c0[0] * c1[1] - c0[1] * c1[0];
#pragma unroll
                for (int r = 0; r < 3; ++r) {                             // R = (c0 | c1 | c2), NaN -> 0
                    W.R[side][j][3 * r + 0] = c0[r] != c0[r] ? 0.0 : c0[r];
                    W.R[side][j][3 * r + 1] = c1[r] != c1[r] ? 0.0 : c1[r];
                    W.R[side][j][3 * r + 2] = c2[r] != c2[r] ? 0.0 : c2[r];
                }
            }
            rc_sync<true>();
            double pb[3] = {0.0, 0.0, 0.0}, J[3] = {0.0, 0.0, 0.0};
            if (joint && j > 0) {                                         // the bone turned by its PARENT's rotation
                const double* Rp = W.R[side][par];
#pragma unroll
                for (int r = 0; r < 3; ++r) pb[r] = (Rp[3 * r] * bn[0] + Rp[3 * r + 1] * bn[1]) + Rp[3 * r + 2] * bn[2];
            }
            if (joint && j == 0) { W.J[side][0][0] = 0.0; W.J[side][0][1] = 0.0; W.J[side][0][2] = 0.0; }
            for (int L = 1; L < RC_LOSS_LEVELS; ++L) {                    // J_i = J_parent(i) + pb_i, root to leaf
                rc_sync<true>();
                if (joint && lvl == L) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) { J[c] = W.J[side][par][c] + pb[c]; W.J[side][j][c] = J[c]; }
                }
            }
            rc_sync<true>();
            double S[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) S[c] = J[c] - __shfl_xor(J[c], 32);   // lanes of x: J(x) - J(y)
            if (joint && side == 0) acc += ((S[0] * S[0] + S[1] * S[1]) + S[2] * S[2]) * cj;
            if (!dx) continue;                                            // (uniform: value only)
#pragma unroll
            for (int c = 0; c < 3; ++c) S[c] *= 2.0 * cj;                 // d value / d J_i, then the subtree sums, leaf to root
            for (int L = RC_LOSS_LEVELS - 1; L >= 1; --L) {
                if (joint && side == 0 && lvl == L) {
#pragma unroll
                    for (int qi = 0; qi < 4; ++qi) {                      // children in ascending order
                        const int i = qi == 0 ? ch0 : qi == 1 ? ch1 : qi == 2 ? ch2 : ch3;
                        if (qi < nch) { S[0] += W.J[1][i][0]; S[1] += W.J[1][i][1]; S[2] += W.J[1][i][2]; }
                    }
                    W.J[1][j][0] = S[0]; W.J[1][j][1] = S[1]; W.J[1][j][2] = S[2];
                }
                rc_sync<true>();
            }
            if (joint && side == 0) {
                double q0[3] = {0, 0, 0}, q1[3] = {0, 0, 0}, q2[3] = {0, 0, 0};   // d / d c0, c1, c2 = columns of dR_p = sum_i S_i b_i^T
#pragma unroll
                for (int qi = 0; qi < 4; ++qi) {
                    const int i = qi == 0 ? ch0 : qi == 1 ? ch1 : qi == 2 ? ch2 : ch3;
                    if (qi < nch) {
#pragma unroll
                        for (int r = 0; r < 3; ++r) {
                            const double Si = W.J[1][i][r];
                            q0[r] += Si * sbone[i][0]; q1[r] += Si * sbone[i][1]; q2[r] += Si * sbone[i][2];
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < 3; ++r) {                             // entries set from NaN to 0 pass no gradient
                    if (c0[r] != c0[r]) q0[r] = 0.0;
                    if (c1[r] != c1[r]) q1[r] = 0.0;
                    if (c2[r] != c2[r]) q2[r] = 0.0;
                }
                // c2 = c0 x c1
                q0[0] += c1[1] * q2[2] - c1[2] * q2[1]; q0[1] += c1[2] * q2[0] - c1[0] * q2[2]; q0[2] += c1[0] * q2[1] - c1[1] * q2[0];
                q1[0] += q2[1] * c0[2] - q2[2] * c0[1]; q1[1] += q2[2] * c0[0] - q2[0] * c0[2]; q1[2] += q2[0] * c0[1] - q2[1] * c0[0];
                // c1 = t / |t|, t = b - d c0, d = c0 . b
                const double p1 = (c1[0] * q1[0] + c1[1] * q1[1]) + c1[2] * q1[2];
                double dt[3], gb[3], ga[3];
#pragma unroll
                for (int r = 0; r < 3; ++r) dt[r] = (q1[r] - c1[r] * p1) / nt;
                const double dd = -((dt[0] * c0[0] + dt[1] * c0[1]) + dt[2] * c0[2]);
#pragma unroll
                for (int r = 0; r < 3; ++r) { gb[r] = dt[r] + dd * c0[r]; q0[r] += dd * b[r] - d * dt[r]; }
                // c0 = a / |a|
                const double p0 = (c0[0] * q0[0] + c0[1] * q0[1]) + c0[2] * q0[2];
#pragma unroll
                for (int r = 0; r < 3; ++r) ga[r] = (q0[r] - c0[r] * p0) / na;
#pragma unroll
                for (int r = 0; r < 3; ++r) { W.g[6 * j + r] = ga[r]; W.g[6 * j + 3 + r] = gb[r]; }
            }
            rc_sync<true>();
            if (lane < 36) {
                f32x4 gv;
#pragma unroll
                for (int e = 0; e < 4; ++e) gv[e] = (float)(dm[e] + W.g[4 * lane + e]);
                *reinterpret_cast<f32x4*>(dx + f * 144 + 4 * lane) = gv;
            }
        }
    }
    return acc;
}

__global__ __launch_bounds__(256) void rc_loss_pose_kernel(const BodyConst* __restrict__ body, const float* __restrict__ x,
                                                           const float* __restrict__ y, long long F, long long units, double cm, double cj,
                                                           double* partial, float* dx) {
    __shared__ double s[256];
    const double acc = rc_loss_pose_units(body, x, y, F, units, cm, cj, (int)blockIdx.x, (int)gridDim.x, dx);
    rc_loss_store_partial(acc, s, partial);
}

// ---- position_error (rc_subnet_eval only): the mean Euclidean distance of the F W / 3 points (articulate/evaluator.py:129) ----------------
// Unit u = points [u RC_EVAL_POINTS, (u + 1) RC_EVAL_POINTS): point 256 i + t of the unit is thread t's i-th. Three dwords of x and of y per
// point (a wave's three loads cover 768 consecutive bytes; any alignment); differences, squares, the square root and the sum in double.
__device__ __forceinline__ double rc_eval_point_units(const float* __restrict__ x, const float* __restrict__ y, long long P, long long units,
                                                      double inv_p, int b, int nb) {
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (long long u = b; u < units; u += nb) {
#pragma unroll
        for (int i = 0; i < RC_EVAL_POINTS / 256; ++i) {
            const long long p = u * RC_EVAL_POINTS + 256 * i + tid;
            if (p < P) {
                const double d0 = (double)x[3 * p] - (double)y[3 * p], d1 = (double)x[3 * p + 1] - (double)y[3 * p + 1],
                             d2 = (double)x[3 * p + 2] - (double)y[3 * p + 2];
                acc += sqrt((d0 * d0 + d1 * d1) + d2 * d2);
            }
        }
    }
    return acc * inv_p;
}

// ---- the geometry of a call, shared by rc_subnet_loss and rc_subnet_eval: units, workgroups and the double reciprocals ----------------------
static inline long long units_of(long long n, long long per) { return (n + per - 1) / per; }

// g.frames, g.frame0 and g.blk0 set by the caller; fills g.nblk and g.c, returns the units
static long long rc_loss_geometry(int kind, int W, EvalGroup& g) {
    const long long F = g.frames, n = F * W;
    long long units = 0;
    g.c[0] = g.c[1] = g.c[2] = g.c[3] = 0.0;
    if (kind == RC_LOSS_MSE || kind == RC_LOSS_BCE_LOGITS) {
        units = units_of(n, RC_LOSS_CHUNK);
        g.c[0] = 1.0 / (double)n;
    } else if (kind == RC_LOSS_WINDOW_MSE) {
        units = units_of(F, RC_LOSS_WINDOW_FRAMES);
        g.c[0] = 1.0 / (3.0 * (double)F); g.c[1] = 1.0 / (3.0 * (double)(F / 6)); g.c[2] = 1.0 / (3.0 * (double)(F / 20));
        g.c[3] = 1.0 / (3.0 * (double)(F / 60));
    } else if (kind == RC_LOSS_POSE_FK) {
        units = units_of(F, RC_LOSS_POSE_FRAMES);
        g.c[0] = 1.0 / (144.0 * (double)F); g.c[1] = 100.0 / (72.0 * (double)F);
    } else {                                                              // RC_EVAL_POSITION_ERROR
        units = units_of(n / 3, RC_EVAL_POINTS);
        g.c[0] = 1.0 / (double)(n / 3);
    }
    g.nblk = (int)(units < RC_LOSS_MAX_PARTIALS ? units : RC_LOSS_MAX_PARTIALS);
    return units;
}

void rc_eval_group(int kind, int W, EvalGroup* g) { rc_loss_geometry(kind, W, *g); }

// x, y (and dx) 16-byte aligned for every kind but window_mse; width and F checked by the caller (rc_subnet_loss)
void rc_launch_subnet_loss(int kind, const BodyConst* body, const float* x, const float* y, long long F, int W, const float* aux,
                           double* partial, float* value, float* dx, hipStream_t st) {
    const long long n = F * W;
    EvalGroup g{0, F, 0, 0, {0.0, 0.0, 0.0, 0.0}};
    const long long units = rc_loss_geometry(kind, W, g);
    const int blocks = g.nblk;
    const dim3 grid((unsigned)blocks), wg(256);
    if (kind == RC_LOSS_MSE) {
        hipLaunchKernelGGL(rc_loss_elem_kernel<RC_LOSS_MSE>, grid, wg, 0, st, x, y, aux, n, units, g.c[0], partial, dx);
    } else if (kind == RC_LOSS_BCE_LOGITS) {
        hipLaunchKernelGGL(rc_loss_elem_kernel<RC_LOSS_BCE_LOGITS>, grid, wg, 0, st, x, y, aux, n, units, g.c[0], partial, dx);
    } else if (kind == RC_LOSS_WINDOW_MSE) {
        const LossWindow A{F, g.c[0], g.c[1], g.c[2], g.c[3]};
        hipLaunchKernelGGL(rc_loss_window_kernel, grid, wg, 0, st, x, y, A, units, partial, dx);
    } else {
        hipLaunchKernelGGL(rc_loss_pose_kernel, grid, wg, 0, st, body, x, y, F, units, g.c[0], g.c[1], partial, dx);
    }
    hipLaunchKernelGGL(rc_loss_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)partial, blocks, value);
}

// ---- rc_subnet_eval: the same sums per GROUP of a concatenated batch, one launch for all groups -----------------------------------------------
// Workgroup B of the launch is workgroup B - tab[g].blk0 of group g's own tab[g].nblk (= what rc_subnet_loss would launch for the group's
// slice): g is the last group with blk0 <= B, found by bisection. It runs the per-workgroup code above on the slice with the slice's
// geometry, value only, and stores partial[B]; rc_eval_finish_kernel, one workgroup per group, adds the group's partials in index order.
template <int KIND>
__global__ __launch_bounds__(256) void rc_eval_kernel(const EvalGroup* __restrict__ tab, int groups, const BodyConst* __restrict__ body,
                                                      const float* __restrict__ x, const float* __restrict__ y, int W,
                                                      const float* __restrict__ aux, double* partial) {
    __shared__ double s[256];
    const int B = (int)blockIdx.x;
    int lo = 0, hi = groups - 1;                                          // (uniform: every thread walks the same way)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].blk0 <= B) lo = mid; else hi = mid - 1;
    }
    const EvalGroup G = tab[lo];
    const int b = B - G.blk0, nb = G.nblk;
    const float* xg = x + G.frame0 * W;
    const float* yg = y + G.frame0 * W;
    const long long F = G.frames, n = F * W;
    double acc;
    if constexpr (KIND == RC_LOSS_MSE || KIND == RC_LOSS_BCE_LOGITS) {
        const bool al = ((((unsigned long long)xg) | ((unsigned long long)yg)) & 15ull) == 0;
        acc = rc_loss_elem_units<KIND>(xg, yg, aux, n, (n + RC_LOSS_CHUNK - 1) / RC_LOSS_CHUNK, G.c[0], b, nb, al, nullptr);
    } else if constexpr (KIND == RC_LOSS_WINDOW_MSE) {
        const LossWindow A{F, G.c[0], G.c[1], G.c[2], G.c[3]};
        acc = rc_loss_window_units(xg, yg, A, (F + RC_LOSS_WINDOW_FRAMES - 1) / RC_LOSS_WINDOW_FRAMES, b, nb, nullptr);
    } else if constexpr (KIND == RC_LOSS_POSE_FK) {                       // (576 bytes a frame: every group starts on the 16-byte grid)
        acc = rc_loss_pose_units(body, xg, yg, F, (F + RC_LOSS_POSE_FRAMES - 1) / RC_LOSS_POSE_FRAMES, G.c[0], G.c[1], b, nb, nullptr);
    } else {
        const long long P = n / 3;
        acc = rc_eval_point_units(xg, yg, P, (P + RC_EVAL_POINTS - 1) / RC_EVAL_POINTS, G.c[0], b, nb);
    }
    rc_loss_store_partial(acc, s, partial);
}

__global__ __launch_bounds__(256) void rc_eval_finish_kernel(const EvalGroup* __restrict__ tab, const double* partial, float* values) {
    __shared__ double s[RC_LOSS_MAX_PARTIALS];
    const EvalGroup G = tab[blockIdx.x];
    for (int i = threadIdx.x; i < G.nblk; i += 256) s[i] = partial[G.blk0 + i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sum = 0.0;
    for (int i = 0; i < G.nblk; ++i) sum += s[i];                         // index order
    values[blockIdx.x] = (float)sum;
}

// tab: DEVICE [groups], filled by rc_eval_group; blocks = sum of nblk; partial: `blocks` doubles. Two launches whatever `groups` is.
void rc_launch_subnet_eval(int kind, const BodyConst* body, const EvalGroup* tab, int groups, long long blocks, const float* x, const float* y,
                           int W, const float* aux, double* partial, float* values, hipStream_t st) {
    const dim3 grid((unsigned)blocks), wg(256);
    if (kind == RC_LOSS_MSE) hipLaunchKernelGGL(rc_eval_kernel<RC_LOSS_MSE>, grid, wg, 0, st, tab, groups, body, x, y, W, aux, partial);
    else if (kind == RC_LOSS_BCE_LOGITS) hipLaunchKernelGGL(rc_eval_kernel<RC_LOSS_BCE_LOGITS>, grid, wg, 0, st, tab, groups, body, x, y, W, aux, partial);
    else if (kind == RC_LOSS_WINDOW_MSE) hipLaunchKernelGGL(rc_eval_kernel<RC_LOSS_WINDOW_MSE>, grid, wg, 0, st, tab, groups, body, x, y, W, aux, partial);
    else if (kind == RC_LOSS_POSE_FK) hipLaunchKernelGGL(rc_eval_kernel<RC_LOSS_POSE_FK>, grid, wg, 0, st, tab, groups, body, x, y, W, aux, partial);
    else hipLaunchKernelGGL(rc_eval_kernel<RC_EVAL_POSITION_ERROR>, grid, wg, 0, st, tab, groups, body, x, y, W, aux, partial);
    hipLaunchKernelGGL(rc_eval_finish_kernel, dim3((unsigned)groups), dim3(256), 0, st, tab, (const double*)partial, values);
}

