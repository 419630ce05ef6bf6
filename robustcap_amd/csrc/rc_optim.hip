// The optimiser step of one trainable sub-net on the device (rc_subnet_optim_step; articulate/utils/torch/train.py:120-121:
// clip_grad_norm_(net.parameters(), 1) and optimizer.step() with Adam): the 2-norm of every gradient, then clip, Adam and the repack of
// rc_update_subnet_weights in one pass over the padded packed matrices. Host side: rc_api.cpp.
//
// Norm: a workgroup owns RC_OPTIM_CHUNK consecutive elements of one gradient (the tensors in the caller's order, a skipped tensor owns
// no workgroup) and stores the sum of their squares, formed in double in a fixed order, as one partial; a single workgroup then adds the
// partials in index order. No atomics: two runs give the same bits.
//
// Update: the element map of rc_repack_lstm_kernel / rc_repack_dense_kernel (rc_subnet.hip) over the padded packed matrix -- one element
// per thread in the dense layers, four consecutive k per thread in the LSTM layers, which hold all but a few per cent of the bytes. A
// master element belongs to exactly one packed element, so its parameter and moments are updated in place by that thread alone.
#include "rc_internal.h"
#include "rc_pack.h"

__global__ __launch_bounds__(256) void rc_optim_sumsq_kernel(const OptimNorm A, double* partial) {
    __shared__ double s[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    int t = 0;
    while (t + 1 < A.count && b >= A.block0[t + 1]) ++t;                  // (a skipped tensor has block0[t] == block0[t + 1])
    const float* g = A.g[t];
    const long long e0 = (long long)(b - A.block0[t]) * RC_OPTIM_CHUNK, e1 = min(A.n[t], e0 + RC_OPTIM_CHUNK);
    double acc = 0.0;
    long long e = e0 + tid;
    for (; e + 3 * 256 < e1; e += 4 * 256) {                              // four loads in flight; added in element order
        const float a0 = g[e], a1 = g[e + 256], a2 = g[e + 512], a3 = g[e + 768];
        acc += (double)a0 * a0; acc += (double)a1 * a1; acc += (double)a2 * a2; acc += (double)a3 * a3;
    }
    for (; e < e1; e += 256) { const float a = g[e]; acc += (double)a * a; }
    s[tid] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) s[tid] += s[tid + w];
        __syncthreads();
    }
    if (tid == 0) partial[b] = s[0];
}

// out2[0] = total norm, out2[1] = clip coefficient min(1, max_norm / (total_norm + 1e-6)) in fp32 (clip_grad_norm_), 1 when max_norm <= 0
__global__ __launch_bounds__(256) void rc_optim_norm_finish_kernel(const double* partial, int n, float max_norm, float* out2) {
    __shared__ double s[2048];
    double sum = 0.0;
    for (int i0 = 0; i0 < n; i0 += 2048) {
        const int m = min(2048, n - i0);
        __syncthreads();
        for (int i = threadIdx.x; i < m; i += 256) s[i] = partial[i0 + i];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < m; ++i) sum += s[i];                      // index order
    }
    if (threadIdx.x != 0) return;
    const float tn = (float)sqrt(sum);
    float coef = 1.0f;
    if (max_norm > 0.0f) {
        const float c = max_norm / (tn + 1e-6f);
        coef = c > 1.0f ? 1.0f : c;                                       // (a NaN norm stays a NaN coefficient, like clamp(max=1))
    }
    out2[0] = tn;
    out2[1] = coef;
}

void rc_launch_optim_norm(const OptimNorm& A, int blocks, double* partial, float max_norm, float* out2, hipStream_t s) {
    if (blocks > 0) hipLaunchKernelGGL(rc_optim_sumsq_kernel, dim3((unsigned)blocks), dim3(256), 0, s, A, partial);
    hipLaunchKernelGGL(rc_optim_norm_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)partial, blocks, max_norm, out2);
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

// One element's clipped Adam step: g' = coef g (+ weight_decay p);  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;
// p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
__device__ __forceinline__ void rc_adam_math(float& p, float g, float& m, float& v, const OptimScalars& a, float coef) {
    g *= coef;
    if (a.weight_decay != 0.0f) g += a.weight_decay * p;
    m = a.beta1 * m + a.one_m_beta1 * g;
    v = a.beta2 * v + a.one_m_beta2 * (g * g);
    p -= a.step_size * (m / (sqrtf(v) / a.bc2_sqrt + a.eps));
}

// ... of element i of a tensor, in place; returns the parameter's value afterwards (unchanged when the tensor has no gradient)
__device__ __forceinline__ float rc_adam_element(const OptimTensor& T, long long i, const OptimScalars& a, float coef) {
    float p = T.p[i];
    if (!T.g) return p;
    float m = T.m[i], v = T.v[i];
    rc_adam_math(p, T.g[i], m, v, a, coef);
    T.p[i] = p; T.m[i] = m; T.v[i] = v;
    return p;
}

// ... of elements i .. i + 3 (i % 4 == 0, the tensors 16-byte aligned)
__device__ __forceinline__ f32x4 rc_adam_element4(const OptimTensor& T, long long i, const OptimScalars& a, float coef) {
    f32x4 p = *reinterpret_cast<const f32x4*>(T.p + i);
    if (!T.g) return p;
    const f32x4 g = *reinterpret_cast<const f32x4*>(T.g + i);
    f32x4 m = *reinterpret_cast<const f32x4*>(T.m + i), v = *reinterpret_cast<const f32x4*>(T.v + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float pe = p[e], me = m[e], ve = v[e];
        rc_adam_math(pe, g[e], me, ve, a, coef);
        p[e] = pe; m[e] = me; v[e] = ve;
    }
    *reinterpret_cast<f32x4*>(T.p + i) = p;
    *reinterpret_cast<f32x4*>(T.m + i) = m;
    *reinterpret_cast<f32x4*>(T.v + i) = v;
    return p;
}

// LSTM layer: rc_repack_lstm_kernel's map (packed column n' <-> torch row g * H + 4 * cb + u, k < H from weight_ih, else weight_hh), four
// consecutive k per thread -- one 16-byte piece of each master tensor and of the fp32 pack, one 8-byte piece of each bf16 plane (the
// values and places of rc_pack_store for k .. k + 3). A workgroup owns the 16 columns of block blockIdx.x and 64 k: every 1 KiB piece of
// the packings it touches is written whole. The threads of k == 0 step the row's two biases, each on its own, and store bl[n'] = bias_ih + bias_hh.
__global__ __launch_bounds__(256) void rc_optim_lstm_kernel(const OptimTensor wi, const OptimTensor wh, const OptimTensor bi, const OptimTensor bh,
                                                            int H, float* W, unsigned short* Ws, float* bl, const OptimScalars a,
                                                            const float* out2) {
    const float coef = out2[1];
    const int cb = blockIdx.x, j = threadIdx.x >> 4, k = 64 * blockIdx.y + 4 * (threadIdx.x & 15), np = 16 * cb + j;
    const long long r = (long long)(j & 3) * H + 4 * cb + (j >> 2);
    const f32x4 v = k < H ? rc_adam_element4(wi, r * H + k, a, coef) : rc_adam_element4(wh, r * H + (k - H), a, coef);
    const int Kp = 2 * H;
    *reinterpret_cast<f32x4*>(&W[(((long long)cb * (Kp / RC_KC) + (k >> 4)) * 64 + ((k >> 2) & 3) * 16 + j) << 2]) = v;
    u16x4 hi, mid, lo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        unsigned short h, m, l;
        rc_split_bf16(v[e], h, m, l);
        hi[e] = h; mid[e] = m; lo[e] = l;
    }
    const int kb = k >> 5, rr = k & 31, lane = ((rr & 15) >> 2) * 16 + j;
    unsigned short* ws = Ws + (((long long)cb * (Kp / 32) + kb) * 3) * 512 + lane * 8 + (rr >> 4) * 4;
    *reinterpret_cast<u16x4*>(ws) = hi;
    *reinterpret_cast<u16x4*>(ws + 512) = mid;
    *reinterpret_cast<u16x4*>(ws + 1024) = lo;
    if (k == 0) {
        const float b0 = rc_adam_element(bi, r, a, coef), b1 = rc_adam_element(bh, r, a, coef);
        bl[np] = b0 + b1;
    }
}

// H % 32 == 0 (every sub-net's: 512, 1024, 1280) and the four tensors of wi and wh 16-byte aligned: checked by the caller
void rc_launch_optim_lstm(const OptimTensor& wi, const OptimTensor& wh, const OptimTensor& bi, const OptimTensor& bh, int H, float* W, void* Ws,
                          float* bl, const OptimScalars& a, const float* out2, hipStream_t s) {
    hipLaunchKernelGGL(rc_optim_lstm_kernel, dim3((unsigned)(4 * H / 16), (unsigned)(2 * H / 64)), dim3(256), 0, s, wi, wh, bi, bh, H, W,
                       (unsigned short*)Ws, bl, a, out2);
}

// dense layer (rc_repack_dense_kernel's threads) from the row-major tensor Wt.p [N, K]: element (n, k) of the padded [Np, Kp] matrix, zeros
// in the padding; the row-major copy Wrm where the layer has one; the thread of k == 0 steps the bias and stores the padded bias bp [Np]
__global__ __launch_bounds__(256) void rc_optim_dense_kernel(const OptimTensor Wt, const OptimTensor bt, int N, int K, int Np, int Kp, float* W,
                                                             unsigned short* Ws, float* Wrm, float* bp, const OptimScalars a, const float* out2) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)Np * Kp) return;
    const float coef = out2[1];
    const int n = (int)(idx / Kp), k = (int)(idx - (long long)n * Kp);
    float v = 0.0f;
    if (n < N && k < K) {
        v = rc_adam_element(Wt, (long long)n * K + k, a, coef);
        if (Wrm) Wrm[(long long)n * K + k] = v;
    }
    rc_pack_store(W, Ws, Kp, n, k, v);
    if (k == 0) bp[n] = n < N ? rc_adam_element(bt, n, a, coef) : 0.0f;
}

void rc_launch_optim_dense(const OptimTensor& Wt, const OptimTensor& bt, int N, int K, int Np, int Kp, float* W, void* Ws, float* Wrm, float* bp,
                           const OptimScalars& a, const float* out2, hipStream_t s) {
    const long long n = (long long)Np * Kp;
    hipLaunchKernelGGL(rc_optim_dense_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, Wt, bt, N, K, Np, Kp, W, (unsigned short*)Ws, Wrm,
                       bp, a, out2);
}
