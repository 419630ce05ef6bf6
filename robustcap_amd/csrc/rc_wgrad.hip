// Weight gradients of a trainable sub-net (rc_subnet_weight_grads; articulate/utils/torch/train.py:117-122: what loss.backward() leaves in
// the .grad of rnn.py:121-133's linear1, LSTM and linear2 parameters): C[M, N] = sum_f A[f, m] B'[f, n], a GEMM whose contraction index
// -- the frame -- is the SLOW index of both row-major operands.
//
// One workgroup = four waves = one 128 x 128 tile of C over a range of frames; wave w owns the 64 x 64 quarter (w >> 1, w & 1) as 4 x 4
// MFMA blocks. MFMA row i of block r stands for column 4 i + r of the quarter (not 16 r + i): the four blocks of a lane are then four
// CONSECUTIVE columns, on the way in (one 16-byte piece per lane and frame) and on the way out (one 16-byte store per lane and row).
//
// Staging, 32 frames at a time: waves 0-1 load the A tile, waves 2-3 the B' tile; a thread loads four consecutive columns of eight
// frames 8 kq .. 8 kq + 7 (predicated: columns past the operand and frames past the range are zeros, nothing is read past an array;
// rows that are only 4-byte aligned -- x, dy -- go as single floats). B' is formed while it is loaded: the site-1 dropout mask from
// Philox (one call per four columns, rc_philox.h) and the shift of h by one frame through the per-frame first-frame index. Mode 1: the
// eight frames of a column are exactly the 8 k of one lane's bf16 MFMA operand, so each column is split ONCE into three bf16 planes here (split3, rc_mma.h) and stored as three 16-byte pieces [plane][kq][column slot]; the waves read
// their fragments back with one ds_read_b128 each, 16 lanes on 16 consecutive pieces (a whole bank row: conflict-free, as are the
// writes: slot = (column & 3) * 32 + column / 4 puts a thread's four columns 32 pieces apart and 32 threads side by side). A transposed
// LDS read (ds_read_b64_tr_b16) is not needed: the transposition happens in registers before the split, on fp32 values. Mode 0: the
// fp32 image [frame][column], read as one 16-byte piece per lane and k (its four blocks) for v_mfma_f32_16x16x4_f32.
// The next image's global loads are issued before the MFMAs of the current one.
//
// Summation over frames, deterministic: the MFMA accumulators take at most 256 frames, then are added into a second accumulator set;
// the frames are cut into `parts` ranges of whole 256-frame blocks (grid z), whose sums go to a scratch and are added in index order
// by rc_wgrad_reduce_kernel. No atomics.
//
// The column sums of A (the bias gradients) run as a kernel of their own, rc_wgrad_colsum_kernel, in the same order -- 256-frame blocks,
// the blocks of a part in frame order, the parts in index order -- on double accumulators, rounded to fp32 once: as a column of ones in
// the GEMM they sat at 7-8 times torch fp32's error in mode 0 (one fp32 chain per 256 frames against torch's cascaded sum), the
// bound's edge; a sum of F M floats is memory traffic, not arithmetic.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

#include "rc_internal.h"
#include "rc_mma.h"
#include "rc_philox.h"

namespace {

constexpr int TILE = RC_WG_TILE;
constexpr int STAGES_PER_BLOCK = RC_WG_BLOCK / RC_WG_KB;
static_assert(TILE == 128 && RC_WG_KB == 32, "the staging and fragment index arithmetic below is written for 128 x 128 x 32");

__device__ __forceinline__ f32x4 load4(const float* row, int col, int ncols, bool vec) {
    f32x4 r = {0.0f, 0.0f, 0.0f, 0.0f};
    if (!row || col >= ncols) return r;
    if (vec && col + 3 < ncols) return *reinterpret_cast<const f32x4*>(row + col);
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (col + q < ncols) r[q] = row[col + q];
    return r;
}

__device__ __forceinline__ void mask4(const WgradLaunch& L, long long f, int col, f32x4& x) {
    const uint4 u = philox4x32_10(make_uint4((uint32_t)f, (uint32_t)(col >> 2), 1u, L.call), L.key);
    x[0] = u.x >= L.T ? x[0] * L.scale : 0.0f;
    x[1] = u.y >= L.T ? x[1] * L.scale : 0.0f;
    x[2] = u.z >= L.T ? x[2] * L.scale : 0.0f;
    x[3] = u.w >= L.T ? x[3] * L.scale : 0.0f;
}

// v[e]: columns col .. col + 3 of frame fb + 8 kq + e of the A tile (is_b = false) or of segment S of B'.
// whole: the tile lies inside the operand's columns and its rows may be read as 16-byte pieces (uniform over the workgroup). Then the
// eight loads are issued back to back, without a branch between them: a frame past the range reads the range's last frame and is
// zeroed afterwards, and the first-frame indices of a shifted operand are all loaded before the first row that depends on one.
__device__ __forceinline__ void fetch(const WgradLaunch& L, const WgradSeg& S, bool is_b, bool whole, long long fb, long long f_end, int col,
                                      int kq, f32x4 (&v)[8]) {
    if (whole) {
        const long long f0 = fb + 8 * kq, last = f_end - 1;
        const bool shift = is_b && S.kind == RC_WG_SHIFT;
        const float* rp[8];
        int sq[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) sq[e] = shift ? L.first[std::min(f0 + e, last)] : -1;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const long long fc = std::min(f0 + e, last);
            if (!is_b) rp[e] = L.A + fc * L.lda + col;
            else if (!shift) rp[e] = S.src + fc * S.ld + col;
            else rp[e] = sq[e] < 0 ? S.src + (fc - 1) * S.ld + col : S.init ? S.init + (long long)sq[e] * S.ld + col : S.src + col;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = *reinterpret_cast<const f32x4*>(rp[e]);
        if (is_b && S.kind == RC_WG_MASKED) {
#pragma unroll
            for (int e = 0; e < 8; ++e) mask4(L, std::min(f0 + e, last), col, v[e]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (f0 + e > last || (sq[e] >= 0 && !S.init)) v[e] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        return;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const long long f = fb + 8 * kq + e;
        f32x4 x = {0.0f, 0.0f, 0.0f, 0.0f};
        if (f < f_end) {
            if (!is_b) x = load4(L.A + f * L.lda, col, L.M, L.a_vec != 0);
            else {
                const float* row;
                if (S.kind == RC_WG_SHIFT) {
                    const int s = L.first[f];
                    row = s < 0 ? S.src + (f - 1) * S.ld : (S.init ? S.init + (long long)s * S.ld : nullptr);
                } else row = S.src + f * S.ld;
                x = load4(row, col, S.ncols, S.vec != 0);
                if (S.kind == RC_WG_MASKED) mask4(L, f, col, x);
            }
        }
        v[e] = x;
    }
}

// columns n .. n + 3 of row m of segment S's output
__device__ __forceinline__ void store_out(const WgradSeg& S, int M, int m, int n, const f32x4& v) {
    if (m >= M) return;
    if (!S.out || n >= S.ncols) return;
    float* p = S.out + (long long)m * S.ldo + n;
    if (n + 3 < S.ncols && (S.ldo & 3) == 0 && ((uintptr_t)S.out & 15) == 0) {
        *reinterpret_cast<f32x4*>(p) = v;
        return;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (n + q < S.ncols) p[q] = v[q];
}

__device__ __forceinline__ int seg_of_tile(const WgradLaunch& L, int tn) {
    int si = 0;
    while (si + 1 < L.nseg && tn >= L.seg[si + 1].tile0) ++si;
    return si;
}

template <bool SPLIT>
__global__ __launch_bounds__(256) void rc_wgrad_kernel(const WgradLaunch L) {
    // SPLIT: [operand][plane][kq][slot] 16-byte pieces (48 KiB); else [operand][frame][column] floats (32 KiB)
    __shared__ u32x4 lds[SPLIT ? 2 * 3 * 4 * TILE : 2 * RC_WG_KB * TILE / 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tn = blockIdx.x, tm = blockIdx.y, part = blockIdx.z;
    const int si = seg_of_tile(L, tn);
    const WgradSeg& S = L.seg[si];
    const int m0 = tm * TILE, n0 = (tn - S.tile0) * TILE;
    const long long f_begin = (long long)part * L.blocks_per_part * RC_WG_BLOCK;
    const long long f_end = std::min<long long>(L.F, f_begin + (long long)L.blocks_per_part * RC_WG_BLOCK);
    const int n_stages = f_end > f_begin ? (int)((f_end - f_begin + RC_WG_KB - 1) / RC_WG_KB) : 0;

    // staging role
    const bool is_b = tid >= 128;
    const int cg = tid & 31, skq = (tid & 127) >> 5;
    const int scol = (is_b ? n0 : m0) + 4 * cg;
    const bool whole = is_b ? S.vec != 0 && n0 + TILE <= S.ncols : L.a_vec != 0 && m0 + TILE <= L.M;
    // compute role
    const int i = lane & 15, kq = lane >> 4;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;

    f32x4 acc1[4][4], acc2[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc1[r][j] = acc2[r][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    f32x4 v[8];
    if (n_stages > 0) fetch(L, S, is_b, whole, f_begin, f_end, scol, skq, v);
    for (int s = 0; s < n_stages; ++s) {
        // ---- the image of stage s ----
        if constexpr (SPLIT) {
            u32x4* base = lds + (is_b ? 3 * 4 * TILE : 0) + skq * TILE + cg;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 x0 = {v[0][q], v[1][q], v[2][q], v[3][q]}, x1 = {v[4][q], v[5][q], v[6][q], v[7][q]};
                u32x4 h, m, l;
                split3(x0, x1, h, m, l);
                base[0 * 4 * TILE + q * 32] = h;
                base[1 * 4 * TILE + q * 32] = m;
                base[2 * 4 * TILE + q * 32] = l;
            }
        } else {
            f32x4* base = reinterpret_cast<f32x4*>(lds) + (is_b ? RC_WG_KB * TILE / 4 : 0) + (8 * skq) * (TILE / 4) + cg;
#pragma unroll
            for (int e = 0; e < 8; ++e) base[e * (TILE / 4)] = v[e];
        }
        __syncthreads();
        if (s + 1 < n_stages) fetch(L, S, is_b, whole, f_begin + (long long)(s + 1) * RC_WG_KB, f_end, scol, skq, v);
        // ---- products ----
        if constexpr (SPLIT) {
            const u32x4* pa = lds + kq * TILE + (wm >> 2) + i;
            const u32x4* pb = lds + 3 * 4 * TILE + kq * TILE + (wn >> 2) + i;
            u32x4 wp[3][4];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
#pragma unroll
                for (int j = 0; j < 4; ++j) wp[pl][j] = pb[pl * 4 * TILE + j * 32];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bf16x8 ah = __builtin_bit_cast(bf16x8, pa[0 * 4 * TILE + r * 32]);
                const bf16x8 am = __builtin_bit_cast(bf16x8, pa[1 * 4 * TILE + r * 32]);
                const bf16x8 al = __builtin_bit_cast(bf16x8, pa[2 * 4 * TILE + r * 32]);
                // the order of mma_kblock (rc_mma.h): small terms first
#define RC_PROD(AV, PL)                                                                                                  \
    _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                                         \
        acc1[r][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(AV, __builtin_bit_cast(bf16x8, wp[PL][j]), acc1[r][j], 0, 0, 0);
#if RC_SPLIT_PRODUCTS == 9
                RC_PROD(al, 2) RC_PROD(am, 2) RC_PROD(al, 1)
#endif
                RC_PROD(al, 0) RC_PROD(ah, 2) RC_PROD(am, 1) RC_PROD(am, 0) RC_PROD(ah, 1) RC_PROD(ah, 0)
#undef RC_PROD
            }
        } else {
            const f32x4* pa = reinterpret_cast<const f32x4*>(lds) + kq * (TILE / 4) + (wm >> 2) + i;
            const f32x4* pb = reinterpret_cast<const f32x4*>(lds) + RC_WG_KB * TILE / 4 + kq * (TILE / 4) + (wn >> 2) + i;
#pragma unroll
            for (int ks = 0; ks < RC_WG_KB / 4; ++ks) {
                const f32x4 a4 = pa[ks * 4 * (TILE / 4)], b4 = pb[ks * 4 * (TILE / 4)];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc1[r][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[r], b4[j], acc1[r][j], 0, 0, 0);
            }
        }
        __syncthreads();
        if ((s + 1) % STAGES_PER_BLOCK == 0 || s + 1 == n_stages) {        // 256 frames (or the range's rest) -> the second level
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc2[r][j] += acc1[r][j];
                    acc1[r][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                }
        }
    }

    // acc2[r][j][e]: row wm + 4 (4 kq + e) + r, column wn + 4 i + j of the tile
    const int ldp = L.ntiles_n * TILE;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int m = m0 + wm + 4 * (4 * kq + e) + r;
            const int nl = wn + 4 * i;
            const f32x4 o = {acc2[r][0][e], acc2[r][1][e], acc2[r][2][e], acc2[r][3][e]};
            if (L.parts > 1)
                *reinterpret_cast<f32x4*>(L.partial + ((long long)part * L.ntiles_m * TILE + m) * ldp + tn * TILE + nl) = o;
            else store_out(S, L.M, m, n0 + nl, o);
        }
}

// one thread per four consecutive columns of the padded [128 ntiles_m][128 ntiles_n] matrix
__global__ __launch_bounds__(256) void rc_wgrad_reduce_kernel(const WgradLaunch L) {
    const int ldp = L.ntiles_n * TILE, n4 = ldp / 4;
    const long long total = (long long)L.ntiles_m * TILE * n4;
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= total) return;
    const int m = (int)(q / n4), n = (int)(q - (long long)m * n4) * 4;
    if (m >= L.M) return;
    const long long ps = (long long)L.ntiles_m * TILE * ldp;
    const float* p = L.partial + (long long)m * ldp + n;
    f32x4 sum = *reinterpret_cast<const f32x4*>(p);
    for (int k = 1; k < L.parts; ++k) sum += *reinterpret_cast<const f32x4*>(p + k * ps);
    const int tn = n / TILE;
    const WgradSeg& S = L.seg[seg_of_tile(L, tn)];
    store_out(S, L.M, m, n - S.tile0 * TILE, sum);
}

// 64 columns x 4 frame lanes per workgroup: lane r of a column adds frames r, r + 4, ... of a 256-frame block in double, the four are
// added in lane order, and the block's sum goes into the column's second accumulator
__global__ __launch_bounds__(256) void rc_wgrad_colsum_kernel(const float* A, int lda, int M, long long F, int parts, int blocks_per_part,
                                                              double* partial, float* out, float* out2) {
    __shared__ double lane_sum[4][64];
    const int c = threadIdx.x & 63, r = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + c, part = blockIdx.y;
    const bool live = col < M;
    const long long f_begin = (long long)part * blocks_per_part * RC_WG_BLOCK;
    const long long f_end = std::min<long long>(F, f_begin + (long long)blocks_per_part * RC_WG_BLOCK);
    double acc2 = 0.0;
    for (long long fb = f_begin; fb < f_end; fb += RC_WG_BLOCK) {
        const long long fe = std::min<long long>(f_end, fb + RC_WG_BLOCK);
        double acc1 = 0.0;
        if (live)
            for (long long f = fb + r; f < fe; f += 4) acc1 += (double)A[f * lda + col];
        lane_sum[r][c] = acc1;
        __syncthreads();
        if (r == 0) acc2 += ((lane_sum[0][c] + lane_sum[1][c]) + lane_sum[2][c]) + lane_sum[3][c];
        __syncthreads();
    }
    if (r != 0 || !live) return;
    if (parts > 1) partial[(long long)part * M + col] = acc2;
    else {
        if (out) out[col] = (float)acc2;
        if (out2) out2[col] = (float)acc2;
    }
}

__global__ __launch_bounds__(256) void rc_wgrad_colsum_reduce_kernel(const double* partial, int M, int parts, float* out, float* out2) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= M) return;
    double sum = partial[col];
    for (int k = 1; k < parts; ++k) sum += partial[(long long)k * M + col];
    if (out) out[col] = (float)sum;
    if (out2) out2[col] = (float)sum;
}

}  // namespace

void rc_launch_wgrad(const WgradLaunch& L, int split, hipStream_t s) {
    const dim3 grid((unsigned)L.ntiles_n, (unsigned)L.ntiles_m, (unsigned)L.parts);
    if (split) hipLaunchKernelGGL(rc_wgrad_kernel<true>, grid, dim3(256), 0, s, L);
    else hipLaunchKernelGGL(rc_wgrad_kernel<false>, grid, dim3(256), 0, s, L);
}

void rc_launch_wgrad_reduce(const WgradLaunch& L, hipStream_t s) {
    const long long total = (long long)L.ntiles_m * TILE * (L.ntiles_n * TILE / 4);
    hipLaunchKernelGGL(rc_wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, L);
}

void rc_launch_wgrad_colsum(const float* A, int lda, int M, long long F, int parts, int blocks_per_part, double* partial, float* out,
                            float* out2, hipStream_t s) {
    hipLaunchKernelGGL(rc_wgrad_colsum_kernel, dim3((unsigned)((M + 63) / 64), (unsigned)parts), dim3(256), 0, s, A, lda, M, F, parts,
                       blocks_per_part, partial, out, out2);
    if (parts > 1)
        hipLaunchKernelGGL(rc_wgrad_colsum_reduce_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, partial, M, parts, out, out2);
}
