// Sub-net forward over ragged sequences (articulate/utils/torch/rnn.py:121-133, RNN.forward on a packed sequence), time-hoisted:
// per time chunk, relu(linear1), the input half x . W_ih of each LSTM layer and linear2 are tall GEMMs over every frame of the chunk;
// only h(t - 1) . W_hh stays in the time loop. Host side: rc_subnet_api.cpp.
//
// One kernel carries all of them (rc_subnet_gemm_kernel): a workgroup of four waves owns 64 * MR rows (16 * MR per wave) x 16 * NC
// columns; the weight k-blocks of its column tile are staged in LDS once and applied to every row of the tile. The packed K of a
// layer is formed as the four quarters the four waves of a stepped tile form (gemm_tile in rc_gemm.hip: wave w chains the k-blocks
// of [w Kp / 4, (w + 1) Kp / 4)), each quarter with the same instructions in the same order (rc_mma.h: mma_chunk / mma_kblock), and
// the quarters are summed in the stepped epilogues' order:
//   linear1 / linear2 / init_net: ((q0 + q1) + q2) + q3 + bias
//   LSTM layer step:              (q0 + q1) + (q2 + q3) + bias -- q0 + q1 is the hoisted x half, stored in fp32 between the launches
// so every output carries the bits of the stepped launches (rc_lstm_step) in each gemm mode.
#include "rc_internal.h"
#include "rc_gates.h"
#include "rc_mma.h"
#include "rc_pack.h"

#define RC_SG_STAGE 4         // k-blocks of weights staged in LDS per round

// BWD: the epilogues of the reverse recurrence (RC_SG_BPLAIN, RC_SG_BSTEP) in place of the forward's; the K loop is the same code.
template <int MR, int NC, bool SPLIT, bool BWD = false>
__global__ __launch_bounds__(256) void rc_subnet_gemm_kernel(const SubGemm G) {
    constexpr int U = SPLIT ? 192 : 128;                 // uint4 per (16-column block, 32-k block): three bf16 planes, or two fp32 chunks
    constexpr int ROWS = 64 * MR, COLS = 16 * NC, LD = COLS + 4;
    __shared__ __attribute__((aligned(16))) u32x4 s_w[RC_SG_STAGE * NC * U];
    __shared__ __attribute__((aligned(16))) float s_o[ROWS * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, kq = lane >> 4;
    const int m0 = blockIdx.x * ROWS, cb0 = blockIdx.y * NC;
    const float* pa[MR];
#pragma unroll
    for (int r = 0; r < MR; ++r) {
        const int row = min(m0 + wave * 16 * MR + 16 * r + i, G.M - 1);    // rows past the end load a valid row and are not stored
        pa[r] = G.A + rc_pk(row, 4 * kq, G.lda);
    }
    const int Qs = G.Kp / 32, nkb = Qs / 4;                               // k-blocks per quarter (Kp % 128 == 0)
    const u32x4* Wv = reinterpret_cast<const u32x4*>(SPLIT ? G.Ws : (const void*)G.W);
    f32x4 sum[MR][NC], acc[MR][NC];
    for (int c = G.c0; c < G.c1; ++c) {
#pragma unroll
        for (int r = 0; r < MR; ++r)
#pragma unroll
            for (int j = 0; j < NC; ++j) acc[r][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kb0 = c * nkb; kb0 < (c + 1) * nkb; kb0 += RC_SG_STAGE) {
            const int ng = min(RC_SG_STAGE, (c + 1) * nkb - kb0);
            __syncthreads();                                              // the previous round's weights are consumed
            for (int idx = tid; idx < ng * NC * U; idx += 256) {
                const int g = idx / (NC * U), rem = idx - g * NC * U, j = rem / U, e = rem - j * U;
                const int cb = min(cb0 + j, G.ncb - 1);                   // column blocks past the packing: a valid block, not stored
                s_w[idx] = Wv[((long long)cb * Qs + kb0 + g) * U + e];
            }
            __syncthreads();
            for (int g = 0; g < ng; ++g) {
                const long long aoff = (long long)((kb0 + g) * 32 - G.a_koff) * 16;
                if constexpr (SPLIT) {
                    FragS<MR, NC, false> f;
#pragma unroll
                    for (int r = 0; r < MR; ++r) {
                        f.a0[r] = *reinterpret_cast<const f32x4*>(pa[r] + aoff);
                        f.a1[r] = *reinterpret_cast<const f32x4*>(pa[r] + aoff + 256);
                    }
#pragma unroll
                    for (int j = 0; j < NC; ++j)
#pragma unroll
                        for (int p = 0; p < 3; ++p) f.b[j][p] = s_w[(g * NC + j) * U + p * 64 + lane];
                    mma_kblock(f, acc);
                } else {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {                         // the k-block's two 16-k chunks, in k order
                        Frag<MR, NC> f;
#pragma unroll
                        for (int r = 0; r < MR; ++r) f.a[r] = *reinterpret_cast<const f32x4*>(pa[r] + aoff + 256 * h);
#pragma unroll
                        for (int j = 0; j < NC; ++j) f.b[j] = __builtin_bit_cast(f32x4, s_w[(g * NC + j) * U + h * 64 + lane]);
                        mma_chunk<MR, NC>(f, acc);
                    }
                }
            }
        }
        // quarters summed left to right: ((q0 + q1) + q2) + q3 for dense layers, q0 + q1 (x half), q2 + q3 (recurrent half)
#pragma unroll
        for (int r = 0; r < MR; ++r)
#pragma unroll
            for (int j = 0; j < NC; ++j) sum[r][j] = c == G.c0 ? acc[r][j] : sum[r][j] + acc[r][j];
    }
    // C layout of 16x16: column lane & 15, row (lane >> 4) * 4 + element
#pragma unroll
    for (int r = 0; r < MR; ++r)
#pragma unroll
        for (int j = 0; j < NC; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) s_o[(wave * 16 * MR + 16 * r + 4 * kq + e) * LD + 16 * j + i] = sum[r][j][e];
    __syncthreads();
    constexpr int C4 = COLS / 4;
    for (int item = tid; item < ROWS * C4; item += 256) {
        const int rl = item / C4, q4 = item - rl * C4;
        const int row = m0 + rl, col = cb0 * 16 + 4 * q4;
        if (row >= G.M || col >= G.ncb * 16 || col >= G.N) continue;
        f32x4 v = *reinterpret_cast<const f32x4*>(&s_o[rl * LD + 4 * q4]);
        if constexpr (BWD) {
            if (G.epi == RC_SG_BPLAIN) {
                const long long orow = G.out_map ? G.out_map[row] : row;
                *reinterpret_cast<f32x4*>(&G.out[orow * G.ldo + col]) = v;
                continue;
            }
            // RC_SG_BSTEP: columns = four consecutive hidden units
            const long long ci = (long long)row * G.H + col;
            if (row >= G.n_next) v = *reinterpret_cast<const f32x4*>(&G.dfin_h[ci]);     // the sequence's last frame: no step t + 1
            const long long arow = G.dha_map ? G.dha_map[row] : row;
            v += *reinterpret_cast<const f32x4*>(&G.dh_above[arow * G.H + col]);
            const f32x4 c4 = *reinterpret_cast<const f32x4*>(&G.tape_c[ci]);
            const f32x4 cp4 = *reinterpret_cast<const f32x4*>(&G.c_prev[ci]);
            const f32x4 dcn = *reinterpret_cast<const f32x4*>(&G.cst[ci]);
            f32x4 dcp, dg[4];                                                 // dg[gate][unit]
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(&G.tape_g[(long long)row * 4 * G.H + 4 * (col + q)]);
                float d0, d1, d2, d3, dp;
                rc_lstm_cell_backward(a[0], a[1], a[2], a[3], c4[q], cp4[q], v[q], dcn[q], d0, d1, d2, d3, dp);
                const f32x4 d = {d0, d1, d2, d3};
                dcp[q] = dp;
                *reinterpret_cast<f32x4*>(&G.hout[rc_pk(row, 4 * (col + q), 4 * G.H)]) = d;
                *reinterpret_cast<f32x4*>(&G.hseq[rc_pk(G.hseq_row0 + row, 4 * (col + q), 4 * G.H)]) = d;
                dg[0][q] = d[0]; dg[1][q] = d[1]; dg[2][q] = d[2]; dg[3][q] = d[3];
            }
            *reinterpret_cast<f32x4*>(&G.cst[ci]) = dcp;
            float* dr = G.dgates + (long long)G.out_map[row] * 4 * G.H + col;
#pragma unroll
            for (int g = 0; g < 4; ++g) *reinterpret_cast<f32x4*>(dr + (long long)g * G.H) = dg[g];
            continue;
        }
        if (G.epi == RC_SG_HALF) {
            *reinterpret_cast<f32x4*>(&G.out[(long long)row * G.ldo + col]) = v;
            continue;
        }
        const f32x4 b = *reinterpret_cast<const f32x4*>(&G.bias[col]);
        if (G.epi == RC_SG_LSTM) {                                        // four consecutive columns = the i, f, g, o gates of one unit
            f32x4 g4 = *reinterpret_cast<const f32x4*>(&G.pre[(long long)row * G.ldp + col]) + v;
            g4 += b;
            const int unit = col >> 2;
            const long long ci = (long long)row * G.H + unit;
            float cn, hn;
            float ai, af, ag, ao;
            rc_lstm_cell_acts(g4[0], g4[1], g4[2], g4[3], G.cst[ci], cn, hn, ai, af, ag, ao);
            G.cst[ci] = cn;
            if (G.tape_g) {
                *reinterpret_cast<f32x4*>(&G.tape_g[(long long)row * 4 * G.H + col]) = f32x4{ai, af, ag, ao};
                G.tape_c[ci] = cn;
            }
            G.hout[rc_pk(row, unit, G.H)] = hn;
            G.hseq[rc_pk(G.hseq_row0 + row, unit, G.H)] = hn;
            continue;
        }
        v += b;
        if (G.epi == RC_SG_RELU) { v[0] = fmaxf(v[0], 0.0f); v[1] = fmaxf(v[1], 0.0f); v[2] = fmaxf(v[2], 0.0f); v[3] = fmaxf(v[3], 0.0f); }
        const long long orow = G.out_map ? G.out_map[row] : row;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (col + q < G.N) G.out[G.out_packed ? rc_pk(orow, col + q, G.ldo) : orow * G.ldo + col + q] = v[q];
    }
}

template <bool BWD>
static void launch_subnet_gemm(const SubGemm& G, int split, int tall, hipStream_t s) {
    if (G.M <= 0) return;
    // tall launches (every frame of a chunk; init_net): 256-row tiles whatever M, so each staged weight k-block serves 256 A rows. A time
    // step's active rows: 256-row tiles above 512 rows, else 64-row tiles, 16 columns wide at most 64 rows (more workgroups streaming
    // slices of W_hh). Below 513 rows the step launches never run the 256-row instantiation: its kernel-trace entries are the tall GEMMs.
    const int mr = (tall || G.M > 512) ? 4 : 1, nc = (tall || G.M > 64) ? 4 : 1;
    const int cbs = (min(G.N, G.ncb * 16) + 15) / 16;
    const dim3 grid((G.M + 64 * mr - 1) / (64 * mr), (cbs + nc - 1) / nc), block(256);
#define RC_SG_GO(MR, NC)                                                                                   \
    do {                                                                                                   \
        if (split) hipLaunchKernelGGL((rc_subnet_gemm_kernel<MR, NC, true, BWD>), grid, block, 0, s, G);  \
        else hipLaunchKernelGGL((rc_subnet_gemm_kernel<MR, NC, false, BWD>), grid, block, 0, s, G);       \
    } while (0)
    if (mr == 4) RC_SG_GO(4, 4);
    else if (nc == 4) RC_SG_GO(1, 4);
    else RC_SG_GO(1, 1);
#undef RC_SG_GO
}

void rc_launch_subnet_gemm(const SubGemm& G, int split, int tall, hipStream_t s) { launch_subnet_gemm<false>(G, split, tall, s); }
void rc_launch_subnet_gemm_bwd(const SubGemm& G, int split, int tall, hipStream_t s) { launch_subnet_gemm<true>(G, split, tall, s); }

__global__ void rc_subnet_pack_kernel(const float* src, int cols, const int* map, float* dst, int ld, int rows) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)rows * ld) return;
    const int j = (int)(idx / ld), k = (int)(idx - (long long)j * ld);
    const long long sr = map ? map[j] : j;
    dst[rc_pk(j, k, ld)] = k < cols ? src[sr * cols + k] : 0.0f;
}

void rc_launch_subnet_pack(const float* src, int cols, const int* map, float* dst, int ld, int rows, hipStream_t s) {
    const long long n = (long long)rows * ld;
    if (n <= 0) return;
    hipLaunchKernelGGL(rc_subnet_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, cols, map, dst, ld, rows);
}

// hp: per layer (+ l * hl) two copies of h [rows, H] in rc_pk order, ps floats apart (step t writes copy t & 1); cp: per layer (+ l * cl) c
__global__ void rc_subnet_state_kernel(float* hp, long long hl, long long ps, const int* par, float* cp, long long cl, float* h, float* c,
                                       const int* perm, int nr, int n, int H, int in) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= 2ll * nr * H) return;
    const int l = (int)(idx / ((long long)nr * H));
    const long long rem = idx - (long long)l * nr * H;
    const int r = (int)(rem / H), e = (int)(rem - (long long)r * H);
    const long long user = ((long long)l * n + perm[r]) * H + e;
    float* hr = hp + l * hl + (in ? 1 : par[r]) * ps + rc_pk(r, e, H);     // (the first step, t = 0, reads copy 1)
    float* cr = cp + l * cl + (long long)r * H + e;
    if (in) {
        *hr = h ? h[user] : 0.0f;
        *cr = c ? c[user] : 0.0f;
    } else {
        if (h) h[user] = *hr;
        if (c) c[user] = *cr;
    }
}

void rc_launch_subnet_state(float* hp, long long hl, long long ps, const int* par, float* cp, long long cl, float* h, float* c,
                            const int* perm, int nr, int n, int H, int in, hipStream_t s) {
    const long long tot = 2ll * nr * H;
    hipLaunchKernelGGL(rc_subnet_state_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, hp, hl, ps, par, cp, cl, h, c, perm,
                       nr, n, H, in);
}

__global__ void rc_subnet_unpack_kernel(const float* src, int ld, const int* map, float* dst, int cols, int rows) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)rows * cols) return;
    const int j = (int)(idx / cols), k = (int)(idx - (long long)j * cols);
    dst[(long long)map[j] * cols + k] = src[rc_pk(j, k, ld)];
}

void rc_launch_subnet_unpack(const float* src, int ld, const int* map, float* dst, int cols, int rows, hipStream_t s) {
    const long long n = (long long)rows * cols;
    if (n <= 0) return;
    hipLaunchKernelGGL(rc_subnet_unpack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, ld, map, dst, cols, rows);
}

__global__ void rc_subnet_bstate_kernel(float* a, float* b, long long ls, const float* src_a, const float* src_b, float* dst_b,
                                        const int* perm, int nr, int n, int H, int in) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= 2ll * nr * H) return;
    const int l = (int)(idx / ((long long)nr * H));
    const long long rem = idx - (long long)l * nr * H;
    const int r = (int)(rem / H);
    const long long user = ((long long)l * n + perm[r]) * H + (rem - (long long)r * H);
    if (in) {
        if (a) a[l * ls + rem] = src_a ? src_a[user] : 0.0f;
        if (b) b[l * ls + rem] = src_b ? src_b[user] : 0.0f;
    } else if (dst_b) {
        dst_b[user] = b[l * ls + rem];
    }
}

void rc_launch_subnet_bstate(float* a, float* b, long long ls, const float* src_a, const float* src_b, float* dst_b, const int* perm,
                             int nr, int n, int H, int in, hipStream_t s) {
    const long long tot = 2ll * nr * H;
    hipLaunchKernelGGL(rc_subnet_bstate_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, a, b, ls, src_a, src_b, dst_b, perm,
                       nr, n, H, in);
}

// ---- packings written on the device: the index arithmetic and the truncation split of pack_weights / pack_weights_split (rc_api.cpp),
// rc_pack_store in rc_pack.h ----
__global__ void rc_subnet_transpose_kernel(const float* Wl, int H, float* WT, unsigned short* WTs) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= 8ll * H * H) return;
    const int n = (int)(idx / (4 * H)), k = (int)(idx - (long long)n * 4 * H);      // the transposed operand's column n < 2H and k < 4H
    // Wl's element (column k, k index n): [cb][q][lane][4] with Q = 2H / 16
    const float v = Wl[((((long long)(k >> 4) * (2 * H / RC_KC) + (n >> 4)) * 64 + ((n >> 2) & 3) * 16 + (k & 15)) << 2) + (n & 3)];
    rc_pack_store(WT, WTs, 4 * H, n, k, v);
}

void rc_launch_subnet_transpose(const float* Wl, int H, float* WT, void* WTs, hipStream_t s) {
    const long long n = 8ll * H * H;
    hipLaunchKernelGGL(rc_subnet_transpose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, Wl, H, WT, (unsigned short*)WTs);
}

// ---- in-place repack of one sub-net's tensors (rc_update_subnet_weights): what make_dense / rc_finalize_weights pack on the host ---------
// dense layer from the row-major tensor W [N, K]: element (n, k) of the padded [Np, Kp] matrix, zeros in the padding
__global__ void rc_repack_dense_kernel(const float* Wsrc, int N, int K, int Np, int Kp, float* W, unsigned short* Ws) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)Np * Kp) return;
    const int n = (int)(idx / Kp), k = (int)(idx - (long long)n * Kp);
    rc_pack_store(W, Ws, Kp, n, k, (n < N && k < K) ? Wsrc[(long long)n * K + k] : 0.0f);
}

void rc_launch_repack_dense(const float* Wsrc, int N, int K, int Np, int Kp, float* W, void* Ws, hipStream_t s) {
    const long long n = (long long)Np * Kp;
    hipLaunchKernelGGL(rc_repack_dense_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, Wsrc, N, K, Np, Kp, W, (unsigned short*)Ws);
}

// LSTM layer from weight_ih, weight_hh [4H, H] and the two biases [4H]: packed column n' <-> torch row g * H + 4 * cb + u (cb = n' / 16,
// u = (n' % 16) / 4, g = n' % 4), k < H from weight_ih, else weight_hh; bl[n'] = bias_ih + bias_hh of that row
__global__ void rc_repack_lstm_kernel(const float* wi, const float* wh, const float* bi, const float* bh, int H, float* W, unsigned short* Ws,
                                      float* bl) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= 8ll * H * H) return;
    const int np = (int)(idx / (2 * H)), k = (int)(idx - (long long)np * 2 * H);
    const long long r = (long long)(np & 3) * H + 4 * (np >> 4) + ((np & 15) >> 2);
    rc_pack_store(W, Ws, 2 * H, np, k, k < H ? wi[r * H + k] : wh[r * H + (k - H)]);
    if (k == 0) bl[np] = bi[r] + bh[r];
}

void rc_launch_repack_lstm(const float* wi, const float* wh, const float* bi, const float* bh, int H, float* W, void* Ws, float* bl,
                           hipStream_t s) {
    const long long n = 8ll * H * H;
    hipLaunchKernelGGL(rc_repack_lstm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, wi, wh, bi, bh, H, W, (unsigned short*)Ws, bl);
}
