// The evaluators' SVD alignments on the device (articulate/evaluator.py:195-209, 298-312 through art.math.svd_rotate, angular.py:144-184),
// gfx950: per frame the R / t / s that carry the predicted joints onto the true ones and, separately, the predicted mesh onto the true
// mesh, and the errors that remain. This is NOT rc_metrics.hip's Procrustes: the scale is the ratio of the two spreads, the fit runs on
// the 24 joints or on all V vertices, and an improper V U^T has ROW 2 negated (angular.py:175-177), which is not the Kabsch rotation.
//
//   * rc_align_frame_kernel (a wave per frame): both joint chains in DOUBLE (a fit divides by its smallest singular value: the float32
//     chain of wave_body_fk would hand it 1e-7 s1 / s3), the joint fit on the 24 points, and the mesh fit WITHOUT a vertex:
//     a skinned vertex is p_v = sum_j w[v,j] A_j x~_v with A_j = [G_j | T_j] (3x4) and x~_v = (x_v, 1), so with B_k the truth's transforms
//         sum_v p_v t_v^T = sum_{j,k} A_j C[j,k] B_k^T,   sum_v p_v = sum_j A_j m_j,   sum_v |p_v|^2 = tr sum_{j,k} A_j C[j,k] A_k^T,
//     C[j,k] = sum_v w[v,j] w[v,k] x~_v x~_v^T (4x4, symmetric, and C[k,j] = C[j,k]) and m_j = sum_v w[v,j] x~_v built once per mesh on the
//     host in double (rc_api.cpp: fold_align). Only the pairs j <= k with a non-zero C are listed, so sparse skinning weights pay. The lanes
//     take the pairs in turn, 11 double sums each, added by a fixed xor butterfly. The kernel then writes the 24 ALIGNED difference
//     transforms D_j = (Gt_j - s R Gp_j | Tt_j - s R Tp_j - t): the weights of a vertex sum to one, so t_v - (s R p_v + t) = sum_j w[v,j] D_j x~_v
//     is one blend per vertex, as in rc_motion.hip;
//   * rc_align_sweep_kernel (rc_motion_sweep_kernel's shape: a thread owns four vertices, weights in registers, a workgroup walks the <= 32
//     frames of a block of ONE group): per (frame, slab) the sum of the vertex errors, in double -- a mean needs no per-vertex statistics,
//     so the six double accumulators per vertex of rc_motion_sweep_kernel are not here;
//   * rc_align_finish_kernel (a workgroup per group): the column sums of the 24 joint errors and of the frame totals of the vertex error,
//     each over eight interleaved runs of frames in index order, merged by a fixed tree.
// No floating-point atomics; every sum has an order fixed by the frame, the slab or the group alone, so two calls give the same bits and
// a group's numbers are those of a call with that group alone.
//
// The rotation. H = (src - mu_s)^T (dst - mu_d) = U S V^T, Q = V U^T: hestenes3 on H leaves W = H V = U S with orthogonal columns and
// V (proper), so u_i = w_i / |w_i| and Q = sum_i v_i u_i^T -- improper exactly when det H < 0, which is what the reference's LAPACK
// returns too (Q is the orthogonal polar factor of H^T, unique for a full-rank H). det Q < -0.9: row 2 of Q is negated.
// Rank-deficient H (columns of W below 1e-13 of the largest): the missing left singular vectors complete U to a PROPER rotation (one
// missing: the cross product of the other two; two missing: the coordinate axis least aligned with u_1, orthogonalised, then the cross
// product; H = 0: R = I), so R is finite and proper; LAPACK's choice there is arbitrary and no test pins it. The scale is the IEEE value
// of the reference's own expression sqrt(sum |dst - mu_d|^2 / sum |src - mu_s|^2): inf or NaN where the source has no spread.
#include "../../include/robustcap_hip.h"
#include "rc_device.h"

#define ALN_VPT 4
#define ALN_SLAB (256 * ALN_VPT)
#define ALN_FG RC_MOTION_FG
#define ALN_FRAME_FLOATS 312   // per frame of scratch: 24 aligned joint errors | 288 aligned difference transforms

namespace {

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ int align_group_of(const MotionGroup* __restrict__ tab, int groups, int blk) {
    int lo = 0, hi = groups - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].blk0 <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

struct Fit { double R[3][3], t[3], s; };

__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
// u_a = the coordinate axis least aligned with u_g, made orthogonal to it; u_b = u_g x u_a
__device__ __forceinline__ void complete_from_one(const double* ug, double* ua, double* ub) {
    const double x = fabs(ug[0]), y = fabs(ug[1]), z = fabs(ug[2]);
    const int ax = (x <= y && x <= z) ? 0 : (y <= z ? 1 : 2);
    const double d = ax == 0 ? ug[0] : (ax == 1 ? ug[1] : ug[2]);
    double e[3] = {(ax == 0 ? 1.0 : 0.0) - d * ug[0], (ax == 1 ? 1.0 : 0.0) - d * ug[1], (ax == 2 ? 1.0 : 0.0) - d * ug[2]};
    const double n = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) ua[c] = e[c] / n;
    cross3(ug, ua, ub);
}

// angular.py:170-178 on H = src^T dst (centred or not): see the file comment
__device__ void svd_rotation(const double (&H)[3][3], double (&R)[3][3]) {
    double W[3][3], V[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) W[r][c] = H[r][c];
    hestenes3(W, V);
    double nrm[3], u[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) nrm[i] = sqrt(W[0][i] * W[0][i] + W[1][i] * W[1][i] + W[2][i] * W[2][i]);
    const double tiny = 1e-13 * fmax(nrm[0], fmax(nrm[1], nrm[2]));
    bool good[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        good[i] = nrm[i] > tiny;                                   // H = 0 (or NaN): none
#pragma unroll
        for (int c = 0; c < 3; ++c) u[i][c] = good[i] ? W[c][i] / nrm[i] : 0.0;
    }
    const int ng = (int)good[0] + (int)good[1] + (int)good[2];
    if (ng == 2) {
        if (!good[0]) cross3(u[1], u[2], u[0]);
        else if (!good[1]) cross3(u[2], u[0], u[1]);
        else cross3(u[0], u[1], u[2]);
    } else if (ng == 1) {
        if (good[0]) complete_from_one(u[0], u[1], u[2]);
        else if (good[1]) complete_from_one(u[1], u[2], u[0]);
        else complete_from_one(u[2], u[0], u[1]);
    } else if (ng == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) u[i][c] = i == c ? 1.0 : 0.0;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[r][c] = (V[r][0] * u[0][c] + V[r][1] * u[1][c]) + V[r][2] * u[2][c];
    const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                       R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
    if (det < -0.9) {                                              // angular.py:175-177: v[i, 2] is ROW 2 of V
#pragma unroll
        for (int c = 0; c < 3; ++c) R[2][c] = -R[2][c];
    }
}

// angular.py:159-182 from the sums: H = sum (src - mu_s)(dst - mu_d)^T, ss = sum |src - mu_s|^2, dd = sum |dst - mu_d|^2 (the means are
// zero without RC_ALIGN_T)
__device__ __forceinline__ void fit_from_sums(unsigned what, const double (&H)[3][3], double ss, double dd, const double* mu_s,
                                              const double* mu_d, Fit& f) {
    f.s = (what & RC_ALIGN_S) ? sqrt(dd / ss) : 1.0;
    if (what & RC_ALIGN_R) {
        svd_rotation(H, f.R);
    } else {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) f.R[r][c] = r == c ? 1.0 : 0.0;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
        f.t[r] = -f.s * ((f.R[r][0] * mu_s[0] + f.R[r][1] * mu_s[1]) + f.R[r][2] * mu_s[2]) + mu_d[r];
}

// the fit of m points (src, dst [m][3], global or LDS) by one wave: the lanes take the points in turn, two passes (means, then centred
// sums: a set without spread gives exactly 0), a fixed xor butterfly. Every lane leaves with the same Fit.
template <class T>
__device__ void wave_fit_points(const T* src, const T* dst, int m, unsigned what, int lane, Fit& f) {
    double mu_s[3] = {0.0, 0.0, 0.0}, mu_d[3] = {0.0, 0.0, 0.0};
    if (what & RC_ALIGN_T) {
        for (int p = lane; p < m; p += 64) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { mu_s[c] += (double)src[3 * (long long)p + c]; mu_d[c] += (double)dst[3 * (long long)p + c]; }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) { mu_s[c] = wave_sum_d(mu_s[c]) / m; mu_d[c] = wave_sum_d(mu_d[c]) / m; }
    }
    double H[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, ss = 0.0, dd = 0.0;
    for (int p = lane; p < m; p += 64) {
        double a[3], b[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a[c] = (double)src[3 * (long long)p + c] - mu_s[c];
            b[c] = (double)dst[3 * (long long)p + c] - mu_d[c];
            ss += a[c] * a[c];
            dd += b[c] * b[c];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) H[r][c] += a[r] * b[c];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) H[r][c] = wave_sum_d(H[r][c]);
    ss = wave_sum_d(ss);
    dd = wave_sum_d(dd);
    fit_from_sums(what, H, ss, dd, mu_s, mu_d, f);
}

__device__ __forceinline__ void store_fit(float* __restrict__ o, const Fit& f) {     // R [9] | t [3] | s
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[3 * r + c] = (float)f.R[r][c];
        o[9 + r] = (float)f.t[r];
    }
    o[12] = (float)f.s;
}

// one body's joint chain in double: wave_body_fk's steps (articulate/model.py:229-235) on float32 local rotations and rest constants
struct ChainD {
    double G[24][9];     // global rotations
    double P[24][3];     // joints, root at the origin
    double A[24][12];    // [G_j | T_j], T_j = P_j - G_j jrest_j: row r is A[j][4 r .. 4 r + 3]
};
__device__ __forceinline__ void wave_chain_d(const BodyConst* body, const float (*Rl)[9], ChainD& s, int lane) {
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) s.G[0][k] = (double)Rl[0][k];
        s.P[0][0] = s.P[0][1] = s.P[0][2] = 0.0;
    }
    __syncthreads();
    const int lvl = lane < 24 ? body->level[lane] : -1;
    for (int l = 1; l < 10; ++l) {
        if (lvl == l) {
            const int p = body->parent[lane];
            double g[9], pb[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    g[3 * r + c] = (s.G[p][3 * r] * (double)Rl[lane][c] + s.G[p][3 * r + 1] * (double)Rl[lane][3 + c]) +
                                   s.G[p][3 * r + 2] * (double)Rl[lane][6 + c];
                pb[r] = (s.G[p][3 * r] * (double)body->bone[lane][0] + s.G[p][3 * r + 1] * (double)body->bone[lane][1]) +
                        s.G[p][3 * r + 2] * (double)body->bone[lane][2];
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) s.G[lane][k] = g[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) s.P[lane][k] = pb[k] + s.P[p][k];
        }
        __syncthreads();
    }
    if (lane < 24) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double gj = (s.G[lane][3 * r] * (double)body->jrest[lane][0] + s.G[lane][3 * r + 1] * (double)body->jrest[lane][1]) +
                              s.G[lane][3 * r + 2] * (double)body->jrest[lane][2];
#pragma unroll
            for (int c = 0; c < 3; ++c) s.A[lane][4 * r + c] = s.G[lane][3 * r + c];
            s.A[lane][4 * r + 3] = s.P[lane][r] - gj;
        }
    }
    __syncthreads();
}

// E = A C: A 3x4 (row-major, 12), C 4x4 symmetric (16)
__device__ __forceinline__ void mul_34_44(const double* A, const double* C, double* E) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            E[4 * r + c] = ((A[4 * r] * C[c] + A[4 * r + 1] * C[4 + c]) + A[4 * r + 2] * C[8 + c]) + A[4 * r + 3] * C[12 + c];
}
// sum over all entries of E .* B (3x4 each): tr(E B^T)
__device__ __forceinline__ double dot12(const double* E, const double* B) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 12; ++k) s += E[k] * B[k];
    return s;
}

}  // namespace

// scratch row of frame b: [0, 24) the aligned joint errors, [24, 312) the aligned difference transforms (mesh only).
// fold == nullptr: no mesh (RC_MOTION_NO_MESH): the mesh halves of per_frame and xform are NaN.
__global__ __launch_bounds__(64) void rc_align_frame_kernel(const BodyConst* __restrict__ body_g, const float* __restrict__ pose_p,
                                                            const float* __restrict__ pose_t, unsigned what,
                                                            const double* __restrict__ fold_m, const AlignPair* __restrict__ pairs,
                                                            int n_pairs, int V, float* __restrict__ scratch,
                                                            float* __restrict__ per_frame, float* __restrict__ xform) {
    __shared__ ChainD sp, st;
    __shared__ float Rlp[24][9], Rlt[24][9];
    __shared__ float s_je[24];
    __shared__ __attribute__((aligned(16))) BodyConst s_body;
    const long long b = blockIdx.x;
    const int lane = threadIdx.x;
    stage_body(&s_body, body_g, lane, 64);
    for (int e = lane; e < 216; e += 64) { Rlp[e / 9][e % 9] = pose_p[b * 216 + e]; Rlt[e / 9][e % 9] = pose_t[b * 216 + e]; }
    __syncthreads();
    wave_chain_d(&s_body, Rlp, sp, lane);
    wave_chain_d(&s_body, Rlt, st, lane);
    float* __restrict__ row = scratch + b * ALN_FRAME_FLOATS;
    // ---- the joint fit (evaluator.py:198-207) and the aligned joint errors (:210)
    Fit fj;
    wave_fit_points<double>(&sp.P[0][0], &st.P[0][0], 24, what, lane, fj);
    if (lane < 24) {
        double e2 = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double d = (fj.s * ((fj.R[r][0] * sp.P[lane][0] + fj.R[r][1] * sp.P[lane][1]) + fj.R[r][2] * sp.P[lane][2]) + fj.t[r]) -
                             st.P[lane][r];
            e2 += d * d;
        }
        const float je = (float)sqrt(e2);
        row[lane] = je;
        s_je[lane] = je;
    }
    __syncthreads();
    if (lane == 0) {
        if (per_frame) {
            double s = 0.0;
            for (int j = 0; j < 24; ++j) s += (double)s_je[j];
            per_frame[b * 2] = (float)(s / 24.0);
        }
        if (xform) store_fit(xform + b * 26, fj);
    }
    if (!pairs) {
        if (lane == 0 && per_frame) per_frame[b * 2 + 1] = __builtin_nanf("");
        if (xform && lane < 13) xform[b * 26 + 13 + lane] = __builtin_nanf("");
        return;
    }
    // ---- the mesh fit from the fold (evaluator.py:301-310 without a vertex)
    double H[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, pp = 0.0, tt = 0.0;
    for (int q = lane; q < n_pairs; q += 64) {
        const AlignPair* __restrict__ pr = pairs + q;
        const int j = pr->j, k = pr->k;
        double C[16], E[12];
#pragma unroll
        for (int i = 0; i < 16; ++i) C[i] = pr->c[i];
        const double w = j == k ? 1.0 : 2.0;
        mul_34_44(sp.A[j], C, E);                                  // A_j C
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                H[r][c] += ((E[4 * r] * st.A[k][4 * c] + E[4 * r + 1] * st.A[k][4 * c + 1]) + E[4 * r + 2] * st.A[k][4 * c + 2]) +
                           E[4 * r + 3] * st.A[k][4 * c + 3];
        pp += w * dot12(E, sp.A[k]);
        if (j != k) {
            mul_34_44(sp.A[k], C, E);                              // A_k C (C[k,j] = C[j,k])
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    H[r][c] += ((E[4 * r] * st.A[j][4 * c] + E[4 * r + 1] * st.A[j][4 * c + 1]) + E[4 * r + 2] * st.A[j][4 * c + 2]) +
                               E[4 * r + 3] * st.A[j][4 * c + 3];
        }
        mul_34_44(st.A[j], C, E);                                  // B_j C
        tt += w * dot12(E, st.A[k]);
    }
    double sum_p[3] = {0.0, 0.0, 0.0}, sum_t[3] = {0.0, 0.0, 0.0};
    if (lane < 24) {
        const double* __restrict__ m = fold_m + 4 * lane;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            sum_p[r] = ((sp.A[lane][4 * r] * m[0] + sp.A[lane][4 * r + 1] * m[1]) + sp.A[lane][4 * r + 2] * m[2]) + sp.A[lane][4 * r + 3] * m[3];
            sum_t[r] = ((st.A[lane][4 * r] * m[0] + st.A[lane][4 * r + 1] * m[1]) + st.A[lane][4 * r + 2] * m[2]) + st.A[lane][4 * r + 3] * m[3];
        }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) H[r][c] = wave_sum_d(H[r][c]);
        sum_p[r] = wave_sum_d(sum_p[r]);
        sum_t[r] = wave_sum_d(sum_t[r]);
    }
    pp = wave_sum_d(pp);
    tt = wave_sum_d(tt);
    double mu_p[3] = {0.0, 0.0, 0.0}, mu_t[3] = {0.0, 0.0, 0.0};
    if (what & RC_ALIGN_T) {                                       // centre: sum (p - mu_p)(t - mu_t)^T = sum p t^T - V mu_p mu_t^T
#pragma unroll
        for (int r = 0; r < 3; ++r) { mu_p[r] = sum_p[r] / V; mu_t[r] = sum_t[r] / V; }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) H[r][c] -= (double)V * mu_p[r] * mu_t[c];
            pp -= (double)V * mu_p[r] * mu_p[r];
            tt -= (double)V * mu_t[r] * mu_t[r];
        }
    }
    Fit fm;
    fit_from_sums(what, H, pp, tt, mu_p, mu_t, fm);
    if (lane == 0 && xform) store_fit(xform + b * 26 + 13, fm);
    // ---- D_j = (Gt_j - s R Gp_j | Tt_j - s R Tp_j - t), the layout rc_motion_sweep_kernel reads
    for (int e = lane; e < 288; e += 64) {
        const int j = e / 12, q = e % 12, r = q >> 2, c = q & 3;
        const double rp = (fm.R[r][0] * sp.A[j][c] + fm.R[r][1] * sp.A[j][4 + c]) + fm.R[r][2] * sp.A[j][8 + c];
        double d = st.A[j][4 * r + c] - fm.s * rp;
        if (c == 3) d -= fm.t[r];
        row[24 + e] = (float)d;
    }
}

struct AlignVertexRegs {
    float x[ALN_VPT][3];
    float w[ALN_VPT][24];
};

// fpart[frame][slab] = sum over the slab's vertices of |t_v - (s R p_v + t)|, in double: a thread's four vertices in index order, the 64
// lanes of a wave by the xor butterfly, the four waves as (0 + 1) + (2 + 3)
__global__ __launch_bounds__(256) void rc_align_sweep_kernel(const BodyConst* __restrict__ body, const float* __restrict__ vt,
                                                             const float* __restrict__ w, int V, const MotionGroup* __restrict__ tab,
                                                             int groups, int n_slab, const float* __restrict__ scratch,
                                                             double* __restrict__ fpart) {
    __shared__ double s_sum[4][ALN_FG];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int blk = blockIdx.x, slab = blockIdx.y;
    const MotionGroup g = tab[align_group_of(tab, groups, blk)];
    const int b = blk - g.blk0;
    const long long left = g.frames - (long long)b * ALN_FG;
    const int nf = left < ALN_FG ? (int)left : ALN_FG;
    const long long f0 = g.frame0 + (long long)b * ALN_FG;
    const float* __restrict__ base = scratch + f0 * ALN_FRAME_FLOATS + 24;
    AlignVertexRegs r;
    const float jr[3] = {body->jroot[0], body->jroot[1], body->jroot[2]};
#pragma unroll
    for (int q = 0; q < ALN_VPT; ++q) {
        const int v = slab * ALN_SLAB + q * 256 + tid;
        const bool ok = v < V;
        const int vv = ok ? v : 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) r.x[q][c] = ok ? vt[3 * vv + c] - jr[c] : 0.0f;
#pragma unroll
        for (int j = 0; j < 24; ++j) r.w[q][j] = ok ? w[(long long)vv * 24 + j] : 0.0f;     // w = 0: a padding vertex adds exactly 0
    }
#pragma unroll 1
    for (int f = 0; f < nf; ++f) {
        const float* __restrict__ X = base + (long long)f * ALN_FRAME_FLOATS;     // wave-uniform: scalar loads
        float acc[ALN_VPT][12];
#pragma unroll
        for (int q = 0; q < ALN_VPT; ++q)
#pragma unroll
            for (int k = 0; k < 12; ++k) acc[q][k] = 0.0f;
#pragma unroll
        for (int j = 0; j < 24; ++j) {
            float xj[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) xj[k] = X[j * 12 + k];
#pragma unroll
            for (int q = 0; q < ALN_VPT; ++q)
#pragma unroll
                for (int k = 0; k < 12; ++k) acc[q][k] = fmaf(r.w[q][j], xj[k], acc[q][k]);
            if (j % 4 == 3) __builtin_amdgcn_sched_barrier(0);    // at most four joints' transforms (48 SGPRs) are requested ahead
        }
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < ALN_VPT; ++q) {
            float d[3];
#pragma unroll
            for (int c = 0; c < 3; ++c)
                d[c] = fmaf(acc[q][4 * c + 2], r.x[q][2], fmaf(acc[q][4 * c + 1], r.x[q][1], acc[q][4 * c] * r.x[q][0])) + acc[q][4 * c + 3];
            s += (double)norm3(d);
        }
        s = wave_sum_d(s);
        if (lane == 0) s_sum[wave][f] = s;
    }
    __syncthreads();
    if (tid < nf) fpart[(f0 + tid) * n_slab + slab] = (s_sum[0][tid] + s_sum[1][tid]) + (s_sum[2][tid] + s_sum[3][tid]);
}

// A workgroup per group. Column c < 24: joint error c; column 24: the frame totals of the vertex error (the slabs of a frame added in index
// order; the frame's mean goes to per_frame). Run q of 8 adds the group's frames q, q + 8, ... in index order; the runs merge as
// ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)).
__global__ __launch_bounds__(256) void rc_align_finish_kernel(const MotionGroup* __restrict__ tab, int V, int n_slab,
                                                              const float* __restrict__ scratch, const double* __restrict__ fpart,
                                                              float* __restrict__ joint_err, float* __restrict__ mesh_err,
                                                              float* __restrict__ per_frame) {
    __shared__ double s_run[8][32];
    const int tid = threadIdx.x, c = tid & 31, q = tid >> 5;
    const long long grp = blockIdx.x;
    const MotionGroup g = tab[grp];
    double acc = 0.0;
    if (c < 24) {
        for (long long i = q; i < g.frames; i += 8) acc += (double)scratch[(g.frame0 + i) * ALN_FRAME_FLOATS + c];
    } else if (c == 24 && fpart) {
        for (long long i = q; i < g.frames; i += 8) {
            const long long f = g.frame0 + i;
            double ft = 0.0;
            for (int s = 0; s < n_slab; ++s) ft += fpart[f * n_slab + s];
            if (per_frame) per_frame[f * 2 + 1] = (float)(ft / V);
            acc += ft;
        }
    }
    s_run[q][c] = acc;
    __syncthreads();
    if (q == 0 && c <= 24) {
        const double tot = ((s_run[0][c] + s_run[1][c]) + (s_run[2][c] + s_run[3][c])) + ((s_run[4][c] + s_run[5][c]) + (s_run[6][c] + s_run[7][c]));
        if (c < 24) {
            if (joint_err) joint_err[grp * 24 + c] = (float)(tot / (double)g.frames);
        } else if (mesh_err) {
            mesh_err[grp] = fpart ? (float)(tot / ((double)g.frames * (double)V)) : __builtin_nanf("");
        }
    }
}

// art.math.svd_rotate (angular.py:144-184) on point sets: a wave per set
__global__ __launch_bounds__(64) void rc_svd_rotate_kernel(const float* __restrict__ src, const float* __restrict__ dst, int m, unsigned what,
                                                           float* __restrict__ R, float* __restrict__ t, float* __restrict__ s,
                                                           float* __restrict__ moved) {
    const long long i = blockIdx.x;
    const int lane = threadIdx.x;
    const float* __restrict__ a = src + i * m * 3;
    Fit f;
    wave_fit_points<float>(a, dst + i * m * 3, m, what, lane, f);
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) if (R) R[i * 9 + 3 * r + c] = (float)f.R[r][c];
            if (t) t[i * 3 + r] = (float)f.t[r];
        }
        if (s) s[i] = (float)f.s;
    }
    if (moved) {
        for (int p = lane; p < m; p += 64) {
            const double x[3] = {(double)a[3 * (long long)p], (double)a[3 * (long long)p + 1], (double)a[3 * (long long)p + 2]};
#pragma unroll
            for (int r = 0; r < 3; ++r)
                moved[(i * m + p) * 3 + r] = (float)(f.s * ((f.R[r][0] * x[0] + f.R[r][1] * x[1]) + f.R[r][2] * x[2]) + f.t[r]);
        }
    }
}

void rc_launch_svd_rotate(const float* src, const float* dst, long long n, int m, unsigned what, float* R, float* t, float* s, float* moved,
                          hipStream_t st) {
    if (n <= 0) return;
    hipLaunchKernelGGL(rc_svd_rotate_kernel, dim3((unsigned)n), dim3(64), 0, st, src, dst, m, what, R, t, s, moved);
}
long long rc_align_scratch_floats(long long n) { return n * ALN_FRAME_FLOATS; }
long long rc_align_partial_doubles(int V, long long n, bool mesh) { return mesh ? n * ((V + ALN_SLAB - 1) / ALN_SLAB) : 0; }
void rc_launch_aligned_metrics(const BodyConst* body, const float* vt, const float* w, int V, const double* fold_m, const AlignPair* pairs,
                               int n_pairs, const MotionGroup* tab, int groups, long long blocks, const float* pose_p, const float* pose_t,
                               long long n, unsigned what, bool mesh, float* scratch, double* partial, float* joint_err, float* mesh_err,
                               float* per_frame, float* xform, hipStream_t st) {
    const int n_slab = (V + ALN_SLAB - 1) / ALN_SLAB;
    hipLaunchKernelGGL(rc_align_frame_kernel, dim3((unsigned)n), dim3(64), 0, st, body, pose_p, pose_t, what, mesh ? fold_m : nullptr,
                       mesh ? pairs : nullptr, n_pairs, V, scratch, per_frame, xform);
    const bool sweep = mesh && (mesh_err || per_frame);            // xform alone needs the fit, not the errors
    if (sweep)
        hipLaunchKernelGGL(rc_align_sweep_kernel, dim3((unsigned)blocks, (unsigned)n_slab), dim3(256), 0, st, body, vt, w, V, tab, groups, n_slab,
                           scratch, partial);
    if (joint_err || mesh_err || sweep)
        hipLaunchKernelGGL(rc_align_finish_kernel, dim3((unsigned)groups), dim3(256), 0, st, tab, V, n_slab, scratch, sweep ? partial : nullptr,
                           joint_err, mesh_err, per_frame);
}
