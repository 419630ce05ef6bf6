// FullMotionEvaluator on the device (articulate/evaluator.py:317-394), gfx950: the eleven (mean, mean of per-column std) rows of every
// motion ("group") of a concatenated batch in one stream-ordered call, and the per-joint column means behind PerJointErrorEvaluator
// (evaluator.py:155-215) and MeshErrorEvaluator (:256-314).
//
// Per group of N frames the reference forms [rows, columns] arrays and takes x.mean() and x.std(dim=0).mean() of each:
//   je, lae, gae, tre [N,24]   ve [N,V]   jkp, jkt [N-3,24]   te [N-fps,1]   masked je / lae / gae: columns of the first three.
// All groups have the same number of rows per column, so x.mean() is the mean of the column means; every row of the result is
// therefore made of per-COLUMN (mean, M2 = sum of squared deviations) pairs. Layout, after rc_metrics.hip:
//   * rc_motion_frame_kernel (a wave per frame): both joint chains with translation; the frame's 4 x 24 column values (je, lae, gae, tre),
//     both sets of translated joints (the stencils need neighbours), and the 24 difference transforms (Gt_j - Gp_j | Tt_j - Tp_j + c),
//     c = (tran_t - tran_p) - offset: skinning weights sum to one, so the vertex error needs nothing else;
//   * frames are cut into blocks of MOT_FG frames PER GROUP (a block never holds frames of two groups; a workgroup finds its group by
//     bisection of the table, like rc_eval_kernel);
//   * rc_motion_col_kernel (a workgroup per block, a thread per column, 145 columns): the block's (mean, M2) of each small column; the jerk
//     and one-second stencils are formed here, in double, from the stored joints, and never leave the group;
//   * rc_motion_sweep_kernel (rc_metrics_pve_kernel's shape: a thread owns MET_VPT vertices, weights in registers, and walks a block's
//     frames): per (block, vertex) the (mean, M2) of the vertex error -- no [N,V] array exists;
//   * rc_motion_vfinish_kernel per (group, slab) and rc_motion_finish_kernel per group merge the blocks in index order.
// The variance: inside a block the values are shifted by the block's FIRST value K (S1 = sum (x - K), S2 = sum (x - K)^2, in double on
// float32 values: the differences are exact), mean = K + S1 / n, M2 = S2 - S1^2 / n: the cancellation in M2 is relative to the block's own
// range, not to the column's mean. Blocks are merged by Chan's update, M2 = M2a + M2b + delta^2 na nb / (na + nb), which only adds
// non-negative terms. A column whose spread is far below its mean (the vertex error of a near-perfect prediction) therefore keeps the
// relative accuracy of double in its spread; the raw sum of squares would lose (mean / std)^2 of it.
// Every sum runs in a fixed order (frames of a block in index order, blocks in index order, columns in index order, a fixed LDS tree over
// the threads of the vertex finish): no floating-point atomics, two runs give the same bits, and a group's result depends on nothing
// outside the group.
#include "rc_device.h"

#define MET_VPT 4          // vertices per thread of the sweep (as rc_metrics.hip)
#define MET_SLAB (256 * MET_VPT)
#define MOT_FG RC_MOTION_FG
#define MOT_NCOL 145       // je 0..23 | lae 24..47 | gae 48..71 | tre 72..95 | jkp 96..119 | jkt 120..143 | te 144
#define MOT_FRAME_FLOATS 528   // per frame of scratch: 96 column values | 144 joint coordinates (p, t) | 288 difference transforms

namespace {

// group of workgroup `blk`: the last table entry with blk0 <= blk
__device__ __forceinline__ int motion_group_of(const MotionGroup* __restrict__ tab, int groups, int blk) {
    int lo = 0, hi = groups - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].blk0 <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

struct Stat { double mean, m2; };
// Chan's merge of (na, a) with (nb, b); na may be 0
__device__ __forceinline__ void stat_merge(double& na, Stat& a, double nb, const Stat& b) {
    if (nb <= 0.0) return;
    if (na <= 0.0) { na = nb; a = b; return; }
    const double n = na + nb, d = b.mean - a.mean;
    a.mean += d * (nb / n);
    a.m2 += b.m2 + d * d * (na * nb / n);
    na = n;
}
// rows of block b (of MOT_FG) among `rows` rows
__device__ __forceinline__ int block_rows(long long rows, int b) {
    const long long r = rows - (long long)b * MOT_FG;
    return r <= 0 ? 0 : (r < MOT_FG ? (int)r : MOT_FG);
}
__device__ __forceinline__ double unbiased_std(double m2, double n) {
    const double var = m2 / (n - 1.0);               // n == 1: 0 / 0, the NaN torch returns
    return sqrt(var < 0.0 ? 0.0 : var);
}

}  // namespace

__global__ __launch_bounds__(64) void rc_motion_frame_kernel(const BodyConst* __restrict__ body_g, const float* __restrict__ pose_p,
                                                             const float* __restrict__ tran_p, const float* __restrict__ pose_t,
                                                             const float* __restrict__ tran_t, int align, float* __restrict__ scratch) {
    __shared__ WaveScratch sp, st;
    __shared__ __attribute__((aligned(16))) BodyConst s_body;
    const long long b = blockIdx.x;
    const int lane = threadIdx.x;
    stage_body(&s_body, body_g, lane, 64);
    for (int e = lane; e < 216; e += 64) { sp.Rl[e / 9][e % 9] = pose_p[b * 216 + e]; st.Rl[e / 9][e % 9] = pose_t[b * 216 + e]; }
    float tp[3], tt[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { tp[c] = tran_p ? tran_p[b * 3 + c] : 0.0f; tt[c] = tran_t ? tran_t[b * 3 + c] : 0.0f; }
    __syncthreads();
    wave_body_fk(&s_body, sp, tp, lane);
    wave_body_fk(&s_body, st, tt, lane);
    float* __restrict__ row = scratch + b * MOT_FRAME_FLOATS;
    float off[3], cc[3];                                          // evaluator.py:371; c = (tran_t - tran_p) - offset
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        off[c] = (st.P[align][c] + tt[c]) - (sp.P[align][c] + tp[c]);
        cc[c] = (tt[c] - tp[c]) - off[c];
    }
    if (lane < 24) {
        float jp[3], jt[3], a[3], d[3], D[9], aa[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            jp[c] = sp.P[lane][c] + tp[c];
            jt[c] = st.P[lane][c] + tt[c];
            a[c] = (jp[c] + off[c]) - jt[c];
            d[c] = jp[c] - jt[c];
            row[96 + lane * 3 + c] = jp[c];
            row[168 + lane * 3 + c] = jt[c];
        }
        row[lane] = norm3(a);
        row[72 + lane] = norm3(d);
        mat3T_mul(sp.Rl[lane], st.Rl[lane], D);                   // the angle of rc_angle_between, in degrees
        rotmat_to_aa(D, aa);
        row[24 + lane] = (float)((double)norm3(aa) * 180.0 / 3.14159265358979323846);
        mat3T_mul(sp.G[lane], st.G[lane], D);
        rotmat_to_aa(D, aa);
        row[48 + lane] = (float)((double)norm3(aa) * 180.0 / 3.14159265358979323846);
    }
    for (int e = lane; e < 288; e += 64) {
        const int j = e / 12, q = e % 12, r = q >> 2, c = q & 3;
        row[240 + e] = c < 3 ? st.G[j][3 * r + c] - sp.G[j][3 * r + c] : (st.T[j][r] - sp.T[j][r]) + cc[r];
    }
}

// part[blk][MOT_NCOL] = (mean, M2) of the block's rows of every small column (a block without rows of a column: zeros, never read)
__global__ __launch_bounds__(192) void rc_motion_col_kernel(const MotionGroup* __restrict__ tab, int groups, int fps,
                                                            const float* __restrict__ scratch, Stat* __restrict__ part) {
    const int blk = blockIdx.x, col = threadIdx.x;
    if (col >= MOT_NCOL) return;
    const MotionGroup g = tab[motion_group_of(tab, groups, blk)];
    const int b = blk - g.blk0;
    const float* __restrict__ base = scratch + (g.frame0 + (long long)b * MOT_FG) * MOT_FRAME_FLOATS;   // the block's first frame
    const double f3 = (double)fps * (double)fps * (double)fps;
    const int kind = col < 96 ? 0 : (col < 144 ? 1 : 2);
    const int rows = block_rows(kind == 0 ? g.frames : (kind == 1 ? g.frames - 3 : g.frames - fps), b);
    double K = 0.0, s1 = 0.0, s2 = 0.0;
    for (int r = 0; r < rows; ++r) {
        const float* __restrict__ fr = base + (long long)r * MOT_FRAME_FLOATS;
        double x;
        if (kind == 0) {
            x = (double)fr[col];
        } else if (kind == 1) {                                   // evaluator.py:377-378; side 0: prediction, 1: truth
            const int o = 96 + (col - 96) * 3;                    // (col - 96) = side * 24 + joint: the joints are stored [side][joint][3]
            double e2 = 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double x0 = fr[o + c], x1 = fr[MOT_FRAME_FLOATS + o + c], x2 = fr[2 * MOT_FRAME_FLOATS + o + c],
                             x3 = fr[3 * MOT_FRAME_FLOATS + o + c];
                const double d = (((x3 - 3.0 * x2) + 3.0 * x1) - x0) * f3;
                e2 += d * d;
            }
            x = sqrt(e2);
        } else {                                                  // evaluator.py:379: joint 0, a window of fps frames
            const float* __restrict__ fw = fr + (long long)fps * MOT_FRAME_FLOATS;
            double e2 = 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double d = ((double)fw[96 + c] - (double)fr[96 + c]) - ((double)fw[168 + c] - (double)fr[168 + c]);
                e2 += d * d;
            }
            x = sqrt(e2);
        }
        if (r == 0) K = x;
        const double d = x - K;
        s1 += d;
        s2 += d * d;
    }
    Stat s = {0.0, 0.0};
    if (rows > 0) { s.mean = K + s1 / rows; s.m2 = s2 - s1 * s1 / rows; }
    part[(long long)blk * MOT_NCOL + col] = s;
}

// vertex data of the four vertices a thread owns (slab * MET_SLAB + q * 256 + tid): rest position and skinning weights
struct MotionVertexRegs {
    float x[MET_VPT][3];
    float w[MET_VPT][24];
};

// vpart[blk][V] = (mean, M2) over the block's frames of |x_t - (x_p + offset)| of every vertex
__global__ __launch_bounds__(256) void rc_motion_sweep_kernel(const BodyConst* __restrict__ body, const float* __restrict__ vt,
                                                              const float* __restrict__ w, int V, const MotionGroup* __restrict__ tab,
                                                              int groups, const float* __restrict__ scratch, Stat* __restrict__ vpart) {
    const int tid = threadIdx.x;
    const int blk = blockIdx.x, slab = blockIdx.y;
    const MotionGroup g = tab[motion_group_of(tab, groups, blk)];
    const int b = blk - g.blk0;
    const int nf = block_rows(g.frames, b);
    const float* __restrict__ base = scratch + (g.frame0 + (long long)b * MOT_FG) * MOT_FRAME_FLOATS + 240;
    MotionVertexRegs r;
    const float jr[3] = {body->jroot[0], body->jroot[1], body->jroot[2]};
#pragma unroll
    for (int q = 0; q < MET_VPT; ++q) {
        const int v = slab * MET_SLAB + q * 256 + tid;
        const bool ok = v < V;
        const int vv = ok ? v : 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) r.x[q][c] = ok ? vt[3 * vv + c] - jr[c] : 0.0f;
#pragma unroll
        for (int j = 0; j < 24; ++j) r.w[q][j] = ok ? w[(long long)vv * 24 + j] : 0.0f;
    }
    double K[MET_VPT], s1[MET_VPT], s2[MET_VPT];
#pragma unroll
    for (int q = 0; q < MET_VPT; ++q) { K[q] = 0.0; s1[q] = 0.0; s2[q] = 0.0; }
#pragma unroll 1
    for (int f = 0; f < nf; ++f) {
        const float* __restrict__ X = base + (long long)f * MOT_FRAME_FLOATS;     // wave-uniform: scalar loads
        float acc[MET_VPT][12];
#pragma unroll
        for (int q = 0; q < MET_VPT; ++q)
#pragma unroll
            for (int k = 0; k < 12; ++k) acc[q][k] = 0.0f;
#pragma unroll
        for (int j = 0; j < 24; ++j) {
            float xj[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) xj[k] = X[j * 12 + k];
#pragma unroll
            for (int q = 0; q < MET_VPT; ++q)
#pragma unroll
                for (int k = 0; k < 12; ++k) acc[q][k] = fmaf(r.w[q][j], xj[k], acc[q][k]);
            if (j % 4 == 3) __builtin_amdgcn_sched_barrier(0);    // at most four joints' transforms (48 SGPRs) are requested ahead
        }
#pragma unroll
        for (int q = 0; q < MET_VPT; ++q) {
            float d[3];
#pragma unroll
            for (int c = 0; c < 3; ++c)
                d[c] = fmaf(acc[q][4 * c + 2], r.x[q][2], fmaf(acc[q][4 * c + 1], r.x[q][1], acc[q][4 * c] * r.x[q][0])) + acc[q][4 * c + 3];
            const double x = (double)norm3(d);
            if (f == 0) K[q] = x;
            const double e = x - K[q];
            s1[q] += e;
            s2[q] += e * e;
        }
    }
#pragma unroll
    for (int q = 0; q < MET_VPT; ++q) {
        const int v = slab * MET_SLAB + q * 256 + tid;
        if (v < V) {
            Stat s;
            s.mean = K[q] + s1[q] / nf;
            s.m2 = s2[q] - s1[q] * s1[q] / nf;
            vpart[(long long)blk * V + v] = s;
        }
    }
}

// vslab[group][slab] = (sum over the slab's vertices of the column mean, sum of the column std): a vertex's blocks merged in index order,
// a thread's vertices added in index order, the 256 threads by a fixed tree
__global__ __launch_bounds__(256) void rc_motion_vfinish_kernel(const MotionGroup* __restrict__ tab, int V, int n_slab,
                                                                const Stat* __restrict__ vpart, double* __restrict__ vslab) {
    __shared__ double s_mean[256], s_std[256];
    const int tid = threadIdx.x, slab = blockIdx.y;
    const MotionGroup g = tab[blockIdx.x];
    double sum_mean = 0.0, sum_std = 0.0;
    for (int q = 0; q < MET_VPT; ++q) {
        const int v = slab * MET_SLAB + q * 256 + tid;
        if (v >= V) continue;
        double n = 0.0;
        Stat a = {0.0, 0.0};
        for (int b = 0; b < g.nblk; ++b) stat_merge(n, a, (double)block_rows(g.frames, b), vpart[(long long)(g.blk0 + b) * V + v]);
        sum_mean += a.mean;
        sum_std += unbiased_std(a.m2, n);
    }
    s_mean[tid] = sum_mean;
    s_std[tid] = sum_std;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) { s_mean[tid] += s_mean[tid + h]; s_std[tid] += s_std[tid + h]; }
        __syncthreads();
    }
    if (tid == 0) {
        vslab[((long long)blockIdx.x * n_slab + slab) * 2] = s_mean[0];
        vslab[((long long)blockIdx.x * n_slab + slab) * 2 + 1] = s_std[0];
    }
}

// out[group][11][2], per_joint[group][4][24] (or nullptr). vslab == nullptr: RC_MOTION_NO_MESH, row 1 is NaN.
__global__ __launch_bounds__(192) void rc_motion_finish_kernel(const MotionGroup* __restrict__ tab, int fps, unsigned mask, int V, int n_slab,
                                                               const Stat* __restrict__ part, const double* __restrict__ vslab,
                                                               float* __restrict__ out, float* __restrict__ per_joint) {
    __shared__ double c_mean[MOT_NCOL], c_std[MOT_NCOL];
    const int col = threadIdx.x;
    const long long grp = blockIdx.x;
    const MotionGroup g = tab[grp];
    if (col < MOT_NCOL) {
        const long long rows = col < 96 ? g.frames : (col < 144 ? g.frames - 3 : g.frames - fps);
        double n = 0.0;
        Stat a = {0.0, 0.0};
        for (int b = 0; b < g.nblk; ++b) stat_merge(n, a, (double)block_rows(rows, b), part[(long long)(g.blk0 + b) * MOT_NCOL + col]);
        const double nan = __builtin_nan("");
        c_mean[col] = n > 0.0 ? a.mean : nan;                     // the mean of an empty set
        c_std[col] = n > 0.0 ? unbiased_std(a.m2, n) : nan;
    }
    __syncthreads();
    float* __restrict__ o = out + grp * 22;
    if (col < 6 || col == 10) {                                   // je, -, lae, gae, jkp, jkt | tre: 24 columns each, in index order
        if (col == 1) {
            double m = __builtin_nan(""), s = __builtin_nan("");
            if (vslab) {
                m = 0.0; s = 0.0;
                for (int q = 0; q < n_slab; ++q) { m += vslab[(grp * n_slab + q) * 2]; s += vslab[(grp * n_slab + q) * 2 + 1]; }
                m /= V; s /= V;
            }
            o[2] = (float)m; o[3] = (float)s;
        } else {
            // first column of the row: je 0 | lae 24 | gae 48 | jkp 96 | jkt 120 | tre 72
            const int first = col == 0 ? 0 : (col == 2 ? 24 : (col == 3 ? 48 : (col == 4 ? 96 : (col == 5 ? 120 : 72))));
            double m = 0.0, s = 0.0;
            for (int j = 0; j < 24; ++j) { m += c_mean[first + j]; s += c_std[first + j]; }
            o[2 * col] = (float)(m / 24.0); o[2 * col + 1] = (float)(s / 24.0);
        }
    } else if (col == 6) {
        o[12] = (float)c_mean[144]; o[13] = (float)c_std[144];
    } else if (col >= 7 && col <= 9) {                            // evaluator.py:380-382; no mask: torch.zeros(1) -> (0, NaN)
        const int first = (col - 7) * 24;
        double m = 0.0, s = 0.0;
        int cnt = 0;
        for (int j = 0; j < 24; ++j)
            if (mask >> j & 1u) { m += c_mean[first + j]; s += c_std[first + j]; ++cnt; }
        o[2 * col] = cnt ? (float)(m / cnt) : 0.0f;
        o[2 * col + 1] = cnt ? (float)(s / cnt) : __builtin_nanf("");
    }
    if (per_joint && col < 96) per_joint[grp * 96 + col] = (float)c_mean[col];   // je | lae | gae | tre: the layout of the columns
}

long long rc_motion_scratch_floats(long long n) { return n * MOT_FRAME_FLOATS; }
long long rc_motion_partial_doubles(int V, long long blocks, int groups, bool mesh) {
    const long long n_slab = (V + MET_SLAB - 1) / MET_SLAB;
    return 2 * (blocks * MOT_NCOL + (mesh ? blocks * V + (long long)groups * n_slab : 0));
}
void rc_launch_motion_metrics(const BodyConst* body, const float* vt, const float* w, int V, const MotionGroup* tab, int groups,
                              long long blocks, const float* pose_p, const float* tran_p, const float* pose_t, const float* tran_t, long long n,
                              int fps, int align, unsigned mask, bool mesh, float* scratch, double* partial, float* out, float* per_joint,
                              hipStream_t st) {
    const int n_slab = (V + MET_SLAB - 1) / MET_SLAB;
    Stat* part = reinterpret_cast<Stat*>(partial);
    Stat* vpart = part + blocks * MOT_NCOL;
    double* vslab = mesh ? reinterpret_cast<double*>(vpart + blocks * V) : nullptr;
    hipLaunchKernelGGL(rc_motion_frame_kernel, dim3((unsigned)n), dim3(64), 0, st, body, pose_p, tran_p, pose_t, tran_t, align, scratch);
    hipLaunchKernelGGL(rc_motion_col_kernel, dim3((unsigned)blocks), dim3(192), 0, st, tab, groups, fps, scratch, part);
    if (mesh) {
        hipLaunchKernelGGL(rc_motion_sweep_kernel, dim3((unsigned)blocks, (unsigned)n_slab), dim3(256), 0, st, body, vt, w, V, tab, groups,
                           scratch, vpart);
        hipLaunchKernelGGL(rc_motion_vfinish_kernel, dim3((unsigned)groups, (unsigned)n_slab), dim3(256), 0, st, tab, V, n_slab, vpart, vslab);
    }
    hipLaunchKernelGGL(rc_motion_finish_kernel, dim3((unsigned)groups), dim3(192), 0, st, tab, fps, mask, V, n_slab, part, vslab, out, per_joint);
}
