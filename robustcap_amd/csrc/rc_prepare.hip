// The motion half of the reference's dataset preparation for a ragged batch of sequences, gfx950 (rc_prepare_motions in rc_prepare_api.cpp).
//
// Reference: preprocess.py:252-306 (AMASS) and :207-237 (AIST++): a host loop per sequence -- [::step] decimation, joint 23 <- 37 of the
// 52-joint layout, the root re-alignment R -> axis-angle frame by frame, a body shaped by the sequence's betas, forward_kinematics with
// calc_mesh=True (6,890 vertices skinned to keep 39) and _syn_acc. Here:
//   rc_prep_rest_kernel    one workgroup per sequence: rest joints J = Jt + JS beta and the 39 picked vertices vt39 + S39 beta from the
//                          folded basis of rc_set_shape_space (in double, rounded once), root-relative with rc_set_body's expressions; or
//                          ONE record from the context's body and mesh when there are no betas. A record is 1,044 B.
//   rc_prep_frame_kernel   one wave per OUTPUT frame: finds its sequence by bisection in the offset table, reads its input frame, aligns the
//                          root, chains the joints (the arithmetic of wave_body_fk) and skins the 33 landmark and 6 IMU vertices (the
//                          arithmetic of rc_imu_frame_kernel and of the full-mesh sweep).
//   rc_prep_acc_kernel     _syn_acc of the six IMU vertices, one lane per element, the stencil confined to its sequence (rc_syn_acc_kernel's
//                          expressions).
// No atomics; every output element has one writer: the same call gives the same bits, and a sequence's rows do not depend on its neighbours.
// HBM per output frame: 288 (or 624) + 12 B in, 288 + 12 + 216 + 288 + 396 + 72 (+ 72) B out.
//
// Camera-frame motions (rc_prepare_camera_motions; preprocess.py:460-470, 477-483 and :571-582, 589-599 for 3DPW / 3DPW-OCC, :359-360 for
// TotalCapture) reuse the rest and the stencil kernels and add, further down:
//   rc_cam_frame_kernel    one wave per OUTPUT frame: a T_cw row per frame (row t / cam_repeat of its sequence), root <- R_cw R_0,
//                          tran <- R_cw tran + t_cw, the pose stored as ROTATION MATRICES (no R -> axis-angle), then the same chain and skins.
//   rc_cam_kp_kernel       30 Hz detections to 60 Hz by midpoint interleaving, one lane per element.
#include "rc_device.h"

namespace {

__device__ __forceinline__ int find_seq(const PrepSeq* __restrict__ tab, int n, long long f) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].out0 <= f) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// rc_axis_angle_to_rotmat's arithmetic operation for operation AS rc_aa2R_kernel (rc_frame.hip) IS COMPILED, so that a matrix formed here
// has that entry's bits (tests/test_gpu_motion_prepare.py: without betas and alignment the pass is bitwise the existing chain). Left to
// the compiler, the source expression of rc_aa2R_kernel contracts differently inside this kernel (about one entry in nine differs in the
// last bit). The forms: |a|^2 = fma(a1, a1, a0 a0) + a2 a2; diagonal fma(t, k_i k_i, c); off-diagonal fma(+-sn, k, t (k_i k_j)), except
// R21 = sn k0 + t (k1 k2) with both products rounded.
__device__ __forceinline__ void aa_to_R_entry(const float* aa, float* R) {
#pragma clang fp contract(off)
    const float a0 = aa[0], a1 = aa[1], a2 = aa[2];
    const float th = sqrtf(__builtin_fmaf(a1, a1, a0 * a0) + a2 * a2);
    float k[3] = {a0 / th, a1 / th, a2 / th};
#pragma unroll
    for (int q = 0; q < 3; ++q) if (!(fabsf(k[q]) <= 3.0e38f)) k[q] = 0.0f;          // NaN / inf -> 0
    const float c = cosf(th), sn = sinf(th), t = 1.0f - c;
    const float p01 = t * (k[0] * k[1]), p02 = t * (k[0] * k[2]), p12 = t * (k[1] * k[2]);
    R[0] = __builtin_fmaf(t, k[0] * k[0], c);
    R[1] = __builtin_fmaf(-k[2], sn, p01);
    R[2] = __builtin_fmaf(sn, k[1], p02);
    R[3] = __builtin_fmaf(sn, k[2], p01);
    R[4] = __builtin_fmaf(t, k[1] * k[1], c);
    R[5] = __builtin_fmaf(-k[0], sn, p12);
    R[6] = __builtin_fmaf(-k[1], sn, p02);
    R[7] = sn * k[0] + p12;
    R[8] = __builtin_fmaf(t, k[2] * k[2], c);
}

// root-relative record from the rest joints J [24][3] (LDS) -- rc_set_body's expressions (model.py:87-92, spatial.py:148-167)
__device__ __forceinline__ void rest_from_joints(const BodyConst* __restrict__ body, const float (*J)[3], PrepRest* rec, int tid) {
    if (tid < 72) {
        const int i = tid / 3, c = tid % 3, p = body->parent[i];
        const float jr = J[i][c] - J[0][c];
        rec->jrest[i][c] = jr;
        rec->bone[i][c] = i == 0 ? jr : jr - (J[p][c] - J[0][c]);
    }
}

}  // namespace

// betas == nullptr: grid 1, the context's body and mesh. Otherwise grid n_seq.
__global__ __launch_bounds__(128) void rc_prep_rest_kernel(const BodyConst* __restrict__ body, const float* __restrict__ mesh_vt,
                                                           PrepShapeSpace sp, const float* __restrict__ betas, PrepRest* __restrict__ rest,
                                                           float* __restrict__ rest_joint_out, int n_out) {
    __shared__ float J[24][3];
    __shared__ float beta[10];
    const int tid = threadIdx.x, i = blockIdx.x;
    if (!betas) {
        if (tid < 72) {
            rest->jrest[tid / 3][tid % 3] = body->jrest[tid / 3][tid % 3];
            rest->bone[tid / 3][tid % 3] = body->bone[tid / 3][tid % 3];
        }
        if (tid < 117) rest->v39[tid / 3][tid % 3] = mesh_vt[3 * sp.vid[tid / 3] + tid % 3] - body->jroot[tid % 3];
        if (rest_joint_out)
            for (int e = tid; e < n_out * 72; e += 128) rest_joint_out[e] = body->jrest[(e % 72) / 3][e % 3] + body->jroot[e % 3];
        return;
    }
    if (tid < 10) beta[tid] = betas[(long long)i * 10 + tid];
    __syncthreads();
    if (tid < 72) {
        double acc = (double)sp.Jt[tid];
#pragma unroll
        for (int b = 0; b < 10; ++b) acc += (double)sp.JS[tid * 10 + b] * (double)beta[b];
        J[tid / 3][tid % 3] = (float)acc;
        if (rest_joint_out) rest_joint_out[(long long)i * 72 + tid] = (float)acc;
    }
    __syncthreads();
    rest_from_joints(body, J, rest + i, tid);
    if (tid < 117) {
        double acc = (double)sp.vt39[tid];
#pragma unroll
        for (int b = 0; b < 10; ++b) acc += (double)sp.S39[tid * 10 + b] * (double)beta[b];
        rest[i].v39[tid / 3][tid % 3] = (float)acc - J[0][tid % 3];
    }
}

struct PrepPick { int jid[6]; float W[9]; int aligned; };

__global__ __launch_bounds__(64) void rc_prep_frame_kernel(const BodyConst* __restrict__ body, const PrepSeq* __restrict__ tab, int n_seq,
                                                           const PrepRest* __restrict__ rest, int per_seq_rest, const float* __restrict__ w39,
                                                           PrepPick pick, const float* __restrict__ pose_aa, int pose_joints,
                                                           const float* __restrict__ tran, float* __restrict__ pose_out,
                                                           float* __restrict__ tran_out, float* __restrict__ ori, float* __restrict__ joint,
                                                           float* __restrict__ sync, float* __restrict__ vert6) {
    __shared__ WaveScratch s;
    __shared__ PrepRest r;
    __shared__ float aa[24][3];
    const long long f = blockIdx.x;
    const int lane = threadIdx.x;
    const int q = find_seq(tab, n_seq, f);
    const PrepSeq sq = tab[q];
    const long long fin = sq.in0 + (long long)sq.step * (f - sq.out0);
    {
        const float* src = reinterpret_cast<const float*>(rest + (per_seq_rest ? q : 0));
        float* dst = reinterpret_cast<float*>(&r);
        for (int e = lane; e < (int)(sizeof(PrepRest) / sizeof(float)); e += 64) dst[e] = src[e];
    }
    const float* pin = pose_aa + fin * pose_joints * 3;
    for (int e = lane; e < 72; e += 64) {
        const int j = e / 3;
        aa[j][e % 3] = pin[(j == 23 && pose_joints == 52 ? 37 : j) * 3 + e % 3];       // preprocess.py:278-279
    }
    const float tin[3] = {tran[fin * 3], tran[fin * 3 + 1], tran[fin * 3 + 2]};
    float t[3] = {tin[0], tin[1], tin[2]};
    if (pick.aligned) mat3_vec(pick.W, tin, t);                                        // :283
    __syncthreads();
    if (pick.aligned && lane == 0) {                                                   // :284-285
        float R0[9], M[9], a0[3];
        aa_to_R_entry(aa[0], R0);
        mat3_mul(pick.W, R0, M);
        rotmat_to_aa(M, a0);
        aa[0][0] = a0[0]; aa[0][1] = a0[1]; aa[0][2] = a0[2];
    }
    __syncthreads();
    for (int e = lane; e < 72; e += 64) pose_out[f * 72 + e] = aa[e / 3][e % 3];
    if (lane < 3) tran_out[f * 3 + lane] = t[lane];
    if (lane < 24) {                                                                   // :292 on the stored pose
        float R[9];
        aa_to_R_entry(aa[lane], R);
#pragma unroll
        for (int k = 0; k < 9; ++k) s.Rl[lane][k] = R[k];
    }
    __syncthreads();
    // the joint chain of wave_body_fk on this sequence's bones
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) s.G[0][k] = s.Rl[0][k];
        s.P[0][0] = s.P[0][1] = s.P[0][2] = 0.0f;
    }
    __syncthreads();
    const int lvl = lane < 24 ? body->level[lane] : -1;
    for (int l = 1; l < 10; ++l) {
        if (lvl == l) {
            const int p = body->parent[lane];
            float g[9], pb[3];
            mat3_mul(s.G[p], s.Rl[lane], g);
            mat3_vec(s.G[p], r.bone[lane], pb);
#pragma unroll
            for (int k = 0; k < 9; ++k) s.G[lane][k] = g[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) s.P[lane][k] = pb[k] + s.P[p][k];
        }
        __syncthreads();
    }
    if (lane < 24) {
        float gj[3];
        mat3_vec(s.G[lane], r.jrest[lane], gj);
#pragma unroll
        for (int k = 0; k < 3; ++k) s.T[lane][k] = s.P[lane][k] - gj[k];
    }
    __syncthreads();
    if (lane < 54) ori[f * 54 + lane] = s.G[pick.jid[lane / 9]][lane % 9];
    if (lane < 24) {
#pragma unroll
        for (int c = 0; c < 3; ++c) joint[(f * 24 + lane) * 3 + c] = s.P[lane][c] + t[c];
    }
    if (lane < 39) {                                                                   // the skin of rc_imu_frame_kernel / the full-mesh sweep
        float A[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) A[k] = 0.0f;
        const float* wv = w39 + lane * 24;
        for (int j = 0; j < 24; ++j) {
            const float wj = wv[j];
#pragma unroll
            for (int rr = 0; rr < 3; ++rr) {
                A[4 * rr + 0] += wj * s.G[j][3 * rr + 0];
                A[4 * rr + 1] += wj * s.G[j][3 * rr + 1];
                A[4 * rr + 2] += wj * s.G[j][3 * rr + 2];
                A[4 * rr + 3] += wj * s.T[j][rr];
            }
        }
        const float x = r.v39[lane][0], y = r.v39[lane][1], z = r.v39[lane][2];
        float* o = lane < 33 ? sync + (f * 33 + lane) * 3 : vert6 + (f * 6 + (lane - 33)) * 3;
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) o[rr] = (((A[4 * rr] * x + A[4 * rr + 1] * y) + A[4 * rr + 2] * z) + A[4 * rr + 3]) + t[rr];
    }
}

// _syn_acc (preprocess.py:22-33) of v [frames, 18] per sequence: rc_syn_acc_kernel's expressions with T and t of the element's own sequence
__global__ void rc_prep_acc_kernel(const PrepSeq* __restrict__ tab, int n_seq, const float* __restrict__ v, float* __restrict__ acc,
                                   long long frames, int n) {
#pragma clang fp contract(off)
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= frames * 18) return;
    const long long f = idx / 18;
    const PrepSeq sq = tab[find_seq(tab, n_seq, f)];
    const long long t = f - sq.out0, T = sq.out_n;
    const long long width = 18;
    float out = 0.0f;
    if (n / 2 != 0 && t >= n && t < T - n)
        out = (((v[idx - n * width] + v[idx + n * width]) - 2.0f * v[idx]) * 3600.0f) / (float)(n * n);
    else if (t >= 1 && t < T - 1)
        out = ((v[idx - width] + v[idx + width]) - 2.0f * v[idx]) * 3600.0f;
    acc[idx] = out;
}

// ---- camera-frame motions (rc_prepare_camera_motions): preprocess.py:460-470 / :571-582 (3DPW, a T_cw per frame) and :359-360 (TotalCapture)
// One wave per OUTPUT frame t of its sequence: local rotations by aa_to_R_entry, root <- R_cw R_0, tran <- R_cw tran + t_cw with the camera row
// cam0 + t / cam_repeat (cam_repeat 0: the sequence's one row), then rc_prep_frame_kernel's chain and skins on them -- its text, copied: that
// kernel's bits are pinned (its comment above), so the two share nothing but the __forceinline__ pieces. The pose is stored as rotation
// matrices, so there is no R -> axis-angle here and none of its float64 registers.
// HBM per output frame: 288 + 12 + 48 B in, 864 + 12 + 216 + 288 (+ 396) + 72 B out.
struct CamScratch { float Rl[24][9], G[24][9], P[24][3], T[24][3]; };
struct CamPick { int jid[6]; int repeat, root_only; };

__device__ __forceinline__ void cam_root(const float* C, const float* R0, float* M) {          // R_cw R_0, every product and sum rounded
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) M[3 * r + c] = (C[4 * r] * R0[c] + C[4 * r + 1] * R0[3 + c]) + C[4 * r + 2] * R0[6 + c];
}
__device__ __forceinline__ void cam_point(const float* C, const float* x, float* y) {          // R_cw x + t_cw, likewise
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < 3; ++r) y[r] = ((C[4 * r] * x[0] + C[4 * r + 1] * x[1]) + C[4 * r + 2] * x[2]) + C[4 * r + 3];
}

// The last step of a skin, (((A0 x + A1 y) + A2 z) + A3) + t per row, operation for operation AS rc_prep_frame_kernel IS COMPILED (and with it
// rc_imu_frame_kernel and the full-mesh sweep, to which tests/test_gpu_motion_prepare.py pins it): of the two products under the first
// sum the compiler rounds A0 x in row 0 and A1 y in rows 1 and 2 and fuses the other one. Left to the compiler, this kernel's row 2 came
// out the other way round, and the landmarks under an identity camera were no longer prepare_motions' bit for bit.
__device__ __forceinline__ void skin_point_entry(const float* A, float x, float y, float z, const float* t, float* o) {
#pragma clang fp contract(off)
    o[0] = (__builtin_fmaf(z, A[2], __builtin_fmaf(y, A[1], x * A[0])) + A[3]) + t[0];
    o[1] = (__builtin_fmaf(z, A[6], __builtin_fmaf(x, A[4], y * A[5])) + A[7]) + t[1];
    o[2] = (__builtin_fmaf(z, A[10], __builtin_fmaf(x, A[8], y * A[9])) + A[11]) + t[2];
}

__global__ __launch_bounds__(64) void rc_cam_frame_kernel(const BodyConst* __restrict__ body, const PrepSeq* __restrict__ tab,
                                                          const PrepCam* __restrict__ cam, int n_seq, const PrepRest* __restrict__ rest,
                                                          int per_seq_rest, const float* __restrict__ w39, CamPick pick,
                                                          const float* __restrict__ pose_aa, const float* __restrict__ tran,
                                                          const PrepCamRow* __restrict__ cam_rows, float* __restrict__ pose_out,
                                                          float* __restrict__ tran_out, float* __restrict__ ori, float* __restrict__ joint,
                                                          float* __restrict__ sync, float* __restrict__ vert6) {
    __shared__ CamScratch s;
    __shared__ PrepRest r;
    __shared__ float aa[24][3];
    const long long f = blockIdx.x;
    const int lane = threadIdx.x;
    const int q = find_seq(tab, n_seq, f);
    const PrepSeq sq = tab[q];
    const long long tq = f - sq.out0, fin = sq.in0 + tq;
    const PrepCamRow C = cam_rows[cam[q].cam0 + (pick.repeat ? tq / pick.repeat : 0)];
    {
        const float* src = reinterpret_cast<const float*>(rest + (per_seq_rest ? q : 0));
        float* dst = reinterpret_cast<float*>(&r);
        for (int e = lane; e < (int)(sizeof(PrepRest) / sizeof(float)); e += 64) dst[e] = src[e];
    }
    const float* pin = pose_aa + fin * 72;
    for (int e = lane; e < 72; e += 64) aa[e / 3][e % 3] = pin[e];
    const float tin[3] = {tran[fin * 3], tran[fin * 3 + 1], tran[fin * 3 + 2]};
    float t[3] = {tin[0], tin[1], tin[2]};
    if (!pick.root_only) cam_point(C.m, tin, t);                                       // :467; TotalCapture keeps Vicon's translation
    __syncthreads();
    if (lane < 3) tran_out[f * 3 + lane] = t[lane];
    if (lane < 24) {                                                                   // :465-466
        float R[9];
        aa_to_R_entry(aa[lane], R);
        if (lane == 0) {
            float M[9];
            cam_root(C.m, R, M);
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = M[k];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) s.Rl[lane][k] = R[k];
    }
    __syncthreads();
    for (int e = lane; e < 216; e += 64) pose_out[f * 216 + e] = (&s.Rl[0][0])[e];
    // the joint chain of wave_body_fk on this sequence's bones (rc_prep_frame_kernel's text)
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) s.G[0][k] = s.Rl[0][k];
        s.P[0][0] = s.P[0][1] = s.P[0][2] = 0.0f;
    }
    __syncthreads();
    const int lvl = lane < 24 ? body->level[lane] : -1;
    for (int l = 1; l < 10; ++l) {
        if (lvl == l) {
            const int p = body->parent[lane];
            float g[9], pb[3];
            mat3_mul(s.G[p], s.Rl[lane], g);
            mat3_vec(s.G[p], r.bone[lane], pb);
#pragma unroll
            for (int k = 0; k < 9; ++k) s.G[lane][k] = g[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) s.P[lane][k] = pb[k] + s.P[p][k];
        }
        __syncthreads();
    }
    if (lane < 24) {
        float gj[3];
        mat3_vec(s.G[lane], r.jrest[lane], gj);
#pragma unroll
        for (int k = 0; k < 3; ++k) s.T[lane][k] = s.P[lane][k] - gj[k];
    }
    __syncthreads();
    if (lane < 54) ori[f * 54 + lane] = s.G[pick.jid[lane / 9]][lane % 9];
    if (lane < 24) {
#pragma unroll
        for (int c = 0; c < 3; ++c) joint[(f * 24 + lane) * 3 + c] = s.P[lane][c] + t[c];
    }
    if (lane < 39 && (lane >= 33 || sync)) {                                           // the skin of rc_imu_frame_kernel / the full-mesh sweep
        float A[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) A[k] = 0.0f;
        const float* wv = w39 + lane * 24;
#pragma unroll 4                                                                       // (unrolled whole, the 24 x 12 LDS reads in flight take 256 VGPRs + 100 AGPRs)
        for (int j = 0; j < 24; ++j) {
            const float wj = wv[j];
#pragma unroll
            for (int rr = 0; rr < 3; ++rr) {
                A[4 * rr + 0] = __builtin_fmaf(wj, s.G[j][3 * rr + 0], A[4 * rr + 0]);
                A[4 * rr + 1] = __builtin_fmaf(wj, s.G[j][3 * rr + 1], A[4 * rr + 1]);
                A[4 * rr + 2] = __builtin_fmaf(wj, s.G[j][3 * rr + 2], A[4 * rr + 2]);
                A[4 * rr + 3] = __builtin_fmaf(wj, s.T[j][rr], A[4 * rr + 3]);
            }
        }
        const float x = r.v39[lane][0], y = r.v39[lane][1], z = r.v39[lane][2];
        float* o = lane < 33 ? sync + (f * 33 + lane) * 3 : vert6 + (f * 6 + (lane - 33)) * 3;
        skin_point_entry(A, x, y, z, t, o);
    }
}

// 30 Hz detections to 60 Hz (preprocess.py:477-483 with [:len(posec)]): output frame t even <- kp[t / 2]; odd <- (kp[t / 2 + 1] + kp[t / 2]) / 2,
// or kp[t / 2] again behind the last detection. One lane per element; a sum and a halving, each exact or rounded once: numpy's bits.
__global__ void rc_cam_kp_kernel(const PrepSeq* __restrict__ tab, const PrepCam* __restrict__ cam, int n_seq, const float* __restrict__ kp_in,
                                 float* __restrict__ kp_out, long long frames) {
#pragma clang fp contract(off)
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= frames * 99) return;
    const long long f = idx / 99;
    const int e = (int)(idx % 99);
    const int q = find_seq(tab, n_seq, f);
    const long long t = f - tab[q].out0, h = t / 2;
    const float* a = kp_in + (cam[q].kp0 + h) * 99 + e;
    kp_out[idx] = (t % 2 == 0 || h + 1 >= cam[q].kp_n) ? a[0] : (a[99] + a[0]) / 2.0f;
}

void rc_launch_prepare_camera_motions(const BodyConst* body, const float* mesh_vt, const PrepShapeSpace& sp, const PrepSeq* tab,
                                      const PrepCam* cam, int n_seq, long long frames, int cam_repeat, bool root_only, const float* pose_aa,
                                      const float* tran, const float* betas, const PrepCamRow* cam_rows, const float* kp_in, const int* jid,
                                      int smooth_n, PrepRest* rest, float* pose_out, float* tran_out, float* ori, float* acc, float* joint,
                                      float* sync, float* vert6, float* kp_out, float* rest_joint_out, hipStream_t st) {
    if (frames <= 0 || n_seq <= 0) return;
    hipLaunchKernelGGL(rc_prep_rest_kernel, dim3(betas ? (unsigned)n_seq : 1u), dim3(128), 0, st, body, mesh_vt, sp, betas, rest, rest_joint_out,
                       n_seq);
    CamPick pick;
    for (int i = 0; i < 6; ++i) pick.jid[i] = jid[i];
    pick.repeat = cam_repeat;
    pick.root_only = root_only ? 1 : 0;
    hipLaunchKernelGGL(rc_cam_frame_kernel, dim3((unsigned)frames), dim3(64), 0, st, body, tab, cam, n_seq, rest, betas ? 1 : 0, sp.w39, pick,
                       pose_aa, tran, cam_rows, pose_out, tran_out, ori, joint, sync, vert6);
    hipLaunchKernelGGL(rc_prep_acc_kernel, dim3((unsigned)((frames * 18 + 255) / 256)), dim3(256), 0, st, tab, n_seq, vert6, acc, frames, smooth_n);
    if (kp_in)
        hipLaunchKernelGGL(rc_cam_kp_kernel, dim3((unsigned)((frames * 99 + 255) / 256)), dim3(256), 0, st, tab, cam, n_seq, kp_in, kp_out, frames);
}

void rc_launch_prepare_motions(const BodyConst* body, const float* mesh_vt, const PrepShapeSpace& sp, const PrepSeq* tab, int n_seq,
                               long long frames, const float* pose_aa, int pose_joints, const float* tran, const float* betas,
                               const float* world_rot, const int* jid, int smooth_n, PrepRest* rest, float* pose_out, float* tran_out,
                               float* ori, float* acc, float* joint, float* sync, float* vert6, float* rest_joint_out, hipStream_t st) {
    if (frames <= 0 || n_seq <= 0) return;
    hipLaunchKernelGGL(rc_prep_rest_kernel, dim3(betas ? (unsigned)n_seq : 1u), dim3(128), 0, st, body, mesh_vt, sp, betas, rest, rest_joint_out,
                       n_seq);
    PrepPick pick;
    for (int i = 0; i < 6; ++i) pick.jid[i] = jid[i];
    for (int k = 0; k < 9; ++k) pick.W[k] = world_rot ? world_rot[k] : (k % 4 == 0 ? 1.0f : 0.0f);
    pick.aligned = world_rot ? 1 : 0;
    hipLaunchKernelGGL(rc_prep_frame_kernel, dim3((unsigned)frames), dim3(64), 0, st, body, tab, n_seq, rest, betas ? 1 : 0, sp.w39, pick, pose_aa,
                       pose_joints, tran, pose_out, tran_out, ori, joint, sync, vert6);
    hipLaunchKernelGGL(rc_prep_acc_kernel, dim3((unsigned)((frames * 18 + 255) / 256)), dim3(256), 0, st, tab, n_seq, vert6, acc, frames, smooth_n);
}
