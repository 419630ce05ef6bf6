// rc_set_shape_space and rc_prepare_motions: the motion half of preprocess.py:207-237, 252-306 for all sequences in one stream-ordered call
// (kernels: rc_prepare.hip). The host forms one table entry per sequence and nothing per frame.
#include "rc_ctx.h"
#include "rc_shape_fold.h"

#include <algorithm>
#include <cmath>

// Folds the joint regressor with the template and the blend directions (each output summed over V in double, in index order, rounded once)
// and keeps the rows of the 39 picked vertices, so that a sequence's shape costs 24*3*10 + 39*3*10 multiply-adds.
int rc_set_shape_space(rc_ctx* ctx, const float* v_template, const float* shapedirs, const float* J_regressor, int32_t V,
                       const int32_t* landmark_ids, const int32_t* imu_vertex_ids) {
    if (!ctx) return RC_ERR_INVALID;
    const std::string f = "rc_set_shape_space: ";
    if (!landmark_ids || !imu_vertex_ids) return fail(ctx, RC_ERR_INVALID, f + "null vertex ids");
    const bool basis = v_template || shapedirs || J_regressor;
    if (basis && (!v_template || !shapedirs || !J_regressor)) return fail(ctx, RC_ERR_INVALID, f + "v_template, shapedirs and J_regressor come together");
    if (ctx->mesh_V == 0) return fail(ctx, RC_ERR_STATE, f + "rc_set_mesh first (the skinning weights)");
    if (V != ctx->mesh_V) return fail(ctx, RC_ERR_INVALID, f + "V differs from rc_set_mesh's");
    int vid[39];
    for (int i = 0; i < 39; ++i) {
        vid[i] = i < 33 ? landmark_ids[i] : imu_vertex_ids[i - 33];
        if (vid[i] < 0 || vid[i] >= V) return fail(ctx, RC_ERR_INVALID, f + "vertex id out of range");
    }
    // layout of the one allocation: Jt 72 | JS 720 | vt39 117 | S39 1170 | w39 936
    std::vector<float> h(72 + 720 + 117 + 1170 + 936, 0.0f);
    float *Jt = h.data(), *JS = Jt + 72, *vt39 = JS + 720, *S39 = vt39 + 117, *w39 = S39 + 1170;
    if (basis) {
        rc_fold_shape_basis(v_template, shapedirs, J_regressor, V, Jt, JS);
        for (int i = 0; i < 39; ++i)
            for (int c = 0; c < 3; ++c) {
                vt39[3 * i + c] = v_template[3 * (size_t)vid[i] + c];
                for (int b = 0; b < 10; ++b) S39[(3 * i + c) * 10 + b] = shapedirs[(3 * (size_t)vid[i] + c) * 10 + b];
            }
    }
    for (int i = 0; i < 39; ++i)
        for (int j = 0; j < 24; ++j) w39[24 * i + j] = ctx->mesh_w_h[(size_t)vid[i] * 24 + j];
    HIP_TRY(ctx, hipDeviceSynchronize());                                      // nothing in flight may still read the old space
    if (!ctx->prep_space) HIP_TRY(ctx, rc_alloc(ctx->prep_space, h.size()));
    HIP_TRY(ctx, hipMemcpy(ctx->prep_space.get(), h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    const float* d = ctx->prep_space.get();
    PrepShapeSpace& sp = ctx->prep_sp;
    sp.Jt = basis ? d : nullptr;
    sp.JS = basis ? d + 72 : nullptr;
    sp.vt39 = basis ? d + 792 : nullptr;
    sp.S39 = basis ? d + 909 : nullptr;
    sp.w39 = d + 2079;
    for (int i = 0; i < 39; ++i) sp.vid[i] = vid[i];
    ctx->prep_V = V;
    ctx->prep_basis = basis;
    return RC_OK;
}

int rc_prepare_motions(rc_ctx* ctx, int32_t n_seq, const int64_t* in_frames_host, const int32_t* step_host, int64_t in_total,
                       const float* pose_aa, int32_t pose_joints, const float* tran, const float* betas, const float* world_rot_host,
                       const int32_t* imu_joint_ids_host, int32_t smooth_n, float* pose_out, float* tran_out, float* imu_ori, float* imu_acc,
                       float* joint3d, float* sync_3d_mp, float* vert6_out, float* rest_joint_out, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    const std::string f = "rc_prepare_motions: ";
    if (!in_frames_host || !pose_aa || !tran || !imu_joint_ids_host || !pose_out || !tran_out || !imu_ori || !imu_acc || !joint3d || !sync_3d_mp)
        return fail(ctx, RC_ERR_INVALID, f + "null argument");
    if (n_seq < 1) return fail(ctx, RC_ERR_INVALID, f + "n_seq must be positive");
    if (pose_joints != 24 && pose_joints != 52) return fail(ctx, RC_ERR_INVALID, f + "pose_joints must be 24 or 52");
    if (smooth_n < 0) return fail(ctx, RC_ERR_INVALID, f + "smooth_n must not be negative");
    if (in_total < 0) return fail(ctx, RC_ERR_INVALID, f + "in_total must not be negative");
    for (int i = 0; i < 6; ++i)
        if (imu_joint_ids_host[i] < 0 || imu_joint_ids_host[i] > 23) return fail(ctx, RC_ERR_INVALID, f + "IMU joint id outside 0 .. 23");
    if (world_rot_host)
        for (int k = 0; k < 9; ++k)
            if (!std::isfinite(world_rot_host[k])) return fail(ctx, RC_ERR_INVALID, f + "world_rot is not finite");
    long long in_sum = 0, frames = 0;
    for (int i = 0; i < n_seq; ++i) {
        const int step = step_host ? step_host[i] : 1;
        const long long in = in_frames_host[i];
        if (step != 1 && step != 2) return fail(ctx, RC_ERR_INVALID, f + "sequence " + std::to_string(i) + ": step must be 1 or 2");
        if (in < 1 || in > in_total) return fail(ctx, RC_ERR_INVALID, f + "sequence " + std::to_string(i) + " gives no frame (or more than in_total)");
        const long long out = (in + step - 1) / step;
        if (smooth_n / 2 != 0 && out < 2 * (long long)smooth_n + 1)
            return fail(ctx, RC_ERR_INVALID, f + "sequence " + std::to_string(i) + " gives " + std::to_string(out) + " frames: 2 * smooth_n + 1 needed");
        in_sum += in;
        frames += out;
    }
    if (in_sum != in_total) return fail(ctx, RC_ERR_INVALID, f + "the sequences hold " + std::to_string(in_sum) + " frames, in_total is " + std::to_string(in_total));
    if (frames >= (1ll << 31)) return fail(ctx, RC_ERR_INVALID, f + "2^31 output frames or more");
    if (!ctx->have_body) return fail(ctx, RC_ERR_STATE, f + "rc_set_body first");
    if (ctx->prep_V == 0) return fail(ctx, RC_ERR_STATE, f + "rc_set_shape_space first (the picked vertices)");
    if (ctx->prep_V != ctx->mesh_V) return fail(ctx, RC_ERR_STATE, f + "rc_set_mesh changed the vertex count since rc_set_shape_space");
    if (betas && !ctx->prep_basis) return fail(ctx, RC_ERR_STATE, f + "betas need the shape basis (rc_set_shape_space with shapedirs and J_regressor)");
    hipStream_t st = (hipStream_t)stream;
    // ---- the sequence table: pinned slot -> device, on `stream`
    const size_t G = (size_t)n_seq;
    PrepSeq* th = nullptr;
    HIP_TRY(ctx, ctx->prep_tab.stage(G, &th));
    long long in0 = 0, out0 = 0;
    for (int i = 0; i < n_seq; ++i) {
        const int step = step_host ? step_host[i] : 1;
        th[i].in0 = in0;
        th[i].out0 = out0;
        th[i].step = step;
        th[i].out_n = (int)((in_frames_host[i] + step - 1) / step);
        in0 += in_frames_host[i];
        out0 += th[i].out_n;
    }
    const size_t need_r = betas ? G : 1, need_v = vert6_out ? 0 : (size_t)frames * 18;
    if (!ctx->prep_tab.holds(G) || need_r > ctx->prep_rest_n || need_v > ctx->prep_vert6_n) {   // (kernels of earlier calls may still use the old buffers)
        HIP_TRY(ctx, hipDeviceSynchronize());                                  // (a call on another stream may still read them)
        HIP_TRY(ctx, ctx->prep_tab.grow(G));
        HIP_TRY(ctx, rc_grow(ctx->prep_rest_n, need_r, 2 * need_r, ctx->prep_rest, 2 * need_r));
        HIP_TRY(ctx, rc_grow(ctx->prep_vert6_n, need_v, need_v, ctx->prep_vert6, need_v));
    }
    HIP_TRY(ctx, ctx->prep_tab.upload(G, st));
    HIP_TRY(ctx, ctx->prep_tab.record(st));
    rc_launch_prepare_motions(ctx->body, ctx->mesh_vt, ctx->prep_sp, ctx->prep_tab.get(), n_seq, frames, pose_aa, pose_joints, tran, betas,
                              world_rot_host, imu_joint_ids_host, smooth_n, ctx->prep_rest.get(), pose_out, tran_out, imu_ori, imu_acc, joint3d,
                              sync_3d_mp, vert6_out ? vert6_out : ctx->prep_vert6.get(), rest_joint_out, st);
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}

// The camera-frame counterpart (preprocess.py:460-483, :571-599 for 3DPW; :359-360 for TotalCapture's static flip): one PrepSeq (step 1) and
// one PrepCam per sequence, and the camera rows -- HOST, so that a non-finite one is refused before anything is enqueued -- through their
// own rings. Rest records, vertex scratch and prep_tab are rc_prepare_motions': calls of one context are ordered by the caller.
int rc_prepare_camera_motions(rc_ctx* ctx, int32_t n_seq, const int64_t* in_frames_host, const int64_t* cam_frames_host, int32_t cam_repeat,
                              int64_t in_total, int64_t cam_total, const float* pose_aa, const float* tran, const float* betas,
                              const float* cam_T_host, const float* kp_in, const int64_t* kp_frames_host, int64_t kp_total,
                              const int32_t* imu_joint_ids_host, int32_t smooth_n, uint32_t flags, float* pose_out, float* tran_out,
                              float* imu_ori, float* imu_acc, float* joint3d, float* sync_3d_mp, float* vert6_out, float* kp_out,
                              float* rest_joint_out, void* stream) {
    if (!ctx) return RC_ERR_INVALID;
    const std::string f = "rc_prepare_camera_motions: ";
    if (!in_frames_host || !cam_frames_host || !pose_aa || !tran || !cam_T_host || !imu_joint_ids_host || !pose_out || !tran_out || !imu_ori ||
        !imu_acc || !joint3d)
        return fail(ctx, RC_ERR_INVALID, f + "null argument");
    if ((kp_in != nullptr) != (kp_out != nullptr) || (kp_in && !kp_frames_host))
        return fail(ctx, RC_ERR_INVALID, f + "kp_in, kp_frames_host and kp_out come together");
    if (n_seq < 1) return fail(ctx, RC_ERR_INVALID, f + "n_seq must be positive");
    if (cam_repeat < 0) return fail(ctx, RC_ERR_INVALID, f + "cam_repeat must not be negative");
    if (flags & ~(uint32_t)RC_CAM_ROOT_ONLY) return fail(ctx, RC_ERR_INVALID, f + "unknown flags");
    if (smooth_n < 0) return fail(ctx, RC_ERR_INVALID, f + "smooth_n must not be negative");
    if (in_total < 0 || cam_total < 0 || (kp_in && kp_total < 0)) return fail(ctx, RC_ERR_INVALID, f + "a total must not be negative");
    for (int i = 0; i < 6; ++i)
        if (imu_joint_ids_host[i] < 0 || imu_joint_ids_host[i] > 23) return fail(ctx, RC_ERR_INVALID, f + "IMU joint id outside 0 .. 23");
    const long long r = cam_repeat;
    long long in_sum = 0, cam_sum = 0, kp_sum = 0, frames = 0;
    for (int i = 0; i < n_seq; ++i) {
        const std::string who = "sequence " + std::to_string(i);
        const long long in = in_frames_host[i], cams = cam_frames_host[i];
        if (in < 1 || in > in_total) return fail(ctx, RC_ERR_INVALID, f + who + " gives no frame (or more than in_total)");
        if (cams < 1 || cams > cam_total) return fail(ctx, RC_ERR_INVALID, f + who + " has no camera row (or more than cam_total)");
        if (r == 0 && cams != 1) return fail(ctx, RC_ERR_INVALID, f + who + ": cam_repeat 0 takes ONE camera row per sequence");
        const long long out = (r == 0 || cams >= (in + r - 1) / r) ? in : r * cams;         // min(in, r cams) without the product overflowing
        if (smooth_n / 2 != 0 && out < 2 * (long long)smooth_n + 1)
            return fail(ctx, RC_ERR_INVALID, f + who + " gives " + std::to_string(out) + " frames: 2 * smooth_n + 1 needed");
        if (kp_in) {
            const long long kp = kp_frames_host[i];
            if (kp < 0 || kp > kp_total || kp < (out + 1) / 2)
                return fail(ctx, RC_ERR_INVALID, f + who + ": " + std::to_string(kp) + " detector frames do not cover " + std::to_string(out) + " output frames");
            kp_sum += kp;
        }
        in_sum += in;
        cam_sum += cams;
        frames += out;
    }
    if (in_sum != in_total) return fail(ctx, RC_ERR_INVALID, f + "the sequences hold " + std::to_string(in_sum) + " frames, in_total is " + std::to_string(in_total));
    if (cam_sum != cam_total) return fail(ctx, RC_ERR_INVALID, f + "the sequences hold " + std::to_string(cam_sum) + " camera rows, cam_total is " + std::to_string(cam_total));
    if (kp_in && kp_sum != kp_total) return fail(ctx, RC_ERR_INVALID, f + "the sequences hold " + std::to_string(kp_sum) + " detector frames, kp_total is " + std::to_string(kp_total));
    if (frames >= (1ll << 31) || cam_total >= (1ll << 31)) return fail(ctx, RC_ERR_INVALID, f + "2^31 output frames or camera rows, or more");
    for (long long c = 0; c < cam_total; ++c)
        for (int k = 0; k < 12; ++k)
            if (!std::isfinite(cam_T_host[c * 16 + k])) return fail(ctx, RC_ERR_INVALID, f + "camera row " + std::to_string(c) + " is not finite");
    if (!ctx->have_body) return fail(ctx, RC_ERR_STATE, f + "rc_set_body first");
    if (ctx->prep_V == 0) return fail(ctx, RC_ERR_STATE, f + "rc_set_shape_space first (the picked vertices)");
    if (ctx->prep_V != ctx->mesh_V) return fail(ctx, RC_ERR_STATE, f + "rc_set_mesh changed the vertex count since rc_set_shape_space");
    if (betas && !ctx->prep_basis) return fail(ctx, RC_ERR_STATE, f + "betas need the shape basis (rc_set_shape_space with shapedirs and J_regressor)");
    hipStream_t st = (hipStream_t)stream;
    // ---- the tables: pinned slots -> device, on `stream`
    const size_t G = (size_t)n_seq, NC = (size_t)cam_total;
    PrepSeq* th = nullptr;
    PrepCam* ch = nullptr;
    PrepCamRow* rh = nullptr;
    HIP_TRY(ctx, ctx->prep_tab.stage(G, &th));
    HIP_TRY(ctx, ctx->cam_tab.stage(G, &ch));
    HIP_TRY(ctx, ctx->cam_rows.stage(NC, &rh));
    long long in0 = 0, out0 = 0, cam0 = 0, kp0 = 0;
    for (int i = 0; i < n_seq; ++i) {
        const long long in = in_frames_host[i], cams = cam_frames_host[i];
        th[i].in0 = in0;
        th[i].out0 = out0;
        th[i].step = 1;
        th[i].out_n = (int)((r == 0 || cams >= (in + r - 1) / r) ? in : r * cams);
        ch[i].cam0 = cam0;
        ch[i].kp0 = kp0;
        ch[i].kp_n = kp_in ? (int)std::min<long long>(kp_frames_host[i], (1ll << 31) - 1) : 0;
        ch[i].pad = 0;
        in0 += in;
        out0 += th[i].out_n;
        cam0 += cams;
        kp0 += kp_in ? kp_frames_host[i] : 0;
    }
    for (size_t c = 0; c < NC; ++c)
        for (int k = 0; k < 12; ++k) rh[c].m[k] = cam_T_host[c * 16 + k];
    const size_t need_r = betas ? G : 1, need_v = vert6_out ? 0 : (size_t)frames * 18;
    if (!ctx->prep_tab.holds(G) || !ctx->cam_tab.holds(G) || !ctx->cam_rows.holds(NC) || need_r > ctx->prep_rest_n || need_v > ctx->prep_vert6_n) {
        HIP_TRY(ctx, hipDeviceSynchronize());                                  // (kernels of earlier calls, on any stream, may still read the old buffers)
        HIP_TRY(ctx, ctx->prep_tab.grow(G));
        HIP_TRY(ctx, ctx->cam_tab.grow(G));
        HIP_TRY(ctx, ctx->cam_rows.grow(NC));
        HIP_TRY(ctx, rc_grow(ctx->prep_rest_n, need_r, 2 * need_r, ctx->prep_rest, 2 * need_r));
        HIP_TRY(ctx, rc_grow(ctx->prep_vert6_n, need_v, need_v, ctx->prep_vert6, need_v));
    }
    HIP_TRY(ctx, ctx->prep_tab.upload(G, st));
    HIP_TRY(ctx, ctx->cam_tab.upload(G, st));
    HIP_TRY(ctx, ctx->cam_rows.upload(NC, st));
    HIP_TRY(ctx, ctx->prep_tab.record(st));
    HIP_TRY(ctx, ctx->cam_tab.record(st));
    HIP_TRY(ctx, ctx->cam_rows.record(st));
    rc_launch_prepare_camera_motions(ctx->body, ctx->mesh_vt, ctx->prep_sp, ctx->prep_tab.get(), ctx->cam_tab.get(), n_seq, frames, cam_repeat,
                                     (flags & RC_CAM_ROOT_ONLY) != 0, pose_aa, tran, betas, ctx->cam_rows.get(), kp_in, imu_joint_ids_host, smooth_n,
                                     ctx->prep_rest.get(), pose_out, tran_out, imu_ori, imu_acc, joint3d, sync_3d_mp,
                                     vert6_out ? vert6_out : ctx->prep_vert6.get(), kp_out, rest_joint_out, st);
    HIP_TRY(ctx, hipGetLastError());
    return RC_OK;
}
