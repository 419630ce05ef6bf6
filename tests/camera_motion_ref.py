"""The camera-frame motion preparation restated in numpy, every operation in float64 or, on request, float32 (helper of
test_camera_motions_cpu.py and test_gpu_camera_motions.py; no library): preprocess.py:460-470 / :571-582 (3DPW and 3DPW-OCC: a T_cw per
frame, the 30 Hz camera poses repeated, ``posec[:, 0] = R_cw posec[:, 0]``, ``tranc = T_cw (tran; 1)``, a body per person,
``forward_kinematics(posec, shape, tranc, calc_mesh=True)``, ``_syn_acc``), the keypoint interleave of :477-483 and the TotalCapture
steps of :351-364, :379-385. The body, the chain, the skin and the stencil are tests/motion_prepare_ref.py's.

The float32 variant follows the reference's order of operations (a batched 3 x 3 product for the root, the 4 x 4 product on the
homogeneous translation), so that its distance from the float64 run is the error the reference's own arithmetic has."""
import numpy as np

import motion_prepare_ref as M
from subnet_corpus_ref import aa_to_R

TC_ORDER = [2, 3, 0, 1, 4, 5]
TC_FLIP = np.diag([-1.0, 1.0, -1.0])


# ------------------------------------------------------------------------------------------------ tables alone
def output_lengths(in_frames, cam_frames, cam_repeat):
    """len(posec) after ``[:len(cam_pose)]`` and ``cam_pose[:len(posec)]`` with ``cam_pose = np.repeat(cam, r)``; r = 0: a static camera"""
    r = int(cam_repeat)
    return [int(n) if r == 0 else len(np.arange(int(n))[:len(np.repeat(np.arange(int(c)), r))]) for n, c in zip(in_frames, cam_frames)]


def camera_rows(cam, out_len, cam_repeat):
    """the [out_len,4,4] rows actually used"""
    cam = np.asarray(cam).reshape(-1, 4, 4)
    return np.repeat(cam, int(cam_repeat), axis=0)[:out_len] if cam_repeat else np.repeat(cam[:1], out_len, axis=0)


def interleave(kp, out_len=None):
    """preprocess.py:477-483 as the reference writes it (a Python loop over the detector's frames), then ``[:len(posec)]`` (:599)"""
    kp = np.asarray(kp)
    out = []
    for index in range(len(kp)):
        if index == len(kp) - 1:
            out.append(kp[index])
            out.append(kp[index])
            continue
        out.append(kp[index])
        out.append((kp[index + 1] + kp[index]) / kp.dtype.type(2.0))
    out = np.stack(out) if out else np.zeros((0,) + kp.shape[1:], kp.dtype)
    return out if out_len is None else out[:out_len]


# ------------------------------------------------------------------------------------------------ arithmetic
def to_camera(R, tran, rows, f, root_only=False):
    """:466-467: (posec [T,24,3,3] with the root left-multiplied by R_cw, tranc = (T_cw (tran; 1))[:3]) in ``f``"""
    rows = np.asarray(rows).astype(f)
    R = np.asarray(R).astype(f).copy()
    R[:, 0] = np.matmul(rows[:, :3, :3], R[:, 0]).astype(f)
    tran = np.asarray(tran).astype(f)
    if root_only:
        return R, tran
    h = np.concatenate([tran, np.ones((tran.shape[0], 1), f)], 1)
    full = rows.copy()
    full[:, 3] = np.array([0, 0, 0, 1], f)                                  # (row 3 of a T_cw; the library ignores what is stored there)
    return R, np.matmul(full, h[..., None])[..., 0].astype(f)[:, :3]


def prepare(body, poses, trans, cams, betas, cam_repeat, smooth_n, landmark_ids, vertex_ids, joint_ids, dtype=np.float64, root_only=False,
            keypoints=None):
    """preprocess.py:460-470 for lists of sequences: poses [T_i,24,3] axis-angle, trans [T_i,3], cams [n_i,4,4]. Returns lists per
    sequence: posec, tranc, joint3d, sync_3d_mp, vert6, imu_accc, imu_oric, cam_T (the rows used), rest_joint and, with ``keypoints``
    (float32, never converted: the interleave is exact in its own format), joint2d_mp."""
    f = dtype
    ids = [int(i) for i in landmark_ids] + [int(i) for i in vertex_ids]
    w = np.asarray(body["weights"])[ids]
    out = {k: [] for k in ("posec", "tranc", "joint3d", "sync_3d_mp", "vert6", "imu_accc", "imu_oric", "cam_T", "rest_joint", "joint2d_mp")}
    lens = output_lengths([len(p) for p in poses], [len(np.asarray(c).reshape(-1, 4, 4)) for c in cams], cam_repeat)
    for i, (p, t, c, T) in enumerate(zip(poses, trans, cams, lens)):
        rows = camera_rows(c, T, cam_repeat)
        R = aa_to_R(np.asarray(p).astype(f)[:T].reshape(-1, 3), f).reshape(T, 24, 3, 3)
        R, tc = to_camera(R, np.asarray(t)[:T], rows, f, root_only)
        J, j, v = M.rest_body(body, None if betas is None else betas[i], f)
        grot, joint, vert = M.forward(body, R, j, v[ids], w, tc, f)
        out["posec"].append(R), out["tranc"].append(tc), out["joint3d"].append(joint), out["sync_3d_mp"].append(vert[:, :33])
        out["vert6"].append(vert[:, 33:]), out["imu_accc"].append(M.syn_acc(vert[:, 33:], smooth_n, f))
        out["imu_oric"].append(grot[:, [int(q) for q in joint_ids]]), out["cam_T"].append(rows), out["rest_joint"].append(J)
        if keypoints is not None:
            out["joint2d_mp"].append(interleave(np.asarray(keypoints[i], np.float32), T))
    return out


def totalcapture_clip(gt_aa, imu_ori, imu_acc, vicon):
    """:351-358, :379-380: the IMU reorder and the clipping to the common length (pose against acc, then the translation)"""
    ori, acc = np.asarray(imu_ori)[:, TC_ORDER], np.asarray(imu_acc)[:, TC_ORDER]
    pose = np.asarray(gt_aa)
    if acc.shape[0] < pose.shape[0]:
        pose = pose[:acc.shape[0]]
    elif acc.shape[0] > pose.shape[0]:
        acc, ori = acc[:pose.shape[0]], ori[:pose.shape[0]]
    tran = np.asarray(vicon)
    if acc.shape[0] < tran.shape[0]:
        tran = tran[:acc.shape[0]]
    return pose, ori, acc, tran


def totalcapture_tran(tran, f):
    """:382-383"""
    t = np.asarray(tran).astype(f).copy()
    t[:, 0] = t[:, 0] - f(0.03)
    t[:, 1] = t[:, 1] + (f(1) / (f(10) + t[:, 2]))
    return t


def totalcapture_flip(ori, acc, f):
    """:362-364 on the re-ordered rows"""
    F = TC_FLIP.astype(f)
    return np.matmul(F, np.asarray(ori).astype(f)).astype(f), np.matmul(F, np.asarray(acc).astype(f)[..., None])[..., 0].astype(f)
