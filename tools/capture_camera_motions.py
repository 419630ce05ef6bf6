#!/usr/bin/env python3
"""Write tests/golden/camera/camera_motions.npz by RUNNING THE REFERENCE on the development machine (never on the GPU box): what the
loops of preprocess_3dpw / preprocess_3dpwocc (preprocess.py:460-470, 477-483; :571-582, 589-599) and the flip of
preprocess_my_totalcapture_pre (:351-364, 379-385) compute for seeded sequences, which the restatement tests/camera_motion_ref.py and
the device pass (robustcap_amd/preprocess.prepare_camera_motions, rc_prepare_camera_motions) have to agree with.

Recipe, after tools/capture_motion_prepare.py's: per sequence the reference's own objects -- ``art.math.axis_angle_to_rotation_matrix``,
``np.repeat(cam_poses, 2)`` with the ``[:len(cam_pose)]`` / ``cam_pose[:len(posec)]`` pair, ``torch.matmul`` on the root,
``cam_pose.matmul(art.math.append_one(trans))``, ``body_model.forward_kinematics(posec, shape=, tran=, calc_mesh=True)`` of its
ParametricModel on the synthetic body pickle, ``preprocess._syn_acc`` and the Python loop of the keypoint interleave -- on seeded poses,
translations, betas, camera poses far from the identity and detector frames. The TotalCapture block runs the lines of :351-364 and
:379-385 (the file reading between them left out) on one more seeded sequence whose pose, IMU and Vicon lengths differ.

  pose.<i> [T,72]  tran.<i> [T,3]  beta.<i> [10]  cam.<i> [n,4,4] (30 Hz)  kp.<i> [k,33,3] (30 Hz)         the inputs
  posec.<i>  tranc.<i>  cam_T.<i>  joint3d.<i>  sync_3d_mp.<i>  vert6.<i>  imu_accc.<i>  imu_oric.<i>  joint2d_mp.<i>   what it computes
  tc.gt  tc.ori_raw  tc.acc_raw  tc.vicon                                                                       TotalCapture inputs
  tc.pose  tc.ori  tc.acc  tc.tran  tc.joint3d  tc.grot6  tc.vert6  tc.sync_3d_mp                               and what :351-385 gives

TEST INFRASTRUCTURE. The reference is imported with the recipe of oracle/capture_reference.py (its stand-in modules and synthetic body
pickle); numbers only are stored. The sha256 goes into tests/golden/camera/meta.json, which tests/test_camera_motions_cpu.py verifies.

Usage:  python tools/capture_camera_motions.py
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from oracle import _npz  # noqa: E402
from oracle import capture_reference as CR  # noqa: E402
from robustcap_amd import config as cfg  # noqa: E402
from robustcap_amd import synth  # noqa: E402

SEED, SMOOTH_N = 29, 2
IN, CAM, KP = (5, 13, 30), (3, 6, 15), (3, 6, 15)              # out = min(in, 2 cam) = (5, 12, 30)
TC = {"gt": 30, "imu": 28, "vicon": 33}                       # TotalCapture: the IMU rows are the shortest


def cameras(seed, stream, n):
    """n T_cw rows [n,4,4]: rotations that drift from a pose far from the identity, translations of a few metres"""
    aa = np.array([1.9, -0.7, 0.4]) + np.cumsum(0.05 * synth.normal(seed, stream, n * 3).reshape(n, 3), 0)
    T = np.zeros((n, 4, 4), np.float32)
    T[:, :3, :3] = synth._rodrigues(aa).astype(np.float32)
    T[:, :3, 3] = (np.array([0.4, -1.2, 4.0]) + np.cumsum(0.03 * synth.normal(seed, stream + 1, n * 3).reshape(n, 3), 0)).astype(np.float32)
    T[:, 3, 3] = 1
    return T


def inputs(seed):
    poses, trans, betas, cams, kps = [], [], [], [], []
    for i, (T, n, k) in enumerate(zip(IN, CAM, KP)):
        walk = np.cumsum(0.04 * synth.normal(seed, 10 + i, T * 72).reshape(T, 72), 0) + 0.5 * synth.normal(seed, 40 + i, 72)
        poses.append(walk.astype(np.float32))
        trans.append((np.cumsum(0.02 * synth.normal(seed, 70 + i, T * 3).reshape(T, 3), 0) + [0.2, 0.9, 0.1]).astype(np.float32))
        betas.append((4 * synth.uniform01(seed, 100 + i, 16) - 2).astype(np.float32))          # 16 entries: the first 10 are used (:461)
        cams.append(cameras(seed, 130 + 2 * i, n))
        kp = synth.uniform01(seed, 160 + i, k * 99).reshape(k, 33, 3).astype(np.float32)
        kp[..., :2] *= np.float32([1920, 1080])
        kps.append(kp)
    return poses, trans, betas, cams, kps


def totalcapture_inputs(seed):
    gt = (np.cumsum(0.04 * synth.normal(seed, 200, TC["gt"] * 72).reshape(-1, 72), 0) + 0.5 * synth.normal(seed, 201, 72)).astype(np.float32)
    ori = synth._rodrigues(2.5 * (synth.uniform01(seed, 202, TC["imu"] * 18).reshape(-1, 3) - 0.5)).astype(np.float32).reshape(-1, 6, 3, 3)
    acc = (3 * synth.normal(seed, 203, TC["imu"] * 18)).reshape(-1, 6, 3).astype(np.float32)
    vicon = (np.cumsum(0.02 * synth.normal(seed, 204, TC["vicon"] * 3).reshape(-1, 3), 0) + [0.5, 1.0, -1.5]).astype(np.float32)
    return gt, ori, acc, vicon


def main():
    art, sig_mp, body = CR.import_reference()                         # (the working directory is now a temporary one)
    import preprocess                                                 # (builds its body model when imported, like net.sig_mp)
    syn_acc, bm = preprocess._syn_acc, sig_mp.body_model
    mp, vi, ji = torch.tensor(cfg.mp_mask), torch.tensor(cfg.vi_mask), torch.tensor(cfg.ji_mask)
    poses, trans, betas, cams, kps = inputs(SEED)
    arrays = {}
    for i, (p, t, b, c, k) in enumerate(zip(poses, trans, betas, cams, kps)):
        # ---- preprocess.py:571-582 (preprocess_3dpwocc: the variant that also cuts the cameras to the pose)
        pose = torch.from_numpy(p.copy()).float()
        shape = torch.from_numpy(b[:10].copy()).float()
        cam_pose = torch.from_numpy(np.repeat(c, 2, axis=0)).float()
        tr = torch.from_numpy(t.copy()).float()[:len(cam_pose)]
        posec = art.math.axis_angle_to_rotation_matrix(pose.reshape(-1, 24, 3)).view(-1, 24, 3, 3)[:len(cam_pose)]
        cam_pose = cam_pose[:len(posec)]
        posec[:, 0] = torch.matmul(cam_pose[:, :3, :3], posec[:, 0])
        tranc = cam_pose.matmul(art.math.append_one(tr).unsqueeze(-1)).squeeze(-1)[..., :3]
        grot, joint, vert = bm.forward_kinematics(posec, shape=shape, tran=tranc, calc_mesh=True)
        oric = grot[:, ji]
        accc = syn_acc(vert[:, vi])
        # ---- :589-599
        mp_data = [torch.from_numpy(x.copy()) for x in k]
        joint_2d = []
        for index in range(len(mp_data)):
            if index == len(mp_data) - 1:
                joint_2d.append(mp_data[index])
                joint_2d.append(mp_data[index])
                continue
            joint_2d.append(mp_data[index])
            joint_2d.append((mp_data[index + 1] + mp_data[index]) / 2.0)
        j2d = torch.stack(joint_2d)[:len(posec)].float()
        assert posec.shape[0] == tranc.shape[0] == oric.shape[0] == accc.shape[0] == j2d.shape[0]
        arrays[f"pose.{i}"], arrays[f"tran.{i}"], arrays[f"beta.{i}"], arrays[f"cam.{i}"], arrays[f"kp.{i}"] = p, t, b[:10], c, k
        for name, v in (("posec", posec), ("tranc", tranc), ("cam_T", cam_pose), ("joint3d", joint), ("sync_3d_mp", vert[:, mp]),
                        ("vert6", vert[:, vi]), ("imu_accc", accc), ("imu_oric", oric), ("joint2d_mp", j2d)):
            arrays[f"{name}.{i}"] = v.numpy().astype(np.float32)
    # ---- TotalCapture: preprocess.py:351-364, 379-385
    gt, ori_raw, acc_raw, vicon = totalcapture_inputs(SEED)
    flip = torch.tensor([[-1, 0, 0], [0, 1, 0], [0, 0, -1]], dtype=torch.float32)
    ori = torch.from_numpy(ori_raw.copy()).float()[:, torch.tensor([2, 3, 0, 1, 4, 5])]
    acc = torch.from_numpy(acc_raw.copy()).float()[:, torch.tensor([2, 3, 0, 1, 4, 5])]
    pose = art.math.axis_angle_to_rotation_matrix(torch.from_numpy(gt.copy()).float()).reshape(-1, 24, 3, 3)
    if acc.shape[0] < pose.shape[0]:
        pose = pose[:acc.shape[0]]
    elif acc.shape[0] > pose.shape[0]:
        acc = acc[:pose.shape[0]]
        ori = ori[:pose.shape[0]]
    pose[:, 0] = torch.matmul(flip, pose[:, 0])
    ori_f = torch.matmul(flip, ori)
    acc_f = torch.matmul(flip, acc.unsqueeze(-1)).squeeze(-1)
    tran = torch.from_numpy(vicon.copy())
    if acc.shape[0] < tran.shape[0]:
        tran = tran[:acc.shape[0]]
    assert tran.shape[0] == acc.shape[0] and acc.shape[0] == ori.shape[0] and ori.shape[0] == pose.shape[0]
    tran[:, 0] = tran[:, 0] - 0.03
    tran[:, 1] = tran[:, 1] + (1 / (10 + tran[:, 2]))
    grot, kp_3d, vert = bm.forward_kinematics(pose, tran=tran, calc_mesh=True)
    arrays.update({"tc.gt": gt, "tc.ori_raw": ori_raw, "tc.acc_raw": acc_raw, "tc.vicon": vicon})
    for name, v in (("pose", pose), ("ori", ori_f), ("acc", acc_f), ("tran", tran), ("joint3d", kp_3d), ("grot6", grot[:, ji]),
                    ("vert6", vert[:, vi]), ("sync_3d_mp", vert[:, mp])):
        arrays[f"tc.{name}"] = v.numpy().astype(np.float32)
    out = os.path.join(CR.OUT, "camera")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "camera_motions.npz")
    _npz.save(path, **arrays)
    with open(path, "rb") as f:
        digest = hashlib.sha256(f.read()).hexdigest()
    with open(os.path.join(out, "meta.json"), "w") as f:
        json.dump({"sha256": {"camera_motions.npz": digest}, "seed": SEED, "in": list(IN), "cam": list(CAM), "kp": list(KP), "cam_repeat": 2,
                   "smooth_n": SMOOTH_N, "body_seed": CR.BODY_SEED, "totalcapture": TC,
                   "variant": "preprocess_3dpwocc (:571-599): the cameras are cut to the pose as well; preprocess_3dpw raises there"},
                  f, indent=1, sort_keys=True)
    print("wrote tests/golden/camera/camera_motions.npz:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
