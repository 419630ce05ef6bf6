#!/usr/bin/env python3
"""Write tests/golden/motion/motion_metrics.npz by RUNNING THE REFERENCE on the development machine (never on the GPU box): the reference's
own ``art.FullMotionEvaluator`` (articulate/evaluator.py:317-394) on the seeded body (synth.make_body, capture_reference._write_body_pickle),
which the restatement tests/motion_metrics_f64.py and the device (csrc/rc_motion.hip) have to agree with.

  motions   the `near` / `far` / `same` poses of oracle/capture_metrics.py against its `gt` (tests/golden/metrics.npz: pose_near, pose_far,
            pose_gt, 24 frames), with the seeded translations of motion_metrics_f64.golden_translations (`same`: the truth's on both sides)
  settings  motion_metrics_f64.GOLDEN_SETTINGS: fps=60 without a mask | fps=5 with a joint mask | align_joint=5
            `long`: motion_metrics_f64.motion_pair(*GOLDEN_LONG), 131 frames, under fps=60 and align_joint=5 only: the one motion long
            enough for a finite te at the reference's default frame rate (71 one-second windows)
  stored    tran_p, tran_t [24,3] float32 and out_<setting>_<motion> [11,2] (the evaluator's float32 result, NaNs included);
            tran_p_long, tran_t_long [131,3] and out_fps60_long, out_align5_long. The long poses are not stored: meta.json holds the sha256 of
            the four input arrays (pose_p, pose_t, tran_p, tran_t), and the tests regenerate them from the seed and compare.

THE ANGLE ROWS PIN THE WIRING ONLY. OpenCV is not installed here, and capture_reference._install_stubs() gives cv2.Rodrigues a stand-in that
returns zeros; this tool replaces that stand-in with its own float64 numpy rotation -> axis-angle (the atan2 form, well conditioned at the
identity). Rows 2, 3, 8 and 9 therefore check which rotations are compared, in which order and in which unit -- not OpenCV's arithmetic:
the standing cv2.Rodrigues caveat (rotation -> axis-angle is unpinned against OpenCV itself) is unchanged.

TEST INFRASTRUCTURE; numbers only are stored. The fixture's sha256 goes into tests/golden/motion/meta.json beside it, which
tests/test_motion_metrics_cpu.py verifies (tests/golden/meta.json lists the top-level fixtures of oracle/capture_*.py only).

Usage:  python tools/capture_motion_metrics.py
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
import motion_metrics_f64 as M  # noqa: E402


def rodrigues_f64(m):
    """rotation matrix [3,3] -> (axis-angle [3,1] float64, None), the call shape of cv2.Rodrigues: angle = atan2(|vee|, (tr - 1) / 2)"""
    R = np.asarray(m, np.float64).reshape(3, 3)
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = np.linalg.norm(v), 0.5 * (np.trace(R) - 1.0)
    theta = np.arctan2(s, c)
    axis = v / s if s > 0.0 else np.zeros(3)
    return (axis * theta).reshape(3, 1), None


def main():
    golden = np.load(os.path.join(CR.OUT, "metrics.npz"))
    poses = {"near": golden["pose_near"], "far": golden["pose_far"], "same": golden["pose_gt"]}
    gt = golden["pose_gt"]
    T = gt.shape[0]
    tran_p, tran_t = M.golden_translations(T)
    art, _, _ = CR.import_reference()
    sys.modules["cv2"].Rodrigues = rodrigues_f64                      # in place of the zeros of _install_stubs (see the module text)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).clone()
    g = {"tran_p": tran_p, "tran_t": tran_t}
    for sname, (fps, mask, align) in M.GOLDEN_SETTINGS.items():
        ev = art.FullMotionEvaluator("models/SMPL_male.pkl", align_joint=align, fps=fps, joint_mask=mask)
        for mname, pose in poses.items():
            tp = tran_t if mname == "same" else tran_p
            out = ev(t(pose), t(gt), tran_p=t(tp), tran_t=t(tran_t))
            assert out.shape == (11, 2) and out.dtype == torch.float32
            g[f"out_{sname}_{mname}"] = out.numpy().astype(np.float64)
    # the `long` motion: 131 frames, so that te at fps 60 is finite (71 windows). Its poses are not stored: the tests regenerate them from
    # the seed and compare their sha256 with meta.json.
    (lpp, lpt, ltp, ltt), long_digests = M.golden_long()
    g["tran_p_long"], g["tran_t_long"] = ltp, ltt
    for sname in M.GOLDEN_LONG_SETTINGS:
        fps, mask, align = M.GOLDEN_SETTINGS[sname]
        ev = art.FullMotionEvaluator("models/SMPL_male.pkl", align_joint=align, fps=fps, joint_mask=mask)
        out = ev(t(lpp), t(lpt), tran_p=t(ltp), tran_t=t(ltt))
        assert out.shape == (11, 2) and out.dtype == torch.float32 and bool(torch.isfinite(out[6]).all())
        g[f"out_{sname}_long"] = out.numpy().astype(np.float64)
    out_dir = os.path.join(CR.OUT, "motion")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "motion_metrics.npz")
    _npz.save(path, **g)
    with open(path, "rb") as f:
        digest = hashlib.sha256(f.read()).hexdigest()
    with open(os.path.join(out_dir, "meta.json"), "w") as f:
        json.dump({"sha256": {"motion_metrics.npz": digest}, "long_inputs_sha256": long_digests}, f, indent=1, sort_keys=True)
    for k in sorted(g):
        if k.startswith("out_"):
            print(k, g[k][:, 0])


if __name__ == "__main__":
    main()
