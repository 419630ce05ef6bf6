#!/usr/bin/env python3
"""Write tests/golden/augment/augment_ops.npz by RUNNING THE REFERENCE on the development machine (never on the GPU box): the two functions of
the AMASS samples (net/sig_mp.py:520-552, :649-679) that the restatement tests/subnet_batches_ref.py has to agree with.

  angles [64, 3]        yaw, pitch, roll in radians (float64) inside the ranges of rnn4's and rnn6's cameras, both ends of every range among them
  euler_yxz [64, 3, 3]  art.math.euler_angle_to_rotation_matrix(angles, 'YXZ') (articulate/math/angular.py:337-350), float32
  kp [64, 33, 3]        keypoint sets (float32)
  bbox_scale [64]       get_bbox_scale(kp) (net/sig_mp.py:277-284), float32

TEST INFRASTRUCTURE. The reference is imported with the recipe of oracle/capture_reference.py (its stand-in modules and synthetic body
pickle); numbers only are stored. The fixture's sha256 goes into tests/golden/augment/meta.json beside it, which
tests/test_subnet_batches_cpu.py verifies (tests/golden/meta.json lists the top-level fixtures of oracle/capture_*.py only).

Usage:  python tools/capture_augment_ops.py
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import _npz  # noqa: E402
from oracle import capture_reference as CR  # noqa: E402
from robustcap_amd import config as cfg  # noqa: E402
from robustcap_amd import synth  # noqa: E402


def angle_triples():
    """64 triples in degrees: the eight corners of each camera's box (both ends of every range), then seeded points inside."""
    out = []
    for name in ("rnn4", "rnn6"):
        c = cfg.CAMERA[name]
        out += [(y, p, r) for y in c["yaw"] for p in c["pitch"] for r in c["roll"]]
    u = synth.uniform01(31, 0, (64 - len(out)) * 3).reshape(-1, 3).astype(np.float64)
    for i, row in enumerate(u):
        c = cfg.CAMERA["rnn4" if i % 2 == 0 else "rnn6"]
        out.append(tuple(lo + (hi - lo) * v for (lo, hi), v in zip((c["yaw"], c["pitch"], c["roll"]), row)))
    return np.radians(np.asarray(out, dtype=np.float64))


def main():
    art, sig_mp, _ = CR.import_reference()
    angles = angle_triples()
    R = art.math.euler_angle_to_rotation_matrix(torch.from_numpy(angles.copy()), seq="YXZ").numpy()
    kp = synth.uniform01(32, 0, 64 * 99).reshape(64, 33, 3).astype(np.float32)
    kp[..., :2] = (kp[..., :2] - 0.5) * np.linspace(0.05, 4.0, 64, dtype=np.float32)[:, None, None]
    scale = sig_mp.get_bbox_scale(torch.from_numpy(kp.copy())).numpy()
    out = os.path.join(CR.OUT, "augment")
    os.makedirs(out, exist_ok=True)
    _npz.save(os.path.join(out, "augment_ops.npz"), angles=angles, euler_yxz=R.astype(np.float32), kp=kp, bbox_scale=scale.astype(np.float32))
    with open(os.path.join(out, "augment_ops.npz"), "rb") as f:
        digest = hashlib.sha256(f.read()).hexdigest()
    with open(os.path.join(out, "meta.json"), "w") as f:
        json.dump({"sha256": {"augment_ops.npz": digest}}, f, indent=1, sort_keys=True)
    print("wrote tests/golden/augment/augment_ops.npz:", angles.shape, R.shape, kp.shape, scale.shape)


if __name__ == "__main__":
    main()
