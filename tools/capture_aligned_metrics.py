#!/usr/bin/env python3
"""Write tests/golden/aligned/aligned_metrics.npz by RUNNING THE REFERENCE on the development machine (never on the GPU box): the reference's
own ``art.PerJointErrorEvaluator`` / ``art.MeshErrorEvaluator`` with ``align_joint`` -1 .. -5 (articulate/evaluator.py:155-215, 256-314) and
``art.math.svd_rotate`` (articulate/math/angular.py:144-184) on the seeded body (synth.make_body, capture_reference._write_body_pickle),
which the restatement tests/aligned_metrics_f64.py and the device (csrc/rc_align.hip) have to agree with.

  motions   `near`: pose_near of oracle/capture_metrics.py against its `gt` (tests/golden/metrics.npz, 24 frames). `far`: a seeded far pair of
            24 frames (aligned_metrics_f64.AUX["golden far"]) in place of that file's pose_far, 4 of whose frames have s3 < 1e-3 s1 in their
            joint H (3.6e-4 at worst), where no bound on a fitted rotation exists; 8 frames of the seeded pair have an improper joint fit
            (the row flip of angular.py:175-177 runs). The poses are regenerated from their seeds, not stored.
  stored    pje_<mode>_<motion> [3,24] and mesh_<mode>_<motion> (the evaluators' float32 results), mode in m1 .. m5;
            svd_<set>_<flags>_{R,t,s,moved} for the seeded point sets of aligned_metrics_f64.GOLDEN_POINTS (m = 3, 4, 24, 33 points and a
            mirrored set of 24) in the five flag combinations Rts, Rt, ts, t, s. The point sets themselves are regenerated from their seeds.

THE ANGLE ROWS PIN THE WIRING ONLY, as in tools/capture_motion_metrics.py: OpenCV is not installed here, cv2.Rodrigues is that tool's float64
numpy stand-in, and rows 1 and 2 of pje_* only have to equal the rows of align_joint=0 (pje_0_<motion> is stored for that).

TEST INFRASTRUCTURE; numbers only are stored. The fixture's sha256 goes into tests/golden/aligned/meta.json beside it, which
tests/test_aligned_metrics_cpu.py verifies.

Usage:  python tools/capture_aligned_metrics.py
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
sys.path.insert(0, os.path.join(REPO, "tools"))
from oracle import _npz  # noqa: E402
from oracle import capture_reference as CR  # noqa: E402
import aligned_metrics_f64 as A  # noqa: E402
from capture_motion_metrics import rodrigues_f64  # noqa: E402


def main():
    golden = np.load(os.path.join(CR.OUT, "metrics.npz"))
    art, _, body = CR.import_reference()
    sys.modules["cv2"].Rodrigues = rodrigues_f64                      # in place of the zeros of _install_stubs (see the module text)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).clone()
    g = {}
    for mname, (pp, pt) in A.golden_motions(golden, body).items():
        p, q = t(pp), t(pt)
        for mode in (0,) + tuple(A.MODES):
            out = art.PerJointErrorEvaluator("models/SMPL_male.pkl", align_joint=mode)(p, q)
            assert out.shape == (3, 24) and out.dtype == torch.float32
            g[f"pje_{'m' + str(-mode) if mode else '0'}_{mname}"] = out.numpy().astype(np.float64)
            if mode:
                mesh = art.MeshErrorEvaluator("models/SMPL_male.pkl", align_joint=mode)(p, q)
                g[f"mesh_m{-mode}_{mname}"] = np.float64(mesh)
    for sname, (seed, n, m, mirrored) in A.GOLDEN_POINTS.items():
        src, dst, _ = A.point_sets(seed, n, m, mirrored)
        for calc in A.FLAG_COMBOS:
            R, tr, s, moved = art.math.svd_rotate(t(src), t(dst), *calc)
            for k, v in (("R", R), ("t", tr), ("s", s), ("moved", moved)):
                g[f"svd_{sname}_{A.flag_name(calc)}_{k}"] = v.numpy().astype(np.float64)
    out_dir = os.path.join(CR.OUT, "aligned")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "aligned_metrics.npz")
    _npz.save(path, **g)
    with open(path, "rb") as f:
        digest = hashlib.sha256(f.read()).hexdigest()
    with open(os.path.join(out_dir, "meta.json"), "w") as f:
        json.dump({"sha256": {"aligned_metrics.npz": digest}}, f, indent=1, sort_keys=True)
    for k in sorted(g):
        if k.startswith("pje_"):
            print(k, g[k][0, :4])
        elif k.startswith("mesh_"):
            print(k, g[k])


if __name__ == "__main__":
    main()
