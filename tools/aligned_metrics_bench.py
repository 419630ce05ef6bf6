"""What the evaluators' SVD alignment (align_joint = -1, R/t/s) costs for an evaluation's worth of rows: ONE rc_aligned_metrics call for all
rows (csrc/rc_align.hip) beside three yardsticks on the same frames:

  * the reference's expression in float32 torch on device tensors: forward_kinematics(calc_mesh=True) of both motions and art.math.svd_rotate
    (articulate/math/angular.py:159-183: one torch.svd per frame in a Python loop) on the joints and on the mesh, timed on --torch-rows rows and
    scaled to all of them (the subsample is stated in the output);
  * rc_motion_metrics with and without the mesh: what the unaligned evaluator costs;
  * rc_mesh_metrics: the 14-keypoint Procrustes and the PVE sweep.

    python tools/aligned_metrics_bench.py [--rows 72] [--frames 600] [--out profiles/aligned_metrics_bench.txt]

The workload is config 3's: 72 (sequence, camera) rows of 600 frames, one group each, the 6890-vertex body. HIP events, the median of 5 after
a warm-up, everything taken twice in one session: other work shares the machine. The call is also taken apart through the C entry: xform
alone runs the frame kernel with the fold and nothing else; RC_MOTION_NO_MESH runs the frame kernel without the fold and the finish. The
counted work (FLOPs and bytes from the shapes) stands beside the measured times; the peaks are the MI355X's vector fp32 / fp64 rates and HBM
bandwidth.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=72)
ap.add_argument("--frames", type=int, default=600)
ap.add_argument("--torch-rows", type=int, default=1, help="rows the torch yardstick is timed on (scaled to --rows)")
ap.add_argument("--out", help="also append the lines to this file")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from robustcap_amd import _lib, synth  # noqa: E402
from robustcap_amd.body import ParametricModel  # noqa: E402

REPS = 5
PEAK_FP32, PEAK_FP64, PEAK_HBM = 157.3e12, 78.6e12, 6.29e12      # vector FLOP/s (spec), HBM bytes/s (measured copy)
FRAME_FLOATS = 312                                                # ALN_FRAME_FLOATS of rc_align.hip


def timed(fn, reps=REPS):
    out = []
    fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def motions(rows, T, device):
    """seeded smooth poses and a prediction a few degrees off: device tensors of rows * T frames"""
    n = rows * T
    t = np.arange(n, dtype=np.float64)[:, None]
    aa = (0.5 * synth.normal(3, 0, 72).astype(np.float64)[None] * np.sin(0.11 * t + 6.28 * synth.uniform01(3, 1, 72).astype(np.float64)[None]))
    gt = synth._rodrigues(aa.reshape(n, 24, 3)).astype(np.float32)
    near = synth._rodrigues((0.08 * synth.normal(3, 2, n * 72)).reshape(n, 24, 3).astype(np.float64)).astype(np.float32)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return d(np.matmul(gt, near)), d(gt)


class TorchAligned:
    """articulate/evaluator.py:193-210 and 296-313 at align_joint = -1, with articulate/model.py:229-241 and angular.py:159-183 written out in
    float32 torch on the device"""

    def __init__(self, body, device):
        f = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(device)
        J = f(body["J"])
        self.j, self.x, self.w = J - J[:1], f(body["v_template"]) - J[:1], f(body["weights"])
        self.parent = [int(p) for p in body["parent"]]

    def fk(self, pose):
        n = pose.shape[0]
        G, P = [pose[:, 0]], [torch.zeros(n, 3, device=pose.device)]
        for i in range(1, 24):
            p = self.parent[i]
            G.append(G[p] @ pose[:, i])
            P.append(P[p] + (G[p] @ (self.j[i] - self.j[p]).view(1, 3, 1)).squeeze(-1))
        G, P = torch.stack(G, 1), torch.stack(P, 1)
        A = torch.cat((G, (P - (G @ self.j.view(1, 24, 3, 1)).squeeze(-1)).unsqueeze(-1)), -1)
        Tv = torch.tensordot(A, self.w, dims=([1], [1])).permute(0, 3, 1, 2)
        return P, (Tv[..., :3] @ self.x.view(1, -1, 3, 1)).squeeze(-1) + Tv[..., 3]

    def svd_rotate(self, src, dst):
        ms, md = src.mean(dim=1, keepdim=True), dst.mean(dim=1, keepdim=True)
        a, b = src - ms, dst - md
        scale = ((b * b).sum(dim=[1, 2]) / (a * a).sum(dim=[1, 2])).sqrt()
        H = a.transpose(1, 2).bmm(b)
        R = []
        for i in range(H.shape[0]):                                  # the reference's loop: one SVD per frame
            u, _, vh = torch.linalg.svd(H[i])                        # on the device; a torch without a device SVD raises: nothing is timed
            v = vh.t().clone()
            q = v.mm(u.t())
            if q.det() < -0.9:
                v[2].neg_()
                q = v.mm(u.t())
            R.append(q)
        R = torch.stack(R)
        tr = -scale.view(-1, 1, 1) * R.bmm(ms.transpose(1, 2)) + md.transpose(1, 2)
        return scale.view(-1, 1, 1) * src.bmm(R.transpose(1, 2)) + tr.transpose(1, 2)

    def __call__(self, pp, pt):
        jp, vp = self.fk(pp)
        jt, vt = self.fk(pt)
        return (self.svd_rotate(jp, jt) - jt).norm(dim=2).mean(dim=0), (self.svd_rotate(vp, vt) - vt).norm(dim=2).mean()


def main():
    dev = torch.device("cuda")
    body = synth.make_body(1)
    model = ParametricModel(body=body, device=dev)
    model._ensure_mesh()
    rows, T = args.rows, args.frames
    n, V = rows * T, body["v_template"].shape[0]
    pp, pt = motions(rows, T, dev)
    sizes = [T] * rows
    arr = (C.c_int64 * rows)(*sizes)
    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))
    say(f"== {rows} rows x {T} frames = {n} frames, V = {V}, align_joint = -1 (R/t/s); ms, HIP events, median of {REPS} after a warm-up")
    w = np.asarray(body["weights"])
    pairs = sum(1 for j in range(24) for k in range(j, 24) if (w[:, j] * w[:, k]).any())
    full = lambda: model.aligned_metrics(pp, pt, group_frames=sizes, align=-1)
    lean = lambda: model.aligned_metrics(pp, pt, group_frames=sizes, align=-1, mesh=False)
    xf = torch.empty(n, 2, 13, device=dev)
    fold_only = lambda: _lib.check(model._ctx, model._lib.rc_aligned_metrics(model._ctx, _lib.ptr(pp), _lib.ptr(pt), n, rows, arr, 7, 0, None, None,
                                                                            None, _lib.ptr(xf), _lib.stream_ptr()), "rc_aligned_metrics")
    motion = lambda: model.motion_metrics(pp, pt, group_frames=sizes)
    motion_lean = lambda: model.motion_metrics(pp, pt, group_frames=sizes, mesh=False)
    per_frame = torch.empty(n, 3, device=dev)
    mesh = lambda: _lib.check(model._ctx, model._lib.rc_mesh_metrics(model._ctx, _lib.ptr(pp), _lib.ptr(pt), n, _lib.ptr(per_frame), None,
                                                                      _lib.stream_ptr()), "rc_mesh_metrics")
    ev = TorchAligned(body, dev)
    k = max(1, min(args.torch_rows, rows))
    rowwise = lambda: [ev(pp[r * T:(r + 1) * T], pt[r * T:(r + 1) * T]) for r in range(k)]
    # the two agree before either is timed (float32 against float64 inside: a loose check that the same thing is measured)
    je, me = full()
    tj, tm = ev(pp[:T], pt[:T])
    rel = max(float(((je[0] - tj).abs() / tj.abs().clamp_min(1e-6)).max()), float((me[0] - tm).abs() / tm.abs()))
    say(f"row 0, device against the torch transcription: largest relative difference of the 24 joint errors and the mesh error {rel:.2e} "
        f"(torch SVD on the device)")
    if not rel < 1e-3:
        raise SystemExit("the device and the torch transcription disagree: nothing timed")
    for run in (1, 2):
        t_full, t_lean, t_fold = timed(full), timed(lean), timed(fold_only)
        t_motion, t_mlean, t_mesh = timed(motion), timed(motion_lean), timed(mesh)
        t_torch = timed(rowwise) * rows / k
        say(f"run {run} rc_aligned_metrics {t_full:8.3f}   RC_MOTION_NO_MESH {t_lean:8.3f}   xform only (frame kernel with the fold, no sweep) {t_fold:8.3f}   "
            f"(sweep + finish {t_full - t_fold:8.3f}; the fold and the mesh fit {t_fold - t_lean:8.3f})")
        say(f"run {run} rc_motion_metrics {t_motion:8.3f}   without the mesh {t_mlean:8.3f}   rc_mesh_metrics {t_mesh:8.3f}   "
            f"torch fp32, {k} of {rows} rows timed and scaled {t_torch:10.1f}")
        say(f"run {run} ratios: torch / rc_aligned_metrics {t_torch / t_full:7.1f}x   rc_aligned_metrics / rc_motion_metrics {t_full / t_motion:5.2f}x   "
            f"rc_aligned_metrics / rc_mesh_metrics {t_full / t_mesh:5.2f}x   the fold / a vertex sweep {(t_fold - t_lean) / max(t_full - t_fold, 1e-9):5.2f}x")
    n_slab = (V + 1023) // 1024
    fold_flop = n * 2 * (pairs * 240 - 24 * 84 + 24 * 24 + 200)      # pairs j < k: 240 double FMAs, j == k: 156; the sums of means; Jacobi and D_j
    sweep_flop = n * V * (2 * 24 * 12 + 2 * 9 + 3 + 5 + 1)
    byts = n * FRAME_FLOATS * 4 * (1 + n_slab) + n * n_slab * 16 + n * 2 * 864
    say(f"counted: the fold {fold_flop / 1e9:.2f} GFLOP fp64 over {pairs} listed pairs of 300 ({fold_flop / PEAK_FP64 * 1e3:.3f} ms at "
        f"{PEAK_FP64 / 1e12:.1f} TFLOP/s; a wave per frame with 64 lanes over the pairs and LDS-resident transforms: latency, not rate); "
        f"the sweep {sweep_flop / 1e9:.1f} GFLOP fp32 ({sweep_flop / PEAK_FP32 * 1e3:.3f} ms at {PEAK_FP32 / 1e12:.1f} TFLOP/s: bound by the fp32 "
        f"vector rate like rc_motion_sweep_kernel, without its six double accumulators per vertex); {byts / 1e6:.1f} MB of poses, scratch rows "
        f"(read once per slab) and frame sums ({byts / PEAK_HBM * 1e3:.3f} ms at {PEAK_HBM / 1e12:.2f} TB/s)")
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
