"""What art.FullMotionEvaluator costs for an evaluation's worth of rows: ONE rc_motion_metrics call for all rows (csrc/rc_motion.hip) beside
the float32 torch transcription of articulate/evaluator.py:365-394 evaluated row by row on the device, and beside rc_mesh_metrics (the
existing PVE sweep, csrc/rc_metrics.hip) on the same frames.

    python tools/motion_metrics_bench.py [--rows 72] [--frames 600] [--out profiles/motion_metrics_bench.txt]
    python tools/motion_metrics_bench.py --tree PATH --label "parent commit" --only mesh ...

The workload is config 3's: 72 (sequence, camera) rows of 600 frames, one group each, the 6890-vertex body. --tree PATH runs the package of
another checkout (built there); one without rc_motion_metrics (the parent commit) times rc_mesh_metrics only (--only mesh). HIP events,
the median of 5 after a warm-up, everything taken twice in one session: other work shares the machine. The counted work of the vertex
sweep (FLOPs and bytes from the shapes) stands beside the measured time; the peaks are the MI355X's vector fp32 rate and HBM bandwidth.
"""
import argparse
import math
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=72)
ap.add_argument("--frames", type=int, default=600)
ap.add_argument("--fps", type=int, default=60)
ap.add_argument("--only", choices=("all", "mesh"), default="all")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose robustcap_amd is timed")
ap.add_argument("--label", default="this tree")
ap.add_argument("--out", help="also append the lines to this file")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from robustcap_amd import _lib, synth  # noqa: E402
from robustcap_amd.body import ParametricModel  # noqa: E402

REPS = 5
PEAK_FP32, PEAK_HBM = 157.3e12, 6.29e12          # vector fp32 FLOP/s (spec), HBM bytes/s (measured copy)
FG, NCOL = 32, 145                               # RC_MOTION_FG, the small columns of rc_motion.hip


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
    """seeded smooth poses, a prediction a few degrees off, and translations: device tensors of rows * T frames"""
    n = rows * T
    t = np.arange(n, dtype=np.float64)[:, None]
    aa = (0.5 * synth.normal(3, 0, 72).astype(np.float64)[None] * np.sin(0.11 * t + 6.28 * synth.uniform01(3, 1, 72).astype(np.float64)[None]))
    gt = synth._rodrigues(aa.reshape(n, 24, 3)).astype(np.float32)
    near = synth._rodrigues((0.08 * synth.normal(3, 2, n * 72)).reshape(n, 24, 3).astype(np.float64)).astype(np.float32)
    tt = (np.cumsum(0.01 * synth.normal(3, 3, n * 3).reshape(n, 3).astype(np.float64), axis=0) % 4.0).astype(np.float32)
    tp = (tt + 0.02 * synth.normal(3, 4, n * 3).reshape(n, 3)).astype(np.float32)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return d(np.matmul(gt, near)), d(gt), d(tp), d(tt)


class TorchEvaluator:
    """articulate/evaluator.py:365-394 with articulate/model.py:229-241 written out, float32, on the device; the angle in the atan2 form"""

    def __init__(self, body, fps, device):
        f = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(device)
        J = f(body["J"])
        self.j, self.x, self.w = J - J[:1], f(body["v_template"]) - J[:1], f(body["weights"])
        self.parent, self.fps = [int(p) for p in body["parent"]], fps

    def fk(self, pose, tran):
        n = pose.shape[0]
        G, P = [pose[:, 0]], [torch.zeros(n, 3, device=pose.device)]
        for i in range(1, 24):
            p = self.parent[i]
            G.append(G[p] @ pose[:, i])
            P.append(P[p] + (G[p] @ (self.j[i] - self.j[p]).view(1, 3, 1)).squeeze(-1))
        G, P = torch.stack(G, 1), torch.stack(P, 1)
        A = torch.cat((G, (P - (G @ self.j.view(1, 24, 3, 1)).squeeze(-1)).unsqueeze(-1)), -1)
        Tv = torch.tensordot(A, self.w, dims=([1], [1])).permute(0, 3, 1, 2)
        v = (Tv[..., :3] @ self.x.view(1, -1, 3, 1)).squeeze(-1) + Tv[..., 3]
        return G, P + tran.view(n, 1, 3), v + tran.view(n, 1, 3)

    @staticmethod
    def angle(a, b):
        D = a.transpose(-1, -2) @ b
        v = torch.stack((D[..., 2, 1] - D[..., 1, 2], D[..., 0, 2] - D[..., 2, 0], D[..., 1, 0] - D[..., 0, 1]), -1) * 0.5
        return torch.atan2(v.norm(dim=-1), (D[..., 0, 0] + D[..., 1, 1] + D[..., 2, 2] - 1) * 0.5) * (180.0 / math.pi)

    def __call__(self, pp, pt, tp, tt):
        f = self.fps
        gp, jp, vp = self.fk(pp, tp)
        gt, jt, vt = self.fk(pt, tt)
        off = (jt[:, 0] - jp[:, 0]).unsqueeze(1)
        tre, ve, je = (jp - jt).norm(dim=2), (vp + off - vt).norm(dim=2), (jp + off - jt).norm(dim=2)
        lae, gae = self.angle(pp, pt), self.angle(gp, gt)
        jkp = ((jp[3:] - 3 * jp[2:-1] + 3 * jp[1:-2] - jp[:-3]) * (f ** 3)).norm(dim=2)
        jkt = ((jt[3:] - 3 * jt[2:-1] + 3 * jt[1:-2] - jt[:-3]) * (f ** 3)).norm(dim=2)
        te = ((jp[f:, :1] - jp[:-f, :1]) - (jt[f:, :1] - jt[:-f, :1])).norm(dim=2)
        return torch.stack([torch.stack((x.mean(), x.std(dim=0).mean())) for x in (je, ve, lae, gae, jkp, jkt, te, tre)])


def main():
    dev = torch.device("cuda")
    body = synth.make_body(1)
    model = ParametricModel(body=body, device=dev)
    model._ensure_mesh()
    rows, T = args.rows, args.frames
    n, V = rows * T, body["v_template"].shape[0]
    pp, pt, tp, tt = motions(rows, T, dev)
    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))
    say(f"== {args.label}: {rows} rows x {T} frames = {n} frames, V = {V}, fps {args.fps}; ms, HIP events, median of {REPS} after a warm-up")
    per_frame = torch.empty(n, 3, device=dev)
    mesh = lambda: _lib.check(model._ctx, model._lib.rc_mesh_metrics(model._ctx, _lib.ptr(pp), _lib.ptr(pt), n, _lib.ptr(per_frame), None,
                                                                      _lib.stream_ptr()), "rc_mesh_metrics")
    has_motion = hasattr(model, "motion_metrics") and args.only == "all"
    if has_motion:
        sizes = [T] * rows
        full = lambda: model.motion_metrics(pp, pt, tp, tt, group_frames=sizes, fps=args.fps)
        lean = lambda: model.motion_metrics(pp, pt, tp, tt, group_frames=sizes, fps=args.fps, mesh=False)
        ev = TorchEvaluator(body, args.fps, dev)
        rowwise = lambda: [ev(pp[r * T:(r + 1) * T], pt[r * T:(r + 1) * T], tp[r * T:(r + 1) * T], tt[r * T:(r + 1) * T]) for r in range(rows)]
        # the two agree before either is timed (float32 both: a loose check that the same thing is measured)
        a, b = full()[0][0].cpu(), ev(pp[:T], pt[:T], tp[:T], tt[:T]).cpu()
        dev_rows = a[[0, 1, 2, 3, 4, 5, 6, 10]]
        rel = ((dev_rows - b).abs() / b.abs().clamp_min(1e-6)).max()
        say(f"row 0, device against the torch transcription: largest relative difference of the 16 entries {float(rel):.2e}")
        if not rel < 1e-3:
            raise SystemExit("the device and the torch transcription disagree: nothing timed")
    for run in (1, 2):
        t_mesh = timed(mesh)
        if not has_motion:
            say(f"run {run} rc_mesh_metrics {t_mesh:8.3f}")
            continue
        t_full, t_lean, t_torch = timed(full), timed(lean), timed(rowwise)
        say(f"run {run} rc_motion_metrics {t_full:8.3f}   RC_MOTION_NO_MESH {t_lean:8.3f}   (vertex sweep + finish {t_full - t_lean:8.3f})   "
            f"torch fp32 row by row {t_torch:9.3f}   rc_mesh_metrics {t_mesh:8.3f}")
        say(f"run {run} ratios: torch / rc_motion_metrics {t_torch / t_full:6.1f}x   rc_motion_metrics / rc_mesh_metrics {t_full / t_mesh:5.2f}x")
    if has_motion:
        blocks = rows * ((T + FG - 1) // FG)
        flop = n * V * (2 * 24 * 12 + 2 * 9 + 3 + 5 + 1 + 6)          # blend FMAs, the three dot products, the norm, the double sums
        byts = blocks * V * 16 * 2 + ((V + 1023) // 1024) * n * 1152
        l2 = blocks * V * 108 * 4                                     # every (frame block, slab) workgroup loads its vertices' weights: L2 hits
        say(f"vertex sweep, counted: {flop / 1e9:.1f} GFLOP (fp32 blend: 24 joints x 12 FMAs per vertex and frame) -> {flop / PEAK_FP32 * 1e3:.3f} ms at "
            f"{PEAK_FP32 / 1e12:.1f} TFLOP/s; {byts / 1e6:.1f} MB of partial sums written and read, transforms read per slab -> "
            f"{byts / PEAK_HBM * 1e3:.3f} ms at {PEAK_HBM / 1e12:.2f} TB/s; {l2 / 1e9:.2f} GB of skinning weights re-read per frame block from L2 "
            f"(the 3 MB constant set stays there): bound by the fp32 vector rate, not by memory")
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
