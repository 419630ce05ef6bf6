"""The host-bound cost of the entries that stage a host-built table, for an A/B of two builds of the library (RC_LIB_PATH selects one):

    python tools/staged_tables_bench.py LABEL

A reduction of tools/subnet_batches_bench.py to its figures (i) ds.batch through Python and (ii) the entry alone, 20 calls back to back, at
256 samples x 200 frames (rnn8 plain, rnn4 world, rnn6 world; that tool's datasets and its timed()), and of tools/motion_metrics_bench.py to
rc_motion_metrics WITHOUT the vertex sweep at its workload (72 rows of 600 frames, one group each), once and 20 back to back. Left out:
those tools' reference's-way, whole-iteration and mesh parts, which do not pass through the staged tables. HIP events, median of 5 after a
warm-up; ms per call. One line "HOSTBOUND LABEL ..." per process: run the two builds alternately, one process per run. No thresholds."""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import motion_metrics_f64 as M
import subnet_batches_ref as R
from robustcap_amd import _lib, batches, body as body_mod, synth
from robustcap_amd.net.sig_mp import Net

REPS, BACK = 5, 20
SEED = (0x9E3779B9 << 32) | 0x1234ABCD
N, T = 256, 200
F = N * T


def timed(fn, reps=REPS):
    out = []
    fn()
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


net = Net(body=synth.make_body(1), batch=1)
net.load_state_dict(synth.make_state_dict(0))
dev = net.device
g = np.random.default_rng(0)
res = {}
for name, kind in (("rnn8", "plain"), ("rnn4", "world"), ("rnn6", "world")):
    tr = net.trainable(name)
    if kind == "plain":
        W, Wl = R.WIDTHS[name]
        d = g.normal(size=(F, W)).astype(np.float32)
        l = (g.uniform(size=(F, Wl)) < 0.3).astype(np.float32)
        pool = None
    else:
        d, l = R.world_corpus(1, (T,) * N)
        pool = torch.from_numpy(R.conf_pool(7, 1000))
    data, label = list(torch.from_numpy(d).split(T)), list(torch.from_numpy(l).split(T))
    ds = tr.dataset(data, label, split_size=T, kind=kind, conf_pool=pool).manual_seed(SEED)
    idx = torch.randperm(N, generator=torch.Generator().manual_seed(1)).tolist()
    res[f"{name} ds.batch"] = timed(lambda: ds.batch(idx))
    Wo, Wlo = ds.out_widths
    x, y = torch.empty(F, Wo, device=dev), torch.empty(F, Wlo, device=dev)
    off = (C.c_int64 * N)(*[ds.samples[i][0] for i in idx])
    lens = (C.c_int32 * N)(*[ds.samples[i][1] for i in idx])
    P = 0 if pool is None else pool.shape[0]
    entry = lambda: [net._lib.rc_subnet_batch(net._ctx, name.encode(), batches.KINDS[kind], _lib.ptr(ds.data), _lib.ptr(ds.label), N, off,
                                              lens, _lib.ptr(ds.pool), P, 1, SEED, k, _lib.ptr(x), _lib.ptr(y), _lib.stream_ptr())
                     for k in range(BACK)]
    res[f"{name} entry alone"] = timed(entry) / BACK
rows, frames = 72, 600
parts = [M.motion_pair(i, frames) for i in range(8)]
ins = [torch.from_numpy(np.ascontiguousarray(np.concatenate([parts[i % 8][q] for i in range(rows)]))).cuda() for q in range(4)]
model = body_mod.ParametricModel(body=synth.make_body(1))
sizes = [frames] * rows
res["motion no mesh"] = timed(lambda: model.motion_metrics(ins[0], ins[1], ins[2], ins[3], group_frames=sizes, mesh=False))
res["motion no mesh x20"] = timed(lambda: [model.motion_metrics(ins[0], ins[1], ins[2], ins[3], group_frames=sizes, mesh=False) for _ in range(BACK)]) / BACK
print("HOSTBOUND " + sys.argv[1] + " " + " | ".join(f"{k} {v:.4f}" for k, v in res.items()), flush=True)
