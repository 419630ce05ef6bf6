"""What a training batch costs: ds.batch (robustcap_amd/batches.py, rc_subnet_batch, csrc/rc_augment.hip) beside the same batch built the
reference's way -- RNNDataset.__getitem__ sample by sample on the host with the sub-net's augment_fn or the AMASS __getitem__
(net/sig_mp.py:520-552, :649-679; the torch transcription of tests/test_subnet_batches_cpu.py in float32, its draws from torch.rand /
torch.randn / random.sample as there), then ``.to(device)`` per sample -- and the share of a whole training iteration either takes.

    python tools/subnet_batches_bench.py [--N 256] [--T 200] [--out profiles/subnet_batches_bench.txt]

Per case (rnn8 plain, rnn4 world, rnn6 world) at N samples of T frames: (i) ds.batch through Python, HIP events, median of 5 after a
warm-up; (ii) the C entry alone, 20 calls back to back through ctypes, and its counted bytes -- the corpus rows read (a world sample's
labels twice: the minimum over the sample, then the frame), the pool rows, both outputs written, from the tensor sizes -- over that time
against the 6.3 TB/s this project takes as achievable; (iii) the reference's way, host wall clock ending in a device synchronise;
(iv) a whole iteration (ds.batch -> tr(xs) -> tr.loss() -> backward -> opt.step()) and the share of it (i) and (iii) would be; for the
plain case (v) ``x + sigma * torch.randn_like(x)`` on the gathered tail on the device. Everything is taken twice: the host-bound figures
move with the host's load. No thresholds."""
import argparse
import ctypes as C
import os
import random
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=256)
ap.add_argument("--T", type=int, default=200)
ap.add_argument("--out", help="also append the lines to this file")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import subnet_batches_ref as R  # noqa: E402
import test_subnet_batches_cpu as TR  # noqa: E402
from robustcap_amd import _lib, batches, losses, synth  # noqa: E402
from robustcap_amd.net.sig_mp import Net  # noqa: E402

REPS, BACK, HBM_BYTES_PER_S = 5, 20, 6.3e12
SEED = (0x9E3779B9 << 32) | 0x1234ABCD


def say(line):
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


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


def walled(fn, reps=REPS):
    out = []
    fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out)


def reference_way(name, kind, data, label, conf, device):
    """One batch as DataLoader(..., collate_fn=RNNDataset.collate_fn) builds it: __getitem__ per sample, each moved to the device."""
    xs, ls = [], []
    for d, l in zip(data, label):
        if kind == "plain":
            x = d.clone()
            cols, sigma = R.AUGMENT[name]
            x[:, -cols:] = torch.normal(x[:, -cols:], sigma)
        else:
            T = d.shape[0]
            u = torch.rand(3).double().numpy()
            ang = [np.radians(lo * (1 - v) + hi * v) for (lo, hi), v in zip(R.CAMERA[name], u)]
            rows = random.sample(range(conf.shape[0]), T)
            x, l = TR.torch_getitem(name, d, l, conf, R.euler_yxz(*ang), torch.rand(3), rows, torch.randn(T, 33, 2), torch.randn(T, 69),
                                    dtype=torch.float32)
        xs.append(x.to(device))
        ls.append(l.to(device))
    return xs, ls


def main():
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    N, T = args.N, args.T
    F = N * T
    net = Net(body=synth.make_body(1), batch=1)
    net.load_state_dict(synth.make_state_dict(0))
    dev = net.device
    say(f"# subnet_batches_bench: N = {N} samples x T = {T} frames = {F} frames; HIP events, median of {REPS} after a warm-up; ms")
    g = np.random.default_rng(0)
    for run in (1, 2):
        for name, kind in (("rnn8", "plain"), ("rnn4", "world"), ("rnn6", "world")):
            tr = net.trainable(name)
            if kind == "plain":
                W, Wl = R.WIDTHS[name]
                d = g.normal(size=(F, W)).astype(np.float32)
                l = (g.uniform(size=(F, Wl)) < 0.3).astype(np.float32)
                pool = None
            else:
                d, l = R.world_corpus(run, (T,) * N)
                pool = torch.from_numpy(R.conf_pool(7, 1000))
            data, label = list(torch.from_numpy(d).split(T)), list(torch.from_numpy(l).split(T))
            ds = tr.dataset(data, label, split_size=T, kind=kind, conf_pool=pool).manual_seed(SEED)
            idx = torch.randperm(N, generator=torch.Generator().manual_seed(run)).tolist()
            t_batch = timed(lambda: ds.batch(idx))
            # the entry alone
            Wo, Wlo = ds.out_widths
            x, y = torch.empty(F, Wo, device=dev), torch.empty(F, Wlo, device=dev)
            off = (C.c_int64 * N)(*[ds.samples[i][0] for i in idx])
            lens = (C.c_int32 * N)(*[ds.samples[i][1] for i in idx])
            P = 0 if pool is None else pool.shape[0]
            entry = lambda: [net._lib.rc_subnet_batch(net._ctx, name.encode(), batches.KINDS[kind], _lib.ptr(ds.data), _lib.ptr(ds.label), N, off,
                                                      lens, _lib.ptr(ds.pool), P, 1, SEED, k, _lib.ptr(x), _lib.ptr(y), _lib.stream_ptr())
                             for k in range(BACK)]
            t_entry = timed(entry) / BACK
            Wi, Wli = ds.data.shape[1], ds.label.shape[1]
            nbytes = 4 * F * (Wi + Wli + Wo + Wlo) + (4 * F * (Wli + 33) if kind == "world" else 0)
            share = nbytes / (t_entry * 1e-3) / HBM_BYTES_PER_S
            conf = None if pool is None else pool[..., None]
            t_ref = walled(lambda: reference_way(name, kind, [data[i] for i in idx], [label[i] for i in idx], conf, dev))
            # a whole iteration on ds.batch
            loss_fn = tr.loss(losses.pos_weight_from_labels(ds)) if name == "rnn8" else tr.loss()
            opt = tr.optimizer(lr=1e-4, clip_grad_norm=1.0)
            tr.train()

            def iteration():
                xs, labels = ds.batch(idx)
                loss = loss_fn(tr(xs), labels)
                opt.zero_grad()
                loss.backward()
                opt.step()

            t_iter = timed(iteration)
            say(f"run {run} {name} {kind:5s}: ds.batch {t_batch:8.3f}  |  rc_subnet_batch alone ({BACK} back to back) {t_entry:8.4f}: counted "
                f"{nbytes / 1e6:7.1f} MB = {100 * share:5.1f} % of 6.3 TB/s  |  the reference's way (host, {N} x __getitem__ + .to(device)) "
                f"{t_ref:9.2f} = {t_ref / t_batch:7.0f} x  |  iteration with ds.batch {t_iter:8.2f}: ds.batch is {100 * t_batch / t_iter:5.2f} % "
                f"of it, the reference's way would add {100 * t_ref / t_iter:6.1f} %")
            if kind == "plain":
                cols, sigma = R.AUGMENT[name]
                rows = torch.cat([torch.arange(a, a + n) for a, n in (ds.samples[i] for i in idx)]).to(dev)

                def torch_device():
                    xg = ds.data.index_select(0, rows)
                    xg[:, -cols:] += sigma * torch.randn(F, cols, device=dev)
                    return xg, ds.label.index_select(0, rows)

                t_torch = timed(torch_device)
                say(f"run {run} {name} plain: gather + x + sigma * torch.randn on the device {t_torch:8.3f} (ds.batch {t_batch:8.3f}, the entry alone "
                    f"{t_entry:8.4f})")
            del ds, tr, opt


if __name__ == "__main__":
    main()
