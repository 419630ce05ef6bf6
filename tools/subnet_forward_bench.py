"""Sub-net forward over sequences (rc_subnet_forward, time-hoisted) against the same frames stepped through rc_lstm_step.

    python tools/subnet_forward_bench.py [--T 512] [--N 1 8 32 256] [--nets rnn2 rnn3 rnn4 rnn6 rnn7 rnn8]

Per sub-net, N sequences of T frames, both gemm modes: the sequence form is one call; the stepped form is T calls of rc_lstm_step
through ctypes on a Net(batch=N) with no synchronisation between them. Each is timed with HIP events around the whole call sequence,
median of 5 repetitions after one warm-up. Prints one line per case: frames/s of each and their ratio.

Roof fraction of the tall GEMMs (relu(linear1), both layers' x halves, linear2 over every frame of a chunk: the 256-row x 64-column
instantiation rc_subnet_gemm_kernel<4, 4, mode>, which the per-step launches of at most 512 rows never use) from a kernel trace, not
from counters -- one net and one N per run so that every such dispatch belongs to it:

    rocprofv3 --kernel-trace --stats -d DIR -o subnet -- python tools/subnet_forward_bench.py --nets rnn4 --N 256 --seq-only
    python tools/subnet_forward_bench.py --nets rnn4 --N 256 --roof-db DIR/.../subnet_results.db

FLOPs are the useful ones, 2 (in H + 2 H 4H + H out) per frame; roofs: split mode 416.7 TFLOP/s fp32-equivalent (2.5 PFLOP/s bf16 / 6
partial products), mode 0 the fp32 MFMA peak, 157.3 TFLOP/s.
"""
import argparse
import ctypes as C
import os
import re
import sqlite3
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from robustcap_amd import _lib, config as cfg, synth  # noqa: E402
from robustcap_amd.net.sig_mp import Net  # noqa: E402


def timed(fn, reps=5):
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


ROOF = {0: 157.3e12, 1: 2.5e15 / 6}
REPS = 5


def roof(args, spec):
    """Tall-GEMM time per mode from a rocpd database of a --seq-only run, against the FLOPs of its (REPS + 1) calls per mode."""
    (name,), (N,) = args.nets, args.N
    nin, H, nout = spec[name]
    flops = 2.0 * (nin * H + 2 * H * 4 * H + H * nout) * N * args.T * (REPS + 1)
    rows_max = (256 << 20) // (4 * ((nin + 127) // 128 * 128 + 6 * H)) // 16 * 16     # RC_SUBNET_SCRATCH_BYTES per chunk
    db = sqlite3.connect(args.roof_db)
    tabs = [r[0] for r in db.execute("select name from sqlite_master where type='table'")]
    disp = next(t for t in tabs if t.startswith("rocpd_kernel_dispatch"))
    sym = next(t for t in tabs if t.startswith("rocpd_info_kernel_symbol"))
    cols = [r[1] for r in db.execute(f"pragma table_info({disp})")]
    scol = [r[1] for r in db.execute(f"pragma table_info({sym})")]
    name_col = "kernel_name" if "kernel_name" in scol else ("display_name" if "display_name" in scol else "name")
    key = "kernel_id" if "kernel_id" in cols else "kernel_symbol_id"
    rows = db.execute(f"select s.{name_col}, count(*), sum(d.end - d.start) from {disp} d join {sym} s on d.{key} = s.id "
                      f"group by s.{name_col}").fetchall()
    for mode in args.modes:
        b = "true" if mode else "false"       # demangled, or the Itanium-mangled symbol (rc_subnet_gemm_kernelILi4ELi4ELb1E...)
        pat = re.compile(r"rc_subnet_gemm_kernel(<4,\s*4,\s*" + b + ">|ILi4ELi4ELb" + str(mode) + "E)")
        hit = [(c, ns) for n, c, ns in rows if pat.search(n)]
        if not hit:
            print(f"mode {mode} {name} N={N}: no tall-GEMM dispatches in the trace")
            continue
        calls, ns = sum(c for c, _ in hit), sum(t for _, t in hit)
        rate = flops / (ns * 1e-9)
        print(f"mode {mode} {name} N={N:4d} T={args.T}: tall GEMM {calls} dispatches, {ns / 1e6:.3f} ms, {rate / 1e12:.1f} TFLOP/s = "
              f"{rate / ROOF[mode]:.3f} of the {ROOF[mode] / 1e12:.1f} TFLOP/s roof (M <= {min(N * args.T, rows_max)} rows per launch)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=512)
    ap.add_argument("--N", type=int, nargs="+", default=[1, 8, 32, 256])
    ap.add_argument("--nets", nargs="+", default=[n for n, *_ in cfg.NETS])
    ap.add_argument("--modes", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--seq-only", action="store_true", help="time the sequence form only (kernel-trace runs)")
    ap.add_argument("--roof-db", help="rocpd database of a --seq-only run of ONE net and ONE N: print the tall GEMM's roof fraction")
    args = ap.parse_args()
    spec = {n: (i, h, o) for n, i, h, o in cfg.NETS}
    if args.roof_db:
        return roof(args, spec)
    sd, body = synth.make_state_dict(0), synth.make_body(1)
    lib = _lib.load()
    for split in args.modes:
        for N in args.N:
            seq = Net(body=body, batch=1)
            seq.load_state_dict(sd)
            seq.set_gemm_mode(bool(split))
            step = Net(body=body, batch=N)
            step.load_state_dict(sd)
            step.set_gemm_mode(bool(split))
            for name in args.nets:
                nin, H, nout = spec[name]
                x = torch.randn(N * args.T, nin, device="cuda")
                y = torch.empty(N * args.T, nout, device="cuda")
                xt = torch.randn(args.T, N, nin, device="cuda")
                yt = torch.empty(N, nout, device="cuda")
                lens = (C.c_int32 * N)(*([args.T] * N))

                def run_seq():
                    _lib.check(seq._ctx, lib.rc_subnet_forward(seq._ctx, name.encode(), N, lens, _lib.ptr(x), _lib.ptr(y), None, None,
                                                               None, None, _lib.stream_ptr()), "rc_subnet_forward")

                def run_step():
                    s = _lib.stream_ptr()
                    for t in range(args.T):
                        _lib.check(step._ctx, lib.rc_lstm_step(step._ctx, name.encode(), _lib.ptr(xt[t]), None, _lib.ptr(yt), s), "rc_lstm_step")

                ms_seq = timed(run_seq, REPS)
                f = N * args.T
                if args.seq_only:
                    print(f"mode {split} {name} N={N:4d} T={args.T}: sequence {f / ms_seq * 1e3:12.0f} frames/s ({ms_seq:8.3f} ms)", flush=True)
                    continue
                ms_step = timed(run_step, REPS)
                print(f"mode {split} {name} N={N:4d} T={args.T}: sequence {f / ms_seq * 1e3:12.0f} frames/s ({ms_seq:8.3f} ms)  "
                      f"stepped {f / ms_step * 1e3:12.0f} frames/s ({ms_step:8.3f} ms)  ratio {ms_step / ms_seq:5.2f}", flush=True)
            del seq, step


if __name__ == "__main__":
    main()
