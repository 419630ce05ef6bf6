"""What moving rows of a running context costs: rc_save_rows and rc_load_rows (csrc/rc_rowstate.hip) at batch 256 and 1,024, for all rows
and for 16 scattered rows (one per 16-row block: the worst case of the rc_pk layout, a row owns 16 bytes of every 256), beside what existed
before for the (h, c) half of a row's state: six rc_get_state calls through the host.

    python tools/row_state_bench.py [--out profiles/row_state_bench.txt]

HIP events round one call, the median of 5 after a warm-up, everything taken twice in one session (other work shares the machine); the
rc_get_state path synchronises and copies to the host, so it is timed on the host clock. Beside every time stands the counted traffic --
the records written (or read) plus the same bytes read (or written) in the context, and the context side again at the 128-byte line
granularity the memory system moves -- divided by the HBM rate of 6.3 TB/s.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, nargs="+", default=[256, 1024])
ap.add_argument("--out", help="also append the lines to this file")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from robustcap_amd import synth  # noqa: E402
from robustcap_amd.net.sig_mp import Net  # noqa: E402
from robustcap_amd.rowstate import HIDDEN  # noqa: E402

REPS = 5
PEAK_HBM = 6.3e12
NETS = ("rnn2", "rnn3", "rnn4", "rnn6", "rnn7", "rnn8")


def timed_us(fn, reps=REPS):
    out = []
    fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(1e3 * a.elapsed_time(b))
    return statistics.median(out)


def host_us(fn, reps=REPS):
    out = []
    fn()
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append(1e6 * (time.perf_counter() - t0))
    return statistics.median(out)


def line_bytes(rows):
    """context-side bytes of a call at 128-byte lines: in rc_pk order a 16-row block's 256-byte piece of four k is two lines, rows 0-7 and
    8-15; c and the small block are contiguous per row"""
    pk_words = 2 * sum(HIDDEN) + 512                     # h of both layers of every net, x4l, x6l
    halves = {(r >> 4, (r >> 3) & 1) for r in rows}
    return len(halves) * (pk_words // 4) * 128 + len(rows) * 4 * (2 * sum(HIDDEN) + 160)


def main():
    lines = []
    say = lambda s: (print(s, flush=True), lines.append(s))
    sd, body = synth.make_state_dict(0), synth.make_body(1)
    say(f"== rc_save_rows / rc_load_rows; us, HIP events round one call, median of {REPS} after a warm-up, two runs; counted bytes / {PEAK_HBM / 1e12:.1f} TB/s")
    for B in args.batches:
        net = Net(body=body, batch=B)
        net.load_state_dict(sd)
        m = synth.make_motion(5, min(B, 32), 4, body, conf="mixed")
        rep = (B + 31) // 32
        ins = [torch.from_numpy(m[k]).repeat(rep, *([1] * (m[k].ndim - 1)))[:B].contiguous().cuda() for k in ("j2dc", "accc", "oric")]
        net.forward_sequence(*ins)                       # a running context: nonzero states and counters
        torch.cuda.synchronize()
        bpr, fmt = net.row_state_info()
        blocks = (B + 15) // 16
        scattered = sorted({min(B - 1, 16 * (i * blocks // 16) + (5 * i) % 16) for i in range(16)})     # one row in each of 16 blocks spread over the batch
        for what, rows in (("all rows", None), ("16 scattered rows", scattered)):
            n = B if rows is None else len(rows)
            state = net.save_rows(rows)
            torch.cuda.synchronize()
            io, keep = net._row_io(rows, n, state.data, bpr)
            save = lambda: net._lib.rc_save_rows(net._ctx, C.byref(io))
            load = lambda: net._lib.rc_load_rows(net._ctx, C.byref(io))
            useful = 2 * n * bpr
            lined = n * bpr + line_bytes(range(B) if rows is None else rows)
            for run in (1, 2):
                ts, tl = timed_us(save), timed_us(load)
                say(f"batch {B:5d} {what:18s} run {run}: save {ts:8.1f} us  load {tl:8.1f} us   counted {useful / 1e6:7.2f} MB -> "
                    f"{useful / PEAK_HBM * 1e6:6.2f} us ({useful / ts / 1e3:7.1f} GB/s save, {useful / tl / 1e3:7.1f} GB/s load); "
                    f"at 128-byte lines {lined / 1e6:7.2f} MB -> {lined / PEAK_HBM * 1e6:6.2f} us")
            assert torch.equal(net.save_rows(rows).data, state.data)          # loading a context's own records changes nothing
        old = lambda: [net.get_state(name) for name in NETS]
        for run in (1, 2):
            say(f"batch {B:5d} six rc_get_state calls through the host, the (h, c) half only, run {run}: {host_us(old):10.1f} us (host clock; "
                f"{B * 4 * 4 * sum(HIDDEN) / 1e6:.2f} MB of (h, c) delivered, every copy of h read back to pick one)")
        del net
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
