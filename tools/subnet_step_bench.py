"""The second half of a training iteration of one sub-net -- clip the gradient norm, Adam, and the packed weights current again -- two ways
on the same build:

    (i)  the existing path:  torch.nn.utils.clip_grad_norm_ + torch.optim.Adam.step() + tr.commit()
    (ii) the fused step:     tr.optimizer(...).step()   (rc_subnet_optim_step: one call, no host synchronisation, no read-back)

    python tools/subnet_step_bench.py [--nets rnn8 rnn4] [--out profiles/subnet_optim_step_bench.txt]

Gradients from one real backward (8 sequences of 20 frames). Timed with HIP events around the whole second half, median of 5 after a
warm-up, on one GPU; the events of (i) span its host synchronisations and its device-to-host copies, which is what the loop waits for.
(iii) the fused step's bytes, counted from the tensor sizes (below), over its time, as a fraction of 6.3 TB/s.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from robustcap_amd import config as cfg, synth  # noqa: E402
from robustcap_amd.net.sig_mp import Net  # noqa: E402

REPS = 5
HBM_BYTES_PER_S = 6.3e12
INIT = ((69, 512), (512, 1024), (1024, 2048))


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


def fused_step_bytes(name, nin, H, nout):
    """What rc_subnet_optim_step moves, from the shapes: the norm reads every gradient once (4 B); the update reads p, g, m, v and writes
    p, m, v per master element (28 B) and writes the fp32 pack and three bf16 planes per PADDED packed element (10 B), the row-major copy
    of a narrow linear2 (4 B); the transposed packs of the two LSTM layers are rebuilt from the fp32 packs (4 B read, 10 B written)."""
    up = lambda x, m: (x + m - 1) // m * m
    dense = [(H, nin), (nout, H)] + (list((n, k) for k, n in INIT) if name == "rnn2" else [])
    masters = 2 * (8 * H * H + 8 * H) + sum(n * k + n for n, k in dense)
    padded = 2 * 8 * H * H + sum(up(n, 32 if n <= 160 else 64) * up(k, 128) for n, k in dense)
    wrm = sum(n * k for n, k in dense if n <= 160)
    return 4 * masters + 28 * masters + 10 * padded + 4 * wrm + 2 * 8 * H * H * 14


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", nargs="+", default=["rnn8", "rnn4"])
    ap.add_argument("--out", help="also append the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("subnet_step_bench.py measures on a GPU; none found")
    spec = {n: (i, h, o) for n, i, h, o in cfg.NETS}
    sd, body = synth.make_state_dict(0), synth.make_body(1)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    net = Net(body=body, batch=1)
    net.load_state_dict(sd)
    for name in args.nets:
        nin, H, nout = spec[name]
        g = torch.Generator().manual_seed(1)
        xs = [torch.randn(20, nin, generator=g) for _ in range(8)]
        if name == "rnn2":
            xs = [(x, torch.randn(69, generator=g)) for x in xs]
        tr = net.trainable(name)
        torch.cat(tr(xs)).square().mean().backward()                  # one real backward; both ways step on these gradients
        grads = [p.grad.clone() for p in tr.parameters()]
        params = list(tr.parameters())
        adam = torch.optim.Adam(params, lr=1e-6)
        fused = tr.optimizer(lr=1e-6, clip_grad_norm=1.0)

        def old():
            for p, gr in zip(params, grads):                          # (clip_grad_norm_ scales in place: fresh copies, outside neither timing)
                p.grad.copy_(gr)
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            adam.step()
            tr.commit()

        def copy_only():
            for p, gr in zip(params, grads):
                p.grad.copy_(gr)

        ms_copy, ms_old, ms_new = timed(copy_only), timed(old), timed(fused.step)
        ms_old -= ms_copy
        nbytes = fused_step_bytes(name, nin, H, nout)
        say(f"{name} (H = {H}, {sum(p.numel() for p in params)} parameters): (i) clip_grad_norm_ + Adam.step + commit {ms_old:9.3f} ms   "
            f"(ii) fused step {ms_new:9.3f} ms   ratio (i) / (ii) {ms_old / ms_new:6.1f}   "
            f"(iii) {nbytes / 1e6:8.1f} MB counted -> {nbytes / (ms_new * 1e-3) / 1e12:5.2f} TB/s = {nbytes / (ms_new * 1e-3) / HBM_BYTES_PER_S:5.1%} of 6.3 TB/s")
        net.state_dict()                                              # (the lazy host copy: one download, outside the timings)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
