"""What dropout costs a training iteration of a sub-net: forward + backward + fused optimiser step (tr.optimizer) in training mode
(tr.train(): the Philox masks of rc_dropout.hip as separate launches between the existing ones, two rc_dropout_apply calls in the
Python backward) beside the same iteration in eval mode.

    python tools/subnet_dropout_bench.py [--nets rnn8 rnn4] [--N 32 256] [--T 200] [--modes 0 1] [--out profiles/subnet_dropout_bench.txt]
    python tools/subnet_dropout_bench.py --tree PATH --label parent ...

N sequences of T frames, HIP events around the whole iteration, median of 5 after a warm-up of the same shape, one GPU. --tree PATH
runs the package of another checkout (built there; e.g. the commit before the masks existed) instead of this one: a trainer without
train() is timed in eval mode only, which is the figure this tree's eval-mode column should equal. Run the two trees in turn, twice:
other work shares the machine.
"""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--T", type=int, default=200)
ap.add_argument("--N", type=int, nargs="+", default=[32, 256])
ap.add_argument("--nets", nargs="+", default=["rnn8", "rnn4"])
ap.add_argument("--modes", type=int, nargs="+", default=[0, 1])
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose robustcap_amd is timed")
ap.add_argument("--label", default="this tree")
ap.add_argument("--out", help="also append the lines to this file")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import torch  # noqa: E402

from robustcap_amd import config as cfg, synth  # noqa: E402
from robustcap_amd.net.sig_mp import Net  # noqa: E402

REPS = 5


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


def main():
    spec = {n: (i, h, o) for n, i, h, o in cfg.NETS}
    sd, body = synth.make_state_dict(0), synth.make_body(1)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for split in args.modes:
        net = Net(body=body, batch=1)
        net.load_state_dict(sd)
        net.set_gemm_mode(bool(split))
        for name in args.nets:
            nin, H, nout = spec[name]
            tr = net.trainable(name)
            opt = tr.optimizer(lr=1e-6, clip_grad_norm=1.0)
            for N in args.N:
                xs = [torch.randn(args.T, nin, device="cuda") for _ in range(N)]

                def iteration():
                    opt.zero_grad()
                    torch.cat(tr(xs)).square().mean().backward()
                    opt.step()

                s = f"{args.label}: gemm mode {split} {name} N={N:4d} T={args.T}: eval mode {timed(iteration):9.3f} ms"
                if hasattr(tr, "train"):
                    tr.train()
                    ms = timed(iteration)
                    tr.eval()
                    s += f"  training mode (p = {tr.dropout}) {ms:9.3f} ms  eval mode again {timed(iteration):9.3f} ms"
                say(s)
        del net
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
