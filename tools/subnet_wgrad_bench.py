"""What the weight-gradient block of a sub-net's backward costs, in torch and in HIP (rc_subnet_weight_grads).

    python tools/subnet_wgrad_bench.py [--nets rnn8 rnn4] [--N 32 256] [--T 200] [--modes 0 1] [--out profiles/subnet_wgrad_bench.txt]
    python tools/subnet_wgrad_bench.py --tree PATH --label "parent commit" ...

N sequences of T frames, training mode at the sub-net's dropout rate, HIP events, median of 5 after a warm-up of the same shape, one GPU.
Per shape:
  (a) block/torch   the block of _SubnetFunction.backward that forms the twelve weight and bias gradients in torch (frames_t_matmul,
                    .sum(0), shift_within_sequences, the site-1 rc_dropout_apply), alone, on random operands;
  (b) block/device  rc_subnet_weight_grads alone on the same operands, with its useful FLOPs (2 F (16 H H + out H + H in)) against the roof
                    of the gemm mode: 157.3 TFLOP/s fp32 MFMA (mode 0), 416.7 TFLOP/s split-bf16 (mode 1);
  (c) iteration     forward + backward + tr.optimizer step, weight_grads="torch" and "device";
  peak              torch.cuda.max_memory_allocated over one backward, above what was allocated when it began.
--tree PATH runs the package of another checkout (built there): one without ``weight_grads`` (the parent commit) gives (a) and (c) for the
torch path only. Run the trees in turn, twice: other work shares the machine.
"""
import argparse
import ctypes as C
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

from robustcap_amd import _lib, config as cfg, synth, train  # noqa: E402
from robustcap_amd.net.sig_mp import Net  # noqa: E402

REPS = 5
ROOF = {0: 157.3, 1: 416.7}           # TFLOP/s


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


def torch_block(net, lengths, xcat, acts, h0, dy, d_gates, dP, drop):
    """The weight-gradient block of robustcap_amd/train.py's backward, as it stands there."""
    g = {}
    g["linear2.weight"], g["linear2.bias"] = train.frames_t_matmul(dy, acts[2]), dy.sum(0)
    inputs = (acts[0], train.dropout_apply(net, acts[1], 1, drop) if drop[0] > 0 else acts[1])
    for l in (0, 1):
        dG = d_gates[l]
        h_prev = train.shift_within_sequences(acts[l + 1], lengths, h0[l])
        g[f"rnn.weight_ih_l{l}"], g[f"rnn.weight_hh_l{l}"] = train.frames_t_matmul(dG, inputs[l]), train.frames_t_matmul(dG, h_prev)
        g[f"rnn.bias_ih_l{l}"] = g[f"rnn.bias_hh_l{l}"] = dG.sum(0)
    g["linear1.weight"], g["linear1.bias"] = train.frames_t_matmul(dP, xcat), dP.sum(0)
    return g


def device_block(net, name, lengths, xcat, acts, h0, dy, d_gates, dP, drop, shapes):
    g = [torch.empty(s, device="cuda") for s in shapes]
    table = (C.c_void_p * len(g))(*[t.data_ptr() for t in g])
    lens = (C.c_int32 * len(lengths))(*lengths)
    p = _lib.ptr
    rc = net._lib.rc_subnet_weight_grads(net._ctx, name.encode(), len(lengths), lens, p(xcat), p(acts), p(h0), p(dy), p(d_gates), p(dP), *drop,
                                         table, _lib.stream_ptr())
    _lib.check(net._ctx, rc, "rc_subnet_weight_grads")
    return g


def main():
    spec = {n: (i, h, o) for n, i, h, o in cfg.NETS}
    sd, body = synth.make_state_dict(0), synth.make_body(1)
    has_device = hasattr(train, "WEIGHT_GRADS")
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
            shapes = [sd[f"{name}.{k}"].shape for k in train.param_names(name) if not k.startswith("init_net.")]
            for N in args.N:
                head = f"{args.label}: gemm mode {split} {name} N={N:4d} T={args.T}:"
                lengths, F = [args.T] * N, args.T * N
                r = lambda *s: torch.randn(*s, device="cuda")
                xcat, acts, h0, dy, d_gates = r(F, nin), r(3, F, H), r(2, N, H), r(F, nout), r(2, F, 4 * H)
                dP = r(F, H) * (acts[0] > 0)
                drop = (float(cfg.DROPOUT[name]), 7, 3)
                s = f"{head} block/torch {timed(lambda: torch_block(net, lengths, xcat, acts, h0, dy, d_gates, dP, drop)):9.3f} ms"
                if has_device:
                    ms = timed(lambda: device_block(net, name, lengths, xcat, acts, h0, dy, d_gates, dP, drop, shapes))
                    tf = 2.0 * F * (16.0 * H * H + nout * H + H * nin) / (ms * 1e-3) / 1e12
                    s += f"  block/device {ms:9.3f} ms = {tf:6.1f} TFLOP/s useful ({100 * tf / ROOF[split]:4.1f} % of {ROOF[split]})"
                say(s)
                del xcat, acts, h0, dy, d_gates, dP
                xs = [torch.randn(args.T, nin, device="cuda") for _ in range(N)]
                s = f"{head} iteration"
                for wg in (("torch", "device") if has_device else ("torch",)):
                    tr = net.trainable(name, weight_grads=wg) if has_device else net.trainable(name)
                    tr.train()
                    opt = tr.optimizer(lr=1e-6, clip_grad_norm=1.0)

                    def iteration():
                        opt.zero_grad()
                        torch.cat(tr(xs)).square().mean().backward()
                        opt.step()

                    ms = timed(iteration)
                    opt.zero_grad()
                    loss = torch.cat(tr(xs)).square().mean()
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    loss.backward()
                    torch.cuda.synchronize()
                    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
                    s += f"  {wg} {ms:9.3f} ms (backward peak +{peak:8.1f} MiB)"
                    del tr, opt, loss
                say(s)
                del xs
                torch.cuda.empty_cache()
        del net
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
