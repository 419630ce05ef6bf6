"""One training step of a sub-net on the device (net.trainable(name): forward + backward + commit) against the same module built from
torch.nn.Linear / torch.nn.LSTM on the same GPU in float32 (forward + backward).

    python tools/subnet_backward_bench.py [--nets rnn3 rnn4] [--N 256 8] [--T 200] [--out profiles/subnet_backward_bench.txt]

N sequences of T frames (256 x 200 is the reference's training batch, net/sig_mp.py:345-348), both gemm modes. Timed with HIP events
around the whole step, median of 5 after a warm-up of the same shapes, on one GPU. The loss is the mean square of the concatenated
outputs; "commit" is rc_update_subnet_weights of parameters that an SGD step has just moved. Also: a commit by itself against
Net.load_state_dict of the same tensors (host wall clock around a synchronised call, median of 3).

The split between the step launches, the tall launches and torch's GEMMs comes from a kernel trace of a short run, on its own:

    rocprofv3 --kernel-trace --stats -d DIR -o bwd -- python tools/subnet_backward_bench.py --nets rnn4 --N 8 --modes 1 --no-torch
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

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


class TorchSubnet(torch.nn.Module):
    def __init__(self, name, sd, nin, H, nout):
        super().__init__()
        self.linear1, self.linear2, self.rnn = torch.nn.Linear(nin, H), torch.nn.Linear(H, nout), torch.nn.LSTM(H, H, 2)
        with torch.no_grad():
            for k, p in self.named_parameters():
                p.copy_(torch.from_numpy(sd[f"{name}.{k}"]))

    def forward(self, x):                                  # x [T, N, in]: equal lengths, no packing needed
        return self.linear2(self.rnn(torch.relu(self.linear1(x)))[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--N", type=int, nargs="+", default=[256, 8])
    ap.add_argument("--nets", nargs="+", default=["rnn3", "rnn4"])
    ap.add_argument("--modes", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--no-torch", action="store_true", help="skip the torch.nn module and the commit comparison (kernel-trace runs)")
    ap.add_argument("--out", help="also append the lines to this file")
    args = ap.parse_args()
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
            opt = torch.optim.SGD(tr.parameters(), lr=1e-6)
            ref = None if args.no_torch else TorchSubnet(name, sd, nin, H, nout).cuda()
            for N in args.N:
                xs = [torch.randn(args.T, nin, device="cuda") for _ in range(N)]
                xt = torch.stack(xs, 1)

                def fwd_bwd():
                    opt.zero_grad()
                    torch.cat(tr(xs)).square().mean().backward()

                def step():
                    fwd_bwd()
                    opt.step()
                    tr.commit()

                f = N * args.T
                ms_fb, ms_step = timed(fwd_bwd), timed(step)
                s = (f"mode {split} {name} N={N:4d} T={args.T}: forward + backward {ms_fb:9.3f} ms ({f / ms_fb * 1e3:10.0f} frames/s)  "
                     f"+ SGD step + commit {ms_step:9.3f} ms")
                if ref is not None:
                    def torch_fb():
                        ref.zero_grad()
                        ref(xt).square().mean().backward()
                    ms_t = timed(torch_fb)
                    s += f"  torch.nn fp32 forward + backward {ms_t:9.3f} ms  ratio torch / here {ms_t / ms_fb:5.2f}"
                say(s)
            if not args.no_torch:
                def wall(fn, reps=3):
                    out = []
                    for _ in range(reps):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        out.append((time.perf_counter() - t0) * 1e3)
                    return statistics.median(out)
                new = {f"{name}.{k}": p.detach().cpu() for k, p in tr.named_parameters()}
                ms_c, ms_l = wall(tr.commit), wall(lambda: net.load_state_dict(new, strict=False))
                say(f"mode {split} {name}: commit alone {ms_c:9.3f} ms (device synchronise at entry, wait at exit)  load_state_dict of the same "
                    f"tensors {ms_l:9.3f} ms  ratio {ms_l / ms_c:6.1f}")
        del net
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
