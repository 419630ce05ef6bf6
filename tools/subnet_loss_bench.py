"""What the loss of a training iteration costs, the way a user wrote it before tr.loss() existed -- in torch on the device, value plus
backward() to dy -- beside rc_subnet_loss (robustcap_amd/losses.py, csrc/rc_loss.hip).

    python tools/subnet_loss_bench.py [--N 256] [--T 200] [--modes 0 1] [--out profiles/subnet_loss_bench.txt]

Part 1, per kind at F = N * T frames: (i) the torch loss (for pose_fk the reference's loop of 23 matmuls per side, net/sig_mp.py:758-762)
and its backward(); (ii) loss_fn(x, y) and its backward(); the ratio (i) / (ii); the entry's counted bytes -- 12 per element (x, y read, dx
written) plus the partial sums (written once, read once) -- over the time of the entry alone, taken from 20 calls back to back through
ctypes (the Python call is bound by the host at this size), against the 6.3 TB/s this project takes as achievable.
Part 2, rnn7 and rnn3 in each gemm mode: a whole iteration (forward + loss + backward + fused optimiser step) the torch way and this
tree's way, in turn. HIP events, the median of 5 after a warm-up, everything taken twice: other work shares the machine.
"""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=256)
ap.add_argument("--T", type=int, default=200)
ap.add_argument("--modes", type=int, nargs="+", default=[0, 1])
ap.add_argument("--out", help="also append the lines to this file")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from robustcap_amd import _lib, config as cfg, losses, synth  # noqa: E402
from robustcap_amd.net.sig_mp import Net  # noqa: E402

REPS = 5
BACK = 20
HBM_BYTES_PER_S = 6.3e12


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


def torch_losses(body, device):
    """{kind: f(x, y)} in plain torch on the device."""
    J = torch.from_numpy(np.asarray(body["J"], np.float32))
    parent = [int(p) for p in body["parent"]]
    bones = torch.stack([J[i] - J[parent[i]] if i else J[0] * 0 for i in range(24)]).to(device).view(24, 3, 1)
    mse = torch.nn.MSELoss()

    def joints(p):
        v = p.view(-1, 6)
        c0 = torch.nn.functional.normalize(v[:, :3], dim=1, eps=0)
        c1 = torch.nn.functional.normalize(v[:, 3:] - (c0 * v[:, 3:]).sum(dim=1, keepdim=True) * c0, dim=1, eps=0)
        r = torch.stack((c0, c1, c0.cross(c1, dim=1)), dim=-1)
        r = torch.where(torch.isnan(r), torch.zeros_like(r), r).view(-1, 24, 3, 3)
        pb = torch.stack([r[:, parent[i]].matmul(bones[i]) for i in range(1, 24)], dim=1).squeeze(-1)
        js = [torch.zeros(r.shape[0], 3, device=device)]
        for i in range(1, 24):
            js.append(js[parent[i]] + pb[:, i - 1])
        return torch.stack(js, dim=1)

    def window(x, y):
        n = x.shape[0]
        return mse(x, y) + sum(mse(x[n % w:].view(-1, w, 3).sum(dim=1), y[n % w:].view(-1, w, 3).sum(dim=1)) for w in losses.WINDOWS)

    pw = torch.tensor([3.5, 0.25], device=device)
    return {"mse": mse, "bce_logits": torch.nn.BCEWithLogitsLoss(pos_weight=pw), "window_mse": window,
            "pose_fk": lambda x, y: mse(x, y) + 100 * mse(joints(x), joints(y))}, pw


def main():
    body, sd = synth.make_body(1), synth.make_state_dict(0)
    F = args.N * args.T
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    net = Net(body=body, batch=1)
    net.load_state_dict(sd)
    tl, pw = torch_losses(body, net.device)
    say(f"part 1: the loss alone, F = {args.N} x {args.T} = {F} frames, value + backward() to dy, median of {REPS} in ms")
    for run in (1, 2):
        for kind, W in (("mse", 69), ("mse", 3), ("bce_logits", 2), ("window_mse", 3), ("pose_fk", 144)):
            x = torch.randn(F, W, device=net.device).requires_grad_()
            y = (torch.rand(F, W, device=net.device) < 0.4).float() if kind == "bce_logits" else torch.randn(F, W, device=net.device)
            ours = losses.SubnetLoss(net, kind, pos_weight=pw if kind == "bce_logits" else None)

            def run_loss(fn):
                x.grad = None
                fn(x, y).backward()

            t_torch, t_ours = timed(lambda: run_loss(tl[kind])), timed(lambda: run_loss(ours))
            with torch.no_grad():
                t_value = timed(lambda: ours(x, y))
            # the entry alone, BACK calls back to back through ctypes: the Python call above is bound by the host at this size
            xd, value, dx = x.detach(), torch.empty((), device=net.device), torch.empty(F, W, device=net.device)
            entry = lambda: [net._lib.rc_subnet_loss(net._ctx, losses.KINDS[kind], _lib.ptr(xd), _lib.ptr(y), F, W, _lib.ptr(ours.pos_weight),
                                                     _lib.ptr(value), _lib.ptr(dx), _lib.stream_ptr()) for _ in range(BACK)]
            t_entry = timed(entry) / BACK
            nbytes = 12 * F * W + 16 * min(losses.MAX_PARTIALS, F * W)
            say(f"run {run} {kind:10s} W={W:3d}: torch {t_torch:8.3f}  tr.loss() + backward {t_ours:8.3f}  ratio {t_torch / t_ours:6.1f}  "
                f"value only, no dx {t_value:7.3f}  |  rc_subnet_loss alone ({BACK} back to back) {t_entry:7.4f}: counted {nbytes / 1e6:7.2f} MB "
                f"-> {nbytes / (t_entry * 1e-3) / 1e12:5.3f} TB/s = {100 * nbytes / (t_entry * 1e-3) / HBM_BYTES_PER_S:5.1f} % of 6.3 TB/s")
    del net
    say(f"part 2: a whole iteration (forward + loss + backward + tr.optimizer step), N = {args.N}, T = {args.T}, median of {REPS} in ms")
    spec = {n: (i, h, o) for n, i, h, o in cfg.NETS}
    for run in (1, 2):
        for split in args.modes:
            net = Net(body=body, batch=1)
            net.load_state_dict(sd)
            net.set_gemm_mode(bool(split))
            tl, _ = torch_losses(body, net.device)
            for name in ("rnn7", "rnn3"):
                nin, H, nout = spec[name]
                tr = net.trainable(name)
                opt = tr.optimizer(lr=1e-6, clip_grad_norm=1.0)
                xs = [torch.randn(args.T, nin, device=net.device) for _ in range(args.N)]
                labels = torch.randn(F, nout, device=net.device)
                kind = cfg.LOSS[name]
                ours = tr.loss()

                def iteration(loss_of):
                    opt.zero_grad()
                    loss_of(tr(xs)).backward()
                    opt.step()

                the_torch_way = lambda ys: tl[kind](torch.cat(ys), labels)
                no_loss = lambda ys: torch.cat(ys).sum()
                a = timed(lambda: iteration(the_torch_way))
                b = timed(lambda: iteration(lambda ys: ours(ys, labels)))
                a2 = timed(lambda: iteration(the_torch_way))
                b2 = timed(lambda: iteration(lambda ys: ours(ys, labels)))
                c = timed(lambda: iteration(no_loss))
                say(f"run {run} gemm mode {split} {name} ({kind}): torch loss {a:9.3f} {a2:9.3f}  tr.loss() {b:9.3f} {b2:9.3f}  "
                    f"sum() in place of a loss {c:9.3f}  -> the loss's share: torch {100 * (min(a, a2) - c) / min(a, a2):5.2f} %  "
                    f"tr.loss() {100 * (min(b, b2) - c) / min(b, b2):5.2f} %")
            del net
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
