"""What the validation pass of the reference's train() costs the per-batch way -- net.rnnK and the loss under no_grad per 64 sequences,
losses.position_error for rnn4: entries every tree since tr.loss() has -- beside ONE ragged forward over the whole set and ONE
rc_subnet_eval (tr.validate's way; robustcap_amd/fit.py, losses.SubnetEval, csrc/rc_loss.hip).

    python tools/subnet_fit_bench.py [--S 256] [--lo 200] [--hi 2400] [--modes 0 1] [--out profiles/subnet_fit_bench.txt]
    python tools/subnet_fit_bench.py --tree PATH --label "parent commit" ...

(a) the validation pass over a seeded set of S sequences with lengths uniform in [lo, hi], full length, 64 a batch; rnn8 (bce_logits)
    and rnn4 (position_error) in each gemm mode: per batch | one pass; then the metric alone: rc_subnet_eval once against rc_subnet_loss
    group by group on aligned copies of the same groups (position_error: losses.position_error group by group).
(b) validation's share of a num_iter_between_vald cycle (config.TRAIN: 20 iterations for rnn8, 60 for rnn4, of 256 x 200 frames):
    between x the median iteration + the validation, both ways.
(c) an iteration of fit.train against the README loop (ds.batch -> tr(xs) -> loss -> backward -> opt.step), wall clock with one
    synchronise at the end, as the difference of an epoch of 20 and one of 10 iterations over 10 (fit.train's file writes cancel).
--tree PATH runs the package of another checkout (built there): one without rc_subnet_eval (the parent commit) gives the per-batch
columns only. HIP events, the median of 5 after a warm-up, everything taken twice in one session: other work shares the machine.
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--S", type=int, default=256)
ap.add_argument("--lo", type=int, default=200)
ap.add_argument("--hi", type=int, default=2400)
ap.add_argument("--N", type=int, default=256, help="sequences of a training iteration")
ap.add_argument("--T", type=int, default=200, help="frames of each")
ap.add_argument("--modes", type=int, nargs="+", default=[0, 1])
ap.add_argument("--parts", default="abc")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose robustcap_amd is timed")
ap.add_argument("--label", default="this tree")
ap.add_argument("--out", help="also append the lines to this file")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import torch  # noqa: E402

from robustcap_amd import _lib, config as cfg, losses, synth  # noqa: E402
from robustcap_amd.net.sig_mp import Net  # noqa: E402

REPS = 5
K = 64                       # valid_batch_size of every sub-net (net/sig_mp.py:352,430,566,693,783,827)
HAS_EVAL = hasattr(losses, "SubnetEval")
SPEC = {n: (i, h, o) for n, i, h, o in cfg.NETS}
PW = (3.5, 0.25)


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


def validation_set(name, device):
    nin, _, nout = SPEC[name]
    g = torch.Generator().manual_seed(11)
    lengths = torch.randint(args.lo, args.hi + 1, (args.S,), generator=g).tolist()
    F = sum(lengths)
    x = torch.randn(F, nin, generator=g).to(device)
    y = ((torch.rand(F, nout, generator=g) < 0.4).float() if name == "rnn8" else torch.randn(F, nout, generator=g)).to(device)
    return lengths, list(torch.split(x, lengths)), list(torch.split(y, lengths))


def main():
    body, sd = synth.make_body(1), synth.make_state_dict(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"== {args.label}: S = {args.S} sequences of {args.lo} .. {args.hi} frames, {K} a validation batch; iterations of {args.N} x {args.T} "
        f"frames; median of {REPS} in ms")
    for run in (1, 2):
        for split in args.modes:
            net = Net(body=body, batch=1)
            net.load_state_dict(sd)
            net.set_gemm_mode(bool(split))
            for name in ("rnn8", "rnn4"):
                tr = net.trainable(name)
                nin, H, nout = SPEC[name]
                lengths, xs, labels = validation_set(name, net.device)
                groups = [sum(lengths[a:a + K]) for a in range(0, args.S, K)]
                steps_batches, steps_one = sum(max(lengths[a:a + K]) for a in range(0, args.S, K)), max(lengths)
                rnn = getattr(net, name)
                loss = tr.loss(PW) if name == "rnn8" else None

                def per_batch():
                    with torch.no_grad():
                        vals = []
                        for a in range(0, args.S, K):
                            ys = rnn(xs[a:a + K])
                            vals.append(loss(ys, labels[a:a + K]) if loss else losses.position_error(ys, labels[a:a + K]))
                        return float(sum(vals) / len(vals))

                t_batch = t_one = float("nan")
                if "a" in args.parts or "b" in args.parts:
                    t_batch = timed(per_batch)
                    if HAS_EVAL:
                        ev = tr.evaluator(pos_weight=PW) if name == "rnn8" else tr.evaluator()

                        def one_pass():
                            with torch.no_grad():
                                return losses.reference_mean(ev(rnn(xs), labels, group_rows=K))

                        t_one = timed(one_pass)
                        v_a, v_b = per_batch(), one_pass()
                        say(f"run {run} gemm mode {split} {name} (a) validation, {sum(lengths)} frames in {len(groups)} batches: per batch "
                            f"{t_batch:9.2f} ({steps_batches} steps)  one pass {t_one:9.2f} ({steps_one} steps)  ratio {t_batch / t_one:5.2f}  "
                            f"values {v_a:.7f} {v_b:.7f}")
                    else:
                        say(f"run {run} gemm mode {split} {name} (a) validation, {sum(lengths)} frames in {len(groups)} batches: per batch "
                            f"{t_batch:9.2f} ({steps_batches} steps)")
                if "a" in args.parts and split == args.modes[0]:
                    # the metric alone on outputs already there: aligned copies of every group, so that rc_subnet_loss takes them
                    yo = torch.randn(sum(lengths), nout, device=net.device)
                    yl = torch.cat(labels)
                    gx, gy = [t.clone() for t in torch.split(yo, groups)], [t.clone() for t in torch.split(yl, groups)]
                    if name == "rnn8":
                        value = torch.empty((), device=net.device)

                        def by_group():
                            for a, b in zip(gx, gy):
                                net._lib.rc_subnet_loss(net._ctx, losses.KINDS["bce_logits"], _lib.ptr(a), _lib.ptr(b), a.shape[0], nout,
                                                        _lib.ptr(loss.pos_weight), _lib.ptr(value), None, _lib.stream_ptr())
                    else:
                        def by_group():
                            for a, b in zip(gx, gy):
                                losses.position_error(a, b)
                    t_group = timed(by_group)
                    if HAS_EVAL:
                        t_eval = timed(lambda: ev(yo, yl, group_sizes=groups))
                        say(f"run {run} {name} (a) the metric alone ({ev.kind}): group by group {t_group:8.4f}  rc_subnet_eval {t_eval:8.4f}  "
                            f"ratio {t_group / t_eval:5.2f}")
                    else:
                        say(f"run {run} {name} (a) the metric alone: group by group {t_group:8.4f}")
                if "b" in args.parts:
                    txs = [torch.randn(args.T, nin, device=net.device) for _ in range(args.N)]
                    tl = (torch.rand(args.N * args.T, nout, device=net.device) < 0.4).float()
                    lf, opt = tr.loss(PW) if name == "rnn8" else tr.loss(), tr.optimizer(lr=1e-6, clip_grad_norm=1.0)

                    def iteration():
                        opt.zero_grad()
                        lf(tr(txs), tl).backward()
                        opt.step()

                    t_it = timed(iteration)
                    between = cfg.TRAIN[name]["num_iter_between_vald"] if hasattr(cfg, "TRAIN") else (20 if name == "rnn8" else 60)
                    share = lambda t: 100 * t / (between * t_it + t)
                    say(f"run {run} gemm mode {split} {name} (b) iteration {t_it:8.2f} x {between}: validation's share of a cycle per batch "
                        f"{share(t_batch):5.1f} %" + (f"  one pass {share(t_one):5.1f} %  cycle {between * t_it + t_batch:9.1f} -> "
                                                      f"{between * t_it + t_one:9.1f}" if HAS_EVAL else ""))
                del tr
            del net
    if "c" in args.parts and HAS_EVAL:
        from robustcap_amd import fit
        for run in (1, 2):
            net = Net(body=body, batch=1)
            net.load_state_dict(sd)
            name = "rnn8"
            nin, H, nout = SPEC[name]
            g = torch.Generator().manual_seed(12)
            data = [torch.randn(args.T, nin, generator=g) for _ in range(20 * args.N)]
            label = [(torch.rand(args.T, nout, generator=g) < 0.4).float() for _ in range(20 * args.N)]
            tr = net.trainable(name)
            ds = {n: tr.dataset(data[:n * args.N], label[:n * args.N]) for n in (10, 20)}

            def readme(n):
                lf, opt = tr.loss(PW), tr.optimizer(lr=1e-6, clip_grad_norm=1.0)
                tr.train()
                for idx in fit.epoch_order(len(ds[n]), 0, 0).split(args.N):
                    xs, labels = ds[n].batch(idx.tolist())
                    loss = lf(tr(xs), labels)
                    opt.zero_grad()
                    loss.backward()
                    opt.step()

            def fitted(n):
                with tempfile.TemporaryDirectory() as d:
                    fit.train(tr, ds[n], None, d, loss_fn=tr.loss(PW), optimizer=tr.optimizer(lr=1e-6), batch_size=args.N, num_epoch=1,
                              clip_grad_norm=1.0, load_last_states=False)

            def wall(fn, n):
                out = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    fn(n)
                    torch.cuda.synchronize()
                    out.append(1e3 * (time.perf_counter() - t))
                return statistics.median(out[1:])

            r10, r20, f10, f20 = wall(readme, 10), wall(readme, 20), wall(fitted, 10), wall(fitted, 20)
            say(f"run {run} (c) {name}, per iteration = (epoch of 20 - epoch of 10) / 10: README loop {(r20 - r10) / 10:8.2f}  fit.train "
                f"{(f20 - f10) / 10:8.2f}  (epochs: {r10:8.1f} {r20:8.1f} | {f10:8.1f} {f20:8.1f})")
            del net
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
