"""What every sub-net is fed and when it steps, read off the device through a wire, on every path that runs a frame.

The cases of oracle/wiring_f64.py load tail_f64's state dict plus a wire: +-1 weights in linear1 and a power of two per column in
the g gate of LSTM layer 0 of every sub-net (and in init_net), everything that would let a sub-net's output depart from its linear2
bias still zero. Layer 0 then keeps c_t = c_{t-1} / 2 + tanh(s x_t) / 2 of each input column over the steps the net took on the row,
so `Net.get_state` shows prep (csrc/rc_frame_dev.h: prep_values / prep_store), fuse (csrc/rc_frame.hip: fuse_body; csrc/rc_live.hip:
rc_live_k4), the updater's inputs written by the tail, init_net's input and the rnn2 state written from its output, and the set of
rows on which rnn4 and rnn6 step. tests/test_wiring_bound_cpu.py shows on the CPU that the cases cover every situation and that each
one-line slip of `wiring_f64.MUTATIONS` lands at three times the Bound or more. Here each case runs, over its two calls, on
  every      forward_batch frame by frame, the states read after EVERY frame (the read flushes a pending updater step)
  stepped    forward_batch frame by frame, the states read after each call only (the deferral flags carry the pending step)
  seq0       forward_sequence, frame-stepped launches
  wave       forward_sequence with the wavefront engine forced (5 / 48 / 97 rows: the plain, split and tri engines; the second
             call's first tick carries the pending step of the first); sequence_stats shows that it ran
  ragged     forward_sequence(lengths=...): rows end at different frames of the last call, some with a step pending; each row is
             compared with the float64 state at its own last frame
  live       forward_live for the batches <= 4 (live_stats shows that lean frames ran)
in both GEMM modes, and
  * h and c of both layers of all six sub-nets are within the Bound of the float64 states in every element;
  * within one GEMM mode every non-live path read at a call's end is bitwise equal to `stepped`.
The resident kernel (batches from 160) is bitwise against the frame-stepped launches in tests/test_gpu_resident.py.
RC_WIRING_RATIOS_OUT=<file> keeps the worst ratio per (path, net).
"""
import os

import numpy as np
import pytest
import torch

from oracle import wiring_f64 as W

pytestmark = pytest.mark.gpu

WORST = {}                                     # (path, net) -> (ratio, case)


@pytest.fixture(scope="module")
def cases(synth_assets):
    return {c.name: c for c in W.build_cases(synth_assets["body"])}


@pytest.fixture(autouse=True)
def _reset_class_live():
    yield
    from robustcap_amd.net.sig_mp import Net
    Net.live = False


def make_net(body, built):
    from robustcap_amd.net.sig_mp import Net
    case = built.case
    Net.live = bool(case.prm.live)                                  # like the reference: read at construction (sig_mp.py:91-93)
    net = Net(body=body, batch=case.B)
    Net.live = False
    net.load_state_dict(built.sd)
    net.gravityc = case.gravity.clone()
    return net


def read(net):
    return {n: tuple(x.numpy().astype(np.float64) for x in net.get_state(n)) for n in W.NET_NAMES}


def run(net, case, path):
    """The case's two calls on one path from a fresh state. Returns [(last [B]: the frame each row's state belongs to, or -1 for
    a row that has not run; {net: (h, c)})], one entry per read."""
    B = case.B
    case.prm.poke_net(net)
    net.reset_states()
    reads, t = [], 0
    last = torch.full((B,), -1)
    for ci, (call, prm) in enumerate(zip(case.calls, W.call_params(case))):
        if call.reset:
            net.reset_states(case.reset_rows)
        prm.poke_net(net)
        ft = case.first_tran if call.first_tran else None
        sl = slice(t, t + call.T)
        if path in ("every", "stepped", "live"):
            for i in range(call.T):
                args = (case.j2dc[:, t + i], case.acc[:, t + i], case.oric[:, t + i], ft if i == 0 else None, call.first_frame and i == 0)
                net.forward_live(*args) if path == "live" else net.forward_batch(*args)
                if path == "every":
                    reads.append((torch.full((B,), t + i), read(net)))
            last = torch.full((B,), t + call.T - 1)
        else:
            lengths = None
            n = torch.full((B,), call.T)
            if path == "ragged" and ci == len(case.calls) - 1:      # rows end at different frames of the last call (from 1 to all)
                n = lengths = torch.tensor([1 + (5 * b) % call.T for b in range(B - 1)] + [call.T])
            net.forward_sequence(case.j2dc[:, sl], case.acc[:, sl], case.oric[:, sl], first_tran=ft, first_frame=call.first_frame, lengths=lengths)
            last = torch.where(n > 0, t + n - 1, last)
        if path != "every":
            reads.append((last.clone(), read(net)))
        t += call.T
    return reads


def worst_ratios(built, reads):
    """{net: worst |state - float64 state| / Bound over the reads}, each row against its own frame"""
    out = {n: 0.0 for n in W.NET_NAMES}
    for last, got in reads:
        for n in W.NET_NAMES:
            for k in (0, 1):
                for t in last.unique().tolist():
                    rows = (last == t).numpy()
                    r = np.abs(got[n][k][:, rows] - built.states[t][n][k][:, rows]) / built.tols[t][n][:, rows]
                    out[n] = max(out[n], float(np.where(np.isfinite(r), r, np.inf).max()))
    return out


@pytest.mark.parametrize("name", W.CASE_NAMES)
def test_states_within_the_bound_and_paths_equal(name, cases, synth_assets):
    case = cases[name]
    built = W.build(synth_assets["body"], case, evals=False)
    net = make_net(synth_assets["body"], built)
    outs = {}
    for split in (False, True):
        net.set_gemm_mode(split)
        tag = "split" if split else "fp32"
        net.set_sequence_mode(False)
        outs["stepped/" + tag] = run(net, case, "stepped")
        outs["every/" + tag] = run(net, case, "every")
        outs["seq0/" + tag] = run(net, case, "seq0")
        before = net.sequence_stats()
        net.set_sequence_mode(True, min_frames=8, force=True)
        outs["wave/" + tag] = run(net, case, "wave")
        after = net.sequence_stats()
        if case.prm.live:       # rc_sequence plans the wavefront engine only for a context that is not live
            assert after[0] == before[0], (name, "a live context left the frame-stepped launches", before, after)
        else:
            # (a call that starts a sequence -- first_tran or first_frame given -- runs its first frame on the frame-stepped launches)
            assert after[0] - before[0] >= case.T - len(case.calls), (name, "the wavefront engine did not run both calls", before, after)
        if case.B <= 4 and not split:                               # (the lean plan streams the fp32 weights)
            net.set_sequence_mode(False)
            lean0 = net.live_stats()[0]
            outs["live"] = run(net, case, "live")
            lean = net.live_stats()[0] - lean0
            assert lean >= case.T // 4, (name, "lean live frames", lean)
    # last: rows that end early leave the live refresh counters apart (they survive a reset), so a live context runs it once
    for split in ((False,) if case.prm.live else (False, True)):
        net.set_gemm_mode(split)
        net.set_sequence_mode(True, min_frames=8, force=True)
        outs["ragged/" + ("split" if split else "fp32")] = run(net, case, "ragged")

    failures = []
    ends = [sum(c.T for c in case.calls[:i + 1]) - 1 for i in range(len(case.calls))]
    for path, reads in outs.items():
        r = worst_ratios(built, reads)
        print(f"{name:12s} {path:14s} " + "  ".join(f"{n} {v:.3f}" for n, v in r.items()))
        for n, v in r.items():
            key = (path.split("/")[0], n)
            if key not in WORST or v > WORST[key][0]:
                WORST[key] = (v, name)
            if not v <= 1.0:
                failures.append((path, "outside the Bound", n, v))
        if path == "live" or path.startswith("stepped"):
            continue
        ref = outs["stepped/" + path.split("/")[1]]
        at_end = [rd for rd in reads if int(rd[0].max()) in ends] if path.startswith("every") else reads
        assert len(at_end) == len(ref)
        for (last, got), (last0, got0) in zip(at_end, ref):
            rows = (last == last0).numpy()                          # (a ragged row that ended early has no counterpart)
            for n in W.NET_NAMES:
                for k in (0, 1):
                    if not np.array_equal(got[n][k][:, rows], got0[n][k][:, rows]):
                        failures.append((path, "not bitwise equal to stepped", n, "hc"[k], int(last0.max()),
                                         float(np.abs(got[n][k][:, rows] - got0[n][k][:, rows]).max())))
    assert not failures, (name, failures)


def test_report_worst_ratios():
    """prints and keeps the worst error / Bound per (path, net) of the cases that ran before it"""
    if not WORST:                                                   # (selected on its own: nothing ran, nothing to report)
        print("no case of test_states_within_the_bound_and_paths_equal ran in this session")
        return
    lines = [f"device paths, M = {W.M:g}: worst error / Bound per (path, net)"]
    lines += [f"  {p:8s} {n:5s} {v:.3f}  ({c})" for (p, n), (v, c) in sorted(WORST.items())]
    for ln in lines:
        print(ln)
    out = os.environ.get("RC_WIRING_RATIOS_OUT")
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")
    assert max(v for v, _ in WORST.values()) <= 1.0
