"""Every branch of the frame tail (csrc/rc_frame_dev.h: tail_impl) against its float64 restatement, on every path that runs it.

The cases of oracle/tail_f64.py load a state dict whose every tensor is zero except the four linear2 biases: each sub-net's
output is its bias, exactly, so the tail's inputs are known and only the tail's own arithmetic is left. tests/test_tail_bound_cpu.py
shows on the CPU that these cases take every branch, that float32 and float64 take the same ones, and that every one-line slip of
`tail_f64.MUTATIONS` lands at three times the Bound or more. Here each case runs on
  stepped    forward_batch frame by frame (rc_tail_kernel<1>), the trace read after every frame
  seq0       forward_sequence, frame-stepped launches (sequence mode 0)
  wave       forward_sequence with the wavefront engine forced (rc_tail_kernel<4>; batches 5, 48, 97: a workgroup's last waves are
             past B), in both GEMM modes; a live context (reproj_live) never takes that engine and must stay frame-stepped
  ragged     forward_sequence(lengths=...) with rows ending at different frames of the second call
  live       forward_live for the batches <= 4: the lean frame's LIVE tail (live_stats shows that lean frames ran)
each over the case's two calls (first_tran / first_frame given or not, a masked reset and parameter pokes between them), and
  * tran and pose are within the Bound of the float64 restatement on every row and frame, in every group;
  * trace columns 0, 3-7 equal the restatement's record after every frame (stepped, live) / after each call (elsewhere),
    fusion_state columns 0-1 too;
  * all non-live paths and both GEMM modes are bitwise equal: with exact sub-net outputs no rounding is left that may differ.
RC_TAIL_RATIOS_OUT=<file> keeps the worst ratio per (path, group).
"""
import dataclasses
import os

import numpy as np
import pytest
import torch

from oracle import tail_f64 as F

pytestmark = pytest.mark.gpu

CASE_NAMES = tuple(s[0] for s in F._SPEC)
TRACE_COLS = (0, 3, 4, 5, 6, 7)
WORST = {}                                     # (path, "tran" | "pose") -> (ratio, case)


@pytest.fixture(scope="module")
def cases(synth_assets):
    return {c.name: c for c in F.build_cases(synth_assets["body"])}


@pytest.fixture(autouse=True)
def _reset_class_live():
    yield
    from robustcap_amd.net.sig_mp import Net
    Net.live = False


def make_net(body, case):
    from robustcap_amd.net.sig_mp import Net
    Net.live = bool(case.prm.live)                                  # like the reference: read at construction (sig_mp.py:91-93)
    net = Net(body=body, batch=case.B)
    Net.live = False
    net.load_state_dict(F.state_dict(case))
    net.gravityc = case.gravity.clone()
    return net


def want_trace(rec, t, rows=None):
    cols = [rec[k][:, t] for k in ("regime", "n_floor", "reach", "use_vel", "foot", "far")]
    w = torch.stack(cols, dim=1).to(torch.int32)
    return w if rows is None else w[rows]


def run(net, case, path, rec):
    """The case's two calls on one path from a fresh state. Returns (pose [B,T,24,3,3], tran [B,T,3], active [B,T]) on the CPU;
    asserts the trace (every frame where the path can read it, else after each call) and the fusion state."""
    B = case.B
    case.prm.poke_net(net)
    net.reset_states()
    pose, tran = torch.zeros(B, case.T, 24, 3, 3), torch.zeros(B, case.T, 3)
    active = torch.ones(B, case.T, dtype=torch.bool)
    last = torch.full((B,), -1)                                     # last frame each row ran
    t = 0
    for ci, call in enumerate(case.calls):
        if call.reset:
            net.reset_states(case.reset_rows)
        if call.poke:
            dataclasses.replace(case.prm, **call.poke).poke_net(net)
        ft = case.first_tran if call.first_tran else None
        sl = slice(t, t + call.T)
        if path in ("stepped", "live"):
            for i in range(call.T):
                args = (case.j2dc[:, t + i], torch.zeros(B, 6, 3), case.oric[:, t + i], ft if i == 0 else None, call.first_frame and i == 0)
                p, x = net.forward_live(*args) if path == "live" else net.forward_batch(*args)
                pose[:, t + i], tran[:, t + i] = p.cpu(), x.cpu()
                got = net.get_trace()[:, TRACE_COLS]
                assert torch.equal(got, want_trace(rec, t + i)), (case.name, path, t + i, got.tolist(), want_trace(rec, t + i).tolist())
            last[:] = t + call.T - 1
        else:
            lengths = None
            if path == "ragged" and ci == len(case.calls) - 1:      # rows end at different frames of the last call (from 1 to all)
                lengths = torch.tensor([1 + (5 * b) % call.T for b in range(B - 1)] + [call.T])
                active[:, sl] = torch.arange(call.T)[None, :] < lengths[:, None]
            acc = torch.zeros(B, call.T, 6, 3)
            p, x = net.forward_sequence(case.j2dc[:, sl], acc, case.oric[:, sl], first_tran=ft, first_frame=call.first_frame, lengths=lengths)
            pose[:, sl], tran[:, sl] = p.cpu(), x.cpu()
            last = torch.where(active[:, sl].any(dim=1), t + active[:, sl].long().sum(dim=1) - 1, last)
            got = net.get_trace()[:, TRACE_COLS]
            want = torch.stack([want_trace(rec, int(last[b]))[b] for b in range(B)])
            assert torch.equal(got, want), (case.name, path, "call", ci, got.tolist(), want.tolist())
        t += call.T
    fs = net.fusion_state()
    assert fs[:, 0].tolist() == [1] * B, (case.name, path)
    assert fs[:, 1].tolist() == [int(rec["n_floor"][b, int(last[b])]) for b in range(B)], (case.name, path)
    return pose, tran, active


@pytest.mark.parametrize("name", CASE_NAMES)
def test_tail_paths_within_the_bound_and_equal(name, cases, synth_assets):
    case = cases[name]
    sim, bound, r32, _ = F.bound_of(synth_assets["body"], case)
    F.conditions(synth_assets["body"], case, sim)
    rec = sim["rec"]
    net = make_net(synth_assets["body"], case)
    outs = {}
    for split in (False, True):
        net.set_gemm_mode(split)
        tag = "split" if split else "fp32"
        net.set_sequence_mode(False)
        outs["stepped/" + tag] = run(net, case, "stepped", rec)
        outs["seq0/" + tag] = run(net, case, "seq0", rec)
        before = net.sequence_stats()
        net.set_sequence_mode(True, min_frames=8, force=True)
        outs["wave/" + tag] = run(net, case, "wave", rec)
        after = net.sequence_stats()
        if case.prm.live:       # rc_sequence plans the wavefront engine only for a context that is not live: these frames stay stepped
            assert after[0] == before[0] and after[1] - before[1] == case.T, (name, "a live context left the frame-stepped launches", before, after)
        else:
            assert after[0] - before[0] > 0, (name, "the wavefront engine did not run", before, after)
    if case.B <= 4:
        net.set_gemm_mode(False)                                    # (the lean plan streams the fp32 weights)
        lean0 = net.live_stats()[0]
        outs["live"] = run(net, case, "live", rec)
        lean = net.live_stats()[0] - lean0
        assert lean >= case.T // 4, (name, "lean live frames", lean)
    net.set_gemm_mode(False)
    net.set_sequence_mode(True, min_frames=8, force=True)
    outs["ragged/fp32"] = run(net, case, "ragged", rec)             # last: rows that end early leave the live refresh counters apart
    assert not bool(outs["ragged/fp32"][2].all()) and bool(outs["ragged/fp32"][2][:, -1].any())

    failures = []
    ref_pose, ref_tran, _ = outs["stepped/fp32"]
    for path, (pose, tran, active) in outs.items():
        r = bound.ratios(pose, tran, active)
        print(f"{name:12s} {path:14s} tran {r[0]:.3f}  pose {r[1:].max():.3f} ({F.GROUP_NAMES[1 + int(r[1:].argmax())]})")
        for group, v in (("tran", float(r[0])), ("pose", float(r[1:].max()))):
            key = (path.split("/")[0], group)
            if key not in WORST or v > WORST[key][0]:
                WORST[key] = (v, name)
        if not float(r.max()) <= 1.0:
            failures.append((path, "outside the Bound", F.GROUP_NAMES[int(r.argmax())], float(r.max())))
        if path != "live":
            a3, a5 = active.view(*active.shape, 1), active.view(*active.shape, 1, 1, 1)
            same = torch.equal(torch.where(a3, tran, ref_tran), ref_tran) and torch.equal(torch.where(a5, pose, ref_pose), ref_pose)
            if not same:
                failures.append((path, "not bitwise equal to stepped/fp32", float((tran - ref_tran).abs()[active].max()),
                                 float((pose - ref_pose).abs()[active].max())))
    assert not failures, (name, failures)


def test_report_worst_ratios():
    """prints and keeps the worst error / Bound per (path, group) of the cases that ran before it"""
    if not WORST:                                                   # (selected on its own: nothing ran, nothing to report)
        print("no case of test_tail_paths_within_the_bound_and_equal ran in this session")
        return
    lines = [f"device paths, M = {F.M:g}: worst error / Bound per (path, group)"]
    lines += [f"  {p:8s} {g:5s} {v:.3f}  ({c})" for (p, g), (v, c) in sorted(WORST.items())]
    for ln in lines:
        print(ln)
    out = os.environ.get("RC_TAIL_RATIOS_OUT")
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")
    assert max(v for v, _ in WORST.values()) <= 1.0
