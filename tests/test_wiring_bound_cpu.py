"""What the sub-nets are fed and when they step: the float64 restatement covers every situation, and its Bound has teeth (CPU only).

tests/test_gpu_wiring.py reads the LSTM states of all six sub-nets off the device (`Net.get_state`) on cases whose state dict is
tail_f64's plus a WIRE (oracle/wiring_f64.py): layer 0 of every sub-net keeps c_t = c_{t-1} / 2 + tanh(s x) / 2 of each input column,
so its state is a geometric memory of every step taken and of every value fed -- prep, fuse, the updater's inputs, init_net's input
and the step set of rnn4 / rnn6 all become visible. Here the same cases and the same Bound are applied to CPU evaluations:
  * tail_f64's `conditions` still hold on the altered cases, the scale condition s |x| <= 1 holds on every column, row and step,
    and the float32 OracleNet on the wired dict returns the pose and translation of tail_f64's zero-weight dict bit for bit;
  * a census: every regime, a first_frame in regime 0, the updater taken / withheld by the live refresh counter, a pending step
    before a visible / an occluded frame on at least 20 row-frames; a pending step at the end of the first call on rows that go on
    / that the masked reset clears, a reach, a reach re-armed by the reset on at least 5 rows;
  * the float32 OracleNet and the float32 restatement in two association orders stay at or below a third of the Bound in every
    state element after every frame;
  * every mutation of `wiring_f64.MUTATIONS` reaches three times the Bound or more on the case named beside it.
Honest limit: a slip of an ulp in one input -- w1 = 1 - (float)k for (float)(1 - k) in the lerp, say -- is below this test's
resolution: the state's own bound starts at 1.5e-6 (lstm_f64.HC_ABS) and an input's at 4 eps32 of its magnitude. The Bound is not
tightened to catch it. RC_WIRING_RATIOS_OUT=<file> keeps the printed tables.
"""
import os

import pytest
import torch

from oracle import tail_f64 as F
from oracle import wiring_f64 as W

CENSUS_FRAMES_MIN, CENSUS_ROWS_MIN = 20, 5
REQUIRED = ("foot0", "foot1", "tie", "hi_lo", "lo_hi", "reproj", "reproj_live")


@pytest.fixture(scope="module")
def body(synth_assets):
    return synth_assets["body"]


@pytest.fixture(scope="module")
def built(body):
    return {c.name: W.build(body, c) for c in W.build_cases(body)}


def _emit(lines):
    for ln in lines:
        print(ln)
    path = os.environ.get("RC_WIRING_RATIOS_OUT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


def test_cases_keep_the_tail_and_the_scale_condition(body, built):
    assert set(REQUIRED) <= set(built) and {built[n].case.B for n in REQUIRED} >= {3, 4, 5, 48, 97}
    prms = {n: W.call_params(b.case) for n, b in built.items()}
    assert any(p[0].use_vision_updater and not p[1].use_vision_updater for p in prms.values())
    assert any(not p[0].use_imu_updater for p in prms.values())
    lines = ["scale condition: largest s |x| per net over every column, row and step (<= 1); the wire's s per column group"]
    for name, b in built.items():
        F.conditions(body, b.case, b.sim)                           # asserts every margin on every row and frame
        assert max(b.scale_worst.values()) <= 1.0, (name, b.scale_worst)
        groups = "  ".join(f"{n}: " + ",".join(f"{b.sc[n][a]:g}" for _, a, _ in W.GROUPS[n]) for n in W.NET_NAMES)
        lines.append(f"{name:12s} B={b.case.B:3d} worst {max(b.scale_worst.values()):.3f}   s  {groups}")
        if name in ("foot0", "lo_hi", "reproj_live", "lo_edge"):    # the wire, the generic IMUs 0-4 and the accelerations change nothing the tail computes
            ref = F.oracle_run(body, b.case)
            assert torch.equal(ref["pose"], b.oracle_pose) and torch.equal(ref["tran"], b.oracle_tran), name
        c = b.case                                                  # generic inputs where tail_f64 has the identity and zero
        eye = torch.eye(3).expand(c.B, c.T, 5, 3, 3)
        assert float((c.oric[:, :, :5] - eye).abs().amax(dim=(3, 4)).min()) > 1e-3 and float(c.acc.abs().amax(dim=3).min()) > 1e-3, name
        assert float(c.acc.abs().max()) <= 4.0
    _emit(lines)


def test_census_every_situation_occurs(built):
    total = {}
    for b in built.values():
        for k, v in W.census(b).items():
            total[k] = total.get(k, 0) + v
    lines = ["census of the float64 restatement over the cases:"]
    lines += [f"  {total[k]:6d} row-frames  {k}" for k in W.CENSUS_FRAMES] + [f"  {total[k]:6d} rows        {k}" for k in W.CENSUS_ROWS]
    _emit(lines)
    assert all(total[k] >= CENSUS_FRAMES_MIN for k in W.CENSUS_FRAMES), total
    assert all(total[k] >= CENSUS_ROWS_MIN for k in W.CENSUS_ROWS), total


def test_float32_evaluations_within_a_third(built):
    evs = (*W.ORDERS, "oracle")
    lines = [f"M = {W.M:g}   float32 evaluations (restatement {', '.join(W.ORDERS)}; OracleNet): worst error / Bound over every state element and frame",
             f"{'case':12s} " + " ".join(f"{e:>9s}" for e in evs) + "   worst net"]
    for name, b in built.items():
        worst = {e: max(b.r32[e].values()) for e in evs}
        e = max(worst, key=worst.get)
        lines.append(f"{name:12s} " + " ".join(f"{worst[k]:9.3f}" for k in evs) + f"   {max(b.r32[e], key=b.r32[e].get)}")
        assert max(worst.values()) <= 1.0 / W.MARGIN, (name, b.r32)
    _emit(lines)


def test_every_mutation_beyond_three_times_the_bound(built):
    assert len(W.MUTATIONS) == 22
    lines = [f"{'mutation':54s} {'case':12s} {'net':5s} error/Bound"]
    found = {}
    for mut, name in W.MUTATIONS.items():
        b = built[name]
        frames = W._masked(W.restate(b.case, b.sim, mut=mut))
        r = W.ratios(W.run_states(b.case, b.params, frames, mut=mut), b.states, b.tols)
        net = max(r, key=r.get)
        found[mut] = r[net]
        lines.append(f"{mut:54s} {name:12s} {net:5s} {r[net]:.3g}")
    _emit(lines)
    for mut, v in found.items():
        assert v >= W.MARGIN, (mut, v)
