"""The float64 restatement of the frame tail takes every branch, and its Bound has teeth (CPU only).

tests/test_gpu_tail_branches.py holds `tail_impl` (rc_tail_kernel<1>, rc_tail_kernel<4>, the lean live frame) to the Bound of
oracle/tail_f64.py on cases whose sub-net outputs are exact (zero weights: each output is its linear2 bias). Here the same
cases and the same Bound are applied to CPU evaluations:
  * every comparison of every row and frame keeps its float64 margin (`conditions`), nothing excluded;
  * a census: every value of every branch is taken at least 20 times, every (contact situation x regime) pair at least once;
  * the float32 OracleNet on each case's zero-weight state dict and the float32 tail in two association orders stay at or below
    a third of the Bound in every group, and the oracle's own branch record equals the restatement's on every frame;
  * every mutation of `tail_f64.MUTATIONS` reaches three times the Bound or more in a group of a case built for it.
So a tail with one of those slips could not pass the GPU test. RC_TAIL_RATIOS_OUT=<file> keeps the printed tables.
"""
import os

import numpy as np
import pytest
import torch

from oracle import sig_mp_oracle as O
from oracle import tail_f64 as F

CENSUS_MIN = 20


@pytest.fixture(scope="module")
def body(synth_assets):
    return synth_assets["body"]


@pytest.fixture(scope="module")
def cases(body):
    return F.build_cases(body)


@pytest.fixture(scope="module")
def bounds(body, cases):
    return {c.name: F.bound_of(body, c) for c in cases}


def _emit(lines):
    for ln in lines:
        print(ln)
    path = os.environ.get("RC_TAIL_RATIOS_OUT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


def test_conditions_hold_on_every_row_and_frame(body, cases, bounds):
    assert len(cases) == 14 and {c.situation for c in cases} == set(F.SITUATIONS)
    assert sorted({c.B for c in cases}) == [3, 4, 5, 48, 97]
    lines = [f"conditions: smallest margin / ({F.COND_FACTOR:g} x M eps32 A) per comparison (contact: / {F.CONTACT_KEEP:g})"]
    for c in cases:
        cond = F.conditions(body, c, bounds[c.name][0])             # asserts > 1 on every checked row and frame
        lines.append(f"{c.name:12s} B={c.B:3d} " + "  ".join(f"{k}: {v:.3g}" for k, v in cond.items()))
        # the margins also exceed the Bound as measured (its e32 part included) of the translation they compare
        sim, b = bounds[c.name][0], bounds[c.name][1]
        for name, margin, A, checked in sim["margins"]:
            if name.startswith("|") and bool(checked.any()):
                assert bool((margin > b.tol_tran)[checked].all()), (c.name, name)
    _emit(lines)
    assert any(c.prm.use_reproj_opt and c.prm.live and c.prm.update_vision_freq > 1 for c in cases)
    assert any(c.prm.use_reproj_opt and not c.prm.live for c in cases) and any(not c.prm.use_flat_floor for c in cases)
    assert any(float(c.bias["r6d"].view(24, 6)[:, :3].abs().sum(1).min()) == 0.0 for c in cases)      # NaN -> 0
    assert any(c.prm.tran_filter_num > 1 for c in cases)


def test_census_every_branch_taken(cases, bounds):
    want = dict(regime=(0, 1, 2), use_vel=(0, 1), foot=(0, 1), far=(0, 1), appended=(0, 1), corr=(0, 1, 2, 3), refresh=(0, 1))
    count = {(k, v): 0 for k, vs in want.items() for v in vs}
    pairs = set()
    first = {k: 0 for k in ("first row-frame, first_tran", "first row-frame, first_frame", "first row-frame, neither", "first row-frame after a masked reset",
                            "floor reaches 11 samples", "correction right after the 11th sample")}
    for c in cases:
        rec = bounds[c.name][0]["rec"]
        for (k, v) in count:
            count[(k, v)] += int((rec[k] == v).sum())
        pairs |= {(c.situation, int(r)) for r in rec["regime"].unique()}
        t = 0
        for i, call in enumerate(c.calls):
            fresh = torch.ones(c.B, dtype=torch.bool) if i == 0 else (c.reset_rows if call.reset else torch.zeros(c.B, dtype=torch.bool))
            n = int(fresh.sum())
            key = "first_tran" if call.first_tran else ("first_frame" if call.first_frame else "neither")
            first["first row-frame, " + key] += n
            if i > 0:
                first["first row-frame after a masked reset"] += n
            assert bool((rec["use_vel"][fresh, t] == 1).all())                      # no last translation: the velocity branch
            t += call.T
        full = (rec["n_floor"] == 11) & (rec["appended"] == 1)
        first["floor reaches 11 samples"] += int(full.sum())
        first["correction right after the 11th sample"] += int((full & (rec["corr"] > 0)).sum())
    lines = ["census of the float64 restatement over the cases (row-frames):"]
    for k, vs in want.items():
        names = F.CORR if k == "corr" else vs
        lines.append(f"  {k:9s} " + "  ".join(f"{n}: {count[(k, v)]}" for n, v in zip(names, vs)))
    lines += [f"  {k}: {v}" for k, v in first.items()]
    lines.append("  (contact situation x regime) pairs taken: " + ", ".join(f"{s}/{r}" for s, r in sorted(pairs)))
    _emit(lines)
    assert all(n >= CENSUS_MIN for n in count.values()), count
    assert all(n >= CENSUS_MIN for n in first.values()), first
    assert pairs == {(s, r) for s in F.SITUATIONS for r in (0, 1, 2)}


def test_float32_evaluations_within_a_third_and_oracle_branches_equal(cases, bounds):
    lines = [f"M = {F.M:g}   (Bound = M max(e32, eps32 A); float32 evaluations: tail_step {', '.join(F.ORDERS)}, OracleNet)",
             f"{'case':12s} " + " ".join(f"{k:>9s}" for k in (*F.ORDERS, "oracle")) + "   worst group   e32 tran max   eps32 A tran min..max"]
    for c in cases:
        sim, b, r32, e32 = bounds[c.name]
        worst = {k: float(r.max()) for k, r in r32.items()}
        k = max(r32, key=lambda k: worst[k])
        lines.append(f"{c.name:12s} " + " ".join(f"{worst[o]:9.3f}" for o in (*F.ORDERS, "oracle")) + f"   {F.GROUP_NAMES[int(r32[k].argmax())]:11s}   "
                     f"{float(b.e32_tran.max()):.2e}       {F.EPS32 * float(sim['A'].min()):.1e}..{F.EPS32 * float(sim['A'].max()):.1e}")
        assert max(worst.values()) <= 1.0 / F.MARGIN, (c.name, worst)
        rec, orec = sim["rec"], e32["oracle"]["rec"]
        assert torch.equal(orec["use_vel"], rec["use_vel"]) and torch.equal(orec["foot"], rec["foot"]), c.name
        assert torch.equal(orec["far"], rec["far"]) and torch.equal(orec["n_floor_add"], rec["appended"]), c.name
        assert torch.equal(orec["n_floor"], rec["n_floor"]) and torch.equal(orec["reach"], rec["reach"]), c.name
        for o in F.ORDERS:                                          # float32 takes float64's branches, as `conditions` promises
            for key in ("regime", "use_vel", "far", "appended", "corr", "refresh", "n_floor"):
                assert torch.equal(e32[o]["rec"][key], rec[key]), (c.name, o, key)
    _emit(lines)


def test_every_mutation_beyond_three_times_the_bound(body, cases, bounds):
    ob = O.OracleBody(body, dtype=F.F64)
    best = {}
    for name, kinds in F.MUTATIONS.items():
        for c in cases:
            if c.kind in kinds:
                mut = F.simulate(ob, c, mut=name)
                r = bounds[c.name][1].ratios(mut["pose"], mut["tran"])
                if name not in best or float(r.max()) > best[name][0]:
                    best[name] = (float(r.max()), c.name, F.GROUP_NAMES[int(r.argmax())])
    lines = [f"{'mutation':52s} {'case':12s} {'group':8s} error/Bound"]
    lines += [f"{name:52s} {best[name][1]:12s} {best[name][2]:8s} {best[name][0]:.3g}" for name in F.MUTATIONS]
    _emit(lines)
    assert len(F.MUTATIONS) == 18
    for name in F.MUTATIONS:
        assert best[name][0] >= F.MARGIN, (name, best[name])
