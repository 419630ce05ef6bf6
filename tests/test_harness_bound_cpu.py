"""The bounds of the evaluation harness's camera-frame inputs are neither too loose nor too tight, shown without a GPU.

tests/test_gpu_harness_inputs.py holds rc_camera_inputs_kernel, rc_camera_inputs_rows_kernel, camera_constants and the host
routines `labels` / `first_translations` to the bounds of oracle/harness_f64.py. Here the same cases and bounds meet CPU evaluations:
  * `Ops` in float64 restates `restate` (the two agree to 1e-6 of the Bound), so its float32 evaluations and its mutations are
    evaluations and mutations of the reference's formulas;
  * eight honest float32 evaluations (each sum of products first-term-first or last-term-first, separate or fused multiply-adds,
    K^-1 by the float64 adjugate rounded once or by torch's float32 inverse), oracle/harness_oracle.py -- which this pins -- and the
    float32 torch expressions of evaluate.labels / first_translations stay at or below a third of the Bound on every case;
  * every single mutation of the list lands at or beyond three times the Bound on the case named beside it, and a transposition is
    invisible on the symmetric 180-degree camera, which is why that camera is not the only rotated one;
  * the case builder holds what it promises.
`first_translations == labels(...)[1][0]` bit for bit stands in the GPU file: `labels` builds its rotation matrices with the HIP
axis-angle kernel and cannot run here. RC_HARNESS_RATIOS_OUT=<file> keeps the printed tables.
"""
import os

import numpy as np
import pytest
import torch

from oracle import harness_f64 as Hf
from oracle import harness_oracle as HO


def _emit(lines):
    for ln in lines:
        print(ln)
    path = os.environ.get("RC_HARNESS_RATIOS_OUT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture(scope="module")
def suite():
    """[(case, reference)] computed once"""
    return [(c, Hf.reference(c)) for c in Hf.cases()]


def test_ops_in_float64_restate_the_restatement(suite):
    for c, ref in suite:
        for op, v in Hf.all_ratios(c, Hf.Ops(Hf.Ar(Hf.F64)).run(c), ref).items():
            assert v <= 1e-6, (c.name, op, v)                                  # 1e-6 of a Bound of a few eps32: 1e-13 relative


def _oracle_outputs(c):
    """oracle/harness_oracle.py and the library's host torch expressions (evaluate.labels / first_translations) on case `c`"""
    j, a, o, g = HO.camera_inputs(c.kp, c.acc, c.ori, c.K, c.Tcw, image_size=c.size)
    Tcw = torch.from_numpy(c.Tcw)
    tran = torch.from_numpy(c.tran) @ Tcw[:3, :3].T + Tcw[:3, 3]                # evaluate.labels, first_translations
    assert torch.equal(HO.first_translation(c.tran, c.Tcw), tran[0])
    return {"j2dc": j[..., :2], "conf": j[..., 2], "accc": a, "oric": o, "gravityc": g, "tran": tran, "root": Tcw[:3, :3] @ torch.from_numpy(c.root)}


def test_float32_evaluations_stay_within_a_third_of_the_bound(suite):
    worst, route = Hf.Worst(), Hf.Worst()
    for c, ref in suite:
        for ar, inv in Hf.VARIANTS:
            worst.note(Hf.all_ratios(c, Hf.Ops(ar, inv=inv).run(c), ref), c.name)
        route.note({"j2dc": float(ref["j2dc"][2].max())}, c.name)
    _emit(worst.lines(f"CPU, honest float32 evaluations ({len(Hf.VARIANTS)} per op): worst error / Bound per op (<= 1/{Hf.MARGIN:g} required)"))
    lines = ["CPU, the reference's float32 K.inverse() route against float64: worst e32 / (eps32 A) of j2dc"]
    for word in ("skew 3.5", "general K", ""):
        v, nm = max((float(ref["j2dc"][2].max()), c.name) for c, ref in suite if word in c.name)
        lines.append(f"  {word or 'all cases':12s} {v:.3f}  ({nm})")
    _emit(lines)
    assert set(worst.w) == set(Hf.M_OF) | {"conf"}
    for op, (v, nm) in worst.w.items():
        assert v <= 1.0 / Hf.MARGIN, (op, nm, v)


def test_harness_oracle_and_host_torch_stay_within_a_third_of_the_bound(suite):
    worst = Hf.Worst()
    for c, ref in suite:
        worst.note(Hf.all_ratios(c, _oracle_outputs(c), ref), c.name)
    _emit(worst.lines(f"CPU, oracle/harness_oracle.camera_inputs and the host torch of evaluate.labels: worst error / Bound (<= 1/{Hf.MARGIN:g} required)"))
    for op, (v, nm) in worst.w.items():
        assert v <= 1.0 / Hf.MARGIN, (op, nm, v)


def test_every_mutation_lands_beyond_three_times_the_bound(suite):
    lines = [f"mutations: error / Bound on the case named (>= {Hf.MARGIN:g} required); [cases of the suite that show it]"]
    smallest = {}
    for mut, (op, word) in Hf.MUTATIONS.items():
        per_case = {c.name: Hf.all_ratios(c, Hf.Ops(Hf.Ar(Hf.F64), mut=mut).run(c), ref) for c, ref in suite}
        for nm, r in per_case.items():                                        # a mutation moves its own op and no other
            assert all(v <= 1e-6 for o, v in r.items() if o != op), (mut, nm, r)
        named = [nm for nm in per_case if word in nm]
        assert named, (mut, word)
        best = max(per_case[nm][op] for nm in named)
        shown = sum(r[op] >= Hf.MARGIN for r in per_case.values())
        lines.append(f"  {mut:24s} {best:12.3g}  {op:9s} {word}  [{shown} of {len(suite)}]")
        smallest[op] = min(smallest.get(op, float("inf")), best)
        assert best >= Hf.MARGIN, f"{mut} stays below {Hf.MARGIN:g} Bound on '{word}' ({best:.3g}); it shows on {shown} cases of the suite"
    lines.append("  smallest per op: " + ", ".join(f"{op} {v:.3g}" for op, v in sorted(smallest.items())))
    for mut, word in Hf.INVISIBLE:
        op = Hf.MUTATIONS[mut][0]
        for c, ref in suite:
            if word in c.name:
                assert Hf.all_ratios(c, Hf.Ops(Hf.Ar(Hf.F64), mut=mut).run(c), ref)[op] <= 1e-6, (mut, c.name)
        lines.append(f"  {mut:24s} invisible on '{word}'")
    _emit(lines)
    assert len(Hf.MUTATIONS) == 13


def test_the_case_builder_holds_its_conditions(suite):
    cs = [c for c, _ in suite]
    names = [c.name for c in cs]
    assert len(set(names)) == len(names) == 11 + 3 * 4
    for c in cs:
        assert c.kp.shape == (Hf.T_FRAMES, 33, 3) and c.kp.dtype == np.float32 and np.isfinite(c.kp).all()
        assert [tuple(p) for p in c.kp[0, :6, :2]] == [tuple(np.float32(p)) for p in Hf.KP_EDGES]
        assert c.kp[0, :5, 2].tobytes() == np.asarray(Hf.CONF_EDGES, np.float32).tobytes()          # bitwise: -0.0 and the denormal
        assert np.signbit(c.kp[0, 2, 2]) and 0 < c.kp[0, 3, 2] < np.finfo(np.float32).tiny and c.kp[-1, 32, 2] == c.kp[0, 3, 2]
        inside = np.delete(c.kp.reshape(-1, 3), [4, 5], axis=0)[:, :2]
        assert inside.min() >= 0 and inside.max() <= 1
        n = np.linalg.norm(c.acc.astype(np.float64), axis=-1)
        assert n[0, 0] == 0 and abs(n[0, 1] - 9.8) < 1e-5 and abs(n[0, 2] - 1e3) < 1e-3 and abs(n[1, 5] - 1e3) < 1e-3
        ref, A = Hf.restate(c), Hf.magnitudes(c)
        for f, i, r in ((0, 3, 0), (1, 5, 2)):                                  # the result cancels to rounding; A does not where
            assert abs(float(ref["accc"][f, i, r])) <= 4 * Hf.EPS32 * float(A["accc"][f, i, r])         # R_cw is far from the axes
            assert float(A["accc"][f, i, r]) > 5.0 or not ("2 rad" in c.name or "180 deg" in c.name)
        assert np.array_equal(c.ori[0, 0], np.eye(3, dtype=np.float32))
        gram = c.ori.astype(np.float64) @ c.ori.astype(np.float64).transpose(0, 1, 3, 2)
        off = np.abs(gram - np.eye(3)).reshape(Hf.T_FRAMES, 6, 9).max(-1)
        assert off[1, 5] > 0.5 and np.delete(off.reshape(-1), 11).max() < 1e-6  # one non-orthonormal matrix, the rest rotations
        assert abs(np.linalg.det(c.K.astype(np.float64))) > 1e5
    by = lambda w: [c for c in cs if w in c.name]
    assert sorted({c.size for c in cs}) == sorted(Hf.SIZES) and all(len(by(f"{w}x{h}")) >= 4 for w, h in Hf.SIZES[1:])
    R = lambda c: c.Tcw[:3, :3].astype(np.float64)
    for w in ("90 deg about x", "90 deg about y", "90 deg about z"):
        (c,) = by(w)
        assert set(np.abs(R(c)).reshape(-1)) == {0.0, 1.0} and np.linalg.det(R(c)) == 1.0 and not np.array_equal(R(c), R(c).T)
    (c,) = by("2 rad")
    assert np.abs(R(c) - R(c).T)[np.triu_indices(3, 1)].min() > 0.4 and np.abs(R(c) @ R(c).T - np.eye(3)).max() < 1e-6
    assert abs(np.arccos((np.trace(R(c)) - 1) / 2) - 2.0) < 1e-6
    (c,) = by("180 deg")
    assert np.array_equal(R(c), R(c).T) and abs(np.trace(R(c)) + 1.0) < 1e-6
    assert np.abs(R(by("synthetic camera 1920")[0]) - np.eye(3)).max() < 0.26
    assert all(c.K[0, 1] == 3.5 for c in by("skew")) and by("fx 1400")[0].K[0, 0] == 1400 and by("fx 1400")[0].K[1, 1] == 900
    assert tuple(by("principal point")[0].K[:2, 2]) == (300.0, 900.0) and all(c.K[2, 2] == 2 for c in by("K22"))
    assert all(tuple(c.K[2]) == (np.float32(1e-4), 0.0, 1.0) and c.K[1, 0] != 0 for c in by("general K"))
    n = Hf.nan_case()
    assert int(np.isnan(n.kp).sum()) == 1 and np.isnan(n.kp[1, 7, 0])
