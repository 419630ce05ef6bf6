"""art.FullMotionEvaluator without a GPU: the float64 restatement tests/motion_metrics_f64.py against the reference's own output
(tests/golden/motion/motion_metrics.npz, written by tools/capture_motion_metrics.py), and the deliberate mistakes the bound must catch.

  fixture    every entry of the nine captured [11,2] results (near / far / same x fps=60 | fps=5 with a mask | align_joint=5) within
             Bound = 8 |float32 transcription - restatement| + 1e-7 scale of the restatement; NaNs where the fixture has them; the
             fixture's sha256 equals its meta.json. The angle rows pin the wiring only (the capture ran a numpy rotation -> axis-angle in
             place of cv2.Rodrigues, which is not installed where the fixture is written).
  mistakes   biased std, std over all elements, a stencil across a group boundary, a window of fps +- 1, the offset's sign, ve without the
             offset, jerk without the translation: each moves its named output by more than the bound.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import motion_metrics_f64 as M


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "motion", "motion_metrics.npz"))


@pytest.fixture(scope="module")
def motions(golden_dir, fixture):
    g = np.load(os.path.join(golden_dir, "metrics.npz"))
    gt = g["pose_gt"]
    tp, tt = fixture["tran_p"], fixture["tran_t"]
    return {"near": (g["pose_near"], gt, tp, tt), "far": (g["pose_far"], gt, tp, tt), "same": (gt, gt, tt, tt)}


def test_fixture_hash_matches_its_meta(golden_dir):
    d = os.path.join(golden_dir, "motion")
    meta = json.load(open(os.path.join(d, "meta.json")))
    assert list(meta["sha256"]) == ["motion_metrics.npz"]
    assert hashlib.sha256(open(os.path.join(d, "motion_metrics.npz"), "rb").read()).hexdigest() == meta["sha256"]["motion_metrics.npz"]


def test_fixture_translations_are_the_seeded_ones(fixture):
    tp, tt = M.golden_translations(24)
    assert np.array_equal(fixture["tran_p"], tp) and np.array_equal(fixture["tran_t"], tt)


@pytest.mark.parametrize("setting", list(M.GOLDEN_SETTINGS))
@pytest.mark.parametrize("motion", M.GOLDEN_MOTIONS)
def test_restatement_matches_the_reference_capture(setting, motion, fixture, motions, synth_assets):
    body = synth_assets["body"]
    fps, mask, align = M.GOLDEN_SETTINGS[setting]
    pp, pt, tp, tt = motions[motion]
    f64, _, scale = M.evaluate(body, pp, pt, tp, tt, fps, align, mask)
    f32 = M.evaluate(body, pp, pt, tp, tt, fps, align, mask, dtype=M.F32)[0]
    ref = fixture[f"out_{setting}_{motion}"]
    assert np.array_equal(np.isnan(f32), np.isnan(f64))
    r = M.ratios(ref, f64, M.bound(f32, f64, scale))                      # asserts the NaN placement
    for k, name in enumerate(M.ROWS):
        print(f"{setting:10s} {motion:5s} {name:5s} mean {f64[k, 0]:12.5e} std {f64[k, 1]:12.5e}  |ref - f64| / Bound {r[k, 0]:.3f} {r[k, 1]:.3f}")
    assert (r <= 1.0).all(), (setting, motion, r)
    # where the reference has NaN: the te row of 24 frames at fps 60 (no window exists), the std of torch.zeros(1) without a mask
    assert np.isnan(ref[6]).all() == (fps >= 24)
    assert (mask is None) == bool(np.isnan(ref[7:10, 1]).all()) and (ref[7:10, 0] == 0).all() == (mask is None or motion == "same")
    if motion == "same":
        assert (f64[[0, 1, 7, 10]][np.isfinite(f64[[0, 1, 7, 10]])] == 0).all() and np.array_equal(f64[4], f64[5])


def test_degenerate_lengths_give_torch_nans(synth_assets):
    body = synth_assets["body"]
    for N, fps in ((1, 60), (3, 60), (4, 60), (5, 5), (6, 5)):
        pp, pt, tp, tt = M.motion_pair(70 + N, N)
        out = M.evaluate(body, pp, pt, tp, tt, fps, 0, [3])[0]
        assert np.isnan(out[[0, 1, 2, 3, 7, 8, 9, 10], 1]).all() == (N == 1) and np.isfinite(out[[0, 1, 2, 3, 7, 8, 9, 10], 0]).all()
        assert np.isnan(out[4:6, 0]).all() == (N <= 3) and np.isnan(out[4:6, 1]).all() == (N <= 4)
        assert np.isnan(out[6, 0]) == (N <= fps) and np.isnan(out[6, 1]) == (N <= fps + 1)


@pytest.mark.parametrize("mut", list(M.MUTATIONS))
def test_deliberate_mistakes_leave_the_bound(mut, motions, synth_assets):
    body = synth_assets["body"]
    fps, mask, align = M.GOLDEN_SETTINGS["fps5_mask"]
    pp, pt, tp, tt = motions["near"]
    f64, _, scale = M.evaluate(body, pp, pt, tp, tt, fps, align, mask)
    f32 = M.evaluate(body, pp, pt, tp, tt, fps, align, mask, dtype=M.F32)[0]
    bad = M.evaluate(body, pp, pt, tp, tt, fps, align, mask, mut=mut)[0]
    row, col = M.MUTATIONS[mut]
    k = M.ROWS.index(row)
    B = M.bound(f32, f64, scale)
    ratio = abs(bad[k, col] - f64[k, col]) / B[k, col]
    print(f"{mut:18s} moves {row}[{col}] by {ratio:.3e} Bound")
    assert ratio > 1.0, (mut, ratio)


def test_a_stencil_across_a_group_boundary_leaves_the_bound(synth_assets):
    body = synth_assets["body"]
    sizes = (7, 9)
    parts = [M.motion_pair(80 + i, N) for i, N in enumerate(sizes)]
    pp, pt, tp, tt = (np.concatenate([p[q] for p in parts]) for q in range(4))
    f64, _, scale = M.evaluate_groups(body, pp, pt, tp, tt, sizes, fps=5)
    f32 = M.evaluate_groups(body, pp, pt, tp, tt, sizes, fps=5, dtype=M.F32)[0]
    mut, (row, col) = M.GROUP_MUTATION
    bad = M.evaluate_groups(body, pp, pt, tp, tt, sizes, fps=5, mut=mut)[0]
    k = M.ROWS.index(row)
    B = M.bound(f32, f64, scale)
    ratio = abs(bad[0, k, col] - f64[0, k, col]) / B[0, k, col]
    print(f"{mut} moves group 0 {row}[{col}] by {ratio:.3e} Bound")
    assert ratio > 1.0
    assert np.array_equal(bad[1], f64[1], equal_nan=True)                 # the last group has no neighbour to reach into
    # and a group of the batch is the motion evaluated alone
    alone = M.evaluate(body, *parts[1], fps=5)[0]
    assert np.array_equal(alone, f64[1], equal_nan=True)
