"""art.FullMotionEvaluator without a GPU: the float64 restatement tests/motion_metrics_f64.py against the reference's own output
(tests/golden/motion/motion_metrics.npz, written by tools/capture_motion_metrics.py), and the deliberate mistakes the bound must catch.

  fixture    every entry of the captured [11,2] results (near / far / same x fps=60 | fps=5 with a mask | align_joint=5) within
             Bound = 8 |float32 transcription - restatement| + 1e-7 scale of the restatement; NaNs where the fixture has them; the
             fixture's sha256 equals its meta.json. The angle rows pin the wiring only (the capture ran a numpy rotation -> axis-angle in
             place of cv2.Rodrigues, which is not installed where the fixture is written).
             Two more captures, of the 131-frame `long` motion (fps=60 | align_joint=5), are the one place where the reference's own te at
             its default frame rate is a number: 71 one-second windows; the 24-frame motions have none, and row 6 is NaN exactly when
             frames <= fps. The long poses are regenerated from the seed and their sha256 is in meta.json.
  mistakes   biased std, std over all elements, a stencil across a group boundary, a window of fps +- 1, the offset's sign, ve without the
             offset, jerk without the translation: each moves its named output by more than the bound.
  blocks     the device forms every (mean, std) from per-block (n, mean, M2) of 32 frames merged in index order. evaluate_blockwise
             restates that in float64 (it shares nothing with the kernel) and equals evaluate(F64) to 1e-10 relative at 1, 3, 4 frames
             (torch's NaNs), 33 and 61 (two blocks), 65 and 67 (a third block of 1 and 3 frames: no jerk rows of its own), 97 and 131
             (four and five blocks; 131 at fps 60: three te blocks) at fps 5 and 60. Five mistakes of the block-wise path -- the running
             count not carried, no cross term, unweighted block means, a te window of fps % 32, jerk rows counted from `frames` -- each
             move their named output by more than the bound at (67 | 97 | 131, fps 60); the first and the fourth move nothing at all
             at the sizes the device tests had before those.
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
    return {"near": (g["pose_near"], gt, tp, tt), "far": (g["pose_far"], gt, tp, tt), "same": (gt, gt, tt, tt), "long": M.golden_long()[0]}


def test_fixture_hash_matches_its_meta(golden_dir):
    d = os.path.join(golden_dir, "motion")
    meta = json.load(open(os.path.join(d, "meta.json")))
    assert list(meta["sha256"]) == ["motion_metrics.npz"]
    assert hashlib.sha256(open(os.path.join(d, "motion_metrics.npz"), "rb").read()).hexdigest() == meta["sha256"]["motion_metrics.npz"]
    # the `long` motion is not stored: the arrays regenerated from its seed are the ones the reference was run on
    assert meta["long_inputs_sha256"] == M.golden_long()[1] and list(M.golden_long()[1]) == list(M.GOLDEN_LONG_INPUTS)


def test_fixture_translations_are_the_seeded_ones(fixture):
    tp, tt = M.golden_translations(24)
    assert np.array_equal(fixture["tran_p"], tp) and np.array_equal(fixture["tran_t"], tt)
    _, _, ltp, ltt = M.golden_long()[0]
    assert ltp.shape == (M.GOLDEN_LONG[1], 3) and np.array_equal(fixture["tran_p_long"], ltp) and np.array_equal(fixture["tran_t_long"], ltt)


GOLDEN_PAIRS = [(s, m) for m in M.GOLDEN_MOTIONS for s in M.GOLDEN_SETTINGS] + [(s, "long") for s in M.GOLDEN_LONG_SETTINGS]


@pytest.mark.parametrize("setting,motion", GOLDEN_PAIRS, ids=[f"{m}-{s}" for s, m in GOLDEN_PAIRS])
def test_restatement_matches_the_reference_capture(setting, motion, fixture, motions, synth_assets):
    body = synth_assets["body"]
    fps, mask, align = M.GOLDEN_SETTINGS[setting]
    pp, pt, tp, tt = motions[motion]
    N = np.asarray(pp).shape[0]
    f64, _, scale = M.evaluate(body, pp, pt, tp, tt, fps, align, mask)
    f32 = M.evaluate(body, pp, pt, tp, tt, fps, align, mask, dtype=M.F32)[0]
    ref = fixture[f"out_{setting}_{motion}"]
    assert np.array_equal(np.isnan(f32), np.isnan(f64))
    r = M.ratios(ref, f64, M.bound(f32, f64, scale))                      # asserts the NaN placement
    for k, name in enumerate(M.ROWS):
        print(f"{setting:10s} {motion:5s} {name:5s} mean {f64[k, 0]:12.5e} std {f64[k, 1]:12.5e}  |ref - f64| / Bound {r[k, 0]:.3f} {r[k, 1]:.3f}")
    assert (r <= 1.0).all(), (setting, motion, r)
    # where the reference has NaN: the te row of 24 frames at fps 60 (no window exists; the 131 frames of `long` have 71), the std of
    # torch.zeros(1) without a mask
    assert np.isnan(ref[6]).all() == (N <= fps)
    assert np.isfinite(ref[6]).all() == (N > fps + 1)
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


BLOCK_SIZES = (1, 3, 4, 33, 61, 65, 67, 97, 131)
NEW_PAIRS = ((67, 60), (97, 60), (131, 60))                               # three, four and five blocks of 32 frames; 7, 37 and 71 te rows
# every (frames, fps) the device's value tests compared before the fps-60 / three-block cases were added, and the 61 frames of the bitwise test
OLD_PAIRS = tuple((N, 60) for N in (1, 3, 4, 31, 32, 33)) + tuple((N, 5) for N in (4, 5, 6, 15, 16, 17, 33, 61))


@pytest.fixture(scope="module")
def block_results(synth_assets):
    """(N, fps) -> the motion and its evaluate(F64) / evaluate(F32) results, computed once"""
    body, cache = synth_assets["body"], {}

    def get(N, fps):
        if (N, fps) not in cache:
            m = M.motion_pair(500 + N, N)
            f64, pj64, scale = M.evaluate(body, *m, fps, 0, [7])
            f32 = M.evaluate(body, *m, fps, 0, [7], dtype=M.F32)[0]
            cache[(N, fps)] = (m, f64, pj64, f32, scale)
        return cache[(N, fps)]
    return get


@pytest.mark.parametrize("fps", (5, 60))
def test_blockwise_merge_is_the_restatement(fps, block_results, synth_assets):
    """32-frame blocks merged by Chan's update give what torch's mean and std give: float64 on both sides, another order of the sums"""
    body = synth_assets["body"]
    for N in BLOCK_SIZES:
        m, f64, pj64, _, _ = block_results(N, fps)
        out, pj, _ = M.evaluate_blockwise(body, *m, fps, 0, [7])
        assert np.array_equal(np.isnan(out), np.isnan(f64)) and np.array_equal(np.isnan(pj), np.isnan(pj64)), (N, fps)
        rel = lambda a, b: np.where(a == b, 0.0, np.abs(a - b) / np.maximum(np.abs(b), 1e-300))[np.isfinite(b)]   # je of the align joint is 0
        r, rj = rel(out, f64).max(), rel(pj, pj64).max()
        print(f"N {N:4d} fps {fps:2d}: |blockwise - restatement| / |restatement| max {r:.2e}, per joint {rj:.2e}")
        assert r <= 1e-10 and rj <= 1e-10, (N, fps)


@pytest.mark.parametrize("mut", list(M.BLOCK_MUTATIONS))
def test_blockwise_mistakes_leave_the_bound_on_the_long_groups_only(mut, block_results, synth_assets):
    """THE GAP THESE SIZES CLOSE. A merge that does not carry the accumulated count (`count_not_carried`: na is the block before's) and a
    one-second window that wraps inside a 32-frame block (`window_wraps_block`: offset fps % 32) move NOTHING -- array_equal, NaNs
    included -- at any (frames, fps) the device's value tests ran before: no group had a third block (with two, na is 32 either way), and
    every te of fps 60 was NaN while fps 5 % 32 is 5. At (67 | 97 | 131 frames, fps 60) every mistake below moves its named output by more
    than 1 Bound: the missing cross term and the unweighted mean of the block means, which two blocks of unequal sizes already show, and
    jerk rows counted from `frames` in place of `frames - 3`, included."""
    body = synth_assets["body"]
    row, col = M.BLOCK_MUTATIONS[mut]
    k = M.ROWS.index(row)
    worst = 0.0
    for N, fps in NEW_PAIRS:
        m, f64, _, f32, scale = block_results(N, fps)
        good = M.evaluate_blockwise(body, *m, fps, 0, [7])[0]
        bad = M.evaluate_blockwise(body, *m, fps, 0, [7], mut=mut)[0]
        B = M.bound(f32, f64, scale)
        assert abs(good[k, col] - f64[k, col]) <= 1e-3 * B[k, col]            # the unmutated path sits far inside the Bound
        ratio = abs(bad[k, col] - f64[k, col]) / B[k, col]
        print(f"{mut:24s} moves {row}[{col}] by {ratio:.3e} Bound at N {N} fps {fps}")
        worst = max(worst, ratio)
    assert worst > 1.0, (mut, worst)
    if mut in ("count_not_carried", "window_wraps_block"):
        for N, fps in OLD_PAIRS:
            m = block_results(N, fps)[0]
            good = M.evaluate_blockwise(body, *m, fps, 0, [7])
            bad = M.evaluate_blockwise(body, *m, fps, 0, [7], mut=mut)
            same = np.array_equal(good[0], bad[0], equal_nan=True) and np.array_equal(good[1], bad[1], equal_nan=True)
            print(f"{mut:24s} moves nothing at N {N} fps {fps}: {same}")
            assert same, (mut, N, fps)


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
