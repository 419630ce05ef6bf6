"""The corpus builders without a GPU: the numpy restatement tests/subnet_corpus_ref.py of the eleven dataset recipes inside
train_rnn2 .. train_rnn8 (net/sig_mp.py:301-839) against the rows the REFERENCE formed from the same dictionaries
(tests/golden/corpus/subnet_corpus.npz, tools/capture_subnet_corpus.py). The bound is the project's (subnet_batches_ref.bound_ratio):
K = 8 x the float32 restatement's own error of the float64 one + 1e-7 of the quantity's scale; the reference's rows and the float32
restatement are both held to it around the float64 restatement. Observed: profiles/subnet_corpus_ratios.txt (the RATIO lines)."""
import hashlib
import json
import os

import numpy as np
import pytest

import subnet_corpus_ref as R
from subnet_batches_ref import bound_ratio
from robustcap_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "corpus")


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(GOLDEN, "subnet_corpus.npz"))
    aist, amass = R.unpack_dicts(z)
    return z, {"aist": aist, "amass": amass}


def test_fixture_sha256():
    meta = json.load(open(os.path.join(GOLDEN, "meta.json")))
    with open(os.path.join(GOLDEN, "subnet_corpus.npz"), "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == meta["sha256"]["subnet_corpus.npz"]


def test_fixture_is_what_make_training_dicts_gives(fixture):
    """The stored inputs are the synthetic dictionaries of the recorded seed: the fixture and the GPU tests' inputs have one source
    (the tables exactly; the numbers to float32 rounding, as another libm may round a float64 intermediate the other way)."""
    z, _ = fixture
    meta = json.load(open(os.path.join(GOLDEN, "meta.json")))
    again = R.pack_dicts(*synth.make_training_dicts(meta["seed"], tuple(meta["lengths"]), synth.make_body(1), meta["n_cam"]))
    assert sorted(again) == sorted(k for k in z.files if k.split(".")[0] in ("aist", "amass"))
    for k, v in again.items():
        if v.dtype == np.int64:
            assert np.array_equal(v, z[k]), k
        else:
            assert v.shape == z[k].shape and np.allclose(v, z[k], rtol=1e-5, atol=1e-5), k


@pytest.mark.parametrize("name,source", R.RECIPES)
def test_restatement_matches_the_reference(fixture, name, source):
    z, dicts = fixture
    ref_x, ref_y = R.captured(z, name, source)
    x64, y64 = R.build(name, source, dicts[source], np.float64)
    x32, y32 = R.build(name, source, dicts[source], np.float32)
    assert [a.shape for a in x64] == [a.shape for a in ref_x] and [a.shape for a in y64] == [a.shape for a in ref_y]   # count, order, rows
    assert all(a.dtype == np.float32 for a in x32 + y32)
    widths = R.WORLD_WIDTHS if (source == "amass" and name in ("rnn4", "rnn6")) else R.WIDTHS[name]
    assert (x64[0].shape[1], y64[0].shape[1]) == widths
    ref_x, x64, x32 = np.concatenate(ref_x), np.concatenate(x64), np.concatenate(x32)
    blocks = [(g, ref_x[:, a:b], x64[:, a:b], x32[:, a:b]) for g, a, b in R.column_groups(widths[0])]
    blocks.append(("label", np.concatenate(ref_y), np.concatenate(y64), np.concatenate(y32)))
    for what, ref, f64, f32 in blocks:
        if name == "rnn8" and what == "label":
            assert np.array_equal(ref, f64) and np.array_equal(ref, f32)
            continue
        r_ref, r_32 = bound_ratio(ref, f64, f32), bound_ratio(f32, f64, f32)
        bound = 8.0 * np.abs(f32.astype(np.float64) - f64).max() + 1e-7 * np.abs(f64).max()
        r_pair = float(np.abs(ref.astype(np.float64) - f32.astype(np.float64)).max() / bound)
        print(f"RATIO {name} {source} {what}: reference vs float64 {r_ref:.4f}, float32 vs float64 {r_32:.4f}, "
              f"float32 vs reference {r_pair:.4f} of the bound {bound:.3e}")
        assert r_ref <= 1.0 and r_32 <= 1.0 and r_pair <= 1.0


def test_sample_counts_and_order(fixture):
    """The None view, the None occlusion entry and the one of the wrong length: which samples exist, and in which order."""
    z, dicts = fixture
    aist = dicts["aist"]
    n_seq, n_cam = len(aist["cam_K"]), len(aist["cam_K"][0])
    mp = np.asarray(z["aist.joint2d_mp.frames"])
    occ = np.asarray(z["aist.joint2d_occ.frames"])
    lengths = [len(a) for a in aist["imu_acc"]]
    assert (mp == 0).sum() == n_seq and (occ == 0).sum() == (n_seq + 1) // 2                     # one None view per sequence, None occlusions
    assert sum(0 < occ[i, j] != lengths[i] for i in range(n_seq) for j in range(n_cam)) == n_seq // 2   # entries a frame short
    expect4, expect6 = [], []
    for i in range(n_seq):
        for j in range(n_cam):
            if mp[i, j] == 0:
                continue
            expect4.append(lengths[i] - 2), expect6.append(lengths[i] - 2)
            if occ[i, j] == lengths[i]:
                expect4.append(lengths[i] - 2)
    assert [int(v) for v in z["rnn4.aist.lengths"]] == expect4 and [int(v) for v in z["rnn6.aist.lengths"]] == expect6
    assert len(expect4) > len(expect6) > n_seq
    x4, _ = R.build("rnn4", "aist", aist, np.float64)
    assert [len(a) for a in x4] == expect4
    # a plain sample and its occlusion sample share the IMU columns and differ in the keypoints
    k = next(s for s in range(len(x4) - 1) if np.array_equal(x4[s][:, :72], x4[s + 1][:, :72]))
    assert not np.array_equal(x4[k][:, 72:], x4[k + 1][:, 72:])


def test_rnn8_labels_are_exact(fixture):
    """A condition on the INPUTS, met by construction (synth.make_training_dicts: a slow and a fast half): no foot speed within 1e-3 of
    the threshold, both classes for both feet -- so float32 and float64 decide alike and the labels are compared for equality."""
    z, dicts = fixture
    speed = np.concatenate([R.foot_speed(j) for j in dicts["amass"]["joint3d"]])
    assert np.abs(speed - 0.25).min() > 1e-3
    contact = speed < 0.25
    assert contact.any(0).all() and (~contact).any(0).all()
    _, ref = R.captured(z, "rnn8", "amass")
    assert np.array_equal(np.concatenate(ref), contact.astype(np.float32))
    assert np.array_equal(np.concatenate(R.build("rnn8", "amass", dicts["amass"], np.float32)[1]), contact.astype(np.float32))


def test_occlusion_sample_is_not_divided(fixture):
    """net/sig_mp.py:480 divides the plain sample's tensor: the captured occlusion rows match the restatement only WITHOUT the
    bounding-box division; a restatement that divides misses the bound by orders of magnitude."""
    z, dicts = fixture
    ref = np.concatenate(R.captured(z, "rnn4", "aist")[0])[:, 72:]
    f64 = np.concatenate(R.build("rnn4", "aist", dicts["aist"], np.float64)[0])[:, 72:]
    f32 = np.concatenate(R.build("rnn4", "aist", dicts["aist"], np.float32)[0])[:, 72:]
    wrong = np.concatenate(R.build("rnn4", "aist", dicts["aist"], np.float64, occ_divides=True)[0])[:, 72:]
    assert bound_ratio(ref, f64, f32) <= 1.0
    bound = 8.0 * np.abs(f32.astype(np.float64) - f64).max() + 1e-7 * np.abs(f64).max()
    r = float(np.abs(ref.astype(np.float64) - wrong).max() / bound)
    print(f"RATIO rnn4 aist keypoints, a restatement that divides the occlusion sample: {r:.3e} of the bound")
    assert r > 100.0
