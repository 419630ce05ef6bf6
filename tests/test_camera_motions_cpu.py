"""The camera-frame motion preparation without a GPU: the numpy restatement tests/camera_motion_ref.py of preprocess.py:460-470, 477-483
(3DPW / 3DPW-OCC) and :351-364, 379-385 (TotalCapture) against what the REFERENCE computed for the same seeded sequences
(tests/golden/camera/camera_motions.npz, tools/capture_camera_motions.py). The bound is the project's (subnet_batches_ref.bound_ratio):
K = 8 x the float32 restatement's own error of the float64 one + 1e-7 of the quantity's scale; the reference's numbers and the float32
restatement are both held to it around the float64 restatement. The interleave, the camera rows used, the TotalCapture flip and its two
translation corrections are exact in float32 and compared bit for bit. Also: the length rules on tables alone, and the parts of the
evaluation harness's camera-frame layout that need no device."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import camera_motion_ref as CM
from subnet_batches_ref import bound_ratio
from subnet_corpus_ref import aa_to_R
from robustcap_amd import config as cfg
from robustcap_amd import evaluate, preprocess, synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "camera")
BLOCKS = ("posec", "tranc", "joint3d", "sync_3d_mp", "vert6", "imu_accc", "imu_oric")


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "camera_motions.npz")), json.load(open(os.path.join(GOLDEN, "meta.json")))


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def test_fixture_sha256():
    meta = json.load(open(os.path.join(GOLDEN, "meta.json")))
    with open(os.path.join(GOLDEN, "camera_motions.npz"), "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == meta["sha256"]["camera_motions.npz"]
    assert "preprocess_3dpwocc" in meta["variant"] and meta["cam_repeat"] == 2
    assert os.path.getsize(os.path.join(GOLDEN, "camera_motions.npz")) < 512 * 1024


def _restated(z, meta, dtype):
    n = len(meta["in"])
    body = synth.make_body(meta["body_seed"])
    return CM.prepare(body, [z[f"pose.{i}"].reshape(-1, 24, 3) for i in range(n)], [z[f"tran.{i}"] for i in range(n)],
                      [z[f"cam.{i}"] for i in range(n)], [z[f"beta.{i}"] for i in range(n)], meta["cam_repeat"], meta["smooth_n"], cfg.mp_mask,
                      cfg.vi_mask, cfg.ji_mask, dtype, keypoints=[z[f"kp.{i}"] for i in range(n)])


def test_restatement_matches_the_reference(fixture):
    z, meta = fixture
    r64, r32 = _restated(z, meta, np.float64), _restated(z, meta, np.float32)
    n = len(meta["in"])
    out = CM.output_lengths(meta["in"], meta["cam"], meta["cam_repeat"])
    assert out == [5, 12, 30] == [z[f"posec.{i}"].shape[0] for i in range(n)]      # the 2 n + 1 minimum; a pose longer than its cameras; 30
    worst = 0.0
    for i in range(n):
        for k in BLOCKS:
            ref, f64, f32 = z[f"{k}.{i}"], r64[k][i], r32[k][i]
            assert ref.shape == f64.shape == f32.shape and f32.dtype == np.float32, (k, i)
            r_ref, r_32 = bound_ratio(ref, f64, f32), bound_ratio(f32, f64, f32)
            print(f"RATIO camera fixture {k}.{i}: reference {r_ref:.4f}, float32 restatement {r_32:.4f} of the bound (max |f64| "
                  f"{np.abs(f64).max():.3e}, float32 restatement's error {np.abs(f32.astype(np.float64) - f64).max():.3e})")
            worst = max(worst, r_ref, r_32)
        assert _bits(r32["cam_T"][i], z[f"cam_T.{i}"])                                  # np.repeat and the two cuts
    assert worst <= 1.0
    # cameras far from the identity: the root really moved
    assert min(np.abs(z[f"cam_T.{i}"][:, :3, :3] - np.eye(3)).max() for i in range(n)) > 0.5


def test_the_interleave_bit_for_bit(fixture):
    z, meta = fixture
    out = CM.output_lengths(meta["in"], meta["cam"], meta["cam_repeat"])
    for i, T in enumerate(out):
        kp, want = z[f"kp.{i}"], z[f"joint2d_mp.{i}"]
        assert _bits(CM.interleave(kp, T), want)
        # the closed form the kernel implements: even <- kp[t/2]; odd <- midpoint, all three columns; odd behind the last frame <- that frame
        t = np.arange(T)
        h = t // 2
        nxt = np.minimum(h + 1, len(kp) - 1)
        closed = np.where((t % 2 == 0)[:, None, None] | (h + 1 >= len(kp))[:, None, None], kp[h], (kp[nxt] + kp[h]) / np.float32(2.0))
        assert _bits(closed, want)
    assert _bits(z["joint2d_mp.1"][11], z["kp.1"][5]) and _bits(z["joint2d_mp.1"][10], z["kp.1"][5])          # the last frame twice
    assert _bits(z["joint2d_mp.0"][3, :, 2], (z["kp.0"][2, :, 2] + z["kp.0"][1, :, 2]) / np.float32(2))      # the confidence is averaged too
    assert len(CM.interleave(z["kp.0"])) == 2 * len(z["kp.0"]) and out[0] == 5                                # and the cut to len(posec)


def test_length_rules_on_tables():
    ins, cams = [5, 7, 30, 131, 14, 9, 1], [3, 3, 13, 66, 7, 100, 1]
    want = [min(n, 2 * c) for n, c in zip(ins, cams)]
    assert want == [5, 6, 26, 131, 14, 9, 1]
    assert CM.output_lengths(ins, cams, 2) == want == preprocess.camera_output_lengths(ins, cams, 2)
    assert preprocess.camera_output_lengths(ins, cams, 1) == [min(n, c) for n, c in zip(ins, cams)] == CM.output_lengths(ins, cams, 1)
    assert preprocess.camera_output_lengths([5, 9], [1, 1], 0) == [5, 9] == CM.output_lengths([5, 9], [1, 1], 0)
    for bad in (dict(in_frames=[5], cam_frames=[0]), dict(in_frames=[5], cam_frames=[2], cam_repeat=0), dict(in_frames=[5], cam_frames=[2], cam_repeat=-1),
                dict(in_frames=[5, 6], cam_frames=[2])):
        with pytest.raises(ValueError):
            preprocess.camera_output_lengths(**bad)


def test_totalcapture_steps_against_the_reference(fixture):
    z, meta = fixture
    pose, ori, acc, tran = CM.totalcapture_clip(z["tc.gt"], z["tc.ori_raw"], z["tc.acc_raw"], z["tc.vicon"])
    T = min(meta["totalcapture"].values())
    assert len(pose) == len(ori) == len(acc) == len(tran) == T == 28 == len(z["tc.pose"])
    assert _bits(ori, z["tc.ori_raw"][:T][:, [2, 3, 0, 1, 4, 5]]) and list(preprocess.TC_IMU_ORDER) == CM.TC_ORDER
    of, af = CM.totalcapture_flip(ori, acc, np.float32)
    assert np.array_equal(of, z["tc.ori"]) and np.array_equal(af, z["tc.acc"])       # products with 0 and +-1: exact (up to the sign of a zero)
    assert _bits(CM.totalcapture_tran(tran, np.float32), z["tc.tran"])
    assert np.array_equal(np.asarray(preprocess.TC_FLIP), CM.TC_FLIP)
    # the root through a static camera that holds the flip, translation kept: the reference's pose, joints and vertices
    body = synth.make_body(meta["body_seed"])
    static = np.eye(4)
    static[:3, :3] = CM.TC_FLIP
    r = {}
    for f in (np.float64, np.float32):
        r[f] = CM.prepare(body, [pose.reshape(-1, 24, 3)], [CM.totalcapture_tran(tran, np.float32)], [static], None, 0, meta["smooth_n"], cfg.mp_mask,
                          cfg.vi_mask, cfg.ji_mask, f, root_only=True)
    assert _bits(r[np.float32]["tranc"][0], z["tc.tran"])
    R32 = aa_to_R(pose.reshape(-1, 3).astype(np.float32), np.float32).reshape(-1, 24, 3, 3)
    assert np.array_equal(r[np.float32]["posec"][0][:, 0], CM.TC_FLIP.astype(np.float32) @ R32[:, 0])       # the flip of the root is exact
    worst = 0.0
    for k, name in (("posec", "pose"), ("joint3d", "joint3d"), ("imu_oric", "grot6"), ("vert6", "vert6"), ("sync_3d_mp", "sync_3d_mp")):
        rr = bound_ratio(z["tc." + name], r[np.float64][k][0], r[np.float32][k][0])
        print(f"RATIO camera fixture tc.{name}: reference {rr:.4f} of the bound")
        worst = max(worst, rr)
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ the harness's layout handling, host only
def _camera_dict(z, n=2):
    return {"posec": [torch.from_numpy(z[f"posec.{i}"]) for i in range(n)], "tranc": [torch.from_numpy(z[f"tranc.{i}"]) for i in range(n)],
            "imu_oric": [torch.from_numpy(z[f"imu_oric.{i}"]) for i in range(n)], "imu_accc": [torch.from_numpy(z[f"imu_accc.{i}"]) for i in range(n)],
            "joint2d_mp": [torch.from_numpy(z[f"joint2d_mp.{i}"]) for i in range(n)], "cam_K": [torch.eye(3)] * n,
            "cam_T": [torch.from_numpy(z[f"cam_T.{i}"]) for i in range(n)]}


def test_the_harness_reads_the_camera_frame_layout(fixture):
    z, _ = fixture
    d = _camera_dict(z)
    assert evaluate.is_camera_layout(d) and not evaluate.is_camera_layout({"pose": [], "cam_K": []})
    assert evaluate.rows_of(d) == [(0, 0), (1, 0)]
    assert [evaluate.sequence_frames(d, i) for i in range(2)] == [5, 12]
    pose, tran = evaluate.labels(d, 1, 0, device="cpu")
    assert _bits(pose.numpy(), z["posec.1"]) and _bits(tran.numpy(), z["tranc.1"])         # as they are
    ft = evaluate.first_translations(d, [(1, 0), (0, 0)])
    assert _bits(ft.numpy(), np.stack([z["tranc.1"][0], z["tranc.0"][0]]))
    assert evaluate.camera_varies(d, 0) and evaluate.camera_varies(d, 1)
    still = dict(d, cam_T=[t[:1].repeat(len(t), 1, 1) for t in d["cam_T"]])
    assert not evaluate.camera_varies(still, 0)
    with pytest.raises(ValueError, match="moving camera"):                                 # before anything touches a device
        evaluate.run_dataset(d, {}, None, use_flat_floor=True, device="cpu")
    with pytest.raises(ValueError):
        evaluate.root_position_errors(d, {}, align="first")
    assert evaluate.root_position_errors(d, {})[0] == {}
