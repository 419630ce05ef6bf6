"""The float32 confidence mean that picks a frame's regime, summed in the reference's order (net/sig_mp.py:138).

CPU-only. ``c = j2dc[:, -1].mean().item()`` is compared as a Python double with conf_lo (>) and conf_hi (>=); on frames whose
mean sits on a threshold the last bit of the float32 mean decides the branch, so the order of the 33 additions is part of
the contract. oracle.sig_mp_oracle.conf_mean_ref_np restates that order; the device sums in it too (rc_conf_mean33,
tests/test_gpu_conf_mean.py). The fixtures seq_threshold_edges / seq_live_pre_edges put frames on the edges where a
64-lane xor butterfly sum (the device's earlier order) falls on the other side.
"""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import sig_mp_oracle as O

t = torch.from_numpy
GOLD = os.path.join(os.path.dirname(__file__), "golden")
EDGE_SEQS = sorted(p for p in glob.glob(os.path.join(GOLD, "seq_*.npz")) if "conf_ref" in np.load(p).files)


regimes = O.conf_regimes


def test_reference_order_equals_torch_strided_mean():
    x = O.conf_edge_frames(7, 40_000, 15_000)
    n = x.shape[0]
    assert n >= 100_000
    frames = np.zeros((n, 33, 3), np.float32)
    frames[..., 2] = x
    frames[..., :2] = 0.25
    want = np.array([torch.from_numpy(frames[i])[:, -1].mean().item() for i in range(n)], np.float64)   # the reference's expression
    got = O.conf_mean_ref_np(x)
    assert got.dtype == np.float32
    bad = np.nonzero(got.astype(np.float64) != want)[0]
    assert bad.size == 0, f"{bad.size} frames differ, first {bad[:5]}"
    assert np.array_equal(O.conf_mean(t(frames)).numpy(), got)   # the oracle's batched strided form: the same bits
    # the generator really sits on the edges: there the butterfly order picks the other regime on many frames
    b = O.conf_mean_butterfly_np(x)
    for lo, hi in ((0.7, 0.8), (0.85, 0.9)):
        assert int((regimes(got, lo, hi) != regimes(b, lo, hi)).sum()) > 1000
    # the worked example: 33 x 0.85f -> 0.84999990 in the reference's order, 0.85000002 in the butterfly's
    eq = np.full((1, 33), np.float32(0.85))
    assert float(O.conf_mean_ref_np(eq)[0]) < 0.85 < float(O.conf_mean_butterfly_np(eq)[0])
    assert float(O.conf_mean_ref_np(np.zeros((1, 33), np.float32))[0]) == 0.0
    assert float(O.conf_mean_ref_np(np.ones((1, 33), np.float32))[0]) == 1.0


def test_edge_fixtures_exist():
    assert sorted(os.path.basename(p) for p in EDGE_SEQS) == ["seq_live_pre_edges.npz", "seq_threshold_edges.npz"]


@pytest.mark.parametrize("path", EDGE_SEQS, ids=[os.path.basename(p)[4:-4] for p in EDGE_SEQS])
def test_edge_fixture_discriminates_the_orders(path):
    """conf_ref is the reference's own mean of every frame; at least 16 frames per threshold where the butterfly order would
    pick the other side, the first of them early (the divergence carries through the LSTM states to the end)."""
    s = np.load(path)
    lo, hi = (0.85, 0.9) if str(s["live"]) == "pre" else (0.7, 0.8)
    c = s["j2dc"][:, :, 2]
    ref = O.conf_mean_ref_np(c)
    assert np.array_equal(ref, s["conf_ref"])
    r, b = ref.astype(np.float64), O.conf_mean_butterfly_np(c).astype(np.float64)
    flip_lo = np.nonzero((r > lo) != (b > lo))[0]
    flip_hi = np.nonzero((r >= hi) != (b >= hi))[0]
    assert flip_lo.size >= 16 and flip_hi.size >= 16, (flip_lo.size, flip_hi.size)
    assert flip_lo[0] < 16 and flip_hi[0] < 32
    reg = regimes(ref, lo, hi)
    assert np.array_equal(reg, O.fixture_regimes(s))
    assert {(int(a), int(b)) for a, b in zip(reg[:-1], reg[1:])} >= {(0, 1), (1, 2), (0, 2), (1, 0), (2, 0)}
    mid = (reg == 1) & (r - lo < 1e-6)
    assert int(mid.sum()) >= 8                                    # mid frames with k = (c - lo) / (hi - lo) below 1e-5


def _oracle_run(s, synth_assets):
    """the oracle over a fixture frame by frame: (branch trace [T, 5], pose, tran)"""
    live = str(s["live"])
    net = O.OracleNet(synth_assets["body"], batch=1, live=(live == "pre"))
    net.load_numpy_state_dict(synth_assets["state_dict"])
    if live == "post":
        net.live = True
    for k in ("use_flat_floor", "use_reproj_opt", "use_vision_updater", "use_imu_updater"):
        setattr(net, k, bool(s[k]))
    net.gravityc = t(s["gravityc"]).view(1, 3)
    ft = t(s["first_tran"]) if s["first_tran"].size else None
    trace, poses, trans = [], [], []
    for i in range(s["pose"].shape[0]):
        p, tr = net.forward_online(t(s["j2dc"][i]), t(s["accc"][i]), t(s["oric"][i]), ft if i == 0 else None,
                                   bool(s["first_frame"]) and i == 0)
        tc = net.trace
        trace.append([int(tc["n4"][0]), int(tc["n6"][0]), int(tc["n_floor_add"][0]), int(tc["n_floor"][0]), int(tc["reach"][0])])
        poses.append(p), trans.append(tr)
    return np.asarray(trace), torch.stack(poses).numpy(), torch.stack(trans).numpy()


@pytest.mark.parametrize("path", EDGE_SEQS, ids=[os.path.basename(p)[4:-4] for p in EDGE_SEQS])
def test_butterfly_mean_is_caught_by_the_edge_fixture(path, synth_assets, monkeypatch):
    """Mutation: the oracle with its mean summed in the butterfly order must disagree with the reference's fixture (branch trace
    or outputs beyond the parity budget); with the reference order it agrees (test_oracle_golden.test_sequence_vs_reference)."""
    s = np.load(path)
    monkeypatch.setattr(O, "conf_mean", lambda j2dc: t(O.conf_mean_butterfly_np(j2dc[:, :, 2].numpy())))
    trace, pose, tran = _oracle_run(s, synth_assets)
    want = s["trace"][:, 1:6].astype(np.int64)
    trace_bad = np.nonzero((trace != want).any(axis=1))[0]
    dt = float(np.abs(tran.astype(np.float64) - s["tran"]).max())
    dp = float(np.abs(pose.astype(np.float64) - s["pose"]).max())
    assert trace_bad.size > 0 or max(dt, dp) > 1e-4, f"butterfly order unnoticed: tran {dt:.2e}, pose {dp:.2e}"


def test_library_build_keeps_float_order():
    """rc_conf_mean33 relies on the compiler keeping the order of its float additions: no fast-math style flags in the build."""
    mk = open(os.path.join(os.path.dirname(__file__), "..", "robustcap_amd", "csrc", "Makefile")).read()
    for flag in ("-ffast-math", "-fassociative-math", "-funsafe-math-optimizations", "-Ofast", "-fno-signed-zeros"):
        assert flag not in mk, flag
