"""The confidence mean that picks a frame's regime (net/sig_mp.py:138) on the device, and whole batches that sit on the thresholds.

rc_conf_mean runs the kernel that plans rc_sequence on the helper the per-frame prep uses (rc_conf_mean33): its mean must be
bitwise the reference's (torch's CPU reduction of the strided row, oracle.sig_mp_oracle.conf_mean_ref_np; tests/test_conf_order.py
pins the two equal), its regime code that of the reference's double compares. A batch whose every frame sits on conf_lo or
conf_hi then has to come out the same on the wavefront engine and frame-stepped, and equal to the oracle."""
import numpy as np
import pytest
import torch

from oracle import sig_mp_oracle as O

pytestmark = pytest.mark.gpu
t = torch.from_numpy


def _conf_mean(j2dc, lo, hi):
    from robustcap_amd import _lib
    lib = _lib.load()
    n = j2dc.shape[0]
    mean = torch.full((n,), float("nan"), device="cuda")
    code = torch.full((n,), -1, dtype=torch.int8, device="cuda")
    rc = lib.rc_conf_mean(_lib.ptr(j2dc), n, lo, hi, _lib.ptr(mean), _lib.ptr(code), _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return mean.cpu().numpy(), code.cpu().numpy()


def test_conf_mean_is_the_reference_order():
    x = O.conf_edge_frames(11, 40_000, 15_000)
    n = x.shape[0]
    assert n >= 100_000
    frames = np.zeros((n, 33, 3), np.float32)
    frames[..., 2] = x
    frames[..., :2] = np.float32(0.3)
    want = O.conf_mean_ref_np(x)
    assert np.array_equal(t(frames)[:, :, 2].mean(dim=1).numpy(), want)      # torch's strided mean, the reference's expression
    j = t(frames).cuda()
    for lo, hi in ((0.7, 0.8), (0.85, 0.9)):
        mean, code = _conf_mean(j, lo, hi)
        bad = np.nonzero(mean.view(np.uint32) != want.view(np.uint32))[0]
        ulps = np.abs(mean.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))[bad]
        assert bad.size == 0, f"{bad.size} of {n} means differ from the reference's (max {ulps.max()} ulp), first frames {bad[:5]}"
        reg = O.conf_regimes(want, lo, hi)
        flips = np.nonzero(code != reg)[0]
        assert flips.size == 0, f"{flips.size} regime codes differ at ({lo}, {hi}), first frames {flips[:5]}"
        assert {0, 1, 2} <= set(code.tolist())


def test_conf_mean_arguments():
    from robustcap_amd import _lib
    lib = _lib.load()
    j = torch.full((3, 33, 3), 0.85, device="cuda")
    mean = torch.empty(3, device="cuda")
    code = torch.empty(3, dtype=torch.int8, device="cuda")
    s = _lib.stream_ptr()
    assert lib.rc_conf_mean(_lib.ptr(j), 3, 0.85, 0.9, _lib.ptr(mean), None, s) == 0
    assert lib.rc_conf_mean(_lib.ptr(j), 3, 0.85, 0.9, None, _lib.ptr(code), s) == 0
    torch.cuda.synchronize()
    want = float(O.conf_mean_ref_np(np.full((1, 33), np.float32(0.85)))[0])
    assert want < 0.85 and mean.cpu().tolist() == [want] * 3 and code.cpu().tolist() == [0] * 3   # 33 x 0.85f: below 0.85
    assert lib.rc_conf_mean(_lib.ptr(j), 3, 0.85, 0.9, None, None, s) != 0
    assert lib.rc_conf_mean(None, 3, 0.85, 0.9, _lib.ptr(mean), None, s) != 0
    assert lib.rc_conf_mean(None, 0, 0.85, 0.9, None, None, s) == 0


def _edge_inputs(assets, B, T, seed):
    """bench inputs whose every (row, frame) has confidences with the reference mean within 2 ulp of 0.7 or 0.8 (or 33 equal
    values at / next to them)"""
    import bench
    from robustcap_amd import synth
    m = bench.make_inputs(assets["body"], B, T, "mixed", seed=seed)
    rows = O.conf_edge_frames(seed, 0, (B * T) // 2 + 1, thresholds=(0.7, 0.8), extremes=False)
    order = np.argsort(synth.uniform01(seed, 3, rows.shape[0]), kind="stable")
    m["j2dc"][..., 2] = rows[order[:B * T]].reshape(B, T, 33)
    return m


@pytest.mark.parametrize("B", [256, 97])
def test_batch_on_the_thresholds_wavefront_frame_stepped_and_oracle(B, synth_assets):
    """Every frame of every row on a threshold, T = 64 in two calls: the wavefront engine (planned from rc_scan_conf_kernel's codes)
    bitwise the frame-stepped launches (flags from the prep kernel) -- outputs, all six states, traces -- and both the oracle."""
    from robustcap_amd.net.sig_mp import Net
    T, cut = 64, 24
    m = _edge_inputs(synth_assets, B, T, 41 + B)
    runs = []
    for seq in (True, False):
        net = Net(body=synth_assets["body"], batch=B)
        net.load_state_dict(synth_assets["state_dict"])
        net.set_sequence_mode(seq, 8, force=True)
        net.gravityc = t(m["gravityc"])
        a = net.forward_sequence(t(m["j2dc"][:, :cut]), t(m["accc"][:, :cut]), t(m["oric"][:, :cut]), first_tran=t(m["first_tran"]))
        b = net.forward_sequence(t(m["j2dc"][:, cut:]), t(m["accc"][:, cut:]), t(m["oric"][:, cut:]))
        torch.cuda.synchronize()
        runs.append((torch.cat([a[0], b[0]], 1).cpu(), torch.cat([a[1], b[1]], 1).cpu(),
                     {n: net.get_state(n) for n in ("rnn2", "rnn3", "rnn4", "rnn6", "rnn7", "rnn8")}, net.get_trace(), net.sequence_stats()))
        del net
    (wp, wt, ws, wtr, wstat), (sp, st, ss, strc, sstat) = runs
    assert wstat[0] == T - 1 and sstat[0] == 0
    assert torch.equal(wp, sp) and torch.equal(wt, st) and torch.equal(wtr, strc)
    for n in ws:
        assert torch.equal(ws[n][0], ss[n][0]) and torch.equal(ws[n][1], ss[n][1]), n
    ora = O.OracleNet(synth_assets["body"], batch=B)
    ora.load_numpy_state_dict(synth_assets["state_dict"])
    ora.gravityc = t(m["gravityc"])
    ob = O.OracleBody(synth_assets["body"])
    regimes = set()
    for i in range(T):
        p, tr = ora.forward_batch(t(m["j2dc"][:, i]), t(m["accc"][:, i]), t(m["oric"][:, i]), t(m["first_tran"]) if i == 0 else None)
        regimes |= set(O.conf_regimes(ora.trace["c"].numpy(), 0.7, 0.8).tolist())
        assert float((wt[:, i] - tr).abs().max()) <= 1e-4, i
        assert float(O.rotation_angle_deg(wp[:, i], p).max()) <= 0.1, i
        jd = (ob.forward_kinematics(wp[:, i], wt[:, i])[1] - ob.forward_kinematics(p, tr)[1]).abs().max()
        assert float(jd) <= 1e-4, i
    assert regimes == {0, 1, 2}
    assert wtr[:, 0].tolist() == O.conf_regimes(O.conf_mean_ref_np(m["j2dc"][:, -1, :, 2]), 0.7, 0.8).tolist()
    for n in ws:
        h, c = ws[n]
        assert float((h - ora.h[n]).abs().max()) <= 1e-4 and float((c - ora.c[n]).abs().max()) <= 2e-4, n
