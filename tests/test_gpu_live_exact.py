"""The lean live frame (csrc/rc_live.hip, the host side in rc_live_api.cpp / rc_aql.cpp) against the frame-stepped plan, BIT FOR BIT.

On oracle/live_exact.py's state dict every linear2 row holds one +-2^e: y[o] = fl(+-2^e h[u(o)] + b[o]) in every summation order
(tests/test_live_exact_cpu.py checks that premise, the operating point, the scripts and that a wrong sum changes bits), so the lean
frame's per-tile partial sums and the frame-stepped GEMM give the same sub-net outputs, and the contract written at the top of
rc_live.hip -- layer steps bitwise those of the frame-stepped plan, lin1_tile the arithmetic of gemm_tile<1, 1>, K4's fuse that of
rc_fuse_kernel -- makes everything else the same bits too: pose, translation and trace of every frame, h and c of all six nets and
the fusion state at the end, with generic W1, W_ih, W_hh and biases. Legs: the AQL chain (hot argument words), the graph replay
(hot = 0), the 16 x 32 tiles of RC_LIVE_LEAN_NC=2 on both, and a pre-step behind every frame; one row and four, the default leg
also two and three. The twin is forward_online without use_graph / forward_batch (rc_step) in gemm mode 0.
One more test takes the ordinary synthetic dict (generic linear2) to the live net's FIRST lean frame: the stage-1 nets read no
linear2 output, so rnn2 and rnn4 are bitwise there as well.
tests/test_gpu_live.py keeps the generic-linear2 case over whole sequences, to a flat tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import live_exact as X

pytestmark = pytest.mark.gpu
t = torch.from_numpy
NETS = ("rnn2", "rnn4", "rnn6", "rnn3", "rnn7", "rnn8")            # stage 1, then stage 2
LIVE_ENV = ("RC_LIVE_AQL", "RC_LIVE_LEAN_NC", "RC_LIVE_PRESTEP", "RC_LIVE_PRESTEP_IDLE_US", "RC_LIVE_LEAN", "RC_LIVE_EAGER", "RC_LIVE_MIRROR_BLIND")


@pytest.fixture(scope="module")
def base_dict():
    from robustcap_amd import synth
    return synth.make_state_dict(X.WEIGHT_SEED, X.GAIN)


def make_pair(sd, body, B, env, monkeypatch):
    """(twin, live): the frame-stepped plan and the live session under `env` (read when the context is created), both fp32 MFMA"""
    from robustcap_amd.net.sig_mp import Net
    for k in LIVE_ENV:
        monkeypatch.delenv(k, raising=False)
    twin = Net(body=body, batch=B)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    live = Net(body=body, batch=B)
    for n in (twin, live):
        n.load_state_dict(sd)
        n.set_gemm_mode(False)
        assert n.gemm_mode == 0
    live.use_graph = True
    return twin, live


def frame(twin, live, m, i, B):
    """frame i on both: (pose, tran) of the twin and of the live net as CPU tensors"""
    if B == 1:
        args = (t(m["j2dc"][0, i]), t(m["accc"][0, i]), t(m["oric"][0, i]))
        return twin.forward_online(*args, first_frame=(i == 0)), live.forward_online(*args, first_frame=(i == 0))
    args = (t(m["j2dc"][:, i]), t(m["accc"][:, i]), t(m["oric"][:, i]))
    pa, ta = twin.forward_batch(*args, first_frame=(i == 0))
    return (pa.cpu(), ta.cpu()), live.forward_live(*args, first_frame=(i == 0))


def backend(net):
    cap, aql, note = C.c_int32(0), C.c_int32(0), C.create_string_buffer(256)
    net._lib.rc_get_live_backend(net._ctx, C.byref(cap), C.byref(aql), note, 256)
    return cap.value, aql.value, note.value.decode()


def first_difference(twin, live):
    """which state differs, in the order a frame computes them (stage 1, stage 2): for the message of a failed frame"""
    out = []
    for n in NETS:
        (ha, ca), (hb, cb) = twin.get_state(n), live.get_state(n)
        for what, a, b in (("h", ha, hb), ("c", ca, cb)):
            for layer in range(2):
                d = (a[layer].view(torch.int32) != b[layer].view(torch.int32))
                if d.any():
                    out.append(f"{n}.{what}{layer}: {int(d.sum())} elements, max |diff| {float((a[layer] - b[layer]).abs().max()):.3g}")
    return out or ["no state differs"]


@pytest.mark.parametrize("case", X.CASES, ids=[c.name for c in X.CASES])
def test_lean_frames_are_the_frame_stepped_plan_bit_for_bit(case, synth_assets, base_dict, monkeypatch):
    body, B, T = synth_assets["body"], case.B, case.T
    sd = X.exact_sum_state_dict(X.WEIGHT_SEED, X.GAIN, case.pick, base=base_dict)
    m = X.motion(case, body)
    twin, live = make_pair(sd, body, B, case.env, monkeypatch)
    twin.gravityc = live.gravityc = t(m["gravityc"])
    for i in range(T):
        (pa, ta), (pb, tb) = frame(twin, live, m, i, B)
        tra, trb = twin.get_trace().tolist(), live.get_trace().tolist()
        if not (torch.equal(pa, pb) and torch.equal(ta, tb)):
            pytest.fail(f"{case.name} frame {i} (lean, full so far: {live.live_stats()}): pose differs in {int((pa != pb).sum())} elements (max "
                        f"{float((pa - pb).abs().max()):.3g}), tran in {int((ta != tb).sum())}; states: {first_difference(twin, live)}")
        assert tra == trb, (case.name, i, tra, trb)
    for n in NETS:
        (ha, ca), (hb, cb) = twin.get_state(n), live.get_state(n)
        assert torch.equal(ha, hb) and torch.equal(ca, cb), (case.name, n, first_difference(twin, live))
    assert torch.equal(twin.fusion_state(), live.fusion_state()), case.name
    lean, full = live.live_stats()
    assert lean + full == T and lean >= T // 2 and full >= 2, (lean, full)    # the steady state IS the lean plan; first frame, init_net, transitions are not
    assert live.live_replayed() == 0
    cap, aql, note = backend(live)
    assert cap == 1, note
    if "RC_LIVE_AQL" in case.env:
        assert aql == 0, note
    wide = "16 x 32" in note
    if case.env.get("RC_LIVE_LEAN_NC") == "2":                                # the plan that ran holds the four wide layer-step kernels
        assert wide and all(k in note for k in ("rc_live_s1_l0w", "rc_live_s1_l1w", "rc_live_s2_l0w", "rc_live_s2_l1w")), note
    else:
        assert not wide, note
    if case.leg == "prestep":
        n_pre, avail = live.live_prestep_stats()
        if avail:                                                             # (a profiler on the queue: no AQL chain, no pre-step)
            assert n_pre >= lean - 1 and n_pre > 0, (n_pre, lean)             # behind every frame


@pytest.mark.parametrize("B, nc", [(1, "1"), (4, "1"), (1, "2"), (4, "2")], ids=["b1", "b4", "b1_nc2", "b4_nc2"])
def test_stage_one_of_the_first_lean_frame_is_bitwise_on_a_generic_dict(B, nc, synth_assets, monkeypatch):
    """The ordinary synthetic dict: twin and live net in lock-step up to the live net's first lean frame. Every frame before it ran the
    same kernels on both, and rnn2 / rnn4 read prep and linear1 only: their h and c of both layers are the same bits after it."""
    from robustcap_amd import synth
    body = synth_assets["body"]
    m = synth.make_motion(211 + B, B, 8, body, conf="mid")
    if B == 4:
        m["j2dc"][1, 1:, :, 2] = 0.4                                          # one row occluded: its rnn4 is computed and discarded (amask)
        m["j2dc"][2, :, :, 2] = 0.76
    twin, live = make_pair(synth_assets["state_dict"], body, B, {"RC_LIVE_LEAN_NC": nc}, monkeypatch)
    twin.gravityc = live.gravityc = t(m["gravityc"])
    seen = False
    for i in range(8):
        before = live.live_stats() if i else (0, 0)
        frame(twin, live, m, i, B)
        if live.live_stats() == (before[0] + 1, before[1]):
            assert before[0] == 0
            seen = True
            break
    assert seen, live.live_stats()
    assert ("16 x 32" in backend(live)[2]) == (nc == "2")
    # get_state runs the updater step a row occluded in this frame has pending: rnn4 then steps on what the tail derived from this
    # frame's pose, behind a generic linear2 -- that row's rnn4 is no longer stage-1 arithmetic alone and is left out
    regime = live.get_trace()[:, 0]
    assert twin.get_trace()[:, 0].tolist() == regime.tolist() and (B == 1 or (regime == 0).sum() == 1)
    for n in ("rnn2", "rnn4"):
        rows = torch.ones(B, dtype=torch.bool) if n == "rnn2" else regime > 0
        (ha, ca), (hb, cb) = twin.get_state(n), live.get_state(n)
        assert torch.equal(ha[:, rows], hb[:, rows]) and torch.equal(ca[:, rows], cb[:, rows]), (n, first_difference(twin, live))
        assert float(ha[:, rows].abs().max()) > 0
