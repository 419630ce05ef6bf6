"""The timing interface of the gate-GEMM launcher (rc_gemm_api.cpp: rc_gemm_timing, rc_gemm_timing_read, rc_gemm_timing_busy), which feeds
the roofline pass of ``bench.py --full``.

Which launch a timing mode covers is decided in one place (timed_launch): mode 1 every gate-GEMM launch, mode 2 all but the launches of
the small-tile kernel, mode 3 only those of the shared-weight kernel. The counters of rc_get_launch_stats count the same launches untimed
(shared-weight | every launch that is not small), so the number of timed launches is pinned to them; and a timed run issues the launches of
an untimed one, so its results are the same bits."""
import math
import time

import numpy as np
import pytest
import torch

from robustcap_amd import synth
from robustcap_amd.net.sig_mp import Net

pytestmark = pytest.mark.gpu
T = 12

# batch, split products | what it exercises
#   8 fp32: every gate-GEMM launch on the small-tile kernels
#  64 split: the largest context below the shared-weight threshold
#  72 split: the smallest batch measured on the shared-weight kernel and the three-stream tick
CASES = [(8, 0), (64, 1), (72, 1)]


def _context(B):
    sd, body = synth.make_state_dict(0), synth.make_body(1)
    m = synth.make_motion(40 + B, B, T, body, conf="mixed")
    net = Net(body=body, batch=B)
    net.load_state_dict(sd)
    net.gravityc = torch.from_numpy(m["gravityc"])
    x4 = torch.from_numpy(np.random.default_rng(B).standard_normal((B, 171)).astype(np.float32))
    return net, m, x4


def _call(net, m, x4):
    """the call of every run: 12 mixed frames through rc_sequence with the default settings, then one rc_lstm_step on rnn4, from a reset state.
    Returns the outputs and the deltas of launch_stats() (shared-weight launches, other wide launches)."""
    t = torch.from_numpy
    net.reset_states()
    lds0, wide0 = net.launch_stats()
    pose, tran = net.forward_sequence(t(m["j2dc"]), t(m["accc"]), t(m["oric"]), first_frame=True)
    y = net.lstm_step("rnn4", x4)
    torch.cuda.synchronize()
    lds1, wide1 = net.launch_stats()
    return (pose.cpu(), tran.cpu(), y.cpu()), (lds1 - lds0, wide1 - wide0)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("B,split", CASES)
def test_timing_modes_count_the_launches_they_cover(B, split):
    net, m, x4 = _context(B)
    assert net.gemm_mode == split
    counted = {}
    for mode in (2, 3, 1):                                             # (mode 1 is compared with mode 2's count)
        ref, (lds, wide) = _call(net, m, x4)
        assert bool(torch.isfinite(ref[0]).all())
        assert (lds > 0) == (B == 72), (B, lds)                         # the shared-weight kernel runs in the case meant to cover it, and only there
        if B == 8:
            assert wide == 0, wide                                      # ... and batch 8 stays on the small-tile kernels
        net.gemm_timing(mode)
        t0 = time.perf_counter()
        out, stats = _call(net, m, x4)
        total_ms, launches = net.gemm_timing_read()
        wall_ms = (time.perf_counter() - t0) * 1e3
        busy_ms = net.gemm_timing_busy()
        print(f"batch {B} mode {mode}: lds {lds} wide {wide} | timed launches {launches}, total {total_ms:.4f} ms, busy {busy_ms:.4f} ms")
        assert _same(out, ref), f"mode {mode}: a timed run differs from the untimed one"
        assert stats == (lds, wide), (mode, stats, lds, wide)
        counted[mode] = launches
        if mode == 3:
            assert launches == lds, (launches, lds)
        elif mode == 2:
            assert launches == lds + wide, (launches, lds, wide)
        else:
            assert launches >= counted[2], (launches, counted[2])
            if B == 8:
                assert launches > 0
        if launches > 0:
            # busy is the length of the union of the intervals [t0, t0 + ms], total the sum of their ms: the union cannot be longer. Both are
            # float64 sums over end points below wall_ms, so each of the 2 * launches end points is off by at most 2^-52 * wall_ms, twice over.
            assert math.isfinite(total_ms) and math.isfinite(busy_ms)
            assert 0.0 < busy_ms <= total_ms + 4 * launches * wall_ms * 2.0 ** -52, (busy_ms, total_ms)
        else:
            assert total_ms == 0.0 and busy_ms == 0.0, (total_ms, busy_ms)
        assert net.gemm_timing_read() == (total_ms, launches)          # nothing new to read: the same pair
        net.gemm_timing(mode)                                           # switching a mode on starts from zero
        assert net.gemm_timing_read() == (0.0, 0)
        net.gemm_timing(0)
        again, stats = _call(net, m, x4)
        assert _same(again, ref) and stats == (lds, wide)
