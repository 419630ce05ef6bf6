"""Every captured non-live reference sequence as ONE ROW of a batched context, on the kernels that carry the FLOPs there.

The ABI promises that within one product arithmetic a row's result does not depend on the batch, the tile shape or the engine,
bitwise (include/robustcap_hip.h, rc_set_gemm_mode). Here the fixture sits at a chosen row of a context whose other rows are
seeded motions of their own, on the wavefront engine (sequence mode 2) with the split-bf16 products:
  (48, 47)    rc_gemm_split48_w32_kernel (contexts of 33-64 rows), the fixture in the last row
  (65, 64)    the smallest context on rc_gemm_lds_kernel, the fixture in its last row
  (256, 17)   a full 256-row tile of rc_gemm_lds_kernel, mixed and all-visible filler
  (257, 256)  a second 256-row block holding one valid row: the fixture
The row must be bitwise the batch-1 split-mode run of the fixture, and within 1e-4 m / 0.1 deg of the REFERENCE's outputs
(guard: 1e-5 m, about four times what the kernels show today)."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import sig_mp_oracle as O
from robustcap_amd import synth

pytestmark = pytest.mark.gpu
t = torch.from_numpy
GOLD = os.path.join(os.path.dirname(__file__), "golden")
NONLIVE = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLD, "seq_*.npz")) if "live" not in os.path.basename(p))
CONTEXTS = [(48, 47, "mixed"), (65, 64, "high"), (256, 17, "mixed"), (256, 17, "high"), (257, 256, "high")]
NETS = ("rnn2", "rnn3", "rnn4", "rnn6", "rnn7", "rnn8")
_cache = {}


def _net(assets, s, B, seq=True):
    from robustcap_amd.net.sig_mp import Net
    net = Net(body=assets["body"], batch=B)
    net.load_state_dict(assets["state_dict"])
    for k in ("use_flat_floor", "use_reproj_opt", "use_vision_updater", "use_imu_updater"):
        setattr(net, k, bool(s[k]))
    net.set_sequence_mode(seq, 8, force=True)
    return net


def _run(net, j2dc, accc, oric, ft, ff, row):
    p, tr = net.forward_sequence(t(j2dc), t(accc), t(oric), first_tran=ft, first_frame=ff)
    torch.cuda.synchronize()
    states = {n: tuple(x[:, row].clone() for x in net.get_state(n)) for n in NETS}
    return p[row].cpu(), tr[row].cpu(), states, net.get_trace()[row].clone()


def _single(assets, name):
    """batch-1 split-mode forward_sequence of the fixture (cached per module)"""
    if name not in _cache:
        s = np.load(os.path.join(GOLD, name))
        net = _net(assets, s, 1)
        net.set_gemm_mode(True)
        net.gravityc = t(s["gravityc"])
        ft = t(s["first_tran"]).view(1, 3) if s["first_tran"].size else None
        _cache[name] = _run(net, s["j2dc"][None], s["accc"][None], s["oric"][None], ft, bool(s["first_frame"]), 0)
        del net
    return _cache[name]


def _context(assets, s, B, row, filler):
    T = int(s["pose"].shape[0])
    key = ("filler", T, filler)
    if key not in _cache:
        _cache[key] = synth.make_motion(1000 + T, 32, T, assets["body"], conf=filler)
    mu = _cache[key]
    rep = (B + 31) // 32
    m = {k: np.concatenate([v] * rep, 0)[:B].copy() for k, v in mu.items()}
    for k in ("j2dc", "accc", "oric", "gravityc"):
        m[k][row] = s[k]
    ft = None
    if s["first_tran"].size:
        ft = t(m["first_tran"].copy())
        ft[row] = t(s["first_tran"])
    return m, ft


@pytest.mark.parametrize("B,row,filler", CONTEXTS, ids=[f"b{b}_row{r}_{f}" for b, r, f in CONTEXTS])
@pytest.mark.parametrize("name", NONLIVE, ids=[n[4:-4] for n in NONLIVE])
def test_fixture_row_of_a_batched_context(name, B, row, filler, synth_assets):
    s = np.load(os.path.join(GOLD, name))
    m, ft = _context(synth_assets, s, B, row, filler)
    modes = (True, False) if (B, row, filler) == (256, 17, "mixed") else (True,)
    ob = O.OracleBody(synth_assets["body"])
    rp, rt = t(s["pose"]), t(s["tran"])
    jr = ob.forward_kinematics(rp, rt)[1]
    sp, st, ss, strace = _single(synth_assets, name)
    for seq in modes:
        net = _net(synth_assets, s, B, seq)
        assert net.gemm_mode == 1                                        # batches from 48 rows: the split products by default
        net.gravityc = t(m["gravityc"])
        p, tr, states, trace = _run(net, m["j2dc"], m["accc"], m["oric"], ft, bool(s["first_frame"]), row)
        lds, _ = net.launch_stats()
        kernel = net.gemm_kernel_name()
        engine = net.sequence_stats()[0]
        del net
        if seq:
            assert engine == p.shape[0] - int(bool(s["first_frame"]) or s["first_tran"].size > 0)
        assert kernel == ("rc_gemm_split48_w32_kernel" if B < 65 else "rc_gemm_lds_kernel"), kernel
        assert (lds > 0) == (B >= 65), lds
        # the ABI's promise: the row is the batch-1 run, bit for bit
        which = f"batch {B} row {row} ({kernel}, sequence mode {2 if seq else 0}) vs batch 1"
        assert torch.equal(tr, st), f"{which}: translation differs by {float((tr - st).abs().max()):.3e}"
        assert torch.equal(p, sp), f"{which}: pose differs by {float((p - sp).abs().max()):.3e}"
        assert torch.equal(trace, strace), which
        for n in NETS:
            assert torch.equal(states[n][0], ss[n][0]) and torch.equal(states[n][1], ss[n][1]), f"{which}: state of {n}"
        # against the reference
        jd = float((ob.forward_kinematics(p, tr)[1] - jr).abs().max())
        dt = float((tr - rt).abs().max())
        assert dt <= 1e-4 and jd <= 1e-4
        assert float(O.rotation_angle_deg(p, rp).max()) <= 0.1
        assert dt <= 1e-5 and jd <= 1e-5, f"regression: tran {dt:.2e} m, joints {jd:.2e} m"
        for n in NETS:
            assert float((states[n][0] - t(s["h_" + n])).abs().max()) <= 1e-4, n
            assert float((states[n][1] - t(s["c_" + n])).abs().max()) <= 2e-4, n
