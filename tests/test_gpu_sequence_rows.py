"""rc_sequence_rows / Net.forward_sequence(lengths=...): rows of different lengths in one call, without padding.

The yardstick is the uniform call: row b of a ragged call must leave, bit for bit, what rc_sequence(T = len[b]) leaves for that
row in a fresh context of the same batch and modes -- outputs of its frames, (h, c) of all six sub-nets, fusion state, trace --
on every engine; nothing past a row's end is read (NaN there) or written (a sentinel stays)."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

from oracle import sig_mp_oracle as O
from robustcap_amd import _lib, synth

pytestmark = pytest.mark.gpu
t = torch.from_numpy
GOLD = os.path.join(os.path.dirname(__file__), "golden")
NETS = ("rnn2", "rnn3", "rnn4", "rnn6", "rnn7", "rnn8")
SENTINEL = 12345.0
MIN_FRAMES = 8


def _net(assets, B, gemm, seq, params=None, resident=False):
    from robustcap_amd.net.sig_mp import Net
    n = Net(body=assets["body"], batch=B)
    n.load_state_dict(assets["state_dict"])
    n.set_gemm_mode(bool(gemm))
    n.set_sequence_mode(seq != 0, MIN_FRAMES, force=seq == 2)
    for k, v in (params or {}).items():
        setattr(n, k, v)
    if resident:
        n.set_resident(True)
    return n


def _dev(m, lo=None, hi=None):
    return tuple(t(m[k][:, lo:hi]).cuda().contiguous() for k in ("j2dc", "accc", "oric"))


def _call_rows(net, T, lens, ins, ft, first_frame, poison=True):
    """rc_sequence_rows through the raw ABI on caller-owned buffers: inputs past a row's end are NaN, outputs start as a sentinel."""
    B = net.batch
    j, a, o = (x.clone() for x in ins)
    if poison:
        for b in range(B):
            j[b, lens[b]:], a[b, lens[b]:], o[b, lens[b]:] = float("nan"), float("nan"), float("nan")
    pose = torch.full((B, T, 24, 3, 3), SENTINEL, device="cuda")
    tran = torch.full((B, T, 3), SENTINEL, device="cuda")
    ln = np.ascontiguousarray(np.asarray(lens, np.int32))
    ftd = None if ft is None else ft.cuda().float().contiguous()
    net._sync_gravity()
    rc = net._lib.rc_sequence_rows(net._ctx, T, ln.ctypes.data_as(C.c_void_p), _lib.ptr(j), T * 99, _lib.ptr(a), T * 18, _lib.ptr(o), T * 54,
                                   _lib.ptr(ftd), _lib.RC_FLAG_FIRST_FRAME if first_frame else 0, _lib.ptr(pose), T * 216, _lib.ptr(tran),
                                   T * 3, _lib.stream_ptr())
    _lib.check(net._ctx, rc, "rc_sequence_rows")
    torch.cuda.synchronize()
    return pose, tran


def _snapshot(net):
    """fusion state and trace first: rc_get_state runs a pending updater step (whose INPUTS the states then reflect)."""
    fus, tr = net.fusion_state().clone(), net.get_trace().clone()
    st = {n: tuple(x.clone() for x in net.get_state(n)) for n in NETS}
    return fus, tr, st


def _assert_row(b, got, want, what):
    gf, gt, gs = got
    wf, wt, ws = want
    assert torch.equal(gf[b], wf[b]), (what, b, "fusion state", gf[b].tolist(), wf[b].tolist())
    assert torch.equal(gt[b], wt[b]), (what, b, "trace", gt[b].tolist(), wt[b].tolist())
    for n in NETS:
        assert torch.equal(gs[n][0][:, b], ws[n][0][:, b]) and torch.equal(gs[n][1][:, b], ws[n][1][:, b]), (what, b, n)


def _motion(assets, B, T, lens, seed=5):
    """Mixed-confidence rows; by length class a row ending on an occluded frame, one ending on the frame where first_reach fires
    (the first frame at or above conf_hi) and one ending while it lags the batch (an occlusion a few frames before its end)."""
    m = synth.make_motion(seed, B, T, assets["body"], conf="mixed")
    m = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in m.items() if k in ("j2dc", "accc", "oric", "gravityc", "first_tran")}
    kinds = {}
    for b in range(B):
        L = int(lens[b])
        kind = kinds.setdefault(L, len(kinds) % 3)
        if L < 6:
            continue
        c = m["j2dc"][b, :, :, 2]
        if kind == 0:
            c[L - 1] = 0.2                                               # ends occluded: the updater step stays pending
        elif kind == 1:
            c[:L - 1] = np.minimum(c[:L - 1], 0.75)                      # never high before ...
            c[L - 1] = 0.95                                              # ... its last frame: init_net fires there
        else:
            c[L - 5:L - 3] = 0.2                                         # occluded, then visible again: the row lags 8 ticks at its end
            c[L - 3:L] = 0.95
    return m


def _lens_for(B, T):
    base = [T, 0, 1, T - 5, T - 9, T // 2]
    return [base[b % len(base)] for b in range(B)]


def _run_case(assets, B, gemm, seq, T=26, lens=None, first_frame=False, first_tran=False, preamble=0, resident=False, env=None, params=None, seed=5):
    lens = _lens_for(B, T) if lens is None else lens
    m = _motion(assets, B, preamble + T, [preamble + L for L in lens], seed)
    grav = t(m["gravityc"])
    ft = t(m["first_tran"]) if first_tran else None

    def fresh():
        n = _net(assets, B, gemm, seq, params, resident)
        n.gravityc = grav
        if preamble:
            n.forward_sequence(*_dev(m, 0, preamble), first_tran=t(m["first_tran"]))
        return n

    ins = _dev(m, preamble, preamble + T)
    net = fresh()
    before = net.sequence_row_frames()
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        pose, tran = _call_rows(net, T, lens, ins, ft, first_frame)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    assert net.sequence_row_frames() - before == sum(lens)
    got = _snapshot(net)
    for L in sorted(set(lens)):
        ref = fresh()
        if L > 0:
            rp, rt = ref.forward_sequence(*(x[:, :L] for x in ins), first_tran=ft, first_frame=first_frame)
            torch.cuda.synchronize()
        want = _snapshot(ref)
        for b in (b for b in range(B) if lens[b] == L):
            if L > 0:
                assert torch.equal(pose[b, :L], rp[b]) and torch.equal(tran[b, :L], rt[b]), (b, L)
            assert bool((pose[b, L:] == SENTINEL).all()) and bool((tran[b, L:] == SENTINEL).all()), (b, L)     # not written
            _assert_row(b, got, want, f"len {L}")
    return net, m, lens, pose, tran


@pytest.mark.parametrize("seq", [0, 1, 2])
@pytest.mark.parametrize("gemm", [0, 1])
@pytest.mark.parametrize("B", [1, 8, 48, 65, 256])
def test_rows_equal_uniform_calls_of_their_own_length(B, gemm, seq, synth_assets):
    if B == 1:
        for L in (1, 21):                                                # one row: every length is its own call (21: ends occluded)
            _run_case(synth_assets, 1, gemm, seq, lens=[L])
        return
    net, _, lens, _, _ = _run_case(synth_assets, B, gemm, seq)
    wave, stepped, _ = net.sequence_stats()
    assert wave + stepped == max(lens)                                   # frame indices, as for a uniform call
    assert (wave > 0) == (seq == 2) or seq == 1


@pytest.mark.parametrize("seq", [0, 2])
@pytest.mark.parametrize("B", [8, 65])
@pytest.mark.parametrize("start", ["first_frame", "first_tran"])
def test_first_frame_and_first_tran_leave_a_row_of_length_zero_alone(start, B, seq, synth_assets):
    """After a preamble call every row has state; the ragged call then starts with first_frame / first_tran, which must not touch the
    rows of length 0 (compared with a context that only ran the preamble) and apply to frame 0 of every other row."""
    _run_case(synth_assets, B, 1 if B >= 48 else 0, seq, T=20, first_frame=start == "first_frame", first_tran=start == "first_tran", preamble=6)


@pytest.mark.parametrize("seq", [0, 2])
@pytest.mark.parametrize("B,gemm", [(8, 0), (65, 1)])
def test_a_second_call_continues_every_row(B, gemm, seq, synth_assets):
    """Ragged call, then a call that gives every row its remaining frames == one uniform call of the full length: a pending updater
    step and first_reach survive a row's early end."""
    T = 30
    lens = [[T, 0, 1, T - 5, T - 9, T // 2][b % 6] for b in range(B)]
    m = _motion(synth_assets, B, T, lens, seed=9)
    grav = t(m["gravityc"])
    full = _net(synth_assets, B, gemm, seq)
    full.gravityc = grav
    fp, ftr = full.forward_sequence(*_dev(m))
    torch.cuda.synchronize()
    net = _net(synth_assets, B, gemm, seq)
    net.gravityc = grav
    ins = _dev(m)
    p1, t1 = _call_rows(net, T, lens, ins, None, False)
    rest = [T - L for L in lens]
    T2 = max(rest)
    ins2 = tuple(torch.zeros((B, T2) + tuple(x.shape[2:]), device="cuda") for x in ins)
    for b in range(B):
        for x2, x in zip(ins2, ins):
            x2[b, :rest[b]] = x[b, lens[b]:]
    p2, t2 = _call_rows(net, T2, rest, ins2, None, False)
    for b in range(B):
        assert torch.equal(torch.cat([p1[b, :lens[b]], p2[b, :rest[b]]]), fp[b]), b
        assert torch.equal(torch.cat([t1[b, :lens[b]], t2[b, :rest[b]]]), ftr[b]), b
    got, want = _snapshot(net), _snapshot(full)
    for b in range(B):
        _assert_row(b, got, want, "continued")
    assert net.sequence_row_frames() == B * T == full.sequence_row_frames()


@pytest.mark.parametrize("seq", [0, 2])
@pytest.mark.parametrize("B,gemm", [(8, 0), (65, 1)])
def test_a_uniform_call_and_a_single_step_follow_a_ragged_call(B, gemm, seq, synth_assets):
    """After a ragged call the context holds ended rows (flag bytes 0, an updater step left pending at an earlier frame than the other
    rows'): a plain rc_sequence and then an rc_step continue every row as they would after a uniform call of the row's own length."""
    T, K = 26, 9
    lens = _lens_for(B, T)
    m = _motion(synth_assets, B, T + K + 1, lens, seed=13)
    grav = t(m["gravityc"])
    ins, follow, one = _dev(m, 0, T), _dev(m, T, T + K), tuple(x[:, 0] for x in _dev(m, T + K, T + K + 1))

    def fresh():
        n = _net(synth_assets, B, gemm, seq)
        n.gravityc = grav
        return n

    net = fresh()
    _call_rows(net, T, lens, ins, None, False)
    p2, t2 = net.forward_sequence(*follow)
    p3, t3 = net.forward_batch(*one)
    torch.cuda.synchronize()
    got = _snapshot(net)
    for L in sorted(set(lens)):
        ref = fresh()
        if L > 0:
            ref.forward_sequence(*(x[:, :L] for x in ins))
        r2, q2 = ref.forward_sequence(*follow)
        r3, q3 = ref.forward_batch(*one)
        torch.cuda.synchronize()
        want = _snapshot(ref)
        for b in (b for b in range(B) if lens[b] == L):
            assert torch.equal(p2[b], r2[b]) and torch.equal(t2[b], q2[b]), (b, L, "rc_sequence after the ragged call")
            assert torch.equal(p3[b], r3[b]) and torch.equal(t3[b], q3[b]), (b, L, "rc_step after it")
            _assert_row(b, got, want, f"len {L}, continued")


@pytest.mark.parametrize("B,gemm", [(8, 0), (65, 1)])
def test_a_live_context_runs_ragged_calls(B, gemm, synth_assets):
    """Live contexts (rc_params.live: landmark refresh counter, no plan) always take the frame-stepped launches."""
    net, _, lens, _, _ = _run_case(synth_assets, B, gemm, 2, params={"live": True})
    assert net.sequence_stats()[0] == 0 and net.sequence_stats()[1] == max(lens)


@pytest.mark.parametrize("B,gemm", [(8, 0), (65, 1)])
def test_a_ragged_call_planned_in_pieces(B, gemm, synth_assets):
    net, _, lens, _, _ = _run_case(synth_assets, B, gemm, 2, T=30, env={"RC_SEQ_MAX_PLAN_FRAMES": "8"})
    assert net.sequence_stats()[0] + net.sequence_stats()[1] == max(lens)


@pytest.mark.parametrize("B", [65, 256])
def test_resident_engine_runs_ragged_calls(B, synth_assets):
    net, _, _, _, _ = _run_case(synth_assets, B, 1, 2, resident=True)
    segments, aborts = net.resident_stats()
    assert segments >= 1 and aborts == 0


@pytest.mark.parametrize("resident", [False, True])
def test_alternating_occlusion_outgrows_the_reserved_table(resident, synth_assets):
    """Rows occluded on every other frame wait TAIL + 1 ticks after each: the plan has more ticks than the B x (T + 64) table entries
    reserved for a call of T frames, ragged or not, so the table is regrown inside the call (tests/test_wave_plan.py has the host side)."""
    B, T = 72, 40
    lens = [[T, T - 7, T // 2][b % 3] for b in range(B)]
    m = synth.make_motion(3, B, T, synth_assets["body"], conf="high")
    m = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in m.items() if k in ("j2dc", "accc", "oric", "gravityc")}
    m["j2dc"][1::4, 0::2, :, 2] = 0.2
    grav = t(m["gravityc"])
    ins = _dev(m)
    net = _net(synth_assets, B, 1, 2, resident=resident)
    net.gravityc = grav
    pose, tran = _call_rows(net, T, lens, ins, None, False)
    assert net.sequence_stats()[2] > T + 64
    got = _snapshot(net)
    for L in sorted(set(lens)):
        ref = _net(synth_assets, B, 1, 2, resident=resident)
        ref.gravityc = grav
        rp, rt = ref.forward_sequence(*(x[:, :L] for x in ins))
        want = _snapshot(ref)
        for b in (b for b in range(B) if lens[b] == L):
            assert torch.equal(pose[b, :L], rp[b]) and torch.equal(tran[b, :L], rt[b]), (b, L)
            _assert_row(b, got, want, f"len {L}")
    if resident:
        assert net.resident_stats()[0] >= 1 and net.resident_stats()[1] == 0


def test_work_saved_without_a_clock(synth_assets):
    """64 all-visible rows, half of T frames, half of T / 4: the engine launches the planner's ticks (those of the longest row) and
    computes sum(len) row-frames; the padded call computes B * T."""
    B, T = 64, 64
    lens = [T if b < B // 2 else T // 4 for b in range(B)]
    m = synth.make_motion(4, B, T, synth_assets["body"], conf="high")
    m = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in m.items() if k in ("j2dc", "accc", "oric", "gravityc")}
    ins = _dev(m)
    net = _net(synth_assets, B, 1, 2)
    net.gravityc = t(m["gravityc"])
    mean = torch.empty(B * T, dtype=torch.float32, device="cuda")
    code = torch.empty(B * T, dtype=torch.int8, device="cuda")
    _lib.check(None, net._lib.rc_conf_mean(_lib.ptr(ins[0]), B * T, net.conf_range[0], net.conf_range[1], _lib.ptr(mean), _lib.ptr(code),
                                           _lib.stream_ptr()), "rc_conf_mean")
    torch.cuda.synchronize()
    codes = np.ascontiguousarray(code.cpu().numpy().reshape(B, T).T)     # frame-major
    assert (codes == 2).all()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ln, fr, pd = np.asarray(lens, np.int32), np.ones(B, np.int32), np.zeros(B, np.int32)
    nt, npre = C.c_int32(), C.c_int32()
    net._lib.rc_plan_wave_rows(p(codes), B, T, 0, p(ln), p(fr), p(pd), 1, 1, None, 0, C.byref(nt), C.byref(npre), None, None)
    _call_rows(net, T, lens, ins, None, False)
    wave, stepped, ticks = net.sequence_stats()
    assert (wave, stepped) == (T, 0) and ticks == nt.value
    assert net.sequence_row_frames() == sum(lens)
    padded = _net(synth_assets, B, 1, 2)
    padded.gravityc = t(m["gravityc"])
    padded.forward_sequence(*ins)
    assert padded.sequence_row_frames() == B * T and padded.sequence_stats()[2] == ticks      # same ticks: the longest row sets them


def test_invalid_lengths(synth_assets):
    B, T = 4, 10
    m = _motion(synth_assets, B, T, [T] * B)
    net = _net(synth_assets, B, 0, 2)
    net.gravityc = t(m["gravityc"])
    ins = _dev(m)
    before = _snapshot(net)
    for bad in ([T, T, -1, 3], [T + 1, 0, 0, 0]):
        with pytest.raises(_lib.RobustcapLibraryError):
            _call_rows(net, T, bad, ins, None, False, poison=False)
        with pytest.raises(ValueError):
            net.forward_sequence(*ins, lengths=bad)
    rc = net._lib.rc_sequence_rows(net._ctx, T, None, _lib.ptr(ins[0]), T * 99, _lib.ptr(ins[1]), T * 18, _lib.ptr(ins[2]), T * 54, None, 0,
                                   _lib.ptr(ins[0]), T * 216, _lib.ptr(ins[1]), T * 3, _lib.stream_ptr())
    assert rc == -1
    assert net.sequence_row_frames() == 0 and net.sequence_stats() == (0, 0, 0)               # nothing enqueued
    after = _snapshot(net)
    for b in range(B):
        _assert_row(b, after, before, "invalid")
    p, tr = net.forward_sequence(*ins, lengths=torch.tensor([T, 0, 3, T]))                    # an int tensor is accepted
    assert p.shape == (B, T, 24, 3, 3) and tr.shape == (B, T, 3)


# ---- reference parity: the captured fixtures as rows of ONE ragged call ---------------------------------------------------------
NONLIVE = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLD, "seq_*.npz")) if "live" not in os.path.basename(p))


def _groups():
    """Switches, first_frame and first_tran belong to the context / the call: fixtures that share them share a call."""
    g = {}
    for name in NONLIVE:
        s = np.load(os.path.join(GOLD, name))
        key = tuple(bool(s[k]) for k in ("use_flat_floor", "use_reproj_opt", "use_vision_updater", "use_imu_updater", "first_frame")) + (s["first_tran"].size > 0,)
        g.setdefault(key, []).append(name)
    return sorted(g.items())


def _joints(body, pose, tran):
    return O.OracleBody(body).forward_kinematics(pose.cpu().float(), tran.cpu().float())[1]


@pytest.mark.parametrize("gemm,seq", [(0, 0), (0, 2), (1, 0), (1, 2)])
@pytest.mark.parametrize("group", range(len(_groups())), ids=["+".join(n[4:-4] for n in names) for _, names in _groups()])
def test_fixtures_as_rows_of_one_ragged_call(group, gemm, seq, synth_assets):
    key, names = _groups()[group]
    flat, reproj, vup, imu, first_frame, has_ft = key
    params = dict(use_flat_floor=flat, use_reproj_opt=reproj, use_vision_updater=vup, use_imu_updater=imu)
    fx = [np.load(os.path.join(GOLD, n)) for n in names]
    lens, seen = [], {}
    for s in fx:                                                         # equally long fixtures: cut the later ones short (prefix parity)
        L = s["pose"].shape[0]
        k = seen.get(L, 0)
        seen[L] = k + 1
        lens.append(L - 5 * k)
    B = 8
    T = max(lens) + 3
    rows = list(range(1, 1 + len(fx)))                                   # fixtures in rows 1.., synthetic rows around them
    all_lens = [T - 2] * B
    m = synth.make_motion(21, B, T, synth_assets["body"], conf="mixed")
    m = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in m.items() if k in ("j2dc", "accc", "oric", "gravityc", "first_tran")}
    for r, s, L in zip(rows, fx, lens):
        all_lens[r] = L
        for k in ("j2dc", "accc", "oric"):
            m[k][r, :L] = s[k][:L]
        m["gravityc"][r] = s["gravityc"].reshape(-1)[:3]
        if has_ft:
            m["first_tran"][r] = s["first_tran"].reshape(-1)[:3]
    all_lens[0] = 0
    net = _net(synth_assets, B, gemm, seq, params)
    net.gravityc = t(m["gravityc"])
    ft = t(m["first_tran"]) if has_ft else None
    pose, tran = _call_rows(net, T, all_lens, _dev(m), ft, first_frame)
    trace = net.get_trace()
    for r, s, L, name in zip(rows, fx, lens, names):
        rp, rt = t(s["pose"][:L]), t(s["tran"][:L])
        p, tr = pose[r, :L].cpu(), tran[r, :L].cpu()
        assert float((tr - rt).abs().max()) <= 1e-4, name
        assert float(O.rotation_angle_deg(p, rp).max()) <= 0.1, name
        assert float((_joints(synth_assets["body"], p, tr) - _joints(synth_assets["body"], rp, rt)).abs().max()) <= 1e-4, name
        # ... and bitwise the fixture's own batch-1 run in the same mode (whose prefix is the run of the prefix)
        one = _net(synth_assets, 1, gemm, seq, params)
        one.gravityc = t(s["gravityc"])
        op, ot = one.forward_sequence(t(s["j2dc"][None, :L]), t(s["accc"][None, :L]), t(s["oric"][None, :L]),
                                      first_tran=t(s["first_tran"]).view(1, 3) if has_ft else None, first_frame=first_frame)
        assert torch.equal(op[0].cpu(), p) and torch.equal(ot[0].cpu(), tr), name
        assert one.get_trace()[0].tolist() == trace[r].tolist(), name                       # regime and branch trace of the last frame: exact
        tc, exp = trace[r].tolist(), s["trace"][L - 1]                                      # ... and the reference's, at the row's last frame
        assert tc[0] == int(O.fixture_regimes(s)[L - 1]), name
        assert tc[1] == int(exp[1]) and tc[2] == int(exp[2]) and tc[3] == int(exp[4]) and tc[4] == int(exp[5]), (name, tc, exp.tolist())


def test_run_dataset_ragged_equals_padded(synth_assets):
    from robustcap_amd import evaluate as ev
    body, sd = synth_assets["body"], synth_assets["state_dict"]
    ds = synth.make_dataset(6, 3, 40, body, n_cam=2)
    for i, n in ((1, 30), (2, 11)):                                      # unequal sequence lengths
        for k in ("pose", "tran", "imu_ori", "imu_acc"):
            ds[k][i] = ds[k][i][:n]
        ds["joint2d_mp"][i] = ds["joint2d_mp"][i][:, :n]
    padded = ev.run_dataset(ds, sd, body)
    ragged = ev.run_dataset(ds, sd, body, ragged=True)
    assert sorted(padded) == sorted(ragged) and len(ragged) == 6
    for k in padded:
        assert ragged[k][0].shape == padded[k][0].shape
        assert torch.equal(ragged[k][0], padded[k][0]) and torch.equal(ragged[k][1], padded[k][1]), k
