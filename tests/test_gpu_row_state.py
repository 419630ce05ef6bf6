"""Row state on the GPU: rc_save_rows / rc_load_rows / rc_set_state (include/robustcap_hip.h) and Net.save_rows / load_rows / set_state.

The yardstick is the project's strictest: a row saved in one context and loaded into ANOTHER row of a context of ANOTHER batch size, whose
own step counters stand elsewhere, continues BIT FOR BIT like the row it was taken from -- outputs, (h, c) of all six sub-nets, fusion
state and trace -- because a row's bits depend neither on the batch, the tile shape or the engine. Every comparison here is on bits.

Engines (rc_set_sequence_mode, as tests/test_gpu_sequence_rows.py forces them): "stepped" = mode 0, the frame-stepped launches; "planned" =
mode 1, the planner on -- frame-stepped frames run without the transition launches where the plan proves every row visible, the all-visible
path -- and "wave" = mode 2, the wavefront engine forced. The resident engine is never enabled.

The fenced side-stream cases of rc_save_rows / rc_load_rows live here and not in tests/test_gpu_stream_order.py: the two entries carry their
stream inside rc_row_io (see the header), so that table does not list them."""
import ctypes as C
import gc
import io
import os
import struct

import numpy as np
import pytest
import torch

import stream_fence as F
from oracle import live_exact as X
from oracle import sig_mp_oracle as O
from robustcap_amd import _lib, synth
from robustcap_amd.rowstate import HIDDEN, RowState

pytestmark = pytest.mark.gpu
t = torch.from_numpy
GOLD = os.path.join(os.path.dirname(__file__), "golden")
NETS = ("rnn2", "rnn3", "rnn4", "rnn6", "rnn7", "rnn8")
MIN_FRAMES = 8
ENGINES = {"stepped": 0, "planned": 1, "wave": 2}
# (gemm mode, engine): mode 1 -- what a context of 65 rows runs by default -- on every engine, modes 0 and 2 on the wavefront engine
MODES = [(1, "stepped"), (1, "planned"), (1, "wave"), (0, "wave"), (2, "wave")]
MODE_IDS = [f"gemm{g}_{e}" for g, e in MODES]
KEYS = ("j2dc", "accc", "oric")


@pytest.fixture(autouse=True)
def _leave_nothing_behind():
    """Every context a test made is released with the test (contexts left alive have changed what later modules see)."""
    yield
    gc.collect()
    torch.cuda.synchronize()


@pytest.fixture(scope="module", autouse=True)
def _give_the_memory_back():
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _net(assets, B, gemm=None, engine="stepped", params=None, sd=None):
    from robustcap_amd.net.sig_mp import Net
    n = Net(body=assets["body"], batch=B)
    n.load_state_dict(assets["state_dict"] if sd is None else sd)
    if gemm is not None:
        n.set_gemm_mode(int(gemm))
        assert n.gemm_mode == int(gemm)
    seq = ENGINES[engine]
    n.set_sequence_mode(seq != 0, MIN_FRAMES, force=seq == 2)
    for k, v in (params or {}).items():
        setattr(n, k, v)
    return n


def _motion(assets, seed, B, T, conf="mixed"):
    m = synth.make_motion(seed, B, T, assets["body"], conf=conf)
    return {k: np.ascontiguousarray(m[k], dtype=np.float32) for k in KEYS + ("gravityc",)}


def _dev(m, lo=None, hi=None):
    return tuple(t(np.ascontiguousarray(m[k][:, lo:hi])).cuda() for k in KEYS)


def _snapshot(net):
    """fusion state and trace first: rc_get_state runs a pending updater step (tests/test_gpu_sequence_rows.py)"""
    fus, tr = net.fusion_state().clone(), net.get_trace().clone()
    st = {n: tuple(x.clone() for x in net.get_state(n)) for n in NETS}
    return fus, tr, st


def _same(a, b):
    return F.same_bits(a, b)


def _assert_rows(got, rg, want, rw, what):
    """row rg of one snapshot is row rw of the other, on bits"""
    (gf, gt, gs), (wf, wt, ws) = got, want
    assert torch.equal(gf[rg], wf[rw]), (what, rg, rw, "fusion state", gf[rg].tolist(), wf[rw].tolist())
    assert torch.equal(gt[rg], wt[rw]), (what, rg, rw, "trace", gt[rg].tolist(), wt[rw].tolist())
    for n in NETS:
        for k, name in enumerate(("h", "c")):
            assert _same(gs[n][k][:, rg], ws[n][k][:, rw]), (what, rg, rw, n, name)


def _run(net, ins, lengths=None):
    p, tr = net.forward_sequence(*ins, lengths=lengths)
    torch.cuda.synchronize()
    return p, tr


# ------------------------------------------------------------------------------------------------------------------ 1. continuation
T1, T2 = 14, 8
SRC_B = 33
SAVED = (15, 16, 31, 32, 20, 7)                # 15 | 16: the rc_pk 16-row block edge; 31 | 32: the last row in front of the Bp padding
# (destination batch, destination rows, the records they take -- indices into SAVED): permuted everywhere
DESTS = [(1, [0], [0]), (5, [4, 0, 2], [3, 1, 2]), (65, [64, 15, 16, 3, 33, 48], [5, 4, 3, 2, 1, 0])]
PRE = 6                                         # frames of other data every destination has run before the load


def _script(assets):
    """33 rows, T1 + T2 frames. Lengths of the first call: the saved rows' counters of the nets that step on every frame stand at 12, 13
    and 14 -- 0, 1 and 2 mod RC_HBUF -- and at 0 (row 7 has not started). Row 15 ends on an occluded frame: its updater step stays pending
    and its rnn4 / rnn6 counters are one behind the other nets'. Rows 16 and 20 are all-visible at high confidence and hold floor samples.
    Row 31 never reaches conf_hi before the save (first_reach has not fired) and does right after it. Row 32 had an occlusion on the way."""
    m = _motion(assets, 41, SRC_B, T1 + T2)
    c = m["j2dc"][..., 2]
    lens = np.asarray([T1 - (b % 3) for b in range(SRC_B)], np.int32)
    lens[15], lens[16], lens[31], lens[32], lens[20], lens[7] = 12, 13, 14, 13, 14, 0
    c[15, 11] = 0.2
    c[16], c[20] = 0.95, 0.95
    c[31, :T1] = np.minimum(c[31, :T1], 0.75)
    c[31, T1:] = 0.95
    c[32, 5:8] = 0.2
    rest = {k: np.stack([m[k][b, lens[b]:lens[b] + T2] for b in range(SRC_B)]) for k in KEYS}
    return m, lens, rest


def _dest_lengths(B):
    return [2 + (b % 4) for b in range(B)]     # unequal, and unequal mod RC_HBUF; mixed confidences move rnn4 / rnn6 apart from the others


@pytest.mark.parametrize("gemm,engine", MODES, ids=MODE_IDS)
def test_restored_rows_continue_bit_for_bit_in_contexts_of_other_sizes(gemm, engine, synth_assets):
    m, lens, rest = _script(synth_assets)
    grav = t(m["gravityc"])
    saved = list(SAVED)
    # the source: first call, save, then the remaining frames of every row
    src = _net(synth_assets, SRC_B, gemm, engine)
    src.gravityc = grav
    _run(src, _dev(m, 0, T1), lengths=lens)
    if engine != "planned":                                                # (the planner chooses by its cost estimate)
        assert (src.sequence_stats()[0] > 0) == (engine == "wave"), (engine, src.sequence_stats())
    state = src.save_rows(saved)
    fus0, trace0 = src.fusion_state().clone(), src.get_trace().clone()        # read after the save (they change nothing)
    assert fus0[15, 4] == 1, "row 15 must end with its updater step pending"
    assert (fus0[saved, 1] > 0).any() and fus0[16, 1] > 0, ("floor samples held", fus0[saved, 1].tolist())
    assert fus0[31, 2] == 1 and fus0[7, 2] == 1 and fus0[7, 0] == 0, "row 31 before first_reach, row 7 not started"
    assert sorted({int(lens[b]) % 3 for b in saved}) == [0, 1, 2]
    host = state.cpu()
    assert len(host) == len(saved) and host.bytes_per_row == src.row_state_info()[0]
    rest_dev = tuple(t(rest[k]).cuda() for k in KEYS)
    p2, t2 = _run(src, rest_dev)
    snap_src = _snapshot(src)
    # the uninterrupted run: one call of every row's full length
    un = _net(synth_assets, SRC_B, gemm, engine)
    un.gravityc = grav
    pu, tu = _run(un, _dev(m), lengths=lens + T2)
    snap_un = _snapshot(un)
    for b in saved:
        L = int(lens[b])
        assert _same(p2[b], pu[b, L:L + T2]) and _same(t2[b], tu[b, L:L + T2]), ("the source's own continuation", b)
        _assert_rows(snap_src, b, snap_un, b, "source vs uninterrupted")
    del un
    # the destinations
    for Bd, rows, recs in DESTS:
        fm = _motion(synth_assets, 100 + Bd, Bd, PRE + T2)
        d = _net(synth_assets, Bd, gemm, engine)
        d.gravityc = t(fm["gravityc"])
        _run(d, _dev(fm, 0, PRE), lengths=_dest_lengths(Bd))
        d.load_rows(host[recs], rows=rows)
        fus, trace = d.fusion_state(), d.get_trace()
        x = [v.clone() for v in _dev(fm, PRE, PRE + T2)]
        for r, k in zip(rows, recs):
            b = saved[k]
            assert torch.equal(fus[r], fus0[b]) and torch.equal(trace[r], trace0[b]), (Bd, r, b, "fusion state / trace right after the load")
            for xi, ri in zip(x, rest_dev):
                xi[r] = ri[b]
        pd, td = _run(d, tuple(x))
        snap = _snapshot(d)
        for r, k in zip(rows, recs):
            b, L = saved[k], int(lens[saved[k]])
            what = f"batch {Bd} row {r} <- row {b}"
            assert _same(pd[r], p2[b]) and _same(td[r], t2[b]), (what, "outputs vs the continued source")
            assert _same(pd[r], pu[b, L:L + T2]) and _same(td[r], tu[b, L:L + T2]), (what, "outputs vs the uninterrupted run")
            _assert_rows(snap, r, snap_src, b, what + " vs the continued source")
            _assert_rows(snap, r, snap_un, b, what + " vs the uninterrupted run")
        del d
    gc.collect()


# ------------------------------------------------------------------------------------------------------------------ 2. neighbours
@pytest.mark.parametrize("engine", list(ENGINES))
def test_a_load_leaves_the_other_rows_bitwise_alone(engine, synth_assets):
    fm = _motion(synth_assets, 51, 5, 9)
    d = _net(synth_assets, 5, None, engine)
    d.gravityc = t(fm["gravityc"])
    _run(d, _dev(fm), lengths=[9, 8, 0, 9, 4])
    sm = _motion(synth_assets, 52, 3, 8)
    sm["j2dc"][0, 7, :, 2] = 0.2                                            # record 1 (row 0) carries a pending step,
    sm["j2dc"][2, 7, :, 2] = 0.9                                            # record 0 (row 2) none
    src = _net(synth_assets, 3, None, engine)
    src.gravityc = t(sm["gravityc"])
    _run(src, _dev(sm))
    recs = src.save_rows([2, 0])
    before = d.save_rows()
    d.load_rows(recs, rows=[3, 1])
    after = d.save_rows()
    torch.cuda.synchronize()
    assert not _same(before.data[3], after.data[3]) and not _same(before.data[1], after.data[1])
    for r in (0, 2, 4):
        assert _same(before.data[r], after.data[r]), ("a row that was not listed changed", r)
    assert _same(after.data[3], recs.data[0]) and _same(after.data[1], recs.data[1])
    assert d.fusion_state()[1, 4] == 1 and d.fusion_state()[3, 4] == 0


# ------------------------------------------------------------------------------------------------------------------ 3. round trips
def _plant(rec):
    """a copy of one record [bytes] with a quiet NaN with a payload, a signalling NaN, -0.0 and a denormal among its first hidden units"""
    rec = rec.clone()
    for k, word in enumerate((0x7FC00001, 0x7F800001, 0x80000000, 0x00000001)):
        rec[8 * k:8 * k + 4] = torch.tensor(list(struct.pack("<I", word)), dtype=torch.uint8)
    return rec


@pytest.mark.parametrize("gemm,engine", MODES, ids=MODE_IDS)
def test_round_trip_through_host_and_torch_save_is_a_direct_load(gemm, engine, synth_assets):
    sm = _motion(synth_assets, 61, 4, 9)
    sm["j2dc"][1, 8, :, 2] = 0.2
    src = _net(synth_assets, 4, gemm, engine)
    src.gravityc = t(sm["gravityc"])
    _run(src, _dev(sm))
    st = src.save_rows()
    torch.cuda.synchronize()
    # regrouping on the device
    assert _same(RowState.cat([st[[2, 0]], st[1]]).data, st.data[[2, 0, 1]]) and _same(st[3].data, st.data[3:4])
    assert _same(st[1:3].data, st.data[1:3])
    # five records: the four rows and a copy of row 1 with NaN and -0.0 planted
    planted = RowState(_plant(st.data[1].cpu())[None], st.format)
    five = RowState.cat([st.cpu(), planted])
    f = io.BytesIO()
    torch.save(five.state_dict(), f)
    f.seek(0)
    back = RowState.from_state_dict(torch.load(f, weights_only=True))
    assert _same(back.data, five.data) and back.device.type == "cpu"
    fm = _motion(synth_assets, 62, 5, PRE + T2)
    outs = []
    for state in (five.to("cuda"), back):                                   # the direct load; the load of what came back from the file
        d = _net(synth_assets, 5, gemm, engine)
        d.gravityc = t(fm["gravityc"])
        _run(d, _dev(fm, 0, PRE), lengths=_dest_lengths(5))
        d.load_rows(state, rows=[4, 2, 0, 1, 3])
        now = d.save_rows()
        p, tr = _run(d, _dev(fm, PRE, PRE + T2))
        outs.append((now.data.clone(), p, tr, d.save_rows().data.clone()))
        del d
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert _same(a, b)
    assert _same(outs[0][0][[4, 2, 0, 1, 3]].cpu(), five.data), "what a load writes is what a save reads, NaN payloads and -0.0 included"
    # rows 4, 2, 0, 1 continue src's rows 0 .. 3; row 3 holds the planted copy of row 1: NaN spreads there and nowhere else
    p, tr = outs[0][1], outs[0][2]
    p2, t2 = _run(src, tuple(v[[4, 2, 0, 1]].contiguous() for v in _dev(fm, PRE, PRE + T2)))      # src row b gets what its copy's row got
    for r, b in ((4, 0), (2, 1), (0, 2), (1, 3)):
        assert _same(p[r], p2[b]) and _same(tr[r], t2[b]), (r, b)
    assert bool(torch.isfinite(p[[4, 2, 0, 1]]).all())


# ------------------------------------------------------------------------------------------------------------------ 5. a fixture, cut in two
FIXTURE = "seq_firstframe_low.npz"


@pytest.mark.parametrize("engine", list(ENGINES))
def test_reference_fixture_cut_in_two_is_the_uncut_run(engine, synth_assets):
    s = np.load(os.path.join(GOLD, FIXTURE))
    T = int(s["pose"].shape[0])
    assert not str(s["live"]) and s["first_tran"].size == 0 and bool(s["first_frame"])
    params = {k: bool(s[k]) for k in ("use_flat_floor", "use_reproj_opt", "use_vision_updater", "use_imu_updater")}
    conf = s["j2dc"][:, :, 2].astype(np.float64).mean(1)
    # the last frame with an occluded frame in front of it: that frame's updater step is pending at the cut, and the second half opens with
    # the transition step of a row that sees the camera again
    pend_cut = max(k for k in range(2, T - 2) if conf[k - 1] < 0.65 and k != T // 2)
    assert conf[pend_cut] > 0.75
    cuts = (1, T // 2, pend_cut)
    ins = tuple(t(np.ascontiguousarray(s[k][None])).cuda() for k in KEYS)
    grav = t(s["gravityc"])

    def part(net, lo, hi, row=0, B=1, filler=None):
        x = tuple(v[:, lo:hi] for v in ins)
        if B > 1:
            x = tuple(f.clone() for f in filler)
            for xi, v in zip(x, ins):
                xi[row] = v[0, lo:hi]
        p, tr = net.forward_sequence(*x, first_frame=(lo == 0))
        torch.cuda.synchronize()
        return p[row].cpu(), tr[row].cpu()

    whole = _net(synth_assets, 1, None, engine, params)
    whole.gravityc = grav
    wp, wt = part(whole, 0, T)
    want = _snapshot(whole)
    # within the project's own bounds of the reference's captured outputs (tests/test_gpu_fixture_in_batch.py)
    ob = O.OracleBody(synth_assets["body"])
    rp, rt = t(s["pose"]), t(s["tran"])
    jr = ob.forward_kinematics(rp, rt)[1]
    a = _net(synth_assets, 1, None, engine, params)
    a.gravityc = grav
    b = _net(synth_assets, 3, None, engine, params)
    fm = _motion(synth_assets, 71, 3, T)
    b.gravityc = t(fm["gravityc"])
    for n, cut in enumerate(cuts):
        if n:
            a.reset_states()
        p1, t1 = part(a, 0, cut)
        fus = a.fusion_state()
        if cut == pend_cut:
            assert fus[0, 4] == 1, "the third cut must carry a pending step"
        b.load_rows(a.save_rows().cpu(), rows=[2])
        filler = tuple(v[:, cut:].contiguous() for v in _dev(fm))
        p2, t2 = part(b, cut, T, row=2, B=3, filler=filler)
        p, tr = torch.cat([p1, p2]), torch.cat([t1, t2])
        assert _same(p, wp) and _same(tr, wt), (engine, "cut at", cut)
        _assert_rows(_snapshot(b), 2, want, 0, f"cut at {cut}")
        assert float((tr - rt).abs().max()) <= 1e-4 and float((ob.forward_kinematics(p, tr)[1] - jr).abs().max()) <= 1e-4, cut
        assert float(O.rotation_angle_deg(p, rp).max()) <= 0.1, cut


# ------------------------------------------------------------------------------------------------------------------ 6. set_state
def test_set_state_takes_the_reference_states_of_a_fixture(synth_assets):
    s = np.load(os.path.join(GOLD, FIXTURE))
    net = _net(synth_assets, 1)
    m = _motion(synth_assets, 81, 1, 4)
    _run(net, _dev(m))                                                      # counters off zero: h goes to the copy they designate
    for n in NETS:
        h, c = t(s["h_" + n].copy())[:, None], t(s["c_" + n].copy())[:, None]
        net.set_state(n, h, c)
    for n in NETS:
        h, c = net.get_state(n)
        assert _same(h[:, 0], t(s["h_" + n].copy())) and _same(c[:, 0], t(s["c_" + n].copy())), n


def test_set_state_of_get_state_changes_nothing_and_a_mask_spares_the_other_rows(synth_assets):
    B = 5
    m = _motion(synth_assets, 82, B, 12)
    m["j2dc"][1, 5, :, 2] = 0.2                                             # row 1 has a step pending after the first six frames
    nets = []
    for k in range(2):
        n = _net(synth_assets, B)
        n.gravityc = t(m["gravityc"])
        _run(n, _dev(m, 0, 6))
        nets.append(n)
    a, b = nets
    assert a.fusion_state()[1, 4] == 1
    for n in NETS:
        a.set_state(n, *a.get_state(n))
    pa, ta = _run(a, _dev(m, 6, 12))
    pb, tb = _run(b, _dev(m, 6, 12))
    assert _same(pa, pb) and _same(ta, tb)
    sa, sb = _snapshot(a), _snapshot(b)
    for r in range(B):
        _assert_rows(sa, r, sb, r, "set_state(get_state())")
    # a row mask
    g = torch.Generator().manual_seed(7)
    before = {n: a.get_state(n) for n in NETS}
    hr, cr = torch.randn(2, B, 1280, generator=g), torch.randn(2, B, 1280, generator=g)
    hr[0, 0, :2] = torch.tensor([float("nan"), -0.0])
    a.set_state("rnn4", hr, cr, rows=[1, 0, 1, 0, 0])
    a.set_state("rnn6", None, torch.ones(2, B, 1024), rows=torch.tensor([False, False, False, False, True]))
    for n in NETS:
        h, c = a.get_state(n)
        for r in range(B):
            if n == "rnn4" and r in (0, 2):
                assert _same(h[:, r], hr[:, r]) and _same(c[:, r], cr[:, r]), r
            elif n == "rnn6" and r == 4:
                assert _same(h[:, r], before[n][0][:, r]) and bool((c[:, r] == 1).all())
            else:
                assert _same(h[:, r], before[n][0][:, r]) and _same(c[:, r], before[n][1][:, r]), (n, r)
    with pytest.raises(_lib.RobustcapLibraryError, match="unknown net"):
        _lib.check(a._ctx, a._lib.rc_set_state(a._ctx, b"rnn5", None, None, None), "rc_set_state")


# ------------------------------------------------------------------------------------------------------------------ 7. live
LIVE_ENV = ("RC_LIVE_AQL", "RC_LIVE_LEAN_NC", "RC_LIVE_PRESTEP", "RC_LIVE_PRESTEP_IDLE_US", "RC_LIVE_LEAN", "RC_LIVE_EAGER", "RC_LIVE_MIRROR_BLIND",
            "RC_LIVE_SPIN", "RC_LIVE_SPIN_B2B", "RC_LIVE_ARM")


def _live_net(sd, body, B, grav):
    from robustcap_amd.net.sig_mp import Net
    n = Net(body=body, batch=B)
    n.load_state_dict(sd)
    n.set_gemm_mode(False)
    n.use_graph = True
    n.gravityc = grav
    return n


def _live_frame(net, m, i, B):
    if B == 1:
        return net.forward_online(t(m["j2dc"][0, i]), t(m["accc"][0, i]), t(m["oric"][0, i]), first_frame=(i == 0))
    return net.forward_live(t(m["j2dc"][:, i]), t(m["accc"][:, i]), t(m["oric"][:, i]), first_frame=(i == 0))


@pytest.mark.parametrize("B,cut", [(1, 16), (3, 12)], ids=["b1", "b3"])
def test_a_live_session_moves_to_a_fresh_context(B, cut, synth_assets, monkeypatch):
    """A paced session (a pre-step behind every frame, what a 60 fps caller gets: RC_LIVE_PRESTEP_IDLE_US=0) on the state dict whose lean
    and full frames agree bitwise, cut inside an occluded stretch: save, rc_live_end, a fresh Net with rc_live_begin, load, go on."""
    for k in LIVE_ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RC_LIVE_PRESTEP_IDLE_US", "0")
    case = next(c for c in X.CASES if c.name == f"aql_b{B}")
    body, T = synth_assets["body"], case.T
    sd = X.exact_sum_state_dict(X.WEIGHT_SEED, X.GAIN, case.pick)
    m = X.motion(case, body)
    grav = t(m["gravityc"])
    whole = _live_net(sd, body, B, grav)
    want = [_live_frame(whole, m, i, B) for i in range(T)]
    want_state = _snapshot(whole)
    first = _live_net(sd, body, B, grav)
    for i in range(cut):
        p, tr = _live_frame(first, m, i, B)
        assert _same(p, want[i][0]) and _same(tr, want[i][1]), i
    assert first.live_stats()[0] > 0                                        # steady state: lean frames ran before the save
    assert first.fusion_state()[0 if B == 1 else 1, 4] == 1             # ... and the cut is inside an occlusion: a step is pending
    state = first.save_rows()
    torch.cuda.synchronize()
    host = state.cpu()
    _lib.check(first._ctx, first._lib.rc_live_end(first._ctx), "rc_live_end")
    first.__dict__["_live_on"] = False
    del first
    second = _live_net(sd, body, B, grav)
    second._sync_gravity()
    torch.cuda.synchronize()
    _lib.check(second._ctx, second._lib.rc_live_begin(second._ctx), "rc_live_begin")
    second.__dict__["_live_on"] = True
    second.load_rows(host)
    for i in range(cut, T):
        p, tr = _live_frame(second, m, i, B)
        assert _same(p, want[i][0]) and _same(tr, want[i][1]), ("after the move", i, second.live_stats())
    lean, full = second.live_stats()
    assert lean > 0 and lean + full == T - cut, (lean, full)
    got = _snapshot(second)
    for r in range(B):
        _assert_rows(got, r, want_state, r, "moved live session")


# ------------------------------------------------------------------------------------------------------------------ 8. stream order
FB = 4


def _fence_net(assets):
    n = _net(assets, FB)
    n.gravityc = t(_motion(assets, F.REAL, FB, 2)["gravityc"])
    n._sync_gravity()
    return n


def _fence_cases(assets):
    def frames(seed):
        m = _motion(assets, seed, FB, 2)
        return [t(np.ascontiguousarray(m[k][:, 1])).cuda() for k in KEYS]

    def save_call(net, x):
        """a frame, then the save behind it: the records are that frame's -- of the payload the stream held when the call was made"""
        p, tr = net.forward_batch(x[0], x[1], x[2])
        return [p, tr, net.save_rows([2, 0, 3]).data]

    def records(seed):
        net = _fence_net(assets)
        net.forward_batch(*frames(seed))
        data = net.save_rows([1, 3]).data
        torch.cuda.synchronize()
        return [data.clone()]

    def load_call(net, x):
        net.load_rows(RowState(x[0], net.row_state_info()[1]), rows=[2, 0])
        return [net.save_rows().data]

    def after(net):
        fus, tr, st = _snapshot(net)
        return [fus, tr] + [v for n in NETS for v in st[n]]

    make = lambda: _fence_net(assets)
    return {"save_rows": F.Case("save_rows", ("rc_save_rows",), make, frames, save_call),
            "load_rows": F.Case("load_rows", ("rc_load_rows", "rc_save_rows"), make, records, load_call, after=after)}


@pytest.mark.parametrize("name", ["save_rows", "load_rows"])
def test_fenced_on_a_side_stream(name, synth_assets):
    """Exactly the fenced run of tests/test_gpu_stream_order.py (tests/stream_fence.py): the call on a torch side stream behind the delay
    kernel, its payload written in front of it and overwritten behind it on that stream only; cold and warm; warm must return held."""
    case = _fence_cases(synth_assets)[name]
    ref = F.reference(case)
    for variant in F.VARIANTS:
        F.run_case(case, variant, ref)                                      # (asserts the bits, and `held` for the warm variant)
    del ref
    gc.collect()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals_leave_context_and_blob_untouched(synth_assets):
    B = 5
    m = _motion(synth_assets, 91, B, 6)
    net = _net(synth_assets, B)
    net.gravityc = t(m["gravityc"])
    _run(net, _dev(m))
    bpr, fmt = net.row_state_info()
    assert bpr == 4 * (4 * sum(HIDDEN) + 512 + 160) and bpr % 16 == 0 and fmt == 1
    before = net.save_rows().data.clone()
    SENT = 0xA5
    blob = torch.full((B * bpr + 16,), SENT, dtype=torch.uint8, device="cuda")
    assert blob.data_ptr() % 16 == 0
    stream = torch.cuda.current_stream().cuda_stream

    def io_of(rows, n, ptr, nbytes=bpr):
        keep = None if rows is None else np.ascontiguousarray(np.asarray(rows, np.int32))
        return _lib.RcRowIO(None if keep is None else keep.ctypes.data, n, ptr, nbytes, stream), keep

    bad = {
        "null blob": io_of(None, 2, None),
        "n < 0": io_of(None, -1, blob.data_ptr()),
        "n > batch": io_of(None, B + 1, blob.data_ptr()),
        "row out of range": io_of([0, B], 2, blob.data_ptr()),
        "negative row": io_of([-1, 1], 2, blob.data_ptr()),
        "row listed twice": io_of([3, 1, 3], 3, blob.data_ptr()),
        "other bytes_per_row": io_of(None, 2, blob.data_ptr(), bpr + 16),
        "misaligned blob": io_of(None, 2, blob.data_ptr() + 4),
    }
    for entry in (net._lib.rc_save_rows, net._lib.rc_load_rows):
        for what, (io_, keep) in bad.items():
            assert entry(net._ctx, C.byref(io_)) == -1, (entry.__name__, what)
            assert net._lib.rc_last_error(net._ctx), what
        assert entry(net._ctx, None) == -1                                  # a null descriptor
        assert entry(None, C.byref(bad["n < 0"][0])) == -1
        io0, _ = io_of(None, 0, None)                                       # n == 0: a no-op, whatever the blob
        assert entry(net._ctx, C.byref(io0)) == 0
    with pytest.raises(_lib.RobustcapLibraryError, match="listed twice"):
        net.save_rows([1, 1])
    with pytest.raises(ValueError, match="format 2"):
        net.load_rows(RowState(before[:1].clone(), 2), rows=[0])
    with pytest.raises(ValueError, match="hidden sizes"):
        net.load_rows(RowState(before[:1].clone(), 1, (512,) * 6), rows=[0])
    torch.cuda.synchronize()
    assert bool((blob == SENT).all()), "a refused call wrote to the blob"
    assert _same(net.save_rows().data, before), "a refused call changed the context"
    # before rc_finalize_weights: RC_ERR_STATE
    from robustcap_amd.net.sig_mp import Net
    raw = Net(body=synth_assets["body"], batch=2)
    io2, _ = io_of(None, 2, blob.data_ptr())
    assert raw._lib.rc_save_rows(raw._ctx, C.byref(io2)) == -3 and raw._lib.rc_load_rows(raw._ctx, C.byref(io2)) == -3
    assert raw._lib.rc_set_state(raw._ctx, b"rnn3", None, None, None) == -3
    torch.cuda.synchronize()
    assert bool((blob == SENT).all())
