"""Host planner of the wavefront engine with per-row ends (rc_plan_wave_rows, no GPU).

Row b of a ragged call starts frames t0 .. len[b] - 1 only. The hazard checker is the one of tests/test_wave_plan.py (``replay``),
run row by row: a row of length L inside a ragged plan must obey exactly the hazards of a call of L frames -- its last frame books
no rider (the updater step stays pending, as at the end of a uniform call) -- so each row's column of the table is replayed as a
one-row plan of its own length, and the plan's tick count and per-tick row counts are the union of those."""
import ctypes as C

import numpy as np
import pytest

from robustcap_amd import _lib
from test_wave_plan import TAIL, plan, replay

RC_ERR_INVALID = -1


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def plan_rows(codes, lens, t0=0, first_reach=None, pend=None, imu=True, vis=True):
    lib = _lib.load()
    codes = np.ascontiguousarray(np.asarray(codes, np.int8))
    T, B = codes.shape
    ln = np.ascontiguousarray(np.asarray(lens, np.int32))
    fr = np.ascontiguousarray(np.ones(B, np.int32) if first_reach is None else np.asarray(first_reach, np.int32))
    pd = np.ascontiguousarray(np.zeros(B, np.int32) if pend is None else np.asarray(pend, np.int32))
    nt, npre = C.c_int32(), C.c_int32()
    est = np.zeros(2)
    args = (_p(codes), B, T, t0, _p(ln), _p(fr), _p(pd), int(imu), int(vis))
    rc = lib.rc_plan_wave_rows(*args, None, 0, C.byref(nt), C.byref(npre), None, _p(est))      # capacity query
    assert rc != 0
    buf = np.full((npre.value + 1, B), -7, np.int32)                     # (+ 1: a plan without a tick still gets a real pointer)
    cnt = np.zeros((4, npre.value), np.int32)
    rc = lib.rc_plan_wave_rows(*args, _p(buf), npre.value * B, C.byref(nt), C.byref(npre), _p(cnt) if npre.value else None, _p(est))
    assert rc == 0 and (buf[npre.value:] == -7).all()
    fa = buf[:npre.value]
    return fa, nt.value, cnt, est


def replay_rows(codes, lens, fa, n_ticks, cnt, t0, first_reach, pend, imu=True, vis=True):
    """``replay`` of tests/test_wave_plan.py with per-row ends: every row's column against a one-row call of the row's own length."""
    codes = np.asarray(codes)
    T, B = codes.shape
    n_prep = fa.shape[0]
    total = np.zeros((4, n_prep), int)
    ticks = 0
    entries = []
    for b in range(B):
        L = int(lens[b])
        col = fa[:, b]
        if L <= t0:
            assert (col == -1).all()                                     # nothing booked, not even the rider of a pending step
            entries.append(np.zeros(0, int))
            continue
        assert col.max() == L - 1                                        # no entry >= len[b]
        # the row alone: its own counts and its own last tick, from the one-row planner (the hazards do not depend on other rows)
        fa1, nt1, cnt1, _ = plan(codes[:L, b:b + 1], t0=t0, first_reach=[first_reach[b]], pend=[pend[b]], imu=imu, vis=vis)
        assert (col[:fa1.shape[0]] == fa1[:, 0]).all() and (col[fa1.shape[0]:] == -1).all()
        e = replay(codes[:L, b:b + 1], fa1, nt1, cnt1, t0, [first_reach[b]], [pend[b]], imu=imu, vis=vis)
        entries.append(e[0, t0:])
        total[:, :cnt1.shape[1]] += cnt1
        ticks = max(ticks, nt1)
    assert n_ticks == ticks
    assert (cnt == total).all()
    return entries


def test_full_lengths_give_the_uniform_plan():
    rng = np.random.default_rng(3)
    for _ in range(10):
        T, B = int(rng.integers(2, 60)), int(rng.integers(1, 6))
        codes = rng.choice([0, 1, 2], size=(T, B), p=[0.3, 0.2, 0.5])
        fr, pd = rng.integers(0, 2, B), rng.integers(0, 2, B)
        t0 = int(rng.integers(0, 2))
        a = plan(codes, t0=t0, first_reach=fr, pend=pd)
        b = plan_rows(codes, np.full(B, T), t0=t0, first_reach=fr, pend=pd)
        assert (a[0] == b[0]).all() and a[1] == b[1] and (a[2] == b[2]).all()
        assert (a[3] == b[3]).all()                                      # both cost estimates, to the bit


def test_all_visible_rows_tick_count_is_the_longest_rows():
    T = 40
    for lens, t0 in (([40, 10, 25, 0, 1], 0), ([7, 40, 40, 2, 0, 1], 1), ([12, 12, 3], 0)):
        B = len(lens)
        codes = np.full((T, B), 2)
        fa, nt, cnt, _ = plan_rows(codes, lens, t0=t0, first_reach=np.zeros(B))
        longest = max(lens)
        _, nt1, _, _ = plan(np.full((longest, 1), 2), t0=t0, first_reach=[0])
        assert nt == nt1
        assert cnt[0].sum() == sum(max(0, L - t0) for L in lens)
        replay_rows(codes, lens, fa, nt, cnt, t0, np.zeros(B, int), np.zeros(B, int))


def test_each_frame_of_a_row_once_in_order_and_none_past_its_end():
    rng = np.random.default_rng(11)
    T, B = 50, 6
    codes = rng.choice([0, 1, 2], size=(T, B), p=[0.3, 0.2, 0.5])
    lens = [0, 1, 50, 17, 33, 2]
    for t0 in (0, 1):
        fa, nt, cnt, _ = plan_rows(codes, lens, t0=t0, first_reach=np.ones(B))
        for b, L in enumerate(lens):
            got = fa[:, b][fa[:, b] >= 0]
            assert got.tolist() == list(range(t0, L))


def test_a_row_ending_on_an_occluded_frame_books_no_rider_after_it():
    T = 20
    codes = np.full((T, 2), 2)
    codes[4:7, 0] = 0                                                    # row 0: occluded on frames 4..6, ends on frame 6
    fa, nt, cnt, _ = plan_rows(codes, [7, T], first_reach=[0, 0])
    # riders of frames 4 and 5 only (slots 4 + TAIL, 5 + TAIL); frame 6 leaves its step pending
    assert cnt[2].sum() == 2 and cnt[2][4 + TAIL] == 1 and cnt[2][5 + TAIL] == 1
    assert nt == T + TAIL                                                # ... and the short row holds nobody up
    replay_rows(codes, [7, T], fa, nt, cnt, 0, [0, 0], [0, 0])
    # the uniform plan of the same codes books the third rider
    _, _, cnt_u, _ = plan(codes, first_reach=[0, 0])
    assert cnt_u[2].sum() == 3


def test_a_row_ending_where_init_net_fires_holds_nobody_up():
    T = 16
    codes = np.full((T, 3), 2)
    codes[:5, 0] = 1                                                     # row 0 reaches the high regime on frame 5 = its last frame
    fa, nt, cnt, _ = plan_rows(codes, [6, T, T], first_reach=[1, 0, 0])
    assert cnt[3].sum() == 1 and cnt[3][5] == 1
    assert (fa[:T, 1] == np.arange(T)).all() and (fa[:T, 2] == np.arange(T)).all()
    assert nt == T + TAIL
    replay_rows(codes, [6, T, T], fa, nt, cnt, 0, [1, 0, 0], [0, 0, 0])


def test_a_row_without_a_frame_keeps_its_pending_step():
    codes = np.full((9, 2), 2)
    fa, nt, cnt, _ = plan_rows(codes, [0, 9], first_reach=[0, 0], pend=[1, 0])
    assert cnt[2].sum() == 0 and (fa[:, 0] == -1).all()
    fa, nt, cnt, _ = plan_rows(codes, [1, 9], t0=1, first_reach=[0, 0], pend=[1, 0])   # frame 0 ran frame-stepped: nothing left of row 0
    assert cnt[2].sum() == 0 and (fa[:, 0] == -1).all()
    fa, nt, cnt, _ = plan_rows(codes, [0, 0], first_reach=[0, 0], pend=[1, 1])
    assert nt == 0 and fa.shape[0] == 0


@pytest.mark.parametrize("seed", range(8))
def test_random_ragged_plans_respect_every_hazard(seed):
    rng = np.random.default_rng(100 + seed)
    for _ in range(10):
        T, B = int(rng.integers(2, 80)), int(rng.integers(3, 8))
        runs = rng.choice([0, 1, 2], size=(T // 5 + 2, B), p=[0.3, 0.2, 0.5])
        codes = np.repeat(runs, 5, axis=0)[:T]
        flip = rng.random((T, B)) < 0.08
        codes = np.where(flip, rng.integers(0, 3, (T, B)), codes)
        lens = rng.integers(0, T + 1, B)
        lens[:3] = (0, 1, T)                                             # the edges, every time
        lens = rng.permutation(lens)
        fr, pd = rng.integers(0, 2, B), rng.integers(0, 2, B)
        t0 = int(rng.integers(0, 2))
        imu, vis = bool(rng.integers(0, 4)), bool(rng.integers(0, 4))
        fa, nt, cnt, est = plan_rows(codes, lens, t0=t0, first_reach=fr, pend=pd, imu=imu, vis=vis)
        replay_rows(codes, lens, fa, nt, cnt, t0, fr, pd, imu=imu, vis=vis)
        assert est[0] > 0 and est[1] > 0


def test_the_frame_stepped_estimate_falls_with_the_live_rows():
    T, B = 64, 128
    codes = np.full((T, B), 2)
    full = plan_rows(codes, np.full(B, T), first_reach=np.zeros(B))[3]
    thin = plan_rows(codes, [T] * 4 + [8] * (B - 4), first_reach=np.zeros(B))[3]
    assert thin[1] < full[1] and thin[0] < full[0]
    assert thin[1] >= 0.45 * full[1]                                    # never below the small-tile share of a frame


def test_invalid_arguments():
    lib = _lib.load()
    codes = np.full((5, 2), 2, np.int8)
    fr, pd = np.zeros(2, np.int32), np.zeros(2, np.int32)
    nt, npre = C.c_int32(), C.c_int32()
    fa = np.zeros(200, np.int32)

    def call(ln, T=5, t0=0):
        lp = None if ln is None else _p(np.ascontiguousarray(np.asarray(ln, np.int32)))
        return lib.rc_plan_wave_rows(_p(codes), 2, T, t0, lp, _p(fr), _p(pd), 1, 1, _p(fa), fa.size, C.byref(nt), C.byref(npre), None, None)

    assert call([5, 3]) == 0
    assert call(None) == RC_ERR_INVALID
    assert call([-1, 3]) == RC_ERR_INVALID
    assert call([6, 3]) == RC_ERR_INVALID
    assert call([5, 3], t0=5) == RC_ERR_INVALID
