"""The device-resident L-BFGS of the smplify path -- the rc_vec_* kernels of csrc/rc_smplify.hip and both backends of
csrc/rc_smplify_api.cpp (SingleRow, and RowBatch::run_round with BatchRow) -- bit for bit against its CPU restatement.

rc_lbfgs_device_probe runs the optimiser of rc_smplify_run (backend 0) and of rc_smplify_run_batch (backend 1) on a synthetic
closure whose fp32 arithmetic tests/lbfgs_device_emu.cpp restates exactly; tests/golden/lbfgs_device_trace.json holds that
program's records (test_lbfgs_device_emu_cpu.py keeps the file current, anchors the program and shows that each of its wrong
variants moves a recorded bit). Here every row of every run must give the recorded n_iter, n_eval, every loss bit and every bit
of x. Rows of 75, 4,050 and 4,125 elements: inside one 4,096-element block, just under one, and two blocks of which the second
holds 29 elements -- in a batch the short rows' partial sums then lie at stride 2 while their own block count is 1.
Reads the fixture only: no compiler, inputs regenerated from the seeds in numpy."""
import ctypes as C
import hashlib
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import lbfgs_device_case as K  # noqa: E402

from robustcap_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
CAP = 80                                          # losses kept per row (max_eval of the longest setting is 75)


@pytest.fixture(scope="module")
def fx():
    return K.load_fixture()


@pytest.fixture(scope="module")
def ctx():
    torch.cuda.set_device(0)
    lib, c = _lib.load(), C.c_void_p()
    assert lib.rc_create(1, 0, C.byref(c)) == 0       # a bare context: no weights, no body, no prior
    yield c
    torch.cuda.synchronize()
    assert lib.rc_destroy(c) == 0


_dev = {}


def _inputs(case):
    key = (case["T"], case["seed"], case["x_scale"])
    if key not in _dev:
        _dev[key] = tuple(torch.from_numpy(v).cuda() for v in K.inputs(*key))
    return _dev[key]


def _report(line):
    print(line)
    path = os.environ.get("RC_LBFGS_EXACT_REPORT")    # (a run that keeps the measured times, e.g. for profiles/lbfgs_device_exact.txt)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _probe(ctx, fx, backend, names, lr, max_iter, label):
    """Run the named cases as the rows of one call and demand the fixture's bits of every row. Returns (max_jobs, rounds)."""
    lib = _lib.load()
    cases = [fx["cases"][n] for n in names]
    n = len(cases)
    ins = [_inputs(c) for c in cases]
    outs = [torch.full((75 * c["T"],), float("nan"), device="cuda") for c in cases]
    tab = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    T_rows = np.array([c["T"] for c in cases], np.int64)
    infos = (_lib.RcSmplifyInfo * n)()
    losses = np.full((n, CAP), np.nan, np.float32)
    max_jobs, rounds = C.c_int32(-1), C.c_int32(-1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = lib.rc_lbfgs_device_probe(ctx, backend, n, T_rows.ctypes.data_as(C.c_void_p), tab([i[0] for i in ins]), tab([i[1] for i in ins]),
                                   tab([i[2] for i in ins]), C.c_float(lr), max_iter, tab(outs), infos, losses.ctypes.data_as(C.c_void_p), CAP,
                                   C.byref(max_jobs), C.byref(rounds), _lib.stream_ptr())
    _lib.check(ctx, rc, "rc_lbfgs_device_probe")
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    bad = []
    for r, (name, c) in enumerate(zip(names, cases)):
        got = losses[r].view(np.uint32)
        x = outs[r].cpu().numpy()
        same = (infos[r].n_iter, infos[r].n_eval) == (c["n_iter"], c["n_eval"]) and c["n_eval"] <= CAP
        first = next((i for i in range(min(c["n_eval"], CAP)) if int(got[i]) != c["losses"][i]), None)
        same = same and first is None and not losses[r, c["n_eval"]:].any()
        same = same and np.float32(infos[r].first_loss).view(np.uint32) == c["losses"][0]
        same_x = hashlib.sha256(x.tobytes()).hexdigest() == c["x_sha256"]
        if n <= 8 or not (same and same_x):
            _report(f"{label} row {r} {name} (T {c['T']}): n_iter {infos[r].n_iter} n_eval {infos[r].n_eval} "
                    f"{'equal' if same and same_x else 'DIFFERENT'}")
        if not (same and same_x):
            sample = [int(v) for v in x.view(np.uint32)[K.sample_index(x.size)]]
            bad.append(f"{name} (row {r}): n_iter {infos[r].n_iter} / {c['n_iter']}, n_eval {infos[r].n_eval} / {c['n_eval']}, first differing "
                       f"evaluation {first}, x {'equal' if same_x else 'differs'}, sample {sample} / {c['x_sample']}")
    _report(f"{label}: backend {backend}, {n} rows, lr {lr:g}, max_iter {max_iter}, {ms:.1f} ms, largest job table {max_jobs.value}, "
            f"rounds {rounds.value}, {'all rows equal' if not bad else f'{len(bad)} rows DIFFERENT'}")
    assert not bad, "\n".join(bad[:8])
    return max_jobs.value, rounds.value


def _env(monkeypatch, setting, totals=None):
    hist = K.SETTINGS[setting]["history_env"]
    if hist:
        monkeypatch.setenv("RC_LBFGS_HISTORY", str(hist))
    else:
        monkeypatch.delenv("RC_LBFGS_HISTORY", raising=False)
    if totals is None:
        monkeypatch.delenv("RC_SMPLIFY_DEVICE_TOTALS", raising=False)
    else:
        monkeypatch.setenv("RC_SMPLIFY_DEVICE_TOTALS", totals)
    return K.SETTINGS[setting]["lr"], K.SETTINGS[setting]["max_iter"]


def _table(fx, names):
    """Largest job table of a lock-step batch of these rows: a round holds every live row's next request."""
    jobs = [fx["cases"][n]["jobs"] for n in names]
    return max(sum(j[k] for j in jobs if k < len(j)) for k in range(max(map(len, jobs))))


@pytest.mark.parametrize("setting", list(K.SETTINGS))
def test_single_row_backend(ctx, fx, monkeypatch, setting):
    """Backend 0: SingleRow, the rows one after another (the row at its optimum among them: one evaluation, nothing moves)."""
    lr, max_iter = _env(monkeypatch, setting)
    names = [f"{setting}_{r}" for r in K.ROWS + ("zero",)]
    assert _probe(ctx, fx, 0, names, lr, max_iter, f"single {setting}") == (0, 0)


@pytest.mark.parametrize("variant", ["together", "reversed", "totals_host", "totals_device", "with_row_at_optimum"])
@pytest.mark.parametrize("setting", list(K.SETTINGS))
def test_batch_backend(ctx, fx, monkeypatch, setting, variant):
    """Backend 1: the three rows in one lock-step batch -- in both orders, with the totals added on the host and on the device, and
    with the row at its optimum, which leaves in the first round while the others go on."""
    lr, max_iter = _env(monkeypatch, setting, {"totals_host": "0", "totals_device": "1"}.get(variant))
    names = [f"{setting}_{r}" for r in K.ROWS]
    if variant == "reversed":
        names = names[::-1]
    if variant == "with_row_at_optimum":
        names.insert(1, f"{setting}_zero")
    max_jobs, rounds = _probe(ctx, fx, 1, names, lr, max_iter, f"batch {setting} {variant}")
    assert max_jobs == _table(fx, names)
    longest = max(len(fx["cases"][n]["jobs"]) for n in names)
    assert longest <= rounds <= longest + 1                            # (+ 1: the flush of the last accepted step)


def test_buffers_reused_and_regrown(fx, monkeypatch):
    """One fresh context: a long history on a short row, then a two-block row with a short history (more frames, fewer pairs), then
    the short row again -- reserve_lbfgs and the batch arenas are first grown, then regrown, then reused."""
    torch.cuda.set_device(0)
    lib, c = _lib.load(), C.c_void_p()
    assert lib.rc_create(1, 0, C.byref(c)) == 0
    try:
        for backend in (0, 1):
            lr, max_iter = _env(monkeypatch, "prod")
            _probe(c, fx, backend, ["prod_T1"], lr, max_iter, f"reuse backend {backend}: long history, T 1")
            lr, max_iter = _env(monkeypatch, "hist2")
            _probe(c, fx, backend, ["hist2_T55"], lr, max_iter, f"reuse backend {backend}: history 2, T 55")
            _probe(c, fx, backend, ["hist2_T1", "hist2_T54"], lr, max_iter, f"reuse backend {backend}: history 2, T 1 and 54")
            lr, max_iter = _env(monkeypatch, "hist4")
            _probe(c, fx, backend, ["hist4_T1"], lr, max_iter, f"reuse backend {backend}: history 4, T 1")
    finally:
        torch.cuda.synchronize()
        assert lib.rc_destroy(c) == 0


def test_job_table_longer_than_a_grid_s_y_extent(ctx, fx, monkeypatch):
    """Enough T = 1 rows (8 seeds cycled) that a round's job table passes 65,535 entries: rc_launch_vec_dots_rows sends it in slices."""
    monkeypatch.delenv("RC_LBFGS_HISTORY", raising=False)
    monkeypatch.delenv("RC_SMPLIFY_DEVICE_TOTALS", raising=False)
    n = fx["grid_rows"]
    names = [K.GRID[r % 8] for r in range(n)]
    g = fx["cases"][K.GRID[0]]
    max_jobs, _ = _probe(ctx, fx, 1, names, g["lr"], g["max_iter"], f"grid-y {n} rows")
    assert max_jobs == fx["grid_max_jobs"] == _table(fx, names) and max_jobs > K.GRID_Y_MAX


def test_probe_refuses_bad_arguments(ctx):
    lib = _lib.load()
    one = (C.c_void_p * 1)(torch.zeros(75, device="cuda").data_ptr())
    T = np.array([1], np.int64)
    infos = (_lib.RcSmplifyInfo * 1)()
    call = lambda backend, max_iter, x0: lib.rc_lbfgs_device_probe(ctx, backend, 1, T.ctypes.data_as(C.c_void_p), x0, one, one, C.c_float(1.0), max_iter,
                                                                    one, infos, None, 0, None, None, _lib.stream_ptr())
    assert call(2, 20, one) == -1 and call(0, 0, one) == -1 and call(0, 20, None) == -1
    assert b"rc_lbfgs_device_probe" in lib.rc_last_error(ctx)
