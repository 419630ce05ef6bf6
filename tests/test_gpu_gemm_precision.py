"""Every gate-GEMM kernel that rc_lstm_step reaches, against a float64 step (oracle/lstm_f64.py) at its dispatch edges.

The bound is oracle/lstm_f64.Bound (error / bound <= 1); tests/test_gemm_bound_cpu.py shows on the CPU that torch fp32 and the
split-bf16 products as built stay below a third of it while a lost partial product, the low terms of half of K skipped or h(t - 1)
of the wrong layer land three times or more above it. Every step is checked against the float64 trajectory, never against the
previous GPU step.

Kernel of the LSTM layer steps of rc_lstm_step (one problem per launch; rows = the batch B): lstm_problem (pick_tile, the 64-row
tile overrides from B >= 192, the shared-weight kernel from RC_LDS_MIN_BATCH = 65 rows in split mode when B >= RC_LDS_MIN_ROWS =
min(160, max(64, B / 2))), launch_problems, rc_launch_gemm (rc_gemm_is_small / _mid / _w32):

  B            fp32 (set_gemm_mode(False))                              split-bf16 (set_gemm_mode(True))
  1, 16        rc_gemm_small_kernel 16 x 4 (1x1)                         rc_gemm_small_split_kernel 1x1
  17, 63       rc_gemm_small_kernel 16 x 32 (1x2)                        rc_gemm_small_split_kernel 1x2
  64           rc_gemm_mid_kernel 32 x 64 (2x4)                          rc_gemm_mid_split_kernel 2x4 (a context below 65 rows)
  65, 127      rc_gemm_mid_kernel 2x4                                    rc_gemm_lds_kernel, ksplit 1 (H 512, 1024) / 2 (H 1280)
  128 .. 191   H 512: rc_gemm_mid_kernel 2x4                             rc_gemm_lds_kernel; ksplit of H 1024: 1 up to 160, 2 above
               H 1024: rc_gemm_kernel 2x8, H 1280: rc_gemm_kernel 2x10
  192 .. 513   rnn2: rc_gemm_mid_kernel 2x4 (no default 64-row tile)     rc_gemm_lds_kernel, ksplit 1 / 2 / 2 (H 512 / 1024 / 1280)
               rnn3/7/8: rc_gemm_kernel 4x4, rnn6 4x8, rnn4 4x5           (B 513: a second 256-row tile)

  Forced through the environment (read by rc_create):
  RC_LDS_KSPLIT_512/1024/1280 = 1 | 2, split, B 128 / 257: rc_gemm_lds_kernel with one / two workgroups per tile
  RC_LDS_MIN_ROWS=0, split:  B 65, 127: rc_gemm_mid_split_kernel 2x4; B 128, 191: H 512 mid_split 2x4, rc_gemm_split_kernel 2x8
                             (H 1024) / 2x10 (H 1280); B 192, 257: rnn2 mid_split 2x4, rc_gemm_split_kernel 4x4 / 4x8 / 4x5
  RC_TILE_RNN6=8x4, RC_TILE_RNN4=4x8, RC_TILE_RNN2=4x4, RC_TILE_S2H512=2x8 (B 256 / 257): rc_gemm_kernel, or with
                             RC_LDS_MIN_ROWS=0 in split mode rc_gemm_split_kernel, on those tiles
  RC_TILE_* of a width that does not divide H (4x5 / 2x10 on H 512 or 1024): rejected by rc_create

  Not reached by rc_lstm_step (no ABI added for them):
  rc_gemm_small_nt_kernel     live frames only (GemmLaunch.live, batch <= 16, fp32): tests/test_gpu_live.py
  rc_gemm_split48_w32_kernel  64 x 128 tiles with one row tile per problem = the wavefront engine of 33-64 row contexts
                              (run_wave2_segment): tests/test_gpu_fixture_in_batch.py, tests/test_gpu_module_surface.py
  rc_gemm_resident_kernel     out of scope here (bitwise against frame-stepped: tests/test_gpu_resident.py)
  live_lstm_body (rc_live.hip), both tile widths: bitwise against the frame-stepped plan over whole sequences on a state dict
                              whose linear2 sums are exact in every order: tests/test_gpu_live_exact.py

linear1 runs on the 2x4 tiles (mid kernels) from 17 rows and on 1x1 tiles below, linear2 on 1x1 tiles (small kernels); in split
mode both use split products too. launch_stats() counts launches of rc_gemm_lds_kernel and of every kernel but the small ones,
rc_get_launch_stats_w32 those of rc_gemm_split48_w32_kernel: what a case's kernel predicts for them is asserted after every step
(the contexts run without the vision updater, whose deferred steps rc_lstm_step would otherwise flush in launches of their own).

Each case: two plain steps (the second is the first with a live h W_hh), a masked step (rows 0, B - 1 and both sides of every
tile edge below B selected, the other rows' x NaN / +-inf), an all-false mask (no bit of h, c or y may change), two plain steps.
y of rows a step does not select is left untouched (include/robustcap_hip.h: rc_lstm_step): pinned with a sentinel-filled y.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import lstm_f64 as R

pytestmark = pytest.mark.gpu

NETS = ("rnn2", "rnn3", "rnn4", "rnn6", "rnn7", "rnn8")
H_OF = {"rnn2": 512, "rnn3": 512, "rnn4": 1280, "rnn6": 1024, "rnn7": 512, "rnn8": 512}
BATCHES = (1, 16, 17, 63, 64, 65, 127, 128, 160, 161, 191, 192, 256, 257)
SENTINEL = 7.25                                       # y is prefilled with it: rows a step does not select must keep it


def lstm_kernel(net, B, split, env=None):
    """The kernel of rc_lstm_step's LSTM layer launches (the table above, as rc_gemm_api.cpp / rc_gemm.hip decide it)."""
    env = env or {}
    H = H_OF[net]
    min_rows = int(env.get("RC_LDS_MIN_ROWS", min(160, max(64, B // 2))))
    if split and min_rows > 0 and B >= 65 and B >= min_rows:
        return "lds"
    if B <= 16:
        mr, nc = 1, 1
    elif B < 64:
        mr, nc = 1, 2
    elif B < 128:
        mr, nc = 2, 4
    else:
        mr, nc = 2, {512: 4, 1024: 8, 1280: 10}[H]
    if B >= 192:
        knob = {"rnn6": "RC_TILE_RNN6", "rnn4": "RC_TILE_RNN4", "rnn2": "RC_TILE_RNN2"}.get(net, "RC_TILE_S2H512")
        default = {"rnn6": "4x8", "rnn4": "4x5", "rnn2": None}.get(net, "4x4")
        t = env.get(knob, default)
        if t:
            mr, nc = (int(v) for v in t.split("x"))
    if mr == 1 and nc <= 2:
        fam = "small"
    elif mr <= 2 and nc <= 4 and not (mr == 2 and nc < 4):
        fam = "mid"
    else:
        fam = "wide"
    return f"{fam}{'_split' if split else ''} {mr}x{nc}"


def ksplit(net, B, env):
    H = H_OF[net]
    k = {512: "RC_LDS_KSPLIT_512", 1024: "RC_LDS_KSPLIT_1024", 1280: "RC_LDS_KSPLIT_1280"}[H]
    default = {512: 1, 1024: 1 if B <= 160 else 2, 1280: 2}[H]
    return 1 if int(env.get(k, default)) == 1 else 2


def family(kernel, net, B, env):
    """kernel-family label of the results table (the lds kernel with its workgroups per tile)."""
    return f"lds ksplit {ksplit(net, B, env)}" if kernel == "lds" else kernel.split(" ")[0]


# ----------------------------------------------------------------------------------------------------------- cases
def _cases():
    cs = []
    for split in (False, True):
        for net in NETS:
            for B in BATCHES:
                cs.append((net, B, split, {}, 6))
        for net in ("rnn4", "rnn6"):
            cs.append((net, 513, split, {}, 3))
    for k in (1, 2):
        env = {"RC_LDS_KSPLIT_512": str(k), "RC_LDS_KSPLIT_1024": str(k), "RC_LDS_KSPLIT_1280": str(k)}
        for net in ("rnn3", "rnn4", "rnn6"):
            for B in (128, 257):
                cs.append((net, B, True, env, 6))
    for net in NETS:
        for B in (65, 127, 128, 191, 192, 257):
            cs.append((net, B, True, {"RC_LDS_MIN_ROWS": "0"}, 6))
    tiles = {"RC_TILE_RNN6": "8x4", "RC_TILE_RNN4": "4x8", "RC_TILE_RNN2": "4x4", "RC_TILE_S2H512": "2x8"}
    for net in ("rnn2", "rnn4", "rnn6", "rnn7"):
        for B in (192, 257):
            cs.append((net, B, False, dict(tiles), 6))
            cs.append((net, B, True, dict(tiles, RC_LDS_MIN_ROWS="0"), 6))
    return sorted(cs, key=lambda c: (c[0], c[1], c[4]))          # (net, B) together: one float64 trajectory serves them all


CASES = _cases()
_KERNELS_SEEN = {lstm_kernel(n, B, s, e).split(" ")[0] for n, B, s, e, _ in CASES}


def test_every_kernel_of_the_list_is_reached():
    """rc_gemm_kernel, rc_gemm_split_kernel, the mid, small and lds kernels: each carries the LSTM steps of some case."""
    assert _KERNELS_SEEN == {"small", "small_split", "mid", "mid_split", "wide", "wide_split", "lds"}, _KERNELS_SEEN
    tiles = {lstm_kernel(n, B, s, e) for n, B, s, e, _ in CASES}
    for t in ("wide 8x4", "wide 4x8", "wide 4x5", "wide 4x4", "wide 2x8", "wide 2x10", "wide_split 8x4", "wide_split 4x8",
              "wide_split 4x5", "wide_split 4x4", "wide_split 2x8", "wide_split 2x10"):
        assert t in tiles, t
    ks = {(H_OF[n], ksplit(n, B, e)) for n, B, s, e, _ in CASES if lstm_kernel(n, B, s, e) == "lds"}
    assert ks == {(h, k) for h in (512, 1024, 1280) for k in (1, 2)}, ks


# ----------------------------------------------------------------------------------------------------------- helpers
@pytest.fixture(scope="module", autouse=True)
def _cpu_threads():
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        yield
        return
    with threadpool_limits(limits=16):
        yield


_SD = {}


def state_dict(gain):
    from robustcap_amd import synth
    if gain not in _SD:
        _SD[gain] = synth.make_state_dict(0, gain=gain)
    return _SD[gain]


def make_net(B, split, env, monkeypatch, gain=1.0):
    from robustcap_amd import synth
    from robustcap_amd.net.sig_mp import Net
    for k, v in env.items():
        monkeypatch.setenv(k, v)                              # (read when the context is created)
    net = Net(body=synth.make_body(1), batch=B)
    net.load_state_dict(state_dict(gain))
    net.set_gemm_mode(split)
    assert net.gemm_mode == int(split)
    net.use_vision_updater = False      # (else every rc_lstm_step first flushes the deferred rnn6 / rnn4 updater steps: launches of
    return net                          # their own, of no row here, that the counters would count too)


def raw_step(net, name, x, rows):
    """rc_lstm_step with y prefilled by SENTINEL (Net.lstm_step zero-fills its y)."""
    from robustcap_amd import _lib
    from robustcap_amd import config as C
    nin, nout = {n: (i, o) for n, i, _, o in C.NETS}[name]
    xd = torch.as_tensor(x).to(device="cuda", dtype=torch.float32).contiguous()
    m = None if rows is None else torch.as_tensor(rows).to(device="cuda", dtype=torch.uint8).contiguous()
    y = torch.full((net.batch, nout), SENTINEL, device="cuda")
    _lib.check(net._ctx, net._lib.rc_lstm_step(net._ctx, name.encode(), _lib.ptr(xd), _lib.ptr(m), _lib.ptr(y), _lib.stream_ptr()),
               "rc_lstm_step")
    torch.cuda.synchronize()
    return y.cpu().numpy()


def counters(net):
    lds, wide = net.launch_stats()
    w = ctypes.c_int64()
    from robustcap_amd import _lib
    _lib.check(net._ctx, net._lib.rc_get_launch_stats_w32(net._ctx, ctypes.byref(w)), "rc_get_launch_stats_w32")
    return lds, wide, w.value


def edge_mask(B):
    """Selected: row 0, B - 1, both sides of every tile edge below B (15/16, 31/32, 63/64, 127/128, 255/256, 511/512) and every
    other row -- so that the compacted row list crosses tile edges as well."""
    m = np.zeros(B, bool)
    m[0::2] = True
    m[[r for e in (16, 32, 64, 128, 256, 512) for r in (e - 1, e) if r < B] + [B - 1]] = True
    return m


def inputs(B, nin, step, kind):
    from robustcap_amd import synth
    x = synth.normal(300 + step, 5, B * nin).reshape(B, nin).astype(np.float32)
    if kind == "mixed":                                   # rows of zeros, 1e-3, 1e3 and unit magnitude
        x *= np.array([0.0, 1e-3, 1e3, 1.0], np.float32)[np.arange(B) % 4, None]
    return x


def schedule(B, steps):
    """[(mask or None, poison the unselected rows' x)]"""
    if steps == 3:
        return [(None, False), (None, False), (edge_mask(B), True)]
    return [(None, False), (None, False), (edge_mask(B), True), (np.zeros(B, bool), True), (None, False), (None, False)]


_REF = {}


def reference(name, B, steps, kind, gain):
    """float64 trajectory of a schedule (shared by both arithmetics and every env variant of a (net, B))."""
    key = (name, B, steps, kind, gain)
    if key not in _REF:
        if len(_REF) > 4:
            _REF.clear()
        from robustcap_amd import config as C
        nin = {n: i for n, i, _, _ in C.NETS}[name]
        p = R.params(state_dict(gain), name)
        h, c = R.zero_state(p, B)
        bound = R.Bound(B)
        out = []
        for s, (mask, poison) in enumerate(schedule(B, steps)):
            x = inputs(B, nin, s, kind)
            y, h, c, S = R.step(p, x, h, c, mask)
            if mask is None or mask.any():
                bound.update(S, c)
            xg = x.copy()
            if poison:
                bad = np.flatnonzero(~mask)
                xg[bad] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(len(bad)) % 3, None]
            out.append((xg, mask, y, h, c, bound.tol_hc().copy(), bound.tol_y().copy() if mask is None or mask.any() else None))
        _REF[key] = out
    return _REF[key]


WORST = {}     # (kernel family, "state" | "y") -> worst error / bound over the cases run (printed at the end of the module)


def run_case(name, B, split, env, steps, monkeypatch, kind="normal", gain=1.0):
    kernel = lstm_kernel(name, B, split, env)
    net = make_net(B, split, env, monkeypatch, gain)
    fam = family(kernel, name, B, env)
    lds0, wide0, w320 = counters(net)
    prev = None
    for s, (xg, mask, y64, h64, c64, tol_hc, tol_y) in enumerate(reference(name, B, steps, kind, gain)):
        y = raw_step(net, name, xg, mask)
        h, c = (t.numpy() for t in net.get_state(name))
        where = (name, B, split, env, kind, gain, s)
        if mask is not None and not mask.any():            # all-false mask: no bit of h, c or y moves
            assert np.array_equal(h.view(np.uint32), prev[0].view(np.uint32)), where
            assert np.array_equal(c.view(np.uint32), prev[1].view(np.uint32)), where
            assert np.all(y == SENTINEL), where
        else:
            sel = np.ones(B, bool) if mask is None else mask
            assert np.all(y[~sel] == SENTINEL), where           # unselected rows' y untouched
            assert np.all(np.isfinite(h)) and np.all(np.isfinite(c)) and np.all(np.isfinite(y[sel])), where
            rs = max(float(np.max(np.abs(h - h64) / tol_hc)), float(np.max(np.abs(c - c64) / tol_hc)))
            ry = float(np.max(np.abs(y[sel] - y64[sel]) / tol_y[sel]))
            for k, r in (("state", rs), ("y", ry)):
                WORST[(fam, k)] = max(WORST.get((fam, k), 0.0), r)
            assert rs <= 1.0 and ry <= 1.0, (where, kernel, rs, ry)
        prev = (h.copy(), c.copy())
        lds, wide, w32 = counters(net)
        n = s + 1
        assert lds - lds0 == (2 * n if kernel == "lds" else 0), (where, kernel, lds - lds0)
        lstm_wide = 0 if kernel == "lds" or kernel.startswith("small") else 2
        assert wide - wide0 == n * ((1 if B > 16 else 0) + lstm_wide), (where, kernel, wide - wide0)
        assert w32 == w320 == 0, where


def _id(c):
    net, B, split, env, steps = c
    e = ",".join(f"{k[3:]}={v}" for k, v in sorted(env.items()))
    return f"{net}-B{B}-{'split' if split else 'fp32'}" + (f"-{e}" if e else "")


@pytest.mark.parametrize("name,B,split,env,steps", CASES, ids=[_id(c) for c in CASES])
def test_lstm_step_vs_float64(name, B, split, env, steps, monkeypatch):
    run_case(name, B, split, env, steps, monkeypatch)


@pytest.mark.parametrize("name,B,split", [("rnn4", 257, True), ("rnn6", 257, False)])
def test_saturated_gates_vs_float64(name, B, split, monkeypatch):
    """Weights x3 (synth gain 3): most gates saturate; rnn4 at 257 rows is on the shared-weight kernel with a second row tile."""
    run_case(name, B, split, {}, 6, monkeypatch, gain=3.0)


@pytest.mark.parametrize("name,B,split", [("rnn6", 257, True), ("rnn4", 17, True), ("rnn3", 192, False)])
def test_rows_of_mixed_magnitude_vs_float64(name, B, split, monkeypatch):
    """Input rows of zeros, 1e-3, 1e3 and unit size side by side in one tile."""
    run_case(name, B, split, {}, 6, monkeypatch, kind="mixed")


@pytest.mark.parametrize("knob,value", [("RC_TILE_S2H512", "4x5"), ("RC_TILE_RNN2", "2x10"), ("RC_TILE_RNN6", "4x5"),
                                        ("RC_TILE_RNN6", "2x10")])
def test_tile_width_that_does_not_divide_h_is_rejected(knob, value, monkeypatch):
    """A tile of 4 nc units must divide H: otherwise the last H % (4 nc) units of every layer step would never be computed."""
    from robustcap_amd import synth
    from robustcap_amd.net.sig_mp import Net
    monkeypatch.setenv(knob, value)
    with pytest.raises(RuntimeError, match=knob):
        Net(body=synth.make_body(1), batch=192)


def test_zz_report_worst_ratios():
    """The largest error / bound per kernel family over the cases above (pytest -s shows it)."""
    for (fam, k), r in sorted(WORST.items()):
        print(f"worst {k:5s} {fam:18s} {r:.3f}")
    assert all(r <= 1.0 for r in WORST.values())
