"""Gemm mode 2 on the device: rc_set_gemm_mode(ctx, 2) -- two round-to-nearest bf16 terms per operand, three products.

What pins the arithmetic is tests/gemm_mode2_ref.py (numpy, from the specification): every rc_lstm_step of a mode-2 context is
compared with `Emulated2` started from the device's OWN state before the step, within the UNSCALED bound of oracle/lstm_f64.py
(what separates the two is the order of the fp32 additions, which the six-product kernels pass at below 0.1 of it; a lost
product, truncated terms or stale planes land hundreds of times above), and with the float64 trajectory within G x the bound
(G = 8: tests/test_gemm_mode2_cpu.py). The dispatch is mode 1's (tests/test_gpu_gemm_precision.py has the table): the same
batches, environment variants and launch counters.

Then: within mode 2 a row's bits do not depend on the engine, the batch or the row it sits in; the fifteen reference fixtures
stay within 1e-4 m / 0.1 deg with exact traces; the planes follow every weight change; modes 0 and 1 are not touched by a visit
to mode 2; the sub-net entries refuse mode 2.
"""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemm_mode2_ref as M
import test_gpu_fixture_in_batch as FB
import test_gpu_gemm_precision as P
from oracle import sig_mp_oracle as O
from robustcap_amd import synth
from test_gemm_mode2_cpu import G

pytestmark = pytest.mark.gpu
t = torch.from_numpy
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NETS = P.NETS
SEQS = sorted(glob.glob(os.path.join(GOLD, "seq_*.npz")))


@pytest.fixture(scope="module", autouse=True)
def _cpu_threads():
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        yield
        return
    with threadpool_limits(limits=16):
        yield


@pytest.fixture(autouse=True)
def _reset_class_live():
    yield
    from robustcap_amd.net.sig_mp import Net
    Net.live = False


def _net(assets, B, mode=2, sd=None):
    from robustcap_amd.net.sig_mp import Net
    net = Net(body=assets["body"], batch=B)
    net.load_state_dict(assets["state_dict"] if sd is None else sd)
    net.set_gemm_mode(mode)
    return net


# ------------------------------------------------------------------------------------------------- 1. the switch
def test_mode_2_is_accepted_and_reported(synth_assets):
    from robustcap_amd import _lib
    from robustcap_amd.net.sig_mp import Net
    net = Net(body=synth_assets["body"], batch=4)
    net.load_state_dict(synth_assets["state_dict"])
    assert net._lib.rc_set_gemm_mode(net._ctx, 2) == 0                      # RC_OK
    assert net._lib.rc_get_gemm_mode(net._ctx) == 2
    assert net._lib.rc_set_gemm_mode(net._ctx, 3) != 0                      # refused, the mode stays
    assert b"rc_set_gemm_mode" in _lib.load().rc_last_error(net._ctx)
    assert net._lib.rc_get_gemm_mode(net._ctx) == 2
    for v, want in ((False, 0), (True, 1), (2, 2), (0, 0), (1, 1)):
        net.set_gemm_mode(v)
        assert net.gemm_mode == want, (v, net.gemm_mode)
    for bad in (3, -1, "2", 2.0, None):
        with pytest.raises(ValueError):
            net.set_gemm_mode(bad)
    assert net.gemm_mode == 1
    for rows in (1, 47, 48, 4096):
        assert _lib.load().rc_default_gemm_mode(rows) in (0, 1)


def test_rc_gemm_split_2_starts_a_context_in_mode_2():
    code = ("from robustcap_amd import synth, _lib\nfrom robustcap_amd.net.sig_mp import Net\n"
            "n = Net(body=synth.make_body(1), batch=2)\nprint('mode', n.gemm_mode, _lib.load().rc_default_gemm_mode(2), _lib.load().rc_default_gemm_mode(256), Net.default_gemm_mode(256))\n")
    env = dict(os.environ, RC_GEMM_SPLIT="2", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "mode 2 1 1 2\n" in out.stdout, out.stdout                         # the library's default never is 2; Net's pin follows the environment


# ------------------------------------------------------------------------------------------------- 2. rc_lstm_step
def _step_cases():
    cs = [(net, B, {}) for net in NETS for B in P.BATCHES]
    for k in (1, 2):
        env = {"RC_LDS_KSPLIT_512": str(k), "RC_LDS_KSPLIT_1024": str(k), "RC_LDS_KSPLIT_1280": str(k)}
        cs += [(net, B, env) for net in NETS for B in (128, 257)]
    cs += [(net, B, {"RC_LDS_MIN_ROWS": "0"}) for net in NETS for B in (128, 257)]
    return sorted(cs, key=lambda c: (c[0], c[1]))                           # (net, B) together: one float64 trajectory serves them


STEP_CASES = _step_cases()
WORST = {}


def test_every_kernel_family_is_reached_in_mode_2():
    seen = {P.lstm_kernel(n, B, True, e).split(" ")[0] for n, B, e in STEP_CASES}
    assert seen == {"small_split", "mid_split", "wide_split", "lds"}, seen
    ks = {(P.H_OF[n], P.ksplit(n, B, e)) for n, B, e in STEP_CASES if P.lstm_kernel(n, B, True, e) == "lds"}
    assert ks == {(h, k) for h in (512, 1024, 1280) for k in (1, 2)}, ks


@pytest.mark.parametrize("name,B,env", STEP_CASES, ids=[P._id((n, B, True, e, 6)).replace("split", "mode2") for n, B, e in STEP_CASES])
def test_lstm_step_vs_emulation_and_float64(name, B, env, monkeypatch):
    kernel = P.lstm_kernel(name, B, True, env)
    fam = P.family(kernel, name, B, env)
    net = P.make_net(B, 2, env, monkeypatch)
    assert net.gemm_mode == 2
    emu = M.Emulated2(P.state_dict(1.0), name, B)
    lds0, wide0, w320 = P.counters(net)
    prev = tuple(x.numpy().copy() for x in net.get_state(name))
    for s, (xg, mask, y64, h64, c64, tol_hc, tol_y) in enumerate(P.reference(name, B, 6, "normal", 1.0)):
        y = P.raw_step(net, name, xg, mask)
        h, c = (x.numpy() for x in net.get_state(name))
        where = (name, B, env, s, kernel)
        if mask is not None and not mask.any():                # all-false mask: no bit of h, c or y moves
            assert np.array_equal(h.view(np.uint32), prev[0].view(np.uint32)) and np.array_equal(c.view(np.uint32), prev[1].view(np.uint32)), where
            assert np.all(y == P.SENTINEL), where
        else:
            sel = np.ones(B, bool) if mask is None else mask
            assert np.all(y[~sel] == P.SENTINEL), where
            assert np.array_equal(h[:, ~sel].view(np.uint32), prev[0][:, ~sel].view(np.uint32)), where       # unselected rows keep h, c
            assert np.array_equal(c[:, ~sel].view(np.uint32), prev[1][:, ~sel].view(np.uint32)), where
            assert np.all(np.isfinite(h)) and np.all(np.isfinite(c)) and np.all(np.isfinite(y[sel])), where
            # the same step from the device's own state, in the specified arithmetic: within the UNSCALED bound
            emu.h, emu.c = prev[0].copy(), prev[1].copy()
            ye, he, ce = emu.step(xg, mask)
            re = max(float(np.max(np.abs(h - he) / tol_hc)), float(np.max(np.abs(c - ce) / tol_hc)),
                     float(np.max(np.abs(y[sel].astype(np.float64) - ye[sel]) / tol_y[sel])))
            # ... and the float64 trajectory, within G x the bound
            r64 = max(float(np.max(np.abs(h - h64) / tol_hc)), float(np.max(np.abs(c - c64) / tol_hc)),
                      float(np.max(np.abs(y[sel] - y64[sel]) / tol_y[sel]))) / G
            print(f"{name} B {B} step {s} {fam}: vs emulation {re:.3f}, vs float64 / G {r64:.3f}")
            for k, r in (("emulation", re), ("float64/G", r64)):
                WORST[(fam, k)] = max(WORST.get((fam, k), 0.0), r)
            assert re <= 1.0, (where, "vs Emulated2", re)
            assert r64 <= 1.0, (where, "vs float64, scaled by G", r64)
        prev = (h.copy(), c.copy())
        lds, wide, w32 = P.counters(net)
        n = s + 1
        assert lds - lds0 == (2 * n if kernel == "lds" else 0), (where, lds - lds0)
        lstm_wide = 0 if kernel == "lds" or kernel.startswith("small") else 2
        assert wide - wide0 == n * ((1 if B > 16 else 0) + lstm_wide), (where, wide - wide0)
        assert w32 == w320 == 0, where


def test_zz_report_worst_ratios():
    for (fam, k), r in sorted(WORST.items()):
        print(f"worst {k:10s} {fam:18s} {r:.3f}")
    assert all(r <= 1.0 for r in WORST.values())


# ------------------------------------------------------------------------------------------------- 3. one row, one result
def _seq_run(assets, m, B, T, seq, lengths=None, fixture=None):
    net = _net(assets, B)
    if fixture is not None:
        for k in ("use_flat_floor", "use_reproj_opt", "use_vision_updater", "use_imu_updater"):
            setattr(net, k, bool(fixture[k]))
    net.set_sequence_mode(seq, 8, force=True)
    net.gravityc = t(m["gravityc"])
    ft = None if m.get("first_tran") is None else t(m["first_tran"])
    p, tr = net.forward_sequence(t(m["j2dc"][:, :T]), t(m["accc"][:, :T]), t(m["oric"][:, :T]), first_tran=ft,
                                 first_frame=bool(m.get("first_frame", False)), lengths=lengths)
    torch.cuda.synchronize()
    return p.cpu(), tr.cpu(), net.sequence_stats(), net.launch_stats()


def test_engines_agree_bitwise_in_mode_2(synth_assets):
    B, T = 4, 56
    m = synth.make_motion(77, B, T, synth_assets["body"], conf="mixed")
    m["j2dc"][1, 10:30, :, 2] = 0.5                                         # one body occluded for a while
    sp, st, sstat, _ = _seq_run(synth_assets, m, B, T, False)
    wp, wt, wstat, _ = _seq_run(synth_assets, m, B, T, True)
    assert sstat[0] == 0 and wstat[0] >= T - 1
    assert torch.equal(wp, sp) and torch.equal(wt, st)
    lengths = [T, 40, T, 17]
    rp, rt, _, _ = _seq_run(synth_assets, m, B, T, True, lengths=lengths)
    for r, n in enumerate(lengths):
        assert torch.equal(rp[r, :n], sp[r, :n]) and torch.equal(rt[r, :n], st[r, :n]), r
    # a fixture at batch 1
    s = np.load(os.path.join(GOLD, "seq_mixed_firsttran.npz"))
    f = {"j2dc": s["j2dc"][None], "accc": s["accc"][None], "oric": s["oric"][None], "gravityc": s["gravityc"].reshape(1, 3),
         "first_tran": s["first_tran"].reshape(1, 3) if s["first_tran"].size else None, "first_frame": bool(s["first_frame"])}
    T1 = s["pose"].shape[0]
    a = _seq_run(synth_assets, f, 1, T1, False, fixture=s)
    b = _seq_run(synth_assets, f, 1, T1, True, fixture=s)
    c = _seq_run(synth_assets, f, 1, T1, True, lengths=[T1], fixture=s)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_resident_setting_is_ignored_in_mode_2(synth_assets):
    """Mode 2 has no instantiation of the resident kernel: the context runs its segments on the three streams, same bits."""
    B, T = 96, 24
    m = synth.make_motion(78, B, T, synth_assets["body"], conf="mixed")
    outs = []
    for resident in (False, True):
        net = _net(synth_assets, B)
        net.set_sequence_mode(True, 8, force=True)
        net.set_resident(resident)
        net.gravityc = t(m["gravityc"])
        p, tr = net.forward_sequence(t(m["j2dc"]), t(m["accc"]), t(m["oric"]), first_frame=True)
        torch.cuda.synchronize()
        outs.append((p.cpu(), tr.cpu(), net.launch_stats()[0], net.resident_stats()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert outs[0][2] == outs[1][2] > 0                                     # the same shared-weight launches: nothing left for a resident one
    assert outs[0][3] == outs[1][3]


@pytest.mark.parametrize("B,row", [(48, 47), (64, 20), (65, 0), (65, 64), (257, 0), (257, 64), (257, 256)])
def test_fixture_row_is_its_batch_1_run_in_mode_2(B, row, synth_assets):
    """Contexts of 33-64 rows run their layer steps as one-reader launches of 64 x 128 tiles -- in mode 2 on rc_gemm_split2_kernel,
    reading the planes (mode 1 streams fp32 weights there: rc_gemm_split48_w32_kernel) --, larger ones on rc_gemm_lds2_kernel: the
    same bits as the batch-1 run."""
    name = "seq_mixed_firsttran.npz"
    s = np.load(os.path.join(GOLD, name))
    key = ("mode2", name)
    if key not in FB._cache:
        net = FB._net(synth_assets, s, 1)
        net.set_gemm_mode(2)
        net.gravityc = t(s["gravityc"])
        ft = t(s["first_tran"]).view(1, 3) if s["first_tran"].size else None
        FB._cache[key] = FB._run(net, s["j2dc"][None], s["accc"][None], s["oric"][None], ft, bool(s["first_frame"]), 0)
    sp, st, ss, strace = FB._cache[key]
    m, ft = FB._context(synth_assets, s, B, row, "mixed")
    net = FB._net(synth_assets, s, B)
    net.set_gemm_mode(2)
    net.gravityc = t(m["gravityc"])
    p, tr, states, trace = FB._run(net, m["j2dc"], m["accc"], m["oric"], ft, bool(s["first_frame"]), row)
    w32 = P.counters(net)[2]
    lds, wide = net.launch_stats()
    assert w32 == 0                                                         # no mode-2 launch streams fp32 weights
    if B <= 64:
        assert lds == 0 and wide > 0, (lds, wide)
        assert net.gemm_kernel_name() == "rc_gemm_split2_kernel"
    else:
        assert lds > 0                                                      # on the shared-weight kernel
        assert net.gemm_kernel_name() == "rc_gemm_lds2_kernel"
    assert torch.equal(p, sp) and torch.equal(tr, st) and torch.equal(trace, strace)
    for n in NETS:
        assert torch.equal(states[n][0], ss[n][0]) and torch.equal(states[n][1], ss[n][1]), n


# ------------------------------------------------------------------------------------------------- 4. the fixtures
WORST_FIX = {}


@pytest.mark.parametrize("path", SEQS, ids=[os.path.basename(p)[4:-4] for p in SEQS])
def test_reference_fixtures_in_mode_2(path, synth_assets):
    """Frame by frame (every frame's trace and regime against the reference's) and, for the fixtures a sequence call can carry,
    as ONE forward_sequence call on the wavefront engine with the same bits; within 1e-4 m / 0.1 deg of the reference."""
    from robustcap_amd.net.sig_mp import Net
    s = np.load(path)
    live = str(s["live"])
    Net.live = live == "pre"
    net = _net(synth_assets, 1)
    if live == "post":
        net.live = True
    for k in ("use_flat_floor", "use_reproj_opt", "use_vision_updater", "use_imu_updater"):
        setattr(net, k, bool(s[k]) if k in s else k != "use_reproj_opt")
    net.gravityc = t(s["gravityc"])
    ft = t(s["first_tran"]) if s["first_tran"].size else None
    T = s["pose"].shape[0]
    regime = O.fixture_regimes(s)
    poses, trans = [], []
    for i in range(T):
        p, tr = net.forward_online(t(s["j2dc"][i]), t(s["accc"][i]), t(s["oric"][i]), ft if i == 0 else None, bool(s["first_frame"]) and i == 0)
        tc, exp = net.get_trace()[0].tolist(), s["trace"][i]
        assert tc[0] == int(regime[i]), f"frame {i}: regime {tc[0]}, the reference's {regime[i]}"
        assert tc[1] == int(exp[1]) and tc[2] == int(exp[2]) and tc[3] == int(exp[4]) and tc[4] == int(exp[5]), f"frame {i}: trace {tc} vs {exp}"
        poses.append(p.cpu()), trans.append(tr.cpu())
    pose, tran = torch.stack(poses), torch.stack(trans)
    last_trace = net.get_trace()[0].tolist()
    rp, rt = t(s["pose"]), t(s["tran"])
    dt = float((tran - rt).abs().max())
    dr = float(O.rotation_angle_deg(pose, rp).max())
    ob = O.OracleBody(synth_assets["body"])
    dj = float((ob.forward_kinematics(pose.reshape(-1, 24, 3, 3), tran)[1] - ob.forward_kinematics(rp, rt)[1]).abs().max())
    WORST_FIX[os.path.basename(path)] = (dt, dr, dj)
    print(f"{os.path.basename(path)}: translation {dt:.2e} m, rotation {dr:.2e} deg, joints {dj:.2e} m")
    assert dt <= 1e-4 and dr <= 0.1 and dj <= 1e-4
    if not live:
        del net
        net = _net(synth_assets, 1)
        for k in ("use_flat_floor", "use_reproj_opt", "use_vision_updater", "use_imu_updater"):
            setattr(net, k, bool(s[k]))
        net.set_sequence_mode(True, 8, force=True)
        net.gravityc = t(s["gravityc"])
        p, tr = net.forward_sequence(t(s["j2dc"][None]), t(s["accc"][None]), t(s["oric"][None]),
                                     first_tran=None if ft is None else ft.view(1, 3), first_frame=bool(s["first_frame"]))
        torch.cuda.synchronize()
        assert net.sequence_stats()[0] >= T - 1
        assert torch.equal(p[0].cpu().reshape(pose.shape), pose) and torch.equal(tr[0].cpu(), tran)
        assert net.get_trace()[0].tolist() == last_trace


def test_zz_report_worst_distances():
    if WORST_FIX:
        w = max(WORST_FIX.items(), key=lambda kv: kv[1][0])
        print(f"mode 2, worst over {len(WORST_FIX)} fixtures: translation {w[1][0]:.2e} m ({w[0]}), rotation "
              f"{max(v[1] for v in WORST_FIX.values()):.2e} deg, joints {max(v[2] for v in WORST_FIX.values()):.2e} m")


# ------------------------------------------------------------------------------------------------- 5. planes follow the weights
def _probe(net, B, T=12, seed=79):
    m = synth.make_motion(seed, B, T, synth.make_body(1), conf="mixed")
    net.reset_states()
    net.gravityc = t(m["gravityc"])
    p, tr = net.forward_sequence(t(m["j2dc"]), t(m["accc"]), t(m["oric"]), first_frame=True)
    torch.cuda.synchronize()
    return p.cpu(), tr.cpu()


@pytest.mark.parametrize("B", [4, 80])
def test_planes_follow_load_state_dict(B, synth_assets):
    other = synth.make_state_dict(3)
    net = _net(synth_assets, B)
    first = _probe(net, B)
    net.load_state_dict(other)                                              # in mode 2: the planes are rebuilt from the new packings
    assert net.gemm_mode == 2
    got = _probe(net, B)
    fresh = _probe(_net(synth_assets, B, sd=other), B)
    assert torch.equal(got[0], fresh[0]) and torch.equal(got[1], fresh[1])
    assert not torch.equal(got[1], first[1])


def test_planes_follow_an_optimiser_step(synth_assets):
    B = 4
    net = _net(synth_assets, B, mode=1)
    warm = _net(synth_assets, B, mode=1)
    warm.set_gemm_mode(2)                                                   # ... and a context whose planes EXIST when the step runs
    warm.set_gemm_mode(1)
    outs = []
    for n in (net, warm):
        tr = n.trainable("rnn8")
        opt = tr.optimizer(lr=1e-2)                                          # the fused device step (rc_subnet_optim_step)
        xs = [torch.from_numpy(synth.normal(80, i, 9 * 141).reshape(9, 141).astype(np.float32)).cuda() for i in range(2)]
        loss = sum((y ** 2).sum() for y in tr(xs))
        opt.zero_grad()
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        sd = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in n.state_dict().items()}
        n.set_gemm_mode(2)
        outs.append((_probe(n, B), sd))
    for got, sd in outs:
        fresh = _probe(_net(synth_assets, B, sd=sd), B)
        assert torch.equal(got[0], fresh[0]) and torch.equal(got[1], fresh[1])
    base = _probe(_net(synth_assets, B), B)
    # (the step did move rnn8, the contact net: the translation follows it)
    assert not (torch.equal(outs[0][0][0], base[0]) and torch.equal(outs[0][0][1], base[1]))


# ------------------------------------------------------------------------------------------------- 6. modes 0 and 1 untouched
@pytest.mark.parametrize("B,mode", [(4, 0), (4, 1), (80, 1)])
def test_a_visit_to_mode_2_leaves_the_other_modes_alone(B, mode, synth_assets):
    net = _net(synth_assets, B, mode=mode)
    before = _probe(net, B)
    net.set_gemm_mode(2)
    two = _probe(net, B)
    net.set_gemm_mode(mode)
    after = _probe(net, B)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert not (torch.equal(before[0], two[0]) and torch.equal(before[1], two[1]))      # mode 2 is another arithmetic


def test_run_dataset_pins_its_contexts_to_mode_2(synth_assets):
    """run_dataset(gemm_mode=2): every row is its own batch-1 run in mode 2, bit for bit; None and True keep what they did."""
    from robustcap_amd import evaluate as ev
    body, sd = synth_assets["body"], synth_assets["state_dict"]
    ds = synth.make_dataset(23, 2, 24, body, n_cam=2, conf="mixed")
    rows = ev.rows_of(ds)
    nets = {}
    fast = ev.run_dataset(ds, sd, body, nets=nets, gemm_mode=2)
    assert [n.gemm_mode for n, _ in nets.values()] == [2]
    for (i, j) in (rows[0], rows[-1]):
        k, a, o, g = ev.camera_inputs(ds["joint2d_mp"][i][j], ds["imu_acc"][i], ds["imu_ori"][i], ds["cam_K"][i][j], ds["cam_T"][i][j])
        net = _net(synth_assets, 1)
        net.gravityc = g
        ft = ev.labels(ds, i, j)[1][0]
        p, tr = net.forward_sequence(k[None], a[None], o[None], first_tran=ft[None])
        assert torch.equal(p[0].cpu(), fast[(i, j)][0]) and torch.equal(tr[0].cpu(), fast[(i, j)][1])
    exact = ev.run_dataset(ds, sd, body, nets=nets, gemm_mode=True)                 # the same contexts, back in mode 1
    assert [n.gemm_mode for n, _ in nets.values()] == [1]
    plain = ev.run_dataset(ds, sd, body)                                            # None: the library's default for 4 rows, fp32
    fp32 = ev.run_dataset(ds, sd, body, gemm_mode=False)
    assert all(torch.equal(plain[r][1], fp32[r][1]) for r in rows)
    assert not all(torch.equal(fast[r][1], exact[r][1]) for r in rows)


def test_run_dataset_without_a_mode_leaves_mode_2(synth_assets):
    """The caller's `nets` after a run pinned to mode 2: gemm_mode=None at 48 rows is the library's default, mode 1, on the same
    context, with the bits of a run pinned to mode 1 -- mode 2 is asked for, never inherited."""
    from robustcap_amd import evaluate as ev
    from robustcap_amd.net.sig_mp import Net
    body, sd = synth_assets["body"], synth_assets["state_dict"]
    ds = synth.make_dataset(24, 6, 16, body, n_cam=8, conf="mixed")
    rows = ev.rows_of(ds)
    assert len(rows) == 48 and Net.default_gemm_mode(48) == 1 and type(Net.default_gemm_mode(48)) is int
    nets = {}
    fast = ev.run_dataset(ds, sd, body, nets=nets, gemm_mode=2)
    (net, _), = nets.values()
    assert net.gemm_mode == 2
    plain = ev.run_dataset(ds, sd, body, nets=nets)
    assert len(nets) == 1 and net.gemm_mode == 1
    exact = ev.run_dataset(ds, sd, body, gemm_mode=1)
    assert all(torch.equal(plain[r][0], exact[r][0]) and torch.equal(plain[r][1], exact[r][1]) for r in rows)
    assert not all(torch.equal(fast[r][1], exact[r][1]) for r in rows)


# ------------------------------------------------------------------------------------------------- 7. what refuses it
def test_subnet_entries_refuse_mode_2(synth_assets):
    net = _net(synth_assets, 2)
    x = [torch.zeros(5, 141, device="cuda")]
    with pytest.raises(Exception, match="gemm mode 2"):
        net.rnn8(x)
    with pytest.raises(Exception, match="gemm mode 2"):
        net.trainable("rnn8")
    net.set_gemm_mode(1)
    assert net.rnn8(x)[0].shape == (5, 2)
