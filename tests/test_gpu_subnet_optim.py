"""The optimiser step of a trainable sub-net on the device (tr.optimizer(...): rc_subnet_optim_step = clip_grad_norm_ + Adam + the repack of
rc_update_subnet_weights in one call; articulate/utils/torch/train.py:120-121): the norm and every updated quantity against the float64
restatement (tests/subnet_optim_f64.py) within K_F32 times the error of torch fp32 on the CPU, the repack bitwise a fresh load, no second
commit and no stale host copy, the old path's values, a skipped tensor, bitwise reruns and resume, a loop that learns, bad input.

Observed on MI355X (profiles/subnet_optim_ratios.txt): see the RATIO lines each accuracy test prints before it asserts."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import subnet_optim_f64 as F64
import test_gpu_subnet_forward as FWD
from robustcap_amd import _lib
from robustcap_amd import synth
from robustcap_amd.net.sig_mp import Net
from robustcap_amd.train import param_names

pytestmark = pytest.mark.gpu

SPEC, K_F32 = FWD.SPEC, FWD.K_F32
_sd, _net, _inputs, _same = FWD._sd, FWD._net, FWD._inputs, FWD._same
LENGTHS = (5, 3, 1)
LR = 1e-2                       # updates stand clear of the parameters' rounding


def _arg(name, xs, seed):
    """The call's argument: the sequences, for rnn2 paired with an x_init each."""
    if name != "rnn2":
        return xs
    v = torch.randn(len(xs), 69, generator=torch.Generator().manual_seed(seed + 50))
    return [(x, v[i]) for i, x in enumerate(xs)]


@functools.lru_cache(maxsize=None)
def _cot(name, seed):
    g = torch.Generator().manual_seed(seed + 100)
    return [torch.randn(T, SPEC[name][2], generator=g) for T in LENGTHS]


def _backward(tr, name, seed, scale=1.0):
    """One real backward of sum(y * cotangent) * scale on fresh gradients; returns the call's argument."""
    arg = _arg(name, _inputs(name, LENGTHS, seed), seed)
    tr.zero_grad()
    ys = tr(arg)
    (sum((y * c.to(y.device)).sum() for y, c in zip(ys, _cot(name, seed))) * scale).backward()
    return arg


def _down(ts):
    return [None if t is None else t.detach().cpu().numpy().copy() for t in ts]


def _grads(tr):
    return _down([p.grad for p in tr.parameters()])


@functools.lru_cache(maxsize=None)
def _unit_norm(name, seed):
    """The gradient norm of the case with unit cotangents (float64 over the downloaded gradients): the cases scale their cotangents from it."""
    tr = _net(1).trainable(name)
    _backward(tr, name, seed)
    return F64.total_norm(_grads(tr))


def _torch_f32_steps(P0, G, steps, max_norm, **hyper):
    """clip_grad_norm_ + torch.optim.Adam on the CPU in fp32 from the same values: (params, exp_avg, exp_avg_sq) after each step."""
    ps = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in P0]
    opt = torch.optim.Adam(ps, **hyper)
    out = []
    for _ in range(steps):
        for p, g in zip(ps, G):
            p.grad = None if g is None else torch.from_numpy(g.copy())          # (clip_grad_norm_ scales in place)
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
        st = [opt.state.get(p, {}) for p in ps]
        out.append((_down(ps), [s["exp_avg"].numpy().copy() if s else np.zeros(p.shape, np.float32) for s, p in zip(st, ps)],
                    [s["exp_avg_sq"].numpy().copy() if s else np.zeros(p.shape, np.float32) for s, p in zip(st, ps)]))
    return out


def _check_bound(label, names, got, f64, t32):
    """max |q_gpu - q_f64| <= K_F32 max |q_t32 - q_f64| + 1e-7 max |q_f64| per tensor and quantity, each figure printed before it is held
    to the bound (profiles/subnet_optim_ratios.txt is this output)."""
    bad = []
    for what, a, b, c in zip(("p", "exp_avg", "exp_avg_sq"), got, f64, t32):
        for k, x, y, z in zip(names, a, b, c):
            scale = float(np.abs(y).max())
            e_gpu, e_t32 = float(np.abs(x.astype(np.float64) - y).max()), float(np.abs(z.astype(np.float64) - y).max())
            print(f"RATIO {label} {what} {k}: scale {scale:.3e} err_gpu {e_gpu:.3e} err_t32 {e_t32:.3e} ratio {e_gpu / max(e_t32, 1e-300):.2f}")
            if not e_gpu <= K_F32 * e_t32 + 1e-7 * scale:
                bad.append((what, k, e_gpu, e_t32, scale))
    assert not bad, (label, bad)


def _state(tr, opt):
    return _down(tr.parameters()), _down(opt.exp_avg), _down(opt.exp_avg_sq)


# ---- 1, 2: the norm, the clip coefficient and the update against float64 ---------------------------------------------------------------
@pytest.mark.parametrize("bites", [True, False])
def test_norm_and_update_against_float64(bites):
    """rnn8 (linear2.bias: 2 elements), one real backward with the cotangents scaled so that the norm is ~10 (the clip bites) or ~0.1
    (coef == 1); the same downloaded fp32 gradients for three steps, checked after the first and the third."""
    name, seed, max_norm = "rnn8", 61, 1.0
    hyper = dict(lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    net = _net(1)
    tr = net.trainable(name)
    opt = tr.optimizer(clip_grad_norm=max_norm, **hyper)
    _backward(tr, name, seed, (10.0 if bites else 0.1) / _unit_norm(name, seed))
    G, P = _grads(tr), _down(tr.parameters())
    M = V = [np.zeros(p.shape) for p in P]
    t32 = _torch_f32_steps(P, G, 3, max_norm, **hyper)
    names = param_names(name)
    for step in (1, 2, 3):
        norm = opt.step()
        assert norm.is_cuda and norm.dim() == 0
        P, M, V, ref_norm, ref_coef = F64.adam_step(P, G, M, V, step, max_norm=max_norm, **hyper)
        tn, coef = (float(v) for v in opt.last_norm_and_coef.cpu())
        # squares of fp32 are exact in double, the sum errs by <= N 2^-53 (N <= 2.7e7), one sqrt and one rounding to fp32: 2e-7 relative
        print(f"NORM bites={int(bites)} step {step}: gpu {tn!r} f64 {ref_norm!r} rel {abs(tn - ref_norm) / ref_norm:.3e} coef {coef!r}")
        assert (tn > max_norm) == bites and float(norm) == tn
        assert abs(tn - ref_norm) <= 2e-7 * ref_norm
        assert np.float32(coef) == F64.clip_coef(np.float32(tn), max_norm, np.float32)     # the fp32 formula on the returned norm
        assert (coef < 1.0) == bites
        assert all(np.array_equal(a, b) for a, b in zip(_grads(tr), G))                    # the gradients are not scaled
        if step in (1, 3):
            _check_bound(f"update-bites{int(bites)}-step{step}", names, _state(tr, opt), (P, M, V), t32[step - 1])
    assert opt.step_count == 3


def test_update_with_weight_decay_against_float64():
    name, seed, max_norm = "rnn8", 62, 1.0
    hyper = dict(lr=LR, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.05)
    tr = _net(1).trainable(name)
    opt = tr.optimizer(clip_grad_norm=max_norm, **hyper)
    _backward(tr, name, seed, 10.0 / _unit_norm(name, seed))
    G, P = _grads(tr), _down(tr.parameters())
    M = V = [np.zeros(p.shape) for p in P]
    t32 = _torch_f32_steps(P, G, 2, max_norm, **hyper)
    for step in (1, 2):
        opt.step()
        P, M, V, _, _ = F64.adam_step(P, G, M, V, step, max_norm=max_norm, **hyper)
    _check_bound("update-wd-step2", param_names(name), _state(tr, opt), (P, M, V), t32[1])


# ---- 3: the repack is exact ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("name", ["rnn8", "rnn2", "rnn4"])
def test_repack_is_bitwise_a_fresh_load(name, split):
    """rnn2: 18 tensors and init_net; rnn4: H = 1280, linear1's K = 171 padded, the row-major copy of the narrow linear2. The first
    backward builds the transposed packs, so the step refreshes them and the second backward runs on the refreshed ones."""
    net = _net(1, split)
    tr = net.trainable(name)
    opt = tr.optimizer(lr=LR, clip_grad_norm=1.0)
    arg = _backward(tr, name, 63)
    before = _down(tr.parameters())
    opt.step()
    assert all(not np.array_equal(a, b) for a, b in zip(before, _down(tr.parameters())))
    fresh = Net(body=synth.make_body(1), batch=1)
    fresh.load_state_dict(net.state_dict())
    fresh.set_gemm_mode(split)
    ftr = fresh.trainable(name)
    for k, p in tr.named_parameters():
        assert torch.equal(p.detach().cpu(), fresh.state_dict()[f"{name}.{k}"]), k
    ys, ref = tr(arg), getattr(fresh, name)(arg)
    assert all(_same(y.detach(), r) for y, r in zip(ys, ref))
    assert all(_same(y.detach(), r) for y, r in zip(ys, getattr(net, name)(arg)))
    _backward(tr, name, 63)
    _backward(ftr, name, 63)
    for (k, p), q in zip(tr.named_parameters(), ftr.parameters()):
        assert _same(p.grad, q.grad), k
    if name == "rnn4":                                                                     # the stepped path reads Wrm and the padded biases
        x = torch.randn(1, SPEC[name][0], generator=torch.Generator().manual_seed(64))
        assert _same(net.lstm_step(name, x), fresh.lstm_step(name, x))


# ---- 4: no second commit, no stale host copy ------------------------------------------------------------------------------------------------
def test_no_second_commit_and_no_stale_host_copy(monkeypatch):
    name = "rnn8"
    net = _net(1)
    tr = net.trainable(name)
    opt = tr.optimizer(lr=LR, clip_grad_norm=1.0)
    calls = []
    real = net._lib.rc_update_subnet_weights
    monkeypatch.setattr(net._lib, "rc_update_subnet_weights", lambda *a: calls.append(1) or real(*a))
    arg = _backward(tr, name, 65)
    old = net.state_dict()[f"{name}.linear2.bias"].clone()
    versions = [p._version for p in tr.parameters()]
    opt.step(); opt.zero_grad()
    assert all(p.grad is None for p in tr.parameters())
    assert all(p._version > v for p, v in zip(tr.parameters(), versions))                  # torch knows the parameters changed
    _backward(tr, name, 65)
    opt.step()
    ys = tr(arg)
    assert not calls                                                                       # the steps repacked; no call committed
    sd = net.state_dict()
    for k, p in tr.named_parameters():
        assert torch.equal(sd[f"{name}.{k}"], p.detach().cpu()), k
    assert not torch.equal(sd[f"{name}.linear2.bias"], old)
    assert torch.equal(net.rnn8.linear2.bias, tr._params["linear2.bias"].detach().cpu())
    assert torch.equal(net.rnn8.rnn.state_dict()["weight_hh_l1"], tr._params["rnn.weight_hh_l1"].detach().cpu())
    assert all(_same(y.detach(), r) for y, r in zip(ys, net.rnn8(arg)))
    with torch.no_grad():                                                                  # the old way still commits by itself
        tr._params["linear2.bias"].add_(1.0)
    tr(arg)
    assert len(calls) == 1
    assert torch.equal(net.state_dict()[f"{name}.linear2.bias"], tr._params["linear2.bias"].detach().cpu())
    for bad in (dict(amsgrad=True), dict(amsgrad=False), dict(foreach=True)):
        with pytest.raises(ValueError):
            tr.optimizer(**bad)


# ---- 5: the old path's values ---------------------------------------------------------------------------------------------------------------
def _torch_forward(name, P, xs, dtype):
    """The sub-net restated with nn.Linear, nn.LSTM and pack_sequence on the CPU in `dtype`, on the parameters P (param_names order)."""
    from torch.nn.utils.rnn import pack_sequence, pad_packed_sequence
    nin, H, nout = SPEC[name]
    P = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in zip(param_names(name), P)}
    l1, l2, rnn = torch.nn.Linear(nin, H).to(dtype), torch.nn.Linear(H, nout).to(dtype), torch.nn.LSTM(H, H, 2).to(dtype)
    with torch.no_grad():
        l1.weight.copy_(P["linear1.weight"]); l1.bias.copy_(P["linear1.bias"])
        l2.weight.copy_(P["linear2.weight"]); l2.bias.copy_(P["linear2.bias"])
        for k, p in rnn.named_parameters():
            p.copy_(P[f"rnn.{k}"])
        out, _ = rnn(pack_sequence([torch.relu(l1(x.to(dtype))) for x in xs], enforce_sorted=False))
        out, _ = pad_packed_sequence(out)
        return [l2(out[: x.shape[0], i]).numpy() for i, x in enumerate(xs)]


def test_one_iteration_equals_the_old_path():
    name, seed, max_norm = "rnn8", 66, 1.0
    hyper = dict(lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    scale = 10.0 / _unit_norm(name, seed)
    a, b = _net(1), _net(1)
    tra, trb = a.trainable(name), b.trainable(name)
    arg = _backward(tra, name, seed, scale)
    _backward(trb, name, seed, scale)
    G, P0 = _grads(trb), _down(trb.parameters())
    assert all(np.array_equal(x, y) for x, y in zip(G, _grads(tra)))
    old = torch.optim.Adam(tra.parameters(), **hyper)                                      # the old way: three passes and a commit
    torch.nn.utils.clip_grad_norm_(list(tra.parameters()), max_norm)
    old.step()
    tra.commit()
    new = trb.optimizer(clip_grad_norm=max_norm, **hyper)                                  # the fused way
    new.step()
    Z = [np.zeros(p.shape) for p in P0]
    P, M, V, _, _ = F64.adam_step(P0, G, Z, Z, 1, max_norm=max_norm, **hyper)
    (tp, tm, tv), = _torch_f32_steps(P0, G, 1, max_norm, **hyper)
    _check_bound("old-path", param_names(name), _state(trb, new), (P, M, V), (tp, tm, tv))
    got_old = (_down(tra.parameters()), _down([old.state[p]["exp_avg"] for p in tra.parameters()]),
               _down([old.state[p]["exp_avg_sq"] for p in tra.parameters()]))
    bad = []
    for what, xs_, ys_, f, t in zip(("p", "exp_avg", "exp_avg_sq"), _state(trb, new), got_old, (P, M, V), (tp, tm, tv)):
        for k, x, y, r, z in zip(param_names(name), xs_, ys_, f, t):
            d, e_t32, s = float(np.abs(x.astype(np.float64) - y).max()), float(np.abs(z.astype(np.float64) - r).max()), float(np.abs(r).max())
            print(f"RATIO old-vs-fused {what} {k}: diff {d:.3e} err_t32 {e_t32:.3e} scale {s:.3e}")
            if not d <= K_F32 * e_t32 + 1e-7 * s:
                bad.append((what, k, d, e_t32, s))
    assert not bad, bad
    # the forwards that follow: each within the forward's own bound of float64 on the float64-stepped parameters
    xs = _inputs(name, LENGTHS, seed)
    ref, t32 = _torch_forward(name, P, xs, torch.float64), _torch_forward(name, tp, xs, torch.float32)
    e_t32 = FWD._err(t32, ref)
    for label, tr in (("old", tra), ("fused", trb)):
        e = FWD._err([y.detach().cpu() for y in tr(arg)], ref)
        print(f"RATIO old-path forward {label}: err {e:.3e} err_t32 {e_t32:.3e}")
        assert e <= K_F32 * e_t32 + 1e-7


# ---- 6: a skipped tensor --------------------------------------------------------------------------------------------------------------------
def test_a_tensor_without_gradient_is_skipped():
    name, seed = "rnn8", 67
    net = _net(1)
    tr = net.trainable(name)
    opt = tr.optimizer(lr=LR, clip_grad_norm=1.0)
    arg = _backward(tr, name, seed)
    opt.step()                                                                             # moments that are not zero
    _backward(tr, name, seed)
    names = param_names(name)
    i = names.index("linear2.bias")
    tr._params["linear2.bias"].grad = None
    G = _grads(tr)
    assert G[i] is None
    before = _state(tr, opt)
    norm = float(opt.step())
    after = _state(tr, opt)
    for q in range(3):
        for j, k in enumerate(names):
            assert np.array_equal(before[q][j], after[q][j]) == (j == i), (q, k)           # bitwise unchanged; everything else moved
    ref = F64.total_norm(G)                                                                # (None: left out of the float64 norm too)
    assert abs(norm - ref) <= 2e-7 * ref
    fresh = Net(body=synth.make_body(1), batch=1)
    fresh.load_state_dict(net.state_dict())
    assert all(_same(y.detach(), r) for y, r in zip(tr(arg), fresh.rnn8(arg)))


def test_a_gradient_view_off_the_16_byte_grid_steps_the_same():
    name, seed = "rnn8", 68
    outs = []
    for shifted in (False, True):
        tr = _net(1).trainable(name)
        opt = tr.optimizer(lr=LR, clip_grad_norm=1.0)
        _backward(tr, name, seed)
        if shifted:
            p = tr._params["rnn.weight_hh_l1"]
            buf = torch.empty(p.numel() + 1, device=p.device)
            buf[1:].copy_(p.grad.reshape(-1))
            p.grad = buf[1:].view(p.shape)
            assert p.grad.data_ptr() % 16 == 4
        opt.step()
        outs.append(_state(tr, opt))
    assert all(np.array_equal(u, w) for q, r in zip(*outs) for u, w in zip(q, r))


# ---- 7: determinism and resume ----------------------------------------------------------------------------------------------------------------
def _iterate(tr, opt, name, iters):
    for it in iters:
        _backward(tr, name, 70 + it)
        opt.step()
        opt.zero_grad()


def test_reruns_and_a_resumed_run_are_bitwise():
    name = "rnn8"
    hyper = dict(lr=LR, clip_grad_norm=1.0, weight_decay=0.01)

    def run(stop_after=None):
        net = _net(1)
        tr = net.trainable(name)
        opt = tr.optimizer(**hyper)
        _iterate(tr, opt, name, (0, 1))
        saved = (opt.state_dict(), {k: v.clone() for k, v in net.state_dict().items()}) if stop_after else None
        _iterate(tr, opt, name, (2,))
        return _state(tr, opt), saved

    (a, saved), (b, _) = run(True), run()
    same = lambda x, y: all(np.array_equal(u.view(np.int32), w.view(np.int32)) for q, r in zip(x, y) for u, w in zip(q, r))
    assert same(a, b)
    osd, nsd = saved
    assert sorted(osd["state"]) == list(range(12)) and all(float(v["step"]) == 2.0 for v in osd["state"].values())
    net = Net(body=synth.make_body(1), batch=1)
    net.load_state_dict(nsd)
    tr = net.trainable(name)
    opt = tr.optimizer()                                                                   # every hyper-parameter comes with the state
    opt.load_state_dict(osd)
    assert (opt.lr, opt.weight_decay, opt.step_count) == (LR, 0.01, 2)
    opt.clip_grad_norm = 1.0                                                               # (not part of torch's layout)
    _iterate(tr, opt, name, (2,))
    assert same(_state(tr, opt), a)
    real = torch.optim.Adam([torch.nn.Parameter(torch.empty_like(p)) for p in tr.parameters()])
    real.load_state_dict(osd)                                                              # a real Adam takes the saved state
    assert real.param_groups[0]["lr"] == LR
    assert all(torch.equal(real.state[p]["exp_avg"], v["exp_avg"]) for p, v in zip(real.param_groups[0]["params"], osd["state"].values()))
    opt.load_state_dict(real.state_dict())                                                 # ... and this object takes the real one's
    assert opt.step_count == 2


# ---- 8: the README loop learns ------------------------------------------------------------------------------------------------------------------
def test_the_loop_learns():
    name = "rnn8"
    lengths = (20, 7, 13, 20, 1, 16, 9, 20)
    xs = _inputs(name, lengths, 80)
    net = _net(1)
    target = 0.1 * torch.randn(sum(lengths), SPEC[name][2], generator=torch.Generator().manual_seed(81)).to(net.device)
    tr = net.trainable(name)
    opt = tr.optimizer(lr=1e-3, clip_grad_norm=1.0)
    losses = []
    for _ in range(20):
        loss = torch.nn.functional.mse_loss(torch.cat(tr(xs)), target)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("LOSSES fused: " + " ".join(f"{v:.5f}" for v in losses))
    assert losses[-1] < losses[0], losses
    assert all(_same(y.detach(), r) for y, r in zip(tr(xs), net.rnn8(xs)))


# ---- 9: bad input ---------------------------------------------------------------------------------------------------------------------------------
def test_bad_input_returns_codes_and_changes_nothing():
    name = "rnn8"
    net = _net(1)
    tr = net.trainable(name)
    opt = tr.optimizer(lr=LR)
    arg = _backward(tr, name, 90)
    ref = [y.clone() for y in net.rnn8(arg)]
    opt._ensure_moments()
    lib, ctx, sp = net._lib, net._ctx, _lib.stream_ptr()
    ps = [p.detach() for p in tr.parameters()]
    keep = _down(ps)
    tab = lambda ts: (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])
    P, G, M, V = tab(ps), tab([p.grad for p in tr.parameters()]), tab(opt.exp_avg), tab(opt.exp_avg_sq)
    out = torch.zeros(2, device=net.device)
    call = lambda net_name, P, M, n, o=out: lib.rc_subnet_optim_step(ctx, net_name, P, G, M, V, n, LR, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, 1.0,
                                                                      _lib.ptr(o), sp)
    assert call(b"rnn8", P, M, 11) == -1                                                   # wrong count
    assert call(b"rnn2", P, M, 12) == -1                                                   # rnn2 has 18
    assert call(b"rnn9", P, M, 12) == -1                                                   # unknown net
    assert call(b"rnn8", tab([None] + ps[1:]), M, 12) == -1                                # a null parameter
    assert call(b"rnn8", P, tab([None] + opt.exp_avg[1:]), 12) == -1                       # a null moment
    assert call(b"rnn8", P, M, 12, None) == -1                                             # nowhere to put the norm
    off = tab(ps)
    off[1] = ps[1].data_ptr() + 4
    assert call(b"rnn8", off, M, 12) == -1                                                 # an LSTM matrix off the 16-byte grid
    assert b"rc_subnet_optim_step" in lib.rc_last_error(ctx)
    torch.cuda.synchronize()
    assert all(np.array_equal(a, b) for a, b in zip(keep, _down(ps))) and not out.any()
    assert all(_same(y, r) for y, r in zip(net.rnn8(arg), ref))
    blank = Net(body=synth.make_body(1), batch=1)                                          # weights not finalised
    assert lib.rc_subnet_optim_step(blank._ctx, b"rnn8", P, G, M, V, 12, LR, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, 1.0, _lib.ptr(out), sp) == -3
