"""Training of one sub-net on the device (net.trainable(name): rc_subnet_forward_tape, rc_subnet_backward, rc_update_subnet_weights;
articulate/utils/torch/train.py:117-122 over rnn.py:121-133): values bitwise net.rnnK, every gradient against torch's own float64
autograd within K_F32 times the error of torch float32, in pieces, chunked, isolated from the Net, committed in place, and a loop that
learns."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import test_gpu_subnet_forward as FWD
from robustcap_amd import _lib
from robustcap_amd import config as cfg
from robustcap_amd import synth
from robustcap_amd.net.sig_mp import Net
from robustcap_amd.train import param_names

pytestmark = pytest.mark.gpu

SPEC = FWD.SPEC
K_F32 = FWD.K_F32         # the forward's bound: this multiple of torch fp32's own error on the CPU, per compared quantity
_sd, _net, _inputs, _same = FWD._sd, FWD._net, FWD._inputs, FWD._same


def _cotangents(name, lengths, seed):
    _, H, nout = SPEC[name]
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(T, nout, generator=g) for T in lengths], torch.randn(2, len(lengths), H, generator=g), torch.randn(2, len(lengths), H, generator=g)


def _init(name, N, seed):
    H = SPEC[name][1]
    g = torch.Generator().manual_seed(seed)
    return 0.5 * torch.randn(2, N, H, generator=g), 0.5 * torch.randn(2, N, H, generator=g)


def _loss(ys, hn, cn, cot):
    ry, rh, rc = cot
    dev, dt = ys[0].device, ys[0].dtype
    return sum((y * r.to(dev, dt)).sum() for y, r in zip(ys, ry)) + (hn * rh.to(dev, dt)).sum() + (cn * rc.to(dev, dt)).sum()


def _torch_grads(name, xs, init, cot, dtype, v=None):
    """The sub-net restated with nn.Linear, nn.LSTM and pack_sequence on the CPU in `dtype`, differentiated by torch's autograd: every
    compared quantity by name. v: rnn2's x_init [N, 69] (the initial state through init_net); else init = (h0, c0)."""
    from torch.nn.utils.rnn import pack_sequence, pad_packed_sequence
    nin, H, nout = SPEC[name]
    sd = _sd()
    t = lambda k: torch.from_numpy(sd[f"{name}.{k}"])
    l1, l2, rnn = torch.nn.Linear(nin, H).to(dtype), torch.nn.Linear(H, nout).to(dtype), torch.nn.LSTM(H, H, 2).to(dtype)
    mods = {"linear1": l1, "linear2": l2}
    with torch.no_grad():
        l1.weight.copy_(t("linear1.weight")); l1.bias.copy_(t("linear1.bias"))
        l2.weight.copy_(t("linear2.weight")); l2.bias.copy_(t("linear2.bias"))
        for k, p in rnn.named_parameters():
            p.copy_(t(f"rnn.{k}"))
    xs = [x.detach().clone().to(dtype).requires_grad_() for x in xs]
    if v is not None:
        inet = torch.nn.Sequential(torch.nn.Linear(69, 512), torch.nn.ReLU(), torch.nn.Linear(512, 1024), torch.nn.ReLU(),
                                   torch.nn.Linear(1024, 2048)).to(dtype)
        with torch.no_grad():
            for q in (0, 2, 4):
                inet[q].weight.copy_(t(f"init_net.{q}.weight")); inet[q].bias.copy_(t(f"init_net.{q}.bias"))
        v = v.detach().clone().to(dtype).requires_grad_()
        s = inet(v).view(-1, 2, 2, 512).permute(1, 2, 0, 3)
        h0, c0 = s[0].contiguous(), s[1].contiguous()
    else:
        h0, c0 = init[0].detach().clone().to(dtype).requires_grad_(), init[1].detach().clone().to(dtype).requires_grad_()
    out, (hn, cn) = rnn(pack_sequence([torch.relu(l1(x)) for x in xs], enforce_sorted=False), (h0, c0))
    out, _ = pad_packed_sequence(out)
    ys = [l2(out[: x.shape[0], i]) for i, x in enumerate(xs)]
    _loss(ys, hn, cn, cot).backward()
    q = {f"dx{i}": x.grad for i, x in enumerate(xs)}
    for m, mod in mods.items():
        q[f"{m}.weight"], q[f"{m}.bias"] = mod.weight.grad, mod.bias.grad
    q.update({f"rnn.{k}": p.grad for k, p in rnn.named_parameters()})
    if v is not None:
        q["d x_init"] = v.grad
        for i in (0, 2, 4):
            q[f"init_net.{i}.weight"], q[f"init_net.{i}.bias"] = inet[i].weight.grad, inet[i].bias.grad
    else:
        q["d init_h"], q["d init_c"] = h0.grad, c0.grad
    return {k: g.double().numpy() for k, g in q.items()}


def _gpu_grads(net, name, xs, init, cot, v=None):
    """The same quantities from tr = net.trainable(name)."""
    tr = net.trainable(name)
    xs = [x.detach().clone().requires_grad_() for x in xs]
    if v is not None:
        v = v.detach().clone().requires_grad_()
        ys, (hn, cn) = tr([(x, v[i]) for i, x in enumerate(xs)], return_state=True)
    else:
        h0, c0 = init[0].detach().clone().requires_grad_(), init[1].detach().clone().requires_grad_()
        ys, (hn, cn) = tr(xs, (h0, c0), return_state=True)
    _loss(ys, hn, cn, cot).backward()
    q = {f"dx{i}": x.grad for i, x in enumerate(xs)}
    q.update({k: p.grad for k, p in tr.named_parameters()})
    if v is not None:
        q["d x_init"] = v.grad
    else:
        q["d init_h"], q["d init_c"] = h0.grad, c0.grad
    return {k: g.detach().double().cpu().numpy() for k, g in q.items()}


@functools.lru_cache(maxsize=None)
def _case(name, lengths, seed, with_v=False):
    """Inputs and the two CPU references of a case, computed once and shared by both gemm modes."""
    xs = _inputs(name, lengths, seed)
    cot = _cotangents(name, lengths, seed + 100)
    init = None if with_v else _init(name, len(lengths), seed + 200)
    v = torch.randn(len(lengths), 69, generator=torch.Generator().manual_seed(seed + 300)) if with_v else None
    f64 = _torch_grads(name, xs, init, cot, torch.float64, v)
    t32 = _torch_grads(name, xs, init, cot, torch.float32, v)
    return xs, init, cot, v, f64, t32


def _check_bound(label, split, got, f64, t32):
    """max |q_gpu - q_f64| <= K_F32 max |q_t32 - q_f64| + 1e-7 max |q_f64| for every quantity; each figure is printed before it is held
    to the bound (profiles/subnet_backward_ratios.txt is this output)."""
    assert sorted(got) == sorted(f64), (sorted(got), sorted(f64))
    bad = []
    for k in sorted(f64):
        scale = float(np.abs(f64[k]).max())
        e_gpu, e_t32 = float(np.abs(got[k] - f64[k]).max()), float(np.abs(t32[k] - f64[k]).max())
        print(f"RATIO {label} mode={int(split)} {k}: scale {scale:.3e} err_gpu {e_gpu:.3e} err_t32 {e_t32:.3e} ratio {e_gpu / max(e_t32, 1e-300):.2f}")
        if not e_gpu <= K_F32 * e_t32 + 1e-7 * scale:
            bad.append((k, e_gpu, e_t32, scale))
    assert not bad, (label, split, bad)


def _run_case(label, name, lengths, seed, split, with_v=False):
    xs, init, cot, v, f64, t32 = _case(name, tuple(lengths), seed, with_v)
    got = _gpu_grads(_net(1, split), name, xs, init, cot, v)
    _check_bound(label, split, got, f64, t32)


# ---- 1: values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("name", [n for n, *_ in cfg.NETS])
def test_values_are_bitwise_the_inference_call(name, split):
    lengths = (1, 5, 64, 130, 257)
    xs = _inputs(name, lengths, 2)
    net = _net(1, split)
    tr = net.trainable(name)
    if name == "rnn2":
        v = torch.randn(len(lengths), 69, generator=torch.Generator().manual_seed(3))
        arg, init = [(x, v[i]) for i, x in enumerate(xs)], None
    else:
        arg, init = xs, _init(name, len(lengths), 3)
    ref, (rh, rc) = getattr(net, name)(arg, init, return_state=True)
    ys, (fh, fc) = tr(arg, init, return_state=True)
    assert all(_same(a, b) for a, b in zip(ys, ref)) and _same(fh, rh) and _same(fc, rc)
    assert all(y.requires_grad for y in ys) and fh.requires_grad
    assert [k for k, _ in tr.named_parameters()] == param_names(name)
    for k, p in tr.named_parameters():
        assert isinstance(p, torch.nn.Parameter) and p.is_cuda and tuple(p.shape) == tuple(_sd()[f"{name}.{k}"].shape)
        assert torch.equal(p.detach().cpu(), torch.from_numpy(_sd()[f"{name}.{k}"]))


# ---- 2: gradients against float64, ragged ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("name,lengths", [("rnn3", (1, 5, 64, 130, 257)), ("rnn8", (1, 5, 64, 130, 257)), ("rnn4", (1, 5, 33, 70)),
                                          ("rnn6", (1, 5, 33, 70)), ("rnn3", (1,))])
def test_gradients_against_float64_ragged(name, lengths, split):
    """rnn3: linear1's K padded 141 -> 256; rnn8: two outputs; rnn4 / rnn6: H = 1280 / 1024; (1,): one frame, no recurrent product."""
    _run_case(f"ragged-{name}-{len(lengths)}", name, lengths, 4, split)


# ---- 3: dispatch edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("N", [65, 520])
def test_gradients_at_the_dispatch_edges(N, split):
    """65 sequences of 1..96 frames: steps of 65 rows and of 64 and fewer (64-column / 16-column tiles); 520 sequences of 1..3 frames:
    steps above and below 512 rows (the 256-row tiles)."""
    rng = np.random.default_rng(N)
    lengths = rng.integers(1, 97, size=N).tolist() if N == 65 else rng.integers(1, 4, size=N).tolist()
    _run_case(f"edges-{N}", "rnn3", lengths, 5, split)


# ---- 4: rnn2 through init_net ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
def test_rnn2_through_init_net(split):
    _run_case("rnn2", "rnn2", (3, 40, 17), 6, split, with_v=True)


# ---- 5, 6: pieces equal the whole ------------------------------------------------------------------------------------------------
def _grads_of(tr, xs, init, cot, k=None):
    """dx per sequence, (d init_h, d init_c) and the parameter gradients of the loss of _loss; k: every sequence's head x[:k] and tail
    x[k:] as two calls chained by (h, c) forward, and so by d_init -> d_final backward."""
    tr.zero_grad()
    xs = [x.clone().requires_grad_() for x in xs]
    h0, c0 = init[0].clone().requires_grad_(), init[1].clone().requires_grad_()
    if k is None:
        ys, (hn, cn) = tr(xs, (h0, c0), return_state=True)
    else:
        keep = [i for i, x in enumerate(xs) if x.shape[0] > k]
        a, (h, c) = tr([x[:k] for x in xs], (h0, c0), return_state=True)
        b, (h2, c2) = tr([xs[i][k:] for i in keep], (h[:, keep], c[:, keep]), return_state=True)
        ys = [torch.cat([a[i], b[keep.index(i)]]) if i in keep else a[i] for i in range(len(xs))]
        hn, cn = h.clone(), c.clone()
        hn[:, keep], cn[:, keep] = h2, c2
    _loss(ys, hn, cn, cot).backward()
    torch.cuda.synchronize()
    return [x.grad for x in xs], (h0.grad, c0.grad), {n: p.grad.clone() for n, p in tr.named_parameters()}, ys


def _pieces(net, name, lengths, ks, seed):
    xs, cot, init = _inputs(name, lengths, seed), _cotangents(name, lengths, seed + 1), _init(name, len(lengths), seed + 2)
    tr = net.trainable(name)
    dx, dinit, gp, ys = _grads_of(tr, xs, init, cot)
    for k in ks:
        dx2, dinit2, gp2, ys2 = _grads_of(tr, xs, init, cot, k)
        for i in range(len(xs)):
            assert _same(ys2[i].detach(), ys[i].detach()) and _same(dx2[i], dx[i]), (k, i)
        assert _same(dinit2[0], dinit[0]) and _same(dinit2[1], dinit[1]), k
        for n in gp:
            scale = float(gp[n].abs().max())
            assert float((gp2[n] - gp[n]).abs().max()) <= 1e-5 * scale, (k, n)


@pytest.mark.parametrize("split", [False, True])
def test_pieces_equal_the_whole(split):
    _pieces(_net(1, split), "rnn6", (1, 9, 33, 70), (1, 8, 33, 50), 7)


@pytest.mark.parametrize("split", [False, True])
def test_pieces_equal_the_whole_at_a_chunk_boundary(split):
    """The forward's chunk test: 160 sequences through step 129 put the first boundary after 126 steps; the tape forward and the backward
    walk the same two chunks."""
    lengths = [200] * 150 + [130] * 10
    net = _net(1, split)
    tr = net.trainable("rnn3")
    c0 = net.subnet_stats()[2]
    ys = tr(_inputs("rnn3", lengths, 12))
    assert net.subnet_stats()[2] - c0 == 2
    c0 = net.subnet_stats()[2]
    torch.cat(ys).sum().backward()
    assert net.subnet_stats()[2] - c0 == 2
    _pieces(net, "rnn3", lengths, (126, 140), 12)


# ---- 7: isolation ------------------------------------------------------------------------------------------------------------------
def test_isolated_from_forward_sequence():
    s = np.load(FWD.GOLD)
    k = FWD._pending_frame(s)
    t = torch.from_numpy
    ft = t(s["first_tran"])[None] if s["first_tran"].size else None
    seq = lambda a, lo, hi: t(a[lo:hi])[None]

    def run(interrupt):
        net = FWD._fixture_net(s)
        p1, t1 = net.forward_sequence(seq(s["j2dc"], 0, k), seq(s["accc"], 0, k), seq(s["oric"], 0, k), ft, bool(s["first_frame"]))
        if interrupt:
            assert int(net.fusion_state()[0, 4]) == 1                  # the deferred updater step the calls must not flush
            for name, lengths in (("rnn6", [200] * 40), ("rnn2", (5, 3)), ("rnn4", (300, 7))):
                tr = net.trainable(name)
                xs = _inputs(name, lengths, 10)
                arg = [(x, torch.randn(69, generator=torch.Generator().manual_seed(11))) for x in xs] if name == "rnn2" else xs
                ys, (hn, cn) = tr(arg, return_state=True)
                (torch.cat(ys).square().sum() + hn.sum() + cn.sum()).backward()
                assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in tr.parameters())
        T = s["j2dc"].shape[0]
        p2, t2 = net.forward_sequence(seq(s["j2dc"], k, T), seq(s["accc"], k, T), seq(s["oric"], k, T))
        torch.cuda.synchronize()
        return torch.cat([p1, p2], 1).cpu(), torch.cat([t1, t2], 1).cpu(), FWD._state(net)

    a, b = run(False), run(True)
    assert _same(a[0], b[0]) and _same(a[1], b[1])
    FWD._same_state(a[2], b[2])


# ---- 8: commit ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _perturbed_sd():
    sd = dict(_sd())
    g = torch.Generator().manual_seed(31)
    for k in param_names("rnn4"):
        v = torch.from_numpy(sd[f"rnn4.{k}"])
        sd[f"rnn4.{k}"] = (v + 0.01 * torch.randn(v.shape, generator=g)).numpy()
    return sd


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("batch", [2, 48, 80])
def test_commit_equals_a_fresh_load(batch, split):
    """rnn4's perturbed parameters committed in place against a fresh Net that loaded the same tensors: the sub-net call, lstm_step
    (batch 48: the one-reader kernel, 80: the shared-weight kernel in split mode), state_dict; the other five nets as before; at
    batch 2 also a forward_sequence of 12 frames and one live frame."""
    body, new = synth.make_body(1), _perturbed_sd()
    a = Net(body=body, batch=batch); a.load_state_dict(_sd()); a.set_gemm_mode(split)
    b = Net(body=body, batch=batch); b.load_state_dict(new); b.set_gemm_mode(split)
    tr = a.trainable("rnn4")
    with torch.no_grad():
        for k, p in tr.named_parameters():
            p.copy_(torch.from_numpy(new[f"rnn4.{k}"]))
    tr.commit()
    for k, v in b.state_dict().items():
        assert torch.equal(a.state_dict()[k], v), k
    assert torch.equal(a.rnn4.rnn.weight_hh_l1, torch.from_numpy(new["rnn4.rnn.weight_hh_l1"]))
    xs = _inputs("rnn4", (3, 20, 7), 32)
    for y, r in zip(a.rnn4(xs), b.rnn4(xs)):
        assert _same(y, r)
    g = torch.Generator().manual_seed(33)
    for name, nin, _, _ in cfg.NETS:
        for _ in range(2):
            x = torch.randn(batch, nin, generator=g)
            assert _same(a.lstm_step(name, x), b.lstm_step(name, x)), name
    if batch == 2:
        m = synth.make_motion(5, batch, 12, body, conf="mixed")
        t = torch.from_numpy
        outs = []
        for net in (a, b):
            net.reset_states()
            net.gravityc = t(m["gravityc"])
            p, q = net.forward_sequence(t(m["j2dc"]), t(m["accc"]), t(m["oric"]), first_frame=True)
            lp, lq = net.forward_live(t(m["j2dc"][:, 0]), t(m["accc"][:, 0]), t(m["oric"][:, 0]))
            outs.append((p.cpu(), q.cpu(), lp, lq))
        assert all(_same(u, w) for u, w in zip(*outs))


def test_a_call_commits_stepped_parameters_first():
    net = _net(1)
    tr = net.trainable("rnn8")
    xs = _inputs("rnn8", (4, 2), 34)
    before = [y.detach().clone() for y in tr(xs)]
    with torch.no_grad():
        next(p for k, p in tr.named_parameters() if k == "linear2.bias").add_(1.0)
    after = tr(xs)                                                     # the version counter moved: committed by the call
    assert all(torch.allclose(y, r + 1.0, atol=1e-5) for y, r in zip(after, before))
    assert all(_same(y.detach(), r) for y, r in zip(after, net.rnn8(xs)))
    assert torch.equal(net.state_dict()["rnn8.linear2.bias"], torch.from_numpy(_sd()["rnn8.linear2.bias"]) + 1.0)
    with pytest.raises(_lib.RobustcapLibraryError):
        net.train(True)


# ---- 9: a training loop moves ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("name", ["rnn8", "rnn3"])
def test_a_training_loop_moves(name, split):
    lengths = (20, 7, 13, 20, 1, 16, 9, 20)
    xs = _inputs(name, lengths, 40)
    target = 0.1 * torch.randn(sum(lengths), SPEC[name][2], generator=torch.Generator().manual_seed(41))
    net = _net(1, split)
    tr = net.trainable(name)
    opt = torch.optim.SGD(tr.parameters(), lr=1e-2)
    losses = []
    for _ in range(8):
        loss = torch.nn.functional.mse_loss(torch.cat(tr(xs)), target.to(net.device))
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(f"LOSSES {name} mode={int(split)}: " + " ".join(f"{v:.5f}" for v in losses))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses


# ---- 10: bad input -----------------------------------------------------------------------------------------------------------------
def test_bad_input_raises_and_changes_nothing():
    net = _net(2)
    for name, nin, _, _ in cfg.NETS:                                   # a state that is not the initial one
        net.lstm_step(name, torch.randn(2, nin))
    tr4, tr2 = net.trainable("rnn4"), net.trainable("rnn2")
    x = _inputs("rnn4", (3,), 11)
    ref = net.rnn4(x)[0].cpu()
    before, stats = FWD._state(net), net.subnet_stats()
    for bad in ([], [torch.zeros(0, 171)], [torch.zeros(3, 170)], torch.zeros(3, 171)):
        with pytest.raises(ValueError):
            tr4(bad)
    with pytest.raises(ValueError):
        tr4(x, (torch.zeros(2, 2, 1280), torch.zeros(2, 1, 1280)))
    with pytest.raises(ValueError):
        tr4(x, torch.zeros(2, 1, 1280))
    with pytest.raises(ValueError):
        tr2([(torch.zeros(3, 72), torch.zeros(68))])
    with pytest.raises(ValueError):
        net.trainable("rnn5")
    # at the C level: a tape, acts or d_h1 whose allocation ends before the call's extent; a wrong tensor count
    lib, ctx, dev = net._lib, net._ctx, net.device
    lengths = (600, 400)
    F, N, H = sum(lengths), 2, 1280
    lens = (C.c_int32 * N)(*lengths)
    nfl = C.c_int64()
    assert lib.rc_subnet_tape_floats(ctx, b"rnn4", N, lens, C.byref(nfl)) == 0 and nfl.value == 2 * N * H + 10 * F * H
    assert lib.rc_subnet_tape_floats(ctx, b"rnn4", 0, lens, C.byref(nfl)) != 0
    big = lambda n: torch.zeros(n, device=dev)
    small = torch.zeros(16, device=dev)
    xc, y, acts, tape = big(F * 171), big(F * 69), big(3 * F * H), big(nfl.value)
    d_h1, d_gates, d_a = big(F * H), big(2 * F * 4 * H), big(F * H)
    p, sp = _lib.ptr, _lib.stream_ptr()
    for ac, tp in ((small, tape), (acts, small), (None, tape)):
        assert lib.rc_subnet_forward_tape(ctx, b"rnn4", N, lens, p(xc), p(y), None, None, None, None, p(ac), p(tp), sp) != 0
    for tp, dh in ((small, d_h1), (tape, small), (None, d_h1), (tape, None)):
        assert lib.rc_subnet_backward(ctx, b"rnn4", N, lens, p(tp), p(dh), None, None, p(d_gates), p(d_a), None, None, sp) != 0
    assert lib.rc_subnet_backward(ctx, b"rnn9", N, lens, p(tape), p(d_h1), None, None, p(d_gates), p(d_a), None, None, sp) != 0
    ptrs = (C.c_void_p * 12)(*[small.data_ptr()] * 12)
    assert lib.rc_update_subnet_weights(ctx, b"rnn4", ptrs, 11, sp) != 0
    assert lib.rc_update_subnet_weights(ctx, b"rnn2", ptrs, 12, sp) != 0
    assert net.subnet_stats() == stats                                 # nothing ran
    FWD._same_state(before, FWD._state(net))
    assert _same(net.rnn4(x)[0], ref)
