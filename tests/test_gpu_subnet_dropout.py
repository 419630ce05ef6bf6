"""Training a sub-net with the reference's dropout (tr.train(): rc_dropout_apply, rc_subnet_forward_train, rc_subnet_backward_train;
articulate/utils/torch/rnn.py:115,130-131 and torch.nn.LSTM's dropout): the mask bit for bit against a numpy Philox4x32-10, eval mode
untouched, site 0 exactly across chunks, values and every gradient against a float64 restatement within K_F32 times the error of the
same restatement in float32, determinism and the saved state, a loop that learns, and bad input."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import subnet_dropout_ref as R
import test_gpu_subnet_backward as BWD
import test_gpu_subnet_forward as FWD
from robustcap_amd import _lib
from robustcap_amd import config as cfg
from robustcap_amd.train import param_names

pytestmark = pytest.mark.gpu

SPEC = FWD.SPEC
_sd, _net, _inputs, _same = FWD._sd, FWD._net, FWD._inputs, FWD._same
RAGGED = (1, 5, 64, 130, 257)
TWO_CHUNKS = tuple([200] * 150 + [130] * 10)       # the existing chunk tests' shape (rnn3): the first boundary after 126 steps
SEED = (0x9E3779B9 << 32) | 0x1234ABCD               # both halves of the key in use


def _apply(net, src, site, p, seed, call, out=None):
    out = torch.empty_like(src) if out is None else out
    rc = net._lib.rc_dropout_apply(net._ctx, _lib.ptr(src), _lib.ptr(out), src.shape[0], src.shape[1], site, p, seed, call, _lib.stream_ptr())
    assert rc == 0, rc
    return out


# ---- 1: the mask, bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(1, 512), (17, 512), (457, 1280)])
def test_mask_bits(rows, cols):
    net = _net()
    dev = net.device
    ones = torch.ones(rows, cols, device=dev)
    x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows)).to(dev)
    for p in (0.4, 0.1):
        for site in (0, 1):
            for call in (0, 3000000001):
                want = R.scaled_mask(rows, cols, site, p, SEED, call)
                got = _apply(net, ones, site, p, SEED, call)
                assert _same(got, torch.from_numpy(want)), (p, site, call)
                y = _apply(net, x, site, p, SEED, call)
                ref = np.where(want != 0, x.cpu().numpy() * R.scale(p), np.float32(0.0)).astype(np.float32)
                assert _same(y, torch.from_numpy(ref)), (p, site, call)        # kept: x * s; dropped: +0, whatever x's sign
                z = x.clone()
                assert _apply(net, z, site, p, SEED, call, out=z) is z and _same(z, y)
    assert not _same(_apply(net, ones, 0, 0.4, SEED, 0), _apply(net, ones, 0, 0.4, SEED ^ (1 << 40), 0))   # the key's high half counts
    assert _same(_apply(net, x, 1, 0.0, SEED, 7), x)                               # p = 0 copies
    z = x.clone()
    assert _same(_apply(net, z, 1, 0.0, SEED, 7, out=z), x)


# ---- the C entries, called the way robustcap_amd/train.py calls them ---------------------------------------------------------------
def _c_forward(net, name, lengths, xcat, drop):
    """drop None: rc_subnet_forward_tape; (p, seed, call): rc_subnet_forward_train. Returns y, final_h, final_c, acts, tape."""
    nin, H, nout = SPEC[name]
    dev, N, F = net.device, len(lengths), sum(lengths)
    lens = (C.c_int32 * N)(*lengths)
    nfl = C.c_int64()
    assert net._lib.rc_subnet_tape_floats(net._ctx, name.encode(), N, lens, C.byref(nfl)) == 0
    y, fh, fc = torch.empty(F, nout, device=dev), torch.empty(2, N, H, device=dev), torch.empty(2, N, H, device=dev)
    acts, tape = torch.empty(3, F, H, device=dev), torch.empty(nfl.value, device=dev)
    p = _lib.ptr
    args = (net._ctx, name.encode(), N, lens, p(xcat), p(y), None, None, p(fh), p(fc), p(acts), p(tape))
    if drop is None:
        rc = net._lib.rc_subnet_forward_tape(*args, _lib.stream_ptr())
    else:
        rc = net._lib.rc_subnet_forward_train(*args, *drop, _lib.stream_ptr())
    assert rc == 0, rc
    return y, fh, fc, acts, tape


def _c_backward(net, name, lengths, tape, d_h1, drop):
    nin, H, nout = SPEC[name]
    dev, N, F = net.device, len(lengths), sum(lengths)
    lens = (C.c_int32 * N)(*lengths)
    d_gates, d_a = torch.empty(2, F, 4 * H, device=dev), torch.empty(F, H, device=dev)
    d_ih, d_ic = torch.empty(2, N, H, device=dev), torch.empty(2, N, H, device=dev)
    p = _lib.ptr
    args = (net._ctx, name.encode(), N, lens, p(tape), p(d_h1), None, None, p(d_gates), p(d_a), p(d_ih), p(d_ic))
    if drop is None:
        rc = net._lib.rc_subnet_backward(*args, _lib.stream_ptr())
    else:
        rc = net._lib.rc_subnet_backward_train(*args, *drop, _lib.stream_ptr())
    assert rc == 0, rc
    return d_gates, d_a, d_ih, d_ic


# ---- 2: eval is untouched --------------------------------------------------------------------------------------------------------------
def _run(tr, xs, init, cot):
    tr.zero_grad()
    xs = [x.clone().requires_grad_() for x in xs]
    h0, c0 = init[0].clone().requires_grad_(), init[1].clone().requires_grad_()
    ys, (hn, cn) = tr(xs, (h0, c0), return_state=True)
    BWD._loss(ys, hn, cn, cot).backward()
    out = {"y": torch.cat(ys).detach(), "h_n": hn.detach(), "c_n": cn.detach(), "dx": torch.cat([x.grad for x in xs]),
           "d init_h": h0.grad, "d init_c": c0.grad}
    out.update({k: p.grad.clone() for k, p in tr.named_parameters()})
    return out


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("name", ["rnn8", "rnn4"])
def test_eval_is_untouched(name, split):
    """A trainer left as constructed, one sent through train() and back to eval(), and one in training mode at rate 0: the same bits in
    y, the final state and every gradient, y those of net.rnnK, and no call counted. At the C level the *_train entries with p = 0 are
    bitwise rc_subnet_forward_tape / rc_subnet_backward."""
    net = _net(1, split)
    xs, cot, init = _inputs(name, RAGGED, 2), BWD._cotangents(name, RAGGED, 102), BWD._init(name, len(RAGGED), 202)
    plain = net.trainable(name)
    assert plain.training is False and plain.dropout == cfg.DROPOUT[name] and plain.dropout_state() == {"seed": 0, "call": 0}
    ref = _run(plain, xs, init, cot)
    ys, (fh, fc) = getattr(net, name)(xs, init, return_state=True)
    assert _same(ref["y"], torch.cat(ys)) and _same(ref["h_n"], fh) and _same(ref["c_n"], fc)
    back = net.trainable(name).train()
    back.manual_seed(5)
    _run(back, xs, init, cot)                                                  # a train-mode iteration in between
    assert back.dropout_state() == {"seed": 5, "call": 1}
    zero = net.trainable(name).train()
    zero.dropout = 0.0
    for tr in (back.eval(), zero):
        state = tr.dropout_state()
        got = _run(tr, xs, init, cot)
        assert sorted(got) == sorted(ref)
        for k in ref:
            assert _same(got[k], ref[k]), (name, split, k)
        assert tr.dropout_state() == state
    lengths, xcat = list(RAGGED), torch.cat(xs).to(net.device)
    a, b = _c_forward(net, name, lengths, xcat, None), _c_forward(net, name, lengths, xcat, (0.0, SEED, 3))
    assert all(_same(u, w) for u, w in zip(a, b))
    d_h1 = torch.randn(sum(lengths), SPEC[name][1], generator=torch.Generator().manual_seed(9)).to(net.device)
    ga, gb = _c_backward(net, name, lengths, a[4], d_h1, None), _c_backward(net, name, lengths, a[4], d_h1, (0.0, SEED, 3))
    assert all(_same(u, w) for u, w in zip(ga, gb))


# ---- 3: site 0 exactly, across chunks ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("name,lengths,chunks", [("rnn8", RAGGED, 1), ("rnn4", RAGGED, 1), ("rnn3", TWO_CHUNKS, 2)])
def test_site0_is_exactly_the_mask_on_the_eval_activations(name, lengths, chunks, split):
    """linear1 is the same launch in both modes, so the train-mode acts[0] is rc_dropout_apply(eval-mode acts[0], site 0) bit for bit --
    keyed by the caller's rows, also where the call runs as two chunks. acts[1] and y then differ from eval mode's."""
    net = _net(1, split)
    p = np.float32(cfg.DROPOUT[name]).item()
    xcat = torch.cat(_inputs(name, lengths, 12)).to(net.device)
    ev = _c_forward(net, name, list(lengths), xcat, None)
    c0 = net.subnet_stats()[2]
    tn = _c_forward(net, name, list(lengths), xcat, (p, SEED, 4))
    assert net.subnet_stats()[2] - c0 == chunks
    assert _same(tn[3][0], _apply(net, ev[3][0].contiguous(), 0, p, SEED, 4))
    assert not _same(tn[3][1], ev[3][1]) and not _same(tn[0], ev[0])
    dropped = float((tn[3][0] == 0).float().mean()) - float((ev[3][0] == 0).float().mean())
    assert dropped > 0.5 * p * float((ev[3][0] > 0).float().mean())


# ---- 4: values and gradients against float64 ----------------------------------------------------------------------------------------
def _restated(name, lengths, xs, init, v, cot, p, seed, call, dtype, device):
    """tests/subnet_dropout_ref.py's train-mode forward in `dtype` on `device` with the helper's masks, differentiated by autograd:
    every compared quantity by name, as float64 numpy."""
    nin, H, nout = SPEC[name]
    sd = _sd()
    t = lambda a: a.detach().to(device=device, dtype=dtype)
    P = {k: t(torch.from_numpy(sd[f"{name}.{k}"])).requires_grad_() for k in param_names(name)}
    F = sum(lengths)
    xcat = t(torch.cat(xs)).requires_grad_()
    m0 = t(torch.from_numpy(R.scaled_mask(F, H, 0, p, seed, call)))
    m1 = t(torch.from_numpy(R.scaled_mask(F, H, 1, p, seed, call)))
    if v is not None:
        v = t(v).requires_grad_()
        a = torch.relu(v @ P["init_net.0.weight"].t() + P["init_net.0.bias"])
        a = torch.relu(a @ P["init_net.2.weight"].t() + P["init_net.2.bias"])
        s = (a @ P["init_net.4.weight"].t() + P["init_net.4.bias"]).view(-1, 2, 2, 512).permute(1, 2, 0, 3)
        h0, c0 = s[0], s[1]
    else:
        h0, c0 = t(init[0]).requires_grad_(), t(init[1]).requires_grad_()
    y, hn, cn = R.forward_train(P, xcat, list(lengths), h0, c0, m0, m1)
    BWD._loss(torch.split(y, list(lengths)), hn, cn, cot).backward()
    q = {"y": y, "h_n": hn, "c_n": cn, "dx": xcat.grad}
    q.update({k: w.grad for k, w in P.items()})
    if v is not None:
        q["d x_init"] = v.grad
    else:
        q["d init_h"], q["d init_c"] = h0.grad, c0.grad
    return {k: g.detach().double().cpu().numpy() for k, g in q.items()}


def _inputs_of(name, lengths, seed, with_v):
    xs = _inputs(name, lengths, seed)
    cot = BWD._cotangents(name, lengths, seed + 100)
    init = None if with_v else BWD._init(name, len(lengths), seed + 200)
    v = torch.randn(len(lengths), 69, generator=torch.Generator().manual_seed(seed + 300)) if with_v else None
    return xs, cot, init, v


@functools.lru_cache(maxsize=None)
def _references(name, lengths, seed, with_v, device):
    """The float64 and the float32 restatement of a case, computed once and shared by both gemm modes."""
    xs, cot, init, v = _inputs_of(name, lengths, seed, with_v)
    p = np.float32(cfg.DROPOUT[name]).item()
    return tuple(_restated(name, lengths, xs, init, v, cot, p, SEED + seed, 0, dt, device) for dt in (torch.float64, torch.float32))


def _trained(net, name, lengths, seed, with_v):
    """The same quantities from tr = net.trainable(name).train(), first call after manual_seed (call 0)."""
    xs, cot, init, v = _inputs_of(name, lengths, seed, with_v)
    tr = net.trainable(name).train()
    tr.manual_seed(SEED + seed)
    xs = [x.clone().requires_grad_() for x in xs]
    if with_v:
        v = v.clone().requires_grad_()
        ys, (hn, cn) = tr([(x, v[i]) for i, x in enumerate(xs)], return_state=True)
    else:
        h0, c0 = init[0].clone().requires_grad_(), init[1].clone().requires_grad_()
        ys, (hn, cn) = tr(xs, (h0, c0), return_state=True)
    BWD._loss(ys, hn, cn, cot).backward()
    q = {"y": torch.cat(ys), "h_n": hn, "c_n": cn, "dx": torch.cat([x.grad for x in xs])}
    q.update({k: w.grad for k, w in tr.named_parameters()})
    if with_v:
        q["d x_init"] = v.grad
    else:
        q["d init_h"], q["d init_c"] = h0.grad, c0.grad
    assert tr.dropout_state()["call"] == 1
    return {k: g.detach().double().cpu().numpy() for k, g in q.items()}


CASES = {
    "rnn8-ragged": ("rnn8", RAGGED, False), "rnn3-ragged": ("rnn3", RAGGED, False),          # H = 512; rnn3: linear1's K padded
    "rnn4-ragged": ("rnn4", (1, 5, 33, 70), False),                                          # H = 1280
    "rnn7-p0.1": ("rnn7", (3, 40), False),                                                   # the other rate
    "rnn2-init_net": ("rnn2", (2, 19, 66), True),                                            # the initial state through init_net
    "rnn3-65x3": ("rnn3", (3,) * 65, False),                                                 # steps of 65 rows: the 64 / 65-row dispatch edge
}


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("case", sorted(CASES))
def test_train_mode_against_float64(case, split):
    """err_gpu <= K_F32 err_torch_fp32 + 1e-7 scale for y, the final state, dx, d init and every parameter gradient (the bound of
    test_gpu_subnet_backward.py), in training mode with the helper's masks; the references on the CPU."""
    name, lengths, with_v = CASES[case]
    f64, t32 = _references(name, lengths, 20, with_v, "cpu")
    got = _trained(_net(1, split), name, lengths, 20, with_v)
    BWD._check_bound(f"dropout-{case}", split, got, f64, t32)


@pytest.mark.parametrize("split", [False, True])
def test_train_mode_against_float64_across_a_chunk_boundary(split):
    """The two-chunk shape: the forward's h of layer 0 -> dropped copy and the backward's mask on dG1 . W_ih1 both take the caller's
    rows through each chunk's map. The float64 and float32 restatements run as plain torch matmuls on the device."""
    net = _net(1, split)
    f64, t32 = _references("rnn3", TWO_CHUNKS, 21, False, "cuda")
    c0 = net.subnet_stats()[2]
    got = _trained(net, "rnn3", TWO_CHUNKS, 21, False)
    assert net.subnet_stats()[2] - c0 == 4                                     # two chunks forward, two backward
    BWD._check_bound("dropout-rnn3-two-chunks", split, got, f64, t32)


# ---- 5: determinism and state ---------------------------------------------------------------------------------------------------------
def test_determinism_and_state():
    net = _net()
    lengths = (7, 3, 12)
    xs, cot, init = _inputs("rnn8", lengths, 30), BWD._cotangents("rnn8", lengths, 31), BWD._init("rnn8", 3, 32)
    tr = net.trainable("rnn8").train()
    assert tr.manual_seed(77) is tr
    a0 = _run(tr, xs, init, cot)
    saved = tr.dropout_state()
    assert saved == {"seed": 77, "call": 1}
    a1 = _run(tr, xs, init, cot)
    a2 = _run(tr, xs, init, cot)
    assert tr.dropout_state() == {"seed": 77, "call": 3}
    assert not _same(a0["y"], a1["y"]) and not _same(a1["y"], a2["y"])           # consecutive calls: consecutive counters, other masks
    tr.set_dropout_state(saved)
    b1 = _run(tr, xs, init, cot)
    tr.manual_seed(77)                                                         # ... resets the counter
    assert tr.dropout_state() == {"seed": 77, "call": 0}
    b0 = _run(tr, xs, init, cot)
    for k in a0:
        assert _same(a0[k], b0[k]) and _same(a1[k], b1[k]), k
    other = net.trainable("rnn8").train()                                      # the masks belong to (seed, call), not to the object
    other.set_dropout_state({"seed": 77, "call": 2})
    c2 = _run(other, xs, init, cot)
    assert all(_same(a2[k], c2[k]) for k in a2)
    tr.manual_seed(78)
    assert not _same(_run(tr, xs, init, cot)["y"], a0["y"])
    # no_grad in training mode: the eval path, and the counter stays
    state = tr.dropout_state()
    with torch.no_grad():
        ys = tr(xs, init)
    assert tr.dropout_state() == state
    assert all(_same(y, r) for y, r in zip(ys, net.rnn8(xs, init)))


# ---- 6: a loop that learns in training mode ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
def test_a_training_loop_learns_with_dropout(split):
    lengths = (20, 7, 13, 20, 1, 16, 9, 20)
    xs = _inputs("rnn8", lengths, 40)
    net = _net(1, split)
    target = 0.1 * torch.randn(sum(lengths), SPEC["rnn8"][2], generator=torch.Generator().manual_seed(41)).to(net.device)
    tr = net.trainable("rnn8")
    tr.manual_seed(42)
    opt = tr.optimizer(lr=1e-3, clip_grad_norm=1.0)

    def eval_loss():
        tr.eval()
        with torch.no_grad():
            return float(torch.nn.functional.mse_loss(torch.cat(tr(xs)), target))

    before = eval_loss()
    for _ in range(20):
        tr.train()
        loss = torch.nn.functional.mse_loss(torch.cat(tr(xs)), target)
        opt.zero_grad()
        loss.backward()
        opt.step()
    after = eval_loss()
    print(f"EVAL LOSS rnn8 mode={int(split)}: {before:.5f} -> {after:.5f} after 20 train-mode iterations")
    assert tr.dropout_state() == {"seed": 42, "call": 20}
    assert after < before


# ---- 7: bad input ---------------------------------------------------------------------------------------------------------------------
def test_bad_input_is_rejected_and_changes_nothing():
    net = _net()
    lib, ctx, dev = net._lib, net._ctx, net.device
    tr = net.trainable("rnn8").train()
    tr.manual_seed(50)
    lengths = (6, 2)
    xs, cot, init = _inputs("rnn8", lengths, 51), BWD._cotangents("rnn8", lengths, 52), BWD._init("rnn8", 2, 53)
    ref = _run(tr, xs, init, cot)
    src = torch.randn(8, 512, generator=torch.Generator().manual_seed(54)).to(dev)
    good = _apply(net, src, 0, 0.4, 1, 2)
    stats, state = net.subnet_stats(), tr.dropout_state()
    dst = torch.full_like(src, 7.0)
    p, sp = _lib.ptr, _lib.stream_ptr()
    INVALID = -1
    for bad_p in (1.0, 1.5, -0.1, float("nan")):
        assert lib.rc_dropout_apply(ctx, p(src), p(dst), 8, 512, 0, bad_p, 1, 2, sp) == INVALID
    assert lib.rc_dropout_apply(ctx, p(src), p(dst), 8, 510, 0, 0.4, 1, 2, sp) == INVALID       # cols % 4
    assert lib.rc_dropout_apply(ctx, p(src), p(dst), 8, 0, 0, 0.4, 1, 2, sp) == INVALID
    assert lib.rc_dropout_apply(ctx, p(src), p(dst), 0, 512, 0, 0.4, 1, 2, sp) == INVALID
    assert lib.rc_dropout_apply(ctx, p(src), p(dst), 1 << 32, 4, 0, 0.4, 1, 2, sp) == INVALID
    for site in (2, -1):
        assert lib.rc_dropout_apply(ctx, p(src), p(dst), 8, 512, site, 0.4, 1, 2, sp) == INVALID
    assert lib.rc_dropout_apply(ctx, None, p(dst), 8, 512, 0, 0.4, 1, 2, sp) == INVALID
    assert lib.rc_dropout_apply(ctx, p(src), None, 8, 512, 0, 0.4, 1, 2, sp) == INVALID
    assert lib.rc_dropout_apply(ctx, p(src), p(dst), 1 << 22, 512, 0, 0.4, 1, 2, sp) == INVALID   # 8 GiB: past the end of either allocation
    assert lib.rc_dropout_apply(ctx, C.c_void_p(src.data_ptr() + 4), p(dst), 7, 512, 0, 0.4, 1, 2, sp) == INVALID   # 16-byte alignment
    assert b"rc_dropout_apply" in lib.rc_last_error(ctx)
    assert lib.rc_dropout_apply(None, p(src), p(dst), 8, 512, 0, 0.4, 1, 2, sp) == INVALID
    xcat = torch.cat(xs).to(dev)
    N, F, H = 2, sum(lengths), 512
    lens = (C.c_int32 * N)(*lengths)
    big = lambda n: torch.zeros(n, device=dev)
    y, acts, tape = big(F * 2), big(3 * F * H), big(2 * N * H + 10 * F * H)
    d_h1, d_gates, d_a = big(F * H), big(8 * F * H), big(F * H)
    for bad_p in (1.0, -0.5, float("nan")):
        assert lib.rc_subnet_forward_train(ctx, b"rnn8", N, lens, p(xcat), p(y), None, None, None, None, p(acts), p(tape), bad_p, 1, 2, sp) == INVALID
        assert lib.rc_subnet_backward_train(ctx, b"rnn8", N, lens, p(tape), p(d_h1), None, None, p(d_gates), p(d_a), None, None, bad_p, 1, 2,
                                            sp) == INVALID
    assert lib.rc_subnet_forward_train(ctx, b"rnn8", N, lens, p(xcat), p(y), None, None, None, None, None, p(tape), 0.4, 1, 2, sp) == INVALID
    assert lib.rc_subnet_backward_train(ctx, b"rnn8", N, lens, None, p(d_h1), None, None, p(d_gates), p(d_a), None, None, 0.4, 1, 2, sp) == INVALID
    for bad in (1.0, -0.25, float("nan")):
        tr.dropout = bad
        with pytest.raises(ValueError):
            tr(xs, init)
    tr.dropout = cfg.DROPOUT["rnn8"]
    with pytest.raises(ValueError):
        tr([torch.zeros(3, 140)])                                              # a bad x in training mode: no call is counted
    with pytest.raises(ValueError):
        tr.set_dropout_state({"seed": 1 << 64, "call": 0})
    with pytest.raises(_lib.RobustcapLibraryError):
        net.train(True)                                                        # the Net itself stays the inference path
    torch.cuda.synchronize()
    assert net.subnet_stats() == stats and tr.dropout_state() == state         # nothing ran, nothing was counted
    assert bool((dst == 7.0).all()) and not bool(y.any()) and not bool(d_a.any())
    assert _same(_apply(net, src, 0, 0.4, 1, 2), good)
    tr.manual_seed(50)
    again = _run(tr, xs, init, cot)
    assert all(_same(again[k], ref[k]) for k in ref)
