"""Sub-nets over ragged sequences (net.rnnK(x, init) = articulate/utils/torch/rnn.py:121-133 RNN.forward, net.rnn2 = RNNWithInit):
bitwise the frame-stepped path (rc_lstm_step) in each gemm mode, against float64, in pieces, chunked, and isolated from the Net."""
import os

import numpy as np
import pytest
import torch

from oracle import lstm_f64
from robustcap_amd import config as cfg
from robustcap_amd import synth
from robustcap_amd.net.sig_mp import Net

pytestmark = pytest.mark.gpu

SPEC = {n: (i, h, o) for n, i, h, o in cfg.NETS}
SD = None
BUDGET = 256 << 20            # RC_SUBNET_SCRATCH_BYTES: per-chunk buffers


def _sd():
    global SD
    if SD is None:
        SD = synth.make_state_dict(0)
    return SD


def _net(batch=1, split=None):
    net = Net(body=synth.make_body(1), batch=batch)
    net.load_state_dict(_sd())
    if split is not None:
        net.set_gemm_mode(split)
    return net


def _inputs(name, lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(T, SPEC[name][0], generator=g) for T in lengths]


def _stepped(name, xs, split):
    """Frame by frame through rc_lstm_step on a fresh Net(batch=N); rows past their end are masked and fed NaN."""
    N, Tmax = len(xs), max(x.shape[0] for x in xs)
    nin, H, nout = SPEC[name]
    net = _net(N, split)
    ys = [torch.empty(x.shape[0], nout) for x in xs]
    for t in range(Tmax):
        rows = torch.tensor([x.shape[0] > t for x in xs])
        xt = torch.full((N, nin), float("nan"))
        for i, x in enumerate(xs):
            if x.shape[0] > t:
                xt[i] = x[t]
        y = net.lstm_step(name, xt, rows=rows).cpu()
        for i, x in enumerate(xs):
            if x.shape[0] > t:
                ys[i][t] = y[i]
    return ys, net.get_state(name)


def _same(a, b):
    return torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


def test_the_sub_nets_are_callable():
    net = _net()
    x1, x2 = _inputs("rnn4", (3, 7), 1)
    y = net.rnn4([x1, x2])
    assert [tuple(t.shape) for t in y] == [(3, 69), (7, 69)] and y[0].is_cuda and y[0].dtype == torch.float32
    assert [tuple(t.shape) for t in net.rnn4.forward([x1])] == [(3, 69)]
    v = torch.randn(2, 69)
    out = net.rnn2.init_net(v)
    assert tuple(out.shape) == (2, 2048)
    y2 = net.rnn2([(torch.randn(4, 72), v[0]), (torch.randn(2, 72), v[1])])
    assert [tuple(t.shape) for t in y2] == [(4, 69), (2, 69)]
    calls, frames, chunks, scratch = net.subnet_stats()
    assert calls == 5 and frames == 10 + 3 + 2 + 2 + 6 and chunks >= 5 and 0 < scratch


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("name", [n for n, *_ in cfg.NETS])
def test_bitwise_the_stepped_path_ragged(name, split):
    xs = _inputs(name, (1, 5, 64, 130, 257), 2)
    ref, (h, c) = _stepped(name, xs, split)
    net = _net(1, split)
    ys, (fh, fc) = net._subnet_forward(name, xs, return_state=True)
    for i in range(len(xs)):
        assert _same(ys[i], ref[i]), (name, split, i)
    assert _same(fh, h) and _same(fc, c)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("N", [65, 256])
@pytest.mark.parametrize("name", ["rnn4", "rnn6", "rnn3"])
def test_bitwise_the_stepped_path_many_sequences(name, N, split):
    """Crosses the stepped path's dispatch edges (64 / 65 rows, the shared-weight kernel at 256 rows in split mode)."""
    lengths = np.random.default_rng(N).integers(1, 97, size=N).tolist()
    xs = _inputs(name, lengths, 3)
    ref, (h, c) = _stepped(name, xs, split)
    ys, (fh, fc) = _net(1, split)._subnet_forward(name, xs, return_state=True)
    assert all(_same(ys[i], ref[i]) for i in range(N))
    assert _same(fh, h) and _same(fc, c)


def _torch_f32_cpu(name, xs, h0, c0, dtype):
    """torch's own packed-sequence construction (nn.Linear + nn.LSTM + pack_padded_sequence) on the CPU in `dtype`."""
    from torch.nn.utils.rnn import pack_sequence, pad_packed_sequence
    nin, H, nout = SPEC[name]
    sd = _sd()
    l1, l2 = torch.nn.Linear(nin, H).to(dtype), torch.nn.Linear(H, nout).to(dtype)
    rnn = torch.nn.LSTM(H, H, 2).to(dtype)
    with torch.no_grad():
        l1.weight.copy_(torch.from_numpy(sd[f"{name}.linear1.weight"])); l1.bias.copy_(torch.from_numpy(sd[f"{name}.linear1.bias"]))
        l2.weight.copy_(torch.from_numpy(sd[f"{name}.linear2.weight"])); l2.bias.copy_(torch.from_numpy(sd[f"{name}.linear2.bias"]))
        for k, v in rnn.named_parameters():
            v.copy_(torch.from_numpy(sd[f"{name}.rnn.{k}"]))
        a = pack_sequence([torch.relu(l1(x.to(dtype))) for x in xs], enforce_sorted=False)
        out, (hn, cn) = rnn(a, (h0.to(dtype), c0.to(dtype)))
        out, _ = pad_packed_sequence(out)
        return [l2(out[: x.shape[0], i]) for i, x in enumerate(xs)], (hn, cn)


def _f64(name, xs, h0, c0):
    p = lstm_f64.params(_sd(), name)
    N, Tmax = len(xs), max(x.shape[0] for x in xs)
    h, c = h0.double().numpy().copy(), c0.double().numpy().copy()
    ys = [np.zeros((x.shape[0], SPEC[name][2])) for x in xs]
    for t in range(Tmax):
        mask = np.array([x.shape[0] > t for x in xs])
        xt = np.stack([x[min(t, x.shape[0] - 1)].double().numpy() for x in xs])
        y, h, c, _ = lstm_f64.step(p, xt, h, c, mask)
        for i, x in enumerate(xs):
            if x.shape[0] > t:
                ys[i][t] = y[i]
    return ys, (h, c)


def _err(a, b):
    return max(float(np.abs(np.asarray(u, dtype=np.float64) - np.asarray(v, dtype=np.float64)).max()) for u, v in zip(a, b))


K_F32 = 8          # bound: this multiple of the error torch fp32 reaches on the CPU on the same data, per compared quantity


@pytest.mark.parametrize("split", [False, True])
def test_against_float64_with_init(split):
    """RNN with a random non-zero init and RNNWithInit (rnn2 through a float64 init_net): outputs, h_n and c_n each within K_F32 times
    the error of torch fp32 on the CPU in the same quantity."""
    name, lengths = "rnn3", (3, 40, 17)
    nin, H, _ = SPEC[name]
    xs = _inputs(name, lengths, 4)
    g = torch.Generator().manual_seed(5)
    h0, c0 = 0.5 * torch.randn(2, len(xs), H, generator=g), 0.5 * torch.randn(2, len(xs), H, generator=g)
    ref, (rh, rc) = _f64(name, xs, h0, c0)
    t32, (th, tc) = _torch_f32_cpu(name, xs, h0, c0, torch.float32)
    ys, (fh, fc) = _net(1, split)._subnet_forward(name, xs, (h0, c0), return_state=True)
    assert _err([y.cpu() for y in ys], ref) <= K_F32 * _err([y.numpy() for y in t32], ref) + 1e-7
    assert _err([fh.cpu()], [rh]) <= K_F32 * _err([th.numpy()], [rh]) + 1e-7
    assert _err([fc.cpu()], [rc]) <= K_F32 * _err([tc.numpy()], [rc]) + 1e-7
    # rnn2: init_net in float64, then the same loop
    sd = _sd()
    v = torch.randn(len(xs), 69, generator=g)
    a = v.double().numpy()
    for q, relu in ((0, True), (2, True), (4, False)):
        a = a @ sd[f"rnn2.init_net.{q}.weight"].astype(np.float64).T + sd[f"rnn2.init_net.{q}.bias"]
        a = np.maximum(a, 0) if relu else a
    s = torch.from_numpy(a).view(-1, 2, 2, 512).permute(1, 2, 0, 3)
    x2 = _inputs("rnn2", lengths, 6)
    ref2, (rh2, rc2) = _f64("rnn2", x2, s[0], s[1])
    t2, (th2, tc2) = _torch_f32_cpu("rnn2", x2, s[0].float(), s[1].float(), torch.float32)
    y2, (fh2, fc2) = _net(1, split).rnn2([(x, v[i]) for i, x in enumerate(x2)], return_state=True)
    assert _err([y.cpu() for y in y2], ref2) <= K_F32 * _err([y.numpy() for y in t2], ref2) + 1e-7
    assert _err([fh2.cpu()], [rh2]) <= K_F32 * _err([th2.numpy()], [rh2]) + 1e-7
    assert _err([fc2.cpu()], [rc2]) <= K_F32 * _err([tc2.numpy()], [rc2]) + 1e-7


def _pieces(net, name, xs, ks):
    whole, (wh, wc) = net._subnet_forward(name, xs, return_state=True)
    for k in ks:
        keep = [i for i, x in enumerate(xs) if x.shape[0] > k]
        a, (h, c) = net._subnet_forward(name, [x[:k] for x in xs], return_state=True)
        b, (h2, c2) = net._subnet_forward(name, [xs[i][k:] for i in keep], (h[:, keep], c[:, keep]), return_state=True)
        for i, x in enumerate(xs):
            got = torch.cat([a[i], b[keep.index(i)]]) if i in keep else a[i]
            assert _same(got, whole[i]), (k, i)
        h[:, keep], c[:, keep] = h2, c2
        assert _same(h, wh) and _same(c, wc)


@pytest.mark.parametrize("split", [False, True])
def test_pieces_equal_the_whole(split):
    # 1 and 8 inside every sequence but the first, 33 / 50 past the end of some
    _pieces(_net(1, split), "rnn6", _inputs("rnn6", (1, 9, 33, 70), 7), (1, 8, 33, 50))


@pytest.mark.parametrize("split", [False, True])
def test_pieces_equal_the_whole_at_a_chunk_boundary(split):
    """rnn3 (linear1 K padded to 256, H = 512): a chunk holds 256 MiB / (4 B x (256 + 6 x 512)) = 20,160 rows. 160 sequences all
    running through step 129 put the first boundary after 126 steps (126 x 160 = 20,160); k = 140 is past the end of the short ones."""
    xs = _inputs("rnn3", [200] * 150 + [130] * 10, 12)
    net = _net(1, split)
    c0 = net.subnet_stats()[2]
    net._subnet_forward("rnn3", xs)
    assert net.subnet_stats()[2] - c0 == 2                      # steps 0..125 | 126..199
    _pieces(net, "rnn3", xs, (126, 140))


def test_chunked_many_sequences_and_a_long_one():
    name = "rnn4"
    net = _net(1, True)
    xs = _inputs(name, [512] * 1024, 8)
    ys = net._subnet_forward(name, xs)
    calls, frames, chunks, scratch = net.subnet_stats()
    assert chunks > 1 and scratch <= BUDGET + 64 * (1 << 20)        # + state of 1024 sequences and the row maps
    sample = [0, 511, 1023]
    ref, _ = _stepped(name, [xs[i][:40] for i in sample], True)
    for j, i in enumerate(sample):
        assert _same(ys[i][:40], ref[j])
    long = _inputs(name, (10000, 3, 700), 9)
    before = net.subnet_stats()
    y = net._subnet_forward(name, long)
    after = net.subnet_stats()
    assert after[2] - before[2] >= 2 and after[3] <= BUDGET + 64 * (1 << 20)
    ref, _ = _stepped(name, [long[0][:300], long[1], long[2][:300]], True)
    assert _same(y[0][:300], ref[0]) and _same(y[1], ref[1]) and _same(y[2][:300], ref[2])
    assert torch.isfinite(y[0]).all()


GOLD = os.path.join(os.path.dirname(__file__), "golden", "seq_threshold_edges.npz")


def _fixture_net(s, use_graph=False):
    net = Net(body=synth.make_body(1), batch=1)
    net.load_state_dict(_sd())
    net.use_flat_floor = bool(s["use_flat_floor"])
    net.use_reproj_opt = bool(s["use_reproj_opt"])
    net.use_vision_updater = bool(s["use_vision_updater"])
    net.use_imu_updater = bool(s["use_imu_updater"])
    net.gravityc = torch.from_numpy(s["gravityc"])
    net.use_graph = use_graph
    return net


def _pending_frame(s):
    """First frame k >= 8 after which a deferred vision-updater step is pending (fusion_state()[:, 4])."""
    net = _fixture_net(s)
    t = torch.from_numpy
    ft = t(s["first_tran"]) if s["first_tran"].size else None
    for i in range(s["j2dc"].shape[0]):
        net.forward_batch(t(s["j2dc"][i])[None], t(s["accc"][i])[None], t(s["oric"][i])[None], ft[None] if (ft is not None and i == 0) else None,
                          bool(s["first_frame"]) and i == 0)
        if i + 1 >= 8 and int(net.fusion_state()[0, 4]) == 1:
            return i + 1
    raise AssertionError("the fixture never leaves an updater step pending")


def _interrupt(net):
    """Sub-net calls with N != batch, large enough to grow the scratch, on every kind of entry point."""
    before = net.subnet_stats()[3]
    net.rnn6(_inputs("rnn6", [200] * 40, 10))
    net.rnn2([(torch.randn(5, 72), torch.randn(69)), (torch.randn(3, 72), torch.randn(69))])
    net.rnn4(_inputs("rnn4", (300, 7), 13), return_state=True)
    assert net.subnet_stats()[3] > before


def _state(net):
    return [net.get_state(n) for n, *_ in cfg.NETS], net.fusion_state(), net.get_trace()


def _same_state(a, b):
    for (h, c), (h2, c2) in zip(a[0], b[0]):
        assert _same(h, h2) and _same(c, c2)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_isolated_from_forward_sequence():
    s = np.load(GOLD)
    k = _pending_frame(s)
    t = torch.from_numpy
    ft = t(s["first_tran"])[None] if s["first_tran"].size else None
    seq = lambda a, lo, hi: t(a[lo:hi])[None]

    def run(interrupt):
        net = _fixture_net(s)
        p1, t1 = net.forward_sequence(seq(s["j2dc"], 0, k), seq(s["accc"], 0, k), seq(s["oric"], 0, k), ft, bool(s["first_frame"]))
        if interrupt:
            assert int(net.fusion_state()[0, 4]) == 1                  # the deferred updater step the call must not flush
            _interrupt(net)
        T = s["j2dc"].shape[0]
        p2, t2 = net.forward_sequence(seq(s["j2dc"], k, T), seq(s["accc"], k, T), seq(s["oric"], k, T))
        torch.cuda.synchronize()
        return torch.cat([p1, p2], 1).cpu(), torch.cat([t1, t2], 1).cpu(), _state(net)

    a, b = run(False), run(True)
    assert _same(a[0], b[0]) and _same(a[1], b[1])
    _same_state(a[2], b[2])


def test_isolated_from_the_live_path():
    s = np.load(GOLD)
    k = _pending_frame(s)
    t = torch.from_numpy
    ft = t(s["first_tran"]) if s["first_tran"].size else None

    def run(interrupt):
        net = _fixture_net(s, use_graph=True)
        out = []
        for i in range(s["j2dc"].shape[0]):
            if i == k and interrupt:
                assert int(net.fusion_state()[0, 4]) == 1
                _interrupt(net)
            out.append(net.forward_online(t(s["j2dc"][i]), t(s["accc"][i]), t(s["oric"][i]), ft if i == 0 else None,
                                          bool(s["first_frame"]) and i == 0))
            if i + 1 == k:
                net.fusion_state()                                     # (the same read in both runs)
        return torch.stack([p for p, _ in out]), torch.stack([q for _, q in out]), _state(net), net.live_stats()

    a, b = run(False), run(True)
    assert _same(a[0], b[0]) and _same(a[1], b[1])
    _same_state(a[2], b[2])
    assert a[3] == b[3]                                                # the same frames on the lean capture


def test_bad_input_raises_and_changes_nothing():
    net = _net(2)
    for name, nin, _, _ in cfg.NETS:                                   # a state that is not the initial one
        net.lstm_step(name, torch.randn(2, nin))
    x = _inputs("rnn4", (3,), 11)
    ref = net.rnn4(x)[0].cpu()
    before, stats = _state(net), net.subnet_stats()
    for bad in ([], [torch.zeros(0, 171)], [torch.zeros(3, 170)], torch.zeros(3, 171)):
        with pytest.raises(ValueError):
            net.rnn4(bad)
    with pytest.raises(ValueError):
        net.rnn4(x, (torch.zeros(2, 2, 1280), torch.zeros(2, 1, 1280)))
    with pytest.raises(ValueError):
        net.rnn4(x, torch.zeros(2, 1, 1280))
    with pytest.raises(ValueError):
        net.rnn2([(torch.zeros(3, 72), torch.zeros(68))])
    with pytest.raises(ValueError):
        net.rnn2.init_net(torch.zeros(2, 70))
    assert net.subnet_stats() == stats
    _same_state(before, _state(net))
    assert _same(net.rnn4(x)[0], ref)
