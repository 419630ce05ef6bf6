"""The yardstick of tests/test_gpu_subnet_forward.py: the float64 restatement of RNN.forward over ragged sequences (oracle/lstm_f64.step
looped with per-frame masks) equals torch's own packed-sequence construction in float64 (articulate/utils/torch/rnn.py:121-133,
RNNWithInit :207-219 with init_net's view / permute)."""
import numpy as np
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from oracle import lstm_f64
from robustcap_amd import config as cfg
from robustcap_amd import synth

SPEC = {n: (i, h, o) for n, i, h, o in cfg.NETS}


def _loop(sd, name, xs, h0, c0):
    p = lstm_f64.params(sd, name)
    h, c = h0.numpy().copy(), c0.numpy().copy()
    ys = [np.zeros((x.shape[0], SPEC[name][2])) for x in xs]
    for t in range(max(x.shape[0] for x in xs)):
        mask = np.array([x.shape[0] > t for x in xs])
        xt = np.stack([x[min(t, x.shape[0] - 1)].numpy() for x in xs])
        y, h, c, _ = lstm_f64.step(p, xt, h, c, mask)
        for i, x in enumerate(xs):
            if x.shape[0] > t:
                ys[i][t] = y[i]
    return ys, h, c


def _torch(sd, name, xs, h0, c0):
    nin, H, nout = SPEC[name]
    l1, l2, rnn = torch.nn.Linear(nin, H).double(), torch.nn.Linear(H, nout).double(), torch.nn.LSTM(H, H, 2).double()
    with torch.no_grad():
        for m, k in ((l1, "linear1"), (l2, "linear2")):
            m.weight.copy_(torch.from_numpy(sd[f"{name}.{k}.weight"])); m.bias.copy_(torch.from_numpy(sd[f"{name}.{k}.bias"]))
        for k, v in rnn.named_parameters():
            v.copy_(torch.from_numpy(sd[f"{name}.rnn.{k}"]))
        lengths = [x.shape[0] for x in xs]
        pad = torch.nn.utils.rnn.pad_sequence([torch.relu(l1(x)) for x in xs])
        out, (hn, cn) = rnn(pack_padded_sequence(pad, lengths, enforce_sorted=False), (h0, c0))
        out, _ = pad_packed_sequence(out)
        return [l2(out[:T, i]).numpy() for i, T in enumerate(lengths)], hn.numpy(), cn.numpy()


def test_restatement_equals_torch_ragged_with_init():
    sd = synth.make_state_dict(0)
    g = torch.Generator().manual_seed(0)
    for name, lengths in (("rnn3", (1, 5, 13, 2)), ("rnn8", (7, 3))):
        H = SPEC[name][1]
        xs = [torch.randn(T, SPEC[name][0], generator=g, dtype=torch.float64) for T in lengths]
        h0 = 0.5 * torch.randn(2, len(xs), H, generator=g, dtype=torch.float64)
        c0 = 0.5 * torch.randn(2, len(xs), H, generator=g, dtype=torch.float64)
        a, ah, ac = _loop(sd, name, xs, h0, c0)
        b, bh, bc = _torch(sd, name, xs, h0, c0)
        assert max(float(np.abs(u - v).max()) for u, v in zip(a, b)) < 1e-12
        assert float(np.abs(ah - bh).max()) < 1e-12 and float(np.abs(ac - bc).max()) < 1e-12


def test_restatement_equals_torch_rnn_with_init():
    sd = synth.make_state_dict(0)
    g = torch.Generator().manual_seed(1)
    lengths = (4, 1, 9)
    v = torch.randn(len(lengths), 69, generator=g, dtype=torch.float64)
    init_net = torch.nn.Sequential(torch.nn.Linear(69, 512), torch.nn.ReLU(), torch.nn.Linear(512, 1024), torch.nn.ReLU(),
                                   torch.nn.Linear(1024, 2048)).double()
    with torch.no_grad():
        for k, p in init_net.named_parameters():
            p.copy_(torch.from_numpy(sd[f"rnn2.init_net.{k}"]))
        s = init_net(v).view(-1, 2, 2, 512).permute(1, 2, 0, 3)       # rnn.py:216
    a = v.numpy()
    for q, relu in ((0, True), (2, True), (4, False)):               # the restatement the GPU test uses
        a = a @ sd[f"rnn2.init_net.{q}.weight"].astype(np.float64).T + sd[f"rnn2.init_net.{q}.bias"]
        a = np.maximum(a, 0) if relu else a
    s2 = torch.from_numpy(a).view(-1, 2, 2, 512).permute(1, 2, 0, 3)
    assert float((s - s2).abs().max()) < 1e-12
    xs = [torch.randn(T, 72, generator=g, dtype=torch.float64) for T in lengths]
    a, ah, _ = _loop(sd, "rnn2", xs, s2[0].contiguous(), s2[1].contiguous())
    b, bh, _ = _torch(sd, "rnn2", xs, s[0].contiguous(), s[1].contiguous())
    assert max(float(np.abs(u - w).max()) for u, w in zip(a, b)) < 1e-12 and float(np.abs(ah - bh).max()) < 1e-12
