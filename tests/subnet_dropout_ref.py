"""The dropout of a trainable sub-net restated (helper of test_subnet_dropout_cpu.py and test_gpu_subnet_dropout.py; no library):
a numpy Philox4x32-10 with the mask rc_dropout.hip draws from it, and the train-mode forward of articulate/utils/torch/rnn.py:121-133
(``RNN.forward`` under ``net.train()``: Dropout(p) on relu(linear1), torch.nn.LSTM(dropout=p) on layer 0's output as layer 1's input)
in plain torch, any dtype, any device, differentiable by autograd, with the masks passed in."""
import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57          # Random123's multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # ... and key increments
U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two; returns the four output words as uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & U32 for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)             # 32 x 32 -> 64 bits, no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & U32, p1 >> np.uint64(32), p1 & U32
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def threshold(p):
    """T: a unit is kept iff its 32 bits are >= T. p as a C float."""
    return int(np.rint(np.float64(np.float32(p)) * 4294967296.0))


def scale(p):
    """s = (float)(1 / (1 - (double)p)): what a kept unit is multiplied by."""
    return np.float32(1.0 / (1.0 - np.float64(np.float32(p))))


def bits(rows, cols, site, seed, call):
    """The 32 bits behind every unit of a [rows, cols] matrix (cols % 4 == 0) whose row j is key row j: one Philox call per four
    consecutive units, counter (row, unit >> 2, site, call), key (seed low, seed high), output lane j -> unit 4 (unit >> 2) + j."""
    assert cols % 4 == 0
    r = np.arange(rows, dtype=np.uint64)[:, None]
    q = np.arange(cols // 4, dtype=np.uint64)[None, :]
    out = philox4x32_10((r, q, site, call), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(out, axis=-1).reshape(rows, cols)


def mask(rows, cols, site, p, seed, call):
    """bool [rows, cols]: True where the unit is kept."""
    return bits(rows, cols, site, seed, call) >= np.uint32(threshold(p)) if threshold(p) else np.ones((rows, cols), bool)


def scaled_mask(rows, cols, site, p, seed, call):
    """float32 [rows, cols]: s where kept, +0 where dropped -- rc_dropout_apply of ones."""
    return np.where(mask(rows, cols, site, p, seed, call), scale(p), np.float32(0.0)).astype(np.float32)


def _lstm_layer(x, lengths, w_ih, w_hh, b_ih, b_hh, h0, c0):
    """One LSTM layer over ragged sequences as a loop over time with matmul. x [F, in], sequence i at rows sum_{j<i} T_j; h0, c0 [N, H].
    Returns h at every frame [F, H] and the state of every sequence after its last frame."""
    N, Tmax = len(lengths), max(lengths)
    lens = np.asarray(lengths)
    starts = np.cumsum(lens) - lens
    index = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(x.device)
    xw = x @ w_ih.t() + (b_ih + b_hh)
    h, c = h0, c0
    rows, hs = [], []
    for t in range(Tmax):
        running = np.nonzero(lens > t)[0]
        act, row = index(running), index(starts[running] + t)
        g = xw[row] + h[act] @ w_hh.t()
        i, f, gg, o = g.chunk(4, dim=1)
        c_new = torch.sigmoid(f) * c[act] + torch.sigmoid(i) * torch.tanh(gg)
        h_new = torch.sigmoid(o) * torch.tanh(c_new)
        if len(running) == N:
            h, c = h_new, c_new
        else:
            h, c = h.index_copy(0, act, h_new), c.index_copy(0, act, c_new)
        rows.append(row)
        hs.append(h_new)
    hs = torch.cat(hs)
    return torch.zeros_like(hs).index_copy(0, torch.cat(rows), hs), h, c


def forward_train(P, xcat, lengths, h0, c0, m0, m1):
    """P: the sub-net's tensors by the reference's names (any dtype / device, the dtype of everything else); xcat [F, in]; h0, c0
    [2, N, H]; m0, m1: the scaled masks [F, H] of sites 0 and 1 (ones: the eval-mode forward). linear1, relu and the site-0 mask once,
    the two LSTM layers as loops over time with the site-1 mask between them, linear2 last. Returns y [F, out], h_n, c_n [2, N, H]."""
    a = torch.relu(xcat @ P["linear1.weight"].t() + P["linear1.bias"]) * m0
    hn, cn = [], []
    for l in (0, 1):
        a, h, c = _lstm_layer(a, lengths, P[f"rnn.weight_ih_l{l}"], P[f"rnn.weight_hh_l{l}"], P[f"rnn.bias_ih_l{l}"],
                              P[f"rnn.bias_hh_l{l}"], h0[l], c0[l])
        hn.append(h)
        cn.append(c)
        if l == 0:
            a = a * m1
    return a @ P["linear2.weight"].t() + P["linear2.bias"], torch.stack(hn), torch.stack(cn)
