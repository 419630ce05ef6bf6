"""Float64 numpy restatement of the sub-net's back-propagation as rc_subnet_backward and robustcap_amd/train.py split it (helper of
test_subnet_backward_cpu.py; no GPU, no library): the forward that records the tape, the transposed-pack getter, the per-unit reverse
recurrence over the PACKED gate order, and the assembly of the ten parameter gradients from d_gates, acts and d_a."""
import numpy as np


def orig(npk, H):
    """torch row of packed gate column n' (rc_finalize_weights): 16-column block cb = units 4 cb .. 4 cb + 3, each with its gates
    i, f, g, o in four consecutive columns."""
    npk = np.asarray(npk)
    return (npk % 4) * H + 4 * (npk // 16) + (npk % 16) // 4


def transposed_operand(w_ih, w_hh):
    """WT [2H, 4H]: WT[n', k'] = W[orig(k')][n'] over W = [W_ih | W_hh] -- the packed gate column is the contraction index. Columns
    (rows here) [0, H) serve dG . W_ih, [H, 2H) serve dG . W_hh."""
    H = w_ih.shape[1]
    W = np.concatenate([w_ih, w_hh], axis=1)                 # [4H, 2H]
    return W[orig(np.arange(4 * H), H)].T.copy()


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def forward_tape(p, xs, h0, c0):
    """p: dict of the sub-net's float64 tensors (reference names). Returns ys, (h_n, c_n), acts [3, F, H] in the caller's row order and
    the tape: per layer the gate activations [F, 4H] in PACKED column order (unit * 4 + gate... of the 16-column blocks) and c [F, H]."""
    H = p["linear1.weight"].shape[0]
    lengths = [x.shape[0] for x in xs]
    F, N = sum(lengths), len(xs)
    X = np.concatenate(xs)
    acts = np.zeros((3, F, H))
    acts[0] = np.maximum(X @ p["linear1.weight"].T + p["linear1.bias"], 0)
    gates, cs = np.zeros((2, F, 4 * H)), np.zeros((2, F, H))
    hn, cn = np.zeros((2, N, H)), np.zeros((2, N, H))
    cols = orig(np.arange(4 * H), H)
    for l in range(2):
        W = np.concatenate([p[f"rnn.weight_ih_l{l}"], p[f"rnn.weight_hh_l{l}"]], axis=1)[cols]      # packed columns as rows
        b = (p[f"rnn.bias_ih_l{l}"] + p[f"rnn.bias_hh_l{l}"])[cols]
        row = 0
        for i, T in enumerate(lengths):
            h, c = h0[l, i], c0[l, i]
            for t in range(T):
                pre = W @ np.concatenate([acts[l, row + t], h]) + b
                g4 = pre.reshape(-1, 4)                                                               # [unit, (i, f, g, o)]
                ig, fg, cg, og = _sig(g4[:, 0]), _sig(g4[:, 1]), np.tanh(g4[:, 2]), _sig(g4[:, 3])
                # packed column 16 cb + 4 u + g <-> unit 4 cb + u: the reshape above lists the units in order
                c = fg * c + ig * cg
                h = og * np.tanh(c)
                gates[l, row + t] = np.stack([ig, fg, cg, og], axis=1).reshape(-1)
                cs[l, row + t] = c
                acts[l + 1, row + t] = h
            hn[l, i], cn[l, i] = h, c
            row += T
    Y = acts[2] @ p["linear2.weight"].T + p["linear2.bias"]
    ys = np.split(Y, np.cumsum(lengths)[:-1])
    return ys, (hn, cn), acts, {"gates": gates, "c": cs, "init_c": np.asarray(c0, dtype=np.float64), "lengths": lengths}


def backward(p, tape, d_h1, d_final_h, d_final_c):
    """The reverse recurrence. Returns d_gates [2, F, 4H] (torch's column order g * H + u), d_a [F, H], d_init_h, d_init_c [2, N, H]."""
    lengths = tape["lengths"]
    F, N = sum(lengths), len(lengths)
    H = d_h1.shape[1]
    cols = orig(np.arange(4 * H), H)
    d_gates = np.zeros((2, F, 4 * H))
    d_init_h, d_init_c = np.zeros((2, N, H)), np.zeros((2, N, H))
    dh_above = d_h1
    for l in (1, 0):
        WT = transposed_operand(p[f"rnn.weight_ih_l{l}"], p[f"rnn.weight_hh_l{l}"])                 # [2H, 4H]
        dG = np.zeros((F, 4 * H))                                                                     # packed column order
        row = 0
        for i, T in enumerate(lengths):
            dh_rec, dc_next = d_final_h[l, i], d_final_c[l, i]                                      # the sequence enters at its last frame
            for t in range(T - 1, -1, -1):
                a = tape["gates"][l, row + t].reshape(-1, 4)
                ig, fg, cg, og = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
                c = tape["c"][l, row + t]
                c_prev = tape["c"][l, row + t - 1] if t > 0 else tape["init_c"][l, i]
                tc = np.tanh(c)
                dh = dh_rec + dh_above[row + t]
                do = dh * tc
                dc = dc_next + dh * og * (1 - tc * tc)
                di, dg, df, dc_next = dc * cg, dc * ig, dc * c_prev, dc * fg
                d4 = np.stack([di * ig * (1 - ig), df * fg * (1 - fg), dg * (1 - cg * cg), do * og * (1 - og)], axis=1).reshape(-1)
                dG[row + t] = d4
                dh_rec = WT[H:] @ d4                                                                  # dG(t) . W_hh
            d_init_h[l, i], d_init_c[l, i] = dh_rec, dc_next
            row += T
        d_gates[l][:, cols] = dG
        dh_above = dG @ WT[:H].T                                                                      # dG . W_ih, every frame at once
    return d_gates, dh_above, d_init_h, d_init_c


def shift(a, lengths, first):
    out = np.zeros_like(a)
    row = 0
    for i, T in enumerate(lengths):
        out[row] = first[i]
        out[row + 1:row + T] = a[row:row + T - 1]
        row += T
    return out


def assemble(p, xs, h0, acts, lengths, dy, d_gates, d_a):
    """The ten parameter gradients and dx, as robustcap_amd/train.py forms them."""
    X = np.concatenate(xs)
    g = {"linear2.weight": dy.T @ acts[2], "linear2.bias": dy.sum(0)}
    for l in range(2):
        dG = d_gates[l]
        g[f"rnn.weight_ih_l{l}"] = dG.T @ acts[l]
        g[f"rnn.weight_hh_l{l}"] = dG.T @ shift(acts[l + 1], lengths, h0[l])
        g[f"rnn.bias_ih_l{l}"] = g[f"rnn.bias_hh_l{l}"] = dG.sum(0)
    dP = d_a * (acts[0] > 0)
    g["linear1.weight"], g["linear1.bias"] = dP.T @ X, dP.sum(0)
    return g, dP @ p["linear1.weight"]
