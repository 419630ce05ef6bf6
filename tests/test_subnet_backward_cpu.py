"""The formulas of the sub-net's backward pass (rc_subnet_backward + robustcap_amd/train.py) in float64 numpy against torch's own
float64 autograd: the per-unit reverse recurrence over the packed gate order, the transposed-pack getter and the assembly of the ten
gradients. No GPU, no library."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(__file__))
import subnet_backward_f64 as B  # noqa: E402

from robustcap_amd import config as cfg  # noqa: E402
from robustcap_amd import synth  # noqa: E402

SPEC = {n: (i, h, o) for n, i, h, o in cfg.NETS}
NAME, LENGTHS = "rnn8", (3, 40, 17)


def _torch_f64(p, xs, h0, c0, ry, rh, rc):
    from torch.nn.utils.rnn import pack_sequence, pad_packed_sequence
    nin, H, nout = SPEC[NAME]
    l1, l2, rnn = torch.nn.Linear(nin, H).double(), torch.nn.Linear(H, nout).double(), torch.nn.LSTM(H, H, 2).double()
    with torch.no_grad():
        l1.weight.copy_(torch.from_numpy(p["linear1.weight"])); l1.bias.copy_(torch.from_numpy(p["linear1.bias"]))
        l2.weight.copy_(torch.from_numpy(p["linear2.weight"])); l2.bias.copy_(torch.from_numpy(p["linear2.bias"]))
        for k, v in rnn.named_parameters():
            v.copy_(torch.from_numpy(p[f"rnn.{k}"]))
    xs = [torch.from_numpy(x).requires_grad_() for x in xs]
    h0, c0 = torch.from_numpy(h0).requires_grad_(), torch.from_numpy(c0).requires_grad_()
    out, (hn, cn) = rnn(pack_sequence([torch.relu(l1(x)) for x in xs], enforce_sorted=False), (h0, c0))
    out, _ = pad_packed_sequence(out)
    ys = [l2(out[: x.shape[0], i]) for i, x in enumerate(xs)]
    loss = sum((y * torch.from_numpy(r)).sum() for y, r in zip(ys, ry)) + (hn * torch.from_numpy(rh)).sum() + (cn * torch.from_numpy(rc)).sum()
    loss.backward()
    g = {"linear1.weight": l1.weight.grad, "linear1.bias": l1.bias.grad, "linear2.weight": l2.weight.grad, "linear2.bias": l2.bias.grad}
    g.update({f"rnn.{k}": v.grad for k, v in rnn.named_parameters()})
    return ([y.detach().numpy() for y in ys], hn.detach().numpy(), cn.detach().numpy(), {k: v.numpy() for k, v in g.items()},
            [x.grad.numpy() for x in xs], h0.grad.numpy(), c0.grad.numpy())


def test_the_transposed_operand_is_the_packed_matrix_transposed():
    H = 32
    rng = np.random.default_rng(0)
    wi, wh = rng.standard_normal((4 * H, H)), rng.standard_normal((4 * H, H))
    WT = B.transposed_operand(wi, wh)
    assert WT.shape == (2 * H, 4 * H)
    cols = B.orig(np.arange(4 * H), H)
    assert sorted(cols.tolist()) == list(range(4 * H))                       # a permutation
    assert cols[0] == 0 and cols[1] == H and cols[2] == 2 * H and cols[3] == 3 * H and cols[4] == 1 and cols[16] == 4
    dG_torch = rng.standard_normal((5, 4 * H))                               # torch's column order
    dG_packed = dG_torch[:, cols]
    assert np.allclose(dG_packed @ WT[:H].T, dG_torch @ wi, rtol=0, atol=1e-12)
    assert np.allclose(dG_packed @ WT[H:].T, dG_torch @ wh, rtol=0, atol=1e-12)


def test_equals_torch_float64_autograd():
    nin, H, nout = SPEC[NAME]
    sd = synth.make_state_dict(0)
    p = {k[len(NAME) + 1:]: np.asarray(v, dtype=np.float64) for k, v in sd.items() if k.startswith(NAME + ".")}
    g = torch.Generator().manual_seed(21)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).numpy()
    xs = [rn(T, nin) for T in LENGTHS]
    N = len(xs)
    h0, c0 = 0.5 * rn(2, N, H), 0.5 * rn(2, N, H)
    ry, rh, rc = [rn(T, nout) for T in LENGTHS], rn(2, N, H), rn(2, N, H)
    ys_t, hn_t, cn_t, g_t, dx_t, dh0_t, dc0_t = _torch_f64(p, xs, h0, c0, ry, rh, rc)

    ys, (hn, cn), acts, tape = B.forward_tape(p, xs, h0, c0)
    dy = np.concatenate(ry)
    d_gates, d_a, d_ih, d_ic = B.backward(p, tape, dy @ p["linear2.weight"], rh, rc)
    grads, dx = B.assemble(p, xs, h0, acts, list(LENGTHS), dy, d_gates, d_a)

    def close(a, b, what):
        scale = np.abs(b).max()
        assert scale > 0 and np.abs(a - b).max() <= 1e-11 * scale, (what, np.abs(a - b).max(), scale)

    close(np.concatenate(ys), np.concatenate(ys_t), "y")
    close(hn, hn_t, "h_n"); close(cn, cn_t, "c_n")
    assert sorted(grads) == sorted(g_t) and len(grads) == 12                 # ten gradients, the bias pairs counted once each way
    for k in g_t:
        close(grads[k], g_t[k], k)
    close(dx, np.concatenate(dx_t), "dx")
    close(d_ih, dh0_t, "d init_h"); close(d_ic, dc0_t, "d init_c")
