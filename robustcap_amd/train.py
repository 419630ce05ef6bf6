"""Training of ONE sub-net on the device: ``tr = net.trainable("rnn4")`` -- the loop of the reference's
``articulate/utils/torch/train.py:117-122`` (``loss_fn(net(d), l)`` -> ``backward()`` -> ``clip_grad_norm_`` -> ``optimizer.step()``) over
an ``RNN`` / ``RNNWithInit`` module (``articulate/utils/torch/rnn.py:121-133``, ``:207-219``), on the arithmetic the sub-net is deployed
with.

    tr = net.trainable("rnn4")
    opt = torch.optim.SGD(tr.parameters(), lr=1e-2)
    ys = tr(xs)                                   # bitwise net.rnn4(xs)
    loss = torch.nn.functional.mse_loss(torch.cat(ys), target)
    opt.zero_grad(); loss.backward(); opt.step()  # the next tr(...) commits the stepped parameters first

What runs where. The forward is ``rc_subnet_forward_tape`` (HIP; the values of ``net.rnnK``). Of the backward, the reverse recurrence --
the only sequential part -- is ``rc_subnet_backward`` (HIP, one launch per step and layer on the transposed weights, in the context's gemm
mode); everything that is parallel over the frames is plain fp32 ``torch.matmul`` here: ``dH1 = dy @ W2``, the weight gradients
``dG^T @ input`` / ``dG^T @ h_prev`` as reductions over all frames (in up to 16 blocks of frames, ``frames_t_matmul``), the bias sums, the relu mask and ``dx = dP @ W1``.

Gradients are those of the EVAL-mode forward: the reference trains with dropout (0.4 after linear1, 0.1 between the LSTM layers); no
dropout mask exists here, in either direction.

``rnn2`` (RNNWithInit): the VALUES of the initial state are those of ``net.rnn2`` (``rc_init_net_forward`` on the packed weights); for
the GRADIENT ``init_net`` is evaluated a second time as three torch matmuls on the trainable parameters, and autograd carries
``d_init`` through that evaluation. The two evaluations differ by fp32 rounding, so the ``init_net`` gradients are exact derivatives of
a function that differs from the forward's by that rounding (a relu unit within rounding of zero may be masked differently).
"""
import ctypes as C
from collections import OrderedDict

import torch

from . import _lib
from . import config as cfg

_SPEC = {n: (i, h, o) for n, i, h, o in cfg.NETS}


def param_names(name):
    """The sub-net's keys of ``Net.state_dict()`` without the ``name.`` prefix, in its order (the order rc_update_subnet_weights takes)."""
    p = name + "."
    return [k[len(p):] for k, _ in cfg.state_dict_spec() if k.startswith(p)]


def shift_within_sequences(a, lengths, first):
    """h(t - 1) at every frame from h(t) at every frame: ``a`` [F, H] shifted by one frame within each sequence, with ``first`` [N, H]
    (None: zeros) at every sequence's first frame."""
    out = torch.empty_like(a)
    out[1:] = a[:-1]
    starts = torch.tensor([0] + list(lengths[:-1]), device=a.device).cumsum(0)
    if first is None:
        out[starts] = 0
    else:
        out[starts] = first
    return out


REDUCE_FRAMES = 256      # frames per partial sum of a weight gradient, at most REDUCE_PARTS partial sums
REDUCE_PARTS = 16


def frames_t_matmul(a, b):
    """a^T @ b over the frames: a [F, A], b [F, B] -> [A, B] -- every weight gradient is this reduction over all frames of the call.
    Plain fp32 matmuls, but over at most 16 blocks of frames whose partial sums are then added: one fp32 GEMM with K = F accumulates the
    frames in sequence, and over 2,820 frames that alone put dW_hh at 8.2-8.6 times torch fp32's error on the CPU (the same d_gates
    reduced in float64: 0.5-1.2 times; in 16 blocks: 1.1-1.8 times -- profiles/subnet_backward_ratios.txt)."""
    F = a.shape[0]
    nc = min(REDUCE_PARTS, -(-F // REDUCE_FRAMES))
    if nc <= 1:
        return a.t() @ b
    C = -(-F // nc)
    pad = nc * C - F
    if pad:
        a, b = torch.cat([a, a.new_zeros(pad, a.shape[1])]), torch.cat([b, b.new_zeros(pad, b.shape[1])])
    return torch.bmm(a.view(nc, C, -1).transpose(1, 2), b.view(nc, C, -1)).sum(0)


class _ValuesOf(torch.autograd.Function):
    """The values of ``values``; the gradient goes to ``graph`` (the same quantity, computed differentiably)."""

    @staticmethod
    def forward(ctx, graph, values):
        return values.clone()

    @staticmethod
    def backward(ctx, g):
        return g, None


class _SubnetFunction(torch.autograd.Function):
    """inputs: trainer, lengths, xcat [F, in], h0, c0 ([2, N, H] or None), then the twelve parameters of linear1, the LSTM and linear2 in ``param_names`` order."""

    @staticmethod
    def forward(ctx, tr, lengths, xcat, h0, c0, *params):
        net, name = tr._net, tr.name
        nin, H, nout = _SPEC[name]
        dev, N, F = net.device, len(lengths), sum(lengths)
        lens = (C.c_int32 * N)(*lengths)
        nfl = C.c_int64()
        _lib.check(net._ctx, net._lib.rc_subnet_tape_floats(net._ctx, name.encode(), N, lens, C.byref(nfl)), "rc_subnet_tape_floats")
        xcat = xcat.contiguous()
        y = torch.empty(F, nout, device=dev)
        fh, fc = torch.empty(2, N, H, device=dev), torch.empty(2, N, H, device=dev)
        acts, tape = torch.empty(3, F, H, device=dev), torch.empty(nfl.value, device=dev)
        rc = net._lib.rc_subnet_forward_tape(net._ctx, name.encode(), N, lens, _lib.ptr(xcat), _lib.ptr(y), _lib.ptr(h0), _lib.ptr(c0),
                                             _lib.ptr(fh), _lib.ptr(fc), _lib.ptr(acts), _lib.ptr(tape), _lib.stream_ptr())
        _lib.check(net._ctx, rc, "rc_subnet_forward_tape")
        ctx.tr, ctx.lengths, ctx.has_init = tr, lengths, h0 is not None
        ctx.save_for_backward(xcat, acts, tape, h0 if h0 is not None else xcat.new_empty(0), *params)
        return y, fh, fc

    @staticmethod
    def backward(ctx, dy, dfh, dfc):
        tr, lengths = ctx.tr, ctx.lengths
        net, name = tr._net, tr.name
        nin, H, nout = _SPEC[name]
        xcat, acts, tape, h0 = ctx.saved_tensors[:4]
        P = dict(zip(param_names(name), ctx.saved_tensors[4:]))
        dev, N, F = net.device, len(lengths), sum(lengths)
        dy, dfh, dfc = dy.contiguous(), dfh.contiguous(), dfc.contiguous()
        g = {}
        d_h1 = (dy @ P["linear2.weight"]).contiguous()
        g["linear2.weight"], g["linear2.bias"] = frames_t_matmul(dy, acts[2]), dy.sum(0)
        d_gates, d_a = torch.empty(2, F, 4 * H, device=dev), torch.empty(F, H, device=dev)
        d_ih = torch.empty(2, N, H, device=dev) if ctx.has_init else None
        d_ic = torch.empty(2, N, H, device=dev) if ctx.has_init else None
        lens = (C.c_int32 * N)(*lengths)
        rc = net._lib.rc_subnet_backward(net._ctx, name.encode(), N, lens, _lib.ptr(tape), _lib.ptr(d_h1), _lib.ptr(dfh), _lib.ptr(dfc),
                                         _lib.ptr(d_gates), _lib.ptr(d_a), _lib.ptr(d_ih), _lib.ptr(d_ic), _lib.stream_ptr())
        _lib.check(net._ctx, rc, "rc_subnet_backward")
        for l in (0, 1):
            dG = d_gates[l]
            h_prev = shift_within_sequences(acts[l + 1], lengths, h0[l] if ctx.has_init else None)
            g[f"rnn.weight_ih_l{l}"], g[f"rnn.weight_hh_l{l}"] = frames_t_matmul(dG, acts[l]), frames_t_matmul(dG, h_prev)
            g[f"rnn.bias_ih_l{l}"] = g[f"rnn.bias_hh_l{l}"] = dG.sum(0)
        dP = d_a * (acts[0] > 0)
        g["linear1.weight"], g["linear1.bias"] = frames_t_matmul(dP, xcat), dP.sum(0)
        dx = dP @ P["linear1.weight"]
        return (None, None, dx, d_ih, d_ic) + tuple(g[k] for k in param_names(name) if not k.startswith("init_net."))


class SubnetTrainer:
    """``net.trainable(name)``: the sub-net's parameters as ``torch.nn.Parameter`` s on the device (the reference module's names and
    shapes, initialised from the loaded weights) and a differentiable call with the arguments, checks and values of ``net.rnnK``.

    ``commit()`` writes the parameters into the context's packed device arrays in place (``rc_update_subnet_weights``); a call commits
    by itself when a parameter was modified since the last commit (its version counter moved: ``optimizer.step()``, ``p.add_()``,
    ``p.data.copy_()`` ...), so the forward never runs on stale packed weights. After a commit ``net.state_dict()`` and the module
    views return the committed values. The gradients are those of the eval-mode forward (no dropout); see the module docstring."""

    def __init__(self, net, name):
        if name not in _SPEC:
            raise ValueError(f"{name!r} is not a sub-net (rnn2 .. rnn8)")
        if not net.__dict__.get("_loaded"):
            raise _lib.RobustcapLibraryError("trainable(): load_state_dict first")
        self._net, self.name = net, name
        self._params = OrderedDict(
            (k, torch.nn.Parameter(torch.from_numpy(net._sd_cpu[f"{name}.{k}"]).to(net.device).clone())) for k in param_names(name))
        self._versions = self._current_versions()

    # ------------------------------------------------------------------------------------------------ parameters
    def named_parameters(self):
        return iter(self._params.items())

    def parameters(self):
        return iter(self._params.values())

    def zero_grad(self, set_to_none=True):
        for p in self._params.values():
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def _current_versions(self):
        return [p._version for p in self._params.values()]

    def commit(self):
        """Write the parameters into the context: every device array rc_finalize_weights derives from this sub-net's tensors is
        rewritten in place, ordered after all work of the context and before anything enqueued later."""
        net = self._net
        ts = [p.detach().contiguous() for p in self._params.values()]
        ptrs = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        rc = net._lib.rc_update_subnet_weights(net._ctx, self.name.encode(), ptrs, len(ts), _lib.stream_ptr())
        _lib.check(net._ctx, rc, "rc_update_subnet_weights")
        for k, t in zip(self._params, ts):                          # what net.state_dict() and the module views return
            net._sd_cpu[f"{self.name}.{k}"] = t.cpu().numpy()
        self._versions = self._current_versions()

    # ------------------------------------------------------------------------------------------------ the call
    def __call__(self, x, init=None, return_state=False):
        return self.forward(x, init, return_state)

    def forward(self, x, init=None, return_state=False):
        """``net.rnnK(x, init, return_state)`` -- the same arguments, checks (ValueError before anything is enqueued) and bits --
        differentiable with respect to the parameters, every ``x_i`` and ``init`` (``rnn2``: every ``x_i`` and ``x_init_i``)."""
        net, name = self._net, self.name
        P = self._params
        if name == "rnn2":
            xs, v = net._rnn2_check(x)
            xs, _, _ = net._subnet_check(name, xs, None)
        else:
            xs, h0, c0 = net._subnet_check(name, x, init)
        if self._current_versions() != self._versions:
            self.commit()
        if name == "rnn2":
            v = torch.stack([t.to(device=net.device, dtype=torch.float32).reshape(-1) for t in v])
            a = torch.relu(v @ P["init_net.0.weight"].t() + P["init_net.0.bias"])
            a = torch.relu(a @ P["init_net.2.weight"].t() + P["init_net.2.bias"])
            a = a @ P["init_net.4.weight"].t() + P["init_net.4.bias"]
            s = _ValuesOf.apply(a, net._init_net_forward(v.detach())).view(-1, 2, 2, 512).permute(1, 2, 0, 3)
            h0, c0 = s[0].contiguous(), s[1].contiguous()
        lengths = [int(t.shape[0]) for t in xs]
        xcat = torch.cat([t.to(device=net.device, dtype=torch.float32) for t in xs]).contiguous()
        core = [p for k, p in P.items() if not k.startswith("init_net.")]
        y, fh, fc = _SubnetFunction.apply(self, lengths, xcat, h0, c0, *core)
        outs = list(torch.split(y, lengths))
        return (outs, (fh, fc)) if return_state else outs
