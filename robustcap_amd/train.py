"""Training of ONE sub-net on the device: ``tr = net.trainable("rnn4")`` -- the loop of the reference's
``articulate/utils/torch/train.py:117-122`` (``loss_fn(net(d), l)`` -> ``backward()`` -> ``clip_grad_norm_`` -> ``optimizer.step()``) over
an ``RNN`` / ``RNNWithInit`` module (``articulate/utils/torch/rnn.py:121-133``, ``:207-219``), on the arithmetic the sub-net is deployed
with.

    tr = net.trainable("rnn4")
    opt = torch.optim.SGD(tr.parameters(), lr=1e-2)
    ys = tr(xs)                                   # bitwise net.rnn4(xs)
    loss = torch.nn.functional.mse_loss(torch.cat(ys), target)
    opt.zero_grad(); loss.backward(); opt.step()  # the next tr(...) commits the stepped parameters first

or, with the second half of the iteration on the device too (``clip_grad_norm_`` + Adam + the repack in one pass, no commit):

    opt = tr.optimizer(lr=1e-3, clip_grad_norm=1.0)
    loss.backward(); norm = opt.step(); opt.zero_grad()

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


class AdamState:
    """The host half of an Adam optimiser over a fixed list of tensors: hyper-parameters, one step count, the two moments per tensor,
    and ``state_dict()`` / ``load_state_dict()`` in ``torch.optim.Adam``'s layout -- ``state[i] = {"step", "exp_avg", "exp_avg_sq"}`` with
    ``i`` in the order of ``params``, plus ``param_groups`` -- so a real ``torch.optim.Adam`` over same-shaped tensors loads what this
    object saves and this object loads what it saves (the reference's ``optimizer_states.pt``). Needs no GPU: the moments live where
    the parameters live.

    One step count for all tensors: torch counts per parameter, which differs only for a tensor that skipped a step (``grad is None``);
    a loaded state whose tensors carry different counts is refused."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_grad_norm=0.0):
        self._plist = list(params)
        self.lr = lr
        self._set_hyper(betas, eps, weight_decay)
        self.clip_grad_norm = float(clip_grad_norm)
        self.step_count = 0
        self.exp_avg = self.exp_avg_sq = None

    def _set_hyper(self, betas, eps, weight_decay):
        betas = (float(betas[0]), float(betas[1]))
        if not (float(self.lr) >= 0.0 and 0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0 and float(eps) >= 0.0 and float(weight_decay) >= 0.0):
            raise ValueError(f"invalid Adam hyper-parameters: lr {self.lr}, betas {betas}, eps {eps}, weight_decay {weight_decay}")
        self.betas, self.eps, self.weight_decay = betas, float(eps), float(weight_decay)

    def _ensure_moments(self):
        if self.exp_avg is None:
            self.exp_avg = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self._plist]
            self.exp_avg_sq = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self._plist]

    def bias_corrections(self):
        """(1 - beta1^t, 1 - beta2^t) of the current step count, in double."""
        return 1.0 - self.betas[0] ** self.step_count, 1.0 - self.betas[1] ** self.step_count

    def state_dict(self):
        state = {}
        if self.exp_avg is not None:
            for i in range(len(self._plist)):
                state[i] = {"step": torch.tensor(float(self.step_count)), "exp_avg": self.exp_avg[i].clone(),
                            "exp_avg_sq": self.exp_avg_sq[i].clone()}
        group = {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "params": list(range(len(self._plist)))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self._plist):
            raise ValueError(f"expected one parameter group of {len(self._plist)} tensors")
        g = groups[0]
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError("amsgrad / maximize states are not supported")
        index = {pid: i for i, pid in enumerate(g["params"])}           # (torch numbers the parameters in order; any ids map back)
        state = {index[k]: v for k, v in sd["state"].items()}
        steps = {int(float(v["step"])) for v in state.values()}         # an int, a float or a tensor
        if len(steps) > 1:
            raise ValueError(f"the tensors carry different step counts {sorted(steps)}: one count is kept for all")
        for i, v in state.items():
            for k in ("exp_avg", "exp_avg_sq"):
                if tuple(v[k].shape) != tuple(self._plist[i].shape):
                    raise ValueError(f"{k} of tensor {i} has shape {tuple(v[k].shape)}, expected {tuple(self._plist[i].shape)}")
        self.lr = g["lr"]
        self._set_hyper(g["betas"], g["eps"], g["weight_decay"])
        self.step_count = steps.pop() if steps else 0
        self.exp_avg = self.exp_avg_sq = None
        if state:
            self._ensure_moments()                                      # a tensor without an entry: zero moments
            for i, v in state.items():
                self.exp_avg[i].copy_(v["exp_avg"])
                self.exp_avg_sq[i].copy_(v["exp_avg_sq"])


class SubnetAdam(AdamState):
    """``tr.optimizer(...)``: ``clip_grad_norm_(tr.parameters(), clip_grad_norm)`` + ``torch.optim.Adam.step()`` + ``tr.commit()`` as ONE
    call, ``rc_subnet_optim_step``, enqueued on the current stream with no host synchronisation: the gradient norm, then per element of
    the packed weights the clipped Adam update in place and the repack. Unlike ``clip_grad_norm_`` the gradients are NOT modified: only
    the update sees the clipped values. A parameter whose ``grad`` is None is skipped like torch skips it (but the step count is one
    for all tensors, see ``AdamState``). The moments are device tensors, zeros from the first step on."""

    def __init__(self, tr, **hyper):
        super().__init__(tr.parameters(), **hyper)
        self._tr = tr
        self.last_norm_and_coef = None          # device [2] of the last step: total norm, clip coefficient

    def zero_grad(self, set_to_none=True):
        self._tr.zero_grad(set_to_none)

    def step(self):
        """One optimiser step. Returns the total gradient norm (before clipping) as a 0-d device tensor; nothing waits for the device."""
        tr = self._tr
        net = tr._net
        self._ensure_moments()
        ps = self._plist
        gs = [None if p.grad is None else p.grad.detach().to(dtype=torch.float32).contiguous() for p in ps]
        gs = [g.clone() if g is not None and g.data_ptr() % 16 else g for g in gs]      # (a view into a larger buffer: the kernels move 16-byte pieces)
        for p, g in zip(ps, gs):
            if not p.is_contiguous() or (g is not None and (g.shape != p.shape or g.device != p.device)):
                raise ValueError("parameters and gradients must be contiguous device tensors of the parameters' shapes")
        self.step_count += 1
        bc1, bc2 = self.bias_corrections()
        table = lambda ts: (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])
        out = torch.empty(2, device=net.device)
        rc = net._lib.rc_subnet_optim_step(net._ctx, tr.name.encode(), table([p.detach() for p in ps]), table(gs), table(self.exp_avg),
                                           table(self.exp_avg_sq), len(ps), float(self.lr), self.betas[0], self.betas[1], self.eps,
                                           self.weight_decay, bc1, bc2, self.clip_grad_norm, _lib.ptr(out), _lib.stream_ptr())
        if rc != 0:
            self.step_count -= 1
        _lib.check(net._ctx, rc, "rc_subnet_optim_step")
        for p in ps:                                                    # the parameters changed under torch: say so, then record that
            torch.autograd.graph.increment_version(p)                   # the packed weights already hold these versions (no commit)
        tr._versions = tr._current_versions()
        net._mark_host_copy_stale(tr)
        self.last_norm_and_coef = out
        return out[0]


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
        net._refresh_host_copy()
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
        net._stale_host_copy.pop(self.name, None)
        self._versions = self._current_versions()

    def optimizer(self, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip_grad_norm=0.0, **other):
        """Adam with gradient-norm clipping over this sub-net's parameters, stepped on the device in one call (``SubnetAdam``):
        ``step()``, ``zero_grad()``, a writable ``lr``, ``state_dict()`` / ``load_state_dict()`` in ``torch.optim.Adam``'s layout.
        ``clip_grad_norm <= 0``: no clipping. ``amsgrad`` or any other argument: ValueError."""
        if other:
            raise ValueError(f"unsupported optimiser arguments {sorted(other)} (Adam without amsgrad only)")
        return SubnetAdam(self, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, clip_grad_norm=clip_grad_norm)

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
