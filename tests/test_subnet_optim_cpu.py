"""The float64 restatement of the fused optimiser step (tests/subnet_optim_f64.py) pinned against torch's own clip_grad_norm_ +
torch.optim.Adam in float64, and the optimiser object's state_dict layout exchanged with a real torch.optim.Adam (CPU: no GPU, no library
call -- robustcap_amd.train.AdamState is the code SubnetAdam saves and loads with)."""
import numpy as np
import pytest
import torch

import subnet_optim_f64 as F64
from robustcap_amd.train import AdamState

SHAPES = [(8, 5), (8,), (3, 8), (3,), (2,)]
RTOL = 1e-12


def _tensors(seed, scale):
    g = torch.Generator().manual_seed(seed)
    ps = [0.1 * torch.randn(s, generator=g, dtype=torch.float64) for s in SHAPES]
    gs = [scale * torch.randn(s, generator=g, dtype=torch.float64).float().double() for s in SHAPES]      # fp32 values, as downloaded gradients are
    return ps, gs


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert float(np.abs(a - b).max()) <= RTOL * max(float(np.abs(b).max()), 1e-300), what


# a clip that bites (norm ~ 30 > 1), one that does not (norm ~ 0.03 < 1), and weight decay with a biting clip
@pytest.mark.parametrize("scale,max_norm,wd,bites", [(3.0, 1.0, 0.0, True), (3e-3, 1.0, 0.0, False), (3.0, 1.0, 0.05, True)])
def test_helper_is_torch_float64_over_three_steps(scale, max_norm, wd, bites):
    ps, gs = _tensors(1, scale)
    hyper = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    tp = [torch.nn.Parameter(p.clone()) for p in ps]
    opt = torch.optim.Adam(tp, **hyper)
    P, M, V = [p.numpy() for p in ps], [np.zeros(s) for s in SHAPES], [np.zeros(s) for s in SHAPES]
    G = [g.numpy() for g in gs]
    for step in (1, 2, 3):
        for p, g in zip(tp, gs):
            p.grad = g.clone()                                                     # (clip_grad_norm_ scales the gradients in place)
        tn = torch.nn.utils.clip_grad_norm_(tp, max_norm)
        opt.step()
        P, M, V, norm, coef = F64.adam_step(P, G, M, V, step, max_norm=max_norm, coef_dtype=np.float64, **hyper)
        assert (norm > max_norm) == bites and (coef < 1.0) == bites
        _close(norm, float(tn), "norm")
        for i, p in enumerate(tp):
            _close(P[i], p.detach().numpy(), (step, i, "p"))
            _close(M[i], opt.state[p]["exp_avg"].numpy(), (step, i, "m"))
            _close(V[i], opt.state[p]["exp_avg_sq"].numpy(), (step, i, "v"))
    # the fp32 coefficient the kernel forms is the double one to fp32 rounding: norm, sum, quotient -- three roundings of 2^-24 each
    c32, c64 = float(F64.clip_coef(norm, max_norm, np.float32)), float(F64.clip_coef(norm, max_norm, np.float64))
    assert abs(c32 - c64) <= 3 * 2.0 ** -24 * c64
    assert F64.clip_coef(norm, 0.0) == 1.0 and F64.clip_coef(norm, -1.0) == 1.0


def test_a_skipped_tensor_is_left_out():
    ps, gs = _tensors(2, 3.0)
    G = [g.numpy() for g in gs]
    G[3] = None
    P0, Z = [p.numpy() for p in ps], [np.zeros(s) for s in SHAPES]
    P, M, V, norm, coef = F64.adam_step(P0, G, Z, Z, 1, lr=1e-2, max_norm=1.0)
    assert np.array_equal(P[3], P0[3]) and not M[3].any() and not V[3].any()
    _close(norm, np.sqrt(sum(float((g ** 2).sum()) for g in G if g is not None)), "norm")
    assert all(not np.array_equal(P[i], P0[i]) for i in (0, 1, 2, 4))


class _StandIn(AdamState):
    """The optimiser object on CPU tensors: AdamState's state code, the float64 helper as its step."""

    def step(self):
        self._ensure_moments()
        self.step_count += 1
        n = lambda ts: [t.detach().numpy() for t in ts]
        P, M, V, norm, _ = F64.adam_step(n(self._plist), [None if p.grad is None else p.grad.numpy() for p in self._plist], n(self.exp_avg),
                                         n(self.exp_avg_sq), self.step_count, lr=self.lr, betas=self.betas, eps=self.eps,
                                         weight_decay=self.weight_decay, max_norm=self.clip_grad_norm, coef_dtype=np.float64)
        with torch.no_grad():
            for dst, src in zip(self._plist + self.exp_avg + self.exp_avg_sq, P + M + V):
                dst.copy_(torch.from_numpy(src))
        return norm


def _pair(seed):
    ps, gs = _tensors(seed, 0.5)
    a, b = [torch.nn.Parameter(p.clone()) for p in ps], [torch.nn.Parameter(p.clone()) for p in ps]
    for p, q, g in zip(a, b, gs):
        p.grad, q.grad = g.clone(), g.clone()
    return a, b


def test_state_dict_layout_is_torch_adams_both_ways():
    hyper = dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.01)
    a, b = _pair(3)
    mine, theirs = _StandIn(a, **hyper), torch.optim.Adam(b)
    assert mine.state_dict()["state"] == {} and mine.state_dict()["param_groups"][0]["params"] == list(range(len(SHAPES)))
    mine.step(); mine.step()
    sd = mine.state_dict()
    assert sorted(sd["state"]) == list(range(len(SHAPES))) and sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
    with torch.no_grad():
        for p, q in zip(a, b):
            q.copy_(p)
    theirs.load_state_dict(sd)                                                     # a real Adam takes this object's state ...
    g = theirs.param_groups[0]
    assert (g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"], g["amsgrad"]) == (3e-3, (0.8, 0.99), 1e-7, 0.01, False)
    assert all(float(theirs.state[q]["step"]) == 2.0 for q in b)
    mine.step(); theirs.step()                                                     # ... and continues like it
    for i, (p, q) in enumerate(zip(a, b)):
        _close(p.detach().numpy(), q.detach().numpy(), (i, "p"))
        _close(mine.exp_avg_sq[i].numpy(), theirs.state[q]["exp_avg_sq"].numpy(), (i, "v"))
    # ... and back: a fresh object takes the real Adam's state (step as a tensor) and continues like it
    a2 = [torch.nn.Parameter(q.detach().clone()) for q in b]
    for p, q in zip(a2, b):
        p.grad = q.grad.clone()
    again = _StandIn(a2)
    again.load_state_dict(theirs.state_dict())
    assert again.step_count == 3 and again.lr == 3e-3 and again.betas == (0.8, 0.99) and again.weight_decay == 0.01
    again.step(); theirs.step()
    for i, (p, q) in enumerate(zip(a2, b)):
        _close(p.detach().numpy(), q.detach().numpy(), (i, "p"))
        _close(again.exp_avg[i].numpy(), theirs.state[q]["exp_avg"].numpy(), (i, "m"))


def test_load_accepts_an_int_step_and_refuses_what_it_cannot_keep():
    a, _ = _pair(4)
    src = _StandIn(a)
    src.step()
    sd = src.state_dict()
    for v in sd["state"].values():
        v["step"] = 7                                                              # an int, as older checkpoints carry it
    dst = _StandIn([torch.nn.Parameter(p.detach().clone()) for p in a])
    dst.load_state_dict(sd)
    assert dst.step_count == 7 and torch.equal(dst.exp_avg[0], src.exp_avg[0])
    sd["state"][1]["step"] = torch.tensor(8.0)
    with pytest.raises(ValueError):
        dst.load_state_dict(sd)                                                    # two step counts
    sd["state"][1]["step"] = 7
    sd["param_groups"][0]["amsgrad"] = True
    with pytest.raises(ValueError):
        dst.load_state_dict(sd)
    sd["param_groups"][0]["amsgrad"] = False
    sd["state"][2]["exp_avg"] = torch.zeros(4, 4)
    with pytest.raises(ValueError):
        dst.load_state_dict(sd)
    with pytest.raises(ValueError):
        _StandIn(a, betas=(1.0, 0.999))
