"""The float64 bound of the gate-GEMM precision tests has teeth (CPU only).

tests/test_gpu_gemm_precision.py holds every gate-GEMM kernel of rc_lstm_step to the bound of oracle/lstm_f64.py (`ratio`:
error / bound, <= 1 passes). Here the same bound is applied to CPU models of the arithmetic, over all six nets, batches 37 and
256 and five steps with a masked one:
  * torch fp32 (the oracle's f(i, x)) and a numpy emulation of the split-bf16 products as built (three truncated bf16 terms per
    operand; hi.hi, hi.mid, mid.hi, hi.lo, lo.hi and mid.mid; the fp32 rounding of the sum) stay at or below a third of it;
  * mutations a kernel could make without any bitwise self-comparison noticing -- mid.mid dropped, the low terms of one K half
    skipped, h(t - 1) read from the other layer -- reach three times it or more.
So a GPU kernel that lost one of those terms could not pass the GPU test.
"""
import copy

import numpy as np
import pytest
import torch

from oracle import lstm_f64 as R
from robustcap_amd import config as C, synth

NETS = [n for n, _, _, _ in C.NETS]
MARGIN = 3.0


@pytest.fixture(scope="module")
def sd():
    return synth.make_state_dict(0)


@pytest.fixture(scope="module", autouse=True)
def _blas_threads():
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:                                  # (numpy's BLAS then keeps its own thread count)
        yield
        return
    with threadpool_limits(limits=16):
        yield


# ------------------------------------------------------------------------------------------- emulated arithmetic
def trunc_bf16(a):
    """fp32 -> the bf16 of its top 16 bits (truncation, as the kernels' operand split), as fp32."""
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def split3(a):
    """a = hi + mid + lo, each a truncated bf16 (rc_gemm.hip: split3)."""
    a = np.asarray(a, dtype=np.float32)
    hi = trunc_bf16(a)
    r1 = a - hi
    mid = trunc_bf16(r1)
    return hi, mid, trunc_bf16(r1 - mid)


_WSPLIT = {}


def weight_planes(w):
    """float64 (hi + mid + lo, hi + mid, hi) of a weight matrix's split, cached for the net under test."""
    key = id(w)
    if key not in _WSPLIT:
        if len(_WSPLIT) > 8:
            _WSPLIT.clear()
        wh, wm, wl = (t.astype(np.float64) for t in split3(w))
        _WSPLIT[key] = (w, wh + wm + wl, wh + wm, wh)                    # (w: keeps id(w) unique while cached)
    return _WSPLIT[key][1:]


def split_gemm(a, w, products, low_k=None):
    """fp32(sum over k of the chosen partial products of a[:, k] and w[:, k]), the products and their sum exact (float64).
    products: "six" (as built), "five" (mid.mid dropped). low_k: a slice of k whose hi.lo and lo.hi terms are skipped."""
    ah, am, al = (t.astype(np.float64) for t in split3(a))
    w_hml, w_hm, w_h = weight_planes(w)

    def part(s, low):
        acc = ah[:, s] @ (w_hml if low else w_hm)[:, s].T                 # ah x (hi, mid[, lo])
        acc += am[:, s] @ (w_hm if products == "six" else w_h)[:, s].T     # am x (hi[, mid])
        return acc + al[:, s] @ w_h[:, s].T if low else acc               # al x hi
    K = a.shape[1]
    if low_k is None:
        acc = part(slice(0, K), True)
    else:
        rest = [s for s in (slice(0, low_k.start), slice(low_k.stop, K)) if s.stop > s.start]
        acc = part(low_k, False) + sum(part(s, True) for s in rest)
    return acc.astype(np.float32)


def _sig32(v):
    return (np.float32(1.0) / (np.float32(1.0) + np.exp(-v))).astype(np.float32)


class Emulated:
    """f(i, x) with every GEMM in split-bf16 products and everything else in fp32 (rc_gemm.hip / rc_gemm_lds.hip), or one
    of the mutations: "five" (mid.mid dropped), "klow" (the layer-input half of K without hi.lo / lo.hi), "hswap" (h(t - 1)
    of the other layer)."""

    def __init__(self, sd, name, batch, mutation=None):
        g = lambda k: np.asarray(sd[f"{name}.{k}"], np.float32)
        self.W1, self.b1, self.W2, self.b2 = g("linear1.weight"), g("linear1.bias"), g("linear2.weight"), g("linear2.bias")
        self.W = [np.concatenate([g(f"rnn.weight_ih_l{l}"), g(f"rnn.weight_hh_l{l}")], axis=1) for l in range(2)]
        self.b = [(g(f"rnn.bias_ih_l{l}") + g(f"rnn.bias_hh_l{l}")).astype(np.float32) for l in range(2)]
        H = self.W1.shape[0]
        self.h = np.zeros((2, batch, H), np.float32)
        self.c = np.zeros((2, batch, H), np.float32)
        self.mutation = mutation

    def gemm(self, a, w, layer_input_k=None):
        m = self.mutation
        return split_gemm(a, w, "five" if m == "five" else "six", layer_input_k if m == "klow" else None)

    def step(self, x, mask=None):
        B, H = self.h.shape[1], self.h.shape[2]
        sel = np.ones(B, bool) if mask is None else np.asarray(mask, bool)
        y = np.full((B, self.W2.shape[0]), np.nan, np.float32)
        a = np.maximum(self.gemm(np.asarray(x, np.float32)[sel], self.W1) + self.b1, np.float32(0.0))
        h_prev = self.h[::-1] if self.mutation == "hswap" else self.h
        hn = [None, None]
        for l in range(2):
            inp = np.concatenate([a, h_prev[l, sel]], axis=1)
            gates = self.gemm(inp, self.W[l], slice(0, H)) + self.b[l]
            i, f, gg, o = np.split(gates, 4, axis=1)
            c = (_sig32(f) * self.c[l, sel] + _sig32(i) * np.tanh(gg)).astype(np.float32)
            hn[l] = (_sig32(o) * np.tanh(c)).astype(np.float32)
            self.c[l, sel] = c
            a = hn[l]
        for l in range(2):
            self.h[l, sel] = hn[l]
        y[sel] = self.gemm(a, self.W2) + self.b2
        return y, self.h, self.c


class TorchFp32:
    """The oracle's f(i, x): torch.nn.Linear / LSTM in fp32 on the CPU (oracle/sig_mp_oracle.py: OracleRNN.step), on aten's own
    kernels: oneDNN's LSTM cell approximates its gate functions (c off by 4e-7 at the first step, twice aten's error)."""

    def __init__(self, sd, name, batch):
        from oracle import sig_mp_oracle as O
        nin, nh, nout = {n: (i, h, o) for n, i, h, o in C.NETS}[name]
        self.m = O.OracleRNN(nin, nh, nout)
        self.m.load_state_dict({k[len(name) + 1:]: torch.as_tensor(v) for k, v in sd.items()
                                if k.startswith(name + ".") and not k.startswith(name + ".init_net")})
        self.h = torch.zeros(2, batch, nh)
        self.c = torch.zeros(2, batch, nh)

    @torch.no_grad()
    def step(self, x, mask=None):
        with torch.backends.mkldnn.flags(enabled=False):
            return self._step(x, mask)

    def _step(self, x, mask):
        x = torch.as_tensor(np.asarray(x, np.float32))
        B = x.shape[0]
        y = torch.full((B, self.m.linear2.out_features), float("nan"))
        if mask is None:
            y = self.m.step(x, self.h, self.c)
        else:
            rows = torch.as_tensor(np.asarray(mask, bool)).nonzero().flatten()
            y[rows] = self.m.step(x[rows], self.h, self.c, rows)
        return y.numpy(), self.h.numpy(), self.c.numpy()


# ------------------------------------------------------------------------------------------------------- the runs
def schedule(name, B):
    """5 steps: two plain, one masked (rows 0, B - 1 and both sides of every tile edge below B), two plain."""
    nin = {n: i for n, i, _, _ in C.NETS}[name]
    mask = np.zeros(B, bool)
    mask[[r for r in (0, 15, 16, 31, 32, 63, 64, 127, 128, 255, B - 1) if r < B]] = True
    mask[1::3] = True
    return [(synth.normal(900 + s, 7, B * nin).reshape(B, nin), mask if s == 2 else None) for s in range(5)]


_REF = {}


def reference(sd, name, B):
    """The float64 trajectory of `schedule` with its bound after every step, computed once per case."""
    if (name, B) not in _REF:
        _REF.clear()
        p = R.params(sd, name)
        h, c = R.zero_state(p, B)
        out = []
        for x, mask in schedule(name, B):
            y, h, c, S = R.step(p, x, h, c, mask)
            bound = R.Bound(B) if not out else copy.deepcopy(out[-1][2])
            bound.update(S, c)
            out.append((x, mask, bound, y, h, c))
        _REF[(name, B)] = out
    return _REF[(name, B)]


def worst_ratio(sd, name, B, model):
    worst = 0.0
    for x, mask, bound, yr, hr, cr in reference(sd, name, B):
        y, h, c = model.step(x, mask)
        worst = max(worst, bound.ratio(y, h, c, yr, hr, cr, mask))
    return worst


CASES = [(n, B) for n in NETS for B in (37, 256)]


@pytest.mark.parametrize("name,B", CASES, ids=[f"{n}-B{B}" for n, B in CASES])
def test_bound_passes_fp32_and_the_built_products_and_rejects_mutations(sd, name, B):
    got = {"torch_fp32": worst_ratio(sd, name, B, TorchFp32(sd, name, B)),
           "six_products": worst_ratio(sd, name, B, Emulated(sd, name, B))}
    for m in ("five", "klow", "hswap"):
        got[m] = worst_ratio(sd, name, B, Emulated(sd, name, B, m))
    print(name, B, {k: round(v, 3) for k, v in got.items()})
    for k in ("torch_fp32", "six_products"):
        assert got[k] <= 1.0 / MARGIN, (name, B, k, got[k])
    for k in ("five", "klow", "hswap"):
        assert got[k] >= MARGIN, (name, B, k, got[k])


def test_split3_is_exact_and_truncating():
    a = synth.normal(3, 1, 4096) * np.float32(37.0)
    hi, mid, lo = split3(a)
    assert np.array_equal((hi.astype(np.float64) + mid + lo), a.astype(np.float64))
    assert np.all(np.abs(hi) <= np.abs(a)) and np.all(np.abs(mid) <= np.abs(a - hi))
    assert np.array_equal(trunc_bf16(hi), hi) and np.array_equal(trunc_bf16(mid), mid) and np.array_equal(trunc_bf16(lo), lo)


def test_oracle_matches_torch_lstm_in_float64(sd):
    """oracle/lstm_f64.step is torch.nn.LSTM (gate order, both biases, masked rows keep their state) -- checked in float64."""
    from oracle import sig_mp_oracle as O
    name, B = "rnn3", 9
    nin, nh, nout = {n: (i, h, o) for n, i, h, o in C.NETS}[name]
    m = O.OracleRNN(nin, nh, nout).double()
    m.load_state_dict({k[len(name) + 1:]: torch.as_tensor(v, dtype=torch.float64) for k, v in sd.items() if k.startswith(name + ".")})
    p = R.params(sd, name)
    h, c = R.zero_state(p, B)
    th, tc = torch.zeros(2, B, nh, dtype=torch.float64), torch.zeros(2, B, nh, dtype=torch.float64)
    mask = np.arange(B) % 2 == 0
    for s in range(3):
        x = synth.normal(40 + s, 2, B * nin).reshape(B, nin).astype(np.float64)
        msk = mask if s == 1 else None
        y, h, c, S = R.step(p, x, h, c, msk)
        with torch.no_grad():
            if msk is None:
                ty = m.step(torch.as_tensor(x), th, tc).numpy()
            else:
                rows = torch.as_tensor(msk).nonzero().flatten()
                ty = np.full_like(y, np.nan)
                ty[msk] = m.step(torch.as_tensor(x)[rows], th, tc, rows).numpy()
        np.testing.assert_allclose(y, ty, rtol=0, atol=1e-12)
        np.testing.assert_allclose(h, th.numpy(), rtol=0, atol=1e-12)
        np.testing.assert_allclose(c, tc.numpy(), rtol=0, atol=1e-12)
        assert np.all(S["y"][~np.isnan(y)] >= np.abs(y[~np.isnan(y)]) - 1e-12)
