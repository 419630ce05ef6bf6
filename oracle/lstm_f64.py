"""float64 reference of one sub-net step f(i, x) (net/sig_mp.py:126-129) with the magnitude scale of every GEMM.

One step = relu(linear1) -> two LSTM layers (torch.nn.LSTM: gate order i, f, g, o; bias_ih + bias_hh) -> linear2, in numpy
float64 from the reference state_dict. An optional row mask advances only the selected rows: the others keep h and c, and
their y is undefined (NaN here).

Next to every GEMM output the step returns its magnitude scale S = sum_k |w_k x_k| + |b| (both biases of a gate), per output
element. A sum of K fp32-rounded terms in any order is off by at most about K 2^-24 S, whatever cancels inside it; the bounds of
tests/test_gemm_bound_cpu.py and tests/test_gpu_gemm_precision.py are stated in S.
"""
import numpy as np

F64 = np.float64


def params(state_dict, name):
    """float64 weights of sub-net `name` ("rnn2".."rnn8") from a state_dict of arrays or tensors."""
    g = lambda k: np.asarray(state_dict[f"{name}.{k}"], dtype=F64)
    p = {"W1": g("linear1.weight"), "b1": g("linear1.bias"), "W2": g("linear2.weight"), "b2": g("linear2.bias")}
    for l in range(2):
        p[f"Wih{l}"] = g(f"rnn.weight_ih_l{l}")
        p[f"Whh{l}"] = g(f"rnn.weight_hh_l{l}")
        p[f"bl{l}"] = g(f"rnn.bias_ih_l{l}") + g(f"rnn.bias_hh_l{l}")
        p[f"bs{l}"] = np.abs(g(f"rnn.bias_ih_l{l}")) + np.abs(g(f"rnn.bias_hh_l{l}"))
    p["H"] = p["W1"].shape[0]
    return p


def zero_state(p, batch):
    """(h, c), each [2, batch, H] float64 zeros: the state of a fresh context."""
    return np.zeros((2, batch, p["H"])), np.zeros((2, batch, p["H"]))


def _sigmoid(v):
    return 0.5 * (1.0 + np.tanh(0.5 * v))


def lstm_cell(gates, c_prev):
    """(h, c) of one LSTM cell from its pre-activations [n, 4H] (i, f, g, o) and c_prev [n, H]."""
    i, f, g, o = np.split(gates, 4, axis=1)
    c = _sigmoid(f) * c_prev + _sigmoid(i) * np.tanh(g)
    return _sigmoid(o) * np.tanh(c), c


def step(p, x, h, c, mask=None):
    """One step on the state (h, c) [2, B, H]; x [B, in]. Returns (y [B, out], h', c', S) where S holds the scales
    "lin1" [B, H], "gates0" / "gates1" [B, 4H] and "y" [B, out]; rows outside `mask` (bool [B]) keep h, c, and their
    y and S are NaN. The inputs are not modified."""
    x = np.asarray(x, dtype=F64)
    B = x.shape[0]
    sel = np.ones(B, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    h, c = np.array(h, dtype=F64), np.array(c, dtype=F64)
    nan = lambda n: np.full((B, n), np.nan)
    y, S = nan(p["W2"].shape[0]), {"lin1": nan(p["H"]), "gates0": nan(4 * p["H"]), "gates1": nan(4 * p["H"]), "y": nan(p["W2"].shape[0])}
    if not sel.any():
        return y, h, c, S
    xs = x[sel]
    a = np.maximum(xs @ p["W1"].T + p["b1"], 0.0)
    S["lin1"][sel] = np.abs(xs) @ np.abs(p["W1"]).T + np.abs(p["b1"])
    for l in range(2):
        hp, cp = h[l, sel], c[l, sel]
        gates = a @ p[f"Wih{l}"].T + hp @ p[f"Whh{l}"].T + p[f"bl{l}"]
        S[f"gates{l}"][sel] = np.abs(a) @ np.abs(p[f"Wih{l}"]).T + np.abs(hp) @ np.abs(p[f"Whh{l}"]).T + p[f"bs{l}"]
        hn, cn = lstm_cell(gates, cp)
        h[l, sel], c[l, sel] = hn, cn
        a = hn
    y[sel] = a @ p["W2"].T + p["b2"]
    S["y"][sel] = np.abs(a) @ np.abs(p["W2"]).T + np.abs(p["b2"])
    return y, h, c, S


EPS32 = 2.0 ** -24       # unit roundoff of fp32
HC_ABS = 1.5e-6          # h and c: absolute error of a row whose gate scales are O(1) ...
HC_REL = 4.0             # ... and HC_REL 2^-24 S_gates of a row whose inputs are large (S_gates: largest gate scale so far) ...
HC_CELL = 4.0            # ... plus HC_CELL 2^-24 sum over its steps of |c| (the cell update's own rounding and gate functions are relative)
Y_REL, Y_ABS = 64.0, 1e-9   # y: Y_REL 2^-24 S_y + Y_ABS per element


class Bound:
    """The error bound of a computed step against `step`, for a trajectory of `batch` rows from the zero state:
        |h - h64|, |c - c64| <= max(HC_ABS, HC_REL 2^-24 Sg[row]) + HC_CELL 2^-24 Cs     every row (unselected ones keep their state)
        |y - y64|            <= Y_REL 2^-24 S_y + Y_ABS                                  the rows the step selected
    Sg[row] = the largest gate pre-activation scale of the row over both layers and every step so far (a row fed 1e3-sized
    inputs has gate sums of that order, whose fp32 rounding alone is ~2^-24 of it); Cs = the sum of |c| of the element over
    the steps that advanced it (saturated gates grow c by ~1 per step). `update` takes each step's S and c before `ratio`."""

    def __init__(self, batch):
        self.sg = np.zeros(batch)
        self.cs = 0.0

    def update(self, S, c=None):
        g = np.fmax(np.nanmax(np.where(np.isnan(S["gates0"]), -np.inf, S["gates0"]), axis=1),
                    np.nanmax(np.where(np.isnan(S["gates1"]), -np.inf, S["gates1"]), axis=1))
        self.sg = np.fmax(self.sg, g)
        self.sy = S["y"]
        if c is not None:
            sel = ~np.isnan(S["y"][:, 0])
            self.cs = self.cs + np.abs(c) * sel[None, :, None]

    def tol_hc(self):
        return np.maximum(HC_ABS, HC_REL * EPS32 * self.sg)[None, :, None] + HC_CELL * EPS32 * self.cs

    def tol_y(self):
        return Y_REL * EPS32 * self.sy + Y_ABS

    def parts(self, y, h, c, y64, h64, c64, mask=None):
        """(worst error / bound of h, of c, of y); inf where a computed value is not finite."""
        def r(got, ref, tol):
            got = np.asarray(got, dtype=F64)
            if not np.all(np.isfinite(got)):
                return np.inf
            return float(np.max(np.abs(got - ref) / tol)) if got.size else 0.0
        sel = np.ones(len(self.sg), bool) if mask is None else np.asarray(mask, bool)
        t = self.tol_hc()
        return r(h, h64, t), r(c, c64, t), r(np.asarray(y)[sel], y64[sel], self.tol_y()[sel])

    def ratio(self, y, h, c, y64, h64, c64, mask=None):
        """worst error / bound over h, c and y (<= 1: within the bound)."""
        return max(self.parts(y, h, c, y64, h64, c64, mask))
