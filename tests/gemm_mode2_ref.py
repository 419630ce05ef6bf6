"""numpy restatement of gemm mode 2 (rc_set_gemm_mode(ctx, 2)) -- a helper of tests/test_gemm_mode2_cpu.py and
tests/test_gpu_gemm_mode2.py, not collected by pytest. Written from the specification, not from the kernels:

  * an fp32 operand a becomes two bf16 terms: hi = RN_bf16(a) (round to nearest, ties to even, on the bit pattern) and
    mid = RN_bf16(a - hi); the subtraction is exact in fp32 and nothing below mid is kept;
  * a GEMM is the sum over k of a_mid.w_hi + a_hi.w_mid + a_hi.w_hi. Each product of two bf16 numbers is exact in fp32; here
    the products and their sum are formed in float64 (exact to 2^-53) and rounded to fp32 ONCE, so that what separates a
    kernel from `gemm3` is the order of its fp32 additions and nothing else.

`Emulated2` steps a sub-net like tests/test_gemm_bound_cpu.Emulated with every GEMM a `gemm3`, or one of the mutations a kernel
could make: "trunc" (terms by truncation), "no_midhi" (a_mid.w_hi dropped), "klow" (a_hi.w_mid dropped on the layer-input half of
K), "mid_from_a" (mid rounded from a instead of a - hi).
"""
import numpy as np

from test_gemm_bound_cpu import Emulated, reference, schedule, trunc_bf16, worst_ratio  # noqa: F401  (re-exported for the tests)

MUTATIONS = ("trunc", "no_midhi", "klow", "mid_from_a")


def rn_bf16(a):
    """fp32 -> the nearest bf16 (ties to even), as fp32: on the bit pattern u, (u + 0x7fff + bit 16 of u) with the low half
    cleared. A NaN stays a NaN (the one case the integer form would get wrong: a payload carried into the exponent)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(a), a, r).astype(np.float32)


def split2_rn(a):
    """(hi, mid) of the operand split, each a bf16 held as fp32."""
    a = np.asarray(a, dtype=np.float32)
    hi = rn_bf16(a)
    with np.errstate(invalid="ignore"):
        return hi, rn_bf16(a - hi)


def split2_mutated(a, mutation):
    a = np.asarray(a, dtype=np.float32)
    if mutation == "trunc":
        hi = trunc_bf16(a)
        return hi, trunc_bf16(a - hi)
    if mutation == "mid_from_a":
        return rn_bf16(a), rn_bf16(a)
    return split2_rn(a)


_WPLANES = {}
WPLANES_MAX = 12         # matrices whose float64 terms stay cached (a whole model, 27 matrices of 63 M weights, is 1 GB)


def _weight_terms(w, mutation):
    """float64 (hi, hi + mid) of a weight matrix's split, cached while the net under test lives."""
    key = (id(w), mutation if mutation in ("trunc", "mid_from_a") else None)
    if key not in _WPLANES:
        if len(_WPLANES) >= WPLANES_MAX:
            _WPLANES.clear()
        wh, wm = (t.astype(np.float64) for t in split2_mutated(w, key[1]))
        _WPLANES[key] = (w, wh, wh + wm)                                  # (w: keeps id(w) unique while cached)
    return _WPLANES[key][1:]


def gemm3(a, w, mutation=None, layer_input_k=None):
    """fp32(sum_k a_mid.w_hi + a_hi.w_mid + a_hi.w_hi) for a [M, K], w [N, K]: exact products, one rounding."""
    ah, am = (t.astype(np.float64) for t in split2_mutated(a, mutation))
    w_h, w_hm = _weight_terms(w, mutation)
    acc = ah @ w_hm.T                                                      # a_hi . (w_hi + w_mid)
    if mutation != "no_midhi":
        acc += am @ w_h.T                                                  # a_mid . w_hi
    if mutation == "klow" and layer_input_k is not None:
        s = layer_input_k
        acc -= ah[:, s] @ (w_hm - w_h)[:, s].T                             # a_hi . w_mid of that half of K, left out
    return acc.astype(np.float32)


class Emulated2(Emulated):
    """f(i, x) with every GEMM in mode 2's arithmetic and everything else in fp32, or one of MUTATIONS."""

    def __init__(self, sd, name, batch, mutation=None):
        assert mutation is None or mutation in MUTATIONS, mutation
        super().__init__(sd, name, batch, None)
        self.mutation2 = mutation

    def gemm(self, a, w, layer_input_k=None):
        return gemm3(a, w, self.mutation2, layer_input_k)


def scaled_ratio(bound, G, y, h, c, y64, h64, c64, mask=None):
    """error / (G x lstm_f64.Bound): every tolerance of the bound multiplied by the one factor G."""
    return bound.ratio(y, h, c, y64, h64, c64, mask) / G
