"""rc_subnet_weight_grads without a GPU: the entry is declared and bound, the trainer takes ``weight_grads``, and a numpy restatement
of the kernel's summation order over the frames shows why the order is what it is."""
import inspect
import re

import numpy as np
import pytest

from robustcap_amd import _lib
from robustcap_amd.net.sig_mp import Net
from robustcap_amd.train import WEIGHT_GRADS, SubnetTrainer


def test_the_entry_is_declared_and_bound():
    header = open(_lib.HEADER_PATH).read()
    m = re.search(r"^int\s+rc_subnet_weight_grads\s*\(([^)]*)\)", header, flags=re.M)
    assert m, "include/robustcap_hip.h does not declare rc_subnet_weight_grads"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 15 and args[0] == "rc_ctx* ctx" and args[-1] == "void* stream" and args[-2] == "void* const* outs_dev"
    assert "articulate/utils/torch/train.py:117-122" in header[:m.start()].rsplit("*/", 2)[-2]      # the lines it stands in for
    res, argtypes = _lib.SIGNATURES["rc_subnet_weight_grads"]
    assert len(argtypes) == len(args)
    assert "rc_set_subnet_wgrad_parts" in _lib.SIGNATURES and re.search(r"^int\s+rc_set_subnet_wgrad_parts\s*\(", header, flags=re.M)


def test_the_trainer_takes_weight_grads():
    for fn in (SubnetTrainer.__init__, Net.trainable):
        p = inspect.signature(fn).parameters["weight_grads"]
        assert p.default == "torch"
    assert WEIGHT_GRADS == ("torch", "device")
    tr = object.__new__(SubnetTrainer)                                 # the property alone: no device behind it
    for v in WEIGHT_GRADS:
        tr.weight_grads = v
        assert tr.weight_grads == v
    for bad in ("cuda", "", None, "Device"):
        with pytest.raises(ValueError):
            tr.weight_grads = bad
    assert tr.weight_grads == "device"


# ---- the order of the sum over frames ----------------------------------------------------------------------------------------------------
BLOCK, MAX_PARTS, MFMA_K = 256, 16, 4      # frames per first-level sum; parts at most; frames one v_mfma_f32_16x16x4_f32 adds at once


def _chain(a, b, acc=None):
    """One fp32 accumulator over the frames of a, b in steps of MFMA_K: the products of a step are taken as summed exactly (the
    instruction's own sum) and rounded once into the accumulator. Mode 0's granularity, the finer of the two modes (mode 1 adds 32)."""
    acc = np.zeros((a.shape[1], b.shape[1]), np.float32) if acc is None else acc
    for f in range(0, a.shape[0], MFMA_K):
        acc = (acc + (a[f:f + MFMA_K].astype(np.float64).T @ b[f:f + MFMA_K].astype(np.float64)).astype(np.float32)).astype(np.float32)
    return acc


def _two_level(a, b, parts, block_sum):
    """rc_wgrad.hip's order: whole BLOCK-frame blocks per part; a part adds its blocks' sums (block_sum) into a second fp32 accumulator
    in frame order; the parts' sums are added in index order."""
    F = a.shape[0]
    nblk = -(-F // BLOCK)
    parts = max(1, min(parts, MAX_PARTS, nblk))
    bpp = -(-nblk // parts)
    out = None
    for p in range(-(-nblk // bpp)):
        acc2 = np.zeros((a.shape[1], b.shape[1]), np.float32)
        for k in range(p * bpp, min(nblk, (p + 1) * bpp)):
            sl = slice(k * BLOCK, min(F, (k + 1) * BLOCK))
            acc2 = (acc2 + block_sum(a[sl], b[sl])).astype(np.float32)
        out = acc2 if out is None else (out + acc2).astype(np.float32)
    return out


@pytest.mark.parametrize("parts", [1, 2, 16])
def test_two_level_order_on_the_long_case(parts):
    """2,820 frames (12 x 235), the count at which one fp32 accumulator over all frames put dW_hh at 8.2 times torch fp32's error. The
    yardstick is the same blocked sum with every 256-frame block formed in float64 and rounded once ("float64-blocked": the error the
    fp32 hand-over between the levels costs by itself). The two-level fp32 order stays within twice that; one accumulator over all
    frames, same instruction granularity, does not."""
    rng = np.random.default_rng(0)
    F, A, B = 2820, 96, 80
    a, b = rng.standard_normal((F, A)).astype(np.float32), rng.standard_normal((F, B)).astype(np.float32)
    ref = a.astype(np.float64).T @ b.astype(np.float64)
    err = lambda x: float(np.abs(x.astype(np.float64) - ref).max())
    f64_blocked = err(_two_level(a, b, parts, lambda u, v: (u.astype(np.float64).T @ v.astype(np.float64)).astype(np.float32)))
    two_level = err(_two_level(a, b, parts, _chain))
    single = err(_chain(a, b))
    print(f"ORDER parts={parts}: float64-blocked {f64_blocked:.3e} two-level {two_level:.3e} ({two_level / f64_blocked:.2f}x) "
          f"single-level {single:.3e} ({single / f64_blocked:.2f}x)")
    assert two_level <= 2.0 * f64_blocked
    assert single > 2.0 * f64_blocked
