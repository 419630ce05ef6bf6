"""float64 numpy restatement of one clipped Adam step as rc_subnet_optim_step specifies it (include/robustcap_hip.h):

    total_norm = sqrt(sum over the non-skipped gradients of g^2)
    coef       = min(1, max_norm / (total_norm + 1e-6))        (1 when max_norm <= 0)
    g' = coef g + weight_decay p;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2
    p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)

The kernel rounds total_norm to fp32 and forms coef in fp32 (clip_grad_norm_ on fp32 gradients does the same): ``coef_dtype=np.float32``,
the default, restates that; ``np.float64`` keeps the coefficient in double, which is what torch computes on float64 tensors and what
tests/test_subnet_optim_cpu.py pins this helper against. A gradient of None skips its tensor: no share of the norm, nothing updated.
"""
import numpy as np


def total_norm(grads):
    """float64 2-norm over every non-None gradient (squares of fp32 values are exact in double)."""
    return float(np.sqrt(sum(float(np.sum(np.square(np.asarray(g, dtype=np.float64)))) for g in grads if g is not None)))


def clip_coef(norm, max_norm, dtype=np.float32):
    """min(1, max_norm / (norm + 1e-6)) with norm rounded to ``dtype`` and every operation in ``dtype``; 1 when max_norm <= 0."""
    if max_norm <= 0:
        return dtype(1.0)
    c = dtype(max_norm) / (dtype(norm) + dtype(1e-6))
    return dtype(1.0) if c > dtype(1.0) else c


def adam_step(params, grads, exp_avg, exp_avg_sq, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=0.0,
              coef_dtype=np.float32):
    """Step number ``step`` (1 for the first). Lists of arrays in, new float64 lists out: (params, exp_avg, exp_avg_sq, total_norm, coef)."""
    norm = total_norm(grads)
    coef = float(clip_coef(norm, max_norm, coef_dtype))
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    P, M, V = [], [], []
    for p, g, m, v in zip(params, grads, exp_avg, exp_avg_sq):
        p, m, v = np.asarray(p, dtype=np.float64), np.asarray(m, dtype=np.float64), np.asarray(v, dtype=np.float64)
        if g is not None:
            g = coef * np.asarray(g, dtype=np.float64) + weight_decay * p
            m = b1 * m + (1.0 - b1) * g
            v = b2 * v + (1.0 - b2) * g * g
            p = p - (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
        P.append(p); M.append(m); V.append(v)
    return P, M, V, norm, coef
