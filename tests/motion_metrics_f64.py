"""float64 restatement of art.FullMotionEvaluator (articulate/evaluator.py:365-394), its float32 transcription, bound, cases and
mutations -- TEST INFRASTRUCTURE, NOT PRODUCT.

`evaluate(..., dtype=F64)` is the restatement: its own forward kinematics and skinning on the body arrays (articulate/model.py:229-241
written out), the atan2 angle of oracle/pose_ops_f64.py, and lines 365-394 in torch, so that the mean of an empty set and the std of
one sample are what torch returns. `evaluate(..., dtype=F32)` is the same text in float32: the transcription of the reference, which
*is* a float32 torch computation. `evaluate_groups` cuts a concatenated batch into its motions first.

The bound of every compared entry (the project's K = 8 convention):
    Bound = K |float32 transcription - float64 restatement| + 1e-7 scale,
scale = the size of the numbers the entry is made of, taken from the restatement's inputs, never from the code under test:
    position rows (je, ve, masked je, tre)   max |x_p| + max |x_t| over the joints (ve: vertices) of both motions, plus max |offset|
    angle rows                              180 / pi max(1, largest angle in radians)   (oracle/pose_ops_f64.py: A = max(1, theta))
    jerk rows                               8 fps^3 max |x|: the stencil's coefficients sum to 8 in magnitude
    te                                      4 max |x_0|: four root positions are added
A NaN must sit exactly where the restatement has one.

`mut` names one deliberate mistake each (tests/test_motion_metrics_cpu.py: each moves a named output by more than the bound).

`evaluate_blockwise` forms the same eleven rows the way the device has to: per-block (n, mean, M2) of 32 rows merged in index order by
Chan's update (`blockwise`), in float64 numpy, sharing no code with the kernel. It equals `evaluate(dtype=F64)` up to the order of the
sums; BLOCK_MUTATIONS are the mistakes of that path, which need a third block or a one-second window that leaves its block to show.
"""
import math

import numpy as np
import torch

from oracle import pose_ops_f64 as P

F32, F64 = torch.float32, torch.float64
K = 8.0
REL = 1e-7
ROWS = ("je", "ve", "lae", "gae", "jkp", "jkt", "te", "mje", "mlae", "mgae", "tre")
MUTATIONS = {                       # mutation -> (row, column of out) it must move
    "biased_std": ("je", 1),
    "std_all_elements": ("je", 1),
    "window_plus_1": ("te", 0),
    "window_minus_1": ("te", 0),
    "offset_sign": ("je", 0),
    "ve_no_offset": ("ve", 0),
    "jerk_no_tran": ("jkp", 0),
}
GROUP_MUTATION = ("stencil_crosses_groups", ("jkp", 0))


def _t(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.float32))).to(dtype)


def fk(body, pose, tran, dtype):
    """articulate/model.py:229-241: (global rotations [n,24,3,3], joints [n,24,3], vertices [n,V,3]), translation added to both"""
    pose = _t(pose, dtype).reshape(-1, 24, 3, 3)
    n = pose.shape[0]
    J = _t(body["J"], dtype)
    j = J - J[:1]
    x = _t(body["v_template"], dtype) - J[:1]
    w = _t(body["weights"], dtype)
    parent = [int(p) for p in body["parent"]]
    G, Pj = [pose[:, 0]], [torch.zeros(n, 3, dtype=dtype)]
    for i in range(1, 24):
        p = parent[i]
        G.append(G[p] @ pose[:, i])
        Pj.append(Pj[p] + (G[p] @ (j[i] - j[p]).view(1, 3, 1)).squeeze(-1))
    G, Pj = torch.stack(G, dim=1), torch.stack(Pj, dim=1)
    T = Pj - (G @ j.view(1, 24, 3, 1)).squeeze(-1)
    A = torch.cat((G, T.unsqueeze(-1)), dim=-1)                                   # [n,24,3,4]
    Tv = torch.tensordot(A, w, dims=([1], [1])).permute(0, 3, 1, 2)               # [n,V,3,4]
    v = (Tv[..., :3] @ x.view(1, -1, 3, 1)).squeeze(-1) + Tv[..., 3]
    tr = torch.zeros(n, 1, 3, dtype=dtype) if tran is None else _t(tran, dtype).view(n, 1, 3)
    return G, Pj + tr, v + tr


def _angle_deg(Ra, Rb, dtype):
    n = Ra.shape[0]
    return (P.Ops(P.Ar(dtype)).angle(Ra.reshape(-1, 3, 3), Rb.reshape(-1, 3, 3)) * 180.0 / math.pi).view(n, 24)


def arrays(body, pose_p, pose_t, tran_p=None, tran_t=None, fps=60, align=0, dtype=F64, mut=None):
    """evaluator.py:365-379: the [rows, columns] arrays and the scale of each row of the result"""
    f = fps + (1 if mut == "window_plus_1" else (-1 if mut == "window_minus_1" else 0))
    lp, lt = _t(pose_p, dtype).reshape(-1, 24, 3, 3), _t(pose_t, dtype).reshape(-1, 24, 3, 3)
    gp, jp, vp = fk(body, pose_p, tran_p, dtype)
    gt, jt, vt = fk(body, pose_t, tran_t, dtype)
    off = (jt[:, align] - jp[:, align]).unsqueeze(1)
    if mut == "offset_sign":
        off = -off
    a = {"tre": (jp - jt).norm(dim=2),
         "ve": ((vp - vt) if mut == "ve_no_offset" else (vp + off - vt)).norm(dim=2),
         "je": (jp + off - jt).norm(dim=2),
         "lae": _angle_deg(lp, lt, dtype), "gae": _angle_deg(gp, gt, dtype)}
    kp, kt = jp, jt
    if mut == "jerk_no_tran":
        kp = jp if tran_p is None else jp - _t(tran_p, dtype).view(-1, 1, 3)
        kt = jt if tran_t is None else jt - _t(tran_t, dtype).view(-1, 1, 3)
    a["jkp"] = ((kp[3:] - 3 * kp[2:-1] + 3 * kp[1:-2] - kp[:-3]) * (fps ** 3)).norm(dim=2)
    a["jkt"] = ((kt[3:] - 3 * kt[2:-1] + 3 * kt[1:-2] - kt[:-3]) * (fps ** 3)).norm(dim=2)
    a["te"] = ((jp[f:, :1] - jp[:-f, :1]) - (jt[f:, :1] - jt[:-f, :1])).norm(dim=2)
    if mut == "window_wraps_block":                                               # the same N - fps rows, read fps % 32 frames ahead
        rows, w = max(jp.shape[0] - f, 0), f % 32
        a["te"] = ((jp[w:w + rows, :1] - jp[:rows, :1]) - (jt[w:w + rows, :1] - jt[:rows, :1])).norm(dim=2)
    mx = lambda z: float(z.double().norm(dim=-1).max())
    pos = mx(jp) + mx(jt) + mx(off)
    ang = lambda z: 180.0 / math.pi * max(1.0, float(z.double().max()) * math.pi / 180.0)
    scale = {"je": pos, "mje": pos, "tre": pos, "ve": mx(vp) + mx(vt) + mx(off), "lae": ang(a["lae"]), "mlae": ang(a["lae"]),
             "gae": ang(a["gae"]), "mgae": ang(a["gae"]), "jkp": 8.0 * fps ** 3 * mx(jp), "jkt": 8.0 * fps ** 3 * mx(jt),
             "te": 4.0 * max(mx(jp[:, :1]), mx(jt[:, :1]))}
    return a, np.array([scale[r] for r in ROWS])


def _pair(x, mut=None):
    """(x.mean(), x.std(dim=0).mean()) of evaluator.py:384-394"""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                           # std of one sample / of nothing: NaN, as in the reference
        if mut == "biased_std":
            s = x.std(dim=0, unbiased=False).mean()
        elif mut == "std_all_elements":
            s = x.std()
        else:
            s = x.std(dim=0).mean()
        return [float(x.mean()), float(s)]


def evaluate(body, pose_p, pose_t, tran_p=None, tran_t=None, fps=60, align=0, mask=None, dtype=F64, mut=None):
    """-> (out [11,2], per_joint [4,24] = column means of je, lae, gae, tre, scale [11]) as float64 numpy arrays"""
    a, scale = arrays(body, pose_p, pose_t, tran_p, tran_t, fps, align, dtype, mut)
    for src, dst in (("je", "mje"), ("lae", "mlae"), ("gae", "mgae")):
        a[dst] = a[src][:, list(mask)] if mask is not None else torch.zeros(1, dtype=dtype)      # evaluator.py:380-382
    out = np.array([_pair(a[r], mut) for r in ROWS], np.float64)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pj = torch.stack([a[r].mean(dim=0) for r in ("je", "lae", "gae", "tre")]).double().numpy()
    return out, pj, scale


def evaluate_groups(body, pose_p, pose_t, tran_p, tran_t, sizes, fps=60, align=0, mask=None, dtype=F64, mut=None):
    """every motion of a concatenated batch on its own: ([G,11,2], [G,4,24], [G,11]). mut == 'stencil_crosses_groups': the jerk rows of a
    group that is not the last are those of its frames followed by the next group's first three"""
    outs, pjs, scs, at = [], [], [], 0
    cut = lambda z, lo, hi: None if z is None else np.asarray(z)[lo:hi]
    n = np.asarray(pose_p).shape[0]
    for N in sizes:
        o, pj, sc = evaluate(body, cut(pose_p, at, at + N), cut(pose_t, at, at + N), cut(tran_p, at, at + N), cut(tran_t, at, at + N), fps,
                             align, mask, dtype)
        if mut == "stencil_crosses_groups" and at + N < n:
            hi = min(at + N + 3, n)
            o2 = evaluate(body, cut(pose_p, at, hi), cut(pose_t, at, hi), cut(tran_p, at, hi), cut(tran_t, at, hi), fps, align, mask, dtype)[0]
            o[4:6] = o2[4:6]
        outs.append(o), pjs.append(pj), scs.append(sc)
        at += N
    return np.stack(outs), np.stack(pjs), np.stack(scs)


# ------------------------------------------------------------------------------------------- the same numbers, block by block
BLOCK_MUTATIONS = {                 # mutation of the block-wise path -> (row, column of out) it must move
    "count_not_carried": ("je", 1),
    "no_cross_term": ("je", 1),
    "unweighted_block_means": ("je", 0),
    "window_wraps_block": ("te", 0),
    "jerk_rows_from_frames": ("jkp", 0),
}


def _blockwise_columns(x, fg, mut):
    """per column (mean, unbiased std) of x [rows, cols]: (n, mean, M2) of every block of fg rows, merged in index order by Chan's update
      n = na + nb,  mean = mean_a + (mean_b - mean_a) nb / n,  M2 = M2_a + M2_b + (mean_b - mean_a)^2 na nb / n.
    No rows: (NaN, NaN); one row: (its value, NaN = 0 / 0), as torch's mean and std(dim=0) give them."""
    x = np.asarray(x, np.float64)
    rows, cols = x.shape
    nan = np.full(cols, np.nan)
    if rows == 0:
        return nan, nan.copy()
    na, mean, m2, prev, block_means = 0, None, None, 0, []
    for lo in range(0, rows, fg):
        blk = x[lo:lo + fg]
        nb, mb = blk.shape[0], blk.mean(axis=0)
        m2b = ((blk - mb) ** 2).sum(axis=0)
        block_means.append(mb)
        if na == 0:
            na, mean, m2 = nb, mb, m2b
        else:
            ca = prev if mut == "count_not_carried" else na       # the mistake: the count of the block before, not of all before
            d = mb - mean
            mean = mean + d * (nb / (ca + nb))
            m2 = m2 + m2b + (0.0 if mut == "no_cross_term" else d * d * (ca * nb / (ca + nb)))
            na += nb
        prev = nb
    if mut == "unweighted_block_means":
        mean = np.mean(block_means, axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        std = np.sqrt(m2 / (rows - 1.0))
    return mean, std


def blockwise(x, fg=32, mut=None):
    """(x.mean(), x.std(dim=0).mean()) of an [rows, cols] float64 array with equal rows per column, formed from per-block (n, mean, M2)
    merged in index order: the mean of the column means and the mean of the unbiased column stds"""
    m, s = _blockwise_columns(x, fg, mut)
    return [float(m.mean()), float(s.mean())]


def evaluate_blockwise(body, pose_p, pose_t, tran_p=None, tran_t=None, fps=60, align=0, mask=None, fg=32, mut=None):
    """evaluate(dtype=F64) with every (mean, std) pair formed by `blockwise`: (out [11,2], per_joint [4,24], scale [11]). It differs from
    evaluate by the order of the sums alone; `mut` names one of BLOCK_MUTATIONS."""
    a, scale = arrays(body, pose_p, pose_t, tran_p, tran_t, fps, align, F64, mut if mut == "window_wraps_block" else None)
    a = {k: v.numpy() for k, v in a.items()}
    for src, dst in (("je", "mje"), ("lae", "mlae"), ("gae", "mgae")):
        a[dst] = a[src][:, list(mask)] if mask is not None else np.zeros((1, 1))
    if mut == "jerk_rows_from_frames":                                            # N rows in place of N - 3: the last valid row read again
        for r in ("jkp", "jkt"):
            if a[r].shape[0] > 0:
                a[r] = np.concatenate([a[r], np.repeat(a[r][-1:], 3, axis=0)])
    out = np.array([blockwise(a[r], fg, mut) for r in ROWS], np.float64)
    pj = np.stack([_blockwise_columns(a[r], fg, mut)[0] for r in ("je", "lae", "gae", "tre")])
    return out, pj, scale


def bound(f32, f64, scale):
    """K |float32 - float64| + 1e-7 scale; scale [..., 11] broadcasts over the two columns of out"""
    with np.errstate(invalid="ignore"):
        e32 = np.abs(np.asarray(f32, np.float64) - np.asarray(f64, np.float64))
    return K * np.where(np.isnan(e32), 0.0, e32) + REL * np.asarray(scale, np.float64)[..., None]


def ratios(got, f64, bnd):
    """|got - f64| / Bound per entry (0 where both are NaN); raises where the NaNs differ"""
    got, f64 = np.asarray(got, np.float64), np.asarray(f64, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(f64)), ("NaN placement", got, f64)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - f64)
        r = err / bnd
    return np.where(np.isnan(f64) | (err == 0.0), 0.0, r)                 # 0 / 0 = 0: an exact entry under a zero Bound


def per_joint_scale(scale):
    """scale [..., 11] -> [..., 4] for the per-joint rows je, lae, gae, tre"""
    s = np.asarray(scale)
    return np.stack([s[..., 0], s[..., 2], s[..., 3], s[..., 10]], axis=-1)


# ------------------------------------------------------------------------------------------------------------ motions
def motion_pair(seed, N, body=None, same=False):
    """a seeded motion of N frames and a plausible prediction of it: (pose_p, pose_t [N,24,3,3], tran_p, tran_t [N,3]) float32.
    Truth: smooth joint angles and a slow walk; prediction: every joint off by a few degrees, the translation by centimetres."""
    from robustcap_amd import synth
    t = np.arange(N, dtype=np.float64)[:, None]
    amp = 0.5 * synth.normal(seed, 0, 72).astype(np.float64)[None]
    ph = 6.28 * synth.uniform01(seed, 1, 72).astype(np.float64)[None]
    fr = 0.05 + 0.2 * synth.uniform01(seed, 2, 72).astype(np.float64)[None]
    aa = (amp * np.sin(fr * t + ph)).reshape(N, 24, 3)
    gt = synth._rodrigues(aa).astype(np.float32)
    near = synth._rodrigues((0.08 * synth.normal(seed, 3, N * 72)).reshape(N, 24, 3).astype(np.float64)).astype(np.float32)
    tran_t = (np.cumsum(0.01 * synth.normal(seed, 4, N * 3).reshape(N, 3).astype(np.float64), axis=0) + [0.1, -0.2, 3.0]).astype(np.float32)
    if same:
        return gt.copy(), gt, tran_t.copy(), tran_t
    pred = np.matmul(gt, near).astype(np.float32)
    tran_p = (tran_t + 0.02 * synth.normal(seed, 5, N * 3).reshape(N, 3)).astype(np.float32)
    return pred, gt, tran_p, tran_t


def golden_translations(T):
    """the seeded translations of the captured fixture (tools/capture_motion_metrics.py): (tran_p, tran_t) [T,3] float32"""
    from robustcap_amd import synth
    tt = (np.cumsum(0.01 * synth.normal(61, 0, T * 3).reshape(T, 3).astype(np.float64), axis=0) + [0.1, -0.2, 3.0]).astype(np.float32)
    tp = (tt + 0.02 * synth.normal(61, 1, T * 3).reshape(T, 3)).astype(np.float32)
    return tp, tt


GOLDEN_SETTINGS = {                    # name -> (fps, joint_mask, align_joint) of the captured fixture
    "fps60": (60, None, 0),
    "fps5_mask": (5, [1, 2, 16, 17, 20], 0),
    "align5": (60, None, 5),
}
GOLDEN_MOTIONS = ("near", "far", "same")
GOLDEN_LONG = (62, 131)                # motion_pair(seed, frames) of the captured `long` motion: 71 one-second windows at fps 60
GOLDEN_LONG_SETTINGS = ("fps60", "align5")
GOLDEN_LONG_INPUTS = ("pose_p", "pose_t", "tran_p", "tran_t")                     # meta.json: sha256 of these arrays' bytes, in this order


def golden_long():
    """the `long` motion of the captured fixture, regenerated from its seed: (pose_p, pose_t, tran_p, tran_t) and {name: sha256 of the
    array's float32 bytes}, which meta.json records for the arrays the reference was run on"""
    import hashlib
    arrs = motion_pair(*GOLDEN_LONG)
    return arrs, {k: hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest() for k, a in zip(GOLDEN_LONG_INPUTS, arrs)}
