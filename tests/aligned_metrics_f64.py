"""float64 restatement of art.math.svd_rotate (articulate/math/angular.py:144-184) and of the three evaluators that align with it
(articulate/evaluator.py:195-210 PerJointErrorEvaluator, :241-253 MeanPerJointErrorEvaluator, :298-313 MeshErrorEvaluator), their float32
transcription, the bound, the inputs and the mutations -- TEST INFRASTRUCTURE, NOT PRODUCT. It shares no code with csrc/rc_align.hip.

`svd_rotate(..., dtype=np.float64)` is the restatement, line by line, with np.linalg.svd in place of torch.svd (H = U S V^T; numpy returns
V^T); `dtype=np.float32` is the same text in float32: the transcription of the reference, which *is* a float32 computation. `evaluate`
runs both evaluators' position halves on the forward kinematics and skinning of tests/motion_metrics_f64.py (model.py:229-241 written out).

The bound of every compared entry (the project's K = 8 convention):
    Bound = K |float32 transcription - float64 restatement| + 1e-7 scale,
per entry, scale taken from the restatement's inputs, never from the code under test:
    positions (errors, t, moved)   max |src| + max |dst| + max |t|
    entries of R                   1
    s                              max(1, s)
This is a bound on a well-conditioned fit only: every input used by the tests has s3 >= 1e-3 s1 for the H of every frame (`conditioning`;
tests/test_aligned_metrics_cpu.py asserts it), joints and mesh alike. No frame or set is dropped to get there: an input that fails is
given another seed (CASES, AUX, SVD_CASES and GOLDEN_POINTS carry seeds found that way), and the `far` pair of the captured fixture is a
seeded pair of this file, because 4 of the 24 `far` frames of tests/golden/metrics.npz fail (3.6e-4 at worst).
Only where the captured float32 reference is one side of a comparison, `bound(..., block=...)` takes the transcription's error over the
entries one fit produces together (see there); the device and the mutations are held to the per-entry form.

`mut` names one deliberate mistake each (MUTATIONS: the output it must move by more than the Bound):
    flip_column          the reflection fix negates COLUMN 2 of V (the reference negates row 2)
    proper_rotation      R = V diag(1, 1, det) U^T, the Kabsch choice; with sorted singular values it is the same matrix as flip_column, reached
                         by the other route (hestenes3's cross products would give it), so both names are kept
    trace_scale          s = trace(R H) / sum |src - mu_s|^2, Procrustes' scale
    means_without_t      the means are subtracted although calc_t is off
    R_transposed         R^T in place of R
    mesh_uses_joint_fit  the mesh is moved by the transform fitted on the joints

`fold_constants` / `fold_sums` restate the fold the device uses for the mesh fit (C[j,k] = sum_v w_vj w_vk x~_v x~_v^T, m_j = sum_v w_vj x~_v)
in float64 numpy; `vertex_sums` are the same sums vertex by vertex.
"""
import numpy as np

import motion_metrics_f64 as M

K = 8.0
REL = 1e-7
MODES = {-1: (True, True, True), -2: (True, True, False), -3: (False, True, True), -4: (False, True, False), -5: (False, False, True)}
WHAT = {mode: (1 if r else 0) | (2 if t else 0) | (4 if s else 0) for mode, (r, t, s) in MODES.items()}
FLAG_COMBOS = tuple(MODES.values())
MUTATIONS = {                       # mutation -> (mode it shows in, output it must move)
    "flip_column": (-1, "joint_err"),
    "proper_rotation": (-2, "joint_err"),
    "trace_scale": (-1, "joint_err"),
    "means_without_t": (-5, "joint_err"),
    "R_transposed": (-2, "joint_err"),
    "mesh_uses_joint_fit": (-1, "mesh_err"),
}
REFLECTION_MUTATIONS = ("flip_column", "proper_rotation")       # they show on frames whose Q is improper only


def svd_rotate(src, dst, calc_R=True, calc_t=False, calc_s=False, dtype=np.float64, mut=None):
    """angular.py:159-184 on [n,m,3] arrays -> (R [n,3,3], t [n,3], s [n], moved [n,m,3]) in `dtype`"""
    src, dst = np.asarray(src).astype(dtype), np.asarray(dst).astype(dtype)
    n = src.shape[0]
    centre = calc_t or mut == "means_without_t"
    mu_s = src.mean(axis=1, keepdims=True, dtype=dtype) if centre else np.zeros_like(src[:, :1])
    mu_d = dst.mean(axis=1, keepdims=True, dtype=dtype) if centre else np.zeros_like(dst[:, :1])
    a, b = src - mu_s, dst - mu_d
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.sqrt((b * b).sum(axis=(1, 2), dtype=dtype) / (a * a).sum(axis=(1, 2), dtype=dtype)) if calc_s else np.ones(n, dtype)
    H = np.matmul(a.transpose(0, 2, 1), b)
    if calc_R:
        R = np.empty((n, 3, 3), dtype)
        for i in range(n):
            u, _, vt = np.linalg.svd(H[i])
            v = vt.T.copy()
            q = v @ u.T
            if np.linalg.det(q) < -0.9:
                if mut == "flip_column":
                    v[:, 2] = -v[:, 2]
                    q = v @ u.T
                elif mut == "proper_rotation":
                    q = v @ np.diag(np.array([1, 1, -1], dtype)) @ u.T
                else:
                    v[2] = -v[2]                                  # angular.py:176: v[i, 2] is a ROW of V
                    q = v @ u.T
            R[i] = q.T if mut == "R_transposed" else q
    else:
        R = np.tile(np.eye(3, dtype=dtype), (n, 1, 1))
    if calc_s and mut == "trace_scale":
        with np.errstate(divide="ignore", invalid="ignore"):
            s = (np.trace(np.matmul(R, H), axis1=1, axis2=2) / (a * a).sum(axis=(1, 2), dtype=dtype)).astype(dtype)
    if not calc_t:
        mu_s, mu_d = np.zeros_like(mu_s), np.zeros_like(mu_d)
    t = -s[:, None, None] * np.matmul(R, mu_s.transpose(0, 2, 1)) + mu_d.transpose(0, 2, 1)
    moved = s[:, None, None] * np.matmul(src, R.transpose(0, 2, 1)) + t.transpose(0, 2, 1)
    return R.astype(dtype), t[:, :, 0].astype(dtype), s.astype(dtype), moved.astype(dtype)


def _fk(body, pose, dtype):
    _, j, v = M.fk(body, pose, None, M.F64 if dtype == np.float64 else M.F32)
    return j.numpy(), v.numpy()


def evaluate(body, pose_p, pose_t, mode, dtype=np.float64, mut=None, mesh=True):
    """one motion: dict(je [N,24], joint_err [24], ve [N,V], mesh_err, per_frame [N,2], xform [N,2,13], pos_j, pos_v) as float64 arrays;
    pos_j / pos_v are the position scales (max |src| + max |dst| + max |t|) of the joint and the mesh half"""
    calc = MODES[mode]
    jp, vp = _fk(body, pose_p, dtype)
    jt, vt = _fk(body, pose_t, dtype)
    N = jp.shape[0]
    nrm = lambda z: float(np.linalg.norm(np.asarray(z, np.float64), axis=-1).max())
    Rj, tj, sj, mj = svd_rotate(jp, jt, *calc, dtype=dtype, mut=mut)
    je = np.linalg.norm(mj - jt, axis=2)
    out = {"je": je, "joint_err": je.mean(axis=0, dtype=dtype), "pos_j": nrm(jp) + nrm(jt) + nrm(tj)}
    xf = np.full((N, 2, 13), np.nan)
    xf[:, 0] = np.concatenate([Rj.reshape(N, 9), tj, sj[:, None]], axis=1)
    pf = np.full((N, 2), np.nan)
    pf[:, 0] = je.mean(axis=1, dtype=dtype)
    if mesh:
        if mut == "mesh_uses_joint_fit":
            Rm, tm, sm = Rj, tj, sj
            mv = sm[:, None, None] * np.matmul(vp, Rm.transpose(0, 2, 1)) + tm[:, None]
        else:
            Rm, tm, sm, mv = svd_rotate(vp, vt, *calc, dtype=dtype, mut=mut)
        ve = np.linalg.norm(mv - vt, axis=2)
        out.update(ve=ve, mesh_err=float(ve.mean(dtype=dtype)), pos_v=nrm(vp) + nrm(vt) + nrm(tm))
        xf[:, 1] = np.concatenate([Rm.reshape(N, 9), tm, sm[:, None]], axis=1)
        pf[:, 1] = ve.mean(axis=1, dtype=dtype)
    out.update(xform=xf, per_frame=pf)
    return {k: (np.asarray(v, np.float64) if isinstance(v, np.ndarray) else v) for k, v in out.items()}


def evaluate_groups(body, pose_p, pose_t, sizes, mode, dtype=np.float64, mut=None, mesh=True):
    """every motion of a concatenated batch on its own: dict(joint_err [G,24], mesh_err [G], per_frame [n,2], xform [n,2,13],
    pos_j [G], pos_v [G], frame_group [n])"""
    parts, at = [], 0
    for N in sizes:
        parts.append(evaluate(body, np.asarray(pose_p)[at:at + N], np.asarray(pose_t)[at:at + N], mode, dtype, mut, mesh))
        at += N
    out = {"joint_err": np.stack([p["joint_err"] for p in parts]), "per_frame": np.concatenate([p["per_frame"] for p in parts]),
           "xform": np.concatenate([p["xform"] for p in parts]), "pos_j": np.array([p["pos_j"] for p in parts]),
           "frame_group": np.concatenate([np.full(N, g) for g, N in enumerate(sizes)])}
    if mesh:
        out["mesh_err"] = np.array([p["mesh_err"] for p in parts])
        out["pos_v"] = np.array([p["pos_v"] for p in parts])
    return out


def bound(f32, f64, scale, block=None):
    """K |float32 - float64| + 1e-7 scale per entry (scale broadcasts against the entry). `block` is for comparisons with the CAPTURED
    float32 reference only: axes over which the transcription's error is taken as its largest entry -- the entries one fit produces
    together (the nine of an R, the three of a t, the moved points of a set, the 24 joint errors of a motion). Two float32 SVDs (torch's
    LAPACK in the fixture, numpy's here) spread a fit's rounding error over those entries in different proportions, so where this
    transcription happens to be exact in one entry it says nothing about the other's error there: the fixture is 2.2 per-entry bounds off in
    one entry of an R of four points and 0.56 of the block bound. The device (float64 inside, rounded once) needs no such allowance."""
    with np.errstate(invalid="ignore"):
        e32 = np.abs(np.asarray(f32, np.float64) - np.asarray(f64, np.float64))
    e32 = np.where(np.isfinite(e32), e32, 0.0)
    if block is not None:
        e32 = e32.max(axis=block, keepdims=True)
    return K * e32 + REL * np.asarray(scale, np.float64)


def ratios(got, f64, bnd):
    """|got - f64| / Bound per entry (0 where both are NaN or both the same infinity); raises where NaNs or infinities differ"""
    got, f64 = np.asarray(got, np.float64), np.asarray(f64, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(f64)), ("NaN placement", got, f64)
    inf = np.isinf(f64)
    assert np.array_equal(got[inf], f64[inf]) and not np.isinf(got[~inf]).any(), ("infinities", got, f64)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - f64)
        r = err / np.broadcast_to(bnd, err.shape)
    return np.where(np.isnan(f64) | inf | (err == 0.0), 0.0, r)


def xform_bound(x32, x64, pos):
    """the per-entry Bound of xform [..., 13] = R [9] | t [3] | s: scale 1 for R, the position scale `pos` (broadcast over the leading axes)
    for t, max(1, s) for s"""
    x32, x64 = np.asarray(x32, np.float64), np.asarray(x64, np.float64)
    pos = np.broadcast_to(np.asarray(pos, np.float64), x64.shape[:-1])[..., None]
    with np.errstate(invalid="ignore"):
        s_scale = np.where(np.isfinite(x64[..., 12:]), np.maximum(1.0, np.abs(x64[..., 12:])), 1.0)
    return np.concatenate([bound(x32[..., :9], x64[..., :9], 1.0), bound(x32[..., 9:12], x64[..., 9:12], pos),
                           bound(x32[..., 12:], x64[..., 12:], s_scale)], axis=-1)


# ---------------------------------------------------------------------------------------------------- the fold, in float64 numpy
def transforms(body, pose):
    """A [n,24,3,4] = [G_j | P_j - G_j J_j], float64: a skinned vertex is sum_j w[v,j] A_j (x_v, 1)"""
    G, P, _ = M.fk({**body, "v_template": np.asarray(body["v_template"])[:1], "weights": np.asarray(body["weights"])[:1]}, pose, None, M.F64)
    G, P = G.numpy(), P.numpy()
    J = np.asarray(body["J"], np.float32).astype(np.float64)
    j = J - J[:1]
    T = P - np.einsum("njrc,jc->njr", G, j)
    return np.concatenate([G, T[..., None]], axis=-1)


def rest_points(body):
    """x~ [V,4] = (v_template - J_0, 1) and the weights [V,24], float64"""
    J = np.asarray(body["J"], np.float32).astype(np.float64)
    x = np.asarray(body["v_template"], np.float32).astype(np.float64) - J[:1]
    return np.concatenate([x, np.ones((x.shape[0], 1))], axis=1), np.asarray(body["weights"], np.float32).astype(np.float64)


def fold_constants(body):
    """C [24,24,4,4] = sum_v w[v,j] w[v,k] x~_v x~_v^T and m [24,4] = sum_v w[v,j] x~_v"""
    xt, w = rest_points(body)
    C = np.zeros((24, 24, 4, 4))
    for j in range(24):
        for k in range(j, 24):
            ww = w[:, j] * w[:, k]
            if ww.any():
                C[j, k] = (xt * ww[:, None]).T @ xt
                C[k, j] = C[j, k]
    return C, w.T @ xt


def fold_sums(C, m, A, B):
    """one frame, A, B [24,3,4]: (sum_v p_v t_v^T [3,3], sum_v p_v [3], sum_v t_v [3], sum_v |p_v|^2, sum_v |t_v|^2) from the fold"""
    return (np.einsum("jra,jkab,ksb->rs", A, C, B), np.einsum("jra,ja->r", A, m), np.einsum("jra,ja->r", B, m),
            float(np.einsum("jra,jkab,krb->", A, C, A)), float(np.einsum("jra,jkab,krb->", B, C, B)))


def vertex_sums(body, A, B):
    """the same five sums vertex by vertex"""
    xt, w = rest_points(body)
    p = np.einsum("vj,jra,va->vr", w, A, xt)
    q = np.einsum("vj,jra,va->vr", w, B, xt)
    return p.T @ q, p.sum(axis=0), q.sum(axis=0), float((p * p).sum()), float((q * q).sum())


def conditioning(body, pose_p, pose_t):
    """(s3 / s1 of every frame's centred joint H [n], of every frame's centred mesh H [n], det of both H [n,2])"""
    jp, vp = _fk(body, pose_p, np.float64)
    jt, vt = _fk(body, pose_t, np.float64)
    out, dets = [], []
    for a, b in ((jp, jt), (vp, vt)):
        a, b = a - a.mean(axis=1, keepdims=True), b - b.mean(axis=1, keepdims=True)
        H = np.matmul(a.transpose(0, 2, 1), b)
        sv = np.linalg.svd(H, compute_uv=False)
        out.append(sv[:, 2] / sv[:, 0])
        dets.append(np.linalg.det(H))
    return out[0], out[1], np.stack(dets, axis=1)


def conditioning_points(src, dst, centre=True):
    """s3 / s1 of the H of every point set [n] (centred: the fits with calc_t; not centred: those without)"""
    a, b = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    if centre:
        a, b = a - a.mean(axis=1, keepdims=True), b - b.mean(axis=1, keepdims=True)
    sv = np.linalg.svd(np.matmul(a.transpose(0, 2, 1), b), compute_uv=False)
    return sv[:, 2] / sv[:, 0]


# ------------------------------------------------------------------------------------------------------------ inputs
def _many_groups():
    """40 groups: 37 of 1, 2, 3, 1, ... frames and, at positions 0, 17 and 39, groups of 33, 65 and 33 frames: the bisection over the
    block table has to find a block inside a long group and one-block groups between long ones"""
    long_ones, short = {0: 33, 17: 65, 39: 33}, iter(range(37))
    return tuple(long_ones[k] if k in long_ones else 1 + next(short) % 3 for k in range(40))


MANY_GROUPS = _many_groups()
COND_MIN = 1e-3
CASES = [
    # name, V, group lengths, seed, far (the seeds: the first from 2000 on whose every frame meets COND_MIN with some margin)
    ("tiny mesh V=5", 5, (1, 2, 33), 2016, False),
    ("slab edge V=1023", 1023, (31, 32), 2020, False),
    ("slab edge V=1024 far", 1024, (33, 1), 2050, True),
    ("slab edge V=1025", 1025, (65, 3), 2053, False),
    ("many groups V=1025", 1025, MANY_GROUPS, 2056, False),
    ("full mesh V=6890 far", 6890, (33,), 2111, True),
]
AUX = {                             # the other pose inputs of the tests: name -> (V, group lengths, seed, far)
    "golden far": (6890, (24,), 2123, True),
    "fold V=5": (5, (2,), 2135, True), "fold V=1025": (1025, (2,), 2139, True), "fold V=6890": (6890, (2,), 2141, True),
    "root turned": (1025, (5,), 2143, False), "mode 4": (1023, (7,), 2145, False),
    "alone 0": (1025, (1,), 2147, False), "alone 1": (1025, (33,), 2157, True), "alone 2": (1025, (7,), 2159, False),
    "alone 3": (1025, (65,), 2161, False),
    "small": (1025, (7,), 2163, False), "large": (1025, (65, 33, 3), 2165, False), "refusals": (1025, (8,), 2169, False),
}


def pose_batch(body, sizes, seed0, far=False):
    """(pose_p, pose_t) [n,24,3,3] float32 of concatenated motions: the truth of motion_metrics_f64.motion_pair and its prediction a few
    degrees off every joint; far: the prediction is the truth of ANOTHER seeded motion, tens of degrees off, and some of its fits are
    improper. `body` is not read (the conditioning of the frames on it is asserted by tests/test_aligned_metrics_cpu.py)."""
    P, T = [], []
    for i, N in enumerate(sizes):
        pp, pt, _, _ = M.motion_pair(seed0 + i, N)
        if far:
            pp = M.motion_pair(seed0 + 1000 + i, N)[1]
        P.append(pp), T.append(pt)
    return np.concatenate(P), np.concatenate(T)


def aux(name, body):
    V, sizes, seed, far = AUX[name]
    assert np.asarray(body["v_template"]).shape[0] == V, name
    return pose_batch(body, sizes, seed, far)


def root_turned(pose, seed):
    """the motion with its root turned by a seeded rotation of 1.5 to 2.5 rad (far from I): joints and mesh turn rigidly about the root"""
    from robustcap_amd import synth
    ax = synth.normal(seed, 0, 3).astype(np.float64)
    ang = 1.5 + float(synth.uniform01(seed, 1, 1)[0])
    Q = synth._rodrigues((ax / np.linalg.norm(ax) * ang)[None])[0]
    out = np.array(pose, np.float32, copy=True)
    out[:, 0] = (Q @ out[:, 0].astype(np.float64)).astype(np.float32)
    return out, Q


def point_sets(seed, n, m, mirrored=False):
    """(src, dst) [n,m,3] float32: seeded sources of anisotropic spread round a seeded centre and dst = s R src + t plus 2 % noise; mirrored:
    dst is the source mirrored in x, then rotated (every set's Q is improper). Also (R, t, s) of the construction. THREE points are
    coplanar once centred: H has rank 2, the sign of det(V U^T) is LAPACK's accident, and with calc_R only s and the orthogonality of R
    are defined (R_DEFINED)."""
    from robustcap_amd import synth
    src = synth.normal(seed, 0, n * m * 3).reshape(n, m, 3).astype(np.float64) * [1.0, 0.7, 0.4] + synth.normal(seed, 1, n * 3).reshape(n, 1, 3)
    aa = 2.5 * (synth.uniform01(seed, 2, n * 3).reshape(n, 3).astype(np.float64) - 0.5)
    R = synth._rodrigues(aa)
    s = 0.5 + synth.uniform01(seed, 3, n).astype(np.float64)
    t = synth.normal(seed, 4, n * 3).reshape(n, 3).astype(np.float64)
    base = src * [-1.0, 1.0, 1.0] if mirrored else src
    dst = s[:, None, None] * np.matmul(base, R.transpose(0, 2, 1)) + t[:, None] + 0.02 * synth.normal(seed, 5, n * m * 3).reshape(n, m, 3)
    return src.astype(np.float32), dst.astype(np.float32), (R, t, s)


def R_DEFINED(m):
    return m >= 4


UNCENTRED_FROM = 24                 # point sets of at least this many points also run calc_R without calc_t (svd_rotate's default flags)
SVD_CASES = [
    # m, n, seed, mirrored (m >= 4: the first seed from 3000 on whose every set meets COND_MIN with some margin; four points leave a set
    # thin in one direction often enough that 64 sets of them never all pass, so n = 64 goes with m = 33)
    (3, 63, 480, False), (4, 1, 3021, False), (24, 65, 3002, False), (33, 64, 3030, False), (64, 5, 3004, False), (65, 5, 3005, False),
    (24, 7, 3006, True),
]
EXACT_POINTS, SPREADLESS_TARGETS = (3016, 9, 24), (3017, 2, 5)     # point_sets(seed, n, m) of two more GPU tests


def exact_point_sets(seed, n, m):
    """(src, dst, (R, t, s)) with dst = s R src + t computed in float64 and rounded to float32: the fit recovers the construction"""
    src, _, (R, t, s) = point_sets(seed, n, m)
    dst = s[:, None, None] * np.matmul(src.astype(np.float64), R.transpose(0, 2, 1)) + t[:, None]
    return src, dst.astype(np.float32), (R, t, s)


# ----------------------------------------------------------------------------------------------------- the captured fixture
GOLDEN_MOTIONS = ("near", "far")


def golden_motions(metrics, body):
    """the pose pairs of the captured fixture: `near` = pose_near against pose_gt of tests/golden/metrics.npz (24 frames), `far` = the seeded
    far pair AUX["golden far"] (24 frames, 8 of them with an improper joint fit): {name: (pose_p, pose_t)}"""
    return {"near": (metrics["pose_near"], metrics["pose_gt"]), "far": aux("golden far", body)}


GOLDEN_POINTS = {"m3": (470, 6, 3, False), "m4": (3012, 6, 4, False), "m24": (3013, 5, 24, False), "m33": (3014, 5, 33, False),
                 "m24_mirrored": (3015, 5, 24, True)}     # name -> point_sets(seed, n, m, mirrored)


def flag_name(calc):
    return "".join(c for c, on in zip("Rts", calc) if on)
