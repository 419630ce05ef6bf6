"""float64 restatement of the evaluation metrics, their bounds, cases and mutations -- TEST INFRASTRUCTURE, NOT PRODUCT.

What rc_metrics.hip computes (Procrustes alignment, MPJPE / PVE / PA-MPJPE over the full mesh, the folded regressor, rc_body_mesh)
restated from the reference's own lines, in float64 on the float32 inputs the device gets:
  utils.py:138-203        compute_similarity_transform / reconstruction_error   -> procrustes (float64 numpy SVD)
  evaluate.py:120-133     cal_mpjpe                                             -> frame_metrics_f64
  articulate/model.py:235-241  full-mesh linear-blend skinning                  -> mesh_f64
oracle/metrics_oracle.py keeps the reference's float32 SVD on purpose (it is pinned to the reference capture); it cannot judge a
float64 Procrustes. `procrustes_second` is an independent formulation (Horn's unit-quaternion method, in mpmath at 50 digits
where mpmath is installed, else float64): the difference e64 of the two shows where a point set is ill-posed.

Bounds:
  MPJPE, PVE, PA of the mesh metrics, mesh vertices:  Bound = M max(e32, eps32 A), M = 4; e32 = the largest deviation from
      float64 of three float32 evaluations of the reference formulation (joint sum j = 0..23, j = 23..0, pairwise; the
      regressor / vertex-mean sums over vertices in index order, reversed, pairwise), A the magnitude of the summed terms:
          vertex coordinate   A_v = sum_j w[v,j] (|G_j| |x_v| + |T_j|) + |tran|
          vertex error        the same sum over both poses
          keypoint            A_k = sum_v |Jr[k,v]| A_v       (pelvis-aligned: A_k + A_0, over both poses)
          per-frame mean      the mean of its terms' A
      PA-MPJPE of the mesh metrics runs the float64 Procrustes on float32 keypoints: the keypoints' rounding is what it
      carries (an aligned residual moves by at most the size of the perturbation of its points times a small constant,
      since scale ~ 1 and the residual is no larger than the set), so it has the MPJPE's A.
  reconstruction_error on raw point sets: float64 on the device, rounded once to float32:
      Bound_pa = 4 * 2^-24 * A, A = mean_j |S2_j - mu2|, the size of the numbers the result is a difference of.
      A case is admitted only if e64 <= Bound_pa / 8.
"""
import dataclasses

import numpy as np

from robustcap_amd import synth

F32, F64 = np.float32, np.float64
EPS32 = 2.0 ** -24
M = 4.0                 # as for the tail and the smplify gradient: the smallest power of two above MARGIN
MARGIN = 3.0            # float32 evaluations at most Bound / MARGIN, mutations at least MARGIN * Bound
ADMIT = 8.0             # a Procrustes case is admitted only if e64 <= Bound_pa / ADMIT
GAP_MIN = 0.05          # (sigma2 - sigma3) / sigma1 of the full-extent det < 0 cases compared in the mean
MET_FG, MET_SLAB, MET_CHUNK = 16, 1024, 65536          # frame group, vertex slab, frames per launch of rc_metrics.hip

try:
    import mpmath as _mp
except ImportError:                                                         # float64 Horn then
    _mp = None

PA_MUTATIONS = ("no_Z", "scale_1", "scale_var2", "R_transposed", "means_kept")
MESH_MUTATIONS = ("pelvis_kp1", "align_before_pve", "pve_padded_count", "mpjpe_all_rows", "tran_kept", "fold_without_root",
                  "weight_row_shifted", "group_last_frame_repeated")


# ------------------------------------------------------------------------------------------------------ Procrustes
def _align_one(S1, S2, mut=None):
    """utils.py:138-187 on one pair [k,3], float64 SVD. Returns (residual [k,3], singular values, sign det(U V^T))."""
    a, b = np.asarray(S1, F64).T, np.asarray(S2, F64).T                     # [3,k]
    mu1, mu2 = a.mean(axis=1, keepdims=True), b.mean(axis=1, keepdims=True)
    if mut == "means_kept":
        mu1, mu2 = np.zeros_like(mu1), np.zeros_like(mu2)
    X1, X2 = a - mu1, b - mu2
    var1 = np.sum(X1 ** 2)
    K = X1.dot(X2.T)
    U, s, Vh = np.linalg.svd(K)
    V = Vh.T
    sign = float(np.sign(np.linalg.det(U.dot(V.T))))
    Z = np.eye(3)
    if mut != "no_Z":
        Z[-1, -1] *= sign
    R = V.dot(Z.dot(U.T))
    if mut == "R_transposed":
        R = R.T
    if var1 == 0.0:                  # the reference divides by zero here; the device's documented value: scale = 0
        scale = 0.0
    elif mut == "scale_1":
        scale = 1.0
    elif mut == "scale_var2":
        scale = np.trace(R.dot(K)) / np.sum(X2 ** 2)
    else:
        scale = np.trace(R.dot(K)) / var1
    return (scale * R.dot(X1) - X2).T, s, sign


def procrustes(S1, S2, mut=None):
    """S1, S2 [n,k,3] float32 -> dict of [n] arrays: mean (per-set mean distance after alignment), ssq (sum of squared
    residuals), sigma [n,3] (singular values of K), sign (sign det(U V^T)), A (mean_j |S2_j - mu2|, for Bound_pa)."""
    S1, S2 = np.asarray(S1, F32), np.asarray(S2, F32)
    n = S1.shape[0]
    out = {"mean": np.zeros(n), "ssq": np.zeros(n), "sigma": np.zeros((n, 3)), "sign": np.zeros(n), "A": np.zeros(n)}
    for i in range(n):
        res, s, sign = _align_one(S1[i], S2[i], mut)
        out["mean"][i] = np.sqrt((res ** 2).sum(axis=1)).mean()
        out["ssq"][i] = (res ** 2).sum()
        out["sigma"][i], out["sign"][i] = s, sign
        b = S2[i].astype(F64)
        out["A"][i] = np.sqrt(((b - b.mean(axis=0)) ** 2).sum(axis=1)).mean()
    return out


def bound_pa(A):
    return 4.0 * EPS32 * np.asarray(A, F64)


def _horn_float64(a, b):
    mu1, mu2 = a.mean(axis=0), b.mean(axis=0)
    X1, X2 = a - mu1, b - mu2
    var1 = (X1 ** 2).sum()
    if var1 == 0.0:
        return X2 * -1.0
    S = X1.T @ X2                                                            # S[r,c] = sum_j x1_r x2_c
    N = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                  [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                  [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                  [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])
    w, x, y, z = np.linalg.eigh(N)[1][:, -1]
    R = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])
    Y = X1 @ R.T
    return (Y * X2).sum() / var1 * Y - X2


def _horn_mpmath(a, b):
    mp = _mp.mp
    k = a.shape[0]
    A = [[mp.mpf(float(v)) for v in row] for row in a]
    B = [[mp.mpf(float(v)) for v in row] for row in b]
    mu1 = [sum(A[j][c] for j in range(k)) / k for c in range(3)]
    mu2 = [sum(B[j][c] for j in range(k)) / k for c in range(3)]
    X1 = [[A[j][c] - mu1[c] for c in range(3)] for j in range(k)]
    X2 = [[B[j][c] - mu2[c] for c in range(3)] for j in range(k)]
    var1 = sum(X1[j][c] ** 2 for j in range(k) for c in range(3))
    if var1 == 0:
        return np.array([[-float(v) for v in row] for row in X2])
    S = [[sum(X1[j][r] * X2[j][c] for j in range(k)) for c in range(3)] for r in range(3)]
    N = mp.matrix([[S[0][0] + S[1][1] + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]],
                   [S[1][2] - S[2][1], S[0][0] - S[1][1] - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]],
                   [S[2][0] - S[0][2], S[0][1] + S[1][0], -S[0][0] + S[1][1] - S[2][2], S[1][2] + S[2][1]],
                   [S[0][1] - S[1][0], S[2][0] + S[0][2], S[1][2] + S[2][1], -S[0][0] - S[1][1] + S[2][2]]])
    E, Q = mp.eigsy(N)                                                       # ascending
    top = max(range(4), key=lambda i: E[i])
    w, x, y, z = (Q[i, top] for i in range(4))
    qn = w * w + x * x + y * y + z * z
    R = [[(w * w + x * x - y * y - z * z) / qn, 2 * (x * y - w * z) / qn, 2 * (x * z + w * y) / qn],
         [2 * (x * y + w * z) / qn, (w * w - x * x + y * y - z * z) / qn, 2 * (y * z - w * x) / qn],
         [2 * (x * z - w * y) / qn, 2 * (y * z + w * x) / qn, (w * w - x * x - y * y + z * z) / qn]]
    Y = [[sum(R[r][c] * X1[j][c] for c in range(3)) for r in range(3)] for j in range(k)]
    scale = sum(Y[j][c] * X2[j][c] for j in range(k) for c in range(3)) / var1
    return np.array([[float(scale * Y[j][c] - X2[j][c]) for c in range(3)] for j in range(k)])


def procrustes_second(S1, S2):
    """The same quantity by Horn's closed form: the rotation is the eigenvector of the largest eigenvalue of the 4x4 matrix
    built from K (always a proper rotation: no SVD, no Z), then the scale. mpmath at 50 digits if available, else float64.
    Returns dict(mean [n], ssq [n])."""
    S1, S2 = np.asarray(S1, F32), np.asarray(S2, F32)
    n = S1.shape[0]
    out = {"mean": np.zeros(n), "ssq": np.zeros(n)}
    for i in range(n):
        if _mp is not None:
            with _mp.workdps(50):
                res = _horn_mpmath(S1[i], S2[i])
        else:
            res = _horn_float64(S1[i].astype(F64), S2[i].astype(F64))
        out["mean"][i] = np.sqrt((res ** 2).sum(axis=1)).mean()
        out["ssq"][i] = (res ** 2).sum()
    return out


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _tail_of_kernel(K, v0, v1, X1, X2, var1, k):
    """the part of procrustes_error behind the two leading right singular vectors (unchanged by the one-sided route)"""
    v = [v0, v1, _cross(v0, v1)]
    u = [None, None, None]
    for i in range(2):
        u[i] = np.array([K[r][0] * v[i][0] + K[r][1] * v[i][1] + K[r][2] * v[i][2] for r in range(3)])
        if i == 1:
            d = u[0][0] * u[1][0] + u[0][1] * u[1][1] + u[0][2] * u[1][2]
            u[1] = u[1] - d * u[0]
        nrm = np.sqrt(u[i][0] * u[i][0] + u[i][1] * u[i][1] + u[i][2] * u[i][2])
        u[i] = u[i] / max(nrm, 1e-300)
    u[2] = _cross(u[0], u[1])
    R = np.zeros((3, 3))
    for r in range(3):
        for c in range(3):
            R[r][c] = v[0][r] * u[0][c] + v[1][r] * u[1][c] + v[2][r] * u[2][c]
    tr = 0.0
    for r in range(3):
        for c in range(3):
            tr += R[r][c] * K[c][r]
    scale = tr / max(var1, 1e-300)
    err = 0.0
    for j in range(k):
        e2 = 0.0
        for r in range(3):
            h = scale * (R[r][0] * X1[j][0] + R[r][1] * X1[j][1] + R[r][2] * X1[j][2]) - X2[j][r]
            e2 += h * h
        err += np.sqrt(e2)
    return err / k


def _kernel_head(S1, S2):
    p1, p2 = np.asarray(S1, F32).astype(F64), np.asarray(S2, F32).astype(F64)
    k = p1.shape[0]
    mu1, mu2 = np.zeros(3), np.zeros(3)
    for j in range(k):
        mu1 += p1[j]
        mu2 += p2[j]
    mu1, mu2 = mu1 / k, mu2 / k
    K, var1 = np.zeros((3, 3)), 0.0
    for j in range(k):
        a, b = p1[j] - mu1, p2[j] - mu2
        for c in range(3):
            var1 += a[c] * a[c]
        for r in range(3):
            for c in range(3):
                K[r][c] += a[r] * b[c]
    return K, var1, p1 - mu1, p2 - mu2, k


def ktk_route_one(S1, S2):
    """Line-for-line float64 emulation of `procrustes_error` as it stood before the one-sided Jacobi: the right singular
    vectors from a cyclic Jacobi on K^T K (which squares the condition number). A MUTATION: the thin rungs expose it."""
    K, var1, X1, X2, k = _kernel_head(S1, S2)
    A = np.zeros((3, 3))
    for r in range(3):
        for c in range(3):
            A[r][c] = K[0][r] * K[0][c] + K[1][r] * K[1][c] + K[2][r] * K[2][c]
    V = np.eye(3)
    for _ in range(12):
        if abs(A[0][1]) + abs(A[0][2]) + abs(A[1][2]) < 1e-300:
            break
        for p in range(2):
            for q in range(p + 1, 3):
                if abs(A[p][q]) < 1e-300:
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q])
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                for kk in range(3):
                    akp, akq = A[kk][p], A[kk][q]
                    A[kk][p], A[kk][q] = c * akp - s * akq, s * akp + c * akq
                for kk in range(3):
                    apk, aqk = A[p][kk], A[q][kk]
                    A[p][kk], A[q][kk] = c * apk - s * aqk, s * apk + c * aqk
                for kk in range(3):
                    vkp, vkq = V[kk][p], V[kk][q]
                    V[kk][p], V[kk][q] = c * vkp - s * vkq, s * vkp + c * vkq
    l0, l1, l2 = A[0][0], A[1][1], A[2][2]
    first = 0 if (l0 >= l1 and l0 >= l2) else (1 if l1 >= l2 else 2)
    second = ((1 if l1 >= l2 else 2) if first == 0 else ((0 if l0 >= l2 else 2) if first == 1 else (0 if l0 >= l1 else 1)))
    return _tail_of_kernel(K, V[:, first].copy(), V[:, second].copy(), X1, X2, var1, k)


def hestenes_route_one(S1, S2):
    """float64 emulation of `procrustes_error` with the one-sided (Hestenes) Jacobi on K itself: the columns of W = K V are
    rotated until they are orthogonal; sigma_i = |w_i|, u_i = w_i / sigma_i. What the device runs now."""
    K, var1, X1, X2, k = _kernel_head(S1, S2)
    W, V = K.copy(), np.eye(3)
    for _ in range(16):
        rotated = False
        for p in range(2):
            for q in range(p + 1, 3):
                al = W[0][p] * W[0][p] + W[1][p] * W[1][p] + W[2][p] * W[2][p]
                be = W[0][q] * W[0][q] + W[1][q] * W[1][q] + W[2][q] * W[2][q]
                ga = W[0][p] * W[0][q] + W[1][p] * W[1][q] + W[2][p] * W[2][q]
                if ga * ga <= 1e-30 * al * be:
                    continue
                rotated = True
                zeta = (be - al) / (2.0 * ga)
                t = (1.0 if zeta >= 0.0 else -1.0) / (abs(zeta) + np.sqrt(zeta * zeta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                for kk in range(3):
                    wp, wq = W[kk][p], W[kk][q]
                    W[kk][p], W[kk][q] = c * wp - s * wq, s * wp + c * wq
                    vp, vq = V[kk][p], V[kk][q]
                    V[kk][p], V[kk][q] = c * vp - s * vq, s * vp + c * vq
        if not rotated:
            break
    l = [W[0][i] * W[0][i] + W[1][i] * W[1][i] + W[2][i] * W[2][i] for i in range(3)]
    l0, l1, l2 = l
    first = 0 if (l0 >= l1 and l0 >= l2) else (1 if l1 >= l2 else 2)
    second = ((1 if l1 >= l2 else 2) if first == 0 else ((0 if l0 >= l2 else 2) if first == 1 else (0 if l0 >= l1 else 1)))
    return _tail_of_kernel(K, V[:, first].copy(), V[:, second].copy(), X1, X2, var1, k)


def route(fn, S1, S2):
    with np.errstate(over="ignore"):                     # theta * theta may overflow to inf (t -> 0), as on the device
        return np.array([fn(a, b) for a, b in zip(S1, S2)])


# ------------------------------------------------------------------------------------------- Procrustes cases
@dataclasses.dataclass
class PaGroup:
    name: str
    S1: np.ndarray          # [n,k,3] float32
    S2: np.ndarray
    kind: str = "mean"      # "mean": compared in the mean distance; "ssq": ill-posed, compared in the sum of squares only
    mirrored: bool = False
    thin: bool = False      # extents (1, e, e) / (1, e, 0): sigma2 / sigma1 <= e by construction


def _rot(seed, stream):
    """a seeded rotation matrix (float64): QR of a normal matrix, det +1"""
    q, r = np.linalg.qr(synth.normal(seed, stream, 9).reshape(3, 3).astype(F64))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def pair_of(seed, k, extents=(1.0, 1.0, 1.0), mirrored=False, scale=1.7, noise=0.02, shift=(0.3, -0.2, 0.5), unit=1.0, offset=0.0):
    """S2 = k seeded normal points with the given extents, rotated; S1 = the same points perturbed by `noise` (relative, per
    axis, so a thin set stays thin), mirrored in axis 1 if asked (inside the plane for an extent (., ., 0)), rotated
    otherwise, scaled and shifted. Both float32 [k,3]."""
    ext = np.asarray(extents, F64)
    base = synth.normal(seed, 1, k * 3).reshape(k, 3).astype(F64) * ext
    pert = base + noise * synth.normal(seed, 2, k * 3).reshape(k, 3).astype(F64) * ext
    if mirrored:
        pert = pert * np.array([1.0, -1.0, 1.0])
    S2 = base @ _rot(seed, 3).T
    S1 = scale * (pert @ _rot(seed, 4).T) + np.asarray(shift, F64)
    return (S1 * unit + offset).astype(F32), (S2 * unit + offset).astype(F32)


LADDER = ([(1.0, e, e) for e in (1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7)] + [(1.0, 1e-2, 0.0), (1.0, 1e-4, 0.0), (1.0, 1e-6, 0.0)])
DRAWS = 8
PA_NK = (3, 4, 14, 24, 33)
NK3_SEEDS = (130, 134, 135, 139)     # three points: the seeds between them draw triangles with sigma2 / sigma1 below GAP_MIN


def _stack(pairs):
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def ext_name(ext):
    return "(" + ",".join(f"{e:g}" for e in ext) + ")"


def build_pa_groups():
    """Every Procrustes group of the device file, one `reconstruction_error` call each (issue section 4)."""
    G = []
    for k in PA_NK:
        for mir in (False, True):
            seeds = NK3_SEEDS if k == 3 else [100 + 10 * k + d for d in range(4)]
            G.append(PaGroup(f"generic nk={k}" + (" mirrored" if mir else ""), *_stack([pair_of(s, k, mirrored=mir) for s in seeds]), mirrored=mir))
    for mir in (False, True):
        G.append(PaGroup("coplanar (1,1,0)" + (" mirrored in the plane" if mir else ""),
                         *_stack([pair_of(300 + d, 14, (1.0, 1.0, 0.0), mirrored=mir) for d in range(4)]), mirrored=mir))
    for r, ext in enumerate(LADDER):
        for mir in (False, True):
            G.append(PaGroup(f"thin {ext_name(ext)}" + (" mirrored" if mir else ""),
                             *_stack([pair_of(1000 + 100 * r + d, 14, ext, mirrored=mir) for d in range(DRAWS)]), mirrored=mir, thin=True))
    G.append(PaGroup("collinear (1,0,0)", *_stack([pair_of(400 + d, 14, (1.0, 0.0, 0.0)) for d in range(4)]), thin=True))
    S2 = np.stack([pair_of(500 + d, 14)[1] for d in range(4)])
    G.append(PaGroup("S1 == S2 bitwise", S2.copy(), S2))
    G.append(PaGroup("rotated scaled shifted copy", *_stack([pair_of(510 + d, 14, noise=0.0) for d in range(4)])))
    G.append(PaGroup("millimetre scale", *_stack([pair_of(520 + d, 14, unit=1e-3) for d in range(4)])))
    G.append(PaGroup("offset 1e3 m", *_stack([pair_of(530 + d, 14, offset=1e3) for d in range(4)])))
    for k in (1, 2):
        G.append(PaGroup(f"nk={k}", *_stack([pair_of(540 + 10 * k + d, k) for d in range(4)])))
    S1, S2 = _stack([pair_of(560 + d, 14) for d in range(4)])
    G.append(PaGroup("var1 = 0", np.broadcast_to(S1[:, :1], S1.shape).copy(), S2))
    return G


def ill_posed_groups():
    """sigma1 = sigma2 = sigma3 and det < 0: the least-squares rotation is not unique and the mean distance differs between
    minimisers; only the sum of squared residuals is defined. CPU file only (nk > 2: no device route without an export)."""
    tet = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], F32)
    cube = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], F32)
    return [PaGroup("regular tetrahedron against its mirror image", (-tet)[None], tet[None], kind="ssq", mirrored=True),
            PaGroup("cube against its mirror image", (cube * np.array([1, 1, -1], F32))[None], cube[None], kind="ssq", mirrored=True)]


# ------------------------------------------------------------------------------------------------------ the mesh
def _chain(body, pose, dtype):
    """model.py:229-235: global rotations G [n,24,3,3] and T_j = P_j - G_j j_j [n,24,3] (root joint at the origin)."""
    J = np.asarray(body["J"], F32).astype(dtype)
    j = J - J[:1]
    parent = [int(p) for p in body["parent"]]
    pose = np.asarray(pose, F32).astype(dtype).reshape(-1, 24, 3, 3)
    n = pose.shape[0]
    G, P = np.zeros((n, 24, 3, 3), dtype), np.zeros((n, 24, 3), dtype)
    G[:, 0] = pose[:, 0]
    for i in range(1, 24):
        p = parent[i]
        G[:, i] = np.matmul(G[:, p], pose[:, i])
        P[:, i] = P[:, p] + np.matmul(G[:, p], (j[i] - j[p])[:, None])[..., 0]
    T = P - np.matmul(G, j[None, :, :, None])[..., 0]
    return G, T


def _ordered_sum(term, count, order):
    """sum_{i < count} term(i) in float32 (or whatever dtype the terms have) in one of three association orders"""
    if order == "fwd" or order == "rev":
        idx = range(count) if order == "fwd" else range(count - 1, -1, -1)
        acc = None
        for i in idx:
            acc = term(i) if acc is None else acc + term(i)
        return acc

    def rec(lo, hi):
        if hi - lo == 1:
            return term(lo)
        mid = (lo + hi) // 2
        return rec(lo, mid) + rec(mid, hi)
    return rec(0, count)


def _axis_sum(x, axis, order):
    """float32 sum along an axis: index order, reversed, or pairwise (halving)"""
    x = np.moveaxis(x, axis, 0)
    if order == "fwd":
        return np.cumsum(x, axis=0, dtype=x.dtype)[-1]
    if order == "rev":
        return np.cumsum(x[::-1], axis=0, dtype=x.dtype)[-1]
    while x.shape[0] > 1:
        if x.shape[0] % 2:
            x = np.concatenate([x, np.zeros_like(x[:1])], axis=0)
        x = x[0::2] + x[1::2]
    return x[0]


ORDERS = ("fwd", "rev", "pair")


def _skin(body, pose, tran, dtype, order="fwd", shift_row=None, root_offset=True):
    """model.py:235-241: T_vertex = sum_j w[v,j] T_global_j, vertex = T_vertex [x_v; 1] (+ tran). [n,V,3] in `dtype`."""
    G, T = _chain(body, pose, dtype)
    w = np.asarray(body["weights"], F32).astype(dtype)
    if shift_row is not None:
        w = w.copy()
        w[shift_row] = np.roll(w[shift_row], 1)
    x = np.asarray(body["v_template"], F32).astype(dtype)
    if root_offset:
        x = x - np.asarray(body["J"], F32).astype(dtype)[:1]
    GT = np.concatenate([G, T[..., None]], axis=-1)                          # [n,24,3,4]
    if dtype == F64:
        Tv = np.einsum("vj,njab->nvab", w, GT)
    else:
        Tv = _ordered_sum(lambda jj: w[None, :, jj, None, None] * GT[:, None, jj], 24, order)
    v = (Tv[..., 0] * x[None, :, None, 0] + Tv[..., 1] * x[None, :, None, 1]) + Tv[..., 2] * x[None, :, None, 2] + Tv[..., 3]
    if tran is not None:
        v = v + np.asarray(tran, F32).astype(dtype).reshape(-1, 1, 3)
    return v


def _vertex_A(body, pose, tran=None):
    """A_v [n,V] = sum_j w[v,j] (|G_j| |x_v| + |T_j|) + |tran|"""
    G, T = _chain(body, pose, F64)
    w = np.asarray(body["weights"], F64)
    x = np.asarray(body["v_template"], F64) - np.asarray(body["J"], F64)[:1]
    gn = np.linalg.norm(G, 2, axis=(-2, -1))                                 # [n,24]
    A = np.einsum("vj,nj->nv", w, gn) * np.linalg.norm(x, axis=1)[None] + np.einsum("vj,nj->nv", w, np.linalg.norm(T, axis=-1))
    if tran is not None:
        A = A + np.linalg.norm(np.asarray(tran, F64).reshape(-1, 3), axis=1)[:, None]
    return A


def mesh_f64(body, pose, tran=None):
    """All V vertices [n,V,3] in float64 and their magnitudes A [n,V]."""
    return _skin(body, pose, tran, F64), _vertex_A(body, pose, tran)


def mesh_f32(body, pose, tran, order):
    return _skin(body, pose, tran, F32, order)


def _keypoints(body, Jr, n_used, pose, vert, dtype, order):
    if Jr is None:                                                           # the 24 SMPL joints: P_j = T_j + G_j j_j
        G, T = _chain(body, pose, dtype)
        J = np.asarray(body["J"], F32).astype(dtype)
        return T + np.matmul(G, (J - J[:1])[None, :, :, None])[..., 0]
    Jr = np.asarray(Jr, F32)[:n_used].astype(dtype)
    if dtype == F64:
        return np.einsum("kv,nva->nka", Jr, vert)
    cols = np.nonzero(np.any(Jr != 0, axis=0))[0]                            # adding an exact zero changes nothing
    return _axis_sum(Jr[None, :, cols, None] * vert[:, None, cols, :], 2, order)


def _metrics(body, Jr, n_used, pose, gt, dtype, order="fwd", mut=None, tran=None):
    n = np.asarray(pose).reshape(-1, 24, 3, 3).shape[0]
    V = np.asarray(body["v_template"]).shape[0]
    tp = tran if mut == "tran_kept" else None
    vp = _skin(body, pose, tp, dtype, order, shift_row=(V - 1 if mut == "weight_row_shifted" else None))
    vt = _skin(body, gt, None, dtype, order)
    rows = None if Jr is None else (np.asarray(Jr).shape[0] if mut == "mpjpe_all_rows" else n_used)
    if mut == "fold_without_root" and Jr is not None:
        kp = _keypoints(body, Jr, rows, pose, _skin(body, pose, None, dtype, order, root_offset=False), dtype, order)
        kt = _keypoints(body, Jr, rows, gt, _skin(body, gt, None, dtype, order, root_offset=False), dtype, order)
    else:
        kp, kt = _keypoints(body, Jr, rows, pose, vp, dtype, order), _keypoints(body, Jr, rows, gt, vt, dtype, order)
    pel = 1 if (mut == "pelvis_kp1" and kp.shape[1] > 1) else 0
    pp, pt = kp[:, pel:pel + 1].copy(), kt[:, pel:pel + 1].copy()
    kp, kt = kp - pp, kt - pt                                                # evaluate.py:126-129
    if mut == "align_before_pve":
        vp, vt = vp - pp, vt - pt
    mp = _axis_sum(np.sqrt(((kt - kp) ** 2).sum(axis=2)), 1, order) / dtype(kp.shape[1])
    dv = np.sqrt(((vt - vp) ** 2).sum(axis=2))
    count = MET_SLAB * ((V + MET_SLAB - 1) // MET_SLAB) if mut == "pve_padded_count" else V
    pve = (dv.sum(axis=1) if dtype == F64 else _axis_sum(dv, 1, order)) / dtype(count)
    nk = n_used if Jr is not None else 24
    pa = procrustes(kp[:, :nk].astype(F32), kt[:, :nk].astype(F32))["mean"] if dtype == F32 else \
        np.array([np.sqrt((_align_one(kp[i, :nk], kt[i, :nk])[0] ** 2).sum(axis=1)).mean() for i in range(n)])
    out = np.stack([mp.astype(F64), pve.astype(F64), pa.astype(F64)], axis=1)
    if mut == "group_last_frame_repeated" and n > MET_FG:
        out[MET_FG::MET_FG] = out[MET_FG - 1:-1:MET_FG][:len(out[MET_FG::MET_FG])]
    return out


def frame_metrics_f64(body, Jr, n_used, pose, gt, mut=None, tran=None):
    """evaluate.py:120-133 in float64: (per-frame [n,3] = MPJPE, PVE, PA-MPJPE; A [n,3], the magnitudes of their bounds).
    Keypoints are Jr[:n_used] @ vertices, or the 24 joints when Jr is None; zero translation for both poses."""
    out = _metrics(body, Jr, n_used, pose, gt, F64, mut=mut, tran=tran)
    Ap, At = _vertex_A(body, pose), _vertex_A(body, gt)
    if Jr is None:
        G, T = _chain(body, pose, F64)
        G2, T2 = _chain(body, gt, F64)
        jn = np.linalg.norm(np.asarray(body["J"], F64) - np.asarray(body["J"], F64)[:1], axis=1)
        Ak = (np.linalg.norm(T, axis=-1) + jn[None]) + (np.linalg.norm(T2, axis=-1) + jn[None])
    else:
        Ak = np.einsum("kv,nv->nk", np.abs(np.asarray(Jr, F64)[:n_used]), Ap + At)
    Amp = (Ak + Ak[:, :1]).mean(axis=1)
    return out, np.stack([Amp, (Ap + At).mean(axis=1), Amp], axis=1)


def frame_metrics_f32(body, Jr, n_used, pose, gt, order):
    return _metrics(body, Jr, n_used, pose, gt, F32, order)


def bound(e32, A):
    """Bound = M max(e32, eps32 A), elementwise in A"""
    return M * np.maximum(e32, EPS32 * np.asarray(A, F64))


# ---------------------------------------------------------------------------------------------------- mesh cases
@dataclasses.dataclass
class MeshCase:
    name: str
    V: int
    reg: str                # "none", "convex", "onehot", "signed"
    n_used: int
    pose: np.ndarray        # [n,24,3,3] float32
    gt: np.ndarray
    tran: np.ndarray        # [n,3]: the API takes none (evaluate.py:120-133 zeroes it); only the mutation `tran_kept` reads it
    exact_zero: bool = False
    pa_zero: bool = False   # a rigid root rotation: PA <= Bound around 0


BODY_SEED = 1
N_FRAMES = 33
FRAME_COUNTS = (1, 15, 16, 17, 33)


def body_of(V):
    """the body of the shared fixtures (seed 1) with V vertices: the joints depend on the seed alone"""
    return synth.make_body(BODY_SEED, num_vertex=V)


def signed_regressor(seed, n_joint, num_vertex, support=48):
    """rows summing to 1 with entries in [-0.5, 1.5]: zero-sum weights of size <= 0.45 plus 1 / support each"""
    Jr = np.zeros((n_joint, num_vertex), F64)
    for k in range(n_joint):
        ids = (synth.uniform01(seed, 2 * k, support).astype(F64) * num_vertex).astype(np.int64) % num_vertex
        d = synth.uniform01(seed, 2 * k + 1, support).astype(F64) - 0.5
        d = d - d.mean()
        d = 0.45 * d / np.abs(d).max() + 1.0 / support
        np.add.at(Jr[k], ids, d)
    Jr = Jr.astype(F32)
    Jr[:, -1] += (1.0 - Jr.astype(F64).sum(axis=1)).astype(F32)              # the float32 rows sum to 1 within an ulp
    return Jr


def regressor_of(case):
    V = case.V
    if case.reg == "none":
        return None
    if case.reg == "convex":
        return synth.make_j_regressor(4, num_vertex=V)
    if case.reg == "signed":
        return signed_regressor(6, 17, V)
    Jr = np.zeros((17, V), F32)                                              # one-hot: slab edges and the last vertex among them
    ids = [0, 255, 256, 1022, V - 1] + [(k * 577 + 31) % V for k in range(12)]
    Jr[np.arange(17), np.asarray(ids) % V] = 1.0
    return Jr


def onehot_ids(case):
    return np.argmax(regressor_of(case), axis=1)


def _rodrigues32(aa):
    return synth._rodrigues(np.asarray(aa, F64)).astype(F32)


def build_mesh_cases(golden):
    """golden: the arrays of tests/golden/metrics.npz (pose_gt / pose_near / pose_far, 24 frames each). 33 frames per case:
    two full frame groups and one frame of a third; the vertex counts sit on both sides of a slab edge."""
    gt24, near24, far24 = (np.asarray(golden[k], F32) for k in ("pose_gt", "pose_near", "pose_far"))
    wrap = lambda a, b: np.concatenate([a, b[:N_FRAMES - 24]])
    gt, near, far = wrap(gt24, far24), wrap(near24, gt24), wrap(far24, near24)
    tran = (0.1 * synth.normal(7, 1, N_FRAMES * 3).reshape(N_FRAMES, 3) + 0.2).astype(F32)
    leaf = gt.copy()
    leaf[:, 22] = np.matmul(gt[:, 22], _rodrigues32(0.4 * synth.normal(8, 1, N_FRAMES * 3).reshape(N_FRAMES, 3)))
    rigid = gt.copy()
    rigid[:, 0] = np.matmul(_rodrigues32(0.8 * synth.normal(9, 1, N_FRAMES * 3).reshape(N_FRAMES, 3)), gt[:, 0])
    C = lambda *a, **k: MeshCase(*a, tran=tran, **k)
    return [
        C("near V=6890 convex14", 6890, "convex", 14, near, gt),
        C("far V=6890 convex14", 6890, "convex", 14, far, gt),
        C("far V=6890 joints24", 6890, "none", 24, far, gt),
        C("far V=6890 signed17", 6890, "signed", 17, far, gt),
        C("near V=1023 convex14", 1023, "convex", 14, near, gt),
        C("far V=1024 convex1", 1024, "convex", 1, far, gt),
        C("far V=1025 convex17", 1025, "convex", 17, far, gt),
        C("near V=1025 onehot17", 1025, "onehot", 17, near, gt),
        C("far V=2049 signed14", 2049, "signed", 14, far, gt),
        C("leaf joint 22 V=2049 convex14", 2049, "convex", 14, leaf, gt),
        C("rigid root rotation V=1025 convex14", 1025, "convex", 14, rigid, gt, pa_zero=True),
        C("rigid root rotation V=6890 joints24", 6890, "none", 24, rigid, gt, pa_zero=True),
        C("identical V=1025 convex14", 1025, "convex", 14, gt, gt, exact_zero=True),
        C("identical V=6890 joints24", 6890, "none", 24, far, far, exact_zero=True),
    ]


def evaluate_case(case):
    """float64 metrics, A, e32 per column and the three float32 evaluations of a case"""
    body, Jr = body_of(case.V), regressor_of(case)
    ref, A = frame_metrics_f64(body, Jr, case.n_used, case.pose, case.gt)
    f32 = {o: frame_metrics_f32(body, Jr, case.n_used, case.pose, case.gt, o) for o in ORDERS}
    e32 = np.max([np.abs(f32[o] - ref).max(axis=0) for o in ORDERS], axis=0)                # [3]
    return {"ref": ref, "A": A, "e32": e32, "f32": f32, "Bound": bound(e32[None, :], A)}


def evaluate_mesh(case, tran):
    """float64 vertices, A, e32 and the Bound [n,V] of forward_mesh on a case's prediction poses"""
    body = body_of(case.V)
    ref, A = mesh_f64(body, case.pose, tran)
    f32 = {o: mesh_f32(body, case.pose, tran, o) for o in ORDERS}
    e32 = max(float(np.abs(f32[o] - ref).max()) for o in ORDERS)
    return {"ref": ref, "A": A, "e32": e32, "f32": f32, "Bound": bound(e32, A)}
