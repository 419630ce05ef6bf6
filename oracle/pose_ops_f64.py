"""float64 restatements, cases and bounds of the pose-algebra and IMU-synthesis ops -- TEST INFRASTRUCTURE, NOT PRODUCT.

The drop-in ``ParametricModel`` / ``art.math`` surface (rc_ops.hip, the per-op kernels of rc_frame.hip, rc_preprocess.hip) against
the restatements of oracle/sig_mp_oracle.py run in float64 on the float32 inputs the device gets:
  r6d_to_rotation_matrix, axis_angle_to_rotation_matrix, rotation_matrix_to_axis_angle, rotation_angle_deg, normalize_keypoints,
  lerp_rows, reprojection_residual and OracleBody(dtype=float64) (IK_R, FK_R, bone FK, forward_kinematics + landmarks).
Beside them stands `Ops`: the same formulas written once more over a small arithmetic object (`Ar`: dtype, association order of
every sum of products, fused or separate multiply-add) with a `mut` switch for one-line wrong variants. `Ops(Ar(F64))` must agree
with the oracle's float64 to 1e-6 of the Bound (tests/test_pose_ops_bound_cpu.py); `Ops(Ar(F32, order, fma))` are the honest float32
evaluations a compiler could legally produce; `Ops(Ar(F64), mut=...)` are the mutations.

Bounds: Bound = M max(e32, eps32 A) per compared value.
  e32   |plain float32 evaluation of the oracle's own function - float64|, per item (its largest component)
  A     the op's magnitude / conditioning term:
          r6d          1 / sin(angle(a, b)): the Gram-Schmidt step divides by |b - (c0.b) c0| = |b| sin
          aa -> R      max(1, theta): cos / sin see theta's own rounding, eps32 theta
          angle        max(1, theta): the angle is 1-Lipschitz in the geodesic distance, R1^T R2 in float32 moves by a few eps32
          normalize    1 for the unit vector, |x| for the norm
          bbox         (|x| + |x_23|) / scale
          IK           sum_k |a_kr| |b_kc| of each entry's dot product
          FK rotations 1 + tree level: a product of orthonormal factors carries the error of each factor over unamplified
          bone FK      sum over the chain of |G_parent| |bone| (componentwise)
          joints       sum over the chain of (1 + level) |bone| + |tran|
          landmarks    sum_j w_j ((1 + level_j) (|x_v| + |j_j|) + A_joint_j) + |tran|   (an overridden row: its joint's A)
          residual     conf^2 (sum_xy gmof'(d) A_uv + 4 gmof) with A_uv = |K| (A_landmark / |z|) (1 + |q|) + sum |K q| + |kp|
          shaped body  sum_b |beta_b sd_b| + |v|;  joints sum_v |Jr_v| A_v
  M     per op (M_OF): the smallest power of two with which tests/test_pose_ops_bound_cpu.py holds -- every honest float32
        evaluation at most Bound / 3, every mutation at least 3 Bound. profiles/pose_ops_ratios.txt records the measured ratios.
R -> aa is float64 on both sides, rounded once to float32 on each: its bound is derived, 2^-22 absolute per component (one float32
ulp at magnitude pi), outside the window of `window_mask`: an oracle s in [0.5e-5, 2e-5] sits at the s < 1e-5 branch point, where
Newton's and the SVD's polar factors may fall on different sides and the two branches may return theta a and theta (-a); such a
case is compared as a rotation (geodesic angle <= 4e-5 rad) and the builder keeps at most WINDOW_MAX of them.
"""
import dataclasses
import math

import numpy as np
import torch

from robustcap_amd import config as C
from robustcap_amd import synth
from . import sig_mp_oracle as O

F32, F64 = torch.float32, torch.float64
EPS32 = 2.0 ** -24
MARGIN = 3.0
R2AA_BOUND = 2.0 ** -22
WINDOW = (0.5e-5, 2e-5)
WINDOW_MAX = 2
WINDOW_ANGLE = 4e-5
# M = 4 is the smallest power of two above MARGIN (a float32 evaluation that defines e32 sits at 1 / M). Measured on the CPU with
# M = 4, the worst honest float32 evaluation / Bound: r6d 0.41, angle 0.42 (the device's own route: float32 R1^T R2, float64 log,
# float32 norm), ik 0.35, bone_fk 0.34, norm 0.34 (65 squares summed one after the other), shape_j 0.31 -- above or at 1 / 3, so
# these six take M = 8; every other op stays below 0.28 with M = 4.
M_OF = {"r6d": 8.0, "aa2R": 4.0, "angle": 8.0, "normalize": 4.0, "norm": 8.0, "bbox": 4.0, "ik": 8.0, "fk_r": 4.0, "bone_fk": 8.0,
        "grot": 4.0, "joint": 4.0, "j33": 4.0, "residual": 4.0, "shape_v": 4.0, "shape_j": 8.0}
PI = math.pi


def t32(a):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.float32)))


def bound(op, e32, A):
    """Bound = M max(e32, eps32 A), elementwise (torch float64)"""
    e32, A = torch.as_tensor(e32, dtype=F64), torch.as_tensor(A, dtype=F64)
    return M_OF[op] * torch.maximum(e32, EPS32 * A)


def ratio(err, bnd):
    """|err| / bound with 0 / 0 = 0"""
    err, bnd = torch.as_tensor(err, dtype=F64).abs(), torch.as_tensor(bnd, dtype=F64)
    return torch.where(err == 0, torch.zeros_like(err), err / torch.where(bnd == 0, torch.full_like(bnd, 1e-300), bnd))


# ------------------------------------------------------------------------------------------------ the arithmetic
@dataclasses.dataclass(frozen=True)
class Ar:
    dtype: torch.dtype = F64
    order: str = "fwd"          # association of every sum of products: first term first, or last term first
    fma: bool = False           # acc = fma(x, y, acc) instead of acc + x * y (float32 only: the product is exact in float64)

    def fmadd(self, x, y, acc):
        if self.fma and self.dtype == F32:
            return (x.double() * y.double() + acc.double()).float()
        return acc + x * y

    def sp(self, pairs):
        """sum of the products x * y of `pairs`"""
        pairs = list(pairs)[::-1] if self.order == "rev" else list(pairs)
        acc = pairs[0][0] * pairs[0][1]
        for x, y in pairs[1:]:
            acc = self.fmadd(x, y, acc)
        return acc

    def dot(self, a, b):
        return self.sp([(a[..., k], b[..., k]) for k in range(a.shape[-1])])

    def mm(self, A, B):
        return self.sp([(A[..., :, k, None], B[..., None, k, :]) for k in range(3)])

    def mv(self, A, x):
        return self.sp([(A[..., :, k], x[..., None, k]) for k in range(3)])


VARIANTS = tuple(Ar(F32, o, f) for o in ("fwd", "rev") for f in (False, True))


def _cross(a, b):
    return torch.stack((a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]), dim=-1)


def _tree(body):
    parent = [0] + [int(p) for p in body["parent"]][1:]
    level = [0] * 24
    for i in range(1, 24):
        level[i] = level[parent[i]] + 1
    return parent, level


class Ops:
    """every value-compared op over one arithmetic; `mut` names a single wrong line"""

    def __init__(self, ar=Ar(), mut=None, body=None):
        self.ar, self.mut = ar, mut
        if body is not None:
            dt = ar.dtype
            self.parent, self.level = _tree(body)
            J = torch.as_tensor(body["J"], dtype=dt)
            self.j_rest = J - J[:1]
            self.bone = self.j_rest - self.j_rest[torch.tensor(self.parent)]
            ids = list(C.mp_mask)
            self.v_rest = (torch.as_tensor(body["v_template"], dtype=dt) - J[:1])[ids]
            self.w = torch.as_tensor(body["weights"], dtype=dt)[ids]
            self.override = sorted(C.mp_joint_override.items())

    def c(self, x):
        return torch.as_tensor(x).to(self.ar.dtype)

    # ---- art.math
    def r6d(self, x):
        ar, x = self.ar, self.c(x).reshape(-1, 6)
        a, b = x[:, :3], x[:, 3:]
        c0 = a / ar.dot(a, a).sqrt().unsqueeze(1)
        d = ar.dot(c0, b).unsqueeze(1)
        t = b if self.mut == "r6d_no_projection" else ar.fmadd(-d, c0, b)
        c1 = t / ar.dot(t, t).sqrt().unsqueeze(1)
        c2 = _cross(c1, c0) if self.mut == "r6d_cross_flipped" else _cross(c0, c1)
        r = torch.stack((c0, c1, c2), dim=-1)
        return torch.where(torch.isnan(r), torch.zeros_like(r), r)

    def aa2R(self, x):
        ar, a = self.ar, self.c(x).reshape(-1, 3)
        th = ar.dot(a, a).sqrt().unsqueeze(1)
        k = a / th
        k = torch.where(torch.isfinite(k), k, torch.zeros_like(k))
        c, s = th.cos().view(-1, 1, 1), th.sin().view(-1, 1, 1)
        if self.mut == "aa2R_sin_sign":
            s = -s
        z = torch.zeros_like(k[:, 0])
        K = torch.stack((z, -k[:, 2], k[:, 1], k[:, 2], z, -k[:, 0], -k[:, 1], k[:, 0], z), dim=1).view(-1, 3, 3)
        eye = torch.eye(3, dtype=a.dtype).expand(a.shape[0], 3, 3)
        R = ar.fmadd(s, K, ar.fmadd(1 - c, k.view(-1, 3, 1) * k.view(-1, 1, 3), c * eye))
        if self.mut == "aa2R_zero_gives_zeros":
            R = torch.where((th == 0).view(-1, 1, 1), torch.zeros_like(R), R)
        return R

    def angle(self, Ra, Rb):
        """the oracle's atan2 form in this arithmetic (radians)"""
        D = self.ar.mm(self.c(Ra).reshape(-1, 3, 3).transpose(1, 2), self.c(Rb).reshape(-1, 3, 3))
        v = torch.stack((D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]), dim=1) * 0.5
        cs = (D[:, 0, 0] + D[:, 1, 1] + D[:, 2, 2] - 1) * 0.5
        return torch.atan2(self.ar.dot(v, v).sqrt(), cs)

    def normalize(self, x):
        """(x / |x|, |x|) over the last dimension; the sum of squares in 64 strided partial sums like a wave, or in index order"""
        x = self.c(x)
        w = x.shape[-1]
        n_sum = min(w, 64) if self.mut == "normalize_first_64" else w
        sq = x[..., :n_sum] * x[..., :n_sum]
        if self.ar.order == "rev":
            sq = sq.flip(-1)
        ss = torch.cumsum(sq, dim=-1)[..., -1:] if self.ar.fma else sq.sum(dim=-1, keepdim=True)
        n = ss.sqrt()
        return x / n, n

    def bbox(self, kp):
        kp = self.c(kp).reshape(-1, 33, 3).clone()
        u, v = kp[..., 0], kp[..., 1]
        wd, ht = u.max(dim=-1).values - u.min(dim=-1).values, v.max(dim=-1).values - v.min(dim=-1).values
        sc = wd if self.mut == "bbox_width_only" else torch.maximum(wd, ht)
        xy = kp[..., :2] / sc.view(-1, 1, 1)
        row = 24 if self.mut == "bbox_row_24" else 23
        hip = xy[:, row:row + 1].clone()
        out = xy - hip
        out[:, row] = xy[:, row]
        return torch.cat((out, kp[..., 2:]), dim=-1)

    # ---- body
    def ik(self, Rg):
        Rg = self.c(Rg).reshape(-1, 24, 3, 3)
        Rp = Rg[:, torch.tensor(self.parent[1:])]
        loc = self.ar.mm(Rp if self.mut == "ik_no_transpose" else Rp.transpose(-1, -2), Rg[:, 1:])
        return torch.cat((Rg[:, :1], loc), dim=1)

    def _par(self, i):
        return max(i - 1, 0) if self.mut == "fk_parent_i_minus_1" else self.parent[i]

    def fk_r(self, Rl):
        Rl = self.c(Rl).reshape(-1, 24, 3, 3)
        G = [Rl[:, 0]]
        for i in range(1, 24):
            G.append(self.ar.mm(G[self._par(i)], Rl[:, i]))
        return torch.stack(G, dim=1)

    def bone_fk(self, Rg):
        Rg = self.c(Rg).reshape(-1, 24, 3, 3)
        P = [torch.zeros(Rg.shape[0], 3, dtype=Rg.dtype)]
        for i in range(1, 24):
            rot = Rg[:, i] if self.mut == "bone_fk_own_rotation" else Rg[:, self.parent[i]]
            P.append(P[self.parent[i]] + self.ar.mv(rot, self.bone[i].expand(Rg.shape[0], 3)))
        return torch.stack(P, dim=1)

    def body_fk(self, pose, tran):
        """(global rotations, joints, the 33 landmarks) of forward_kinematics(calc_mesh=True) + sync_mp3d"""
        ar = self.ar
        pose, tran = self.c(pose).reshape(-1, 24, 3, 3), self.c(tran).reshape(-1, 1, 3)
        n = pose.shape[0]
        G, P = [pose[:, 0]], [torch.zeros(n, 3, dtype=pose.dtype)]
        for i in range(1, 24):
            p = self._par(i)
            G.append(ar.mm(G[p], pose[:, i]))
            P.append(ar.mv(G[p], self.bone[i].expand(n, 3)) + P[p])
        G, P = torch.stack(G, dim=1), torch.stack(P, dim=1)
        T = P - ar.mv(G, self.j_rest.expand(n, 24, 3))
        A = torch.cat((G, T.unsqueeze(-1)), dim=-1)                                     # [n,24,3,4]
        Av = ar.sp([(self.w[None, :, j, None, None], A[:, None, j]) for j in range(24)])  # [n,33,3,4]
        v = ar.mv(Av[..., :3], self.v_rest.expand(n, 33, 3)) + Av[..., 3]
        joint, j33 = P + tran, v + tran
        if self.mut != "landmarks_no_override":
            j33 = j33.clone()
            for row, jid in self.override:
                j33[:, row] = joint[:, jid]
        return G, joint, j33

    def residual(self, pose, tran, kp, K, sigma, ignored=C.smplify_ignored_landmarks):
        ar = self.ar
        kp, K = self.c(kp).reshape(-1, 33, 3), self.c(K).reshape(3, 3)
        j33 = self.body_fk(pose, tran)[2]
        q = j33 / j33[..., 2:]
        uv = ar.mv(K.expand(q.shape[0], 33, 3, 3), q)[..., :2]
        conf = kp[..., 2].clone()
        if self.mut != "residual_no_ignore":
            conf[:, list(ignored)] = 0.0
        s = torch.tensor(sigma, dtype=F32).to(ar.dtype)
        s2 = s if self.mut == "residual_sigma_not_squared" else s * s
        d2 = (uv - kp[..., :2]) ** 2
        return conf * conf * ((s2 * d2) / (s2 + d2)).sum(dim=-1)

    def shape(self, body, beta):
        """(v [V,3], J [24,3]) of the shaped body before the root alignment"""
        ar = self.ar
        sd, vt, Jr, beta = self.c(body["shapedirs"])[:, :, :10], self.c(body["v_template"]), self.c(body["J_regressor"]), self.c(beta)
        v = ar.sp([(beta[b], sd[:, :, b]) for b in range(10)]) + vt
        if ar.dtype == F64 or not ar.fma:
            j = Jr @ v if ar.order == "fwd" else (Jr.flip(1) @ v.flip(0))
        else:
            j = torch.cumsum(Jr.t()[:, :, None] * v[:, None, :], dim=0)[-1]
        return v, j


def syn_acc_f64(v, n, mut=None):
    """the stencil of rc_syn_acc_kernel's comment in float64 (only the mutation test uses it: the device is compared bitwise)"""
    v = torch.as_tensor(v).double()
    acc = torch.zeros_like(v)
    acc[1:-1] = ((v[:-2] + v[2:]) - 2.0 * v[1:-1]) * 3600.0
    if n // 2 != 0:
        acc[n:-n] = (((v[:-2 * n] + v[2 * n:]) - 2.0 * v[n:-n]) * 3600.0) / float(n if mut == "syn_acc_div_n" else n * n)
    return acc


# ------------------------------------------------------------------------------------------- R -> aa (float64 both)
def r2aa_newton(R, mut=None):
    """rotmat_to_aa of csrc/rc_device.h line for line in float64 numpy, rounded once to float32. [n,3,3] float32 -> [n,3]"""
    Rn = np.asarray(R, np.float32).reshape(-1, 3, 3).astype(np.float64)
    out = np.zeros((Rn.shape[0], 3), np.float32)
    for i, Q in enumerate(Rn):
        if not np.all(np.abs(Q) < 100.0):                                               # NaN fails the compare
            continue
        Q, singular = Q.copy(), False
        for _ in range(0 if mut == "r2aa_no_polar" else 24):
            Cf = np.array([[Q[1, 1] * Q[2, 2] - Q[1, 2] * Q[2, 1], Q[1, 2] * Q[2, 0] - Q[1, 0] * Q[2, 2], Q[1, 0] * Q[2, 1] - Q[1, 1] * Q[2, 0]],
                           [Q[0, 2] * Q[2, 1] - Q[0, 1] * Q[2, 2], Q[0, 0] * Q[2, 2] - Q[0, 2] * Q[2, 0], Q[0, 1] * Q[2, 0] - Q[0, 0] * Q[2, 1]],
                           [Q[0, 1] * Q[1, 2] - Q[0, 2] * Q[1, 1], Q[0, 2] * Q[1, 0] - Q[0, 0] * Q[1, 2], Q[0, 0] * Q[1, 1] - Q[0, 1] * Q[1, 0]]])
            det = Q[0, 0] * Cf[0, 0] + Q[0, 1] * Cf[0, 1] + Q[0, 2] * Cf[0, 2]
            if not abs(det) > 1e-300:
                singular = True
                break
            g = math.sqrt(math.sqrt((Cf * Cf).sum()) / (abs(det) * math.sqrt((Q * Q).sum())))
            Qn = 0.5 * (g * Q + Cf / (det * g))
            delta = np.abs(Qn - Q).max()
            Q = Qn
            if delta < 1e-15:
                break
        if singular:
            continue
        r = np.array([Q[2, 1] - Q[1, 2], Q[0, 2] - Q[2, 0], Q[1, 0] - Q[0, 1]])
        s = math.sqrt((r * r).sum() * 0.25)
        c = min(1.0, max(-1.0, (Q[0, 0] + Q[1, 1] + Q[2, 2] - 1.0) * 0.5))
        theta = math.acos(c)
        if s < 1e-5:
            if c > 0.0 and mut != "r2aa_no_c_exit":
                continue
            r = np.array([math.sqrt(max((Q[0, 0] + 1.0) * 0.5, 0.0)),
                          math.sqrt(max((Q[1, 1] + 1.0) * 0.5, 0.0)) * (-1.0 if Q[0, 1] < 0.0 else 1.0),
                          math.sqrt(max((Q[2, 2] + 1.0) * 0.5, 0.0)) * (-1.0 if Q[0, 2] < 0.0 else 1.0)])
            if mut != "r2aa_no_fixup" and abs(r[0]) < abs(r[1]) and abs(r[0]) < abs(r[2]) and ((Q[1, 2] > 0.0) != (r[1] * r[2] > 0.0)):
                r[2] = -r[2]
            n = math.sqrt((r * r).sum())
            if not n > 0.0:
                continue
            out[i] = (r * (theta / n)).astype(np.float32)
        else:
            out[i] = (r * (theta / (2.0 * s))).astype(np.float32)
    return out


def oracle_s(R):
    """s = |vee(Q - Q^T)| / 2 of the oracle's SVD polar factor Q (NaN where the range check fails)"""
    Rn = np.asarray(R, np.float32).reshape(-1, 3, 3).astype(np.float64)
    s = np.full(Rn.shape[0], np.nan)
    ok = np.all(np.isfinite(Rn) & (np.abs(Rn) < 100.0), axis=(1, 2))
    if ok.any():
        U, _, Vt = np.linalg.svd(Rn[ok])
        Q = U @ Vt
        r = np.stack((Q[:, 2, 1] - Q[:, 1, 2], Q[:, 0, 2] - Q[:, 2, 0], Q[:, 1, 0] - Q[:, 0, 1]), axis=1)
        s[ok] = np.sqrt((r * r).sum(1) * 0.25)
    return s


def window_mask(R):
    s = oracle_s(R)
    return (s >= WINDOW[0]) & (s <= WINDOW[1])


def r2aa_errors(got, R):
    """(error / bound [n], in-window mask): 2^-22 per component against the oracle; inside the window the geodesic angle between
    the two vectors' rotations against WINDOW_ANGLE"""
    got = np.asarray(got, np.float64).reshape(-1, 3)
    ref = O.rotation_matrix_to_axis_angle(t32(R)).numpy().astype(np.float64)
    win = window_mask(R)
    r = np.abs(got - ref).max(axis=1) / R2AA_BOUND
    if win.any():
        Ra = O.axis_angle_to_rotation_matrix(torch.from_numpy(got[win]))
        Rb = O.axis_angle_to_rotation_matrix(torch.from_numpy(ref[win]))
        r[win] = torch.deg2rad(O.rotation_angle_deg(Ra, Rb)).numpy() / WINDOW_ANGLE
    return np.where(np.isfinite(r), r, np.inf), win


# ------------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass
class Cases:
    names: list
    x: tuple                    # float32 numpy arrays, one row per case

    def __len__(self):
        return len(self.names)

    def pick(self, words):
        idx = [i for i, nm in enumerate(self.names) if any(w in nm for w in ([words] if isinstance(words, str) else words))]
        return Cases([self.names[i] for i in idx], tuple(a[idx] for a in self.x))


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _rodrigues(aa):
    return synth._rodrigues(np.asarray(aa, np.float64))


def _rand_rot(seed, stream, n):
    """n seeded rotations (float64) with angles spread over (0, pi)"""
    ax = _unit(synth.normal(seed, stream, 3 * n).reshape(n, 3))
    th = (0.01 + 3.09 * synth.uniform01(seed, stream + 50, n).astype(np.float64))[:, None]
    return _rodrigues(ax * th), ax, th[:, 0]


R6D_ANGLES = (1e-3, 1e-2, PI / 2, PI - 1e-2)
R6D_DEGENERATE = ("a = 0", "b = 0", "b = 1 a", "b = -2 a")


def r6d_cases():
    names, rows = [], []
    for i in range(12):                                                               # generic, |a| |b| log-uniform in [1e-3, 1e3]
        v = _unit(synth.normal(21, i, 6).reshape(2, 3)) * 10.0 ** (6.0 * synth.uniform01(21, 100 + i, 2).astype(np.float64)[:, None] - 3.0)
        names.append(f"generic {i} |a|={np.linalg.norm(v[0]):.1e} |b|={np.linalg.norm(v[1]):.1e}")
        rows.append(v.reshape(6))
    for i, ang in enumerate(R6D_ANGLES):
        for j, (la, lb) in enumerate(((1.0, 1.0), (30.0, 0.02))):
            a = _unit(synth.normal(22, 2 * i + j, 3))
            p = _unit(np.cross(a, synth.normal(22, 40 + 2 * i + j, 3)))
            names.append(f"angle {ang:.4g} |a|={la:g} |b|={lb:g}")
            rows.append(np.concatenate([la * a, lb * (math.cos(ang) * a + math.sin(ang) * p)]))
    names.append("orthonormal axes")
    rows.append(np.array([0, 0, 1, 1, 0, 0], np.float64))
    a = _unit(synth.normal(23, 0, 3))
    names.append("b orthogonal to unit a")
    rows.append(np.concatenate([a, 0.7 * _unit(np.cross(a, synth.normal(23, 1, 3)))]))
    # b = k a: a along a coordinate axis, so that c0, c0.b and b - (c0.b) c0 = 0 are exact in every arithmetic and the second
    # column is 0 / 0 everywhere; for another a the remainder is rounding noise and its zero pattern is nobody's to define
    a, e = synth.normal(24, 0, 3).astype(np.float64), np.array([0.0, 2.0, 0.0])
    for nm, row in zip(R6D_DEGENERATE, (np.concatenate([0 * a, a]), np.concatenate([a, 0 * a]), np.concatenate([e, e]), np.concatenate([e, -2 * e]))):
        names.append("degenerate " + nm)
        rows.append(row)
    return Cases(names, (np.stack(rows).astype(np.float32),))


def r6d_A(x):
    x = torch.as_tensor(x).double().reshape(-1, 6)
    a, b = x[:, :3], x[:, 3:]
    sin = torch.linalg.cross(a, b, dim=1).norm(dim=1) / (a.norm(dim=1) * b.norm(dim=1))
    return 1.0 / sin


AA_THETAS = (0.0, 1e-30, 1e-4, 1.0, PI - 1e-3, PI, 2 * PI, 10 * PI)
AA_AXES = (("-y", (0.0, -1.0, 0.0)), ("(1,1,0)/sqrt2", (1.0, 1.0, 0.0)), ("generic", (0.3, -0.5, 0.81)))


def aa_cases():
    names, rows = [], []
    for th in AA_THETAS:
        for nm, ax in AA_AXES:
            names.append(f"theta {th:.6g} axis {nm}")
            rows.append(_unit(ax) * th)
    return Cases(names, (np.stack(rows).astype(np.float32),))


def aa_A(x):
    return torch.as_tensor(x).double().reshape(-1, 3).norm(dim=1).clamp(min=1.0)


HALF_TURN_AXES = (("+x", (1, 0, 0)), ("-x", (-1, 0, 0)), ("+y", (0, 1, 0)), ("-y", (0, -1, 0)), ("+z", (0, 0, 1)), ("-z", (0, 0, -1)),
                  ("(1,1,0)/sqrt2", (1, 1, 0)), ("(1,-1,0)/sqrt2", (1, -1, 0)), ("(0,1,-1)/sqrt2", (0, 1, -1)),
                  ("(1,1,1)/sqrt3", (1, 1, 1)), ("(-1,2,3)/sqrt14", (-1, 2, 3)),
                  ("r_x smallest R12 > 0: (0,0.6,0.8)", (0, 0.6, 0.8)), ("r_x smallest R12 < 0: (0,0.6,-0.8)", (0, 0.6, -0.8)),
                  ("r_x smallest R12 > 0: (0.1,0.7,0.7)", (0.1, 0.7, 0.7)), ("r_x smallest R12 < 0: (0.1,-0.7,0.7)", (0.1, -0.7, 0.7)))
NEAR_PI = (1e-3, 1e-4, 4e-5, 5e-6, 1e-6)


def r2aa_cases():
    names, mats = ["identity"], [np.eye(3)]
    for th in (1e-6, 4e-6, 1e-4):                                                      # s < 1e-5 and c > 0: zero; 1e-4 is past it
        names.append(f"theta {th:g} (c > 0 exit)" if th < 1e-5 else f"theta {th:g}")
        mats.append(_rodrigues(_unit((0.3, -0.5, 0.81)) * th))
    Rg, _, th = _rand_rot(31, 0, 12)
    for i in range(12):
        names.append(f"generic {i} theta {th[i]:.3f}")
        mats.append(Rg[i])
    for i, d in enumerate(NEAR_PI):
        names.append(f"theta pi - {d:g}")
        mats.append(_rodrigues(_unit(synth.normal(32, i, 3)) * (PI - d)))
    for nm, ax in HALF_TURN_AXES:
        a = _unit(ax)
        names.append(f"half-turn {nm}")
        mats.append(2.0 * np.outer(a, a) - np.eye(3))
    Rp, _, _ = _rand_rot(33, 0, 2)
    names.append("perturbed entrywise by 1e-4")
    mats.append(Rp[0] + 1e-4 * synth.normal(33, 9, 9).reshape(3, 3))
    names.append("1.01 R")
    mats.append(1.01 * Rp[1])
    names.append("improper diag(1,1,-1)")
    mats.append(np.diag([1.0, 1.0, -1.0]))
    big = Rg[0].copy()
    big[1, 2] = 100.0
    nan = Rg[1].copy()
    nan[2, 0] = np.nan
    for nm, m in (("entry 100", big), ("entry NaN", nan), ("zero matrix", np.zeros((3, 3)))):
        names.append(nm + " (zero vector)")
        mats.append(m)
    return Cases(names, (np.stack(mats).astype(np.float32),))


ANGLES_BETWEEN = (1e-3, PI / 2, PI - 1e-3, PI)


def angle_cases():
    names, A, B = [], [], []
    base, _, _ = _rand_rot(41, 0, 16)
    names.append("identical")
    A.append(base[0]); B.append(base[0])
    for i, th in enumerate(ANGLES_BETWEEN):
        names.append(f"angle {th:.6g}")
        A.append(base[1 + i]); B.append(base[1 + i] @ _rodrigues(_unit(synth.normal(42, i, 3)) * th))
    for i in range(8):
        names.append(f"generic {i}")
        A.append(base[6 + i]); B.append(base[15 - i] if i != 4 else base[5])
    return Cases(names, (np.stack(A).astype(np.float32), np.stack(B).astype(np.float32)))


NORMALIZE_WIDTHS = (1, 3, 7, 63, 64, 65, 129)
NORMALIZE_ROWS = (1, 3)


def normalize_cases():
    """list of (name, x [rows, width] float32); the three-row sets have a zero middle row"""
    out = []
    for w in NORMALIZE_WIDTHS:
        for rows in NORMALIZE_ROWS:
            mag = 10.0 ** (6.0 * synth.uniform01(51, 1000 * rows + w, rows * w).astype(np.float64) - 3.0)
            sgn = np.where(synth.uniform01(51, 2000 * rows + w, rows * w) < 0.5, -1.0, 1.0)
            x = (mag * sgn).reshape(rows, w).astype(np.float32)
            if rows == 3:
                x[1] = 0.0
            out.append((f"width {w} rows {rows}" + (" (row 1 zero)" if rows == 3 else ""), x))
    return out


def bbox_cases():
    names, rows = [], []

    def frame(seed, sx, sy, off=(0.0, 0.0)):
        xy = (synth.uniform01(seed, 1, 66).astype(np.float64).reshape(33, 2) - 0.5) * np.array([sx, sy]) + np.asarray(off)
        cf = synth.uniform01(seed, 2, 33).astype(np.float64)
        return np.concatenate([xy, cf[:, None]], axis=1)
    names.append("wide box"); rows.append(frame(61, 4.0, 0.5))
    names.append("tall box"); rows.append(frame(62, 0.3, 2.5))
    for nm, col, sgn in (("row 23 max x", 0, 1.0), ("row 23 min x", 0, -1.0), ("row 23 max y", 1, 1.0), ("row 23 min y", 1, -1.0)):
        f = frame(63 + len(names), 1.0, 1.0)
        f[23, col] = sgn * 0.9
        names.append(nm); rows.append(f)
    names.append("negative coordinates"); rows.append(frame(69, 300.0, 500.0, off=(-900.0, -700.0)))
    f = frame(70, 1.0, 1.0)
    f[:, 0], f[:, 1] = 0.37, -1.25
    names.append("all 33 points equal"); rows.append(f)
    return Cases(names, (np.stack(rows).astype(np.float32),))


def bbox_A(kp):
    kp = torch.as_tensor(kp).double().reshape(-1, 33, 3)
    sc = O.bbox_scale(kp).view(-1, 1, 1)
    xy = kp[..., :2].abs()
    A = (xy + xy[:, 23:24]) / sc
    A[:, 23] = xy[:, 23] / sc[:, 0]
    return A


BODY_SEED = 1


def body_of():
    return synth.make_body(BODY_SEED)


def pose_cases():
    """local rotations [n,24,3,3] + translations [n,3]"""
    names, poses, trans = [], [], []
    eye = np.broadcast_to(np.eye(3), (24, 3, 3)).copy()
    small = 0.2 * synth.normal(71, 9, 3).astype(np.float64)
    names.append("identity pose"); poses.append(eye); trans.append(np.zeros(3))
    for i in range(3):
        aa = _unit(synth.normal(71, i, 72).reshape(24, 3)) * (PI * synth.uniform01(71, 10 + i, 24).astype(np.float64))[:, None]
        names.append(f"random pose {i} (joints up to pi)"); poses.append(_rodrigues(aa)); trans.append(small * (i + 1))
    leaf = eye.copy()
    leaf[22] = _rodrigues(np.array([0.4, -1.1, 0.7]))
    names.append("leaf joint 22 rotated"); poses.append(leaf); trans.append(small)
    rigid = eye.copy()
    rigid[0] = _rodrigues(np.array([1.2, 0.4, -2.0]))
    names.append("rigid root rotation"); poses.append(rigid); trans.append(-small)
    aa = 0.5 * synth.normal(72, 0, 72).reshape(24, 3).astype(np.float64)
    names.append("translation of 100 m"); poses.append(_rodrigues(aa)); trans.append(np.array([100.0, -100.0, 50.0]))
    return Cases(names, (np.stack(poses).astype(np.float32), np.stack(trans).astype(np.float32)))


CAM_K = np.array([[1.2, 0.0, 0.05], [0.0, 1.1, -0.03], [0.0, 0.0, 1.0]], np.float32)
SIGMA = 100.0
SIGMA_SMALL = 0.01


def residual_cases(body):
    """(Cases(pose, tran, kp), sigma per case): every pose in front of (z ~ +4) and behind (z ~ -4) the camera; keypoints near the
    projection (residual far below sigma = 100) or a plain offset judged against sigma = 0.01 (far above); confidence 0 rows"""
    pc = pose_cases()
    ob = Ops(Ar(F64), body=body)
    names, P, T, KP, sig = [], [], [], [], []
    for i, nm in enumerate(pc.names):
        for side, z in (("front", 4.0), ("behind", -4.0)):
            tran = pc.x[1][i].astype(np.float64) + np.array([0.1, -0.2, z])
            if abs(pc.x[1][i][2]) > 10:
                tran = pc.x[1][i].astype(np.float64) * (1.0 if z > 0 else -1.0)
            j33 = ob.body_fk(t32(pc.x[0][i:i + 1]), t32(tran[None]))[2][0].numpy()
            uv = (j33 / j33[:, 2:]) @ CAM_K.astype(np.float64).T
            small = (i + (z < 0)) % 2 == 0
            noise = synth.normal(81, 2 * i + (z < 0), 66).reshape(33, 2).astype(np.float64) * (0.02 if small else 0.5)
            cf = 0.2 + 0.8 * synth.uniform01(81, 100 + 2 * i + (z < 0), 33).astype(np.float64)
            cf[[3, 17]] = 0.0
            names.append(f"{nm}, {side}, residual {'far below sigma 100' if small else 'far above sigma 0.01'}")
            P.append(pc.x[0][i]); T.append(tran); KP.append(np.concatenate([uv[:, :2] + noise, cf[:, None]], axis=1))
            sig.append(SIGMA if small else SIGMA_SMALL)
    return Cases(names, (np.stack(P).astype(np.float32), np.stack(T).astype(np.float32), np.stack(KP).astype(np.float32))), sig


def beta_cases():
    names, rows = ["beta = 0"], [np.zeros(10)]
    for k in (0, 4, 9):
        e = np.zeros(10)
        e[k] = 1.0
        names.append(f"one-hot beta {k}"); rows.append(e)
    names.append("random beta in [-5, 5]"); rows.append(10.0 * synth.uniform01(91, 0, 10).astype(np.float64) - 5.0)
    return Cases(names, (np.stack(rows).astype(np.float32),))


# ------------------------------------------------------------------------------------- magnitudes of the body ops
def ik_A(body, Rg):
    par, _ = _tree(body)
    Rg = torch.as_tensor(Rg).double().reshape(-1, 24, 3, 3).abs()
    A = torch.ones_like(Rg)
    A[:, 1:] = Rg[:, torch.tensor(par[1:])].transpose(-1, -2) @ Rg[:, 1:]
    return A


def level_A(body):
    return 1.0 + torch.tensor(_tree(body)[1], dtype=F64)                                # [24]


def bone_fk_A(body, Rg):
    ob = Ops(Ar(F64), body=body)
    Rg = torch.as_tensor(Rg).double().reshape(-1, 24, 3, 3).abs()
    A = [torch.zeros(Rg.shape[0], 3, dtype=F64)]
    for i in range(1, 24):
        A.append(A[ob.parent[i]] + (Rg[:, ob.parent[i]] @ ob.bone[i].abs().view(1, 3, 1)).squeeze(-1))
    return torch.stack(A, dim=1).clamp(min=1e-3)


def body_fk_A(body, pose, tran):
    """(A_grot [24], A_joint [n,24], A_j33 [n,33]) -- norms, applied to every component"""
    ob = Ops(Ar(F64), body=body)
    lv = level_A(body)
    tn = torch.as_tensor(tran).double().reshape(-1, 3).norm(dim=1)
    bn = ob.bone.norm(dim=1)
    Aj = [torch.zeros((), dtype=F64)]
    for i in range(1, 24):
        Aj.append(Aj[ob.parent[i]] + lv[i] * bn[i])
    Aj = torch.stack(Aj)                                                                # [24]
    per_joint = lv[None, :] * (ob.v_rest.norm(dim=1)[:, None] + ob.j_rest.norm(dim=1)[None, :]) + Aj[None, :]   # [33,24]
    Av = (ob.w * per_joint).sum(dim=1)
    for row, jid in ob.override:
        Av[row] = Aj[jid]
    floor = 1e-2                                                                        # the root joint itself: |j| = 0
    return lv, (Aj.clamp(min=floor)[None] + tn[:, None]), (Av.clamp(min=floor)[None] + tn[:, None])


def residual_A(body, pose, tran, kp, K, sigma):
    ob = Ops(Ar(F64), body=body)
    kp, K = torch.as_tensor(kp).double().reshape(-1, 33, 3), torch.as_tensor(K).double().reshape(3, 3)
    j33 = ob.body_fk(pose, tran)[2]
    A33 = body_fk_A(body, pose, tran)[2]
    z = j33[..., 2].abs()
    q = j33 / j33[..., 2:]
    Aq = (A33 / z)[..., None] * (1.0 + q.abs())
    Auv = ((K.abs()[None, None] * (Aq + q.abs())[:, :, None, :]).sum(-1))[..., :2] + kp[..., :2].abs()
    d = (K[None, None] * q[:, :, None, :]).sum(-1)[..., :2] - kp[..., :2]
    s2 = float(np.float32(sigma)) ** 2
    g = s2 * d * d / (s2 + d * d)
    gp = 2.0 * s2 * s2 * d.abs() / (s2 + d * d) ** 2
    return kp[..., 2] ** 2 * ((gp * Auv).sum(-1) + 4.0 * g.sum(-1))


def shape_A(body, beta):
    sd, vt, Jr = (torch.as_tensor(body[k]).double() for k in ("shapedirs", "v_template", "J_regressor"))
    Av = (sd[:, :, :10].abs() * torch.as_tensor(beta).double().abs()).sum(-1) + vt.abs()
    return Av, Jr.abs() @ Av


# ------------------------------------------------------------------------ reference + Bound of every value-compared op
def _item_max(e, keep):
    """largest |e| of each item over the dimensions after `keep`, broadcastable back"""
    e = e.abs().double()
    flat = e.reshape(e.shape[:keep] + (-1,)).max(dim=-1).values
    return flat.reshape(flat.shape + (1,) * (e.dim() - keep))


def _nan0(x):
    return torch.where(torch.isnan(x), torch.zeros_like(x), x)


def ev_r6d(x):
    x = t32(x)
    ref = O.r6d_to_rotation_matrix(x.double())
    e32 = _item_max(O.r6d_to_rotation_matrix(x).double() - ref, 1)
    return ref, bound("r6d", e32, r6d_A(x).view(-1, 1, 1))


def ev_aa2R(x):
    x = t32(x)
    ref = O.axis_angle_to_rotation_matrix(x.double())
    e32 = _item_max(O.axis_angle_to_rotation_matrix(x).double() - ref, 1)
    return ref, bound("aa2R", e32, aa_A(x).view(-1, 1, 1))


def ev_angle(Ra, Rb):
    """the oracle's float64 angle in radians; e32 from the same atan2 form in float32"""
    Ra, Rb = t32(Ra), t32(Rb)
    ref = torch.deg2rad(O.rotation_angle_deg(Ra, Rb))
    e32 = (Ops(Ar(F32)).angle(Ra, Rb).double() - ref).abs()
    return ref, bound("angle", e32, ref.clamp(min=1.0))


def ev_normalize(x):
    x = t32(x)
    with np.errstate(all="ignore"):
        ref, refn = Ops(Ar(F64)).normalize(x)
        p, pn = x / x.norm(dim=-1, keepdim=True), x.norm(dim=-1, keepdim=True)
    e32 = _item_max(_nan0(p.double() - ref), x.dim() - 1)
    return (ref, bound("normalize", e32, torch.ones_like(ref))), (refn, bound("norm", (pn.double() - refn).abs(), refn))


def ev_bbox(kp):
    kp = t32(kp).reshape(-1, 33, 3)
    ref = O.normalize_keypoints(kp.double())
    p32 = O.normalize_keypoints(kp)
    e32 = _item_max(_nan0(p32.double()[..., :2] - ref[..., :2]), 1)
    return ref, bound("bbox", e32, _nan0(bbox_A(kp))), p32


def ev_ik(body, Rg):
    Rg = t32(Rg)
    ref = O.OracleBody(body, dtype=F64).inverse_kinematics_R(Rg.double())
    e32 = _item_max(O.OracleBody(body).inverse_kinematics_R(Rg).double() - ref, 1)
    return ref, bound("ik", e32, ik_A(body, Rg))


def ev_fk_r(body, Rl):
    Rl = t32(Rl)
    ref = O.OracleBody(body, dtype=F64).forward_kinematics_R(Rl.double())
    e32 = _item_max(O.OracleBody(body).forward_kinematics_R(Rl).double() - ref, 1)
    return ref, bound("fk_r", e32, level_A(body).view(1, 24, 1, 1))


def ev_bone_fk(body, Rg):
    Rg = t32(Rg)
    ob64 = O.OracleBody(body, dtype=F64)
    Rd = Rg.double().reshape(-1, 24, 3, 3)
    pb = (Rd[:, ob64.par[1:]] @ ob64.bone[1:].view(1, 23, 3, 1)).squeeze(-1)        # OracleBody.bone_fk with a float64 zero root
    ref = ob64.bone_to_joint(torch.cat((torch.zeros(Rd.shape[0], 1, 3, dtype=F64), pb), dim=1))
    e32 = _item_max(O.OracleBody(body).bone_fk(Rg).double() - ref, 1)
    return ref, bound("bone_fk", e32, bone_fk_A(body, Rg))


def ev_body_fk(body, pose, tran):
    """((grot, Bound), (joint, Bound), (j33, Bound)) of forward_kinematics(calc_mesh=True) + landmarks"""
    pose, tran = t32(pose), t32(tran)
    o64, o32 = O.OracleBody(body, dtype=F64), O.OracleBody(body)
    G, J, V = o64.forward_kinematics(pose.double(), tran.double())
    L = o64.landmarks(V, J)
    g, j, v = o32.forward_kinematics(pose, tran)
    l = o32.landmarks(v, j)
    Ag, Aj, Al = body_fk_A(body, pose, tran)
    return ((G, bound("grot", _item_max(g.double() - G, 1), Ag.view(1, 24, 1, 1))),
            (J, bound("joint", _item_max(j.double() - J, 1), Aj[..., None])),
            (L, bound("j33", _item_max(l.double() - L, 1), Al[..., None])))


def ev_residual(body, pose, tran, kp, K, sigma):
    pose, tran, kp, K = t32(pose), t32(tran), t32(kp), t32(K)
    s = float(np.float32(sigma))
    ref = O.reprojection_residual(O.OracleBody(body, dtype=F64), pose.double(), tran.double(), kp.double(), K.double(), s)
    p32 = O.reprojection_residual(O.OracleBody(body), pose, tran, kp, K, s)
    return ref, bound("residual", _item_max(p32.double() - ref, 1), residual_A(body, pose, tran, kp, K, sigma))


def ev_shape(body, beta):
    ref_v, ref_j = Ops(Ar(F64)).shape(body, beta)
    v32, j32 = Ops(Ar(F32)).shape(body, beta)
    Av, Aj = shape_A(body, beta)
    return ((ref_v, bound("shape_v", float((v32.double() - ref_v).abs().max()), Av)),
            (ref_j, bound("shape_j", float((j32.double() - ref_j).abs().max()), Aj)))


# ------------------------------------------------------------------------------------------- the value suite
@dataclasses.dataclass
class Entry:
    op: str                     # key of M_OF and of the ratios record
    fn: str                     # the function that produces it (Ops method / device call)
    out: object                 # index into that function's outputs, or None
    names: list                 # one name per leading row of ref
    args: tuple                 # float32 numpy inputs
    ref: torch.Tensor           # float64
    bound: torch.Tensor         # broadcastable to ref
    extra: object = None        # sigma / beta-independent data the call needs


def suite(body):
    """every value-compared (op, cases, float64 reference, Bound) of the issue's section 1"""
    S = []
    c = r6d_cases().pick(["generic", "angle", "ortho"])
    S.append(Entry("r6d", "r6d", None, c.names, c.x, *ev_r6d(c.x[0])))
    c = aa_cases()
    S.append(Entry("aa2R", "aa2R", None, c.names, c.x, *ev_aa2R(c.x[0])))
    c = angle_cases()
    S.append(Entry("angle", "angle", None, c.names, c.x, *ev_angle(*c.x)))
    for nm, x in normalize_cases():
        (ref, B), (refn, Bn) = ev_normalize(x)
        S.append(Entry("normalize", "normalize", 0, [nm] * x.shape[0], (x,), ref, B))
        S.append(Entry("norm", "normalize", 1, [nm] * x.shape[0], (x,), refn, Bn))
    c = bbox_cases()
    ref, B, _ = ev_bbox(c.x[0])
    S.append(Entry("bbox", "bbox", None, c.names, c.x, ref, torch.cat((B, torch.zeros_like(B[..., :1])), dim=-1)))   # confidence: exact
    pc = pose_cases()
    pose, tran = pc.x
    Rg = Ops(Ar(F64), body=body).fk_r(pose).float().numpy()                             # global rotations of the same poses
    S.append(Entry("ik", "ik", None, pc.names, (Rg,), *ev_ik(body, Rg)))
    S.append(Entry("fk_r", "fk_r", None, pc.names, (pose,), *ev_fk_r(body, pose)))
    S.append(Entry("bone_fk", "bone_fk", None, pc.names, (Rg,), *ev_bone_fk(body, Rg)))
    for i, (op, (ref, B)) in enumerate(zip(("grot", "joint", "j33"), ev_body_fk(body, pose, tran))):
        S.append(Entry(op, "body_fk", i, pc.names, (pose, tran), ref, B))
    rc, sig = residual_cases(body)
    for sg in (SIGMA, SIGMA_SMALL):
        idx = [i for i, s in enumerate(sig) if s == sg]
        xs = tuple(a[idx] for a in rc.x)
        S.append(Entry("residual", "residual", None, [rc.names[i] for i in idx], xs, *ev_residual(body, *xs, CAM_K, sg), extra=sg))
    bc = beta_cases()
    for nm, b in zip(bc.names, bc.x[0]):
        (rv, Bv), (rj, Bj) = ev_shape(body, b)
        S.append(Entry("shape_v", "shape", 0, [nm], (b,), rv[None], Bv[None]))
        S.append(Entry("shape_j", "shape", 1, [nm], (b,), rj[None], Bj[None]))
    return S


def host_eval(e, body, ar=Ar(), mut=None):
    """entry `e` through Ops in arithmetic `ar` (float64 tensor of ref's shape)"""
    ops = Ops(ar, mut, body=body)
    with np.errstate(all="ignore"):
        if e.fn == "residual":
            out = ops.residual(*e.args, CAM_K, e.extra)
        elif e.fn == "shape":
            out = tuple(o[None] for o in ops.shape(body, e.args[0]))
        else:
            out = getattr(ops, e.fn)(*e.args)
    out = out if e.out is None else out[e.out]
    return out.double().reshape(e.ref.shape)


def case_ratios(e, got):
    """error / Bound per case row [n]; a non-finite reference value must be matched in kind (NaN / +inf / -inf), else inf"""
    got = torch.as_tensor(got).double().reshape(e.ref.shape)
    fin = torch.isfinite(e.ref)
    same = torch.where(fin, torch.isfinite(got), (torch.isnan(got) == torch.isnan(e.ref)) & ((got == e.ref) | torch.isnan(e.ref)))
    err = torch.where(fin & torch.isfinite(got), got - e.ref, torch.zeros_like(e.ref))
    r = ratio(err, e.bound.expand_as(e.ref))
    r = torch.where(same, r, torch.full_like(r, float("inf")))
    return r.reshape(r.shape[0], -1).max(dim=1).values


class Worst:
    """the largest ratio per op and the case it came from"""

    def __init__(self):
        self.w = {}

    def note(self, op, ratios, names):
        i = int(torch.as_tensor(ratios).argmax())
        v = float(torch.as_tensor(ratios)[i])
        if op not in self.w or v > self.w[op][0]:
            self.w[op] = (v, names[i])

    def lines(self, title):
        return [title] + [f"  {op:10s} M = {M_OF.get(op, 0):g}  {v:.3f}  ({nm})" if op in M_OF else f"  {op:10s} derived  {v:.3f}  ({nm})"
                          for op, (v, nm) in sorted(self.w.items())]
