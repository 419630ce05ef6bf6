"""Float64 numpy restatement of the four losses of robustcap_amd/losses.py (rc_subnet_loss): value and closed-form gradient with respect
to x, written from the formulas of the kinds (helper of test_subnet_loss_cpu.py and test_gpu_subnet_loss.py; no GPU, no library).
x, y: [F, W] arrays (converted to float64). Every function returns (value, dx)."""
import numpy as np

WINDOWS = (6, 20, 60)


def _f64(*a):
    return [np.asarray(t, dtype=np.float64) for t in a]


def mse(x, y):
    x, y = _f64(x, y)
    d = x - y
    return float((d * d).sum() / d.size), 2.0 * d / d.size


def bce_logits(x, y, pos_weight):
    """mean of (1 - y) x + L (max(-x, 0) + log1p(exp(-|x|))), L = 1 + (pw - 1) y; dx = ((1 - y) - L (1 - sigmoid(x))) / (F W)."""
    x, y, pw = _f64(x, y, pos_weight)
    L = 1.0 + (pw - 1.0) * y
    e = np.exp(-np.abs(x))
    one_m_sig = np.where(x >= 0, e / (1.0 + e), 1.0 / (1.0 + e))
    v = (1.0 - y) * x + L * (np.maximum(-x, 0.0) + np.log1p(e))
    return float(v.sum() / x.size), ((1.0 - y) - L * one_m_sig) / x.size


def window_of(F, w):
    """Per frame f the window it belongs to counted from the END of the batch (e = F - 1 - f, window e // w), -1 for the first F % w
    frames, which belong to none; and the number of windows F // w."""
    e = F - 1 - np.arange(F)
    k = e // w
    return np.where(k < F // w, k, -1), F // w


def window_mse(x, y):
    """mse(x, y) + sum over w in (6, 20, 60) of the mse of the window sums; ValueError below 60 frames (the reference: NaN)."""
    x, y = _f64(x, y)
    F = x.shape[0]
    if F < max(WINDOWS):
        raise ValueError(f"window_mse needs at least {max(WINDOWS)} frames ({F} given)")
    d = x - y
    value, dx = (d * d).sum() / (3 * F), 2.0 * d / (3 * F)
    for w in WINDOWS:
        k, nw = window_of(F, w)
        S = np.zeros((nw, 3))
        np.add.at(S, k[k >= 0], d[k >= 0])
        value += (S * S).sum() / (3 * nw)
        dx[k >= 0] += 2.0 * S[k[k >= 0]] / (3 * nw)
    return float(value), dx


def rotations(v):
    """[..., 6] -> the three columns c0, c1, c2 [..., 3] before the NaN -> 0 step, and |a|, |t|, d = c0 . b."""
    a, b = v[..., :3], v[..., 3:]
    with np.errstate(all="ignore"):
        na = np.sqrt((a * a).sum(-1, keepdims=True))
        c0 = a / na
        d = (c0 * b).sum(-1, keepdims=True)
        t = b - d * c0
        nt = np.sqrt((t * t).sum(-1, keepdims=True))
        c1 = t / nt
        c2 = np.cross(c0, c1)
    return c0, c1, c2, na, nt, d


def joints(v, bones, parent):
    """J [F, 24, 3] of v [F, 24, 6]: pb_i = R_parent(i) b_i (i >= 1), J_i = pb_i + J_parent(i), J_0 = 0; R = (c0 | c1 | c2), NaN -> 0."""
    c0, c1, c2, _, _, _ = rotations(v)
    R = np.nan_to_num(np.stack([c0, c1, c2], axis=-1), nan=0.0, posinf=np.inf, neginf=-np.inf)      # R[..., r, k] = c_k[r]
    J = np.zeros(v.shape[:-1] + (3,))
    for i in range(1, 24):
        p = int(parent[i])
        assert 0 <= p < i
        J[:, i] = J[:, p] + R[:, p] @ bones[i]
    return J


def pose_fk(x, y, bones, parent):
    """mean (x - y)^2 over F 144 + 100 mean (J(x) - J(y))^2 over F 72 (the root's zeros count). bones [24, 3]: rest bone vectors."""
    x, y, bones = _f64(x, y, bones)
    F = x.shape[0]
    vx = x.reshape(F, 24, 6)
    Jx, Jy = joints(vx, bones, parent), joints(y.reshape(F, 24, 6), bones, parent)
    d, dJ = x - y, Jx - Jy
    value = (d * d).sum() / (144 * F) + 100.0 * (dJ * dJ).sum() / (72 * F)
    S = 200.0 * dJ / (72 * F)                                   # d value / d J_i, then the subtree sums (children before parents)
    for i in range(23, 0, -1):
        S[:, int(parent[i])] += S[:, i]
    q = np.zeros((F, 24, 3, 3))                                 # d value / d R_p = sum over children i of S_i b_i^T
    for i in range(1, 24):
        q[:, int(parent[i])] += S[:, i, :, None] * bones[i][None, None, :]
    c0, c1, c2, na, nt, dd0 = rotations(vx)
    b = vx[..., 3:]
    with np.errstate(all="ignore"):
        q0, q1, q2 = (np.where(np.isnan(c), 0.0, q[..., k]) for k, c in enumerate((c0, c1, c2)))   # an entry set to 0 passes nothing on
        q0 = q0 + np.cross(c1, q2)                              # c2 = c0 x c1
        q1 = q1 + np.cross(q2, c0)
        dt = (q1 - c1 * (c1 * q1).sum(-1, keepdims=True)) / nt  # c1 = t / |t|
        dd = -(dt * c0).sum(-1, keepdims=True)                  # t = b - d c0, d = c0 . b
        gb = dt + dd * c0
        q0 = q0 + dd * b - dd0 * dt
        ga = (q0 - c0 * (c0 * q0).sum(-1, keepdims=True)) / na  # c0 = a / |a|
    g = np.concatenate([ga, gb], axis=-1).reshape(F, 144)
    return float(value), 2.0 * d / (144 * F) + g


def rest_bones(body):
    """The rest bone vectors [24, 3] of a body dict (J, parent) in float64: J_i - J_parent(i), the root's own position removed
    (joint_position_to_bone_vector of get_zero_pose_joint_and_vertex()[0])."""
    J = np.asarray(body["J"], dtype=np.float32)
    J = (J - J[:1]).astype(np.float32)                          # the root at the origin, in fp32 as the context holds it
    parent = np.asarray(body["parent"]).astype(np.int64)
    b = np.zeros((24, 3), np.float32)
    for i in range(1, 24):
        b[i] = (-J[parent[i]]) + J[i]
    return b.astype(np.float64), parent


def loss(kind, x, y, pos_weight=None, bones=None, parent=None):
    if kind == "mse":
        return mse(x, y)
    if kind == "bce_logits":
        return bce_logits(x, y, pos_weight)
    if kind == "window_mse":
        return window_mse(x, y)
    if kind == "pose_fk":
        return pose_fk(x, y, bones, parent)
    raise ValueError(kind)
