"""The batches of robustcap_amd/batches.py restated in numpy (helper of test_subnet_batches_cpu.py and test_gpu_subnet_batches.py; no
library): every draw of csrc/rc_augment.hip generated from integers with the Philox4x32-10 of subnet_dropout_ref.py, and the sample
arithmetic of the reference's ``augment_fn`` s and AMASS ``__getitem__`` s (net/sig_mp.py:360-363, 520-552, 578-581, 649-679, 701-703,
792-795) in float64 or, on request, float32.

Draws: key = (seed low, seed high), counter = (sample, frame, site | index << 8, call) with ``sample`` the position in the batch and
``frame`` the frame within the sample. Uniforms u = (w >> 8) 2^-24, under a logarithm u = ((w >> 9) + 0.5) 2^-23 (both exact in
float32). Normals: Box-Muller, units 4q, 4q + 1 = r cos t, r sin t from words (0, 1) of call q, units 4q + 2, 4q + 3 from words (2, 3).
Pool rows: a 4-round balanced Feistel network on m bits (m the smallest even number with 2^m >= P) whose round function is word 0 of
the call (sample, right half, PERM | round << 8, call) masked to m / 2 bits, cycle-walked from the frame index until the value is < P."""
import numpy as np

from subnet_dropout_ref import philox4x32_10

SITE_NOISE, SITE_CAMERA, SITE_TRAN, SITE_PERM, SITE_KP = 2, 3, 4, 5, 6
AUGMENT = {"rnn2": None, "rnn3": (69, 0.04), "rnn4": None, "rnn6": (69, 0.03), "rnn7": (141, 0.03), "rnn8": (69, 0.03)}   # noisy columns from the end, sigma
CAMERA = {"rnn4": ((-180, 180), (-30, 30), (-5, 5)), "rnn6": ((-90, 90), (-30, 30), (-5, 5))}
WIDTHS = {"rnn2": (72, 69), "rnn3": (141, 3), "rnn4": (171, 69), "rnn6": (240, 3), "rnn7": (141, 144), "rnn8": (141, 2)}
MUTATIONS = ("minz_first_frame", "minz_landmarks", "row23_relative", "noise_by_p", "root_before_translation", "rcw_not_transposed")


def _key(seed):
    return seed & 0xFFFFFFFF, seed >> 32


def words(sample, frame, site, index, seed, call):
    """The four words of one call, as uint32 arrays of the broadcast shape of the arguments."""
    index = np.asarray(index, dtype=np.uint64)
    return philox4x32_10((sample, frame, np.uint64(site) | (index << np.uint64(8)), call), _key(seed))


def u_closed0(w):
    """(w >> 8) 2^-24 in [0, 1): float64 holding a float32-exact value."""
    return (np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def u_open(w):
    """((w >> 9) + 0.5) 2^-23 in (0, 1)."""
    return ((np.asarray(w, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def box_muller(wa, wb, dtype=np.float64):
    """(r cos t, r sin t), r = sqrt(-2 ln u_open(wa)), t = 2 pi u_closed0(wb), every operation in ``dtype``."""
    ua, ub = u_open(wa).astype(dtype), u_closed0(wb).astype(dtype)
    r = np.sqrt(dtype(-2.0) * np.log(ua))
    t = dtype(6.283185307179586) * ub
    return r * np.cos(t), r * np.sin(t)


def normals(sample, frames, site, units, seed, call, dtype=np.float64):
    """[len(frames), units]: the standard normals of units 0 .. units - 1 of every frame in ``frames`` of sample ``sample``."""
    frames = np.asarray(frames, dtype=np.uint64)
    nq = -(-units // 4)
    w = words(sample, frames[:, None], site, np.arange(nq, dtype=np.uint64)[None, :], seed, call)
    z0, z1 = box_muller(w[0], w[1], dtype)
    z2, z3 = box_muller(w[2], w[3], dtype)
    return np.stack([z0, z1, z2, z3], axis=-1).reshape(len(frames), 4 * nq)[:, :units]


def feistel_bits(P):
    m = 0
    while (1 << m) < P:
        m += 2
    return m


def perm(sample, frames, P, seed, call):
    """Pool row of every frame in ``frames`` (< P) of sample ``sample``: int64 array; a permutation of [0, P) over frames 0 .. P - 1."""
    h = feistel_bits(P) // 2
    mask = np.uint64((1 << h) - 1)
    x = np.asarray(frames, dtype=np.uint64).copy()
    assert x.size == 0 or int(x.max()) < P
    todo = np.ones(x.shape, bool)
    while todo.any():
        v = x[todo]
        L, R = v >> np.uint64(h), v & mask
        for r in range(4):
            f = words(sample, R, SITE_PERM, r, seed, call)[0].astype(np.uint64) & mask
            L, R = R, L ^ f
        v = (L << np.uint64(h)) | R
        x[todo] = v
        todo[todo] = v >= np.uint64(P)
    return x.astype(np.int64)


def euler_yxz(yaw, pitch, roll):
    """Ry(yaw) Rx(pitch) Rz(roll) in float64 (radians): intrinsic 'YXZ' (articulate/math/angular.py:205-218, :337-350)."""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    return np.array([[cy * cr + sy * sp * sr, -cy * sr + sy * sp * cr, sy * cp],
                     [cp * sr, cp * cr, -sp],
                     [-sy * cr + cy * sp * sr, sy * sr + cy * sp * cr, cy * cp]], dtype=np.float64)


def camera_angles(name, sample, seed, call):
    """(yaw, pitch, roll) in radians, float64: radians(lo (1 - u) + hi u) with u from words 0, 1, 2 of the CAMERA call."""
    w = words(sample, 0, SITE_CAMERA, 0, seed, call)
    return [(lo * (1.0 - float(u_closed0(w[i]))) + hi * float(u_closed0(w[i]))) * (np.pi / 180.0) for i, (lo, hi) in enumerate(CAMERA[name])]


def rcw_of(Rc0c):
    """(diag(-1, -1, 1) float32(Rc0c))^T as float32."""
    return (np.diag([-1.0, -1.0, 1.0]) @ Rc0c.astype(np.float32).astype(np.float64)).T.astype(np.float32)


def world_draws(name, T, P, sample, seed, call):
    """Everything random of one ``world`` sample, as integers and exact values: Rcw (float32), the three translation uniforms, the
    pool rows [T] and the words behind the normals (so that either precision can form them)."""
    wt = words(sample, 0, SITE_TRAN, 0, seed, call)
    fr = np.arange(T, dtype=np.uint64)
    return {"Rcw": rcw_of(euler_yxz(*camera_angles(name, sample, seed, call))),
            "ut": np.array([float(u_closed0(wt[i])) for i in range(3)]),
            "rows": perm(sample, fr, P, seed, call),
            "kp": lambda dtype: normals(sample, fr, SITE_KP, 66, seed, call, dtype).reshape(T, 33, 2),
            "tail": lambda dtype: normals(sample, fr, SITE_NOISE, 69, seed, call, dtype)}


def world_arith(name, data, label, pool, draws, dtype=np.float64, mutate=None):
    """The AMASS __getitem__ of rnn4 (net/sig_mp.py:520-552) / rnn6 (:649-679) on one sample with the draws handed in, every operation
    in ``dtype``. data [T, 171], label [T, 72], pool [P, 33]. Returns a dict of the quantities: x [T, 171 or 240], label, and the pieces
    accc, oric, xy, conf (and tail for rnn6). ``mutate``: one of MUTATIONS -- a deliberate mistake, for the tests of the tests."""
    f = dtype
    T = data.shape[0]
    data, label, pool = np.asarray(data).astype(f), np.asarray(label).astype(f), np.asarray(pool).astype(f)
    R = draws["Rcw"].astype(f)
    if mutate == "rcw_not_transposed":
        R = R.T
    acc, ori = data[:, :18].reshape(T, 6, 3), data[:, 18:72].reshape(T, 6, 3, 3)
    mp, j = data[:, 72:].reshape(T, 33, 3), label.reshape(T, 24, 3)
    accc = np.einsum("rk,tik->tir", R, acc)
    oric = np.einsum("rk,tikc->tirc", R, ori)
    j3dc = np.einsum("rk,tjk->tjr", R, j)
    j3dc_mp = np.einsum("rk,tjk->tjr", R, mp)
    u = draws["ut"].astype(f)
    t = np.array([-1, -1, 3], f) * (f(1) - u) + np.array([1, 1, 8], f) * u
    zsrc = j3dc_mp if mutate == "minz_landmarks" else j3dc
    t[2] = t[2] - (zsrc[0, :, 2].min() if mutate == "minz_first_frame" else zsrc[..., 2].min())
    root_before = j3dc[:, 0].copy()
    j3dc = j3dc + t
    j3dc_mp = j3dc_mp + t
    xy = j3dc_mp[..., :2] / j3dc_mp[..., 2:]
    p = pool[draws["rows"]]                                                 # [T, 33]
    w = p if mutate == "noise_by_p" else (f(1) - p)
    xy = xy + (f(0.003) * w)[..., None] * draws["kp"](f)
    rel = (j3dc[:, 1:] - j3dc[:, :1]).reshape(T, 69)
    out = {"accc": accc.reshape(T, 18), "oric": oric.reshape(T, 54), "conf": p}
    if name == "rnn4":
        sc = np.maximum(xy[..., 0].max(1) - xy[..., 0].min(1), xy[..., 1].max(1) - xy[..., 1].min(1))
        xy = xy / sc[:, None, None]
        hip = xy[:, 23:24].copy()
        keep = np.zeros(33, bool) if mutate == "row23_relative" else (np.arange(33) == 23)
        xy = np.where(keep[None, :, None], xy, xy - hip)
        out["label"] = rel
        cols = [out["accc"], out["oric"], np.concatenate([xy, p[..., None]], -1).reshape(T, 99)]
    else:
        out["label"] = root_before if mutate == "root_before_translation" else j3dc[:, 0]
        out["tail"] = rel + f(0.03) * draws["tail"](f)
        cols = [out["accc"], out["oric"], np.concatenate([xy, p[..., None]], -1).reshape(T, 99), out["tail"]]
    out["xy"] = xy.reshape(T, 66)
    out["x"] = np.concatenate(cols, 1)
    return out


def world_sample(name, data, label, pool, sample, seed, call, dtype=np.float64, mutate=None):
    return world_arith(name, data, label, pool, world_draws(name, data.shape[0], pool.shape[0], sample, seed, call), dtype, mutate)


def plain_noise(name, T, sample, seed, call, dtype=np.float64):
    """[T, noisy columns] sigma * z of a ``plain`` sample (None for a sub-net without augmentation), and the first noisy column."""
    if AUGMENT[name] is None:
        return None, WIDTHS[name][0]
    cols, sigma = AUGMENT[name]
    z = normals(sample, np.arange(T, dtype=np.uint64), SITE_NOISE, cols, seed, call, dtype)
    return dtype(sigma) * z, WIDTHS[name][0] - cols


def plain_sample(name, data, sample, seed, call, dtype=np.float64):
    """RNNDataset.__getitem__ with the sub-net's augment_fn on one sample: x + sigma z on the noisy columns, the rest untouched."""
    x = np.asarray(data).astype(dtype).copy()
    nz, c0 = plain_noise(name, x.shape[0], sample, seed, call, dtype)
    if nz is not None:
        x[:, c0:] = x[:, c0:] + nz
    return x


def split_table(lengths, split_size):
    """(first frame, frames) of every sample of sequences of ``lengths`` split like Tensor.split."""
    out, at = [], 0
    for T in lengths:
        step = split_size if split_size > 0 else T
        out += [(at + a, min(step, T - a)) for a in range(0, T, step)]
        at += T
    return out


def world_corpus(seed, lengths, box=0.8):
    """A seeded ``world`` corpus: data [F, 171] = acc | ori | j3dw_mp, label [F, 72] = j3dw, float32. Joints uniform in a +-``box`` m
    cube, landmarks within 0.1 m of a joint each (so within +-0.9 m: a landmark stays in front of the camera, whose depth is at least
    3 m above the lowest JOINT), accelerations normal, orientations random rotations."""
    g = np.random.default_rng(seed)
    F = int(sum(lengths))
    j = g.uniform(-box, box, (F, 24, 3))
    mp = j[:, g.integers(0, 24, 33)] + g.uniform(-0.1, 0.1, (F, 33, 3))
    acc = g.normal(0, 3.0, (F, 6, 3))
    q, r = np.linalg.qr(g.normal(size=(F * 6, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 0] *= np.linalg.det(q)[:, None]
    data = np.concatenate([acc.reshape(F, 18), q.reshape(F, 54), mp.reshape(F, 99)], 1).astype(np.float32)
    return data, j.reshape(F, 72).astype(np.float32)


def conf_pool(seed, P, distinct=False):
    """[P, 33] float32 confidences in (0, 1); ``distinct``: column 0 of row i is (i + 0.5) / P, so a row identifies itself."""
    pool = np.random.default_rng(seed).uniform(0.02, 0.98, (P, 33)).astype(np.float32)
    if distinct:
        pool[:, 0] = ((np.arange(P) + 0.5) / P).astype(np.float32)
    return pool


def bound_ratio(got, f64, f32, K=8.0, floor=1e-7):
    """max |got - f64| / (K max |f32 - f64| + floor max |f64|): at most 1 within the project's bound."""
    f64 = np.asarray(f64, np.float64)
    err = np.abs(np.asarray(got, np.float64) - f64).max()
    e32 = np.abs(np.asarray(f32, np.float64) - f64).max()
    return float(err / (K * e32 + floor * np.abs(f64).max())) if err > 0 else 0.0
