"""The eleven dataset builders inside ``train_rnn2 .. train_rnn8`` (net/sig_mp.py:301-839) restated in numpy, every operation in float64
or, on request, float32 (helper of test_subnet_corpus_cpu.py and test_gpu_subnet_corpus.py; no library). ``build(name, source, dataset,
dtype)`` returns the reference's ``data`` and ``label`` lists: one [T - 2, in] and one [T - 2, out] array per sample, in the reference's
order (sequence-major, then view, a plain sample before its occlusion sample).

What is restated as written rather than as meant: the AIST and AMASS spellings of the root-frame joints (``Rrw.matmul(j)`` then the
difference, against ``(j - j0).bmm(R)``); rnn7's sensor 5 left in the world frame; and rnn4's occlusion sample, whose xy is NOT divided
by the bounding-box scale because :480 divides the plain sample's tensor (``occ_divides=True`` restates what was meant: the tests use it
to show that the captured rows tell the two apart). K^-1 is the float64 inverse rounded once to ``dtype`` (the library's route; the
reference takes torch's float32 LU inverse)."""
import numpy as np

PARENT = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)
OVERRIDE = {11: 16, 12: 17, 13: 18, 14: 19, 15: 20, 16: 21, 23: 1, 24: 2, 25: 4, 26: 5, 27: 7, 28: 8}
WIDTHS = {"rnn2": (72, 69), "rnn3": (141, 3), "rnn4": (171, 69), "rnn6": (240, 3), "rnn7": (141, 144), "rnn8": (141, 2)}
WORLD_WIDTHS = (171, 72)
RECIPES = [(n, s) for n in ("rnn2", "rnn3", "rnn4", "rnn6", "rnn7") for s in ("aist", "amass")] + [("rnn8", "amass")]
VEL_SCALE = 3


def column_groups(width):
    """(name, first column, end) of the blocks of a data row whose scales differ: accelerations, orientations, everything after."""
    return [("acc", 0, 18), ("ori", 18, 72)] + ([("rest", 72, width)] if width > 72 else [])


def aa_to_R(aa, f):
    """art.math.axis_angle_to_rotation_matrix (articulate/math/angular.py:221-233): [n, 3] -> [n, 3, 3] in dtype ``f``."""
    a = np.asarray(aa).astype(f).reshape(-1, 3)
    th = np.sqrt((a * a).sum(1, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        k = a / th
    k[~np.isfinite(k)] = 0
    c, s = np.cos(th)[..., None], np.sin(th)[..., None]
    K = np.zeros((a.shape[0], 3, 3), f)
    K[:, 0, 1], K[:, 0, 2] = -k[:, 2], k[:, 1]
    K[:, 1, 0], K[:, 1, 2] = k[:, 2], -k[:, 0]
    K[:, 2, 0], K[:, 2, 1] = -k[:, 1], k[:, 0]
    return (c * np.eye(3, dtype=f) + (f(1) - c) * (k[:, :, None] * k[:, None, :]) + s * K).astype(f)


def foot_speed(joint3d, f=np.float64):
    """[T - 2, 2]: |(j[t + 1] - j[t - 1]) 30| of joints 10 and 11 (net/sig_mp.py:812-815)."""
    j = np.asarray(joint3d).astype(f)
    v = (j[2:] - j[:-2]) * f(30)
    return np.sqrt((v[:, 10:12] ** 2).sum(-1))


def _root_frame(name, source, d, i, f):
    T = len(d["imu_acc"][i])
    acc, ori = np.asarray(d["imu_acc"][i]).astype(f), np.asarray(d["imu_ori"][i]).astype(f)
    j = np.asarray(d["joint3d"][i]).astype(f)
    pose = np.asarray(d["pose"][i]).astype(f).reshape(T, 24, 3)
    R = aa_to_R(pose[:, 0], f)
    Rrw = np.swapaxes(R, 1, 2)
    accr = np.einsum("trk,tik->tir", Rrw, acc)
    orir = np.einsum("trk,tikc->tirc", Rrw, ori)
    if name == "rnn7":
        orir[:, 5] = ori[:, 5]
    if source == "aist":
        j3dr = np.einsum("trk,tjk->tjr", Rrw, j)
        j3dr = j3dr[:, 1:] - j3dr[:, :1]
    else:
        j3dr = np.einsum("tjk,tkc->tjc", j[:, 1:] - j[:, :1], R)
    imu = np.concatenate([accr.reshape(T, 18), orir.reshape(T, 54)], 1)
    rel = j3dr.reshape(T, 69)
    if name == "rnn2":
        return imu[1:-1], rel[1:-1]
    x = np.concatenate([imu, rel], 1)[1:-1]
    if name == "rnn3":
        v = (j[2:, 0] - j[:-2, 0]) * f(30) / f(VEL_SCALE)
        return x, np.einsum("trk,tk->tr", Rrw[1:-1], v)
    if name == "rnn8":
        return x, (foot_speed(j, f) < f(0.25)).astype(f)
    Rl = aa_to_R(pose.reshape(-1, 3), f).reshape(T, 24, 3, 3)
    Rl[:, 0] = np.eye(3, dtype=f)
    G = [Rl[:, 0]]
    for q in range(1, 24):
        G.append(np.einsum("tab,tbc->tac", G[PARENT[q]], Rl[:, q]))
    G = np.stack(G, 1)
    r6d = np.swapaxes(G[..., :2], -1, -2).reshape(T, 144)                  # (R00, R10, R20, R01, R11, R21) per joint
    return x, r6d[1:-1]


def _unproject(kp, Kinv, image_size, f):
    kp = np.asarray(kp).astype(f)
    uv1 = np.stack([kp[..., 0] * f(image_size[0]), kp[..., 1] * f(image_size[1]), np.ones(kp.shape[:-1], f)], -1)
    return np.einsum("rk,tjk->tjr", Kinv, uv1)[..., :2], kp[..., 2]


def _bbox_scale(xy):
    return np.maximum(xy[..., 0].max(-1) - xy[..., 0].min(-1), xy[..., 1].max(-1) - xy[..., 1].min(-1))


def _hip_relative(xy):
    out = xy - xy[:, 23:24]
    out[:, 23] = xy[:, 23]
    return out


def _views(name, d, i, f, image_size, occ_divides):
    T = len(d["imu_acc"][i])
    acc, ori = np.asarray(d["imu_acc"][i]).astype(f), np.asarray(d["imu_ori"][i]).astype(f)
    j = np.asarray(d["joint3d"][i]).astype(f)
    out = []
    for c in range(len(d["cam_K"][i])):
        if d["joint2d_mp"][i][c] is None:
            continue
        Tcw = np.asarray(d["cam_T"][i][c]).astype(f)
        Kinv = np.linalg.inv(np.asarray(d["cam_K"][i][c]).astype(np.float64)).astype(f)
        Rcw, t = Tcw[:3, :3], Tcw[:3, 3]
        oric = np.einsum("rk,tikc->tirc", Rcw, ori)
        accc = np.einsum("rk,tik->tir", Rcw, acc)
        j3dc = np.einsum("rk,tjk->tjr", Rcw, j) + t
        rel = (j3dc[:, 1:] - j3dc[:, :1]).reshape(T, 69)
        imu = np.concatenate([accc.reshape(T, 18), oric.reshape(T, 54)], 1)
        xy, conf = _unproject(d["joint2d_mp"][i][c], Kinv, image_size, f)
        if name == "rnn6":
            tranc = np.einsum("rk,tk->tr", Rcw, np.asarray(d["tran"][i]).astype(f)) + t
            kp = np.concatenate([xy, conf[..., None]], -1).reshape(T, 99)
            out.append((np.concatenate([imu, kp, rel], 1)[1:-1], tranc[1:-1]))
            continue
        kp = np.concatenate([_hip_relative(xy / _bbox_scale(xy)[:, None, None]), conf[..., None]], -1).reshape(T, 99)
        out.append((np.concatenate([imu, kp], 1)[1:-1], rel[1:-1]))
        occ = d["joint2d_occ"][i][c] if "joint2d_occ" in d else None
        if occ is None or len(occ) != T:
            continue
        xy, conf = _unproject(occ, Kinv, image_size, f)
        if occ_divides:
            xy = xy / _bbox_scale(xy)[:, None, None]
        kp = np.concatenate([_hip_relative(xy), conf[..., None]], -1).reshape(T, 99)
        out.append((np.concatenate([imu, kp], 1)[1:-1], rel[1:-1]))
    return out


def _world(d, i, f):
    T = len(d["imu_acc"][i])
    j = np.asarray(d["joint3d"][i]).astype(f)
    root = j[0, 0].copy()
    j3dw = j - root
    mp = np.asarray(d["sync_3d_mp"][i]).astype(f) - root
    for row, q in OVERRIDE.items():
        mp[:, row] = j3dw[:, q]
    x = np.concatenate([np.asarray(d["imu_acc"][i]).astype(f).reshape(T, 18), np.asarray(d["imu_ori"][i]).astype(f).reshape(T, 54),
                        mp.reshape(T, 99)], 1)
    return x[1:-1], j3dw.reshape(T, 72)[1:-1]


def build(name, source, dataset, dtype=np.float64, image_size=(1920, 1080), occ_divides=False):
    """(data, label): lists of arrays in ``dtype``, one pair per sample."""
    f = dtype
    samples = []
    for i in range(len(dataset["imu_acc"])):
        if name in ("rnn4", "rnn6"):
            samples += _views(name, dataset, i, f, image_size, occ_divides) if source == "aist" else [_world(dataset, i, f)]
        else:
            samples.append(_root_frame(name, source, dataset, i, f))
    return [x for x, _ in samples], [y for _, y in samples]


# ---- the fixture tests/golden/corpus/subnet_corpus.npz (tools/capture_subnet_corpus.py) -------------------------------------------------------
FIELDS = ("pose", "tran", "imu_ori", "imu_acc", "joint3d", "sync_3d_mp", "shape")


def pack_dicts(aist, amass):
    """The two dictionaries as flat arrays (numbers only): per source and field the sequences concatenated, the cameras, and the
    keypoint lists concatenated over their present entries with the frames of each ([n_seq, n_cam], 0: None)."""
    out = {}
    for src, d in (("aist", aist), ("amass", amass)):
        out[f"{src}.lengths"] = np.asarray([len(a) for a in d["imu_acc"]], np.int64)
        for k in FIELDS:
            out[f"{src}.{k}"] = np.concatenate([np.asarray(a, np.float32).reshape(-1) for a in d[k]])
    out["aist.cam_K"] = np.stack([np.asarray(a, np.float32) for a in aist["cam_K"]])
    out["aist.cam_T"] = np.stack([np.asarray(a, np.float32) for a in aist["cam_T"]])
    for k in ("joint2d_mp", "joint2d_occ"):
        out[f"aist.{k}.frames"] = np.asarray([[0 if e is None else len(e) for e in row] for row in aist[k]], np.int64)
        out[f"aist.{k}"] = np.concatenate([np.asarray(e, np.float32).reshape(-1) for row in aist[k] for e in row if e is not None])
    return out


def unpack_dicts(z):
    """``pack_dicts`` undone: (aist, amass) with float32 numpy arrays and None where an entry was None."""
    dicts = []
    for src in ("aist", "amass"):
        lengths = [int(v) for v in z[f"{src}.lengths"]]
        d = {}
        for k in FIELDS:
            flat, at, d[k] = np.asarray(z[f"{src}.{k}"]), 0, []
            per = flat.size // (len(lengths) if k == "shape" else sum(lengths))
            for T in lengths:
                n = per if k == "shape" else T * per
                d[k].append(flat[at:at + n].reshape((10,) if k == "shape" else (T, -1)))
                at += n
        d["imu_ori"] = [a.reshape(-1, 6, 3, 3) for a in d["imu_ori"]]
        d["imu_acc"] = [a.reshape(-1, 6, 3) for a in d["imu_acc"]]
        d["joint3d"] = [a.reshape(-1, 24, 3) for a in d["joint3d"]]
        d["sync_3d_mp"] = [a.reshape(-1, 33, 3) for a in d["sync_3d_mp"]]
        if src == "amass":
            d["pose"] = [a.reshape(-1, 24, 3) for a in d["pose"]]
        dicts.append(d)
    aist = dicts[0]
    aist["cam_K"], aist["cam_T"] = list(np.asarray(z["aist.cam_K"])), list(np.asarray(z["aist.cam_T"]))
    for k in ("joint2d_mp", "joint2d_occ"):
        flat, at, aist[k] = np.asarray(z[f"aist.{k}"]), 0, []
        for row in np.asarray(z[f"aist.{k}.frames"]):
            entries = []
            for T in row:
                entries.append(None if T == 0 else flat[at:at + int(T) * 99].reshape(int(T), 33, 3))
                at += int(T) * 99
            aist[k].append(entries)
    return aist, dicts[1]


def captured(z, name, source):
    """The reference's (data, label) lists of one recipe out of the fixture."""
    lengths = [int(v) for v in z[f"{name}.{source}.lengths"]]
    cuts = np.cumsum(lengths)[:-1]
    return np.split(np.asarray(z[f"{name}.{source}.data"]), cuts), np.split(np.asarray(z[f"{name}.{source}.label"]), cuts)
