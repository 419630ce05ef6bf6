"""IMU synthesis of the reference's dataset preparation on the GPU.

Mirrors ``preprocess.py``: ``_syn_acc`` (L22-33) and the recipe of L206-214 that turns SMPL pose + translation into the
six virtual IMU readings (global orientation of joints ``ji_mask``, acceleration of vertices ``vi_mask``). The
arithmetic runs in librobustcap_hip.so (rc_syn_acc, rc_synth_imu).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from . import body as _body
from . import config as cfg


def _syn_acc(v, smooth_n=2, device="cuda"):
    """preprocess._syn_acc: v [T, ...] positions (60 fps) -> accelerations of the same shape (device tensor)."""
    x = _body._f32c(v, torch.device(device))
    T = x.shape[0]
    width = int(np.prod(x.shape[1:])) if x.dim() > 1 else 1
    out = torch.empty_like(x)
    lib = _lib.load()
    rc = lib.rc_syn_acc(_lib.ptr(x), T, width, int(smooth_n), _lib.ptr(out), _lib.stream_ptr())
    if rc != 0:
        raise _lib.RobustcapLibraryError(f"rc_syn_acc failed ({rc}): needs smooth_n >= 0 and, for smooth_n >= 2, "
                                         f"at least 2 * smooth_n + 1 frames (got T={T}, smooth_n={smooth_n})")
    return out


def synthesize_imu(model, pose, tran, smooth_n=2, vertex_ids=cfg.vi_mask, joint_ids=cfg.ji_mask):
    """preprocess.py:206-214 for one sequence. ``model`` = robustcap_amd.body.ParametricModel, pose [T,24,3,3] local
    rotation matrices (or [T,72] axis-angle), tran [T,3]. Returns device tensors
    (imu_ori [T,6,3,3], imu_acc [T,6,3], joint3d [T,24,3], vert6 [T,6,3])."""
    dev = model.device
    pose = torch.as_tensor(pose)
    if pose.shape[-1] == 72 or (pose.dim() == 3 and pose.shape[-2:] == (24, 3)):
        pose = _body.axis_angle_to_rotation_matrix(pose.reshape(-1, 3), dev)
    pose = _body._f32c(pose, dev).view(-1, 24, 3, 3)
    T = pose.shape[0]
    tran = _body._f32c(tran, dev).view(T, 3)
    model._ensure_mesh()
    ori, acc = torch.empty(T, 6, 3, 3, device=dev), torch.empty(T, 6, 3, device=dev)
    joint, vert6 = torch.empty(T, 24, 3, device=dev), torch.empty(T, 6, 3, device=dev)
    vid = (C.c_int32 * 6)(*[int(v) for v in vertex_ids])
    jid = (C.c_int32 * 6)(*[int(j) for j in joint_ids])
    rc = model._lib.rc_synth_imu(model._ctx, _lib.ptr(pose), _lib.ptr(tran), vid, jid, T, int(smooth_n), _lib.ptr(ori), _lib.ptr(acc),
                                 _lib.ptr(joint), _lib.ptr(vert6), _lib.stream_ptr())
    _lib.check(model._ctx, rc, "rc_synth_imu")
    return ori, acc, joint, vert6


def make_motion_device(seed, B, T, body, conf="mixed", noise=0.003, model=None, device="cuda"):
    """``synth.make_motion`` with the heavy part on the GPU ("on-device generator for benchmark inputs (FK -> ori /
    acc / 2D), removes host prep from large-B runs"; the recipe is preprocess.py:22-33, 206-222 + the projection of evaluate.py:70-72).

    The seeded random walks (24 axis-angles, root yaw / tilt, root translation, confidence schedule, unit keypoint noise) are a few
    hundred floats per frame and stay host numpy -- the SAME numbers as ``make_motion``; forward kinematics + the 33 landmarks
    (``rc_body_fk``), the six virtual IMUs (``rc_synth_imu``: global orientation of joints ji_mask, smoothed second difference of vertices
    vi_mask) and the projection run on the device and the outputs stay there. Returns the dict of ``make_motion`` with device tensors for
    j2dc / accc / oric / pose / tran and host arrays for gravityc / first_tran / conf; equal to the host generator to fp32 rounding."""
    from . import synth
    dev = torch.device(device)
    model = model or _body.ParametricModel(body=body, device=device)
    R, tr, ck, unit, grav = [], [], [], [], []
    for b in range(B):
        s = seed * 7919 + b
        r, g, t_ = synth.motion_trajectory(s, T)
        c, u = synth.motion_confidence(s, T, conf)
        R.append(r); tr.append(t_); ck.append(c); unit.append(u); grav.append(g)
    pose = torch.from_numpy(np.stack(R).astype(np.float32)).to(dev)                      # [B,T,24,3,3]
    tran = torch.from_numpy(np.stack(tr).astype(np.float32)).to(dev)                      # [B,T,3]
    ckd = torch.from_numpy(np.stack(ck).astype(np.float32)).to(dev)                       # [B,T,33]
    unitd = torch.from_numpy(np.stack(unit).astype(np.float32)).to(dev)                   # [B,T,33,2]
    _, _, j33 = model.forward_kinematics(pose.view(-1, 24, 3, 3), tran=tran.view(-1, 3), calc_mesh=True)
    j33 = j33.view(B, T, 33, 3)
    uv = j33[..., :2] / j33[..., 2:] + noise * (1.0 - ckd)[..., None] * unitd
    j2dc = torch.cat([uv, ckd[..., None]], -1).contiguous()
    ori = torch.empty(B, T, 6, 3, 3, device=dev)
    acc = torch.empty(B, T, 6, 3, device=dev)
    for b in range(B):                                                                    # (the stencil runs along one sequence)
        o, a, _, _ = synthesize_imu(model, pose[b], tran[b], smooth_n=2 if T > 4 else 1)
        ori[b], acc[b] = o, a
    return {"j2dc": j2dc, "accc": acc, "oric": ori, "pose": pose, "tran": tran,
            "gravityc": np.stack(grav).astype(np.float32), "first_tran": np.stack(tr)[:, 0].astype(np.float32),
            "conf": np.stack(ck).mean(-1).astype(np.float32)}


# ---- the motion half of preprocess_amass / preprocess_aist for all sequences in one call (rc_prepare_motions, csrc/rc_prepare.hip) --------
AMASS_ROT = ((1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, -1.0, 0.0))        # preprocess.py:282
AIST_ROOT_OFFSET = (-0.00217368, -0.240789175, 0.028583793)             # preprocess.py:43 (the SMPL root of the mean shape)
FIELDS = ("pose", "tran", "joint3d", "sync_3d_mp", "imu_acc", "imu_ori")
_TAILS = {"tran": (3,), "joint3d": (24, 3), "sync_3d_mp": (33, 3), "imu_acc": (6, 3), "imu_ori": (6, 3, 3)}


def output_lengths(in_frames, steps=None):
    """Frames of ``x[::step]`` per sequence (preprocess.py:268-271): ceil(in / step), step 1 or 2."""
    steps = [1] * len(in_frames) if steps is None else [int(s) for s in steps]
    if len(steps) != len(in_frames):
        raise ValueError(f"{len(steps)} steps for {len(in_frames)} sequences")
    if any(s not in (1, 2) for s in steps):
        raise ValueError("a step is 1 or 2")
    return [(int(n) + s - 1) // s for n, s in zip(in_frames, steps)]


def amass_step(framerate):
    """preprocess.py:263-266: 2 for 120 fps, 1 for 60 / 59 fps, None (the file is skipped) for any other rate."""
    fr = int(framerate)
    return 2 if fr == 120 else 1 if fr in (60, 59) else None


def kept_sequences(in_frames, steps=None, min_frames=0):
    """(kept, dropped) sequence indices: a sequence whose output length is <= ``min_frames`` is dropped (preprocess.py:291, ``l <= 12``)."""
    out = output_lengths(in_frames, steps)
    kept = [i for i, n in enumerate(out) if n > min_frames]
    return kept, [i for i in range(len(out)) if out[i] <= min_frames]


class PreparedMotions:
    """What ``prepare_motions`` leaves on the device: the concatenated fields of the reference's preprocessed dictionary -- ``pose``
    [frames,72], ``tran`` [frames,3], ``joint3d`` [frames,24,3], ``sync_3d_mp`` [frames,33,3], ``imu_acc`` [frames,6,3], ``imu_ori``
    [frames,6,3,3], ``vert6`` [frames,6,3] -- with ``lengths`` (output frames per kept sequence), ``shape`` ([n,10] host, or None),
    ``kept`` / ``dropped`` (indices into the caller's lists) and ``extra`` (host entries that pass through: ``cam_K``, ``cam_T``, keypoint
    lists, names). ``corpus.build`` reads the buffers in place; ``as_dict()`` gives the reference's layout as per-sequence views."""

    def __init__(self, layout, lengths, fields, vert6, rest_joint, shape, kept, dropped, extra=None):
        self.layout, self.lengths, self.fields, self.vert6, self.rest_joint = layout, list(lengths), fields, vert6, rest_joint
        self.shape, self.kept, self.dropped, self.extra = shape, kept, dropped, dict(extra or {})
        for k, v in fields.items():
            setattr(self, k, v)

    @property
    def frames(self):
        return sum(self.lengths)

    def __contains__(self, key):
        return key in self.fields or key in self.extra or (key == "shape" and self.shape is not None)

    def __getitem__(self, key):
        return self.extra[key] if key in self.extra else self.as_dict()[key]

    def get(self, key, default=None):
        return self[key] if key in self else default

    def as_dict(self):
        """The dictionary of preprocess.py:289 (AMASS: ``pose`` [T,24,3]), :229-237 (AIST++: ``pose`` [T,72]), :406 (TotalCapture:
        ``pose`` [T,24,3]) or :454 (3DPW, layout "camera": ``posec`` [T,24,3,3], ``tranc``, ``imu_oric``, ``imu_accc``, ...): lists of
        per-sequence views of the device buffers, plus ``shape`` (AMASS, 3DPW) and whatever ``extra`` holds."""
        d = {}
        for k in (CAMERA_FIELDS if self.layout == "camera" else FIELDS):
            if k not in self.fields:                                       # (camera layout: ``joint2d_mp`` only where keypoints came in)
                continue
            parts = torch.split(self.fields[k], self.lengths)
            d[k] = [p.view(-1, 24, 3) for p in parts] if k == "pose" and self.layout in ("amass", "totalcapture") else list(parts)
        if self.shape is not None:
            d["shape"] = list(self.shape)
        d.update(self.extra)
        return d


def _concat(seqs, lengths, width, what):
    """One host float32 tensor [sum T_i, width] from a list of per-sequence arrays, or from one concatenated array plus ``lengths``."""
    def one(a):
        return a.detach().to(dtype=torch.float32).reshape(a.shape[0], -1) if isinstance(a, torch.Tensor) else \
            torch.as_tensor(np.asarray(a, dtype=np.float32)).reshape(np.shape(a)[0], -1)
    if lengths is None:
        parts = [one(a) for a in seqs]
        lengths = [int(p.shape[0]) for p in parts]
        x = torch.cat(parts) if parts else torch.zeros(0, width or 1)
    else:
        lengths, x = [int(n) for n in lengths], one(seqs)
        if x.shape[0] != sum(lengths):
            raise ValueError(f"{what}: {x.shape[0]} frames, the lengths sum to {sum(lengths)}")
    if width is not None and x.shape[0] and x.shape[1] != width:
        raise ValueError(f"{what}: rows of {width} floats expected, got {x.shape[1]}")
    return x, lengths


def prepare_motions(model, poses, trans, betas=None, steps=None, world_rot=None, smooth_n=2, min_frames=0, lengths=None, layout="amass",
                    extra=None, vertex_ids=cfg.vi_mask, joint_ids=cfg.ji_mask, landmark_ids=cfg.mp_mask):
    """preprocess.py:276-302 (and :216-222) for every sequence at once, in ONE ``rc_prepare_motions`` call: raw axis-angle poses
    (24 or 52 joints), translations and one beta row per sequence in, the fields of the preprocessed dictionary out, on the device.

    ``poses`` / ``trans``: lists of per-sequence arrays ([T_i, J, 3] or [T_i, 3 J]; [T_i, 3]), or one concatenated array each plus
    ``lengths`` (raw frames per sequence). ``betas`` [n, 10] or None (the model's current body). ``steps``: 1 or 2 per sequence
    (``[::step]``). ``world_rot`` [3,3] or None (``AMASS_ROT``). Sequences whose output length is <= ``min_frames`` are dropped before the
    call (their indices: ``.dropped``). Host or device tensors are accepted; the upload is one copy per input. Returns a
    ``PreparedMotions``."""
    dev = model.device
    if isinstance(poses, torch.Tensor) and poses.is_cuda and lengths is not None:
        pose_all, in_len = poses.to(torch.float32).reshape(poses.shape[0], -1), [int(n) for n in lengths]
        tran_all = torch.as_tensor(trans).to(device=dev, dtype=torch.float32).reshape(-1, 3)
        if pose_all.shape[0] != sum(in_len) or tran_all.shape[0] != sum(in_len):
            raise ValueError("poses / trans: the lengths do not sum to their frames")
    else:
        pose_all, in_len = _concat(poses, lengths, None, "poses")
        tran_all, t_len = _concat(trans, lengths, 3, "trans")
        if t_len != in_len:
            raise ValueError("poses and trans differ in their frames per sequence")
    n = len(in_len)
    if n and pose_all.shape[1] not in (72, 156):
        raise ValueError(f"poses: 24 or 52 joints expected, got rows of {pose_all.shape[1]} floats")
    pose_joints = pose_all.shape[1] // 3
    steps = [1] * n if steps is None else [int(s) for s in steps]
    kept, dropped = kept_sequences(in_len, steps, min_frames)
    if not kept:
        raise ValueError("no sequence is left")
    beta = None
    if betas is not None:
        beta = torch.as_tensor(np.asarray(betas, dtype=np.float32) if not isinstance(betas, torch.Tensor) else betas).detach().to("cpu", torch.float32).reshape(-1, 10)
        if beta.shape[0] != n:
            raise ValueError(f"betas: {beta.shape[0]} rows for {n} sequences")
    if dropped:                                                            # (rows of dropped sequences never reach the device call)
        off = np.concatenate([[0], np.cumsum(in_len)])
        idx = torch.cat([torch.arange(int(off[i]), int(off[i + 1])) for i in kept]).to(pose_all.device)
        pose_all, tran_all = pose_all[idx], tran_all[idx.to(tran_all.device)]
        beta = None if beta is None else beta[kept]
    in_k, step_k = [in_len[i] for i in kept], [steps[i] for i in kept]
    out_len = output_lengths(in_k, step_k)
    F, m = sum(out_len), len(kept)
    pose_d, tran_d = _body._f32c(pose_all, dev), _body._f32c(tran_all, dev)
    beta_d = None if beta is None else beta.to(dev).contiguous()
    model._ensure_shape_space(landmark_ids, vertex_ids)
    f = {"pose": torch.empty(F, 72, device=dev), "tran": torch.empty(F, 3, device=dev), "joint3d": torch.empty(F, 24, 3, device=dev),
         "sync_3d_mp": torch.empty(F, 33, 3, device=dev), "imu_acc": torch.empty(F, 6, 3, device=dev),
         "imu_ori": torch.empty(F, 6, 3, 3, device=dev)}
    vert6, rest = torch.empty(F, 6, 3, device=dev), torch.empty(m, 24, 3, device=dev)
    W = None if world_rot is None else (C.c_float * 9)(*[float(v) for v in np.asarray(world_rot, dtype=np.float64).reshape(9)])
    rc = model._lib.rc_prepare_motions(model._ctx, m, (C.c_int64 * m)(*in_k), (C.c_int32 * m)(*step_k), sum(in_k), _lib.ptr(pose_d), pose_joints,
                                       _lib.ptr(tran_d), _lib.ptr(beta_d), W, (C.c_int32 * 6)(*[int(j) for j in joint_ids]), int(smooth_n),
                                       _lib.ptr(f["pose"]), _lib.ptr(f["tran"]), _lib.ptr(f["imu_ori"]), _lib.ptr(f["imu_acc"]),
                                       _lib.ptr(f["joint3d"]), _lib.ptr(f["sync_3d_mp"]), _lib.ptr(vert6), _lib.ptr(rest), _lib.stream_ptr())
    _lib.check(model._ctx, rc, "rc_prepare_motions")
    for t in (pose_d, tran_d, beta_d):                                     # the inputs outlive the asynchronous launch
        if t is not None:
            t.record_stream(torch.cuda.current_stream())
    return PreparedMotions(layout, out_len, f, vert6, rest, beta, kept, dropped, extra)


def prepare_amass(model, poses52, trans, betas, framerates, smooth_n=2):
    """The body of ``preprocess_amass`` (preprocess.py:263-302) from the arrays of the ``*_poses.npz`` files: ``poses52[i]`` [T_i, 156],
    ``trans[i]`` [T_i, 3], ``betas[i]`` (its first 10 entries are used), ``framerates[i]`` (``mocap_framerate``). Files of 120 fps are
    decimated by 2, 60 / 59 fps kept, any other rate skipped (:263-266); the world frame is turned by ``AMASS_ROT``; sequences of 12
    frames or fewer are dropped (:291). ``.kept`` / ``.dropped`` index the caller's lists (skipped rates count as dropped)."""
    steps = [amass_step(fr) for fr in framerates]
    use = [i for i, s in enumerate(steps) if s is not None]
    if not use:
        raise ValueError("no file with a frame rate of 120, 60 or 59")
    b = np.stack([np.asarray(betas[i], dtype=np.float32).reshape(-1)[:10] for i in use])
    out = prepare_motions(model, [poses52[i] for i in use], [trans[i] for i in use], b, [steps[i] for i in use], AMASS_ROT, smooth_n,
                          min_frames=12, layout="amass")
    skipped = [i for i, s in enumerate(steps) if s is None]
    out.kept, out.dropped = [use[i] for i in out.kept], sorted(skipped + [use[i] for i in out.dropped])
    return out


def aist_cameras(cameras, scale):
    """``cam_K`` [9,3,3], ``cam_T`` [9,4,4] of preprocess.py:211-214 from the camera dictionaries of one setting (``matrix``,
    ``rotation`` axis-angle, ``translation``), on the host in float64 and rounded once."""
    K = np.stack([np.asarray(d["matrix"], dtype=np.float64).reshape(3, 3) for d in cameras])
    T = np.zeros((len(cameras), 4, 4))
    for i, d in enumerate(cameras):
        a = np.asarray(d["rotation"], dtype=np.float64).reshape(3)
        th = np.linalg.norm(a)
        k = a / th if th > 0 else np.zeros(3)
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        T[i, :3, :3] = np.cos(th) * np.eye(3) + (1 - np.cos(th)) * np.outer(k, k) + np.sin(th) * Kx
        T[i, :3, 3] = np.asarray(d["translation"], dtype=np.float64).reshape(3) / float(scale)
        T[i, 3, 3] = 1.0
    return torch.from_numpy(K.astype(np.float32)), torch.from_numpy(T.astype(np.float32))


def prepare_aist(model, smpl_poses, smpl_trans, smpl_scaling, cameras=None, tran_offset=AIST_ROOT_OFFSET, smooth_n=2, extra=None):
    """The motion part of ``preprocess_aist`` (preprocess.py:207-222) for lists of sequences: ``tran / scale + tran_offset`` on the mean
    shape (``tran_offset``: the local constant of preprocess.py:43, which :209 adds; pass ``config.tran_offset`` for the other one),
    ``pose`` [T,72]. ``cameras[i]``: the nine camera dictionaries of sequence i -> ``cam_K`` / ``cam_T`` in ``.extra`` (built on the
    host). Keypoint lists (``joint2d_mp``, ``joint2d_occ``) are the caller's: pass them in ``extra``."""
    model.set_shape(None)
    off = np.asarray(tran_offset, dtype=np.float32)
    scales = [float(np.asarray(s).reshape(-1)[0]) for s in smpl_scaling]
    trans = [np.asarray(t, dtype=np.float32) / np.float32(s) + off for t, s in zip(smpl_trans, scales)]
    ex = dict(extra or {})
    if cameras is not None:
        KT = [aist_cameras(c, s) for c, s in zip(cameras, scales)]
        ex["cam_K"], ex["cam_T"] = [k for k, _ in KT], [t for _, t in KT]
    return prepare_motions(model, smpl_poses, trans, None, None, None, smooth_n, 0, layout="aist", extra=ex)


# ---- camera-frame motions: 3DPW / 3DPW-OCC (a T_cw per frame) and TotalCapture (rc_prepare_camera_motions, csrc/rc_prepare.hip) -----------
CAMERA_FIELDS = ("posec", "tranc", "joint3d", "sync_3d_mp", "imu_accc", "imu_oric", "joint2d_mp")
TC_IMU_ORDER = (2, 3, 0, 1, 4, 5)                                       # preprocess.py:351-352
TC_FLIP = ((-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, -1.0))         # :359


def camera_output_lengths(in_frames, cam_frames, cam_repeat=2):
    """Output frames per sequence: ``min(in, cam_repeat * cam)`` -- the ``[:len(cam_pose)]`` / ``cam_pose[:len(posec)]`` pair of
    preprocess.py:463-465, :577 -- or ``in`` for ``cam_repeat=0`` (one static camera row per sequence)."""
    r = int(cam_repeat)
    if r < 0:
        raise ValueError("cam_repeat must not be negative")
    if len(in_frames) != len(cam_frames):
        raise ValueError(f"{len(cam_frames)} camera tables for {len(in_frames)} sequences")
    if any(int(c) < 1 for c in cam_frames):
        raise ValueError("a sequence without a camera row")
    if r == 0 and any(int(c) != 1 for c in cam_frames):
        raise ValueError("cam_repeat=0 takes one camera row per sequence")
    return [int(n) if r == 0 else min(int(n), r * int(c)) for n, c in zip(in_frames, cam_frames)]


def prepare_camera_motions(model, poses, trans, cam_T, betas=None, cam_repeat=2, keypoints=None, root_only=False, smooth_n=2, extra=None,
                           vertex_ids=cfg.vi_mask, joint_ids=cfg.ji_mask, landmark_ids=cfg.mp_mask):
    """preprocess.py:460-470 (and :571-582) for every sequence at once, in ONE ``rc_prepare_camera_motions`` call: axis-angle poses
    [T_i,24,3] (or [T_i,72]) and translations [T_i,3] in the world frame, ``cam_T[i]`` [n_i,4,4] the T_cw rows of sequence i (a single
    [4,4] for ``cam_repeat=0``), output frame t under row ``t // cam_repeat``. ``betas`` [n,10] or None (the model's current body).
    ``keypoints[i]`` [k_i,33,3]: 30 Hz detections raised to 60 Hz by the midpoint interleave of :477-483, cut to the output length.
    ``root_only``: the translation is kept as it is (TotalCapture). Returns a ``PreparedMotions`` with ``layout="camera"``: ``posec``
    [frames,24,3,3] ROTATION MATRICES, ``tranc``, ``imu_oric``, ``imu_accc``, ``joint3d``, ``sync_3d_mp`` and ``joint2d_mp`` on the
    device; ``as_dict()`` adds ``shape``, ``cam_T`` (the rows actually used, [T,4,4] per sequence, host) and what ``extra`` holds."""
    dev = model.device
    pose_all, in_len = _concat(poses, None, 72, "poses")
    tran_all, t_len = _concat(trans, None, 3, "trans")
    if t_len != in_len:
        raise ValueError("poses and trans differ in their frames per sequence")
    n = len(in_len)
    cams = [np.asarray(c.detach().cpu() if isinstance(c, torch.Tensor) else c, dtype=np.float32).reshape(-1, 4, 4) for c in cam_T]
    if len(cams) != n:
        raise ValueError(f"{len(cams)} camera tables for {n} sequences")
    cam_len = [int(c.shape[0]) for c in cams]
    r = int(cam_repeat)
    out_len = camera_output_lengths(in_len, cam_len, r)
    F = sum(out_len)
    beta = None
    if betas is not None:
        beta = torch.as_tensor(np.asarray(betas, dtype=np.float32) if not isinstance(betas, torch.Tensor) else betas).detach().to("cpu", torch.float32).reshape(-1, 10)
        if beta.shape[0] != n:
            raise ValueError(f"betas: {beta.shape[0]} rows for {n} sequences")
    kp_d, kp_len = None, None
    if keypoints is not None:
        kp_all, kp_len = _concat(keypoints, None, 99, "keypoints")
        if len(kp_len) != n:
            raise ValueError(f"{len(kp_len)} keypoint lists for {n} sequences")
        kp_d = _body._f32c(kp_all, dev)
    cam_all = np.ascontiguousarray(np.concatenate(cams))
    pose_d, tran_d = _body._f32c(pose_all, dev), _body._f32c(tran_all, dev)
    beta_d = None if beta is None else beta.to(dev).contiguous()
    model._ensure_shape_space(landmark_ids, vertex_ids)
    f = {"posec": torch.empty(F, 24, 3, 3, device=dev), "tranc": torch.empty(F, 3, device=dev), "joint3d": torch.empty(F, 24, 3, device=dev),
         "sync_3d_mp": torch.empty(F, 33, 3, device=dev), "imu_accc": torch.empty(F, 6, 3, device=dev),
         "imu_oric": torch.empty(F, 6, 3, 3, device=dev)}
    if kp_d is not None:
        f["joint2d_mp"] = torch.empty(F, 33, 3, device=dev)
    vert6, rest = torch.empty(F, 6, 3, device=dev), torch.empty(n, 24, 3, device=dev)
    i64 = lambda v: (C.c_int64 * n)(*[int(x) for x in v])
    rc = model._lib.rc_prepare_camera_motions(
        model._ctx, n, i64(in_len), i64(cam_len), r, sum(in_len), sum(cam_len), _lib.ptr(pose_d), _lib.ptr(tran_d), _lib.ptr(beta_d),
        cam_all.ctypes.data_as(C.c_void_p), _lib.ptr(kp_d), None if kp_len is None else i64(kp_len), 0 if kp_len is None else sum(kp_len),
        (C.c_int32 * 6)(*[int(j) for j in joint_ids]), int(smooth_n), 1 if root_only else 0, _lib.ptr(f["posec"]), _lib.ptr(f["tranc"]),
        _lib.ptr(f["imu_oric"]), _lib.ptr(f["imu_accc"]), _lib.ptr(f["joint3d"]), _lib.ptr(f["sync_3d_mp"]), _lib.ptr(vert6),
        _lib.ptr(f.get("joint2d_mp")), _lib.ptr(rest), _lib.stream_ptr())
    _lib.check(model._ctx, rc, "rc_prepare_camera_motions")
    for t in (pose_d, tran_d, beta_d, kp_d):                               # the inputs outlive the asynchronous launch
        if t is not None:
            t.record_stream(torch.cuda.current_stream())
    ex = dict(extra or {})
    ex["cam_T"] = [torch.from_numpy(c[(np.arange(T) // r) if r else np.zeros(T, np.int64)]) for c, T in zip(cams, out_len)]
    return PreparedMotions("camera", out_len, f, vert6, rest, beta, list(range(n)), [], ex)


def prepare_pw3d(model, poses_60hz, trans_60hz, betas, cam_poses, cam_intrinsics, keypoints30, names=None, generator=None):
    """The body of ``preprocess_3dpw`` / ``preprocess_3dpwocc`` (preprocess.py:459-494, :570-606) from the arrays of the sequence
    pickles, one entry per PERSON: ``poses_60hz[i]`` [T_i,72], ``trans_60hz[i]`` [T_i,3], ``betas[i]`` (its first 10 entries),
    ``cam_poses[i]`` [n_i,4,4] at 30 Hz (repeated twice, :462), ``cam_intrinsics[i]`` [3,3], ``keypoints30[i]`` the detector's list: one
    [33,3] array per 30 Hz frame, None or empty where it found nothing. Such a frame becomes uniform [0,1) draws with confidence 0
    (:473-476), taken on the host from ``generator`` before the upload -- THE REFERENCE DRAWS UNSEEDED (``torch.rand``), so its files
    differ from run to run in exactly these rows; pass a seeded ``torch.Generator`` for a repeatable dictionary. Where the pose is
    shorter than the repeated cameras the cameras are cut (``preprocess_3dpwocc``; ``preprocess_3dpw`` raises there)."""
    kps = []
    for frames in keypoints30:
        rows = []
        for k in frames:
            if k is None or len(k) == 0:
                k = torch.rand(33, 3, generator=generator)
                k[:, 2] = 0.0
            rows.append(torch.as_tensor(np.asarray(k, dtype=np.float32) if not isinstance(k, torch.Tensor) else k).to(torch.float32).reshape(33, 3))
        kps.append(torch.stack(rows) if rows else torch.zeros(0, 33, 3))
    b = np.stack([np.asarray(x, dtype=np.float32).reshape(-1)[:10] for x in betas])
    ex = {"cam_K": [torch.as_tensor(np.asarray(k, dtype=np.float32)).reshape(3, 3) for k in cam_intrinsics]}
    if names is not None:
        ex["name"] = list(names)
    return prepare_camera_motions(model, poses_60hz, trans_60hz, cam_poses, b, 2, kps, False, 2, ex)


def prepare_totalcapture(model, gt_aa, imu_ori, imu_acc, vicon_hips_m, cam_K=None, cam_T=None, keypoints=None, names=None, smooth_n=2):
    """The motion part of ``preprocess_my_totalcapture_pre`` / ``preprocess_my_totalcapture`` (preprocess.py:351-364, 379-385, 429-445)
    for lists of sequences: ``gt_aa[i]`` [T,72], the real ``imu_ori[i]`` [T,6,3,3] and ``imu_acc[i]`` [T,6,3] in the file's IMU order
    (re-ordered by ``TC_IMU_ORDER``), ``vicon_hips_m[i]`` [T',3] the Vicon hip position in metres. Pose and IMU rows are clipped to their
    common length and the translation to it; root, orientations and accelerations are flipped by ``diag(-1,1,-1)`` (the root through
    a static camera with ``root_only``, the real IMU rows in torch: they are element-wise); ``tran[:,0] -= 0.03`` and
    ``tran[:,1] += 1 / (10 + tran[:,2])``. Returns a ``PreparedMotions`` in the AIST++ layout (``pose`` [T,24,3] axis-angle through
    ``body.rotation_matrix_to_axis_angle``, PARITY UNPINNED against OpenCV's ``cv2.Rodrigues`` like that function; real ``imu_ori`` /
    ``imu_acc``; ``cam_K`` [8,3,3] / ``cam_T`` [8,4,4] and ``joint2d_mp`` as given, cut to the pose). ``.extra["imu_consistency_deg"]``:
    device tensor [n], per sequence the mean ``angle_between(real, synthetic)`` in degrees -- the reference asserts < 17 (:445), here it is
    returned. The joint check of :446 needs the HUMBI body's 33 vertices and is not made."""
    dev = model.device
    order = list(TC_IMU_ORDER)
    flip = torch.tensor(TC_FLIP, dtype=torch.float32, device=dev)
    t32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32) if not isinstance(a, torch.Tensor) else a).detach().to(torch.float32)
    poses, trans, oris, accs = [], [], [], []
    for i, (p, o, a, v) in enumerate(zip(gt_aa, imu_ori, imu_acc, vicon_hips_m)):
        p, o, a, v = t32(p).reshape(-1, 72), t32(o).reshape(-1, 6, 3, 3)[:, order], t32(a).reshape(-1, 6, 3)[:, order], t32(v).reshape(-1, 3).clone()
        T = min(p.shape[0], a.shape[0])                                    # :354-358
        if v.shape[0] < T or o.shape[0] < T:
            raise ValueError(f"sequence {i}: {v.shape[0]} Vicon frames and {o.shape[0]} orientation rows for {T} pose / IMU frames")
        v = v[:T]                                                          # :379-380
        v[:, 0] = v[:, 0] - 0.03                                           # :382-383
        v[:, 1] = v[:, 1] + (1 / (10 + v[:, 2]))
        poses.append(p[:T]), trans.append(v)
        oris.append(flip @ o[:T].to(dev)), accs.append((flip @ a[:T].to(dev).unsqueeze(-1)).squeeze(-1))       # :362-364
    model.set_shape(None)
    n = len(poses)
    static = np.eye(4, dtype=np.float32)
    static[:3, :3] = np.asarray(TC_FLIP, dtype=np.float32)
    cam = prepare_camera_motions(model, poses, trans, [static] * n, None, 0, None, True, smooth_n)
    real_ori, real_acc = torch.cat(oris), torch.cat(accs)
    pose = _body.rotation_matrix_to_axis_angle(cam.posec.view(-1, 3, 3), dev).view(-1, 72)                     # :434
    ang = torch.rad2deg(_body.angle_between(real_ori.view(-1, 3, 3), cam.imu_oric.view(-1, 3, 3), dev)).view(-1, 6)
    ex = {"imu_consistency_deg": torch.stack([a.mean() for a in torch.split(ang, cam.lengths)])}              # :445, returned
    if names is not None:
        ex["name"] = list(names)
    if cam_K is not None:
        ex["cam_K"] = [torch.as_tensor(cam_K, dtype=torch.float32)] * n
    if cam_T is not None:
        ex["cam_T"] = [torch.as_tensor(cam_T, dtype=torch.float32)] * n
    if keypoints is not None:
        ex["joint2d_mp"] = [torch.stack([t32(k)[:T] for k in per]) for per, T in zip(keypoints, cam.lengths)]   # :426-427, :437
    f = {"pose": pose, "tran": cam.tranc, "joint3d": cam.joint3d, "sync_3d_mp": cam.sync_3d_mp, "imu_acc": real_acc, "imu_ori": real_ori}
    return PreparedMotions("totalcapture", cam.lengths, f, cam.vert6, cam.rest_joint, None, cam.kept, [], ex)
