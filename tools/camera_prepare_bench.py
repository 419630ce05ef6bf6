"""What preparing 3DPW-style camera-frame motions costs: ONE rc_prepare_camera_motions call for all persons
(robustcap_amd/preprocess.prepare_camera_motions, csrc/rc_prepare.hip: rc_cam_frame_kernel) beside the route the project had before it, the
reference's recipe in torch, and rc_prepare_motions on the same frame count.

    python tools/camera_prepare_bench.py [--small] [--out profiles/camera_prepare_bench.txt]

Workloads (seeded random walks, only the shapes matter): 64 persons x 1,200 frames at 60 Hz with 64 shapes, 600 camera poses and 600
detector frames each (cam_repeat 2); and 8 x 600. Every candidate is warmed on its shape first; (a), (d) and (e) alternate in one process,
INNER calls per timed window between two HIP events, the median of the REPS windows is reported per call.
  (a) rc_prepare_camera_motions, the C entry itself on buffers made beforehand (inside the events: the host check and the staging of
      the camera rows, the table uploads and the four launches), with its bytes counted from the shapes against 6.3 TB/s: per output
      frame 288 + 12 B pose and translation, 48 B camera row and 198 B detections in (each read once per frame that uses it), 864 + 12 + 216 + 288 + 396 + 72 + 72 +
      396 B out, plus the 72 B the stencil reads back.
  (b) the route of the parent commit, per person: axis_angle_to_rotation_matrix, the torch root / translation transform under the
      repeated cameras, ParametricModel.set_shape, synthesize_imu, forward_mesh[:, mp_mask] and the torch interleave; wall clock ending
      in a synchronise (set_shape synchronises by itself).
  (c) the reference's recipe in torch (preprocess.py:571-599: full-mesh shape blend, J_regressor @ v, the 4 x 4 chain, the blend of the
      transforms over all vertices, _syn_acc, the interleave loop) on the host with 16 threads, measured on 2 persons and scaled by frames.
  (d) rc_prepare_motions, the C entry likewise (24 joints, one shape per sequence, no alignment), on the same frames: the yardstick for
      the lighter frame kernel.
  (e) preprocess.prepare_camera_motions, the Python wrapper around (a) on lists of per-person device tensors: its torch.cat of the
      lists, the numpy handling of the camera rows, the per-person ``cam_T`` views and nine torch.empty calls are host work in front of
      the entry.
No thresholds."""
import ctypes as C
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--small", action="store_true", help="an eighth of the persons (a quick look)")
ap.add_argument("--out", help="also append the lines to this file")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from robustcap_amd import body as B  # noqa: E402
from robustcap_amd import config as cfg  # noqa: E402
from robustcap_amd import _lib, preprocess, synth  # noqa: E402

REPS, INNER, HBM_BYTES_PER_S, HOST_SEQ = 7, 20, 6.3e12, 2
PARENT = cfg.smpl_parent
BYTES_PER_FRAME = 288 + 12 + 48 + 198 + 864 + 12 + 216 + 288 + 396 + 72 + 72 + 396 + 72


def say(line):
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def event_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t)


def inputs(seed, n, T):
    g = np.random.default_rng(seed)
    poses = [(np.cumsum(0.02 * g.standard_normal((T, 24, 3)), 0) + 0.3 * g.standard_normal((24, 3))).astype(np.float32) for _ in range(n)]
    trans = [np.cumsum(0.01 * g.standard_normal((T, 3)), 0).astype(np.float32) for _ in range(n)]
    betas = (4 * g.random((n, 10)) - 2).astype(np.float32)
    cams = []
    for _ in range(n):
        c = np.zeros((T // 2, 4, 4), np.float32)
        c[:, :3, :3] = synth._rodrigues(np.array([1.7, -0.9, 0.5]) + np.cumsum(0.01 * g.standard_normal((T // 2, 3)), 0)).astype(np.float32)
        c[:, :3, 3] = (np.array([0.3, -1.1, 4.2]) + np.cumsum(0.01 * g.standard_normal((T // 2, 3)), 0)).astype(np.float32)
        c[:, 3, 3] = 1
        cams.append(c)
    kps = [g.random((T // 2, 33, 3)).astype(np.float32) for _ in range(n)]
    return poses, trans, betas, cams, kps


def interleave_torch(kp, T):
    """preprocess.py:477-483 vectorised: [k,33,3] -> [T,33,3]"""
    nxt = torch.cat([kp[1:], kp[-1:]])
    mid = (nxt + kp) / 2.0
    mid[-1] = kp[-1]
    return torch.stack([kp, mid], 1).reshape(-1, 33, 3)[:T]


# ---- (b) the route of the parent commit ---------------------------------------------------------------------------------------------------
def old_way(model, poses, trans, betas, cams, kps):
    mp = torch.tensor(cfg.mp_mask, device=model.device)
    out = []
    for p, t, b, c, k in zip(poses, trans, betas, cams, kps):
        T = min(p.shape[0], 2 * c.shape[0])
        rows = c.repeat_interleave(2, dim=0)[:T]
        R = B.axis_angle_to_rotation_matrix(p[:T].reshape(-1, 3)).view(-1, 24, 3, 3)
        R[:, 0] = rows[:, :3, :3] @ R[:, 0]
        tc = (rows[:, :3, :3] @ t[:T].unsqueeze(-1)).squeeze(-1) + rows[:, :3, 3]
        model.set_shape(b)
        ori, acc, joint, _ = preprocess.synthesize_imu(model, R, tc)
        out.append((R, tc, ori, acc, joint, model.forward_mesh(R, tc)[:, mp], interleave_torch(k, T)))
    return out


# ---- (c) the reference's recipe in torch, full mesh, on the host ------------------------------------------------------------------------------
def torch_recipe(c, p, beta, t, cam, kp):
    T = min(p.shape[0], 2 * cam.shape[0])
    rows = cam.repeat_interleave(2, dim=0)[:T]
    a = p[:T].reshape(-1, 3)
    th = a.norm(dim=1, keepdim=True)
    k = a / th
    k[~torch.isfinite(k)] = 0
    K = torch.zeros(a.shape[0], 3, 3)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
    cs, sn = th.cos().view(-1, 1, 1), th.sin().view(-1, 1, 1)
    R = (cs * torch.eye(3) + (1 - cs) * k.unsqueeze(2) * k.unsqueeze(1) + sn * K).view(T, 24, 3, 3)
    R[:, 0] = rows[:, :3, :3] @ R[:, 0]
    tc = (rows @ torch.cat([t[:T], torch.ones(T, 1)], 1).unsqueeze(-1)).squeeze(-1)[:, :3]
    v = torch.tensordot(beta.view(1, 10), c["sd"], dims=([1], [2]))[0] + c["vt"]
    j = c["Jr"] @ v
    j, v = j - j[:1], v - j[:1]
    bone = torch.cat([j[:1], j[1:] - j[c["parent"][1:]]])
    Tl = torch.zeros(T, 24, 4, 4)
    Tl[:, :, :3, :3], Tl[:, :, :3, 3], Tl[:, :, 3, 3] = R, bone, 1
    Tg = [Tl[:, 0]]
    for i in range(1, 24):
        Tg.append(Tg[PARENT[i]] @ Tl[:, i])
    Tg = torch.stack(Tg, 1)
    grot, joint = Tg[:, :, :3, :3].clone(), Tg[:, :, :3, 3] + tc[:, None]
    Tg[..., -1:] -= Tg @ torch.cat([j, torch.zeros(24, 1)], 1).unsqueeze(-1)
    Tv = torch.tensordot(Tg, c["w"], dims=([1], [1])).permute(0, 3, 1, 2)
    vert = (Tv @ torch.cat([v, torch.ones(v.shape[0], 1)], 1).unsqueeze(-1)).squeeze(-1)[..., :3] + tc[:, None]
    v6 = vert[:, c["vi"]]
    acc = torch.zeros_like(v6)
    acc[1:-1] = (v6[:-2] + v6[2:] - 2 * v6[1:-1]) * 3600
    acc[2:-2] = (v6[:-4] + v6[4:] - 2 * v6[2:-2]) * 3600 / 4
    joint_2d = []
    for index in range(len(kp)):                                                                    # the reference's own loop
        if index == len(kp) - 1:
            joint_2d.append(kp[index])
            joint_2d.append(kp[index])
            continue
        joint_2d.append(kp[index])
        joint_2d.append((kp[index + 1] + kp[index]) / 2.0)
    return joint, vert[:, c["mp"]], acc, grot[:, c["ji"]], torch.stack(joint_2d)[:T]


def body_tensors(body):
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32))
    return {"vt": t(body["v_template"]), "sd": t(body["shapedirs"])[:, :, :10], "Jr": t(body["J_regressor"]), "w": t(body["weights"]),
            "parent": torch.tensor([0] + list(PARENT[1:])), "mp": torch.tensor(cfg.mp_mask), "vi": torch.tensor(cfg.vi_mask),
            "ji": torch.tensor(cfg.ji_mask)}


def case(label, body, model, n, T):
    poses, trans, betas, cams, kps = inputs(11, n, T)
    dev = model.device
    frames = n * T
    pd, td = [torch.from_numpy(p).to(dev) for p in poses], [torch.from_numpy(t).to(dev) for t in trans]
    cd, kd = [torch.from_numpy(c).to(dev) for c in cams], [torch.from_numpy(k).to(dev) for k in kps]
    bd = torch.from_numpy(betas)
    pose_all, tran_all = torch.cat(pd), torch.cat(td)

    def wrapper():
        return preprocess.prepare_camera_motions(model, pd, td, cams, betas, 2, kd)

    # the two C entries on buffers made once
    model._ensure_shape_space()
    lib, ctx, st = model._lib, model._ctx, _lib.stream_ptr()
    beta_d, kp_all, cam_all = bd.to(dev), torch.cat(kd), np.ascontiguousarray(np.concatenate(cams))
    o = {k: torch.empty(frames, w, device=dev) for k, w in (("posec", 216), ("pose", 72), ("tran", 3), ("ori", 54), ("acc", 18), ("joint", 72),
                                                            ("sync", 99), ("vert6", 18), ("kp", 99))}
    rest = torch.empty(n, 72, device=dev)
    i64 = lambda v: (C.c_int64 * n)(*[int(x) for x in v])
    jid = (C.c_int32 * 6)(*[int(j) for j in cfg.ji_mask])
    in_f, cam_f, kp_f = i64([T] * n), i64([T // 2] * n), i64([T // 2] * n)

    def new_way():
        rc = lib.rc_prepare_camera_motions(ctx, n, in_f, cam_f, 2, frames, frames // 2, _lib.ptr(pose_all), _lib.ptr(tran_all), _lib.ptr(beta_d),
                                           cam_all.ctypes.data_as(C.c_void_p), _lib.ptr(kp_all), kp_f, frames // 2, jid, 2, 0, _lib.ptr(o["posec"]),
                                           _lib.ptr(o["tran"]), _lib.ptr(o["ori"]), _lib.ptr(o["acc"]), _lib.ptr(o["joint"]), _lib.ptr(o["sync"]),
                                           _lib.ptr(o["vert6"]), _lib.ptr(o["kp"]), _lib.ptr(rest), st)
        _lib.check(ctx, rc, "rc_prepare_camera_motions")

    def yardstick():
        rc = lib.rc_prepare_motions(ctx, n, in_f, None, frames, _lib.ptr(pose_all), 24, _lib.ptr(tran_all), _lib.ptr(beta_d), None, jid, 2,
                                    _lib.ptr(o["pose"]), _lib.ptr(o["tran"]), _lib.ptr(o["ori"]), _lib.ptr(o["acc"]), _lib.ptr(o["joint"]),
                                    _lib.ptr(o["sync"]), _lib.ptr(o["vert6"]), _lib.ptr(rest), st)
        _lib.check(ctx, rc, "rc_prepare_motions")

    new_way(), yardstick(), wrapper(), old_way(model, pd[:2], td[:2], bd[:2], cd[:2], kd[:2])       # warm all on their shapes
    t_a, t_d, t_e, t_b = [], [], [], []
    for _ in range(REPS):                                                                           # alternated in one process
        t_a.append(event_ms(new_way, INNER))
        t_d.append(event_ms(yardstick, INNER))
        t_e.append(event_ms(wrapper, INNER))
    for _ in range(3):
        t_b.append(wall_ms(lambda: old_way(model, pd, td, bd, cd, kd)))
    model.set_shape(None)
    spread = lambda v: f"{min(v):.3f} .. {max(v):.3f}"
    a, d, e, b = statistics.median(t_a), statistics.median(t_d), statistics.median(t_e), statistics.median(t_b)
    nbytes = frames * BYTES_PER_FRAME + n * 4 * (10 + 72)
    say(f"{label}: {n} persons x {T} frames, one shape per person, {T // 2} camera poses and detector frames each: "
        f"(a) rc_prepare_camera_motions {a:8.3f} per call ({spread(t_a)} over {REPS} windows of {INNER} calls): counted {nbytes / 1e6:6.1f} MB = "
        f"{100 * nbytes / (a * 1e-3) / HBM_BYTES_PER_S:5.1f} % of 6.3 TB/s ({1e6 * a / frames:6.1f} ns per frame, {BYTES_PER_FRAME} B per frame)")
    say(f"{label}: (d) rc_prepare_motions on the same {frames} frames {d:8.3f} per call ({spread(t_d)}) = {d / a:5.2f} x (a) "
        f"({1e6 * d / frames:6.1f} ns per frame)")
    say(f"{label}: (e) preprocess.prepare_camera_motions, the wrapper on per-person lists {e:8.3f} per call ({spread(t_e)}) = {e / a:5.2f} x (a)")
    say(f"{label}: (b) per person set_shape + torch root / translation + synthesize_imu + forward_mesh[:, mp_mask] + torch interleave "
        f"{b:9.2f} ({spread(t_b)}) = {b / a:7.1f} x (a)")
    torch.set_num_threads(16)
    ch = body_tensors(body)
    nh = min(HOST_SEQ, n)
    hp, ht, hc, hk = [torch.from_numpy(p).reshape(T, 72) for p in poses[:nh]], [torch.from_numpy(t) for t in trans[:nh]], \
        [torch.from_numpy(c) for c in cams[:nh]], [torch.from_numpy(k) for k in kps[:nh]]

    def host():
        return [torch_recipe(ch, hp[i], bd[i], ht[i], hc[i], hk[i]) for i in range(nh)]

    ref = host()
    t_h = statistics.median([wall_ms(host) for _ in range(3)]) * n / nh
    p_new = wrapper()
    diff = max(float((ref[0][0].to(dev) - p_new.joint3d[:T]).abs().max()), float((ref[0][1].to(dev) - p_new.sync_3d_mp[:T]).abs().max()),
               float((ref[0][3].to(dev) - p_new.imu_oric[:T]).abs().max()), float((ref[0][4].to(dev) - p_new.joint2d_mp[:T]).abs().max()))
    say(f"{label}: (c) the reference's recipe in torch, full mesh, on the host with 16 threads, scaled from {nh} persons {t_h:10.1f} = "
        f"{t_h / a:8.1f} x (a)  |  max |(c) - (a)| over joints, landmarks, orientations, keypoints of person 0: {diff:.2e}")


def main():
    body = synth.make_body(1)
    model = B.ParametricModel(body=body)
    k = 8 if args.small else 1
    say("# camera_prepare_bench: HIP events for (a) and (d), wall clock ending in a synchronise for (b) and (c); medians; ms")
    for run in (1, 2):
        say(f"# run {run}")
        case("pw3d", body, model, 64 // k, 1200)
        case("pw3d-small", body, model, max(8 // k, 2), 600)


if __name__ == "__main__":
    main()
