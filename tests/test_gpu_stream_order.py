"""Every entry of include/robustcap_hip.h that takes a `stream`, called from a torch side stream behind a delay kernel and compared bit
for bit with the same call made alone on the default stream (tests/stream_fence.py: the fenced run, cold and warm), then the three
cross-stream promises of the header's Conventions -- distinct contexts on distinct streams are independent, sub-net calls of one context
on different streams are ordered, an eager entry makes the next live frame wait -- under the same fence.

CASES is the table tests/test_stream_cases_cpu.py checks against the header: every stream-taking entry is in a case or in EXEMPT. A case
whose `sync` is set goes through an entry the header documents to synchronise `stream` (the clause is quoted): bits only. Every other
case must, warm, also return while its stream is still held up.

Payloads are floats and byte row masks of one distribution under two seeds; everything a kernel indexes with (lengths, group sizes,
sequence tables, sample picks, row maps) is fixed per case, on the host or uploaded and synchronised before the fence, so a mis-ordered
read gives wrong numbers and never an address out of range. The live case comes last: its engine waits on device counters. The
resident layer-step kernel (rc_set_resident, off by default) has NO case: a fresh Net of 160 rows with it switched on, called from a
side stream, ended in a memory-access fault of the device at the synchronise behind its first call -- the open issue of DESIGN.md
("The abort path is not memory-safe": the second stream sharing a hardware queue with the caller's), whose cause is not established;
rc_sequence itself is covered on the other three engines."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest
import torch

import stream_fence as F
from stream_fence import Case

SEED = (0x9E3779B9 << 32) | 0x1234ABCD
NETS = ("rnn2", "rnn3", "rnn4", "rnn6", "rnn7", "rnn8")
N = 65                                                  # two blocks of 64 threads, the second with one row
GROUPS = (33, 2)                                        # evaluator groups: more than a block of 32 frames, and a short one
V_SMALL = 1025                                          # mesh vertices: four blocks of 256 and one vertex
SEQ_LENGTHS = (5, 23, 1, 9)                             # sub-net sequences
K_CAM = np.array([[600.0, 0.0, 320.0], [0.0, 600.0, 240.0], [0.0, 0.0, 1.0]], np.float32)
t = torch.from_numpy


# ------------------------------------------------------------------------------------------------------------------ shared pieces
def _lib():
    from robustcap_amd import _lib as L
    return L


@functools.lru_cache(maxsize=None)
def _assets():
    from robustcap_amd import synth
    return {"state_dict": synth.make_state_dict(0), "body": synth.make_body(1), "small": synth.make_body(1, num_vertex=V_SMALL)}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(seed, *shape, scale=1.0):
    return (scale * torch.randn(*shape, generator=_gen(seed))).cuda()


def _rot(seed, *lead, scale=0.5):
    """random rotation matrices [*lead, 3, 3], formed on the device in front of the fence"""
    from robustcap_amd import body
    n = int(np.prod(lead))
    return body.axis_angle_to_rotation_matrix(_randn(seed, n, 3, scale=scale)).view(*lead, 3, 3).contiguous()


def _kp(seed, *lead, pixels=False):
    """keypoints [*lead, 33, 3]: positions and a confidence in [0, 1)"""
    g = _gen(seed)
    xy = torch.randn(*lead, 33, 2, generator=g) * (200.0 if pixels else 0.3) + (400.0 if pixels else 0.0)
    return torch.cat([xy, torch.rand(*lead, 33, 1, generator=g)], -1).cuda().contiguous()


def _rigid(seed, n):
    """n host T_cw [n, 4, 4]: a rotation and a translation"""
    from robustcap_amd import synth
    Ts = np.zeros((n, 4, 4), np.float32)
    for i in range(n):
        Ts[i, :3, :3] = synth._rodrigues(0.4 * synth.normal(seed, 2 * i, 3).astype(np.float64))
        Ts[i, :3, 3] = synth.normal(seed, 2 * i + 1, 3) + np.array([0.0, 0.0, 3.0], np.float32)
        Ts[i, 3, 3] = 1.0
    return np.ascontiguousarray(Ts)


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


def _model(V=None, shape_space=False):
    """a ParametricModel on the shared body; V: with a V-vertex mesh (the joints depend on the seed alone)"""
    from robustcap_amd.body import ParametricModel
    m = ParametricModel(body=_assets()["body"])
    if V is not None:
        assert V == V_SMALL
        m.set_mesh(_assets()["small"]["v_template"], _assets()["small"]["weights"])
    else:
        m._ensure_mesh()
    if shape_space:
        m._ensure_shape_space()
    return m


@functools.lru_cache(maxsize=None)
def _motion(seed, B, T):
    from robustcap_amd import synth
    m = synth.make_motion(seed, B, T, _assets()["body"], conf="mixed")
    return {k: np.ascontiguousarray(m[k], np.float32) for k in ("j2dc", "accc", "oric", "gravityc")}


def _motion_inputs(B, T):
    def inputs(seed):
        m = _motion(seed, B, T)
        return [t(m[k]).cuda().contiguous() for k in ("j2dc", "accc", "oric")]
    return inputs


def _net(B, seq=None, gemm=None, T=1):
    """a Net of batch B with the weights loaded and the gravity of the REAL motion (a host setter: no payload)"""
    from robustcap_amd.net.sig_mp import Net
    net = Net(body=_assets()["body"], batch=B)
    net.load_state_dict(_assets()["state_dict"])
    if gemm is not None:
        net.set_gemm_mode(gemm)
    if seq is not None:
        net.set_sequence_mode(seq != "stepped", 8, force=seq == "wave")
    net.gravityc = t(_motion(F.REAL, B, T)["gravityc"])
    net._sync_gravity()
    return net


def _net_state(net):
    """trace and fusion state first: rc_get_state runs a pending updater step (tests/test_gpu_sequence_rows.py)"""
    out = [net.fusion_state().clone(), net.get_trace().clone()]
    for n in NETS:
        h, c = net.get_state(n)
        out += [h.clone(), c.clone()]
    return out


# ------------------------------------------------------------------------------------------------------------------ stateless ops
def _stateless():
    from robustcap_amd import body, preprocess
    L = _lib()
    none = lambda: None

    def conf_mean(_, x):
        mean, code = torch.empty(N, device="cuda"), torch.empty(N, dtype=torch.int8, device="cuda")
        L.check(None, L.load().rc_conf_mean(L.ptr(x[0]), N, 0.7, 0.8, L.ptr(mean), L.ptr(code), L.stream_ptr()), "rc_conf_mean")
        return [mean, code]

    def point_distance(_, x, mean=False):
        d, m = torch.empty(N, device="cuda"), C.c_double()
        L.check(None, L.load().rc_position_error(L.ptr(x[0]), L.ptr(x[1]), N, L.ptr(d), C.byref(m) if mean else None, L.stream_ptr()),
                "rc_position_error")
        return [d] + ([torch.tensor([m.value], dtype=torch.float64)] if mean else [])

    Tcw = _rigid(7, 1)[0]

    def camera_inputs(_, x):
        j, a, o = torch.empty(N, 33, 3, device="cuda"), torch.empty(N, 6, 3, device="cuda"), torch.empty(N, 6, 3, 3, device="cuda")
        g = np.zeros(3, np.float32)
        rc = L.load().rc_camera_inputs(L.ptr(x[0]), L.ptr(x[1]), L.ptr(x[2]), _hp(K_CAM), _hp(Tcw), L.ptr(j), L.ptr(a), L.ptr(o), _hp(g), N,
                                       L.stream_ptr())
        L.check(None, rc, "rc_camera_inputs")
        return [j, a, o, t(g.copy())]

    rows_K, rows_T = np.ascontiguousarray(np.stack([K_CAM, K_CAM * np.float32(1.1), K_CAM])), _rigid(8, 3)
    rows_K[1, 2, 2] = 1.0
    ROWS, SEQS, TMAX = 3, 2, 7

    def rows_make():
        tables = (torch.tensor([1, 0, 1], dtype=torch.int32).cuda(), torch.tensor([7, 0, 4], dtype=torch.int32).cuda())
        torch.cuda.synchronize()                                          # the row map and the lengths: on the device before the fence
        return tables

    def camera_inputs_rows(tables, x):
        j, a = torch.empty(ROWS, TMAX, 33, 3, device="cuda"), torch.empty(ROWS, TMAX, 6, 3, device="cuda")
        o, scratch = torch.empty(ROWS, TMAX, 6, 3, 3, device="cuda"), torch.empty(ROWS * 18, device="cuda")
        g = np.zeros((ROWS, 3), np.float32)
        rc = L.load().rc_camera_inputs_rows(L.ptr(x[0]), L.ptr(x[1]), L.ptr(x[2]), L.ptr(tables[0]), L.ptr(tables[1]), _hp(rows_K), _hp(rows_T),
                                            1920.0, 1080.0, ROWS, TMAX, L.ptr(j), L.ptr(a), L.ptr(o), _hp(g), L.ptr(scratch), L.stream_ptr())
        L.check(None, rc, "rc_camera_inputs_rows")
        return [j, a, o, t(g.copy())]

    return [
        Case("r6d_to_rotmat", ("rc_r6d_to_rotmat",), none, lambda s: [_randn(s, N, 6)], lambda _, x: [body.r6d_to_rotation_matrix(x[0])]),
        Case("axis_angle_to_rotmat", ("rc_axis_angle_to_rotmat",), none, lambda s: [_randn(s, N, 3)],
             lambda _, x: [body.axis_angle_to_rotation_matrix(x[0])]),
        Case("rotmat_to_axis_angle", ("rc_rotmat_to_axis_angle",), none, lambda s: [_rot(s, N)],
             lambda _, x: [body.rotation_matrix_to_axis_angle(x[0])]),
        Case("rotmat_to_r6d", ("rc_rotmat_to_r6d",), none, lambda s: [_rot(s, N)], lambda _, x: [body.rotation_matrix_to_r6d(x[0])]),
        Case("angle_between", ("rc_angle_between",), none, lambda s: [_rot(s, N), _rot(s + 1, N)],
             lambda _, x: [body.angle_between(x[0], x[1])]),
        Case("lerp", ("rc_lerp",), none, lambda s: [_randn(s, N, 7), _randn(s + 1, N, 7)], lambda _, x: [body.lerp(x[0], x[1], 0.3)]),
        Case("normalize_rows", ("rc_normalize_rows",), none, lambda s: [_randn(s, N, 5)],
             lambda _, x: list(body.normalize_tensor(x[0], return_norm=True))),
        Case("bbox_normalise", ("rc_bbox_normalise",), none, lambda s: [_kp(s, N)], lambda _, x: [body.normalize_keypoints(x[0])]),
        Case("conf_mean", ("rc_conf_mean",), none, lambda s: [_kp(s, N)], conf_mean),
        Case("point_distance", ("rc_position_error",), none, lambda s: [_randn(s, N, 3), _randn(s + 1, N, 3)], point_distance),
        Case("point_distance_host_mean", ("rc_position_error",), none, lambda s: [_randn(s, N, 3), _randn(s + 1, N, 3)],
             lambda _, x: point_distance(_, x, True), sync='rc_position_error: "if mean_host is not NULL, their mean (synchronises `stream`)"'),
        Case("procrustes", ("rc_procrustes_error",), none, lambda s: [_randn(s, N, 14, 3), _randn(s + 1, N, 14, 3)],
             lambda _, x: [body.reconstruction_error(x[0], x[1])]),
        Case("svd_rotate", ("rc_svd_rotate",), none, lambda s: [_randn(s, N, 24, 3), _randn(s + 1, N, 24, 3)],
             lambda _, x: list(body.svd_rotate(x[0], x[1], True, True, True))),
        Case("syn_acc", ("rc_syn_acc",), none, lambda s: [_randn(s, N, 18)], lambda _, x: [preprocess._syn_acc(x[0], 2)]),
        Case("camera_inputs", ("rc_camera_inputs",), none,
             lambda s: [_kp(s, N, pixels=True), _randn(s + 1, N, 6, 3), _rot(s + 2, N, 6)], camera_inputs),
        Case("camera_inputs_rows", ("rc_camera_inputs_rows",), rows_make,
             lambda s: [_kp(s, ROWS, TMAX), _randn(s + 1, SEQS, TMAX, 6, 3), _rot(s + 2, SEQS, TMAX, 6)], camera_inputs_rows,
             sync='Conventions: "rc_camera_inputs_rows once (constant upload)"'),
    ]


# ------------------------------------------------------------------------------------------------------------------ body ops
def _pose(seed, n):
    return _rot(seed, n, 24, scale=0.3)


def _body_ops():
    from robustcap_amd import preprocess
    L = _lib()
    K_dev = lambda s: (t(K_CAM) * (1.0 if s == F.REAL else 1.25)).cuda()

    def zero_pose(m, _):
        return list(m.get_zero_pose_joint_and_vertex())

    def mesh_metrics(m, x, mean=False):
        n = x[0].shape[0]
        pf, mh = torch.empty(n, 3, device="cuda"), (C.c_double * 3)()
        L.check(m._ctx, m._lib.rc_mesh_metrics(m._ctx, L.ptr(x[0]), L.ptr(x[1]), n, L.ptr(pf), mh if mean else None, L.stream_ptr()),
                "rc_mesh_metrics")
        return [pf] + ([torch.tensor(list(mh), dtype=torch.float64)] if mean else [])

    pair = lambda s: [_pose(s, sum(GROUPS)), _pose(s + 1, sum(GROUPS))]
    motion = lambda s: pair(s) + [_randn(s + 2, sum(GROUPS), 3), _randn(s + 3, sum(GROUPS), 3)]
    small = lambda: _model(V_SMALL)

    def motion_metrics(mesh):
        return lambda m, x: list(m.motion_metrics(x[0], x[1], x[2], x[3], group_frames=GROUPS, fps=30, joint_mask=0b1010, mesh=mesh))

    def aligned_metrics(mesh):
        return lambda m, x: [o for o in m.aligned_metrics(x[0], x[1], group_frames=GROUPS, align=-1, mesh=mesh, per_frame=True) if o is not None]

    return [
        Case("fk_r", ("rc_fk_r",), _model, lambda s: [_pose(s, N)], lambda m, x: [m.forward_kinematics_R(x[0])]),
        Case("ik_r", ("rc_ik_r",), _model, lambda s: [_pose(s, N)], lambda m, x: [m.inverse_kinematics_R(x[0])]),
        Case("fk_bone", ("rc_fk_bone",), _model, lambda s: [_pose(s, N)], lambda m, x: [m.bone_fk(x[0])]),
        Case("bone_to_joint", ("rc_bone_to_joint",), _model, lambda s: [_randn(s, N, 24, 3)], lambda m, x: [m.bone_vector_to_joint_position(x[0])]),
        Case("joint_to_bone", ("rc_joint_to_bone",), _model, lambda s: [_randn(s, N, 24, 3)], lambda m, x: [m.joint_position_to_bone_vector(x[0])]),
        Case("zero_pose", ("rc_zero_pose",), small, lambda s: [], zero_pose, payload=False),
        Case("body_fk", ("rc_body_fk",), _model, lambda s: [_pose(s, N), _randn(s + 1, N, 3)],
             lambda m, x: list(m.forward_kinematics(x[0], tran=x[1], calc_mesh=True))),
        Case("body_mesh", ("rc_body_mesh",), small, lambda s: [_pose(s, 5), _randn(s + 1, 5, 3)], lambda m, x: [m.forward_mesh(x[0], x[1])]),
        Case("reproj_residual", ("rc_reproj_residual",), _model,
             lambda s: [_pose(s, N), _randn(s + 1, N, 3, scale=0.2) + torch.tensor([0.0, 0.0, 3.0]).cuda(), _kp(s + 2, N, pixels=True), K_dev(s)],
             lambda m, x: [m.reprojection_residual(x[0], x[1], x[2], x[3])]),
        Case("synth_imu", ("rc_synth_imu",), _model, lambda s: [_pose(s, 7), _randn(s + 1, 7, 3)],
             lambda m, x: list(preprocess.synthesize_imu(m, x[0], x[1], smooth_n=2))),
        Case("mesh_metrics", ("rc_mesh_metrics",), small, pair, mesh_metrics),
        Case("mesh_metrics_host_mean", ("rc_mesh_metrics",), small, pair, lambda m, x: mesh_metrics(m, x, True),
             sync='rc_mesh_metrics: "mean_host ... receives the means over the n frames (synchronises `stream`)"'),
        Case("motion_metrics", ("rc_motion_metrics",), small, motion, motion_metrics(True)),
        Case("motion_metrics_no_mesh", ("rc_motion_metrics",), _model, motion, motion_metrics(False)),
        Case("aligned_metrics", ("rc_aligned_metrics",), small, pair, aligned_metrics(True)),
        Case("aligned_metrics_no_mesh", ("rc_aligned_metrics",), _model, pair, aligned_metrics(False)),
    ]


# ------------------------------------------------------------------------------------------------------------------ preparation
PREP_FRAMES = (5, 33)


def _preparation():
    from robustcap_amd import config as cfg
    L = _lib()
    n, Ft = len(PREP_FRAMES), sum(PREP_FRAMES)
    i64 = lambda v: (C.c_int64 * len(v))(*v)
    ji = (C.c_int32 * 6)(*[int(j) for j in cfg.ji_mask])
    make = lambda: _model(shape_space=True)
    outs = lambda pose_w: ([torch.empty(Ft, *pose_w, device="cuda"), torch.empty(Ft, 3, device="cuda"), torch.empty(Ft, 6, 3, 3, device="cuda"),
                            torch.empty(Ft, 6, 3, device="cuda"), torch.empty(Ft, 24, 3, device="cuda"), torch.empty(Ft, 33, 3, device="cuda"),
                            torch.empty(Ft, 6, 3, device="cuda")], torch.empty(n, 24, 3, device="cuda"))
    payload = lambda s: [_randn(s, Ft, 72, scale=0.3), _randn(s + 1, Ft, 3), _randn(s + 2, n, 10, scale=0.5)]

    def prepare_motions(m, x):
        o, rest = outs((72,))
        rc = m._lib.rc_prepare_motions(m._ctx, n, i64(PREP_FRAMES), None, Ft, L.ptr(x[0]), 24, L.ptr(x[1]), L.ptr(x[2]), None, ji, 2,
                                       *[L.ptr(a) for a in o], L.ptr(rest), L.stream_ptr())
        L.check(m._ctx, rc, "rc_prepare_motions")
        return o + [rest]

    cams = (3, 17)                                                        # 30 Hz camera rows, repeated twice: 6 and 34 frames
    cam_T = _rigid(9, sum(cams))

    def prepare_camera_motions(m, x):
        o, rest = outs((24, 3, 3))
        kp_out = torch.empty(Ft, 33, 3, device="cuda")
        rc = m._lib.rc_prepare_camera_motions(m._ctx, n, i64(PREP_FRAMES), i64(cams), 2, Ft, sum(cams), L.ptr(x[0]), L.ptr(x[1]), L.ptr(x[2]),
                                              _hp(cam_T), L.ptr(x[3]), i64(cams), sum(cams), ji, 2, 0, *[L.ptr(a) for a in o], L.ptr(kp_out),
                                              L.ptr(rest), L.stream_ptr())
        L.check(m._ctx, rc, "rc_prepare_camera_motions")
        return o + [kp_out, rest]

    return [Case("prepare_motions", ("rc_prepare_motions",), make, payload, prepare_motions),
            Case("prepare_camera_motions", ("rc_prepare_camera_motions",), make, lambda s: payload(s) + [_kp(s + 3, sum(cams))],
                 prepare_camera_motions)]


# ------------------------------------------------------------------------------------------------------------------ frame path
def _frame_path():
    L = _lib()
    B = 4

    def frames(s):
        m = _motion(s, B, 3)
        mask = torch.tensor([1, 0, 1, 0] if s == F.REAL else [0, 1, 0, 0], dtype=torch.uint8)
        return [t(np.ascontiguousarray(np.swapaxes(m[k], 0, 1))).cuda() for k in ("j2dc", "accc", "oric")] + [mask.cuda()]

    def steps(net, x):
        outs = []
        for f in range(3):
            if f == 2:
                L.check(net._ctx, net._lib.rc_reset(net._ctx, L.ptr(x[3]), L.stream_ptr()), "rc_reset")
            outs += list(net.forward_batch(x[0][f], x[1][f], x[2][f], None, f == 0))
        return outs

    def lstm_step(net, x):
        y = torch.zeros(B, 3, device="cuda")
        L.check(net._ctx, net._lib.rc_lstm_step(net._ctx, b"rnn3", L.ptr(x[0]), L.ptr(x[1]), L.ptr(y), L.stream_ptr()), "rc_lstm_step")
        return [y]

    def read_back(net, x):
        """the synchronising read-backs INSIDE the fence, behind one frame"""
        return list(net.forward_batch(x[0][0], x[1][0], x[2][0], None, True)) + _net_state(net)

    return [
        Case("reset_and_steps", ("rc_reset", "rc_step"), lambda: _net(B, T=3), frames, steps, after=_net_state),
        Case("lstm_step", ("rc_lstm_step",), lambda: _net(B, T=3),
             lambda s: [_randn(s, B, 141), torch.tensor([1, 1, 0, 1] if s == F.REAL else [0, 1, 1, 1], dtype=torch.uint8).cuda()], lstm_step,
             after=lambda net: list(net.get_state("rnn3"))),
        Case("state_read_backs", ("rc_get_state", "rc_get_trace", "rc_get_fusion_state"), lambda: _net(B, T=3), frames, read_back,
             sync='rc_get_state / rc_get_trace: "Synchronises `stream`"; rc_get_fusion_state: "Synchronises."'),
    ]


# ------------------------------------------------------------------------------------------------------------------ rc_sequence
PLANNED = 'Conventions: "rc_sequence synchronises `stream` ONCE per call when its launch planner is on AND the call has at least min_frames frames"'
ROW_LENGTHS = (1, 4, 2, 0, 3, 4, 1, 2)


def _sequence(net, x):
    return list(net.forward_sequence(x[0], x[1], x[2], first_frame=True))


def _sequence_rows(net, x):
    L = _lib()
    B, T = 8, 4
    pose, tran = torch.zeros(B, T, 24, 3, 3, device="cuda"), torch.zeros(B, T, 3, device="cuda")
    ln = np.ascontiguousarray(np.asarray(ROW_LENGTHS, np.int32))
    rc = net._lib.rc_sequence_rows(net._ctx, T, _hp(ln), L.ptr(x[0]), T * 99, L.ptr(x[1]), T * 18, L.ptr(x[2]), T * 54, None,
                                   L.RC_FLAG_FIRST_FRAME, L.ptr(pose), T * 216, L.ptr(tran), T * 3, L.stream_ptr())
    L.check(net._ctx, rc, "rc_sequence_rows")
    return [pose, tran]


def _engine_state(expect):
    """_net_state, after a look at the counters: the case ran on the engine it is named after"""
    def after(net):
        wave, stepped, _ = net.sequence_stats()
        lds, _ = net.launch_stats()
        if expect == "stepped":
            assert wave == 0 and stepped > 0
        else:
            assert wave > 0, (expect, wave, stepped)
        if expect == "shared-weight":
            assert lds > 0
        return _net_state(net)
    return after


def _sequences():
    return [
        Case("sequence_stepped", ("rc_sequence",), lambda: _net(4, "stepped", T=6), _motion_inputs(4, 6), _sequence, after=_engine_state("stepped")),
        Case("sequence_rows", ("rc_sequence_rows",), lambda: _net(8, T=4), _motion_inputs(8, 4), _sequence_rows, after=_engine_state("stepped")),
        Case("sequence_streams", ("rc_sequence",), lambda: _net(64, "wave", T=12), _motion_inputs(64, 12), _sequence, after=_engine_state("streams"),
             sync=PLANNED),
        Case("sequence_mode2", ("rc_sequence",), lambda: _net(64, "wave", gemm=2, T=12), _motion_inputs(64, 12), _sequence,
             after=_engine_state("streams"), sync=PLANNED),
        Case("sequence_shared_weight", ("rc_sequence",), lambda: _net(256, "wave", T=12), _motion_inputs(256, 12), _sequence,
             after=_engine_state("shared-weight"), sync=PLANNED),
    ]


# ------------------------------------------------------------------------------------------------------------------ training
F_SEQ = sum(SEQ_LENGTHS)
PLAN_WAIT = ('rc_subnet_forward: "the host waits only for the previous call\'s plan upload to leave the pinned buffer" -- the chain makes three '
             'sub-net calls (forward, backward, forward) on the held stream, and the second waits there for the first one\'s upload')
UPDATE = ('rc_update_subnet_weights: "Ordered after all work the context has enqueued on any stream (a device synchronise at entry) and '
          'before anything enqueued later (the call returns when its kernels on `stream` are done)"')


def _training():
    from robustcap_amd import losses, train
    from robustcap_amd.batches import SubnetDataset
    L = _lib()

    def trainer(fused):
        def make():
            net = _net(1)
            tr = net.trainable("rnn8", weight_grads="device")
            tr.train().manual_seed(SEED)
            return {"net": net, "tr": tr, "opt": tr.optimizer(lr=1e-2, clip_grad_norm=1.0) if fused else None,
                    "loss": tr.loss(pos_weight=torch.tensor([1.5, 0.7]))}
        return make

    def chain(fused):
        def call(made, x):
            """batch -> forward with dropout -> loss -> backward -> weight gradients -> step -> forward, nothing waited for"""
            net, tr, opt = made["net"], made["tr"], made["opt"]
            ds = SubnetDataset.from_buffers(tr, x[0], x[1], SEQ_LENGTHS)
            ds.set_state({"seed": SEED, "call": 5})
            xs, labels = ds.batch([2, 0, 3, 1])
            tr.zero_grad()
            ys = tr(xs)
            for y in ys:
                y.retain_grad()
            value = made["loss"](ys, labels)
            value.backward()
            params = list(tr.parameters())
            grads = [p.grad.clone() for p in params]
            if fused:
                norm = opt.step()
                extra = [norm.reshape(1)] + list(opt.exp_avg) + list(opt.exp_avg_sq)
            else:
                with torch.no_grad():
                    for p in params:
                        p.add_(p.grad, alpha=-1e-2)
                tr.commit()
                extra = []
            again = net.rnn8([a.detach() for a in xs])
            return ([torch.cat(xs).detach(), torch.cat(labels), value.detach().reshape(1), torch.cat([y.grad for y in ys])] + grads
                    + [p.detach() for p in params] + extra + [torch.cat(again)])
        return call

    corpus_payload = lambda s: [_randn(s, F_SEQ, 141), (torch.rand(F_SEQ, 2, generator=_gen(s + 1)) < 0.5).float().cuda()]

    def forward(net, x):
        outs, (h, c) = net._subnet_forward("rnn3", list(torch.split(x[0], SEQ_LENGTHS)), return_state=True)
        return [torch.cat(outs), h, c]

    def corpus_make():
        from robustcap_amd import corpus, synth
        net = _net(1)
        tr = net.trainable("rnn3")
        aist, _ = synth.make_training_dicts(6, (5, 35), _assets()["body"], 1)
        return corpus.prepare(tr, "aist", aist)

    def corpus_fields(s):
        from robustcap_amd import synth
        aist, _ = synth.make_training_dicts(s, (5, 35), _assets()["body"], 1)
        cat = lambda k, w: torch.cat([torch.as_tensor(np.asarray(a), dtype=torch.float32).reshape(-1, w) for a in aist[k]]).cuda().contiguous()
        return [cat("pose", 72), cat("imu_acc", 18), cat("imu_ori", 54), cat("joint3d", 72)]

    def corpus_call(p, x):
        for k, a in zip(("pose", "imu_acc", "imu_ori", "joint3d"), x):
            p.fields[k], p.args[k] = a, L.ptr(a)
        xo, yo = torch.empty(p.rows, p.widths[0], device="cuda"), torch.empty(p.rows, p.widths[1], device="cuda")
        L.check(p.net._ctx, p.call(xo, yo), "rc_subnet_corpus")
        return [xo, yo]

    PLAIN, WORLD = (2, 3, 3, 2, 3), (3, 2, 3)

    def parts_make():
        import subnet_batches_ref as R
        net = _net(1)
        pool = t(R.conf_pool(92, 8)).cuda().contiguous()
        return {"net": net, "tr": net.trainable("rnn4"), "pool": pool}

    def parts_payload(s):
        import subnet_batches_ref as R
        wd, wl = R.world_corpus(s, WORLD)
        return [_randn(s, sum(PLAIN), 171), _randn(s + 1, sum(PLAIN), 69), t(np.ascontiguousarray(wd, np.float32)).cuda(),
                t(np.ascontiguousarray(wl, np.float32)).cuda()]

    def parts_call(made, x):
        tr = made["tr"]
        cat = tr.concat([SubnetDataset.from_buffers(tr, x[0], x[1], PLAIN),
                         SubnetDataset.from_buffers(tr, x[2], x[3], WORLD, kind="world", conf_pool=made["pool"])])
        cat.set_state({"seed": SEED, "call": 3000000001})
        xs, labels = cat.batch([(7 * i + 1) % len(cat) for i in range(5)])
        return [torch.cat(xs), torch.cat(labels)]

    # ---- the entries of the chain one at a time: a single call holds no earlier upload back, so each must return with its stream held up
    LENS = lambda: (C.c_int32 * len(SEQ_LENGTHS))(*SEQ_LENGTHS)
    DROP = (0.4, SEED, 3)
    H8 = 512

    def batch(made, x):
        ds = SubnetDataset.from_buffers(made["tr"], x[0], x[1], SEQ_LENGTHS)
        ds.set_state({"seed": SEED, "call": 5})
        xs, labels = ds.batch([2, 0, 3, 1])
        return [torch.cat(xs), torch.cat(labels)]

    def forward_train(net, x):
        nfl = C.c_int64()
        L.check(net._ctx, net._lib.rc_subnet_tape_floats(net._ctx, b"rnn8", len(SEQ_LENGTHS), LENS(), C.byref(nfl)), "rc_subnet_tape_floats")
        y, fh, fc = torch.empty(F_SEQ, 2, device="cuda"), torch.empty(2, 4, H8, device="cuda"), torch.empty(2, 4, H8, device="cuda")
        acts, tape = torch.empty(3, F_SEQ, H8, device="cuda"), torch.empty(nfl.value, device="cuda")
        rc = net._lib.rc_subnet_forward_train(net._ctx, b"rnn8", len(SEQ_LENGTHS), LENS(), L.ptr(x[0]), L.ptr(y), None, None, L.ptr(fh), L.ptr(fc),
                                              L.ptr(acts), L.ptr(tape), *DROP, L.stream_ptr())
        L.check(net._ctx, rc, "rc_subnet_forward_train")
        return [y, fh, fc, acts, tape]

    def taped():
        net = _net(1)
        tape = forward_train(net, [_randn(7, F_SEQ, 141)])[4]
        torch.cuda.synchronize()
        return {"net": net, "tape": tape}

    def backward_train(made, x):
        net = made["net"]
        d_gates, d_a = torch.empty(2, F_SEQ, 4 * H8, device="cuda"), torch.empty(F_SEQ, H8, device="cuda")
        rc = net._lib.rc_subnet_backward_train(net._ctx, b"rnn8", len(SEQ_LENGTHS), LENS(), L.ptr(made["tape"]), L.ptr(x[0]), None, None,
                                               L.ptr(d_gates), L.ptr(d_a), None, None, *DROP, L.stream_ptr())
        L.check(net._ctx, rc, "rc_subnet_backward_train")
        return [d_gates, d_a]

    def loss_make():
        net = _net(1)
        pw = torch.tensor([1.5, 0.7]).cuda()
        torch.cuda.synchronize()
        return {"net": net, "pw": pw}

    def loss(made, x):
        net = made["net"]
        value, dx = torch.empty(1, device="cuda"), torch.empty(F_SEQ, 2, device="cuda")
        rc = net._lib.rc_subnet_loss(net._ctx, losses.KINDS["bce_logits"], L.ptr(x[0]), L.ptr(x[1]), F_SEQ, 2, L.ptr(made["pw"]), L.ptr(value),
                                     L.ptr(dx), L.stream_ptr())
        L.check(net._ctx, rc, "rc_subnet_loss")
        return [value, dx]

    def wgrad_make():
        net = _net(1)
        return {"net": net, "shapes": [tuple(p.shape) for p in net.trainable("rnn8").parameters()]}

    def weight_grads(made, x):
        net = made["net"]
        g = [torch.empty(*shape, device="cuda") for shape in made["shapes"]]
        table = (C.c_void_p * len(g))(*[a.data_ptr() for a in g])
        rc = net._lib.rc_subnet_weight_grads(net._ctx, b"rnn8", len(SEQ_LENGTHS), LENS(), L.ptr(x[0]), L.ptr(x[1]), None, L.ptr(x[2]), L.ptr(x[3]),
                                             L.ptr(x[4]), *DROP, table, L.stream_ptr())
        L.check(net._ctx, rc, "rc_subnet_weight_grads")
        return g

    def step_make():
        made = trainer(True)()
        made["opt"]._ensure_moments()                                      # (zeros: allocated in front of the fence)
        torch.cuda.synchronize()
        return made

    def step_payload(s):
        return [_randn(s + i, *shape, scale=1e-2) for i, shape in enumerate(wgrad_shapes())]

    @functools.lru_cache(maxsize=None)
    def wgrad_shapes():
        from robustcap_amd import config as cfg
        return tuple(tuple(shape) for k, shape in cfg.state_dict_spec() if k.startswith("rnn8."))

    def optim_step(made, x):
        params = list(made["tr"].parameters())
        for p, g in zip(params, x):
            p.grad = g
        norm = made["opt"].step()
        return [norm.reshape(1), made["opt"].last_norm_and_coef] + [p.detach() for p in params] + list(made["opt"].exp_avg) + list(made["opt"].exp_avg_sq)

    singles = [
        Case("subnet_batch", ("rc_subnet_batch",), trainer(False), corpus_payload, batch),
        Case("subnet_forward_train", ("rc_subnet_forward_train",), lambda: _net(1), lambda s: [_randn(s, F_SEQ, 141)], forward_train),
        Case("subnet_backward_train", ("rc_subnet_backward_train",), taped, lambda s: [_randn(s, F_SEQ, H8)], backward_train),
        Case("subnet_loss", ("rc_subnet_loss",), loss_make, lambda s: [_randn(s, F_SEQ, 2), corpus_payload(s)[1]], loss),
        Case("subnet_weight_grads", ("rc_subnet_weight_grads",), wgrad_make,
             lambda s: [_randn(s, F_SEQ, 141), _randn(s + 1, 3, F_SEQ, H8), _randn(s + 2, F_SEQ, 2), _randn(s + 3, 2, F_SEQ, 4 * H8),
                        _randn(s + 4, F_SEQ, H8)], weight_grads),
        Case("subnet_optim_step", ("rc_subnet_optim_step",), step_make, step_payload, optim_step),
    ]

    return singles + [
        Case("train_chain", ("rc_subnet_batch", "rc_subnet_forward_train", "rc_subnet_loss", "rc_subnet_backward_train", "rc_dropout_apply",
                             "rc_subnet_weight_grads", "rc_subnet_optim_step", "rc_subnet_forward"), trainer(True), corpus_payload, chain(True),
             sync=PLAN_WAIT),
        Case("train_chain_update_weights", ("rc_subnet_batch", "rc_subnet_forward_train", "rc_subnet_loss", "rc_subnet_backward_train",
                                            "rc_subnet_weight_grads", "rc_update_subnet_weights", "rc_subnet_forward"),
             trainer(False), corpus_payload, chain(False), sync=UPDATE),
        Case("subnet_forward", ("rc_subnet_forward",), lambda: _net(1), lambda s: [_randn(s, F_SEQ, 141)], forward),
        Case("init_net_forward", ("rc_init_net_forward",), lambda: _net(1), lambda s: [_randn(s, 2, 69)], lambda net, x: [net._init_net_forward(x[0])]),
        Case("subnet_eval", ("rc_subnet_eval",), lambda: losses.SubnetEval(_net(1), "mse", width=3),
             lambda s: [_randn(s, 34, 3), _randn(s + 1, 34, 3)], lambda ev, x: [ev(x[0], x[1], group_sizes=[1, 33])]),
        Case("dropout_apply", ("rc_dropout_apply",), lambda: _net(1), lambda s: [_randn(s, N, 512)],
             lambda net, x: [train.dropout_apply(net, x[0], 0, (0.4, SEED, 7))]),
        Case("subnet_corpus", ("rc_subnet_corpus",), corpus_make, corpus_fields, corpus_call),
        Case("subnet_batch_parts", ("rc_subnet_batch_parts",), parts_make, parts_payload, parts_call),
    ]


# ------------------------------------------------------------------------------------------------------------------ smplify
SMPLIFY = 'Conventions: "rc_smplify_* as documented with them" (rc_smplify_loss_grad: "Synchronises `stream`"; the runs read back every round)'


@functools.lru_cache(maxsize=None)
def _fk_model():
    return _model()


def _smplify():
    from robustcap_amd import body, synth
    from robustcap_amd.smplify import TemporalSMPLify
    make = lambda: TemporalSMPLify(body=_assets()["body"], gmm=synth.make_gmm(3))

    def scene(s, T):
        """(axis-angle pose, rotation matrices, translation, pixel keypoints, landmarks, IMU orientations) of T frames"""
        aa = _randn(s, T, 72, scale=0.35)
        R = body.axis_angle_to_rotation_matrix(aa.view(-1, 3)).view(T, 24, 3, 3)
        tran = _randn(s + 1, T, 3, scale=0.2) + torch.tensor([0.1, -0.2, 3.0]).cuda()
        _, _, mj = _fk_model().forward_kinematics(R, tran=tran, calc_mesh=True)
        proj = (t(K_CAM).cuda() @ (mj / mj[..., 2:]).unsqueeze(-1)).squeeze(-1)[..., :2]
        kp = torch.cat([proj + _randn(s + 2, T, 33, 2, scale=5.0), torch.rand(T, 33, 1, generator=_gen(s + 3)).cuda()], -1).contiguous()
        return aa, R.contiguous(), tran, kp, (mj + _randn(s + 4, T, 33, 3, scale=0.05)).contiguous(), _rot(s + 5, T, 6)

    def closure_inputs(T):
        def inputs(s):
            aa, _, tran, kp, ref3d, ori = scene(s, T)
            return [aa, tran, kp, ref3d, body.rotation_matrix_to_axis_angle(ori.view(-1, 3, 3)).view(T, 18).contiguous()]
        return inputs

    def closure(r, x):
        loss, gp, gt = r.loss_and_grad(x[0], x[1], x[2], x[3], x[4], K_CAM)
        return [gp, gt, torch.tensor([loss], dtype=torch.float64)]

    def info(d):
        return torch.tensor([d["status"], d["n_iter"], d["n_eval"], d["first_loss"], d["final_loss"]], dtype=torch.float64)

    def upd(u, T):
        return torch.zeros(T, dtype=torch.bool) if u is None else u

    def run_inputs(s):
        _, R, tran, kp, _, ori = scene(s, 3)
        return [R, tran, kp, ori]

    def run(r, x):
        p, tr, u = r.run(x[0], x[1], x[2], x[3], K_CAM, lr=0.001, max_iter=3)
        return [p, tr, upd(u, 3), info(r.last_info)]

    def run_batch(r, x):
        out = r.run_batch([(x[0], x[1], x[2], x[3], K_CAM), (x[4], x[5], x[6], x[7], K_CAM * np.float32(1.0))], lr=0.001, max_iter=3)
        res = []
        for (p, tr, u), d in zip(out, r.last_batch_info):
            res += [p, tr, upd(u, 3), info(d)]
        return res

    return [
        Case("smplify_loss_grad_2", ("rc_smplify_loss_grad",), make, closure_inputs(2), closure, sync=SMPLIFY),
        Case("smplify_loss_grad_65", ("rc_smplify_loss_grad",), make, closure_inputs(N), closure, sync=SMPLIFY),
        Case("smplify_run", ("rc_smplify_run",), make, run_inputs, run, sync=SMPLIFY),
        Case("smplify_run_batch", ("rc_smplify_run_batch",), make, lambda s: run_inputs(s) + run_inputs(s + 10), run_batch, sync=SMPLIFY),
    ]


def _cases():
    return _stateless() + _body_ops() + _preparation() + _frame_path() + _sequences() + _training() + _smplify()


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
# Entries with a stream parameter that no case calls: only what wraps an entry of a case, and the diagnostic probe.
EXEMPT = {
    "rc_subnet_forward_tape": "rc_subnet_forward_train with p == 0 IS this entry (header): one function behind both, run by train_chain",
    "rc_subnet_backward": "rc_subnet_backward_train with p == 0 IS this entry (header): one function behind both, run by train_chain",
    "rc_lbfgs_device_probe": "DIAGNOSTIC (header): the backends of rc_smplify_run / rc_smplify_run_batch on a synthetic closure; "
                             "both are cases, and the probe synchronises `stream`",
}

pytestmark = pytest.mark.gpu
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    """The model, the motions and the references that the tests of this module share are released with its last test."""
    yield
    _REF.clear()
    for cached in (_fk_model, _motion):
        cached.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


class _Recorded:
    """While it lives, every stream-taking entry of the library that is called is noted by name (the loaded library is one object, shared
    by every wrapper): what a case's `entries` declare is checked against what its call reaches."""

    def __init__(self):
        self.lib, self.called, self.saved = _lib().load(), set(), {}

    def __enter__(self):
        import test_stream_cases_cpu as H
        for name in H._stream_entries():
            fn = getattr(self.lib, name)
            self.saved[name] = fn
            setattr(self.lib, name, functools.partial(self._note, name, fn))
        return self

    def _note(self, name, fn, *args):
        self.called.add(name)
        return fn(*args)

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.lib, name, fn)


def _reference(case):
    if case.name not in _REF:
        with _Recorded() as rec:
            _REF[case.name] = F.reference(case)
        missing = sorted(set(case.entries) - rec.called)
        assert not missing, (case.name, "declared in `entries` but never called", missing)
    return _REF[case.name]


@pytest.mark.parametrize("variant", F.VARIANTS)
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_fenced(name, variant):
    case = BY_NAME[name]
    F.run_case(case, variant, _reference(case))
    if variant == F.VARIANTS[-1]:
        _REF.pop(name, None)                                              # (the payloads and references of a finished case are released)
        gc.collect()


# ------------------------------------------------------------------------------------------------------------------ cross-stream promises
def _alone(case, payloads):
    """the outputs of call(p) for p in payloads, one after the other on a fresh context on the default stream"""
    made = case.make()
    torch.cuda.synchronize()
    want = []
    for p in payloads:
        outs = case.call(made, p)
        torch.cuda.synchronize()
        want.append([o.clone() for o in outs])
    want.append([a.clone() for a in case.after(made)] if case.after else [])
    del made
    return want


def _through(case, made, x, src, junk):
    """x <- src, the call, clones of its outputs, x <- junk: all on the current stream"""
    for a, b in zip(x, src):
        a.copy_(b)
    outs = case.call(made, x)
    kept = [o.clone() for o in outs]
    for a, b in zip(x, junk):
        a.copy_(b)
    return kept


def test_two_contexts_on_two_streams_are_independent():
    """"distinct contexts on distinct streams are independent": a ParametricModel (rc_aligned_metrics) and a Net of four rows
    (rc_sequence), each on a side stream of its own behind a delay of its own, their calls interleaved A, B, A, B with no
    synchronisation; every output is that context's run alone."""
    cases = [BY_NAME["aligned_metrics"], BY_NAME["sequence_stepped"]]
    pay = [[c.inputs(F.REAL), c.inputs(F.DECOY)] for c in cases]
    want = [_alone(c, p) for c, p in zip(cases, pay)]
    made = [c.make() for c in cases]
    cases[0].call(made[0], pay[0][1])                                      # (the model's first call folds the mesh and synchronises the device: header)
    x = [[a.clone() for a in p[1]] for p in pay]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    got, evs = [[], []], []
    for s in streams:
        with torch.cuda.stream(s):
            evs.append(F.hold(s, 100.0))
    for k in range(2):
        for i, c in enumerate(cases):
            with torch.cuda.stream(streams[i]):
                got[i].append(_through(c, made[i], x[i], pay[i][k], pay[i][1 - k]))
    held = [not e.query() for e in evs]
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()
    F.report(f"two contexts, two streams: delay 100.0 ms each, held {held}")
    for i, c in enumerate(cases):
        for k in range(2):
            F.assert_same(got[i][k], want[i][k], (c.name, "call", k))
        if c.after:
            F.assert_same([a.clone() for a in c.after(made[i])], want[i][2], (c.name, "state"))
    assert all(held), ("a call returned only after its stream's delay (rc_aligned_metrics, unplanned rc_sequence)", held)


def _one_context_two_streams(case, caller_orders):
    pay = [case.inputs(F.REAL), case.inputs(F.DECOY)]
    want = _alone(case, [pay[1], pay[0], pay[1]])                          # (a warm-up call first: no scratch grows inside the fence)
    made = case.make()
    torch.cuda.synchronize()
    case.call(made, pay[1])
    torch.cuda.synchronize()
    x = [[a.clone() for a in pay[1]], [a.clone() for a in pay[0]]]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        ev = F.hold(s1, 100.0)
        got1 = _through(case, made, x[0], pay[0], pay[1])
    if caller_orders:
        s2.wait_stream(s1)
    with torch.cuda.stream(s2):
        got2 = _through(case, made, x[1], pay[1], pay[0])
    held = not ev.query()
    s1.synchronize()
    s2.synchronize()
    torch.cuda.synchronize()
    F.report(f"one context, two streams ({case.name}, {'the caller orders them' if caller_orders else 'ordered by the entry'}): delay 100.0 ms, held {held}")
    F.assert_same(got1, want[1], (case.name, "call on the first stream"))
    F.assert_same(got2, want[2], (case.name, "call on the second stream"))
    assert held, (case.name, "the calls returned only after the first stream's delay")


LONG, SHORT = 257, 5                                    # frames of one sequence: hundreds of dependent steps of device time | a short enqueue


def test_subnet_forward_on_two_streams_is_ordered_by_the_entry():
    """rc_subnet_forward: "Calls on different streams are ordered: a call waits for the previous call's work, whose scratch it reuses".
    Call 1, one sequence of 257 dependent steps, goes on s1 behind a delay; call 2, five frames of other inputs, on s2 straight after.
    The host side of call 2 waits for call 1's plan upload (the same paragraph), which the delay keeps back: it is enqueued when the delay
    has just run out and call 1 is at work on the scratch -- the event behind call 1's outputs has not fired when call 2 has returned."""
    net = _net(1)

    def call(x):
        outs, (h, c) = net._subnet_forward("rnn3", [x], return_state=True)
        return [outs[0], h, c]

    long_in, short_in = _randn(F.REAL, LONG, 141), _randn(F.DECOY, SHORT, 141)
    junk = [_randn(F.DECOY + 1, LONG, 141), _randn(F.REAL + 1, SHORT, 141)]
    torch.cuda.synchronize()
    want = []
    for p in (long_in, short_in, long_in, short_in):                       # (the first pair grows the scratch: not inside the fence)
        outs = call(p)
        torch.cuda.synchronize()
        want.append([o.clone() for o in outs])
    x = [junk[0].clone(), junk[1].clone()]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        F.hold(s1, 50.0)
        x[0].copy_(long_in)
        got1 = [o.clone() for o in call(x[0])]
        done1 = s1.record_event()
        x[0].copy_(junk[0])
    with torch.cuda.stream(s2):
        x[1].copy_(short_in)
        outs2 = call(x[1])
        pending = not done1.query()
        got2 = [o.clone() for o in outs2]
        x[1].copy_(junk[1])
    s1.synchronize()
    s2.synchronize()
    torch.cuda.synchronize()
    F.report(f"one context, two streams (rc_subnet_forward, ordered by the entry): delay 50.0 ms, call 1 pending when call 2 returned {pending}")
    F.assert_same(got1, want[2], "rc_subnet_forward on the first stream")
    F.assert_same(got2, want[3], "rc_subnet_forward on the second stream")
    assert pending, "call 1 had finished before call 2 was enqueued: the order was not put to the test"


@pytest.mark.parametrize("name", ["subnet_loss", "subnet_eval", "motion_metrics_no_mesh"])
def test_shared_scratch_on_two_streams_ordered_by_the_caller(name):
    """rc_subnet_loss, rc_subnet_eval, rc_motion_metrics: "a caller who uses a second stream orders it itself" -- with s2.wait_stream(s1) and nothing else"""
    _one_context_two_streams(BY_NAME[name], True)


def test_an_eager_reset_makes_the_next_live_frame_wait():
    """"the next live frame waits for the work just enqueued": a live session of one row, two frames, rc_reset(row_mask) on a side
    stream behind a delay and rc_live_step straight after it; the frames that follow equal those of the same session with the reset on the
    default stream -- and differ from those of a session with no reset at all, so the reset is seen. rc_reset itself returns while its
    stream is held up (the fence is real); the live step behind it returns only when the delay has run out (it did wait)."""
    L = _lib()
    m = _motion(F.REAL, 1, 4)
    frames = [[t(m[k][:, f]).contiguous() for k in ("j2dc", "accc", "oric")] for f in range(4)]
    mask = torch.ones(1, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()

    def session(reset, stream=None):
        net = _net(1, T=4)
        outs, held = [], None
        for f in range(4):
            if f == 2 and reset:
                if stream is None:
                    L.check(net._ctx, net._lib.rc_reset(net._ctx, L.ptr(mask), L.stream_ptr()), "rc_reset")
                else:
                    with torch.cuda.stream(stream):
                        ev = F.hold(stream, 50.0)
                        L.check(net._ctx, net._lib.rc_reset(net._ctx, L.ptr(mask), L.stream_ptr()), "rc_reset")
                        held = [not ev.query()]
            outs += [o.clone() for o in net.forward_live(*frames[f], first_frame=f == 0)]
            if f == 2 and held:
                held.append(not ev.query())
        lean, aql, note = C.c_int32(), C.c_int32(), C.create_string_buffer(256)
        L.check(net._ctx, net._lib.rc_get_live_backend(net._ctx, C.byref(lean), C.byref(aql), note, 256), "rc_get_live_backend")
        torch.cuda.synchronize()
        return outs + _net_state(net), (lean.value, aql.value, note.value.decode(errors="replace")), held

    want, _, _ = session(True)
    plain, _, _ = session(False)
    assert any(not F.same_bits(a, b) for a, b in zip(plain[4:8], want[4:8])), "the reset changes nothing in the frames behind it: nothing is tested"
    got, backend, held = session(True, torch.cuda.Stream())
    F.report(f"eager then live: delay 50.0 ms, held when rc_reset returned {held[0]}, when rc_live_step returned {held[1]}, "
             f"backend lean {backend[0]} aql {backend[1]} {backend[2]!r}")
    F.assert_same(got, want, "live frames behind a reset on a side stream")
    assert held[0], "rc_reset returned only after its stream's delay"
    assert not held[1], "rc_live_step returned while the reset in front of it was still held up"
