"""Camera-frame motions on the device (preprocess.prepare_camera_motions: rc_prepare_camera_motions, csrc/rc_prepare.hip) against the
numpy restatement tests/camera_motion_ref.py of preprocess.py:460-470, 477-483 and against the reference's own numbers
(tests/golden/camera), and the evaluation harness on the camera-frame layout.

Six ragged sequences. (a) .. (e) are moving-camera sequences in one call with cam_repeat 2:

        in   cam  out  detector
    a    5    3    5    3     the 2 smooth_n + 1 minimum; an odd end frame on a camera row used once
    b    7    3    6    3     the pose longer than the cameras; the last detector frame twice
    c   30   13   26   13     the same with neighbours on both sides
    d  131   66  131   66     more than 64 frames
    e   14    7   14    7

(d), (e) and (f, 9 frames) run again with cam_repeat 0, one camera row each, with and without betas. Distinct betas in +-2 with one
all-zero and one repeated row; cameras far from the identity.

Accuracy within K = 8 times the float32 restatement's own error of the float64 one (+ 1e-7 of the quantity's scale), per output block,
and within the same bound of the reference fixture; identity cameras bit for bit prepare_motions; the local rotations bit for bit
rc_axis_angle_to_rotmat; the interleave bit for bit numpy; two calls the same bits; a sequence's rows those of a call with it alone;
nothing written outside the rows; every refusal before anything is enqueued; run_dataset / the metrics on the camera-frame layout bit for
bit the AIST-layout run of the same rows.

Observed on MI355X (profiles/camera_prepare_ratios.txt): the RATIO lines each accuracy test prints before it asserts."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import camera_motion_ref as CM
import test_gpu_subnet_forward as FWD
from subnet_batches_ref import bound_ratio
from robustcap_amd import _lib, body as body_mod, evaluate as ev, preprocess, synth
from robustcap_amd import config as cfg

pytestmark = pytest.mark.gpu

_same = FWD._same
IN, CAM, KP = (5, 7, 30, 131, 14), (3, 3, 13, 66, 7), (3, 3, 13, 66, 7)
OUT = (5, 6, 26, 131, 14)
STATIC = (3, 4, 5)                      # (d), (e), (f) of the static call
IN_ALL = IN + (9,)
SEED, SMOOTH = 19, 2
BLOCKS = ("posec", "tranc", "joint3d", "sync_3d_mp", "vert6", "imu_accc", "imu_oric")
WIDTH = {"posec": 216, "tranc": 3, "imu_oric": 54, "imu_accc": 18, "joint3d": 72, "sync_3d_mp": 99, "vert6": 18, "joint2d_mp": 99}
INVALID, STATE = -1, -3
SENT = 7.25
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "camera")


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    """The models and prepared buffers that the tests of this module share are released with its last test."""
    yield
    import gc
    for cached in (_prepared, _ref, _inputs, _model, _body, _eval_pair):
        cached.cache_clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _body():
    return synth.make_body(1)


@functools.lru_cache(maxsize=None)
def _model():
    return body_mod.ParametricModel(body=_body())


def _cameras(stream, n):
    """n T_cw rows [n,4,4] drifting from a rotation of about two radians, a few metres away"""
    aa = np.array([1.7, -0.9, 0.5]) + np.cumsum(0.05 * synth.normal(SEED, stream, n * 3).reshape(n, 3), 0)
    T = np.zeros((n, 4, 4), np.float32)
    T[:, :3, :3] = synth._rodrigues(aa).astype(np.float32)
    T[:, :3, 3] = (np.array([0.3, -1.1, 4.2]) + np.cumsum(0.03 * synth.normal(SEED, stream + 1, n * 3).reshape(n, 3), 0)).astype(np.float32)
    T[:, 3] = [0, 0, 0, 1]
    return T


@functools.lru_cache(maxsize=None)
def _inputs():
    """(poses [T_i,24,3], trans [T_i,3], betas [6,10], cams [n_i,4,4], kps [k_i,33,3]) float32 for (a) .. (f); (f) has one camera row."""
    poses, trans, cams, kps = [], [], [], []
    for i, T in enumerate(IN_ALL):
        walk = np.cumsum(0.03 * synth.normal(SEED, 10 + i, T * 72).reshape(T, 24, 3), 0) + 0.4 * synth.normal(SEED, 40 + i, 72).reshape(24, 3)
        poses.append(walk.astype(np.float32))
        trans.append((np.cumsum(0.02 * synth.normal(SEED, 70 + i, T * 3).reshape(T, 3), 0) + [0.3, 0.9, -0.2]).astype(np.float32))
        n = CAM[i] if i < 5 else 1
        cams.append(_cameras(130 + 2 * i, n))
        k = KP[i] if i < 5 else 5
        kp = synth.uniform01(SEED, 160 + i, k * 99).reshape(k, 33, 3).astype(np.float32)
        kp[..., :2] *= np.float32([1920, 1080])
        kps.append(kp)
    betas = (4 * synth.uniform01(SEED, 100, 60).reshape(6, 10) - 2).astype(np.float32)
    betas[1] = 0
    betas[3] = betas[0]
    assert min(np.abs(c[:, :3, :3] - np.eye(3)).max() for c in cams) > 0.5                  # far from the identity
    return poses, trans, betas, cams, kps


def _pick(kind):
    """(sequence indices, cam_repeat, with betas) of a call"""
    return {"moving": (tuple(range(5)), 2, True), "static": (STATIC, 0, True), "static_nobetas": (STATIC, 0, False)}[kind]


def _args(kind):
    poses, trans, betas, cams, kps = _inputs()
    idx, r, wb = _pick(kind)
    cam = [cams[i] if r else cams[i][:1] for i in idx]
    return [poses[i] for i in idx], [trans[i] for i in idx], cam, (betas[list(idx)] if wb else None), r, ([kps[i] for i in idx] if r else None)


@functools.lru_cache(maxsize=None)
def _prepared(kind, again=0):
    p, t, c, b, r, k = _args(kind)
    if not _pick(kind)[2]:
        _model().set_shape(None)
    return preprocess.prepare_camera_motions(_model(), p, t, c, b, r, k, False, SMOOTH)


@functools.lru_cache(maxsize=None)
def _ref(kind, dtype):
    p, t, c, b, r, k = _args(kind)
    return CM.prepare(_body(), p, t, c, b, r, SMOOTH, cfg.mp_mask, cfg.vi_mask, cfg.ji_mask, dtype, keypoints=k)


def _got(p, k):
    return (p.vert6 if k == "vert6" else p.fields[k]).cpu().numpy()


def test_the_tables():
    p = _prepared("moving")
    _, _, _, cams, _ = _inputs()
    assert p.lengths == list(OUT) == CM.output_lengths(IN, CAM, 2) and p.frames == sum(OUT) and p.layout == "camera"
    d = p.as_dict()
    assert sorted(d) == sorted(["posec", "tranc", "joint3d", "sync_3d_mp", "imu_accc", "imu_oric", "joint2d_mp", "shape", "cam_T"])
    assert [tuple(a.shape) for a in d["posec"]] == [(T, 24, 3, 3) for T in OUT] and [tuple(a.shape) for a in d["joint2d_mp"]] == [(T, 33, 3) for T in OUT]
    assert d["posec"][1].data_ptr() == p.posec.data_ptr() + OUT[0] * 216 * 4                              # views, not copies
    for i, T in enumerate(OUT):
        assert np.array_equal(d["cam_T"][i].numpy(), np.repeat(cams[i], 2, axis=0)[:T])                   # the rows actually used
    s = _prepared("static")
    assert s.lengths == [IN_ALL[i] for i in STATIC] and "joint2d_mp" not in s.as_dict()
    assert all(np.array_equal(c.numpy(), np.repeat(cams[i][:1], IN_ALL[i], axis=0)) for c, i in zip(s.as_dict()["cam_T"], STATIC))


@pytest.mark.parametrize("kind", ["moving", "static", "static_nobetas"])
def test_blocks_within_the_bound(kind):
    p = _prepared(kind)
    r64, r32 = _ref(kind, np.float64), _ref(kind, np.float32)
    F = p.frames
    worst = 0.0
    for k in BLOCKS:
        got, f64, f32 = _got(p, k).reshape(F, -1), np.concatenate(r64[k]).reshape(F, -1), np.concatenate(r32[k]).reshape(F, -1)
        r = bound_ratio(got, f64, f32)
        print(f"RATIO camera {kind} {k}: {r:.4f} of the bound (max |f64| {np.abs(f64).max():.3e}, float32 restatement's error "
              f"{np.abs(f32.astype(np.float64) - f64).max():.3e})")
        worst = max(worst, r)
    assert worst <= 1.0


def test_rest_joints_are_prepare_motions_records():
    """The rest kernel is shared: the same betas give the same rest joints, bit for bit, through either entry."""
    poses, trans, betas, _, _ = _inputs()
    p = _prepared("moving")
    q = preprocess.prepare_motions(_model(), list(poses[:5]), list(trans[:5]), betas[:5], None, None, SMOOTH, layout="aist")
    assert _same(p.rest_joint, q.rest_joint)
    assert np.array_equal(p.rest_joint[3].cpu().numpy(), p.rest_joint[0].cpu().numpy()) and not np.array_equal(p.rest_joint[2].cpu().numpy(), p.rest_joint[0].cpu().numpy())


def test_the_device_pass_against_the_reference_fixture():
    z, meta = np.load(os.path.join(GOLDEN, "camera_motions.npz")), json.load(open(os.path.join(GOLDEN, "meta.json")))
    n = len(meta["in"])
    body = synth.make_body(meta["body_seed"])
    model = body_mod.ParametricModel(body=body)
    poses, trans = [z[f"pose.{i}"] for i in range(n)], [z[f"tran.{i}"] for i in range(n)]
    cams, betas, kps = [z[f"cam.{i}"] for i in range(n)], np.stack([z[f"beta.{i}"] for i in range(n)]), [z[f"kp.{i}"] for i in range(n)]
    p = preprocess.prepare_camera_motions(model, poses, trans, cams, betas, meta["cam_repeat"], kps, False, meta["smooth_n"])
    r = {f: CM.prepare(body, [q.reshape(-1, 24, 3) for q in poses], trans, cams, betas, meta["cam_repeat"], meta["smooth_n"], cfg.mp_mask,
                       cfg.vi_mask, cfg.ji_mask, f) for f in (np.float64, np.float32)}
    assert p.lengths == [z[f"posec.{i}"].shape[0] for i in range(n)]
    worst = 0.0
    for k in BLOCKS:
        got = np.split(_got(p, k), np.cumsum(p.lengths)[:-1])
        for i in range(n):
            # the device against the reference's numbers, by the bound around float64 widened by the reference's own distance from it
            f64, f32, ref = r[np.float64][k][i], r[np.float32][k][i], z[f"{k}.{i}"]
            r_dev, r_ref = bound_ratio(got[i], f64, f32), bound_ratio(ref, f64, f32)
            print(f"RATIO camera fixture {k}.{i}: device {r_dev:.4f}, reference {r_ref:.4f} of the bound")
            worst = max(worst, r_dev, r_ref)
    assert worst <= 1.0
    for i, j in enumerate(np.split(p.joint2d_mp.cpu().numpy(), np.cumsum(p.lengths)[:-1])):
        assert np.array_equal(j.view(np.int32), z[f"joint2d_mp.{i}"].view(np.int32))                      # the reference's interleave, bit for bit


# ------------------------------------------------------------------------------------------------ bitwise ties
def test_identity_cameras_are_prepare_motions_bit_for_bit():
    model = _model()
    poses, trans, betas, _, _ = _inputs()
    idx = list(STATIC)
    P, T = [poses[i] for i in idx], [trans[i] for i in idx]
    eye = [np.eye(4, dtype=np.float32)] * 3
    for b in (betas[idx], None):
        if b is None:
            model.set_shape(None)
        c = preprocess.prepare_camera_motions(model, P, T, eye, b, 0, None, False, SMOOTH)
        m = preprocess.prepare_motions(model, P, T, b, None, None, SMOOTH, layout="aist")
        for kc, km in (("tranc", "tran"), ("imu_oric", "imu_ori"), ("joint3d", "joint3d"), ("sync_3d_mp", "sync_3d_mp"), ("imu_accc", "imu_acc")):
            assert _same(c.fields[kc], m.fields[km]), kc
        assert _same(c.vert6, m.vert6) and _same(c.rest_joint, m.rest_joint)
        R = body_mod.axis_angle_to_rotation_matrix(torch.from_numpy(np.concatenate(P)).reshape(-1, 3)).view(-1, 24, 3, 3)
        assert _same(c.posec, R)


def test_local_rotations_translation_copy_and_interleave_are_exact():
    poses, trans, _, _, kps = _inputs()
    p = _prepared("moving")
    pin = np.concatenate([poses[i][:T] for i, T in enumerate(OUT)])
    R = body_mod.axis_angle_to_rotation_matrix(torch.from_numpy(pin).reshape(-1, 3)).view(-1, 24, 3, 3)
    assert _same(p.posec[:, 1:].contiguous(), R[:, 1:].contiguous())                                      # joints 1 .. 23 under real cameras
    assert not _same(p.posec[:, 0].contiguous(), R[:, 0].contiguous())
    want = np.concatenate([CM.interleave(kps[i], T) for i, T in enumerate(OUT)])
    assert np.array_equal(p.joint2d_mp.cpu().numpy().view(np.int32), want.view(np.int32))
    P, T, c, b, r, k = _args("moving")
    ro = preprocess.prepare_camera_motions(_model(), P, T, c, b, r, k, True, SMOOTH)                       # root_only: the translation is a bit copy
    tin = np.concatenate([trans[i][:n] for i, n in enumerate(OUT)])
    assert np.array_equal(ro.tranc.cpu().numpy().view(np.int32), tin.view(np.int32))
    assert _same(ro.posec, p.posec) and _same(ro.imu_oric, p.imu_oric) and not _same(ro.joint3d, p.joint3d)


def test_two_calls_give_the_same_bits():
    a, b = _prepared("moving"), _prepared("moving", 1)
    assert a is not b
    for k in BLOCKS + ("joint2d_mp",):
        assert _same(torch.from_numpy(_got(a, k)), torch.from_numpy(_got(b, k))), k
    assert _same(a.rest_joint, b.rest_joint)


@pytest.mark.parametrize("i", [1, 2, 3])
def test_a_sequence_alone_gives_its_rows(i):
    poses, trans, betas, cams, kps = _inputs()
    whole = _prepared("moving")
    one = preprocess.prepare_camera_motions(_model(), [poses[i]], [trans[i]], [cams[i]], betas[i:i + 1], 2, [kps[i]], False, SMOOTH)
    a = sum(OUT[:i])
    for k in BLOCKS + ("joint2d_mp",):
        assert _same(torch.from_numpy(_got(whole, k)[a:a + OUT[i]]), torch.from_numpy(_got(one, k))), k
    assert _same(whole.rest_joint[i:i + 1], one.rest_joint)


# ------------------------------------------------------------------------------------------------ the raw entry: sentinels and refusals
class Call:
    """The arguments of one rc_prepare_camera_motions call on (a) .. (e), every output a view at an odd offset of a sentinel-filled buffer."""

    def __init__(self, model):
        poses, trans, betas, cams, kps = _inputs()
        dev = model.device
        self.model = model
        self.pose = torch.from_numpy(np.concatenate(poses[:5])).to(dev).contiguous()
        self.tran = torch.from_numpy(np.concatenate(trans[:5])).to(dev).contiguous()
        self.betas = torch.from_numpy(betas[:5]).to(dev).contiguous()
        self.kp = torch.from_numpy(np.concatenate(kps[:5])).to(dev).contiguous()
        self.cam = np.ascontiguousarray(np.concatenate(cams[:5]))
        F, self.pad, n = sum(OUT), 3, 5
        self.buf = {k: torch.full(((F + 2) * w + 2 * self.pad,), SENT, device=dev) for k, w in WIDTH.items()}
        self.buf["rest"] = torch.full((5 * 72 + 2 * self.pad,), SENT, device=dev)
        self.out = {k: b[self.pad:self.pad + (5 * 72 if k == "rest" else F * WIDTH[k])] for k, b in self.buf.items()}
        self.args = {"ctx": model._ctx, "n_seq": n, "in_frames": (C.c_int64 * n)(*IN), "cam_frames": (C.c_int64 * n)(*CAM), "cam_repeat": 2,
                     "in_total": sum(IN), "cam_total": sum(CAM), "pose_aa": _lib.ptr(self.pose), "tran": _lib.ptr(self.tran),
                     "betas": _lib.ptr(self.betas), "cam_T": self.cam.ctypes.data_as(C.c_void_p), "kp_in": _lib.ptr(self.kp),
                     "kp_frames": (C.c_int64 * n)(*KP), "kp_total": sum(KP), "joint_ids": (C.c_int32 * 6)(*cfg.ji_mask), "smooth_n": SMOOTH,
                     "flags": 0, "pose_out": _lib.ptr(self.out["posec"]), "tran_out": _lib.ptr(self.out["tranc"]),
                     "imu_ori": _lib.ptr(self.out["imu_oric"]), "imu_acc": _lib.ptr(self.out["imu_accc"]), "joint3d": _lib.ptr(self.out["joint3d"]),
                     "sync_3d_mp": _lib.ptr(self.out["sync_3d_mp"]), "vert6_out": _lib.ptr(self.out["vert6"]),
                     "kp_out": _lib.ptr(self.out["joint2d_mp"]), "rest_joint_out": _lib.ptr(self.out["rest"])}

    def __call__(self):
        return self.model._lib.rc_prepare_camera_motions(*self.args.values(), _lib.stream_ptr())

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((b == SENT).all()) for b in self.buf.values())


def test_nothing_outside_the_rows_is_written():
    model = _model()
    model._ensure_shape_space()
    c = Call(model)
    before = (c.pose.clone(), c.tran.clone(), c.betas.clone(), c.kp.clone(), c.cam.copy())
    assert c() == 0
    torch.cuda.synchronize()
    whole = _prepared("moving")
    for k in WIDTH:
        want = (whole.vert6 if k == "vert6" else whole.fields[k]).reshape(-1)
        assert _same(c.out[k], want), k
    assert _same(c.out["rest"], whole.rest_joint.reshape(-1))
    for k, b in c.buf.items():
        n = c.out[k].numel()
        assert bool((b[:c.pad] == SENT).all()) and bool((b[c.pad + n:] == SENT).all()), k
    assert _same(before[0], c.pose) and _same(before[1], c.tran) and _same(before[2], c.betas) and _same(before[3], c.kp)
    assert np.array_equal(before[4], c.cam)
    # the optional outputs left out: the others keep their bits, the ones left out are not written
    for k in ("sync_3d_mp", "vert6_out", "rest_joint_out", "kp_out"):
        c.args[k] = None
    c.args["kp_in"], c.args["kp_frames"], c.args["kp_total"] = None, None, 0
    for b in c.buf.values():
        b.fill_(SENT)
    assert c() == 0
    torch.cuda.synchronize()
    for k in ("posec", "tranc", "imu_oric", "imu_accc", "joint3d"):
        assert _same(c.out[k], whole.fields[k].reshape(-1)), k
    for k in ("sync_3d_mp", "vert6", "joint2d_mp", "rest"):
        assert bool((c.buf[k] == SENT).all()), k


def test_refusals_leave_the_outputs_untouched():
    model = _model()
    model._ensure_shape_space()
    lib = model._lib

    def attempt(what, expect=INVALID, model_=model, **edit):
        c = Call(model_)
        c.args.update(edit)
        if "cam_edit" in edit:
            c.args.pop("cam_edit")
            edit["cam_edit"](c.cam)
        rc = c()
        assert rc == expect, (what, rc)
        if c.args["ctx"] is not None:
            assert b"rc_prepare_camera_motions" in lib.rc_last_error(c.args["ctx"]), what
        assert c.untouched(), what

    i64, i32 = (lambda *v: (C.c_int64 * len(v))(*v)), (lambda *v: (C.c_int32 * len(v))(*v))
    attempt("null context", ctx=None)
    for k in ("in_frames", "cam_frames", "pose_aa", "tran", "cam_T", "joint_ids", "pose_out", "tran_out", "imu_ori", "imu_acc", "joint3d"):
        attempt("null " + k, **{k: None})
    attempt("kp_in without kp_out", kp_out=None)
    attempt("kp_in without kp_frames", kp_frames=None)
    attempt("kp_out without kp_in", kp_in=None)
    attempt("n_seq 0", n_seq=0)
    attempt("n_seq -1", n_seq=-1)
    attempt("cam_repeat -1", cam_repeat=-1)
    attempt("a sequence without a camera row", cam_frames=i64(3, 0, 13, 66, 10))
    attempt("cam_repeat 0 with more than one camera row", cam_repeat=0)
    attempt("cam_repeat 0 with two rows in one sequence", cam_repeat=0, cam_frames=i64(1, 1, 2, 1, 1), cam_total=6)
    attempt("camera tables that do not sum to cam_total", cam_total=sum(CAM) + 1)
    attempt("camera tables that do not sum to cam_total", cam_frames=i64(3, 3, 13, 66, 6))
    attempt("tables that do not sum to in_total", in_total=sum(IN) + 1)
    attempt("tables that do not sum to in_total", in_frames=i64(5, 7, 30, 131, 13))
    attempt("detector tables that do not sum to kp_total", kp_total=sum(KP) + 1)
    attempt("two detector frames for five output frames", kp_frames=i64(2, 3, 13, 66, 8))
    attempt("a negative detector count", kp_frames=i64(-1, 3, 13, 66, 11))
    attempt("a sequence without a frame", in_frames=i64(5, 7, 0, 131, 44))
    attempt("a sequence of 4 frames under smooth_n 2", in_frames=i64(4, 7, 30, 131, 15))
    attempt("4 output frames under smooth_n 2: two camera rows", cam_frames=i64(3, 2, 13, 66, 8))
    attempt("2^31 frames", n_seq=2, in_frames=i64(1 << 30, 1 << 30), cam_frames=i64(1, 1), cam_repeat=0, in_total=1 << 31, cam_total=2,
            kp_in=None, kp_out=None, kp_frames=None, kp_total=0)
    attempt("smooth_n -1", smooth_n=-1)
    attempt("an unknown flag", flags=2)
    attempt("an unknown flag beside the known one", flags=1 | 8)
    attempt("an IMU joint of 24", joint_ids=i32(18, 19, 4, 5, 15, 24))
    for bad in (float("nan"), float("inf"), float("-inf")):
        for row, col in ((0, 0), (sum(CAM) - 1, 11), (40, 7)):
            def edit(cam, bad=bad, row=row, col=col):
                cam.reshape(-1, 16)[row, col] = bad
            attempt("a non-finite camera row", cam_edit=edit)
    c = Call(model)                                                          # row 3 of a T_cw is ignored, whatever it holds
    c.cam.reshape(-1, 16)[:, 12:] = float("nan")
    assert c() == 0
    assert _same(c.out["posec"], _prepared("moving").posec.reshape(-1)) and _same(c.out["tranc"], _prepared("moving").tranc.reshape(-1))
    fresh = body_mod.ParametricModel(body=_body())                            # no rc_set_shape_space yet
    fresh._ensure_mesh()
    attempt("without rc_set_shape_space", STATE, fresh)
    bare = {k: v for k, v in _body().items() if k not in ("shapedirs", "J_regressor")}
    lean = body_mod.ParametricModel(body=bare)
    lean._ensure_shape_space()                                                # the picks alone: no basis
    attempt("betas without the shape basis", STATE, lean)
    with pytest.raises(ValueError):
        preprocess.prepare_camera_motions(model, [np.zeros((5, 23, 3), np.float32)], [np.zeros((5, 3), np.float32)], [np.eye(4)])
    with pytest.raises(ValueError):
        preprocess.prepare_camera_motions(model, [np.zeros((5, 24, 3), np.float32)], [np.zeros((4, 3), np.float32)], [np.eye(4)])
    with pytest.raises(ValueError):
        preprocess.prepare_camera_motions(model, [np.zeros((5, 24, 3), np.float32)], [np.zeros((5, 3), np.float32)], [np.eye(4)] * 2)


# ------------------------------------------------------------------------------------------------ the public routes
def test_prepare_pw3d_is_the_reference_loop():
    poses, trans, betas, cams, kps = _inputs()
    whole = _prepared("moving")
    b16 = [np.concatenate([betas[i], [9.0] * 6]).astype(np.float32) for i in range(5)]
    Ks = [np.eye(3, dtype=np.float32) * (1000 + i) for i in range(5)]
    p = preprocess.prepare_pw3d(_model(), [q.reshape(-1, 72) for q in poses[:5]], trans[:5], b16, cams[:5], Ks, [list(k) for k in kps[:5]],
                                names=list("abcde"))
    for k in BLOCKS + ("joint2d_mp",):
        assert _same(torch.from_numpy(_got(p, k)), torch.from_numpy(_got(whole, k))), k
    d = p.as_dict()
    assert d["name"] == list("abcde") and tuple(d["cam_K"][2].shape) == (3, 3) and float(d["cam_K"][2][0, 0]) == 1002.0
    assert np.array_equal(np.stack([np.asarray(s) for s in d["shape"]]), betas[:5])
    # frames where the detector found nothing: uniform draws with confidence 0, repeatable under a seeded generator
    holes = [list(k) for k in kps[:5]]
    holes[0][1], holes[2][4] = None, np.zeros((0, 3), np.float32)
    runs = [preprocess.prepare_pw3d(_model(), [q.reshape(-1, 72) for q in poses[:5]], trans[:5], b16, cams[:5], Ks, holes,
                                    generator=torch.Generator().manual_seed(3)).joint2d_mp.cpu() for _ in range(2)]
    assert torch.equal(runs[0], runs[1])
    a = runs[0][:OUT[0]]
    assert bool((a[2, :, 2] == 0).all()) and bool(((a[2, :, :2] >= 0) & (a[2, :, :2] < 1)).all())         # output frame 2 = detector frame 1
    assert torch.equal(a[0], torch.from_numpy(kps[0][0])) and torch.equal(a[4], torch.from_numpy(kps[0][2]))
    assert bool((runs[0][OUT[0] + OUT[1] + 8, :, 2] == 0).all())                                          # sequence c, detector frame 4


def test_prepare_totalcapture_against_the_reference_fixture():
    z, meta = np.load(os.path.join(GOLDEN, "camera_motions.npz")), json.load(open(os.path.join(GOLDEN, "meta.json")))
    body = synth.make_body(meta["body_seed"])
    model = body_mod.ParametricModel(body=body)
    K, Tc = np.tile(np.eye(3, dtype=np.float32), (8, 1, 1)), np.tile(np.eye(4, dtype=np.float32), (8, 1, 1))
    kp = [[np.zeros((33, 33, 4), np.float32)] * 8]
    p = preprocess.prepare_totalcapture(model, [z["tc.gt"]], [z["tc.ori_raw"]], [z["tc.acc_raw"]], [z["tc.vicon"]], K, Tc, kp, ["s1_acting1"])
    T = z["tc.pose"].shape[0]
    assert p.lengths == [T] and p.layout == "totalcapture"
    d = p.as_dict()
    assert tuple(d["pose"][0].shape) == (T, 24, 3) and tuple(d["joint2d_mp"][0].shape) == (8, T, 33, 4) and tuple(d["cam_T"][0].shape) == (8, 4, 4)
    assert np.array_equal(d["tran"][0].cpu().numpy().view(np.int32), z["tc.tran"].view(np.int32))         # the two corrections, bit for bit
    assert np.array_equal(d["imu_ori"][0].cpu().numpy(), z["tc.ori"]) and np.array_equal(d["imu_acc"][0].cpu().numpy(), z["tc.acc"])
    pose, _, _, tran = CM.totalcapture_clip(z["tc.gt"], z["tc.ori_raw"], z["tc.acc_raw"], z["tc.vicon"])
    static = np.eye(4)
    static[:3, :3] = CM.TC_FLIP
    r = {f: CM.prepare(body, [pose.reshape(-1, 24, 3)], [CM.totalcapture_tran(tran, np.float32)], [static], None, 0, meta["smooth_n"], cfg.mp_mask,
                       cfg.vi_mask, cfg.ji_mask, f, root_only=True) for f in (np.float64, np.float32)}
    worst = 0.0
    for k, name, got in (("joint3d", "joint3d", p.joint3d), ("sync_3d_mp", "sync_3d_mp", p.sync_3d_mp), ("vert6", "vert6", p.vert6)):
        rr = max(bound_ratio(got.cpu().numpy(), r[np.float64][k][0], r[np.float32][k][0]), bound_ratio(z["tc." + name], r[np.float64][k][0], r[np.float32][k][0]))
        print(f"RATIO camera totalcapture {name}: {rr:.4f} of the bound")
        worst = max(worst, rr)
    assert worst <= 1.0
    # the stored axis-angle pose gives the flipped rotations back (R -> axis-angle -> R, float32 both ways)
    back = body_mod.axis_angle_to_rotation_matrix(d["pose"][0].reshape(-1, 3)).view(T, 24, 3, 3).cpu().numpy()
    assert np.abs(back - z["tc.pose"]).max() < 5e-6
    # :445 returned: mean angle between the real (here: unrelated random) and the synthetic orientations, in degrees
    ang = p["imu_consistency_deg"]
    G = r[np.float64]["imu_oric"][0]
    D = np.einsum("tiab,tiac->tibc", z["tc.ori"].astype(np.float64), G)
    want = np.degrees(np.arccos(np.clip((np.trace(D, axis1=-2, axis2=-1) - 1) / 2, -1, 1))).mean()
    assert tuple(ang.shape) == (1,) and abs(float(ang[0]) - want) < 1e-2


# ------------------------------------------------------------------------------------------------ the evaluation harness on the layout
@functools.lru_cache(maxsize=None)
def _eval_pair():
    """(AIST-layout data set of 2 sequences x 2 cameras x 24 frames, the camera-frame dictionary of its four rows): the IMU rows are the
    very accc / oric that camera_inputs_rows produces, the labels those of ``labels``, the keypoints in pixels."""
    ds = synth.make_dataset(9, 2, 24, _body(), n_cam=2)
    rows = ev.rows_of(ds)
    _, accc, oric, _ = ev.camera_inputs_rows(ds, rows, 24)
    cam = {k: [] for k in ("posec", "tranc", "imu_oric", "imu_accc", "joint2d_mp", "cam_K", "cam_T")}
    for r, (i, j) in enumerate(rows):
        pose, tran = ev.labels(ds, i, j)
        cam["posec"].append(pose), cam["tranc"].append(tran), cam["imu_oric"].append(oric[r].clone()), cam["imu_accc"].append(accc[r].clone())
        cam["joint2d_mp"].append(torch.from_numpy(ds["joint2d_mp"][i][j] * np.float32([1920, 1080, 1])))
        cam["cam_K"].append(torch.from_numpy(ds["cam_K"][i][j]))
        cam["cam_T"].append(torch.from_numpy(ds["cam_T"][i][j]).repeat(24, 1, 1))                         # a camera that stands still
    return ds, cam, rows


def test_run_dataset_on_the_camera_frame_layout_is_the_aist_run(synth_assets):
    ds, cam, rows = _eval_pair()
    sd, body = synth_assets["state_dict"], _body()
    assert ev.rows_of(cam) == [(k, 0) for k in range(4)]
    j_a, a_a, o_a, g_a = ev.camera_inputs_rows(ds, rows, 24)
    j_c, a_c, o_c, g_c = ev.camera_inputs_rows(cam, ev.rows_of(cam), 24)
    assert _same(j_a, j_c) and _same(a_a, a_c) and _same(o_a, o_c) and torch.equal(g_a, g_c)
    assert torch.equal(ev.first_translations(ds, rows), ev.first_translations(cam, ev.rows_of(cam)))
    for kw in (dict(), dict(use_first_tran=False), dict(ragged=True)):
        res_a = ev.run_dataset(ds, sd, body, use_flat_floor=False, **kw)
        res_c = ev.run_dataset(cam, sd, body, use_flat_floor=False, **kw)
        for k, (i, j) in enumerate(rows):
            assert _same(res_a[(i, j)][0], res_c[(k, 0)][0]) and _same(res_a[(i, j)][1], res_c[(k, 0)][1]), (kw, i, j)
    res_flat = ev.run_dataset(cam, sd, body, use_flat_floor=True)             # a still camera may use the flat floor
    assert sorted(res_flat) == sorted(res_c)
    moving = dict(cam, cam_T=[t.clone() for t in cam["cam_T"]])
    moving["cam_T"][2][7, 0, 3] += 0.01
    with pytest.raises(ValueError, match="moving camera"):
        ev.run_dataset(moving, sd, body, use_flat_floor=True)
    assert sorted(ev.run_dataset(moving, sd, body, use_flat_floor=False)) == sorted(res_c)
    # the metrics
    model = _model()
    as_cam = {(k, 0): res_a[r] for k, r in enumerate(rows)}
    # dataset_metrics forms the AIST layout's label root R_cw R_0 ON THE DEVICE, ``labels`` on the host, and the two float32 products can
    # differ in the last bit. The exact tie is therefore made on a dictionary whose posec root is that device product; on the dictionary
    # taken from ``labels`` the metrics agree within what one ulp of the root rotation moves a body point: the nine entries change by at
    # most 2^-24 each, a point within 2 m of the root by at most 3 * 2^-24 * 2 m < 4e-7 m, a mean distance by no more than that.
    dev = torch.device("cuda")
    exact = dict(cam, posec=[])
    for (i, j) in rows:
        gt = body_mod.axis_angle_to_rotation_matrix(torch.as_tensor(ds["pose"][i]).reshape(-1, 3)).view(-1, 24, 3, 3)
        gt[:, 0] = torch.as_tensor(ds["cam_T"][i][j], dtype=torch.float32)[:3, :3].to(dev) @ gt[:, 0]
        exact["posec"].append(gt)
    m_a, mean_a = ev.dataset_metrics(model, ds, res_a)
    m_e, mean_e = ev.dataset_metrics(model, exact, as_cam)
    assert [m_a[r] for r in rows] == [m_e[(k, 0)] for k in range(4)] and mean_a == mean_e
    m_c, mean_c = ev.dataset_metrics(model, cam, as_cam)
    assert max(abs(a - b) for k, r in enumerate(rows) for a, b in zip(m_a[r], m_c[(k, 0)])) < 4e-7 and max(abs(a - b) for a, b in zip(mean_a, mean_c)) < 4e-7
    f_a, fm_a = ev.motion_metrics(model, ds, res_a)
    f_c, fm_c = ev.motion_metrics(model, cam, as_cam)
    assert all(_same(f_a[r], f_c[(k, 0)]) for k, r in enumerate(rows)) and _same(fm_a, fm_c)             # (bits: 24 frames at 60 fps leave NaNs)
    assert bool(torch.isfinite(f_a[rows[0]][0]).all())
    per_a, mean_ea = ev.evaluate(ds, sd, body, use_flat_floor=False)
    per_c, mean_ec = ev.evaluate(cam, sd, body, use_flat_floor=False)
    assert [per_a[r] for r in rows] == [per_c[(k, 0)] for k in range(4)] and mean_ea == mean_ec


def test_root_position_errors_aligned_at_the_last_frame(synth_assets):
    ds, cam, rows = _eval_pair()
    res = {}
    for k, (i, j) in enumerate(rows):                                         # predictions: the labels, drifting and offset
        pose, tran = ev.labels(ds, i, j)
        drift = torch.from_numpy((np.cumsum(0.01 * synth.normal(4, k, 72).reshape(24, 3), 0) + [0.3, -0.2, 0.5]).astype(np.float32))
        res[(i, j)] = (pose, tran + drift)
    worst = 0.0
    for data, results in ((ds, res), (cam, {(k, 0): res[r] for k, r in enumerate(rows)})):
        for align in ("none", "last"):
            per, mean = ev.root_position_errors(data, results, align=align)
            f = {np.float64: [], np.float32: []}
            for key, (_, tp) in results.items():
                tt = ev.labels(data, *key)[1]
                for dt in f:                                                  # the float64 expression, and its float32 run for the bound
                    p, t = tp.numpy().astype(dt), tt.numpy().astype(dt)
                    if align == "last":
                        p = p + (t[-1] - p[-1])
                    f[dt].append(np.sqrt(((p - t) ** 2).sum(1, dtype=dt)).mean(dtype=dt))
            r = bound_ratio(np.array([per[k] for k in results]), np.array(f[np.float64]), np.array(f[np.float32]))
            print(f"RATIO camera root error {align}: {r:.4f} of the bound over {len(results)} rows ({[round(per[k], 6) for k in results]} m)")
            worst = max(worst, r)
            assert abs(mean - np.mean(list(per.values()))) < 1e-12
        assert all(ev.root_position_errors(data, results, "last")[0][k] < ev.root_position_errors(data, results, "none")[0][k] for k in results)
    assert worst <= 1.0
