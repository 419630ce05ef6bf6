"""rc_ops.hip, the per-op kernels of rc_frame.hip and rc_preprocess.hip against the float64 restatements of oracle/pose_ops_f64.py.

  values      every case of pose_ops_f64.suite (r6d, aa -> R, angle_between, normalize_tensor, the bbox normalisation, IK_R, FK_R,
              bone FK, forward_kinematics with landmarks, the reprojection residual, the shaped body at V = 6890) through the Python
              surface, within Bound = M max(e32, eps32 A) of the float64 restatement; R -> aa within 2^-22 of the oracle (as a
              rotation inside the s ~ 1e-5 window); the exactly degenerate r6d rows and the zero-size box in their zero / inf / NaN
              pattern, which is the float32 oracle's.
  bit for bit bone_vector_to_joint_position / joint_position_to_bone_vector (the reference's add order), rotation_matrix_to_r6d (a
              permutation), lerp (lerp_rows), _syn_acc (a float32 restatement of the kernel's stencil, smooth_n 0..4 at the 2n + 1
              edge), synthesize_imu's ori / joint / vert6 against forward_kinematics / forward_mesh.
  launches    every op on a batch that cycles its cases up to n items, n on the kernel's own block edges: each item bitwise the
              item run alone; n = 0 gives an empty tensor of the right shape.
tests/test_pose_ops_bound_cpu.py shows on the CPU that honest float32 evaluations stay within a third of these bounds and every
mutation lands beyond three times them. RC_POSE_OPS_RATIOS_OUT=<file> keeps the worst error / Bound per op and its case.
"""
import os

import numpy as np
import pytest
import torch

from oracle import pose_ops_f64 as P
from oracle import sig_mp_oracle as O

pytestmark = pytest.mark.gpu
WORST = P.Worst()


def d(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).cuda()


def bits_equal(a, b):
    """bitwise equality (NaN equals the same NaN, -0 differs from +0)"""
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture(scope="module")
def body(synth_assets):
    return synth_assets["body"]


@pytest.fixture(scope="module")
def model(body):
    from robustcap_amd.body import ParametricModel
    return ParametricModel(body=body)


@pytest.fixture(scope="module")
def suite(body):
    return P.suite(body)


def device_eval(e, model, body):
    from robustcap_amd import body as B
    a = [d(x) for x in e.args]
    if e.fn == "r6d":
        out = B.r6d_to_rotation_matrix(*a)
    elif e.fn == "aa2R":
        out = B.axis_angle_to_rotation_matrix(*a)
    elif e.fn == "angle":
        out = B.angle_between(*a)
    elif e.fn == "normalize":
        out = B.normalize_tensor(a[0], return_norm=True)
    elif e.fn == "bbox":
        out = B.normalize_keypoints(*a)
    elif e.fn == "ik":
        out = model.inverse_kinematics_R(*a)
    elif e.fn == "fk_r":
        out = model.forward_kinematics_R(*a)
    elif e.fn == "bone_fk":
        out = model.bone_fk(*a)
    elif e.fn == "body_fk":
        out = model.forward_kinematics(a[0], tran=a[1], calc_mesh=True)
    elif e.fn == "residual":
        out = model.reprojection_residual(a[0], a[1], a[2], d(P.CAM_K), e.extra)
    elif e.fn == "shape":
        sb = B.shaped_body(model._ctx, body, torch.from_numpy(e.args[0]))
        out = (torch.from_numpy(sb["v_template"])[None], torch.from_numpy(sb["J"])[None])
    out = out if e.out is None else out[e.out]
    return out.cpu()


# ----------------------------------------------------------------------------------------------------------- values
def test_every_case_within_its_float64_bound(suite, model, body):
    failed = []
    for e in suite:
        got = device_eval(e, model, body)
        r = P.case_ratios(e, got)
        if e.op == "residual":                                                  # ignored landmarks and confidence 0: exactly 0
            assert (got[:, list(P.C.smplify_ignored_landmarks) + [17]] == 0).all() and (got[:, 18] > 0).all()
        WORST.note(e.op, r, e.names)
        i = int(r.argmax())
        print(f"{e.op:10s} {len(e.names):3d} cases: worst error / Bound {float(r[i]):.3f}  ({e.names[i]})")
        failed += [(e.op, nm, float(v)) for nm, v in zip(e.names, r) if not v <= 1.0]
    assert not failed, failed


def test_rotmat_to_axis_angle_within_one_rounding_of_the_oracle():
    from robustcap_amd.body import rotation_matrix_to_axis_angle
    c = P.r2aa_cases()
    got = rotation_matrix_to_axis_angle(d(c.x[0])).cpu().numpy()
    assert np.isfinite(got).all()
    r, win = P.r2aa_errors(got, c.x[0])
    assert int(win.sum()) <= P.WINDOW_MAX
    for nm, v, w in zip(c.names, r, win):
        print(f"R -> aa  {nm:52s} error / 2^-22 {v:.3f}" + ("  (in the window: angle / 4e-5)" if w else ""))
    WORST.note("R -> aa", torch.from_numpy(r), c.names)
    assert r.max() <= 1.0, c.names[int(np.argmax(r))]
    for nm in ("identity", "theta 1e-06 (c > 0 exit)", "theta 4e-06 (c > 0 exit)", "entry 100 (zero vector)", "entry NaN (zero vector)", "zero matrix (zero vector)"):
        assert (got[c.names.index(nm)] == 0).all(), nm


def test_degenerate_rows_keep_the_float32_oracles_pattern():
    from robustcap_amd.body import normalize_keypoints, normalize_tensor, r6d_to_rotation_matrix
    deg = P.r6d_cases().pick("degenerate")
    got = r6d_to_rotation_matrix(d(deg.x[0])).cpu()
    assert not torch.isnan(got).any()
    assert torch.equal(got == 0, O.r6d_to_rotation_matrix(P.t32(deg.x[0])) == 0)
    c = P.bbox_cases()
    kp = P.t32(c.x[0])
    got, want = normalize_keypoints(kp).cpu(), O.normalize_keypoints(kp)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.isinf(got), torch.isinf(want))
    assert torch.equal(torch.sign(got[torch.isinf(got)]), torch.sign(want[torch.isinf(want)]))
    assert int(torch.isnan(got).sum()) == 64 and int(torch.isinf(got).sum()) == 2              # the frame of 33 equal points
    assert bits_equal(got[..., 2], kp[..., 2])                                                  # confidence passes through
    x = P.t32(np.stack([np.ones(7), np.zeros(7)]))
    out, nrm = normalize_tensor(x, return_norm=True)
    assert torch.isnan(out[1]).all() and float(nrm[1]) == 0.0 and torch.isfinite(out[0]).all()


# ------------------------------------------------------------------------------------------------------ bit for bit
def test_bone_vectors_and_joint_positions_keep_the_references_add_order(model, body):
    ob = O.OracleBody(body)
    x = P.synth.normal(101, 0, 65 * 72).reshape(65, 24, 3) * 10.0 ** (4.0 * P.synth.uniform01(101, 1, 65 * 72).reshape(65, 24, 3) - 2.0)
    x = P.t32(x)
    assert bits_equal(model.bone_vector_to_joint_position(x).cpu(), ob.bone_to_joint(x))
    want = torch.cat((x[:, :1], (-x[:, ob.par[1:]]) + x[:, 1:]), dim=1)                         # spatial.py: add(neg(parent), child)
    assert bits_equal(model.joint_position_to_bone_vector(x).cpu(), want)
    assert bits_equal(model.bone_vector_to_joint_position(x.reshape(65, 72)).cpu(), ob.bone_to_joint(x))


def test_rotation_matrix_to_r6d_is_the_index_permutation():
    from robustcap_amd.body import rotation_matrix_to_r6d
    R = P.t32(P.synth.normal(102, 0, 128 * 9).reshape(128, 3, 3))
    R[5, 1, 1], R[6, 2, 0], R[7, 0, 0] = float("inf"), -0.0, 1e-42
    assert bits_equal(rotation_matrix_to_r6d(R).cpu(), R[:, :, :2].transpose(1, 2).reshape(-1, 6))


LERP_T = (0.0, 1.0, -0.5, 1.5, 1e-8, 0.3)


@pytest.mark.parametrize("tw", LERP_T)
def test_lerp_is_lerp_rows(tw):
    from robustcap_amd.body import lerp
    a = P.t32(P.synth.normal(103, 0, 257 * 5).reshape(257, 5) * 100.0)
    b = P.t32(P.synth.normal(103, 1, 257 * 5).reshape(257, 5))
    want = O.lerp_rows(a, b, torch.full((257,), tw, dtype=torch.float64))
    assert bits_equal(lerp(a, b, tw).cpu(), want)
    for n in (255, 256, 257):                                                                   # elements: the 256-thread block edge
        assert bits_equal(lerp(a.reshape(-1)[:n], b.reshape(-1)[:n], tw).cpu(), want.reshape(-1)[:n])


def syn_acc_f32(v, n):
    """rc_syn_acc_kernel's comment in float32 torch: zero end frames, ((v[t-1] + v[t+1]) - 2 v[t]) * 3600 inside, and for
    n // 2 != 0 the frames n <= t < T - n from the wide stencil (((v[t-n] + v[t+n]) - 2 v[t]) * 3600) / n^2"""
    acc = torch.zeros_like(v)
    acc[1:-1] = ((v[:-2] + v[2:]) - 2.0 * v[1:-1]) * 3600.0
    if n // 2 != 0:
        acc[n:-n] = (((v[:-2 * n] + v[2 * n:]) - 2.0 * v[n:-n]) * 3600.0) / float(n * n)
    return acc


SYN_ACC = [(n, T) for n in (0, 1, 2, 3, 4) for T in (2 * n + 1, 2 * n + 2, 40, 14, 15) if T >= 3]


@pytest.mark.parametrize("n,T", SYN_ACC)
def test_syn_acc_is_the_float32_stencil(n, T):
    from robustcap_amd.preprocess import _syn_acc
    v = P.t32(P.synth.normal(104, 10 * n + T, T * 18).reshape(T, 18) * 0.3 + 1.0)
    assert bits_equal(_syn_acc(v, smooth_n=n).cpu(), syn_acc_f32(v, n))
    assert bits_equal(_syn_acc(v.reshape(T, 6, 3), smooth_n=n).cpu(), syn_acc_f32(v, n).reshape(T, 6, 3))


@pytest.mark.parametrize("n", (2, 3, 4))
def test_syn_acc_raises_below_2n_plus_1_frames(n):
    from robustcap_amd import _lib
    from robustcap_amd.preprocess import _syn_acc
    with pytest.raises(_lib.RobustcapLibraryError):
        _syn_acc(torch.ones(2 * n, 18), smooth_n=n)
    with pytest.raises(_lib.RobustcapLibraryError):
        _syn_acc(torch.ones(8, 18), smooth_n=-1)


def test_synthesize_imu_is_forward_kinematics_and_the_mesh_sweep(model):
    from robustcap_amd.preprocess import _syn_acc, synthesize_imu
    pc = P.pose_cases()
    idx = np.arange(65) % len(pc)
    pose, tran = d(pc.x[0][idx]), d(pc.x[1][idx] + 0.01 * np.arange(65, dtype=np.float32)[:, None])
    for T, n in ((65, 2), (65, 4), (17, 3), (2, 1), (1, 1)):
        ori, acc, joint, vert6 = synthesize_imu(model, pose[:T], tran[:T], smooth_n=n)
        G, J = model.forward_kinematics(pose[:T], tran=tran[:T])
        assert bits_equal(ori, G[:, list(P.C.ji_mask)]), T
        assert bits_equal(joint, J), T
        assert bits_equal(vert6, model.forward_mesh(pose[:T], tran[:T])[:, list(P.C.vi_mask)]), T
        if T >= 3:
            assert bits_equal(acc, _syn_acc(vert6, smooth_n=n)), T


# --------------------------------------------------------------------------------------------------- launch edges
def _as_tuple(o):
    return o if isinstance(o, tuple) else (o,)


def _edges(fn, arrays, ns):
    """fn on the cases cycled up to n items: every item bitwise the item run alone"""
    arrays = [d(a) for a in arrays]
    m = arrays[0].shape[0]
    alone = [_as_tuple(fn(*(a[i:i + 1] for a in arrays))) for i in range(m)]
    alone = [torch.cat([o[k] for o in alone]) for k in range(len(alone[0]))]
    for n in ns:
        idx = torch.arange(n, device="cuda") % m
        out = _as_tuple(fn(*(a[idx].contiguous() for a in arrays)))
        for o, al in zip(out, alone):
            assert bits_equal(o, al[idx]), (fn, n)


def test_one_thread_per_item_kernels_at_the_256_block_edge():
    from robustcap_amd import body as B
    ns = (1, 255, 256, 257)
    _edges(B.r6d_to_rotation_matrix, P.r6d_cases().x, ns)
    _edges(B.axis_angle_to_rotation_matrix, P.aa_cases().x, ns)
    _edges(B.rotation_matrix_to_axis_angle, P.r2aa_cases().x, ns)
    _edges(B.angle_between, P.angle_cases().x, ns)
    R = P.synth.normal(105, 0, 30 * 9).reshape(30, 3, 3)
    _edges(B.rotation_matrix_to_r6d, (R,), (42, 43, 128))                                      # 6 threads per item


def test_body_kernels_at_their_block_edges(model, body):
    pc = P.pose_cases()
    pose, tran = pc.x
    Rg = P.Ops(body=body).fk_r(pose).float().numpy()
    _edges(model.inverse_kinematics_R, (Rg,), (10, 11, 32))                                    # 24 threads per body
    x = P.synth.normal(106, 0, 13 * 72).reshape(13, 24, 3)
    _edges(model.joint_position_to_bone_vector, (x,), (3, 4, 32))                              # 72 threads per body
    _edges(model.bone_vector_to_joint_position, (x,), (63, 64, 65))                            # 192 threads = 64 bodies
    one_wave = (1, 2, 65)
    _edges(model.forward_kinematics_R, (pose,), one_wave)
    _edges(model.bone_fk, (Rg,), one_wave)
    _edges(lambda p, t: model.forward_kinematics(p, tran=t, calc_mesh=True), (pose, tran), one_wave)
    rc, _ = P.residual_cases(body)
    K = d(P.CAM_K)
    _edges(lambda p, t, k: model.reprojection_residual(p, t, k, K, P.SIGMA), rc.x, one_wave)
    from robustcap_amd.preprocess import synthesize_imu
    _edges(lambda p, t: tuple(o for i, o in enumerate(synthesize_imu(model, p, t, smooth_n=1)) if i != 1), (pose, tran), one_wave)


def test_wave_per_row_ops_at_their_edges():
    from robustcap_amd import body as B
    _edges(B.normalize_keypoints, P.bbox_cases().x, (1, 2, 65))
    for w in (7, 64, 65, 129):
        x = P.synth.normal(107, w, 9 * w).reshape(9, w)
        _edges(lambda v: B.normalize_tensor(v, return_norm=True), (x,), (1, 2, 65))


def test_empty_batches_give_empty_tensors(model):
    from robustcap_amd import body as B
    from robustcap_amd.preprocess import _syn_acc, synthesize_imu
    z = lambda *s: torch.zeros(*s)
    assert B.r6d_to_rotation_matrix(z(0, 6)).shape == (0, 3, 3)
    assert B.axis_angle_to_rotation_matrix(z(0, 3)).shape == (0, 3, 3)
    assert B.rotation_matrix_to_axis_angle(z(0, 3, 3)).shape == (0, 3)
    assert B.rotation_matrix_to_r6d(z(0, 3, 3)).shape == (0, 6)
    assert B.angle_between(z(0, 3, 3), z(0, 3, 3)).shape == (0,)
    assert B.lerp(z(0, 5), z(0, 5), 0.3).shape == (0, 5)
    out, nrm = B.normalize_tensor(z(0, 7), return_norm=True)
    assert out.shape == (0, 7) and nrm.shape == (0, 1)
    assert B.normalize_keypoints(z(0, 33, 3)).shape == (0, 33, 3)
    assert model.inverse_kinematics_R(z(0, 24, 3, 3)).shape == (0, 24, 3, 3)
    assert model.forward_kinematics_R(z(0, 24, 3, 3)).shape == (0, 24, 3, 3)
    assert model.bone_fk(z(0, 24, 3, 3)).shape == (0, 24, 3)
    assert model.bone_vector_to_joint_position(z(0, 24, 3)).shape == (0, 24, 3)
    assert model.joint_position_to_bone_vector(z(0, 24, 3)).shape == (0, 24, 3)
    assert [tuple(o.shape) for o in model.forward_kinematics(z(0, 24, 3, 3), tran=z(0, 3), calc_mesh=True)] == [(0, 24, 3, 3), (0, 24, 3), (0, 33, 3)]
    assert model.reprojection_residual(z(0, 24, 3, 3), z(0, 3), z(0, 33, 3), torch.eye(3)).shape == (0, 33)
    assert _syn_acc(z(0, 18), smooth_n=3).shape == (0, 18)
    assert [tuple(o.shape) for o in synthesize_imu(model, z(0, 24, 3, 3), z(0, 3))] == [(0, 6, 3, 3), (0, 6, 3), (0, 24, 3), (0, 6, 3)]


def test_zz_report_worst_ratios():
    """The largest error / Bound per op over the tests above (pytest -s shows it)."""
    if not WORST.w:
        print("no test of this file ran before the report")
        return
    lines = WORST.lines("device (rc_ops.hip, rc_frame.hip per-op kernels, rc_preprocess.hip): worst error / Bound per op")
    for ln in lines:
        print(ln)
    path = os.environ.get("RC_POSE_OPS_RATIOS_OUT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")
    assert max(v for v, _ in WORST.w.values()) <= 1.0
