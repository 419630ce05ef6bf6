"""Parity of the HIP path (through the C ABI) against the reference-captured golden vectors and the CPU oracle.

Run on the GPU box: python -m pytest tests -m gpu. Tolerances (north star): joint positions 1e-4 m, joint
angles 0.1 deg (float64 atan2 form); per-op kernels 2e-6; branch traces exact.
"""
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

t = torch.from_numpy


def maxdiff(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())


@pytest.fixture(scope="module")
def ops(golden_dir):
    return np.load(os.path.join(golden_dir, "ops.npz"))


@pytest.fixture(scope="module")
def pm(synth_assets):
    from robustcap_amd.body import ParametricModel
    return ParametricModel(body=synth_assets["body"])


def make_net(synth_assets, batch=1, live_ctor=False):
    """live_ctor mirrors `Net.live = True` BEFORE construction (evaluate.py:392). Like the reference, `live` stays
    a class attribute that the instance reads at call time, so the caller resets it when the scenario is over."""
    from robustcap_amd.net.sig_mp import Net
    Net.live = live_ctor
    net = Net(body=synth_assets["body"], batch=batch)
    net.load_state_dict(synth_assets["state_dict"])
    return net


@pytest.fixture(autouse=True)
def _reset_class_live():
    yield
    from robustcap_amd.net.sig_mp import Net
    Net.live = False


def make_oracle(synth_assets, batch=1, live_ctor=False):
    from oracle import sig_mp_oracle as O
    o = O.OracleNet(synth_assets["body"], batch=batch, live=live_ctor)
    o.load_numpy_state_dict(synth_assets["state_dict"])
    return o


# ---------------------------------------------------------------------------------------------------- per-op
def test_library_is_the_hip_one():
    from robustcap_amd import _lib
    lib = _lib.load()
    assert os.path.samefile(lib._name, _lib.LIB_PATH)
    maps = open("/proc/self/maps").read()
    assert "librobustcap_hip.so" in maps and "libamdhip64" in maps


def test_r6d(ops):
    from robustcap_amd.body import r6d_to_rotation_matrix
    out = r6d_to_rotation_matrix(t(ops["r6d_in"]))
    assert maxdiff(out, ops["r6d_out"]) <= 2e-6
    assert float(out[-1, :, 0].abs().max()) == 0.0 and not torch.isnan(out).any()
    assert r6d_to_rotation_matrix(torch.zeros(0, 6)).shape == (0, 3, 3)            # empty input


def test_axis_angle_both_ways(ops):
    from oracle import sig_mp_oracle as O
    from robustcap_amd.body import axis_angle_to_rotation_matrix, rotation_matrix_to_axis_angle
    R = axis_angle_to_rotation_matrix(t(ops["aa_in"]))
    assert maxdiff(R, ops["aa_out"]) <= 2e-6                                       # vs the reference (pure torch there)
    aa = rotation_matrix_to_axis_angle(t(ops["aa_out"]))                           # unpinned vs cv2: round trip + oracle
    assert maxdiff(axis_angle_to_rotation_matrix(aa), ops["aa_out"]) <= 5e-6
    assert maxdiff(aa, O.rotation_matrix_to_axis_angle(t(ops["aa_out"]))) <= 5e-6
    assert float(aa.norm(dim=1).max()) <= 3.1416 and float(aa[0].abs().max()) == 0.0   # identity -> zero vector
    half = torch.tensor([[[1.0, 0, 0], [0, -1, 0], [0, 0, -1]], [[-1.0, 0, 0], [0, -1, 0], [0, 0, 1]]])   # theta = pi
    out = rotation_matrix_to_axis_angle(half).cpu()
    assert maxdiff(out.abs(), torch.tensor([[3.14159265, 0, 0], [0, 0, 3.14159265]])) <= 1e-6
    assert rotation_matrix_to_axis_angle(torch.zeros(0, 3, 3)).shape == (0, 3)


def test_ik_and_bone_fk(ops, pm):
    assert maxdiff(pm.inverse_kinematics_R(t(ops["ik_in"])), ops["ik_out"]) <= 2e-6
    from oracle import sig_mp_oracle as O
    ob = O.OracleBody(pm._body)
    Rg = t(ops["fk_grot"])
    assert maxdiff(pm.bone_fk(Rg), ob.bone_fk(Rg)) <= 2e-6
    # bone FK of zero-pose globals = rest joints
    eye = torch.eye(3).expand(1, 24, 3, 3).contiguous()
    assert maxdiff(pm.bone_fk(eye)[0], ob.j_rest) <= 1e-6


def test_model_surface_vs_reference_vectors(ops, pm, synth_assets):
    """The rest of the ParametricModel / art.math surface SURVEY.md 8(b) lists, each on its HIP entry point against the
    vectors the reference itself produced (oracle/capture_reference.py: fkr_out, bonefk_*, bone_rest, bbox_*, lerp_*,
    rot2r6d_out, norm_*)."""
    from robustcap_amd import body as B
    assert maxdiff(pm.forward_kinematics_R(t(ops["ik_out"])), ops["fkr_out"]) <= 2e-6        # FK_R(IK_R(R)) from the reference
    assert maxdiff(pm.forward_kinematics_R(t(ops["ik_out"])), ops["ik_in"]) <= 5e-6          # ... which is R again
    assert maxdiff(pm.bone_vector_to_joint_position(t(ops["bonefk_in"])), ops["bonefk_out"]) <= 1e-6
    assert maxdiff(pm.joint_position_to_bone_vector(t(ops["bonefk_out"])), ops["bonefk_in"]) <= 2e-6
    j0, v0 = pm.get_zero_pose_joint_and_vertex()
    body = synth_assets["body"]
    assert maxdiff(j0, body["J"] - body["J"][:1]) == 0.0 and maxdiff(v0, body["v_template"] - body["J"][:1]) == 0.0
    assert maxdiff(pm.joint_position_to_bone_vector(j0.view(1, 24, 3))[0], ops["bone_rest"]) <= 1e-7
    assert pm.parent[0] is None and pm.parent[1:] == [int(p) for p in body["parent"][1:]]
    assert maxdiff(B.normalize_keypoints(t(ops["bbox_in"])), ops["bbox_out"]) <= 1e-6
    for k, want in zip(ops["lerp_k"], ops["lerp_out"]):
        assert maxdiff(B.lerp(t(ops["lerp_a"]), t(ops["lerp_b"]), float(k)), want) == 0.0     # double weights, no fma
    assert maxdiff(B.rotation_matrix_to_r6d(t(ops["ik_in"])), ops["rot2r6d_out"]) == 0.0
    assert maxdiff(B.r6d_to_rotation_matrix(B.rotation_matrix_to_r6d(t(ops["ik_in"]))), ops["ik_in"].reshape(-1, 3, 3)) <= 2e-6
    n, ln = B.normalize_tensor(t(ops["norm_in"]), return_norm=True)
    ok = np.isfinite(ops["norm_out"]).all(axis=1)
    assert maxdiff(n.cpu().numpy()[ok], ops["norm_out"][ok]) <= 2e-7 and maxdiff(ln, ops["norm_len"]) <= 1e-6
    assert torch.isnan(n[~torch.from_numpy(ok)]).all()                                       # zero row -> NaN like the reference
    assert n.shape == ops["norm_out"].shape and ln.shape == ops["norm_len"].shape
    # angle_between goes through the (unpinned) Rodrigues vector: checked against the known angle of a constructed offset
    aa = t(ops["aa_in"])
    R = B.axis_angle_to_rotation_matrix(aa)
    base = t(ops["ik_in"]).reshape(-1, 3, 3)[:R.shape[0]].cuda()
    ang = B.angle_between(base, base @ R)
    want = aa.norm(dim=1)
    want = torch.where(want > np.pi, 2 * np.pi - want, want)
    assert maxdiff(ang, want) <= 2e-4                                                        # float32 products near pi


def test_shaped_body_vs_reference_vectors(ops, synth_assets):
    """forward_kinematics(shape=...) / get_zero_pose_joint_and_vertex(shape) (articulate/model.py:88-92, 209-241): shape
    blendshapes + joint regressor on the device (rc_shape_body), then the ordinary kernels on the shaped constants."""
    from robustcap_amd.body import ParametricModel
    model = ParametricModel(body=synth_assets["body"])
    beta = t(ops["shape_beta"])
    j0, v0 = model.get_zero_pose_joint_and_vertex(beta)
    ids = [int(i) for i in ops["fk_vert_extra_ids"]]
    assert maxdiff(j0, ops["shape_j0"]) <= 1e-6 and maxdiff(v0[ids], ops["shape_v0_extra"]) <= 1e-6
    N = ops["fk_pose"].shape[0]
    G, J, L = model.forward_kinematics(t(ops["fk_pose"]), shape=beta.view(1, 10).expand(N, 10), tran=t(ops["fk_tran"]), calc_mesh=True)
    assert maxdiff(J, ops["shape_joint"]) <= 2e-6 and maxdiff(L, ops["shape_j33"]) <= 2e-6
    assert maxdiff(model.forward_mesh(t(ops["fk_pose"]), t(ops["fk_tran"]))[:, ids], ops["shape_vert_extra"]) <= 2e-6
    assert maxdiff(J, ops["fk_joint"]) > 1e-3                                              # the shape really moved the joints
    G0, J0, L0 = model.forward_kinematics(t(ops["fk_pose"]), tran=t(ops["fk_tran"]), calc_mesh=True)   # shape=None: mean body again
    assert maxdiff(J0, ops["fk_joint"]) <= 2e-6 and maxdiff(L0, ops["fk_j33"]) <= 2e-6
    # per-row shapes (model.py:209-229 takes [batch, 10]): frames of different subjects in one call -- here shaped and mean
    # (beta = 0) frames interleaved: every frame must equal its own single-shape run
    rows = torch.zeros(N, 10)
    rows[::2] = beta
    Gm, Jm, Lm = model.forward_kinematics(t(ops["fk_pose"]), shape=rows, tran=t(ops["fk_tran"]), calc_mesh=True)
    assert torch.equal(Jm[::2], J[::2]) and torch.equal(Lm[::2], L[::2]) and torch.equal(Gm, G)
    # (beta = 0 goes through the joint regressor, model.py:88-91; only for a real SMPL file is that the pickled mean J)
    Gz, Jz, Lz = model.forward_kinematics(t(ops["fk_pose"][1::2]), shape=torch.zeros(10), tran=t(ops["fk_tran"][1::2]), calc_mesh=True)
    assert torch.equal(Jm[1::2], Jz) and torch.equal(Lm[1::2], Lz)
    jz, vz = model.get_zero_pose_joint_and_vertex(rows[:3])
    assert jz.shape == (3, 24, 3) and vz.shape[0] == 3 and torch.equal(jz[0], j0) and torch.equal(jz[2], j0)
    assert torch.equal(jz[1], model.get_zero_pose_joint_and_vertex(torch.zeros(10))[0])
    with pytest.raises(ValueError):
        model.forward_kinematics(t(ops["fk_pose"][:3]), shape=rows[:2])                   # neither one row nor one per frame


def test_body_fk_landmarks(ops, pm):
    G, J, L = pm.forward_kinematics(t(ops["fk_pose"]), tran=t(ops["fk_tran"]), calc_mesh=True)
    assert maxdiff(G, ops["fk_grot"]) <= 2e-6
    assert maxdiff(J, ops["fk_joint"]) <= 2e-6
    assert maxdiff(L, ops["fk_j33"]) <= 2e-6
    G2, J2 = pm.forward_kinematics(t(ops["fk_pose"]))                                 # tran=None
    assert maxdiff(J2 + t(ops["fk_tran"]).cuda().view(-1, 1, 3), ops["fk_joint"]) <= 2e-6


def test_reprojection_residual(ops, pm):
    r = pm.reprojection_residual(t(ops["res_pose"]), t(ops["res_tran"]), t(ops["res_kp"]), t(ops["res_K"]))
    scale = float(np.abs(ops["res_loss"]).max())
    assert maxdiff(r, ops["res_loss"]) <= 2e-6 * scale
    assert float(r[:, [1, 5, 9, 31, 32]].abs().max()) == 0.0


# --------------------------------------------------------------------------------------------- sub-net steps
@pytest.mark.parametrize("split", [False, True], ids=["fp32mfma", "splitbf16"])
@pytest.mark.parametrize("name", ["rnn2", "rnn3", "rnn4", "rnn6", "rnn7", "rnn8"])
def test_lstm_step_vs_torch(name, split, synth_assets):
    """f(i, x) of one sub-net for 5 steps incl. a masked step, vs torch.nn.LSTM on the CPU (oracle module), in both product
    arithmetics of the gate GEMM (rc_set_gemm_mode): fp32 MFMA and split-bf16 partial products."""
    from robustcap_amd import config as C, synth
    B = 37                                                      # ragged: not a multiple of the 32-row tile
    nin = {n: i for n, i, _, _ in C.NETS}[name]
    net = make_net(synth_assets, batch=B)
    net.set_gemm_mode(split)
    assert net.gemm_mode == int(split)
    ora = make_oracle(synth_assets, batch=B)
    for step in range(5):
        x = t(synth.normal(50 + step, 1, B * nin).reshape(B, nin))
        rows = None
        if step == 3:
            rows = torch.zeros(B, dtype=torch.bool)
            rows[[0, 5, 31, 32, 36]] = True
        y = net.lstm_step(name, x, rows)
        idx = None if rows is None else rows.nonzero().flatten()
        yo = ora._step(name, x, idx)
        got = y.cpu() if rows is None else y.cpu()[idx]
        assert maxdiff(got, yo) <= 2e-5, (name, step)
    h, c = net.get_state(name)
    assert maxdiff(h, ora.h[name]) <= 2e-5 and maxdiff(c, ora.c[name]) <= 2e-5


def test_partial_state_dict_reload_goes_on_top_of_the_previous_load(synth_assets):
    """load_state_dict(strict=False) with a subset of the keys (torch semantics): the library keeps no host copy of the
    weights, the Python host re-sends the tensors of the earlier loads by reference."""
    sd = dict(synth_assets["state_dict"])
    net = make_net(synth_assets, 3)
    x = t(np.linspace(-1, 1, 3 * 141, dtype=np.float32).reshape(3, 141))
    y0 = net.lstm_step("rnn7", x).cpu()
    w = np.array(sd["rnn7.linear2.weight"], copy=True) * 0.5
    res = net.load_state_dict({"rnn7.linear2.weight": w}, strict=False)
    assert len(res.missing_keys) == len(sd) - 1 and not res.unexpected_keys
    net.reset_states()
    y1 = net.lstm_step("rnn7", x).cpu()
    full = make_net({"state_dict": {**sd, "rnn7.linear2.weight": w}, "body": synth_assets["body"]}, 3)
    y2 = full.lstm_step("rnn7", x).cpu()
    assert torch.equal(y1, y2) and not torch.equal(y0, y1)
    with pytest.raises(RuntimeError):
        net.load_state_dict({"rnn7.linear2.weight": w})                       # strict: every key is required


# ------------------------------------------------------------------------------------------- full sequences
SEQS = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "seq_*.npz")))


def joint_positions(body, pose, tran):
    from oracle import sig_mp_oracle as O
    ob = O.OracleBody(body)
    return ob.forward_kinematics(pose.reshape(-1, 24, 3, 3), tran.reshape(-1, 3))[1]


@pytest.mark.parametrize("split", [False, True], ids=["fp32mfma", "splitbf16"])
@pytest.mark.parametrize("path", SEQS, ids=[os.path.basename(p)[4:-4] for p in SEQS])
def test_sequence_vs_reference_capture(path, split, synth_assets):
    """forward_online (batch 1, frame by frame, like evaluate.py) against the REFERENCE's own outputs, in both product
    arithmetics of the GEMMs (batch-1 contexts default to the fp32 MFMA, batch >= 48 to the split-bf16 products)."""
    from oracle import sig_mp_oracle as O
    s = np.load(path)
    live = str(s["live"])
    net = make_net(synth_assets, 1, live_ctor=(live == "pre"))
    net.set_gemm_mode(split)
    if live == "post":
        net.live = True
    net.use_flat_floor = bool(s["use_flat_floor"])
    net.use_reproj_opt = bool(s["use_reproj_opt"]) if "use_reproj_opt" in s else False
    net.use_vision_updater = bool(s["use_vision_updater"]) if "use_vision_updater" in s else True
    net.use_imu_updater = bool(s["use_imu_updater"]) if "use_imu_updater" in s else True
    net.gravityc = t(s["gravityc"])
    ft = t(s["first_tran"]) if s["first_tran"].size else None
    T = s["pose"].shape[0]
    regime = O.fixture_regimes(s)                              # the reference's float32 mean, its double compares
    poses, trans = [], []
    for i in range(T):
        p, tr = net.forward_online(t(s["j2dc"][i]), t(s["accc"][i]), t(s["oric"][i]), ft if i == 0 else None,
                                   bool(s["first_frame"]) and i == 0)
        tc = net.get_trace()[0].tolist()
        exp = s["trace"][i]
        assert tc[0] == int(regime[i]), f"frame {i}: regime {tc[0]}, the reference's {regime[i]}"
        assert tc[1] == int(exp[1]) and tc[2] == int(exp[2]), f"frame {i}: rnn4/rnn6 step counts {tc} vs {exp}"
        assert tc[3] == int(exp[4]) and tc[4] == int(exp[5]), f"frame {i}: floor/reach {tc} vs {exp}"
        poses.append(p), trans.append(tr)
    pose, tran = torch.stack(poses), torch.stack(trans)
    rp, rt = t(s["pose"]), t(s["tran"])
    assert maxdiff(tran, rt) <= 1e-4
    assert float(O.rotation_angle_deg(pose, rp).max()) <= 0.1
    assert maxdiff(joint_positions(synth_assets["body"], pose, tran), joint_positions(synth_assets["body"], rp, rt)) <= 1e-4
    for n in ("rnn2", "rnn3", "rnn4", "rnn6", "rnn7", "rnn8"):
        h, c = net.get_state(n)
        assert maxdiff(h[:, 0], s["h_" + n]) <= 1e-4 and maxdiff(c[:, 0], s["c_" + n]) <= 2e-4, n


def test_batched_sequence_vs_oracle(synth_assets):
    """forward_sequence on a ragged batch in mixed regimes == the oracle, row by row, incl. the branch trace."""
    from oracle import sig_mp_oracle as O
    from robustcap_amd import synth
    B, T = 11, 72
    m = synth.make_motion(77, B, T, synth_assets["body"], conf="mixed")
    m["j2dc"][3, :20, :, 2] = 0.45
    net = make_net(synth_assets, B)
    ora = make_oracle(synth_assets, B)
    net.gravityc = t(m["gravityc"])
    ora.gravityc = t(m["gravityc"])
    pose, tran = net.forward_sequence(t(m["j2dc"]), t(m["accc"]), t(m["oric"]), first_tran=t(m["first_tran"]))
    op, ot = [], []
    for i in range(T):
        p, tr = ora.forward_batch(t(m["j2dc"][:, i]), t(m["accc"][:, i]), t(m["oric"][:, i]), t(m["first_tran"]) if i == 0 else None)
        op.append(p), ot.append(tr)
    op, ot = torch.stack(op, 1), torch.stack(ot, 1)
    assert maxdiff(tran, ot) <= 1e-4
    assert float(O.rotation_angle_deg(pose.cpu(), op).max()) <= 0.1
    assert maxdiff(joint_positions(synth_assets["body"], pose.cpu(), tran.cpu()), joint_positions(synth_assets["body"], op, ot)) <= 1e-4
    tr = net.get_trace()
    assert tr[:, 3].tolist() == ora.trace["n_floor"].tolist()
    assert tr[:, 5].tolist() == ora.trace["use_vel"].long().tolist()       # velocity branch, stance foot, jump reset of the last frame
    assert tr[:, 6].tolist() == ora.trace["foot"].tolist()
    assert tr[:, 7].tolist() == ora.trace["far"].long().tolist()


def test_step_api_equals_sequence_api_bitwise(synth_assets):
    from robustcap_amd import synth
    B, T = 5, 24
    m = synth.make_motion(91, B, T, synth_assets["body"], conf="mixed")
    a, b = make_net(synth_assets, B), make_net(synth_assets, B)
    a.gravityc = b.gravityc = t(m["gravityc"])
    ps, ts = a.forward_sequence(t(m["j2dc"]), t(m["accc"]), t(m["oric"]), first_frame=True)
    for i in range(T):
        p, tr = b.forward_batch(t(m["j2dc"][:, i]), t(m["accc"][:, i]), t(m["oric"][:, i]), None, i == 0)
        assert torch.equal(p, ps[:, i]) and torch.equal(tr, ts[:, i])


def test_reset_states_and_row_mask(synth_assets):
    """reset_states() restores a fresh sequence; a row mask resets only those rows (bitwise)."""
    from robustcap_amd import synth
    B, T = 4, 16
    m = synth.make_motion(93, B, T, synth_assets["body"], conf="high")
    net = make_net(synth_assets, B)
    net.gravityc = t(m["gravityc"])
    args = (t(m["j2dc"]), t(m["accc"]), t(m["oric"]))
    p1, t1 = net.forward_sequence(*args)
    net.reset_states()
    p2, t2 = net.forward_sequence(*args)
    assert torch.equal(p1, p2) and torch.equal(t1, t2)
    # continue rows 0,2; restart rows 1,3
    net.reset_states(rows=torch.tensor([0, 1, 0, 1]))
    p3, t3 = net.forward_sequence(*args)
    assert torch.equal(p3[[1, 3]], p1[[1, 3]]) and torch.equal(t3[[1, 3]], t1[[1, 3]])
    assert not torch.equal(t3[[0, 2]], t1[[0, 2]])


def test_error_behaviour(synth_assets):
    from robustcap_amd import _lib
    from robustcap_amd.net.sig_mp import Net
    net = Net(body=synth_assets["body"], batch=1)
    with pytest.raises(_lib.RobustcapLibraryError):            # weights not loaded -> loud error, no fallback
        net.forward_online(torch.zeros(33, 3), torch.zeros(6, 3), torch.eye(3).repeat(6, 1, 1))
    bad = dict(synth_assets["state_dict"])
    bad.pop("rnn4.linear1.bias")
    with pytest.raises(RuntimeError):
        net.load_state_dict(bad)
    with pytest.raises(_lib.RobustcapLibraryError):
        Net(body=synth_assets["body"], batch=1, device="cpu")


def test_default_construction_reads_the_smpl_pickle(synth_assets, tmp_path, monkeypatch):
    """`Net()` with no body= (net/sig_mp.py:19-20 -> articulate/model.py:29-40): models/SMPL_male.pkl of the working directory,
    official layout, through body.load_smpl_pickle -- the same outputs as the net built from the dict; no pickle -> loud error."""
    from oracle.capture_reference import _write_body_pickle
    from robustcap_amd import synth
    from robustcap_amd.net.sig_mp import Net
    monkeypatch.chdir(tmp_path)
    with pytest.raises(FileNotFoundError):
        Net()
    _write_body_pickle(str(tmp_path / "models" / "SMPL_male.pkl"), synth_assets["body"])
    a = Net()
    a.load_state_dict(synth_assets["state_dict"])
    b = make_net(synth_assets, 1)
    m = synth.make_motion(99, 1, 12, synth_assets["body"], conf="mixed")
    m["j2dc"][0, 4:9, :, 2] = 0.4                                 # occluded frames: the landmark skinning (w33 / v33 of the pickle) feeds the updater
    a.gravityc = b.gravityc = t(m["gravityc"])
    for i in range(12):
        args = (t(m["j2dc"][0, i]), t(m["accc"][0, i]), t(m["oric"][0, i]))
        pa, ta = a.forward_online(*args, first_frame=(i == 0))
        pb, tb = b.forward_online(*args, first_frame=(i == 0))
        assert torch.equal(pa, pb) and torch.equal(ta, tb), i


def test_live_graph_step_equals_eager(synth_assets, monkeypatch):
    """config 5: the hipGraph-captured frame-stepped frame (host tensors in/out) == the ordinary enqueue path, bitwise.
    (RC_LIVE_LEAN=0: every live frame on the frame-stepped captures; the lean seven-launch capture that batch <= 4 replays for
    steady-state frames by default has its own tests, tests/test_gpu_live.py.)"""
    from robustcap_amd import synth
    monkeypatch.setenv("RC_LIVE_LEAN", "0")
    T = 40
    m = synth.make_motion(95, 1, T, synth_assets["body"], conf="mixed")
    m["j2dc"][0, 10:25, :, 2] = 0.4                              # an occluded stretch: exercises the deferred updater
    for i, c in zip(range(28, 36), (0.7, 0.70001, 0.69999, 0.7, 0.9, 0.69995, 0.70005, 0.5)):
        m["j2dc"][0, i, :, 2] = c                                # hugging conf_lo: the host-side graph choice must stay safe
    a, b = make_net(synth_assets, 1), make_net(synth_assets, 1)
    a.gravityc = b.gravityc = t(m["gravityc"])
    b.use_graph = True
    from oracle import sig_mp_oracle as O
    ora = make_oracle(synth_assets, 1)                           # ... and both right: the oracle sums the means in the reference's order
    ora.gravityc = t(m["gravityc"])
    for i in range(T):
        args = (t(m["j2dc"][0, i]), t(m["accc"][0, i]), t(m["oric"][0, i]))
        pa, ta = a.forward_online(*args, first_frame=(i == 0))
        pb, tb = b.forward_online(*args, first_frame=(i == 0))
        assert torch.equal(pa, pb) and torch.equal(ta, tb), i
        po, to = ora.forward_online(*args, first_frame=(i == 0))
        assert a.get_trace()[0].tolist()[:3] == [int(O.conf_regimes(ora.trace["c"].numpy(), 0.7, 0.8)[0]), int(ora.trace["n4"][0]),
                                                  int(ora.trace["n6"][0])], i
        assert maxdiff(ta, to) <= 1e-4 and float(O.rotation_angle_deg(pa.cpu(), po).max()) <= 0.1, i
    b.use_flat_floor = False                                     # attribute poke re-captures the graph
    a.use_flat_floor = False
    for i in range(T - 5, T):
        args = (t(m["j2dc"][0, i]), t(m["accc"][0, i]), t(m["oric"][0, i]))
        pa, ta = a.forward_online(*args)
        pb, tb = b.forward_online(*args)
        assert torch.equal(pa, pb) and torch.equal(ta, tb)


def test_mass_regime_transition_vs_oracle(synth_assets):
    """Every row leaves the occluded regime in the same frame: the deferred updater steps of ALL rows become
    transition steps at once (far more rows than the narrow transition launch is sized for) -- and back again."""
    from oracle import sig_mp_oracle as O
    from robustcap_amd import synth
    B, T = 70, 30
    m = synth.make_motion(123, B, T, synth_assets["body"], conf="high")
    m["j2dc"][:, 5:12, :, 2] = 0.5          # all rows occluded for frames 5..11, visible again from 12
    m["j2dc"][:, 20:24, :, 2] = 0.55
    net, ora = make_net(synth_assets, B), make_oracle(synth_assets, B)
    net.gravityc = t(m["gravityc"])
    ora.gravityc = t(m["gravityc"])
    pose, tran = net.forward_sequence(t(m["j2dc"]), t(m["accc"]), t(m["oric"]), first_frame=True)
    for i in range(T):
        p, tr = ora.forward_batch(t(m["j2dc"][:, i]), t(m["accc"][:, i]), t(m["oric"][:, i]), None, i == 0)
        assert maxdiff(tran[:, i], tr) <= 1e-4, i
        assert float(O.rotation_angle_deg(pose[:, i].cpu(), p).max()) <= 0.1, i
    for n in ("rnn4", "rnn6"):
        h, c = net.get_state(n)
        assert maxdiff(h, ora.h[n]) <= 1e-4 and maxdiff(c, ora.c[n]) <= 2e-4, n


def test_live_session_over_the_wire_format(synth_assets):
    """live_server.py loop on the GPU path: detector packets in, Unity packets out; poses equal a direct run."""
    from robustcap_amd import live, synth
    from robustcap_amd.body import rotation_matrix_to_axis_angle
    T = 12
    m = synth.make_motion(97, 1, T, synth_assets["body"], conf="high")
    rcm = synth._rodrigues(np.array([0.1, 0.2, -0.05])).astype(np.float32)
    net = make_net(synth_assets, 1)
    net.live = True                                               # live_server.py:64-65
    net.use_graph = True
    sess = live.LiveSession(net)
    ref = make_net(synth_assets, 1)
    ref.live = True
    ref.use_graph = True                                          # the same captures as the session's net: packets equal digit for digit
    ref.gravityc = t(rcm) @ torch.tensor([0.0, -1.0, 0.0])
    first = None
    for i in range(-1, T):
        k = max(i, 0)
        out = sess.handle(live.format_detector_packet(m["j2dc"][0, k], m["oric"][0, k], m["accc"][0, k], rcm))
        if i < 0:
            assert out is None
            continue
        p, tr = ref.forward_online(t(m["j2dc"][0, k]), t(m["accc"][0, k]), t(m["oric"][0, k]), first_frame=(i == 0))
        p = p.clone()
        p[0] = t(rcm).T @ p[0]
        tr = t(rcm).T @ tr
        first = tr.clone() if first is None else first
        aa = rotation_matrix_to_axis_angle(p).cpu().view(-1)
        assert out == live.format_unity_packet(aa.tolist(), (tr - first).tolist()), i


@pytest.mark.parametrize("vis,imu", [(False, True), (True, False), (False, False)])
def test_updater_switches_vs_oracle(vis, imu, synth_assets):
    """use_vision_updater / use_imu_updater off (net/sig_mp.py:33-34,178,264): no deferred rnn6/rnn4 steps, no init_net
    write -- against the oracle with the same switches."""
    from oracle import sig_mp_oracle as O
    from robustcap_amd import synth
    B, T = 6, 36
    m = synth.make_motion(131, B, T, synth_assets["body"], conf="mixed")
    m["j2dc"][2, 8:20, :, 2] = 0.45
    m["j2dc"][4, :6, :, 2] = 0.5
    net, ora = make_net(synth_assets, B), make_oracle(synth_assets, B)
    net.use_vision_updater = ora.use_vision_updater = vis
    net.use_imu_updater = ora.use_imu_updater = imu
    net.gravityc = t(m["gravityc"])
    ora.gravityc = t(m["gravityc"])
    pose, tran = net.forward_sequence(t(m["j2dc"]), t(m["accc"]), t(m["oric"]), first_frame=True)
    for i in range(T):
        p, tr = ora.forward_batch(t(m["j2dc"][:, i]), t(m["accc"][:, i]), t(m["oric"][:, i]), None, i == 0)
        assert maxdiff(tran[:, i], tr) <= 1e-4, i
        assert float(O.rotation_angle_deg(pose[:, i].cpu(), p).max()) <= 0.1, i
    for n in ("rnn2", "rnn4", "rnn6"):
        h, c = net.get_state(n)
        assert maxdiff(h, ora.h[n]) <= 1e-4 and maxdiff(c, ora.c[n]) <= 2e-4, n
    tr8 = net.get_trace()
    if not imu:
        assert int(tr8[:, 4].sum()) == 0                                   # init_net never fired


def test_rotmat_to_axis_angle_against_scipy():
    """The reference calls OpenCV's cv2.Rodrigues here (absent: parity with cv2 itself stays unpinned).
    The restatement of its steps (re-orthonormalisation, acos, the s < 1e-5 branches) is cross-checked against scipy's
    independent log map on random rotations, angles close to 0 and to pi, exactly pi, and NON-orthonormal inputs
    (where OpenCV first projects onto the nearest orthonormal matrix)."""
    from scipy.spatial.transform import Rotation
    from robustcap_amd import synth
    from robustcap_amd.body import rotation_matrix_to_axis_angle
    aa = synth.normal(9, 0, 3000).reshape(-1, 3).astype(np.float64)
    aa[:100] *= 1e-4                                                        # tiny angles
    ax = aa[100:200] / np.linalg.norm(aa[100:200], axis=1, keepdims=True)
    aa[100:200] = ax * (np.pi - 0.01 - 0.04 * synth.uniform01(9, 1, 100)[:, None])   # 0.6 .. 2.9 degrees below pi
    n = np.linalg.norm(aa, axis=1)
    aa[n > np.pi] *= ((np.pi - 0.05) / n[n > np.pi])[:, None]                # keep the principal branch
    R = Rotation.from_rotvec(aa).as_matrix().astype(np.float32)
    got = rotation_matrix_to_axis_angle(t(R)).cpu().numpy()
    want = Rotation.from_matrix(R.astype(np.float64)).as_rotvec()
    assert np.abs(got - want).max() <= 2e-4                                  # float32 matrices: the log map is ill-conditioned near pi
    assert np.abs(got[200:] - want[200:]).max() <= 5e-6
    from oracle import sig_mp_oracle as O                                   # SVD-based restatement of the same steps
    assert np.abs(got - O.rotation_matrix_to_axis_angle(t(R)).numpy()).max() <= 2e-6
    # OpenCV's s < 1e-5 band: exactly zero near the identity, sqrt-of-diagonal branch near pi (round trip within float32)
    tiny = Rotation.from_rotvec(ax * 1e-7).as_matrix().astype(np.float32)
    R = tiny
    assert np.abs(rotation_matrix_to_axis_angle(t(R)).cpu().numpy()).max() == 0.0
    for eps in (0.0, 1e-7, 1e-6):
        R = Rotation.from_rotvec(ax * (np.pi - eps)).as_matrix().astype(np.float32)
        got = rotation_matrix_to_axis_angle(t(R)).cpu().numpy().astype(np.float64)
        assert np.abs(np.linalg.norm(got, axis=1) - np.pi).max() <= 2e-5
        assert np.abs(Rotation.from_rotvec(got).as_matrix() - R).max() <= 5e-6
    # non-orthonormal inputs: same answer as the log map of the polar factor U V^T; out-of-range / NaN -> zeros
    noisy = (Rotation.from_rotvec(aa[200:1000]).as_matrix() + 0.05 * synth.normal(9, 5, 7200).reshape(-1, 3, 3)).astype(np.float32)
    R = noisy
    U, _, Vt = np.linalg.svd(noisy.astype(np.float64))
    want = Rotation.from_matrix(U @ Vt).as_rotvec()
    got = rotation_matrix_to_axis_angle(t(R)).cpu().numpy()
    assert np.abs(got - want).max() <= 5e-6
    R = np.stack([np.full((3, 3), 1000.0), np.full((3, 3), np.nan)]).astype(np.float32)
    assert np.abs(rotation_matrix_to_axis_angle(t(R)).cpu().numpy()).max() == 0.0