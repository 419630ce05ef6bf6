"""The bounds of the pose-algebra and IMU-synthesis ops are neither too loose nor too tight, shown without a GPU.

tests/test_gpu_pose_ops_edges.py holds rc_ops.hip, the per-op kernels of rc_frame.hip and rc_preprocess.hip to the bounds of
oracle/pose_ops_f64.py. Here the same cases and bounds meet CPU evaluations:
  * `Ops` in float64 restates the oracle's own functions (the two agree to 1e-12 of the Bound's scale), so its float32
    evaluations and its mutations are evaluations and mutations of the oracle's formulas;
  * four honest float32 evaluations of every op (each sum of products first-term-first or last-term-first, with separate or
    fused multiply-adds), and for angle_between the device's own route (float32 R1^T R2, float64 log map, float32 norm), stay
    at or below a third of the Bound on every case;
  * R -> aa, float64 on both sides: the line-for-line emulation of the kernel's Newton polar route agrees with the oracle's
    SVD route within the derived 2^-22 on every case outside the s ~ 1e-5 window and as a rotation inside it (this bound is
    derived, not measured: one float32 rounding on each side; "a third" has no meaning for it);
  * every single mutation of the list lands beyond three times the Bound on the case named beside it;
  * the case builders hold what they promise: counts, the window cap, the degenerate patterns, both sides of every branch.
RC_POSE_OPS_RATIOS_OUT=<file> keeps the printed tables.
"""
import os

import numpy as np
import pytest
import torch

from oracle import pose_ops_f64 as P
from oracle import sig_mp_oracle as O


def _emit(lines):
    for ln in lines:
        print(ln)
    path = os.environ.get("RC_POSE_OPS_RATIOS_OUT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture(scope="module")
def body(synth_assets):
    return synth_assets["body"]


@pytest.fixture(scope="module")
def suite(body):
    return P.suite(body)


def test_ops_in_float64_restate_the_oracle(suite, body):
    for e in suite:
        r = P.case_ratios(e, P.host_eval(e, body))
        assert float(r.max()) <= 1e-6, (e.op, e.names[int(r.argmax())], float(r.max()))     # 1e-6 of a Bound of a few eps32: 1e-13 relative


def _device_like_angle(e, ar):
    """angle_between as the device routes it: D = R1^T R2 in float32, the float64 log map rounded to float32, its float32 norm"""
    D = ar.mm(P.t32(e.args[0]).transpose(1, 2), P.t32(e.args[1]))
    aa = torch.from_numpy(P.r2aa_newton(D.numpy()))
    return ar.dot(aa, aa).sqrt()


def test_float32_evaluations_stay_within_a_third_of_the_bound(suite, body):
    worst = P.Worst()
    for e in suite:
        for ar in P.VARIANTS:
            worst.note(e.op, P.case_ratios(e, P.host_eval(e, body, ar)), e.names)
            if e.op == "angle":
                worst.note(e.op, P.case_ratios(e, _device_like_angle(e, ar)), e.names)
    _emit(worst.lines(f"CPU, honest float32 evaluations ({len(P.VARIANTS)} per op): worst error / Bound per op (<= 1/{P.MARGIN:g} required)"))
    assert set(worst.w) == set(P.M_OF)
    for op, (v, nm) in worst.w.items():
        assert v <= 1.0 / P.MARGIN, (op, nm, v)


def test_newton_route_agrees_with_the_svd_oracle():
    c = P.r2aa_cases()
    r, win = P.r2aa_errors(P.r2aa_newton(c.x[0]), c.x[0])
    i = int(np.argmax(r))
    _emit([f"CPU, R -> aa: Newton polar route against the SVD oracle, worst error / 2^-22 (in the window: angle / {P.WINDOW_ANGLE:g}): "
           f"{r[i]:.3f} ({c.names[i]}); cases in the window: {int(win.sum())}"])
    assert r.max() <= 1.0, c.names[i]


# mutation -> (op whose entry shows it, a word of the case it must show on)
MUTATIONS = {
    "r6d_no_projection": ("r6d", "generic 4"),
    "r6d_cross_flipped": ("r6d", "orthonormal axes"),
    "aa2R_sin_sign": ("aa2R", "theta 1 axis -y"),
    "aa2R_zero_gives_zeros": ("aa2R", "theta 0 axis generic"),
    "ik_no_transpose": ("ik", "random pose 0"),
    "fk_parent_i_minus_1": ("fk_r", "leaf joint 22"),
    "bone_fk_own_rotation": ("bone_fk", "random pose 1"),
    "landmarks_no_override": ("j33", "identity pose"),
    "bbox_width_only": ("bbox", "tall box"),
    "bbox_row_24": ("bbox", "negative coordinates"),
    "normalize_first_64": ("normalize", "width 65 rows 1"),
    "residual_no_ignore": ("residual", "leaf joint 22 rotated, front"),
    "residual_sigma_not_squared": ("residual", "random pose 0 (joints up to pi), front"),
}
R2AA_MUTATIONS = {
    "r2aa_no_fixup": "half-turn (0,1,-1)/sqrt2",
    "r2aa_no_polar": "perturbed entrywise by 1e-4",
    "r2aa_no_c_exit": "theta 4e-06 (c > 0 exit)",
}


def test_every_mutation_lands_beyond_three_times_the_bound(suite, body):
    lines = [f"mutations: error / Bound on the case named (>= {P.MARGIN:g} required)"]
    for mut, (op, word) in MUTATIONS.items():
        best = 0.0
        for e in suite:
            if e.op != op:
                continue
            r = P.case_ratios(e, P.host_eval(e, body, mut=mut))
            for nm, v in zip(e.names, r):
                if word in nm:
                    best = max(best, float(v))
        lines.append(f"  {mut:28s} {best:12.3g}  {op:9s} {word}")
        assert best >= P.MARGIN, mut
    c = P.r2aa_cases()
    for mut, name in R2AA_MUTATIONS.items():
        r, _ = P.r2aa_errors(P.r2aa_newton(c.x[0], mut), c.x[0])
        v = float(r[c.names.index(name)])
        lines.append(f"  {mut:28s} {v:12.3g}  R -> aa   {name}")
        assert v >= P.MARGIN, mut
    for m in ("1.01 R",):                                                        # the polar step also carries the scaled input
        assert float(P.r2aa_errors(P.r2aa_newton(c.x[0], "r2aa_no_polar"), c.x[0])[0][c.names.index(m)]) >= P.MARGIN
    v = P.t32(P.synth.normal(5, 5, 40 * 18).reshape(40, 18))
    for n in (2, 3, 4):                                                          # compared bitwise on the device: any difference shows
        d = float((P.syn_acc_f64(v, n, "syn_acc_div_n") - P.syn_acc_f64(v, n)).abs().max())
        lines.append(f"  {'syn_acc_div_n':28s} {d:12.3g}  m/s^2 at smooth_n = {n} (the device is compared bit for bit)")
        assert d > 1.0
    _emit(lines)


def test_the_case_builders_hold_their_conditions(suite, body):
    # r6d: magnitudes, angles, the exactly degenerate rows
    c = P.r6d_cases()
    x = c.x[0].astype(np.float64)
    na, nb = np.linalg.norm(x[:, :3], axis=1), np.linalg.norm(x[:, 3:], axis=1)
    gen = [i for i, n in enumerate(c.names) if n.startswith("generic")]
    assert len(gen) == 12 and (na[gen] >= 1e-3).all() and (na[gen] <= 1e3).all() and (nb[gen] >= 1e-3).all() and (nb[gen] <= 1e3).all()
    assert max(na[gen].max(), nb[gen].max()) > 50 and min(na[gen].min(), nb[gen].min()) < 0.02
    for ang in P.R6D_ANGLES:
        idx = [i for i, n in enumerate(c.names) if n.startswith(f"angle {ang:.4g} ")]
        assert len(idx) == 2
        got = np.arccos(np.clip((x[idx, :3] * x[idx, 3:]).sum(1) / (na[idx] * nb[idx]), -1, 1))
        assert np.abs(got - ang).max() <= 1e-5 * max(1.0, 1.0 / np.sin(ang)) ** 2
    deg = c.pick("degenerate")
    assert [n.split("degenerate ")[1] for n in deg.names] == list(P.R6D_DEGENERATE)
    d = deg.x[0]
    assert (d[0, :3] == 0).all() and (d[1, 3:] == 0).all() and (d[2, 3:] == d[2, :3]).all() and (d[3, 3:] == np.float32(-2) * d[3, :3]).all()
    pat = O.r6d_to_rotation_matrix(P.t32(d))
    assert not torch.isnan(pat).any()
    zero = (pat == 0)
    assert zero[0].all()                                                        # a = 0: every column is NaN -> 0
    for k in (1, 2, 3):                                                         # c0 survives, c1 = 0 / 0, c2 with it
        assert zero[k][:, 1:].all() and not zero[k][:, 0].all()
    for ar in P.VARIANTS:                                                       # the pattern does not depend on the arithmetic
        assert torch.equal(P.Ops(ar).r6d(d) == 0, zero)
    # aa -> R
    c = P.aa_cases()
    assert len(c) == len(P.AA_THETAS) * len(P.AA_AXES) == 24
    th32 = np.linalg.norm(c.x[0].astype(np.float64), axis=1)
    assert (th32[:3] == 0).all() and (np.abs(th32[3:6] - 1e-30) < 1e-36).all() and (c.x[0][3:6].astype(np.float32) ** 2).sum() == 0   # squares underflow
    # R -> aa: the window cap from the oracle alone; both sides of s < 1e-5; the special inputs; the fix-up flips
    c = P.r2aa_cases()
    win = P.window_mask(c.x[0])
    assert int(win.sum()) <= P.WINDOW_MAX
    s = P.oracle_s(c.x[0])
    near = [s[c.names.index(f"theta pi - {d:g}")] for d in P.NEAR_PI]
    assert sum(v >= 1e-5 for v in near) == 3 and sum(v < 1e-5 for v in near) == 2
    ref = O.rotation_matrix_to_axis_angle(P.t32(c.x[0])).numpy()
    for nm in ("identity", "theta 1e-06 (c > 0 exit)", "theta 4e-06 (c > 0 exit)", "entry 100 (zero vector)", "entry NaN (zero vector)", "zero matrix (zero vector)"):
        assert (ref[c.names.index(nm)] == 0).all(), nm
    assert np.abs(ref[c.names.index("theta 0.0001")]).max() > 1e-5
    half = [i for i, n in enumerate(c.names) if n.startswith("half-turn")]
    assert len(half) == len(P.HALF_TURN_AXES) == 15
    assert np.abs(np.linalg.norm(ref[half].astype(np.float64), axis=1) - np.pi).max() <= 1e-6
    flipped = [c.names[i] for i in half if not np.array_equal(P.r2aa_newton(c.x[0][i:i + 1], "r2aa_no_fixup"), P.r2aa_newton(c.x[0][i:i + 1]))]
    assert "half-turn (0,1,-1)/sqrt2" in flipped and "half-turn r_x smallest R12 < 0: (0,0.6,-0.8)" in flipped
    for nm, sign in (("R12 > 0: (0,0.6,0.8)", 1), ("R12 < 0: (0,0.6,-0.8)", -1), ("R12 > 0: (0.1,0.7,0.7)", 1), ("R12 < 0: (0.1,-0.7,0.7)", -1)):
        i = c.names.index("half-turn r_x smallest " + nm)
        assert np.sign(c.x[0][i, 1, 2]) == sign and abs(ref[i, 0]) < min(abs(ref[i, 1]), abs(ref[i, 2]))
    imp = c.x[0][c.names.index("improper diag(1,1,-1)")]
    assert np.linalg.det(imp.astype(np.float64)) < 0
    # angle_between
    c = P.angle_cases()
    ref = torch.deg2rad(O.rotation_angle_deg(P.t32(c.x[0]), P.t32(c.x[1]))).numpy()
    assert ref[0] == 0.0 and np.abs(ref[1:5] - np.array(P.ANGLES_BETWEEN)).max() <= 2e-6 and len(c) == 13
    # normalize: widths x row counts, one zero row each in the three-row sets, magnitudes
    nc = P.normalize_cases()
    assert [x.shape for _, x in nc] == [(r, w) for w in P.NORMALIZE_WIDTHS for r in P.NORMALIZE_ROWS]
    for _, x in nc:
        nz = np.abs(x[x != 0])
        assert nz.min() >= 1e-3 and nz.max() <= 1e3
        if x.shape[0] == 3:
            assert (x[1] == 0).all() and torch.isnan(P.t32(x[1]) / P.t32(x[1]).norm()).all()
    # bbox
    c = P.bbox_cases()
    kp = c.x[0].astype(np.float64)
    wd, ht = np.ptp(kp[..., 0], axis=1), np.ptp(kp[..., 1], axis=1)
    i = c.names.index
    assert wd[i("wide box")] > 2 * ht[i("wide box")] and ht[i("tall box")] > 2 * wd[i("tall box")]
    assert kp[i("row 23 max x"), :, 0].argmax() == 23 and kp[i("row 23 min x"), :, 0].argmin() == 23
    assert kp[i("row 23 max y"), :, 1].argmax() == 23 and kp[i("row 23 min y"), :, 1].argmin() == 23
    assert (kp[i("negative coordinates"), :, :2] < 0).all()
    eq = O.normalize_keypoints(P.t32(c.x[0][i("all 33 points equal")][None]))[0]
    assert torch.isinf(eq[23, :2]).all() and torch.isnan(eq[:23, :2]).all() and torch.isnan(eq[24:, :2]).all()
    assert torch.equal(eq[:, 2], P.t32(c.x[0][i("all 33 points equal")])[:, 2])
    # poses and the residual's situations
    pc = P.pose_cases()
    assert len(pc) == 7 and np.abs(pc.x[1]).max() == 100.0
    aa = O.rotation_matrix_to_axis_angle(P.t32(pc.x[0][1:4]).reshape(-1, 3, 3)).norm(dim=1)
    assert float(aa.max()) > 2.8                                                # joints near pi among the random poses
    rc, sig = P.residual_cases(body)
    ob = P.Ops(body=body)
    z = ob.body_fk(rc.x[0], rc.x[1])[2][..., 2]
    front = np.array(["front" in n for n in rc.names])
    assert len(rc) == 14 and front.sum() == 7
    assert (z[front] > 0.5).all() and (z[~front] < -0.5).all()
    assert (rc.x[2][:, [3, 17], 2] == 0).all() and (rc.x[2][:, 4, 2] > 0).all()
    ign = list(P.C.smplify_ignored_landmarks)
    for e in suite:
        if e.op == "residual":
            assert (e.ref[:, ign] == 0).all() and (e.ref[:, [3, 17]] == 0).all()
            live = [k for k in range(33) if k not in ign + [3, 17]]
            d2 = e.ref[:, live] / torch.as_tensor(e.args[2][:, live, 2]).double() ** 2          # gmof_x + gmof_y
            if e.extra == P.SIGMA:
                assert float(d2.max()) < 1e-4 * P.SIGMA ** 2                                     # |d| << sigma
            else:
                assert float(d2.min()) > 0.5 * P.SIGMA_SMALL ** 2                               # |d| >> sigma: gmof saturates at sigma^2
    bc = P.beta_cases()
    assert len(bc) == 5 and (bc.x[0][0] == 0).all() and [int((b != 0).sum()) for b in bc.x[0][1:4]] == [1, 1, 1]
    assert np.abs(bc.x[0][4]).max() <= 5 and body["v_template"].shape[0] == 6890 and 6890 % 256 != 0
