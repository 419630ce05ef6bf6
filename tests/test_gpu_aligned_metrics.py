"""rc_aligned_metrics and rc_svd_rotate (csrc/rc_align.hip): the evaluators' SVD alignments (align_joint -1 .. -5) on the device.

  values     every output (joint_err, mesh_err, per_frame, xform; R, t, s, moved), entry by entry, within Bound = 8 |float32 transcription
             - float64 restatement| + 1e-7 scale of the restatement (tests/aligned_metrics_f64.py), in all five modes. Meshes of V = 5, 1023, 1024,
             1025 (the 1024-vertex slab edge) and 6890; group lengths 1, 2, 3, 31 / 32 / 33 (the 32-frame block) and 65; 40 groups in one
             call (33, 65, 33 at positions 0, 17, 39) for the bisection; near predictions and far ones with improper fits (the row flip).
             rc_svd_rotate at m = 3, 4, 24, 33, 64, 65 points and n = 63, 1, 65, 64, 5, 5 sets, and a mirrored set. Three points are coplanar
             once centred (rank 2): with calc_R only s and the orthogonality of R are compared there.
             RC_ALIGNED_RATIOS_OUT=path: the largest ratio per output is appended when the module is done
             (profiles/aligned_metrics_ratios.txt).
  identities prediction = truth with the root turned far from I: modes -1 and -2 within the Bound of zero, mode -4 not; dst = s R src + t
             gives back R, t, s and moved = dst; mode -4 is the difference of the centred joints.
  bitwise    a group in a batch = the call with it alone, in any order; reruns; a call that regrows the scratch between two small calls;
             RC_MOTION_NO_MESH changes the mesh outputs only; PerJointErrorEvaluator(align_joint=-k)[1:] = the align_joint=0 rows.
  python     the three evaluator classes and body.svd_rotate against the captured fixture (tests/golden/aligned): the Bound with the
             transcription's error taken per block of a fit's entries, as wherever a float32 LAPACK is the other side (see bound());
             evaluate.aligned_metrics on a two-row dataset of unequal lengths = the per-row calls, bitwise.
  bad input  every refusal returns its code and leaves sentinel-filled outputs alone; no mesh: RC_ERR_STATE; align_joint=-6: RuntimeError;
             FullMotionEvaluator(align_joint=-1): NotImplementedError.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import aligned_metrics_f64 as A

pytestmark = pytest.mark.gpu
t = torch.from_numpy
WORST = {}
bits = lambda x: x.contiguous().numpy().view(np.int32)


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """when the module is done: the largest error / Bound per output over its value tests (pytest -s shows it; RC_ALIGNED_RATIOS_OUT keeps it)"""
    yield
    if not WORST:
        return
    lines = [f"device (rc_align.hip), K = {A.K:g}, + {A.REL:g} scale, per entry: worst error / Bound per output"]
    lines += [f"  {row:18s} {v:.3f}  ({what})" for row, (v, what) in sorted(WORST.items())]
    print("\n" + "\n".join(lines))
    path = os.environ.get("RC_ALIGNED_RATIOS_OUT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


def _note(row, ratio, what):
    if row not in WORST or ratio > WORST[row][0]:
        WORST[row] = (float(ratio), what)


def _small_mesh_model(full_body, V):
    """a ParametricModel on the shared body whose mesh has V vertices, and the body dict the restatement reads"""
    from robustcap_amd import _lib, synth
    from robustcap_amd.body import ParametricModel
    m = ParametricModel(body=full_body)
    if V == full_body["v_template"].shape[0]:
        return m, full_body
    small = synth.make_body(1, num_vertex=V)
    assert np.array_equal(small["J"], full_body["J"])
    vt = np.ascontiguousarray(small["v_template"], dtype=np.float32)
    w = np.ascontiguousarray(small["weights"], dtype=np.float32)
    _lib.check(m._ctx, m._lib.rc_set_mesh(m._ctx, vt.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), V), "rc_set_mesh")
    m._mesh_set, m._V = True, V
    return m, small


@pytest.fixture(scope="module")
def models(synth_assets):
    cache = {}

    def model_of(V):
        if V not in cache:
            cache[V] = _small_mesh_model(synth_assets["body"], V)
        return cache[V]
    return model_of


def _dev(a):
    return t(np.ascontiguousarray(a)).cuda()


def _call(model, pp, pt, sizes, mode, mesh=True):
    """(joint_err [G,24], mesh_err [G] or None, per_frame [n,2], xform [n,2,13]) on the CPU"""
    out = model.aligned_metrics(_dev(pp), _dev(pt), group_frames=sizes, align=mode, mesh=mesh, per_frame=True)
    return tuple(None if o is None else o.cpu() for o in out)


def _check(name, mode, got, f64, f32, mesh=True):
    """every output of one call against the restatement; returns the largest ratio per output"""
    je, me, pf, xf = got
    grp = f64["frame_group"]
    r = {"joint_err": A.ratios(je.double().numpy(), f64["joint_err"], A.bound(f32["joint_err"], f64["joint_err"], f64["pos_j"][:, None])),
         "per_frame joint": A.ratios(pf[:, 0].double().numpy(), f64["per_frame"][:, 0],
                                     A.bound(f32["per_frame"][:, 0], f64["per_frame"][:, 0], f64["pos_j"][grp])),
         "xform joint": A.ratios(xf[:, 0].double().numpy(), f64["xform"][:, 0], A.xform_bound(f32["xform"][:, 0], f64["xform"][:, 0], f64["pos_j"][grp]))}
    if mesh:
        r["mesh_err"] = A.ratios(me.double().numpy(), f64["mesh_err"], A.bound(f32["mesh_err"], f64["mesh_err"], f64["pos_v"]))
        r["per_frame mesh"] = A.ratios(pf[:, 1].double().numpy(), f64["per_frame"][:, 1],
                                       A.bound(f32["per_frame"][:, 1], f64["per_frame"][:, 1], f64["pos_v"][grp]))
        r["xform mesh"] = A.ratios(xf[:, 1].double().numpy(), f64["xform"][:, 1], A.xform_bound(f32["xform"][:, 1], f64["xform"][:, 1], f64["pos_v"][grp]))
    worst = {k: float(v.max()) for k, v in r.items()}
    print(f"{name:26s} mode {mode}: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        _note(k, v, f"{name}, mode {mode}")
    return worst


@pytest.mark.parametrize("case", A.CASES, ids=[c[0] for c in A.CASES])
def test_values_within_the_bound(case, models):
    name, V, sizes, seed, far = case
    model, body = models(V)
    pp, pt = A.pose_batch(body, sizes, seed, far)
    for mode in A.MODES:
        f64 = A.evaluate_groups(body, pp, pt, sizes, mode)
        f32 = A.evaluate_groups(body, pp, pt, sizes, mode, np.float32)
        worst = _check(name, mode, _call(model, pp, pt, sizes, mode), f64, f32)
        assert max(worst.values()) <= 1.0, (name, mode, worst)


def _svd(src, dst, calc):
    from robustcap_amd import body as B
    return tuple(o.cpu().double().numpy() for o in B.svd_rotate(_dev(src), _dev(dst), *calc))


def _check_svd(name, m, src, dst, calc, got):
    f64, f32 = A.svd_rotate(src, dst, *calc), A.svd_rotate(src, dst, *calc, dtype=np.float32)
    pos = np.abs(src).max() + np.abs(dst).max() + np.abs(f64[1]).max()
    scales = (1.0, pos, np.maximum(1.0, f64[2]), pos)
    worst = {}
    for k, out in enumerate(("R", "t", "s", "moved")):
        if calc[0] and not A.R_DEFINED(m) and out != "s":
            continue                                                 # three points: rank 2, the sign of det(V U^T) is LAPACK's accident
        r = A.ratios(got[k], f64[k], A.bound(f32[k], f64[k], scales[k]))
        worst[out] = float(r.max())
        _note("svd_rotate " + out, worst[out], f"{name}, {A.flag_name(calc)}")
    assert np.isfinite(got[0]).all() and np.abs(np.matmul(got[0], got[0].transpose(0, 2, 1)) - np.eye(3)).max() < 1e-5
    return worst


@pytest.mark.parametrize("case", A.SVD_CASES, ids=[f"m={c[0]} n={c[1]}" + (" mirrored" if c[3] else "") for c in A.SVD_CASES])
def test_svd_rotate_within_the_bound(case):
    m, n, seed, mirrored = case
    src, dst, _ = A.point_sets(seed, n, m, mirrored)
    extra = ((True, False, False), (False, False, False)) if m >= A.UNCENTRED_FROM else ()   # svd_rotate's default flags, and none at all
    for calc in A.FLAG_COMBOS + extra:
        worst = _check_svd(f"m={m} n={n}", m, src, dst, calc, _svd(src, dst, calc))
        print(f"m={m} n={n} {A.flag_name(calc) or '-':4s}" + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        assert max(worst.values()) <= 1.0, (case, calc, worst)


def test_svd_rotate_recovers_an_exact_transform():
    src, dst, (R, tr, s) = A.exact_point_sets(*A.EXACT_POINTS)
    gR, gt, gs, gm = _svd(src, dst, (True, True, True))
    worst = _check_svd("exact", 24, src, dst, (True, True, True), (gR, gt, gs, gm))
    assert max(worst.values()) <= 1.0, worst
    assert np.abs(gR - R).max() < 1e-5 and np.abs(gt - tr).max() < 1e-5 and np.abs(gs - s).max() < 1e-5
    assert np.abs(gm - dst).max() < 1e-5


def test_svd_rotate_without_spread_gives_the_ieee_values():
    """every source point the same point: the reference's sqrt(x / 0) is inf, 0 / 0 NaN; without calc_s everything is finite"""
    src = np.tile(np.array([[[0.25, -1.5, 3.0]]], np.float32), (2, 5, 1))
    dst, _, _ = A.point_sets(*A.SPREADLESS_TARGETS)
    dst[1] = dst[1, :1]                                              # the second target has no spread either: 0 / 0
    R, tr, s, moved = _svd(src, dst, (True, True, True))
    assert np.isposinf(s[0]) and np.isnan(s[1]) and np.isfinite(R).all()
    R, tr, s, moved = _svd(src, dst, (True, True, False))
    assert (s == 1).all() and np.isfinite(R).all() and np.isfinite(tr).all() and np.isfinite(moved).all()
    assert np.abs(np.matmul(R, R.transpose(0, 2, 1)) - np.eye(3)).max() < 1e-6


def test_root_turned_prediction(models):
    model, body = models(1025)
    _, pt = A.aux("root turned", body)
    pp, _ = A.root_turned(pt, 491)
    for mode in (-1, -2):
        f64, f32 = A.evaluate_groups(body, pp, pt, (5,), mode), A.evaluate_groups(body, pp, pt, (5,), mode, np.float32)
        assert f64["joint_err"].max() < 1e-6 and f64["mesh_err"].max() < 1e-6
        worst = _check("root turned", mode, _call(model, pp, pt, (5,), mode), f64, f32)
        assert max(worst.values()) <= 1.0, (mode, worst)
    je = _call(model, pp, pt, (5,), -4)[0]
    assert float(je.max()) > 1e-2


def test_mode_4_is_the_difference_of_the_centred_joints(models):
    import motion_metrics_f64 as M
    model, body = models(1023)
    pp, pt = A.aux("mode 4", body)
    jp, jt = (M.fk(body, x, None, M.F64)[1].numpy() for x in (pp, pt))
    ref = np.linalg.norm((jp - jp.mean(axis=1, keepdims=True)) - (jt - jt.mean(axis=1, keepdims=True)), axis=2).mean(axis=0)
    f64, f32 = A.evaluate_groups(body, pp, pt, (7,), -4), A.evaluate_groups(body, pp, pt, (7,), -4, np.float32)
    je = _call(model, pp, pt, (7,), -4)[0].double().numpy()[0]
    assert (A.ratios(je, ref, A.bound(f32["joint_err"][0], f64["joint_err"][0], f64["pos_j"][0])) <= 1.0).all()


def test_groups_of_one_call_are_the_calls_alone_in_any_order(models):
    model, body = models(1025)
    sizes = (1, 33, 7, 65)
    parts = [A.aux(f"alone {i}", body) for i in range(4)]
    assert tuple(p[0].shape[0] for p in parts) == sizes
    alone = [_call(model, p[0], p[1], (N,), -1) for p, N in zip(parts, sizes)]
    for order in ((0, 1, 2, 3), (3, 2, 1, 0), (2, 0, 3, 1)):
        pp, pt = (np.concatenate([parts[i][q] for i in order]) for q in range(2))
        je, me, pf, xf = _call(model, pp, pt, [sizes[i] for i in order], -1)
        at = 0
        for k, i in enumerate(order):
            N = sizes[i]
            assert np.array_equal(bits(je[k]), bits(alone[i][0][0])) and np.array_equal(bits(me[k:k + 1]), bits(alone[i][1])), (order, i)
            assert np.array_equal(bits(pf[at:at + N]), bits(alone[i][2])) and np.array_equal(bits(xf[at:at + N]), bits(alone[i][3])), (order, i)
            at += N
    assert len({float(a[1][0]) for a in alone}) == 4                                         # distinct groups: a mix-up would show


def test_reruns_regrown_buffers_and_no_mesh_are_bitwise(synth_assets):
    """a small call, its rerun, a call that has to grow the scratch, the partial sums and the group table, and the small call again, on
    one fresh context: the small results are the same bits; without the mesh the joint outputs keep theirs and the mesh outputs are NaN"""
    model, body = _small_mesh_model(synth_assets["body"], 1025)
    try:
        a, b = A.aux("small", body), A.aux("large", body)
        a1 = _call(model, *a, (7,), -2)
        a2 = _call(model, *a, (7,), -2)
        b1 = _call(model, *b, (65, 33, 3), -2)
        a3 = _call(model, *a, (7,), -2)
        lean = _call(model, *a, (7,), -2, mesh=False)
    finally:
        model.__del__()
    for x in (a2, a3):
        assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(a1, x))
    assert torch.isfinite(b1[1]).all() and torch.isfinite(a1[1]).all()
    assert lean[1] is None and np.array_equal(bits(lean[0]), bits(a1[0]))
    assert np.array_equal(bits(lean[2][:, 0]), bits(a1[2][:, 0])) and np.array_equal(bits(lean[3][:, 0]), bits(a1[3][:, 0]))
    assert torch.isnan(lean[2][:, 1]).all() and torch.isnan(lean[3][:, 1]).all()


def test_refusals_leave_the_outputs_alone(models, synth_assets):
    from robustcap_amd import _lib
    from robustcap_amd.body import ParametricModel
    model, body = models(1025)
    lib = model._lib
    n = 8
    pp, pt = A.aux("refusals", body)
    pose_p, pose_t = _dev(pp), _dev(pt)
    je, me = torch.full((2, 24), 7.0, device="cuda"), torch.full((2,), 7.0, device="cuda")
    pf, xf = torch.full((n, 2), 7.0, device="cuda"), torch.full((n, 2, 13), 7.0, device="cuda")
    p = _lib.ptr

    def call(ctx=None, a=pose_p, b=pose_t, n_=n, groups=2, sizes=(3, 5), what=7, flags=0, outs=(je, me, pf, xf)):
        arr = (C.c_int64 * max(len(sizes), 1))(*sizes) if sizes is not None else None
        return lib.rc_aligned_metrics(model._ctx if ctx is None else ctx, p(a), p(b), n_, groups, arr, what, flags, *[p(o) for o in outs],
                                      _lib.stream_ptr())
    bad = {"pose_p": dict(a=None), "pose_t": dict(b=None), "group_frames": dict(sizes=None), "no output": dict(outs=(None,) * 4),
           "n<0": dict(n_=-1), "groups<1": dict(groups=0), "entry<1": dict(sizes=(0, 8)), "sum": dict(sizes=(3, 4)), "what=0": dict(what=0),
           "what bits": dict(what=8), "flag": dict(flags=2)}
    for name, kw in bad.items():
        assert call(**kw) == -1, name
        assert b"rc_aligned_metrics" in lib.rc_last_error(model._ctx), name
    assert lib.rc_aligned_metrics(None, p(pose_p), p(pose_t), n, 1, (C.c_int64 * 1)(n), 7, 0, p(je), None, None, None, None) == -1
    assert call(n_=0, groups=0, sizes=()) == 0                                               # the documented no-op
    bare = ParametricModel(body=synth_assets["body"])                                        # a context without a mesh
    assert call(ctx=bare._ctx) == -3 and b"rc_set_mesh" in lib.rc_last_error(bare._ctx)
    R = torch.full((n, 3, 3), 7.0, device="cuda")
    for kw in (dict(m=0), dict(what=8), dict(n_=-1), dict(src=None)):
        a = dict(src=pose_p, n_=n, m=24, what=7)
        a.update(kw)
        assert lib.rc_svd_rotate(p(a["src"]), p(pose_t), a["n_"], a["m"], a["what"], p(R), None, None, None, _lib.stream_ptr()) == -1, kw
    assert lib.rc_svd_rotate(p(pose_p), p(pose_t), n, 24, 7, None, None, None, None, _lib.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in (je, me, pf, xf, R))
    assert call(ctx=bare._ctx, flags=1) == 0 and call() == 0                                  # and the same arguments are accepted
    torch.cuda.synchronize()
    assert not (je == 7.0).any() and not (pf == 7.0).any()
    # rc_motion_metrics keeps refusing a negative align_joint
    out = torch.full((1, 11, 2), 7.0, device="cuda")
    assert lib.rc_motion_metrics(model._ctx, p(pose_p), None, p(pose_t), None, n, 1, (C.c_int64 * 1)(n), 60, -1, 0, 0, p(out), None,
                                 _lib.stream_ptr()) == -1


# ------------------------------------------------------------------------------------------------------ Python layer
@pytest.fixture(scope="module")
def fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "metrics.npz"))
    f = np.load(os.path.join(golden_dir, "aligned", "aligned_metrics.npz"))
    from robustcap_amd import synth
    return f, A.golden_motions(g, synth.make_body(1))


@pytest.mark.parametrize("mode", list(A.MODES))
def test_evaluator_classes_match_the_reference_capture(mode, fixture, synth_assets):
    from robustcap_amd import evaluator as E
    f, motions = fixture
    body = synth_assets["body"]
    pje_ev, mean_ev, mesh_ev = (cls(body=body, align_joint=mode) for cls in (E.PerJointErrorEvaluator, E.MeanPerJointErrorEvaluator, E.MeshErrorEvaluator))
    plain = E.PerJointErrorEvaluator(body=body, align_joint=0)
    for motion, (pp, pt) in motions.items():
        f64, f32 = A.evaluate(body, pp, pt, mode), A.evaluate(body, pp, pt, mode, np.float32)
        bj = A.bound(f32["joint_err"], f64["joint_err"], f64["pos_j"])                       # per entry: against the restatement
        bj_ref = A.bound(f32["joint_err"], f64["joint_err"], f64["pos_j"], block=(0,))       # per block: against the float32 reference
        bm = A.bound(f32["mesh_err"], f64["mesh_err"], f64["pos_v"])
        pje = pje_ev(t(pp), t(pt))
        assert pje.shape == (3, 24) and pje.device.type == "cpu"
        assert np.array_equal(bits(pje[1:]), bits(plain(t(pp), t(pt))[1:]))                  # the alignment does not touch the angle rows
        got = pje[0].double().numpy()
        mesh = float(mesh_ev(t(pp), t(pt)))
        rr = max(A.ratios(got, f[f"pje_m{-mode}_{motion}"][0], bj_ref).max(), A.ratios(mesh, f[f"mesh_m{-mode}_{motion}"], bm).max())
        r64 = max(A.ratios(got, f64["joint_err"], bj).max(), A.ratios(mesh, f64["mesh_err"], bm).max())
        print(f"mode {mode} {motion:5s} |device - reference| / Bound: max {rr:.3f}; |device - restatement| / Bound: max {r64:.3f}")
        assert rr <= 1.0 and r64 <= 1.0, (mode, motion, rr, r64)
        assert torch.equal(mean_ev(t(pp), t(pt)), pje.mean(dim=1))


def test_svd_rotate_matches_the_reference_capture(fixture):
    f, _ = fixture
    for sname, (seed, n, m, mirrored) in A.GOLDEN_POINTS.items():
        src, dst, _ = A.point_sets(seed, n, m, mirrored)
        for calc in A.FLAG_COMBOS:
            got = _svd(src, dst, calc)
            f64, f32 = A.svd_rotate(src, dst, *calc), A.svd_rotate(src, dst, *calc, dtype=np.float32)
            pos = np.abs(src).max() + np.abs(dst).max() + np.abs(f64[1]).max()
            scales = (1.0, pos, np.maximum(1.0, f64[2]), pos)
            for k, out in enumerate(("R", "t", "s", "moved")):
                if calc[0] and not A.R_DEFINED(m) and out != "s":
                    continue
                ref = f[f"svd_{sname}_{A.flag_name(calc)}_{out}"]
                r = A.ratios(got[k], ref, A.bound(f32[k], f64[k], scales[k], block=None if out == "s" else tuple(range(1, got[k].ndim))))
                assert r.max() <= 1.0, (sname, calc, out, r.max())


def test_evaluators_refuse_what_the_reference_refuses(synth_assets):
    from robustcap_amd import evaluator as E
    body = synth_assets["body"]
    eye = torch.eye(3).repeat(2, 24, 1, 1)
    for cls in (E.PerJointErrorEvaluator, E.MeanPerJointErrorEvaluator, E.MeshErrorEvaluator):
        with pytest.raises(RuntimeError, match="Undefined align_joint=-6"):
            cls(body=body, align_joint=-6)(eye, eye)
    with pytest.raises(NotImplementedError, match="align_joint"):
        E.FullMotionEvaluator(body=body, align_joint=-1)


def test_dataset_aligned_metrics_equals_the_rows_alone(synth_assets):
    from robustcap_amd import evaluate as ev
    from robustcap_amd import synth
    ds = synth.make_dataset(5, 2, 40, synth_assets["body"], n_cam=1)
    for k in ("pose", "tran"):                                                               # two rows of unequal lengths
        ds[k][1] = ds[k][1][:23]
    model, _ = _small_mesh_model(synth_assets["body"], 1025)
    res = {}
    for (i, j) in ev.rows_of(ds):
        pt, tt = ev.labels(ds, i, j)
        near = t(synth._rodrigues((0.05 * synth.normal(90 + i, 0, pt.shape[0] * 72)).reshape(-1, 24, 3).astype(np.float64)).astype(np.float32))
        res[(i, j)] = (pt @ near, tt)
    je, me, je_mean, me_mean = ev.aligned_metrics(model, ds, res, align=-1)
    assert list(je) == [(0, 0), (1, 0)] and je_mean.shape == (24,)
    for (i, j), (pose, _) in res.items():
        pt, _ = ev.labels(ds, i, j)
        one_j, one_m = model.aligned_metrics(pose, pt, align=-1)
        assert np.array_equal(bits(one_j[0].cpu()), bits(je[(i, j)])), (i, j)
        assert float(one_m[0]) == me[(i, j)], (i, j)
    assert torch.isfinite(je_mean).all() and np.isfinite(me_mean)
