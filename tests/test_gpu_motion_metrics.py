"""rc_motion_metrics (csrc/rc_motion.hip): art.FullMotionEvaluator per motion of a concatenated batch, on the device.

  values    every finite entry of out [G,11,2] and per_joint [G,4,24] within Bound = 8 |float32 transcription - float64 restatement| +
            1e-7 scale of the restatement (tests/motion_metrics_f64.py), NaNs exactly where it has them. Small synthetic meshes with V =
            1, 1023, 1024, 1025 (the 1024-vertex slab edge) and the full 6890; group lengths 1, 3, 4, 15 / 16 / 17 and 31 / 32 / 33 (the
            32-frame block of the sweeps); fps = 5 with 5 and 6 frames; masks none / one joint / all 24; align_joint 0 and 5; tran NULL on
            one side or both. RC_MOTION_RATIOS_OUT=path appends the largest ratio per row (profiles/motion_metrics_ratios.txt).
            At fps = 60, the reference's default, where the window of row 6 starts two blocks ahead: 61 and 62 frames (one and two te
            rows), 64 / 65 / 67 (a last block of 32 / 1 / 3 frames with 29 / 0 / 0 jerk rows), 96 / 97 / 131 (three, four and five blocks
            merged; 131: 71 te rows in three blocks and two blocks without any); 125 and 93 with align_joint 5, all joints masked and
            tran_p NULL (65 te rows: a third te block of one row). fps = 32 and 33 on 33, 34, 65, 66 frames: the window exactly one
            block ahead and one frame past that. 75 groups in one call (70 of 1-3 frames; 67, 33, 97, 64, 131 at positions 0, 17, 40,
            58, 74; 106 blocks) for the bisection over the block table. 67 frames at fps 60 on the full mesh: the vertex merge over
            three blocks on seven slabs. (tests/test_motion_metrics_cpu.py: a merge that drops the running count, or a window that
            wraps inside a block, moves nothing at the sizes of the first paragraph and hundreds of Bounds at these.)
  bitwise   groups of (1, 4, 7, 61) frames at fps 5 and of (67, 1, 131, 96) at fps 60 in one call = the four calls alone, in any order;
            tran NULL = zeros; reruns; RC_MOTION_NO_MESH changes row 1 only; a call that regrows the scratch, the partial sums and the
            group table between two small calls leaves their bits alone and is itself the bits of a fresh context.
  identical exact zeros in je, ve, lae, gae, te, tre; jkp == jkt bitwise.
  bad input every refusal returns its code and leaves sentinel-filled outputs alone; no mesh: RC_ERR_STATE.
  python    the evaluator classes and evaluate.motion_metrics against the captured fixture (tests/golden/motion) at the same bound;
            the 131-frame `long` capture gives the reference's own finite te at fps 60. evaluate.motion_metrics on a two-row dataset of
            unequal lengths = the per-row calls, bitwise; at its default fps on rows of 131 and 70 frames = the per-row calls at fps=60,
            within the Bound of the restatement, te finite.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import motion_metrics_f64 as M

pytestmark = pytest.mark.gpu
t = torch.from_numpy
WORST = {}


def _note(row, ratio, what):
    if row not in WORST or ratio > WORST[row][0]:
        WORST[row] = (float(ratio), what)


def _small_mesh_model(full_body, V):
    """a ParametricModel on the shared body whose mesh has V vertices (the joints depend on the seed alone; the 33 landmarks the
    constructor takes from the mesh need the full one), and the body dict the restatement reads"""
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
    """model_of(V) -> (model, body) with a V-vertex mesh"""
    cache = {}

    def model_of(V):
        if V not in cache:
            cache[V] = _small_mesh_model(synth_assets["body"], V)
        return cache[V]
    return model_of


def _batch(sizes, seed0, same=False):
    parts = [M.motion_pair(seed0 + i, N, same=same) for i, N in enumerate(sizes)]
    return [np.concatenate([p[q] for p in parts]) for q in range(4)], parts


def _dev(a):
    return None if a is None else t(np.ascontiguousarray(a)).cuda()


def _mask_bits(mask):
    return 0 if mask is None else sum(1 << j for j in mask)


def _call(model, pp, pt, tp, tt, sizes, fps=60, align=0, mask=None, mesh=True):
    out, pj = model.motion_metrics(_dev(pp), _dev(pt), _dev(tp), _dev(tt), group_frames=sizes, fps=fps, align_joint=align,
                                   joint_mask=_mask_bits(mask), mesh=mesh)
    return out.cpu(), pj.cpu()


def _many_groups():
    """75 groups, 106 blocks: 70 of 1, 2, 3, 1, ... frames and, at positions 0, 17, 40, 58 and 74, groups of 67, 33, 97, 64 and 131: the
    bisection over the block table has to find a block in the middle of a long group and a one-block group between long ones"""
    long_ones, short = {0: 67, 17: 33, 40: 97, 58: 64, 74: 131}, iter(range(70))
    sizes = tuple(long_ones[k] if k in long_ones else 1 + next(short) % 3 for k in range(75))
    assert len(sizes) == 75 and sum(1 for s in sizes if s <= 3) == 70
    return sizes


MANY_GROUPS = _many_groups()
CASES = [
    # name, V, group lengths, fps, mask, align, tran_p given, tran_t given
    ("blocks V=1025", 1025, (1, 3, 4, 31, 32, 33), 60, None, 0, True, True),
    ("fps5 one joint V=1023 align5", 1023, (5, 6), 5, [7], 5, True, True),
    ("all joints V=1024 tran_p NULL", 1024, (15, 16, 17), 5, list(range(24)), 0, False, True),
    ("V=1 no tran", 1, (4, 33), 5, None, 0, False, False),
    ("one joint V=1025 tran_t NULL", 1025, (17,), 5, [0], 0, True, False),
    ("full mesh V=6890", 6890, (33,), 5, [1, 2, 16, 17, 20], 5, True, True),
    # fps 60, the reference's default: the window of row 6 starts two 32-frame blocks ahead of the row's own block. 61 | 62 frames: one |
    # two te rows; 64 | 65 | 67: a last block of 32 | 1 | 3 frames with 29 | 0 | 0 jerk rows; 96 | 97 | 131: three, four and five blocks;
    # 131: 71 te rows in three blocks, and two blocks without any
    ("fps60 windows V=1025", 1025, (61, 62, 64, 65, 67, 96, 97, 131), 60, [7], 0, True, True),
    ("fps60 align5 tran_p NULL V=1024", 1024, (125, 93), 60, list(range(24)), 5, False, True),       # 125: 65 te rows, a third te block of one
    ("fps32 V=1", 1, (33, 34, 65, 66), 32, None, 0, True, True),                                    # the window exactly one block ahead
    ("fps33 V=1", 1, (33, 34, 65, 66), 33, None, 0, True, True),                                    # and one frame past that
    ("many groups V=1023", 1023, MANY_GROUPS, 5, [0], 0, True, True),
    ("full mesh three blocks V=6890", 6890, (67,), 60, None, 0, True, True),                        # the vertex merge over three blocks, 7 slabs
]
_RESTATED = {}


def _restated(case, body, arrs):
    """the float64 restatement and the float32 transcription of a case, computed once per module (the full mesh of 67 frames is a
    [67, 6890, 3, 4] tensor per motion and precision)"""
    name, V, sizes, fps, mask, align, has_p, has_t = case
    if name not in _RESTATED:
        f64, pj64, scale = M.evaluate_groups(body, *arrs, sizes, fps, align, mask)
        f32, pj32, _ = M.evaluate_groups(body, *arrs, sizes, fps, align, mask, dtype=M.F32)
        _RESTATED[name] = (f64, pj64, scale, f32, pj32)
    return _RESTATED[name]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_values_within_the_bound_and_nans_in_place(case, models):
    name, V, sizes, fps, mask, align, has_p, has_t = case
    model, body = models(V)
    (pp, pt, tp, tt), _ = _batch(sizes, 200 + V % 97)
    tp, tt = (tp if has_p else None), (tt if has_t else None)
    f64, pj64, scale, f32, pj32 = _restated(case, body, (pp, pt, tp, tt))
    out, pj = _call(model, pp, pt, tp, tt, sizes, fps, align, mask)
    r = M.ratios(out.double().numpy(), f64, M.bound(f32, f64, scale))                       # asserts the NaN placement
    sj = M.per_joint_scale(scale)
    with np.errstate(invalid="ignore"):
        bj = M.K * np.abs(pj32 - pj64) + M.REL * sj[..., None]
    rj = M.ratios(pj.double().numpy(), pj64, bj)
    for k, row in enumerate(M.ROWS):
        print(f"{name:32s} {row:5s} error / Bound: mean {r[:, k, 0].max():.3f} std {r[:, k, 1].max():.3f}")
        _note(row, r[:, k].max(), name)
    for k, row in enumerate(("je", "lae", "gae", "tre")):
        _note("per_joint " + row, rj[:, k].max(), name)
    assert (r <= 1.0).all(), (name, r.max())
    assert (rj <= 1.0).all(), (name, rj.max())
    for g, N in enumerate(sizes):                                                            # torch's NaNs of the degenerate sets
        assert bool(torch.isnan(out[g, 0, 1])) == (N == 1)
        assert bool(torch.isnan(out[g, 4, 0])) == (N <= 3) and bool(torch.isnan(out[g, 4, 1])) == (N <= 4)
        assert bool(torch.isnan(out[g, 6, 0])) == (N <= fps) and bool(torch.isnan(out[g, 6, 1])) == (N <= fps + 1)
        if mask is None:
            assert (out[g, 7:10, 0] == 0).all() and torch.isnan(out[g, 7:10, 1]).all()


def test_groups_of_one_call_are_the_calls_alone_in_any_order(models):
    model, _ = models(1025)
    sizes = (1, 4, 7, 61)
    _, parts = _batch(sizes, 300)
    alone = [_call(model, *p, [N], fps=5, mask=[3, 9]) for p, N in zip(parts, sizes)]
    for order in ((0, 1, 2, 3), (3, 2, 1, 0), (2, 0, 3, 1), (1, 3, 0, 2)):
        arrs = [np.concatenate([parts[i][q] for i in order]) for q in range(4)]
        out, pj = _call(model, *arrs, [sizes[i] for i in order], fps=5, mask=[3, 9])
        for k, i in enumerate(order):
            assert np.array_equal(out[k].numpy().view(np.int32), alone[i][0][0].numpy().view(np.int32)), (order, i)
            assert np.array_equal(pj[k].numpy().view(np.int32), alone[i][1][0].numpy().view(np.int32)), (order, i)
    assert len({float(a[0][0, 0, 0]) for a in alone}) == 4                                   # distinct groups: a mix-up would show


def test_long_groups_at_fps60_are_the_calls_alone_in_any_order(models):
    """groups of three to five blocks with te rows of their own (67: 7, 131: 71, 96: 36) and a group of one frame between them"""
    model, _ = models(1025)
    sizes = (67, 1, 131, 96)
    _, parts = _batch(sizes, 330)
    bits = lambda x: x.numpy().view(np.int32)
    alone = [_call(model, *p, [N], fps=60, mask=[3, 9]) for p, N in zip(parts, sizes)]
    for order in ((0, 1, 2, 3), (3, 2, 1, 0), (2, 0, 3, 1), (1, 3, 0, 2)):
        arrs = [np.concatenate([parts[i][q] for i in order]) for q in range(4)]
        out, pj = _call(model, *arrs, [sizes[i] for i in order], fps=60, mask=[3, 9])
        for k, i in enumerate(order):
            assert np.array_equal(bits(out[k]), bits(alone[i][0][0])), (order, i)
            assert np.array_equal(bits(pj[k]), bits(alone[i][1][0])), (order, i)
    assert len({float(a[0][0, 0, 0]) for a in alone}) == 4                                   # distinct groups: a mix-up would show
    assert all(bool(torch.isfinite(a[0][0, 6]).all()) == (N > 61) for a, N in zip(alone, sizes))


def test_regrown_buffers_give_the_same_bits(synth_assets):
    """a small call, a call that has to grow the scratch, the partial sums and the group table, and the small call again, on one fresh
    context: the small results are the same bits, and the large one is that of a second fresh context that sees it alone"""
    sizes_a, sizes_b = (7,), (131, 67, 3)
    (a, _), (b, _) = _batch(sizes_a, 340), _batch(sizes_b, 341)
    bits = lambda x: x.numpy().view(np.int32)
    model, _ = _small_mesh_model(synth_assets["body"], 1025)
    other, _ = _small_mesh_model(synth_assets["body"], 1025)
    try:
        a1 = _call(model, *a, sizes_a, fps=60, mask=[2])
        b1 = _call(model, *b, sizes_b, fps=60, mask=[2])
        a2 = _call(model, *a, sizes_a, fps=60, mask=[2])
        b2 = _call(other, *b, sizes_b, fps=60, mask=[2])
    finally:
        model.__del__(), other.__del__()                                                     # rc_destroy now, not at collection
    assert np.array_equal(bits(a1[0]), bits(a2[0])) and np.array_equal(bits(a1[1]), bits(a2[1]))
    assert np.array_equal(bits(b1[0]), bits(b2[0])) and np.array_equal(bits(b1[1]), bits(b2[1]))
    assert torch.isfinite(b1[0][:2, 6]).all() and torch.isnan(b1[0][2, 6]).all() and torch.isnan(a1[0][0, 6]).all()
    assert torch.isfinite(a1[0][0, [0, 1, 2, 3, 4, 5, 7, 8, 9, 10]]).all()


def test_null_translation_reruns_and_no_mesh_are_bitwise(models):
    model, _ = models(1025)
    sizes = (7, 33)
    (pp, pt, tp, tt), _ = _batch(sizes, 310)
    bits = lambda x: x.numpy().view(np.int32)
    zero = np.zeros_like(tp)
    base = _call(model, pp, pt, tp, tt, sizes, fps=5, mask=[2])
    again = _call(model, pp, pt, tp, tt, sizes, fps=5, mask=[2])
    assert np.array_equal(bits(base[0]), bits(again[0])) and np.array_equal(bits(base[1]), bits(again[1]))
    for a, b in (((None, tt), (zero, tt)), ((tp, None), (tp, zero)), ((None, None), (zero, zero))):
        x, y = _call(model, pp, pt, *a, sizes, fps=5), _call(model, pp, pt, *b, sizes, fps=5)
        assert np.array_equal(bits(x[0]), bits(y[0])) and np.array_equal(bits(x[1]), bits(y[1]))
    lean = _call(model, pp, pt, tp, tt, sizes, fps=5, mask=[2], mesh=False)
    assert torch.isnan(lean[0][:, 1]).all() and torch.isfinite(base[0][:, 1]).all()
    keep = [0] + list(range(2, 11))
    assert np.array_equal(bits(lean[0][:, keep]), bits(base[0][:, keep])) and np.array_equal(bits(lean[1]), bits(base[1]))


def test_identical_motions_give_exact_zeros(models):
    model, _ = models(1025)
    sizes = (9, 33)
    (pp, pt, tp, tt), _ = _batch(sizes, 320, same=True)
    for trans in ((tp, tt), (None, None)):
        out, pj = _call(model, pp, pt, *trans, sizes, fps=5, mask=[4, 5])
        for row in (0, 1, 2, 3, 6, 7, 8, 9, 10):                                             # je, ve, lae, gae, te, the masked rows, tre
            assert (out[:, row] == 0).all(), (row, out[:, row])
        assert (pj == 0).all()
        assert np.array_equal(out[:, 4].numpy().view(np.int32), out[:, 5].numpy().view(np.int32)) and (out[:, 4] > 0).all()


def test_bad_input_returns_its_code_and_writes_nothing(models, synth_assets):
    from robustcap_amd import _lib
    from robustcap_amd.body import ParametricModel
    model, body = models(1025)
    lib = model._lib
    n = 8
    pose = torch.eye(3, device="cuda").repeat(n, 24, 1, 1).contiguous()
    tran = torch.zeros(n, 3, device="cuda")
    out = torch.full((2, 11, 2), 7.0, device="cuda")
    pj = torch.full((2, 4, 24), 7.0, device="cuda")
    p = _lib.ptr

    def call(ctx=None, pp=pose, pt=pose, n_=n, groups=2, sizes=(3, 5), fps=60, align=0, mask=0, flags=0, o=out):
        arr = (C.c_int64 * max(len(sizes), 1))(*sizes) if sizes is not None else None
        return lib.rc_motion_metrics(model._ctx if ctx is None else ctx, p(pp), p(tran), p(pt), p(tran), n_, groups, arr, fps, align, mask,
                                     flags, p(o), p(pj), _lib.stream_ptr())
    bad = {"pose_p": dict(pp=None), "pose_t": dict(pt=None), "out": dict(o=None), "group_frames": dict(sizes=None), "n<0": dict(n_=-1),
           "groups<1": dict(groups=0), "entry<1": dict(sizes=(0, 8)), "sum": dict(sizes=(3, 4)), "fps": dict(fps=0), "align-": dict(align=-1),
           "align+": dict(align=24), "mask": dict(mask=1 << 24), "flag": dict(flags=2)}
    for name, kw in bad.items():
        assert call(**kw) == -1, name
        assert b"rc_motion_metrics" in lib.rc_last_error(model._ctx), name
    assert lib.rc_motion_metrics(None, p(pose), None, p(pose), None, n, 1, (C.c_int64 * 1)(n), 60, 0, 0, 0, p(out), None, None) == -1
    assert call(n_=0, groups=0, sizes=()) == 0                                               # the documented no-op
    bare = ParametricModel(body=synth_assets["body"])                                        # a context without a mesh
    assert call(ctx=bare._ctx) == -3 and b"rc_set_mesh" in lib.rc_last_error(bare._ctx)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (pj == 7.0).all()
    assert call(ctx=bare._ctx, flags=1) == 0 and call() == 0                                  # and the same arguments are accepted
    torch.cuda.synchronize()
    assert not (out == 7.0).any()


# ------------------------------------------------------------------------------------------------------ Python layer
@pytest.fixture(scope="module")
def fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "metrics.npz"))
    f = np.load(os.path.join(golden_dir, "motion", "motion_metrics.npz"))
    gt = g["pose_gt"]
    tp, tt = f["tran_p"], f["tran_t"]
    arrs, digests = M.golden_long()                                                          # 131 frames, regenerated from the seed
    assert digests == json.load(open(os.path.join(golden_dir, "motion", "meta.json")))["long_inputs_sha256"]
    return f, {"near": (g["pose_near"], gt, tp, tt), "far": (g["pose_far"], gt, tp, tt), "same": (gt, gt, tt, tt), "long": arrs}


@pytest.mark.parametrize("setting", list(M.GOLDEN_SETTINGS))
def test_evaluator_classes_match_the_reference_capture(setting, fixture, synth_assets):
    from robustcap_amd import evaluator as E
    from robustcap_amd import body as B
    f, motions = fixture
    body = synth_assets["body"]
    fps, mask, align = M.GOLDEN_SETTINGS[setting]
    ev = E.FullMotionEvaluator(body=body, align_joint=align, fps=fps, joint_mask=mask)
    for motion, (pp, pt, tp, tt) in motions.items():
        if motion == "long" and setting not in M.GOLDEN_LONG_SETTINGS:                       # captured at fps 60 only: the finite te there
            continue
        f64, pj64, scale = M.evaluate(body, pp, pt, tp, tt, fps, align, mask)
        f32, pj32, _ = M.evaluate(body, pp, pt, tp, tt, fps, align, mask, dtype=M.F32)
        bnd = M.bound(f32, f64, scale)
        ref = f[f"out_{setting}_{motion}"]
        out = ev(t(pp), t(pt), tran_p=t(tp), tran_t=t(tt))
        assert out.shape == (11, 2) and out.device.type == "cpu"
        got = out.double().numpy()
        assert (M.ratios(got, f64, bnd) <= 1.0).all(), (setting, motion)
        rr = M.ratios(got, ref, bnd)                                                             # the reference's own numbers, same Bound
        print(f"{setting:10s} {motion:5s} |device - reference| / Bound: max {rr.max():.3f}")
        assert (rr <= 1.0).all(), (setting, motion, rr)
        assert bool(np.isfinite(got[6]).all()) == (motion == "long" or fps == 5) and np.isnan(got[6]).all() == (pp.shape[0] <= fps)
        if setting == "fps60" and motion == "near":
            # the column views, and the other representations through the body.* conversions
            pje = E.PerJointErrorEvaluator(body=body, align_joint=align)(t(pp), t(pt))
            sj = M.per_joint_scale(scale)
            assert pje.shape == (3, 24)
            assert (M.ratios(pje.double().numpy(), pj64[:3], M.K * np.abs(pj32 - pj64)[:3] + M.REL * sj[:3, None]) <= 1.0).all()
            assert torch.equal(E.MeanPerJointErrorEvaluator(body=body, align_joint=align)(t(pp), t(pt)), pje.mean(dim=1))
            mesh = E.MeshErrorEvaluator(body=body, align_joint=align)(t(pp), t(pt))
            f64z = M.evaluate(body, pp, pt, None, None, fps, align, mask)
            f32z = M.evaluate(body, pp, pt, None, None, fps, align, mask, dtype=M.F32)[0]
            assert abs(float(mesh) - f64z[0][1, 0]) <= M.bound(f32z, f64z[0], f64z[2])[1, 0]
            r6p, r6t = B.rotation_matrix_to_r6d(t(pp).reshape(-1, 3, 3)).view(-1, 144), B.rotation_matrix_to_r6d(t(pt).reshape(-1, 3, 3)).view(-1, 144)
            via = E.FullMotionEvaluator(body=body, rep=E.RotationRepresentation.R6D, fps=fps)(r6p, r6t, tran_p=t(tp), tran_t=t(tt))
            Rp, Rt = B.r6d_to_rotation_matrix(r6p.reshape(-1, 6)).view(-1, 24, 3, 3), B.r6d_to_rotation_matrix(r6t.reshape(-1, 6)).view(-1, 24, 3, 3)
            assert torch.equal(via.view(torch.int32), ev(Rp, Rt, tran_p=t(tp), tran_t=t(tt)).view(torch.int32))
            aap, aat = B.rotation_matrix_to_axis_angle(t(pp).reshape(-1, 3, 3)).view(-1, 72), B.rotation_matrix_to_axis_angle(t(pt).reshape(-1, 3, 3)).view(-1, 72)
            via = E.FullMotionEvaluator(body=body, rep=E.RotationRepresentation.AXIS_ANGLE, fps=fps)(aap, aat, tran_p=t(tp), tran_t=t(tt))
            Rp, Rt = B.axis_angle_to_rotation_matrix(aap.reshape(-1, 3)).view(-1, 24, 3, 3), B.axis_angle_to_rotation_matrix(aat.reshape(-1, 3)).view(-1, 24, 3, 3)
            assert torch.equal(via.view(torch.int32), ev(Rp, Rt, tran_p=t(tp), tran_t=t(tt)).view(torch.int32))


def test_evaluator_refuses_what_is_not_implemented(synth_assets):
    from robustcap_amd import evaluator as E
    body = synth_assets["body"]
    for kw, word in ((dict(rep=E.RotationRepresentation.QUATERNION), "rep"), (dict(use_pose_blendshape=True), "use_pose_blendshape"),
                     (dict(align_joint=-1), "align_joint")):
        with pytest.raises(NotImplementedError, match=word):
            E.FullMotionEvaluator(body=body, **kw)
    ev = E.FullMotionEvaluator(body=body)
    eye = torch.eye(3).repeat(2, 24, 1, 1)
    with pytest.raises(NotImplementedError, match="shape"):
        ev(eye, eye, shape_p=torch.zeros(10), shape_t=torch.ones(10))


def test_dataset_motion_metrics_matches_the_reference_capture(fixture, synth_assets):
    """evaluate.motion_metrics on a dataset whose three sequences are the fixture's truth (one camera at the identity) and whose results are
    its near / far / same predictions: every row within the Bound of the captured fps=5 result. The labels are the truth turned into axis
    angles and back (the dataset's layout), which moves a rotation by a few 2^-24: inside the 1e-7 scale term."""
    from robustcap_amd import body as B
    from robustcap_amd import evaluate as ev
    from robustcap_amd.body import ParametricModel
    f, motions = fixture
    body = synth_assets["body"]
    fps, mask, align = M.GOLDEN_SETTINGS["fps5_mask"]
    gt, tt = motions["near"][1], motions["near"][3]
    aa = B.rotation_matrix_to_axis_angle(t(gt).reshape(-1, 3, 3)).view(-1, 72).cpu().numpy()
    names = list(M.GOLDEN_MOTIONS)                                                           # the three 24-frame motions
    ds = {"pose": [aa] * 3, "tran": [tt] * 3, "cam_T": [[np.eye(4, dtype=np.float32)]] * 3, "cam_K": [[np.eye(3, dtype=np.float32)]] * 3}
    res = {(i, 0): (t(motions[n][0]), t(motions[n][2])) for i, n in enumerate(names)}
    per_row, mean = ev.motion_metrics(ParametricModel(body=body), ds, res, fps=fps, joint_mask=mask)
    for i, n in enumerate(names):
        pp, pt, tp, tt_ = motions[n]
        f64, _, scale = M.evaluate(body, pp, pt, tp, tt_, fps, align, mask)
        f32 = M.evaluate(body, pp, pt, tp, tt_, fps, align, mask, dtype=M.F32)[0]
        rr = M.ratios(per_row[(i, 0)].double().numpy(), f[f"out_fps5_mask_{n}"], M.bound(f32, f64, scale))
        print(f"evaluate.motion_metrics {n:5s} |device - reference| / Bound: max {rr.max():.3f}")
        assert (rr <= 1.0).all(), (n, rr)
    assert torch.equal(mean.view(torch.int32), torch.stack([per_row[(i, 0)] for i in range(3)]).mean(dim=0).view(torch.int32))


def test_dataset_motion_metrics_equals_the_rows_alone(synth_assets):
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
        res[(i, j)] = (pt @ near, tt + 0.01)
    per_row, mean = ev.motion_metrics(model, ds, res, fps=5, joint_mask=[1, 2])
    assert list(per_row) == [(0, 0), (1, 0)] and mean.shape == (11, 2)
    for (i, j), (pose, tran) in res.items():
        pt, tt = ev.labels(ds, i, j)
        one, _ = model.motion_metrics(pose, pt, tran, tt, fps=5, joint_mask=0b110)
        assert np.array_equal(one[0].cpu().numpy().view(np.int32), per_row[(i, j)].numpy().view(np.int32)), (i, j)
    assert torch.isfinite(mean).all()


def test_dataset_motion_metrics_default_fps_on_long_rows(models, synth_assets):
    """evaluate.motion_metrics without an fps argument is the reference's fps = 60: rows of 131 and 70 frames (71 and 10 one-second
    windows, five and three blocks) are bitwise the per-row calls at fps=60 and within the Bound of the restatement at fps=60"""
    from robustcap_amd import evaluate as ev
    from robustcap_amd import synth
    ds = synth.make_dataset(6, 2, 131, synth_assets["body"], n_cam=1)
    for k in ("pose", "tran"):
        ds[k][1] = ds[k][1][:70]
    model, body = models(1025)
    res = {}
    for (i, j) in ev.rows_of(ds):
        pt, tt = ev.labels(ds, i, j)
        T = pt.shape[0]
        near = t(synth._rodrigues((0.05 * synth.normal(95 + i, 0, T * 72)).reshape(-1, 24, 3).astype(np.float64)).astype(np.float32))
        res[(i, j)] = (pt @ near, tt + t((0.02 * synth.normal(95 + i, 1, T * 3)).reshape(T, 3).astype(np.float32)))
    per_row, mean = ev.motion_metrics(model, ds, res)
    assert list(per_row) == [(0, 0), (1, 0)] and mean.shape == (11, 2)
    assert [res[r][0].shape[0] for r in per_row] == [131, 70]
    for (i, j), (pose, tran) in res.items():
        pt, tt = ev.labels(ds, i, j)
        one, _ = model.motion_metrics(pose, pt, tran, tt, fps=60)
        assert np.array_equal(one[0].cpu().numpy().view(np.int32), per_row[(i, j)].numpy().view(np.int32)), (i, j)
        arrs = [x.cpu().numpy() for x in (pose, pt, tran, tt)]
        f64, _, scale = M.evaluate(body, *arrs, fps=60)
        f32 = M.evaluate(body, *arrs, fps=60, dtype=M.F32)[0]
        rr = M.ratios(per_row[(i, j)].double().numpy(), f64, M.bound(f32, f64, scale))       # asserts the NaN placement
        print(f"evaluate.motion_metrics row {i} ({pose.shape[0]} frames) error / Bound: max {rr.max():.3f}, te {rr[6, 0]:.3f} {rr[6, 1]:.3f}")
        assert (rr <= 1.0).all(), (i, rr)
        assert torch.isfinite(per_row[(i, j)][6]).all() and (per_row[(i, j)][6] > 0).all()
    assert torch.equal(mean.view(torch.int32), torch.stack([per_row[(i, 0)] for i in range(2)]).mean(dim=0).view(torch.int32))


def test_zz_report_worst_ratios():
    """The largest error / Bound per row over the value tests above (pytest -s shows it)."""
    if not WORST:
        print("no value test of this file ran before the report")
        return
    lines = [f"device (rc_motion.hip), K = {M.K:g}, + {M.REL:g} scale: worst error / Bound per row"]
    lines += [f"  {row:16s} {v:.3f}  ({what})" for row, (v, what) in sorted(WORST.items())]
    for ln in lines:
        print(ln)
    path = os.environ.get("RC_MOTION_RATIOS_OUT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")
    assert max(v for v, _ in WORST.values()) <= 1.0
