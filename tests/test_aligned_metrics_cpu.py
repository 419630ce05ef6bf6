"""The restatement behind tests/test_gpu_aligned_metrics.py (tests/aligned_metrics_f64.py), checked without a GPU.

  fold        on meshes of V = 5, 1025 and 6890 the folded sums (C, m -> sum p t^T, sum p, sum t, sum |p|^2, sum |t|^2) equal the vertex-wise
              sums to 1e-12 relative.
  mutations   every named mistake moves its named output by more than the per-entry Bound on an input the GPU tests use (the far case: the
              two reflection mistakes need a frame with an improper fit); the reflection mistakes also move `moved` of the mirrored sets.
  fixture     the restatement is within the Bound of the captured reference (tests/golden/aligned, tools/capture_aligned_metrics.py) --
              the one comparison with a float32 LAPACK on the other side, and the one place the transcription's error is taken per block
              of a fit's entries (aligned_metrics_f64.bound) --, the fixture's sha256 is meta.json's, and its angle rows are the rows of
              align_joint=0 bit for bit.
  condition   every frame of every pose input and every point set of four or more points used here and on the GPU has s3 >= 1e-3 s1 for its
              centred H, joints and mesh alike; nothing is filtered, an input that failed got another seed. (Three points are coplanar
              once centred -- rank 2 --: with calc_R only s and the orthogonality of R are defined there, and only those are compared.)
  reflection  the mirrored point sets and at least one frame of each far pose case -- joints and mesh -- have an improper V U^T: the row-flip
              branch runs.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import aligned_metrics_f64 as A

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def bodies():
    from robustcap_amd import synth
    cache = {}

    def body_of(V):
        if V not in cache:
            cache[V] = synth.make_body(1, num_vertex=V)
        return cache[V]
    return body_of


@pytest.mark.parametrize("V", [5, 1025, 6890])
def test_fold_equals_the_vertex_sums(V, bodies):
    body = bodies(V)
    pp, pt = A.aux(f"fold V={V}", body)
    C, m = A.fold_constants(body)
    Ap, At = A.transforms(body, pp), A.transforms(body, pt)
    for f in range(2):
        for got, ref in zip(A.fold_sums(C, m, Ap[f], At[f]), A.vertex_sums(body, Ap[f], At[f])):
            got, ref = np.asarray(got), np.asarray(ref)
            assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (V, f, got, ref)
    # the fold is symmetric in (j, k) and each C[j,k] is a symmetric 4x4 (the seeded body gives every vertex one random fourth joint, so all
    # 300 pairs j <= k occur here; SMPL's weights leave most of them empty)
    assert np.array_equal(C, C.transpose(1, 0, 2, 3)) and np.abs(C - C.transpose(0, 1, 3, 2)).max() <= 1e-15 * np.abs(C).max()


def _far_case():
    return next(c for c in A.CASES if c[0] == "slab edge V=1024 far")


@pytest.mark.parametrize("mut", sorted(A.MUTATIONS))
def test_every_mutation_moves_its_output(mut, bodies):
    name, V, sizes, seed, far = _far_case()
    body = bodies(V)
    pp, pt = A.pose_batch(body, sizes, seed, far)
    mode, outn = A.MUTATIONS[mut]
    f64 = A.evaluate_groups(body, pp, pt, sizes, mode)
    f32 = A.evaluate_groups(body, pp, pt, sizes, mode, np.float32)
    bad = A.evaluate_groups(body, pp, pt, sizes, mode, mut=mut)
    scale = f64["pos_j"][:, None] if outn == "joint_err" else f64["pos_v"]
    moved = np.abs(bad[outn] - f64[outn]) / A.bound(f32[outn], f64[outn], scale)
    print(f"{mut:20s} mode {mode} {outn}: {moved.max():.1f} Bounds")
    assert moved.max() > 1.0, (mut, moved.max())


@pytest.mark.parametrize("mut", A.REFLECTION_MUTATIONS + ("R_transposed", "trace_scale"))
def test_point_set_mutations_move_the_moved_points(mut):
    m, n, seed, mirrored = next(c for c in A.SVD_CASES if c[3])
    src, dst, _ = A.point_sets(seed, n, m, mirrored)
    f64 = A.svd_rotate(src, dst, True, True, True)
    f32 = A.svd_rotate(src, dst, True, True, True, np.float32)
    bad = A.svd_rotate(src, dst, True, True, True, mut=mut)
    scale = np.abs(src).max() + np.abs(dst).max() + np.abs(f64[1]).max()
    assert (np.abs(bad[3] - f64[3]) / A.bound(f32[3], f64[3], scale)).max() > 1.0


def test_fixture_digest_and_angle_rows():
    path = os.path.join(GOLD, "aligned", "aligned_metrics.npz")
    with open(os.path.join(GOLD, "aligned", "meta.json")) as f:
        meta = json.load(f)
    with open(path, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == meta["sha256"]["aligned_metrics.npz"]
    g = np.load(path)
    for mname in A.GOLDEN_MOTIONS:
        for mode in A.MODES:
            assert np.array_equal(g[f"pje_m{-mode}_{mname}"][1:], g[f"pje_0_{mname}"][1:])     # "the alignment does not affect the rotation error"


def test_restatement_is_within_the_bound_of_the_captured_reference(bodies):
    g = np.load(os.path.join(GOLD, "aligned", "aligned_metrics.npz"))
    metrics = np.load(os.path.join(GOLD, "metrics.npz"))
    body = bodies(6890)
    worst = 0.0
    for mname, (pp, pt) in A.golden_motions(metrics, body).items():
        for mode in A.MODES:
            f64, f32 = A.evaluate(body, pp, pt, mode), A.evaluate(body, pp, pt, mode, np.float32)
            rj = A.ratios(g[f"pje_m{-mode}_{mname}"][0], f64["joint_err"], A.bound(f32["joint_err"], f64["joint_err"], f64["pos_j"], block=(0,)))
            rm = A.ratios(g[f"mesh_m{-mode}_{mname}"], f64["mesh_err"], A.bound(f32["mesh_err"], f64["mesh_err"], f64["pos_v"]))
            worst = max(worst, rj.max(), rm.max())
            assert rj.max() <= 1.0 and rm.max() <= 1.0, (mname, mode, rj.max(), rm.max())
    for sname, (seed, n, m, mirrored) in A.GOLDEN_POINTS.items():
        src, dst, _ = A.point_sets(seed, n, m, mirrored)
        for calc in A.FLAG_COMBOS:
            f64, f32 = A.svd_rotate(src, dst, *calc), A.svd_rotate(src, dst, *calc, dtype=np.float32)
            pos = np.abs(src).max() + np.abs(dst).max() + np.abs(f64[1]).max()
            got = [g[f"svd_{sname}_{A.flag_name(calc)}_{k}"] for k in ("R", "t", "s", "moved")]
            scales = (1.0, pos, np.maximum(1.0, f64[2]), pos)
            for k in range(4):
                if calc[0] and not A.R_DEFINED(m) and k != 2:
                    continue                                     # three points: rank 2, only s is defined (and R orthogonal, below)
                r = A.ratios(got[k], f64[k], A.bound(f32[k], f64[k], scales[k], block=None if k == 2 else tuple(range(1, got[k].ndim))))
                worst = max(worst, r.max())
                assert r.max() <= 1.0, (sname, calc, k, r.max())
            assert np.abs(np.matmul(got[0], got[0].transpose(0, 2, 1)) - np.eye(3)).max() < 1e-5
    print(f"captured reference against the restatement: largest error / Bound {worst:.3f}")


def test_every_input_is_well_conditioned_and_the_reflection_runs(bodies):
    metrics = np.load(os.path.join(GOLD, "metrics.npz"))
    improper = {}
    for name, V, sizes, seed, far in [c for c in A.CASES] + [(k,) + v for k, v in A.AUX.items()]:
        body = bodies(V)
        pp, pt = A.pose_batch(body, sizes, seed, far)
        assert pp.shape[0] == sum(sizes)
        cj, cm, det = A.conditioning(body, pp, pt)
        assert cj.min() >= A.COND_MIN and cm.min() >= A.COND_MIN, (name, cj.min(), cm.min())
        improper[name] = (det < 0).sum(axis=0)
        if far and sum(sizes) > 2:
            assert improper[name][0] >= 1 and improper[name][1] >= 1, (name, improper[name])
    for mname, (pp, pt) in A.golden_motions(metrics, bodies(6890)).items():
        assert pp.shape[0] == 24
        cj, cm, det = A.conditioning(bodies(6890), pp, pt)
        assert cj.min() >= A.COND_MIN and cm.min() >= A.COND_MIN, (mname, cj.min(), cm.min())
        improper["golden " + mname] = (det < 0).sum(axis=0)
    assert improper["golden far"][0] >= 1                         # the captured reference ran its row flip on a pose pair
    sets = [(f"m={m} n={n}", A.point_sets(seed, n, m, mirrored), m, mirrored) for m, n, seed, mirrored in A.SVD_CASES]
    sets += [(k, A.point_sets(*v), v[2], v[3]) for k, v in A.GOLDEN_POINTS.items()]
    sets += [("exact", A.point_sets(*A.EXACT_POINTS), A.EXACT_POINTS[2], False)]
    for name, (src, dst, _), m, mirrored in sets:
        if A.R_DEFINED(m):
            assert A.conditioning_points(src, dst).min() >= A.COND_MIN, name
        if m >= A.UNCENTRED_FROM:
            assert A.conditioning_points(src, dst, centre=False).min() >= A.COND_MIN, name
        if mirrored:
            a, b = src.astype(np.float64), dst.astype(np.float64)
            a, b = a - a.mean(axis=1, keepdims=True), b - b.mean(axis=1, keepdims=True)
            assert (np.linalg.det(np.matmul(a.transpose(0, 2, 1), b)) < 0).all(), name
    print("frames with an improper fit (joints, mesh):", {k: tuple(int(x) for x in v) for k, v in improper.items()})


def test_root_turned_prediction_is_recovered_by_the_rotating_modes(bodies):
    """prediction = truth with the root turned far from I: modes -1 and -2 undo it, mode -4 (translation only) cannot"""
    body = bodies(1025)
    _, pt = A.aux("root turned", body)
    pp, _ = A.root_turned(pt, 491)
    cj, cm, _ = A.conditioning(body, pp, pt)
    assert cj.min() >= A.COND_MIN and cm.min() >= A.COND_MIN
    for mode in (-1, -2):
        r = A.evaluate(body, pp, pt, mode)
        assert r["joint_err"].max() < 1e-6 and r["mesh_err"] < 1e-6
    assert A.evaluate(body, pp, pt, -4)["joint_err"].max() > 1e-2
