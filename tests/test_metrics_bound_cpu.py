"""The bounds of the evaluation metrics are neither too loose nor too tight, shown without a GPU.

tests/test_gpu_metrics_edges.py holds rc_metrics.hip (reconstruction_error, mesh_metrics, forward_mesh) to the bounds of
oracle/metrics_f64.py at its frame-group, vertex-slab, chunk and lane edges. Here the same cases and bounds meet CPU evaluations:
  * every Procrustes case is admitted: the float64 SVD restatement and Horn's quaternion form (mpmath, 50 digits, where it is
    installed) agree to Bound_pa / 8; the deliberately mirrored full-extent sets keep (sigma2 - sigma3) / sigma1 >= 0.05. A thin,
    collinear or two-point set has sigma2 / sigma1 <= its thin extent by construction: what is not unique there is a turn
    about the long axis, whose lever is that extent; the e64 gate measures it, and the relative gap (sigma2 - sigma3) / sigma2
    is reported. The regular tetrahedron and the cube against their mirror images (sigma1 = sigma2 = sigma3, det < 0) are
    compared in the sum of squared residuals only;
  * three float32 association orders of the reference formulation stay at or below a third of the Bound on every mesh case;
  * the reference's own capture (tests/golden/metrics.npz) sits inside the bounds: the restatement is the reference's;
  * every mutation of the restatement reaches three times the Bound or more on the case named beside it;
  * a line-for-line float64 emulation of the Procrustes stage as it stood before the one-sided Jacobi (right singular vectors
    from the eigenvectors of K^T K) exceeds Bound_pa on thin rungs, the emulation of the one-sided route stays inside on all.
So a kernel with one of those slips could not pass the GPU test. RC_METRICS_RATIOS_OUT=<file> keeps the printed tables.
"""
import os

import numpy as np
import pytest

from oracle import metrics_f64 as F


def _emit(lines):
    for ln in lines:
        print(ln)
    path = os.environ.get("RC_METRICS_RATIOS_OUT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "metrics.npz"))


@pytest.fixture(scope="module")
def cases(golden):
    return F.build_mesh_cases(golden)


@pytest.fixture(scope="module")
def evaluated(cases):
    return {c.name: F.evaluate_case(c) for c in cases}


@pytest.fixture(scope="module")
def pa_groups():
    out = []
    for g in F.build_pa_groups() + F.ill_posed_groups():
        out.append((g, F.procrustes(g.S1, g.S2), F.procrustes_second(g.S1, g.S2)))
    return out


def _ratio(err, bound):
    """err / bound with 0 / 0 = 0 (a single point: every quantity is exactly zero)"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    return np.where(err == 0.0, 0.0, err / np.where(bound == 0.0, 1e-300, bound))


def test_every_procrustes_case_is_admitted(pa_groups):
    names = [g.name for g, _, _ in pa_groups]
    for k in F.PA_NK:
        assert f"generic nk={k}" in names and f"generic nk={k} mirrored" in names
    for ext in F.LADDER:
        assert f"thin {F.ext_name(ext)}" in names and f"thin {F.ext_name(ext)} mirrored" in names
    lines = [f"Procrustes cases: e64 = |float64 SVD - Horn ({'mpmath 50 digits' if F._mp is not None else 'float64'})| / Bound_pa (admitted: <= 1/{F.ADMIT:g});"
             " gap = min (s2 - s3) / s1, rel = min (s2 - s3) / s2"]
    gaps = []
    for g, r, s in pa_groups:
        sg = r["sigma"]
        with np.errstate(invalid="ignore", divide="ignore"):
            gap = float(np.nanmin(np.where(sg[:, 0] > 0, (sg[:, 1] - sg[:, 2]) / sg[:, 0], np.nan))) if (sg[:, 0] > 0).any() else float("nan")
            rel = float(np.nanmin(np.where(sg[:, 1] > 0, (sg[:, 1] - sg[:, 2]) / sg[:, 1], np.nan))) if (sg[:, 1] > 0).any() else float("nan")
        if g.kind == "ssq":
            d = float(np.max(np.abs(r["ssq"] - s["ssq"]) / r["ssq"]))
            lines.append(f"  {g.name:46s} ssq only: |ssq SVD - ssq Horn| / ssq {d:.1e}, mean distance {r['mean'][0]:.4f} (SVD) {s['mean'][0]:.4f} (Horn), gap {gap:.1e}")
            assert d <= 1e-12 and gap <= 1e-12 and (r["sign"] < 0).all()
            continue
        e64 = float(_ratio(np.abs(r["mean"] - s["mean"]), F.bound_pa(r["A"])).max())
        lines.append(f"  {g.name:46s} n {len(r['mean']):2d} det<0 {int((r['sign'] < 0).sum()):2d}  e64 {e64:.1e}  gap {gap:.1e}  rel {rel:.1e}")
        assert e64 <= 1.0 / F.ADMIT, g.name
        flat = sg[:, 2] <= 1e-12 * sg[:, 0]               # a coplanar set (three points too): its mirror image is a turned copy
        if g.mirrored and not g.thin:
            assert ((r["sign"] < 0) | flat).all(), g.name
            assert gap >= F.GAP_MIN, g.name
            gaps.append(gap)
        elif g.mirrored:
            assert ((r["sign"] < 0) | flat).all() and rel >= F.GAP_MIN, g.name
    lines.append(f"  min (s2 - s3) / s1 over the mirrored full-extent sets compared in the mean: {min(gaps):.3f} (>= {F.GAP_MIN})")
    _emit(lines)
    assert len(gaps) == len(F.PA_NK) + 1


def test_float32_orders_stay_within_a_third_of_the_bound(cases, evaluated):
    lines = [f"mesh metrics, M = {F.M:g}: worst float32 order / Bound per case (MPJPE, PVE, PA); e32; eps32 A"]
    for c in cases:
        ev = evaluated[c.name]
        r = np.max([_ratio(np.abs(ev["f32"][o] - ev["ref"]), ev["Bound"]) for o in F.ORDERS], axis=(0, 1))
        lines.append(f"  {c.name:40s} " + " ".join(f"{v:.3f}" for v in r) + "   e32 " + " ".join(f"{v:.1e}" for v in ev["e32"]) +
                     "   eps32 A " + " ".join(f"{v:.1e}" for v in F.EPS32 * ev["A"].max(axis=0)))
        assert (r <= 1.0 / F.MARGIN).all(), c.name
        if c.exact_zero:
            assert (ev["ref"][:, :2] == 0.0).all() and all((ev["f32"][o][:, :2] == 0.0).all() for o in F.ORDERS)
    lines.append("mesh vertices: worst float32 order / Bound; e32; eps32 max A")
    for c, tran in ((cases[4], 100.0), (cases[6], 0.0), (cases[0], 100.0)):
        t = np.full((F.N_FRAMES, 3), tran, np.float32) * np.array([1.0, -1.0, 0.5], np.float32)
        mv = F.evaluate_mesh(c, t)
        r = max(float(_ratio(np.abs(mv["f32"][o] - mv["ref"]), mv["Bound"][..., None]).max()) for o in F.ORDERS)
        lines.append(f"  {c.name:40s} tran {tran:5.1f} m  {r:.3f}   e32 {mv['e32']:.1e}   eps32 A {F.EPS32 * mv['A'].max():.1e}")
        assert r <= 1.0 / F.MARGIN
    _emit(lines)


def test_reference_capture_sits_inside_the_bounds(golden, cases, evaluated):
    lines = ["reference capture (tests/golden/metrics.npz) / Bound: MPJPE, PVE, PA per pose pair; pa_err per set"]
    for c, key in ((cases[0], "near"), (cases[1], "far")):
        ev = evaluated[c.name]
        gold = np.stack([golden["frame_mpjpe_" + key], golden["frame_pve_" + key], golden["frame_pa_" + key]], axis=1).astype(np.float64)
        r = (np.abs(gold - ev["ref"][:24]) / ev["Bound"][:24]).max(axis=0)
        lines.append(f"  {key:5s} " + " ".join(f"{v:.3f}" for v in r))
        assert (r <= 1.0).all(), key
        mean = np.abs(golden["cal_" + key] - ev["ref"][:24].mean(axis=0)) / ev["Bound"][:24].max(axis=0)
        assert (mean <= 1.0).all(), key
    body, Jr = F.body_of(6890), F.regressor_of(cases[0])
    ref, A = F.frame_metrics_f64(body, Jr, 14, golden["pose_gt"], golden["pose_gt"])
    gold = np.stack([golden["frame_mpjpe_same"], golden["frame_pve_same"], golden["frame_pa_same"]], axis=1).astype(np.float64)
    r = (np.abs(gold - ref) / F.bound(0.0, A)).max(axis=0)
    lines.append("  same  " + " ".join(f"{v:.3f}" for v in r))
    assert (r <= 1.0).all() and (ref[:, :2] == 0.0).all()
    pr = F.procrustes(golden["pa_S1"], golden["pa_S2"])
    r = np.abs(golden["pa_err"] - pr["mean"]) / F.bound_pa(pr["A"])
    lines.append("  pa_err " + " ".join(f"{v:.3f}" for v in r) + "   (float32 SVD in the reference; det<0: " + " ".join("yes" if s < 0 else "no" for s in pr["sign"]) + ")")
    assert (r <= 1.0).all()
    _emit(lines)


# mutation -> the case built for it (and the column it must show in: 0 MPJPE, 1 PVE, 2 PA)
MESH_MUTATION_CASES = {
    "pelvis_kp1": ("near V=1025 onehot17", 0),
    "align_before_pve": ("far V=2049 signed14", 1),
    "pve_padded_count": ("far V=1025 convex17", 1),
    "mpjpe_all_rows": ("far V=1024 convex1", 0),
    "tran_kept": ("identical V=1025 convex14", 1),
    "fold_without_root": ("near V=1025 onehot17", 0),
    "weight_row_shifted": ("near V=1023 convex14", 1),
    "group_last_frame_repeated": ("rigid root rotation V=1025 convex14", 0),
}
PA_MUTATION_CASES = {
    "no_Z": "generic nk=14 mirrored",
    "scale_1": "generic nk=14",
    "scale_var2": "generic nk=14",
    "R_transposed": "generic nk=4",
    "means_kept": "offset 1e3 m",
}


def test_every_mutation_lands_beyond_three_times_the_bound(cases, evaluated, pa_groups):
    assert set(MESH_MUTATION_CASES) == set(F.MESH_MUTATIONS) and set(PA_MUTATION_CASES) == set(F.PA_MUTATIONS)
    by_name = {c.name: c for c in cases}
    lines = [f"mutations: error / Bound on the case named (>= {F.MARGIN:g} required)"]
    for mut, (name, col) in MESH_MUTATION_CASES.items():
        c, ev = by_name[name], evaluated[name]
        out = F.frame_metrics_f64(F.body_of(c.V), F.regressor_of(c), c.n_used, c.pose, c.gt, mut=mut, tran=c.tran)[0]
        r = float((np.abs(out - ev["ref"]) / ev["Bound"])[:, col].max())
        lines.append(f"  {mut:26s} {r:12.1f}  {('MPJPE', 'PVE', 'PA')[col]:5s} {name}")
        assert r >= F.MARGIN, mut
    c = by_name["near V=1023 convex14"]
    mv = F.evaluate_mesh(c, None)
    shifted = F._skin(F.body_of(c.V), c.pose, None, np.float64, shift_row=c.V - 1)
    r = float((np.abs(shifted - mv["ref"]) / mv["Bound"][..., None]).max())
    lines.append(f"  {'weight_row_shifted':26s} {r:12.1f}  vertex {c.name} (the last vertex of the slab)")
    assert r >= F.MARGIN
    groups = {g.name: (g, r) for g, r, _ in pa_groups}
    for mut, name in PA_MUTATION_CASES.items():
        g, ref = groups[name]
        out = F.procrustes(g.S1, g.S2, mut=mut)
        r = float(_ratio(np.abs(out["mean"] - ref["mean"]), F.bound_pa(ref["A"])).max())
        lines.append(f"  {mut:26s} {r:12.1f}  PA    {name}")
        assert r >= F.MARGIN, mut
    _emit(lines)


# thin rungs on which the K^T K emulation must exceed Bound_pa (measured on these seeds; the others are recorded)
KTK_FAILS = ("thin (1,0.0001,0.0001) mirrored", "thin (1,0.0001,0)", "thin (1,0.0001,0) mirrored")


def test_ktk_route_fails_thin_rungs_and_the_one_sided_route_does_not(pa_groups):
    """Measured here (8 draws per rung, error / Bound_pa against Horn in mpmath): the K^T K route reaches 9.9 on (1,1e-4,1e-4)
    mirrored and 11.9 / 13.6 on (1,1e-4,0); (1,1e-5,1e-5) mirrored reaches 0.18 on these eight draws (the 200 draws behind the
    route's replacement found 6e-7 m there, 4.5 x the bound). The one-sided route stays below 2e-7 of the bound on every rung."""
    lines = ["thin ladder, error / Bound_pa against Horn: K^T K eigen route (before) | one-sided Jacobi on K (now)"]
    worst = {}
    for g, r, s in pa_groups:
        if not g.thin:
            continue
        B = F.bound_pa(r["A"])
        ktk = float(_ratio(np.abs(F.route(F.ktk_route_one, g.S1, g.S2) - s["mean"]), B).max())
        hes = float(_ratio(np.abs(F.route(F.hestenes_route_one, g.S1, g.S2) - s["mean"]), B).max())
        worst[g.name] = (ktk, hes)
        lines.append(f"  {g.name:36s} {ktk:10.2e} | {hes:10.2e}")
    _emit(lines)
    for name in KTK_FAILS:
        assert worst[name][0] >= F.MARGIN, name
    assert max(h for _, h in worst.values()) <= 1.0 / F.ADMIT
    assert sum(k > 1.0 for k, _ in worst.values()) >= len(KTK_FAILS)
