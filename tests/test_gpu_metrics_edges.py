"""rc_metrics.hip against the float64 restatement of oracle/metrics_f64.py at its dispatch edges.

  reconstruction_error   every Procrustes group of metrics_f64.build_pa_groups (generic and mirrored sets at nk in {3, 4, 14, 24, 33},
                         coplanar, the thin ladder (1, e, e) / (1, e, 0), collinear, bitwise equal sets, an exact similarity copy,
                         millimetre scale, an offset of 1e3 m, nk = 1 and 2, var1 = 0) within Bound_pa = 4 * 2^-24 * A of the float64
                         SVD restatement; n in {1, 63, 64, 65, 129} sets in one launch (the 64-lane edge) bitwise equal to each alone.
                         (The regular tetrahedron and the cube against their mirror images are ill-posed in the mean distance and
                         have more than two points: they stay in tests/test_metrics_bound_cpu.py, compared in the sum of squares.)
  mesh_metrics           every case of metrics_f64.build_mesh_cases -- V in {1023, 1024, 1025, 2049, 6890} (the 1024-vertex slab edge),
                         no regressor / convex with n_used in {1, 14, 17} / one-hot / signed rows, the capture's near and far pairs,
                         identical poses, one leaf joint, a rigid root rotation -- within Bound = M max(e32, eps32 A) per column;
                         n in {1, 15, 16, 17, 33} frames (the 16-frame group edge) and every frame alone, bitwise equal to the batch.
  forward_mesh           all V vertices within the vertex Bound (a translation of 100 m among them), the same frame counts bitwise.
  the chunk edge         65,537 frames at V = 1025 (33 distinct frames repeated: frame 65,536 is a copy of frame 31, not of frame 0),
                         mesh_metrics and forward_mesh (0.8 GB of vertices), every frame bitwise equal to its copy in a 33-frame call.
A smaller mesh than the landmark ids reach cannot go through ParametricModel's constructor: the helper below sets it through
rc_set_mesh on a model built from the 6890-vertex body (same seed, hence the same joints). tests/test_metrics_bound_cpu.py shows
on the CPU that float32 orders stay within a third of these bounds and every mutation lands beyond three times them.
RC_METRICS_RATIOS_OUT=<file> keeps the worst error / Bound per group.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import metrics_f64 as F

pytestmark = pytest.mark.gpu
t = torch.from_numpy
WORST = {}
N_CASES = 14


def _note(key, ratio, what):
    if key not in WORST or ratio > WORST[key][0]:
        WORST[key] = (float(ratio), what)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "metrics.npz"))


@pytest.fixture(scope="module")
def cases(golden):
    cs = F.build_mesh_cases(golden)
    assert len(cs) == N_CASES
    return cs


@pytest.fixture(scope="module")
def models(synth_assets):
    """model_of(V, regressor or None): a ParametricModel on the shared body whose mesh has V vertices"""
    from robustcap_amd import _lib
    from robustcap_amd.body import ParametricModel
    body = synth_assets["body"]
    cache = {}

    def model_of(V, Jr, n_used):
        key = (V, Jr is None)
        if key not in cache:
            m = ParametricModel(body=body)
            if V != body["v_template"].shape[0]:
                small = F.body_of(V)
                assert np.array_equal(small["J"], body["J"])                 # the joints depend on the seed alone
                vt = np.ascontiguousarray(small["v_template"], dtype=np.float32)
                w = np.ascontiguousarray(small["weights"], dtype=np.float32)
                _lib.check(m._ctx, m._lib.rc_set_mesh(m._ctx, vt.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), V), "rc_set_mesh")
                m._mesh_set, m._V = True, V
            cache[key] = m
        m = cache[key]
        if Jr is not None:
            m.set_regressor(Jr, n_used)
        return m
    return model_of


# ------------------------------------------------------------------------------------------------------ Procrustes
def test_procrustes_groups_within_the_float64_bound():
    from robustcap_amd.body import reconstruction_error
    groups = F.build_pa_groups()
    assert len(groups) == 2 * len(F.PA_NK) + 2 + 2 * len(F.LADDER) + 8
    for g in groups:
        ref = F.procrustes(g.S1, g.S2)
        B = F.bound_pa(ref["A"])
        dev = reconstruction_error(t(g.S1), t(g.S2)).cpu().numpy().astype(np.float64)
        err = np.abs(dev - ref["mean"])
        ratio = float(np.where(err == 0.0, 0.0, err / np.where(B == 0.0, 1e-300, B)).max())
        print(f"{g.name:46s} error / Bound_pa {ratio:.3f}  (mean {ref['mean'].max():.3e}, Bound {B.max():.2e})")
        _note(("procrustes", g.name), ratio, f"nk={g.S1.shape[1]}")
        assert np.isfinite(dev).all() and (err <= B).all(), (g.name, ratio)
        if g.name in ("S1 == S2 bitwise", "nk=1"):
            assert (dev == 0.0).all(), g.name
        if g.name in ("nk=2", "rotated scaled shifted copy"):
            assert (dev <= B).all(), g.name                                  # <= Bound around 0
        if g.name == "var1 = 0":                                             # the documented value: mean |S2_j - mu2|
            b = g.S2.astype(np.float64)
            want = np.sqrt(((b - b.mean(axis=1, keepdims=True)) ** 2).sum(axis=2)).mean(axis=1)
            assert (np.abs(dev - want) <= B).all()


def test_procrustes_sets_of_one_launch_equal_each_alone():
    """one lane per set, 64 lanes per workgroup: n in {1, 63, 64, 65, 129} sets in one launch, each bitwise the set run alone"""
    from robustcap_amd.body import reconstruction_error
    pool = [g for g in F.build_pa_groups() if g.S1.shape[1] == 14 and g.name != "var1 = 0"]
    S1, S2 = np.concatenate([g.S1 for g in pool])[::-1][:129].copy(), np.concatenate([g.S2 for g in pool])[::-1][:129].copy()
    assert S1.shape == (129, 14, 3)
    d1, d2 = t(S1).cuda(), t(S2).cuda()
    alone = torch.cat([reconstruction_error(d1[i:i + 1], d2[i:i + 1]) for i in range(129)])
    assert len({float(v) for v in alone}) > 100                             # distinct sets: a lane reading its neighbour's set shows
    for n in (1, 63, 64, 65, 129):
        assert torch.equal(reconstruction_error(d1[:n], d2[:n]), alone[:n]), n


# ---------------------------------------------------------------------------------------------------- mesh metrics
@pytest.mark.parametrize("idx", range(N_CASES))
def test_mesh_metrics_within_the_bound_and_rows_bitwise(idx, cases, models):
    c = cases[idx]
    ev = F.evaluate_case(c)
    Jr = F.regressor_of(c)
    model = models(c.V, Jr, c.n_used)
    pose, gt = t(c.pose).cuda(), t(c.gt).cuda()
    pf, mean = model.mesh_metrics(pose, gt)
    dev = pf.cpu().numpy().astype(np.float64)
    ratio = (np.abs(dev - ev["ref"]) / ev["Bound"]).max(axis=0)
    print(f"{c.name:40s} error / Bound: MPJPE {ratio[0]:.3f} PVE {ratio[1]:.3f} PA {ratio[2]:.3f}   Bound " + " ".join(f"{v:.1e}" for v in ev["Bound"].max(axis=0)))
    for col, name in enumerate(("MPJPE", "PVE", "PA")):
        _note(("mesh_metrics", name), ratio[col], c.name)
    assert np.isfinite(dev).all() and (ratio <= 1.0).all(), (c.name, ratio)
    assert np.abs(np.asarray(mean) - dev.mean(axis=0)).max() <= 1e-12
    if c.exact_zero:
        assert (dev == 0.0).all()
    if c.pa_zero:
        assert (dev[:, 2] <= ev["Bound"][:, 2]).all() and (dev[:, 0] > 1e-3).all()
    for n in F.FRAME_COUNTS[:-1]:                                            # a frame group's frames must not leak into the next
        assert torch.equal(model.mesh_metrics(pose[:n], gt[:n])[0], pf[:n]), n
    for f in range(F.N_FRAMES):
        assert torch.equal(model.mesh_metrics(pose[f:f + 1], gt[f:f + 1])[0], pf[f:f + 1]), f
    if c.reg == "onehot":                                                    # the keypoints are vertices of forward_mesh
        ids = F.onehot_ids(c)[:c.n_used]
        mv = F.evaluate_mesh(c, None)
        vp = model.forward_mesh(pose)[:, ids].cpu().numpy().astype(np.float64)
        vt = model.forward_mesh(gt)[:, ids].cpu().numpy().astype(np.float64)
        assert (np.abs(vp - mv["ref"][:, ids]) <= mv["Bound"][:, ids, None]).all()
        mp = np.sqrt((((vt - vt[:, :1]) - (vp - vp[:, :1])) ** 2).sum(axis=2)).mean(axis=1)
        assert (np.abs(mp - dev[:, 0]) <= ev["Bound"][:, 0]).all()


MESH_OF_V = {1023: (4, 100.0), 1024: (5, 0.3), 1025: (6, 0.0), 2049: (8, 0.3), 6890: (0, 100.0)}


@pytest.mark.parametrize("V", sorted(MESH_OF_V))
def test_forward_mesh_within_the_vertex_bound_and_rows_bitwise(V, cases, models):
    idx, size = MESH_OF_V[V]
    c = cases[idx]
    assert c.V == V
    tran = (np.full((F.N_FRAMES, 3), size, np.float32) * np.array([1.0, -1.0, 0.5], np.float32) + c.tran).astype(np.float32)
    mv = F.evaluate_mesh(c, tran)
    model = models(V, None, 0)
    pose, tr = t(c.pose).cuda(), t(tran).cuda()
    vert = model.forward_mesh(pose, tr)
    assert vert.shape == (F.N_FRAMES, V, 3)
    dev = vert.cpu().numpy().astype(np.float64)
    ratio = float((np.abs(dev - mv["ref"]) / mv["Bound"][..., None]).max())
    print(f"forward_mesh V={V} tran ~{size:g} m: error / Bound {ratio:.3f}  (e32 {mv['e32']:.1e}, Bound max {mv['Bound'].max():.1e})")
    _note(("forward_mesh", f"V={V}"), ratio, c.name)
    assert np.isfinite(dev).all() and ratio <= 1.0
    for n in F.FRAME_COUNTS[:-1]:
        assert torch.equal(model.forward_mesh(pose[:n], tr[:n]), vert[:n]), n
    for f in range(F.N_FRAMES):
        assert torch.equal(model.forward_mesh(pose[f:f + 1], tr[f:f + 1]), vert[f:f + 1]), f


def test_the_chunk_edge_of_65536_frames(cases, models):
    c = cases[6]
    assert c.V == 1025
    n, k = F.MET_CHUNK + 1, F.N_FRAMES
    idx = torch.arange(n, device="cuda") % k
    assert int(idx[F.MET_CHUNK]) == 31
    pose33, gt33 = t(c.pose).cuda(), t(c.gt).cuda()
    tran33 = t(c.tran).cuda()
    pose, gt = pose33[idx].contiguous(), gt33[idx].contiguous()
    model = models(c.V, F.regressor_of(c), c.n_used)
    pf33 = model.mesh_metrics(pose33, gt33)[0]
    assert not torch.equal(pf33[31], pf33[0])
    pf = model.mesh_metrics(pose, gt)[0]
    assert torch.equal(pf, pf33[idx])
    v33 = model.forward_mesh(pose33, tran33)
    vert = model.forward_mesh(pose, tran33[idx].contiguous())
    full = (n // k) * k
    assert torch.equal(vert[:full].view(n // k, k, c.V, 3), v33[None].expand(n // k, k, c.V, 3))
    assert torch.equal(vert[full:], v33[:n - full])


def test_zz_report_worst_ratios():
    """The largest error / Bound per group over the tests above (pytest -s shows it)."""
    if not WORST:
        print("no test of this file ran before the report")
        return
    lines = [f"device (rc_metrics.hip), M = {F.M:g}: worst error / Bound per group"]
    lines += [f"  {a:14s} {b:46s} {v:.3f}  ({what})" for (a, b), (v, what) in sorted(WORST.items())]
    for ln in lines:
        print(ln)
    path = os.environ.get("RC_METRICS_RATIOS_OUT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")
    assert max(v for v, _ in WORST.values()) <= 1.0
