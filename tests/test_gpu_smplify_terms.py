"""rc_smplify_loss_grad against the float64 closure, term by term and joint by joint.

tests/test_gpu_smplify.py holds the whole gradient to 1e-4 .. 2e-4 of its largest component, which the reprojection term sets:
the gradients of the GMM prior, of the 3D term and of the 2D smoothness lie wholly below that bar. Here every case of
oracle/smplify_f64.build_cases (near the optimum; prior alone; 3D term alone; smoothness alone, also with bitwise-equal
neighbouring frames; poses with joints at exactly 0, components of 1e-6, an angle of 3.1 and the angle prior at +-1.5; T in
{1, 2, 64, 65, 150}; a camera with skew) is compared in 25 groups (24 joints, translation) and in the loss with the float64
closure: error / Bound <= 1, Bound = M max(e32, eps32 A) (oracle/smplify_f64.Bound; tests/test_smplify_bound_cpu.py shows on
the CPU that float32 orders of the reference formulation stay within a third of it and every mutation lands beyond three
times it). The mixture chosen per frame shows only through the gradient: that is what the prior-alone cases are for.
RC_SMPLIFY_RATIOS_OUT=<file> keeps the table of the last test.
"""
import os

import pytest
import torch

from oracle import smplify_f64 as F

pytestmark = pytest.mark.gpu
WORST = {}                               # (kind, group kind) -> (ratio, case, group)
_RUNNERS = {}


@pytest.fixture(scope="module")
def body(synth_assets):
    return synth_assets["body"]


def runner_of(body, case):
    from robustcap_amd.smplify import TemporalSMPLify
    key = (id(body), case.gmm, case.use_head)
    if key not in _RUNNERS:
        _RUNNERS[key] = (body, TemporalSMPLify(body=body, gmm=F.gmm_of(case.gmm), use_head=case.use_head))
    return _RUNNERS[key][1]


def kernel(body, case):
    loss, gp, gt = runner_of(body, case).loss_and_grad(case.body_pose, case.tran, case.kp, case.ref3d, case.imu_aa, case.K)
    return loss, gp.cpu(), gt.cpu()


def _note(kind, case, ratios, loss_ratio):
    for gk, r, name in (("joint", float(ratios[:24].max()), F.GROUP_NAMES[int(ratios[:24].argmax())]), ("tran", float(ratios[24]), "tran"),
                        ("loss", float(loss_ratio), "loss")):
        if r >= WORST.get((kind, gk), (-1.0,))[0]:
            WORST[(kind, gk)] = (r, case.name, name)


@pytest.mark.parametrize("kind", ["near", "prior", "body3d", "smooth", "edges"])
def test_every_group_within_the_float64_bound(kind, body):
    failures = []
    cases = F.build_cases(body, kinds=(kind,))
    assert len(cases) == {"near": 10, "prior": 10, "body3d": 20, "smooth": 24, "edges": 10}[kind]
    for c in cases:
        ev, b, _ = F.bound_of(body, c)
        loss, gp, gt = kernel(body, c)
        r, lr = b.ratios(gp, gt), b.loss_ratio(loss)
        _note(kind, c, r, lr)
        k = int(r.argmax())
        print(f"{c.name:24s} worst group {F.GROUP_NAMES[k]:7s} error/Bound {r[k]:.3f}  tran {r[24]:.3f}  loss {lr:.3f}")
        if not (r.max() <= 1.0 and lr <= 1.0):
            failures.append((c.name, F.GROUP_NAMES[k], float(r[k]), float(lr)))
    assert not failures, failures


@pytest.mark.parametrize("T", [3, 65])
def test_copies_of_one_frame_have_the_single_frame_gradient(T, body):
    """T bitwise-equal frames: every smoothness difference is exactly 0 (sgn(0) = 0), so every frame's gradient is the T = 1
    gradient of that frame, bit for bit, on both sides of the prior kernel's 64-frame block edge."""
    one = F.build_cases(body, kinds=("near",))[0]
    assert one.T == 1
    rep = lambda x: x.expand(T, *x.shape[1:]).contiguous()
    many = F.Case("near", f"copies-T{T}", rep(one.body_pose), rep(one.tran), rep(one.kp), rep(one.ref3d), rep(one.imu_ori), one.K)
    _, gp1, gt1 = kernel(body, one)
    _, gp, gt = kernel(body, many)
    assert bool(torch.isfinite(gp).all()) and float(gp1.abs().max()) > 0
    for f in range(T):
        assert torch.equal(gp[f], gp1[0]) and torch.equal(gt[f], gt1[0]), f


def test_zz_report_worst_ratios():
    """The largest error / Bound per (case kind, group kind) over the cases above (pytest -s shows it)."""
    lines = [f"worst {kind:7s} {gk:5s} {r:.3f}  ({case}, {name})" for (kind, gk), (r, case, name) in sorted(WORST.items())]
    for ln in lines:
        print(ln)
    path = os.environ.get("RC_SMPLIFY_RATIOS_OUT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")
    assert len(WORST) == 15 and all(v[0] <= 1.0 for v in WORST.values())
