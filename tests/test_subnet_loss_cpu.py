"""The losses of the sub-nets without a GPU: the float64 restatement (tests/subnet_loss_f64.py: value and closed-form gradient) against
torch float64 autograd of the same formulas to 1e-12 relative, the window indexing from the end of the batch, the degenerate joints of
pose_fk, pos_weight_from_labels, config.LOSS, and that the geometry constants of robustcap_amd/losses.py are those the kernels are built
with. The torch formulas below are also the fp32 leg of test_gpu_subnet_loss.py."""
import os
import re

import numpy as np
import pytest
import torch

import subnet_loss_f64 as F64
from robustcap_amd import config as cfg
from robustcap_amd import losses
from robustcap_amd import synth

REL = 1e-12


# ---- the formulas in torch (any dtype), differentiated by autograd ------------------------------------------------------------------------
def torch_mse(x, y):
    return ((x - y) ** 2).mean()


def torch_bce_logits(x, y, pw):
    return torch.nn.functional.binary_cross_entropy_with_logits(x, y, pos_weight=pw)


def torch_window_mse(x, y):
    F = x.shape[0]
    v = torch_mse(x, y)
    for w in F64.WINDOWS:
        v = v + torch_mse(x[F % w:].reshape(-1, w, 3).sum(dim=1), y[F % w:].reshape(-1, w, 3).sum(dim=1))
    return v


def torch_joints(p, bones, parent):
    v = p.reshape(-1, 6)
    a, b = v[:, :3], v[:, 3:]
    c0 = a / a.norm(dim=1, keepdim=True)
    t = b - (c0 * b).sum(dim=1, keepdim=True) * c0
    c1 = t / t.norm(dim=1, keepdim=True)
    c2 = torch.cross(c0, c1, dim=1)
    R = torch.stack((c0, c1, c2), dim=-1)
    R = torch.where(torch.isnan(R), torch.zeros_like(R), R).reshape(-1, 24, 3, 3)
    J = [torch.zeros(R.shape[0], 3, dtype=p.dtype)]
    for i in range(1, 24):
        J.append(J[int(parent[i])] + R[:, int(parent[i])] @ bones[i])
    return torch.stack(J, dim=1)


def torch_pose_fk(x, y, bones, parent):
    return torch_mse(x, y) + 100 * torch_mse(torch_joints(x, bones, parent), torch_joints(y, bones, parent))


def torch_loss(kind, x, y, dtype, pos_weight=None, bones=None, parent=None):
    """(value, dx) as float64 numpy from torch autograd on the CPU in `dtype`."""
    x = torch.as_tensor(np.asarray(x)).to(dtype).requires_grad_()
    y = torch.as_tensor(np.asarray(y)).to(dtype)
    if kind == "mse":
        v = torch_mse(x, y)
    elif kind == "bce_logits":
        v = torch_bce_logits(x, y, torch.as_tensor(np.asarray(pos_weight)).to(dtype))
    elif kind == "window_mse":
        v = torch_window_mse(x, y)
    else:
        v = torch_pose_fk(x, y, torch.as_tensor(np.asarray(bones)).to(dtype), parent)
    v.backward()
    return float(v.detach().double()), x.grad.double().numpy()


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max()) <= REL * max(float(np.abs(b).max()), 1e-300)


def _rand(shape, seed, scale=1.0):
    return (scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))).numpy()


# ---- the inputs both test files use -----------------------------------------------------------------------------------------------------
BCE_POS_WEIGHT = (3.5, 0.25)


def bce_inputs(F, seed):
    """Labels in {0, 1}; x random with 0, +-30 and +-100 planted in both columns (as far as F reaches)."""
    g = torch.Generator().manual_seed(seed)
    x = 3.0 * torch.randn(F, 2, generator=g)
    y = (torch.rand(F, 2, generator=g) < 0.4).float()
    for i, v in enumerate((0.0, 30.0, -30.0, 100.0, -100.0, 100.0, -100.0, 0.0, 30.0, -30.0)):
        if i < 2 * F:
            x.view(-1)[(7 * i) % (2 * F)] = v
    return x.numpy(), y.numpy()


def pose_inputs(F, seed):
    """Labels: the first two columns of random rotations; predictions: labels + 0.2 randn. float32 arrays [F, 144]."""
    g = torch.Generator().manual_seed(seed)
    q, r = torch.linalg.qr(torch.randn(F * 24, 3, 3, generator=g))
    q = q * torch.sign(torch.diagonal(r, dim1=1, dim2=2)).unsqueeze(1)
    y = q[:, :, :2].transpose(1, 2).reshape(F, 144).contiguous()
    x = y + 0.2 * torch.randn(F, 144, generator=g)
    return x.numpy(), y.numpy()


def pose_margins(v):
    """min |a| and min sin of the angle between a and b over all joints of v [F, 144]."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 6)
    a, b = v[:, :3], v[:, 3:]
    na, nb = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)
    return float(na.min()), float((np.linalg.norm(np.cross(a, b), axis=1) / (na * nb)).min())


DEGENERATE = ((1, 3), (2, 12))      # (frame, joint) with a = 0 | with b = 2 a; both joints have children


def degenerate_pose_inputs(F=4, seed=23):
    """pose_inputs with joint 3 of frame 1 given a = 0 and joint 12 of frame 2 given a = (0, 0.5, 0), b = 2 a. The second is axis-aligned
    on purpose: c0 = (0, 1, 0), d = 1 and t = b - d c0 = 0 are then EXACT in every precision, so |t| = 0 and the branch (NaN -> 0) is
    taken by float64, by fp32 and by the kernel alike; a general a leaves t as rounding noise whose direction no two of them share."""
    x, y = pose_inputs(F, seed)
    (f0, j0), (f1, j1) = DEGENERATE
    x[f0, 6 * j0:6 * j0 + 3] = 0.0
    x[f1, 6 * j1:6 * j1 + 6] = (0.0, 0.5, 0.0, 0.0, 1.0, 0.0)
    keep = np.ones((F, 144), bool)
    keep[f0, 6 * j0:6 * j0 + 6] = False
    keep[f1, 6 * j1:6 * j1 + 6] = False
    return x, y, keep


WINDOW_FRAMES = (60, 61, 119, 120, 121, 125)
WINDOW_LISTS = ((59, 1), (7, 60, 58))


def body_bones():
    return F64.rest_bones(synth.make_body(1))


# ---- the restatement against torch float64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [69, 3])
def test_mse_restatement(W):
    x, y = _rand((37, W), 1), _rand((37, W), 2)
    v, g = F64.mse(x, y)
    tv, tg = torch_loss("mse", x, y, torch.float64)
    assert _close(v, tv) and _close(g, tg)


def test_bce_logits_restatement():
    x, y = bce_inputs(41, 3)
    assert {0.0, 30.0, -30.0, 100.0, -100.0} <= set(x.reshape(-1).tolist()) and set(y.reshape(-1).tolist()) == {0.0, 1.0}
    v, g = F64.bce_logits(x, y, BCE_POS_WEIGHT)
    tv, tg = torch_loss("bce_logits", x, y, torch.float64, pos_weight=BCE_POS_WEIGHT)
    assert np.isfinite(v) and np.isfinite(g).all()
    assert _close(v, tv) and _close(g, tg)


@pytest.mark.parametrize("lengths", [(F,) for F in WINDOW_FRAMES] + list(WINDOW_LISTS))
def test_window_mse_restatement_and_indexing(lengths):
    F = sum(lengths)
    xs, ys = [_rand((T, 3), 10 + i) for i, T in enumerate(lengths)], [_rand((T, 3), 20 + i) for i, T in enumerate(lengths)]
    x, y = np.concatenate(xs), np.concatenate(ys)                      # RNNLossWrapper: concatenated first, windows cross the boundaries
    v, g = F64.window_mse(x, y)
    tv, tg = torch_loss("window_mse", x, y, torch.float64)
    assert _close(v, tv) and _close(g, tg)
    for w in F64.WINDOWS:
        k, nw = F64.window_of(F, w)
        assert nw == F // w and (k[:F % w] == -1).all() and (k[F % w:] >= 0).all()
        assert k[-1] == 0 and k[F % w] == nw - 1 and all((k == q).sum() == w for q in range(nw))


def test_window_mse_below_60_frames():
    x, y = _rand((59, 3), 30), _rand((59, 3), 31)
    tv, _ = torch_loss("window_mse", x, y, torch.float64)
    assert np.isnan(tv)                                                # the mean of an empty tensor
    with pytest.raises(ValueError, match="60"):
        F64.window_mse(x, y)
    with pytest.raises(ValueError, match="60"):
        losses.check_frames("window_mse", 59)
    losses.check_frames("window_mse", 60)
    losses.check_frames("mse", 1)


@pytest.mark.parametrize("F", [1, 5])
def test_pose_fk_restatement(F):
    bones, parent = body_bones()
    x, y = pose_inputs(F, 40 + F)
    assert min(pose_margins(x)) > 0.05
    v, g = F64.pose_fk(x, y, bones, parent)
    tv, tg = torch_loss("pose_fk", x, y, torch.float64, bones=bones, parent=parent)
    assert _close(v, tv) and _close(g, tg)
    leaves = [j for j in range(24) if j not in set(int(p) for p in parent[1:])]
    assert leaves == [10, 11, 15, 22, 23]
    _, gm = F64.mse(x, y)
    for j in leaves:                                                   # a leaf turns no bone: only the mse part
        assert np.array_equal(g[:, 6 * j:6 * j + 6], gm[:, 6 * j:6 * j + 6])


def test_pose_fk_degenerate_joints():
    bones, parent = body_bones()
    x, y, keep = degenerate_pose_inputs()
    v, g = F64.pose_fk(x, y, bones, parent)
    tv, tg = torch_loss("pose_fk", x, y, torch.float64, bones=bones, parent=parent)
    assert np.isfinite(v) and _close(v, tv)
    assert np.isfinite(tg[keep]).all() and np.isnan(tg[~keep]).all()   # autograd: NaN in exactly the two joints' six inputs
    assert np.isfinite(g[keep]).all() and _close(g[keep], tg[keep])


def test_pos_weight_from_labels():
    ls = [torch.tensor([[1.0, 0.0], [1.0, 1.0]]), torch.tensor([[0.0, 0.0], [1.0, 0.0], [0.0, 0.0]])]
    pw = losses.pos_weight_from_labels(ls)
    l = torch.cat(ls)
    assert torch.equal(pw, (1 - l).sum(dim=0) / l.sum(dim=0)) and pw.tolist() == [float(np.float32(2.0) / np.float32(3.0)), 4.0]
    assert torch.equal(losses.pos_weight_from_labels(l), pw)


def test_config_loss_covers_the_sub_nets():
    assert sorted(cfg.LOSS) == sorted(n for n, *_ in cfg.NETS)
    out = {n: o for n, _, _, o in cfg.NETS}
    for name, kind in cfg.LOSS.items():
        assert kind in losses.KINDS and out[name] in losses.WIDTHS[kind], name
    assert cfg.LOSS["rnn3"] == "window_mse" and cfg.LOSS["rnn7"] == "pose_fk" and cfg.LOSS["rnn8"] == "bce_logits"


def test_geometry_constants_are_the_kernels():
    src = open(os.path.join(os.path.dirname(losses.__file__), "csrc", "rc_internal.h")).read()
    define = lambda k: int(re.search(rf"^#define {k}\s+(\d+)", src, flags=re.M).group(1))
    assert (losses.VEC, losses.CHUNK, losses.WINDOW_FRAMES, losses.POSE_FRAMES, losses.MAX_PARTIALS) == tuple(
        define(k) for k in ("RC_LOSS_VEC", "RC_LOSS_CHUNK", "RC_LOSS_WINDOW_FRAMES", "RC_LOSS_POSE_FRAMES", "RC_LOSS_MAX_PARTIALS"))
    assert losses.WINDOW_FRAMES % 60 == 0 and losses.CHUNK % (256 * losses.VEC) == 0 and losses.POSE_FRAMES % 4 == 0
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(losses.__file__)), "include", "robustcap_hip.h")).read()
    for kind, code in losses.KINDS.items():
        assert re.search(rf"RC_LOSS_{kind.upper()} = {code}\b", hdr), kind


def test_wrapper_checks_need_no_device():
    class FakeNet:
        device = torch.device("cpu")
    with pytest.raises(ValueError):
        losses.SubnetLoss(FakeNet(), "huber")
    with pytest.raises(ValueError):
        losses.SubnetLoss(FakeNet(), "mse", width=2)
    with pytest.raises(ValueError):
        losses.SubnetLoss(FakeNet(), "mse", pos_weight=[1.0, 1.0])
    loss = losses.SubnetLoss(FakeNet(), "window_mse", width=3)
    with pytest.raises(ValueError, match="60"):
        loss([torch.zeros(59, 3)], [torch.zeros(59, 3)])
    with pytest.raises(ValueError, match="width"):
        loss(torch.zeros(60, 2), torch.zeros(60, 2))
    with pytest.raises(ValueError, match="frames"):
        loss([torch.zeros(30, 3), torch.zeros(31, 3)], [torch.zeros(60, 3)])
    with pytest.raises(ValueError, match="float32"):
        loss(torch.zeros(60, 3), torch.zeros(60, 3, dtype=torch.float64))
    a = torch.arange(30.0).reshape(10, 3)
    views = list(torch.split(a, [3, 1, 6]))
    flat = losses._flat_view(views)
    assert flat is not None and flat.data_ptr() == a.data_ptr() and torch.equal(flat, a)
    assert losses._flat_view([views[0], views[2]]) is None and losses._flat_view([views[1], views[0]]) is None
