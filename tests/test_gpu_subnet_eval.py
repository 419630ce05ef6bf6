"""The validation metric per validation batch in one call (losses.SubnetEval: rc_subnet_eval, csrc/rc_loss.hip; the reference's
``[eval_fn(net(d), l) for d, l in vald_dataloader]`` of articulate/utils/torch/train.py:101,131).

The four loss kinds are held BITWISE, group by group, to losses.SubnetLoss on the group's own slice (the entry runs the per-workgroup
code of rc_subnet_loss's kernels on every group); position_error is held to a float64 restatement: within 1e-7 |f64| (summed in double,
rounded to fp32 once: the floor test_gpu_subnet_loss.py holds such values to) and within K_F32 times the error of the fp32 torch
expression. Every figure is printed as a RATIO line before it is held to its bound (kept in profiles/subnet_eval_ratios.txt)."""
import ctypes as C

import numpy as np
import pytest
import torch

import subnet_loss_f64 as F64  # noqa: F401  (the float64 restatements of the four losses: what SubnetLoss itself is pinned to)
import test_gpu_subnet_forward as FWD
import test_subnet_loss_cpu as CPU
from robustcap_amd import _lib
from robustcap_amd import losses

pytestmark = pytest.mark.gpu

K_F32 = FWD.K_F32
PW = CPU.BCE_POS_WEIGHT
NET = None


def _shared_net():
    global NET
    if NET is None:
        NET = FWD._net(1)
    return NET


def _inputs(kind, F, W, seed):
    if kind == "bce_logits":
        return CPU.bce_inputs(F, seed)
    if kind == "pose_fk":
        return CPU.pose_inputs(F, seed)
    return CPU._rand((F, W), seed), CPU._rand((F, W), seed + 1)


def _per_group(kind, W, x, y, sizes):
    """SubnetLoss of that kind on every group's slice under no_grad (torch.split's views are cloned by the loss where they leave the
    16-byte grid: the aligned copy the entry's contract names), as a list of fp32 byte strings."""
    net = _shared_net()
    loss = losses.SubnetLoss(net, kind, pos_weight=PW if kind == "bce_logits" else None, width=W)
    out = []
    with torch.no_grad():
        for xg, yg in zip(torch.split(x, sizes), torch.split(y, sizes)):
            out.append(loss(xg, yg).cpu().numpy().tobytes())
    return out


def _bitwise(kind, W, sizes, seed):
    net = _shared_net()
    sizes = list(sizes)
    xn, yn = _inputs(kind, sum(sizes), W, seed)
    x, y = torch.from_numpy(np.ascontiguousarray(xn)).cuda(), torch.from_numpy(np.ascontiguousarray(yn)).cuda()
    ev = losses.SubnetEval(net, kind, pos_weight=PW if kind == "bce_logits" else None, width=W)
    got = ev(x, y, group_sizes=sizes)
    assert got.is_cuda and got.shape == (len(sizes),) and got.dtype == torch.float32 and not got.requires_grad
    got = got.cpu().numpy()
    want = _per_group(kind, W, x, y, sizes)
    bad = [g for g in range(len(sizes)) if got[g:g + 1].tobytes() != want[g]]
    assert not bad, (kind, W, [(g, sizes[g], float(got[g]), float(np.frombuffer(want[g], np.float32)[0])) for g in bad[:8]])
    assert np.isfinite(got).all()
    return x, y, got


# a group of more units than MAX_PARTIALS (its workgroups loop) behind an odd-sized first group (width 3: off the 16-byte grid)
_OVER = -(-(losses.MAX_PARTIALS * losses.CHUNK + 3 * losses.CHUNK + 7) // 3)
CASES = [
    # width 69: every start off the 16-byte grid (69 f floats, f odd sums), one 4096-element chunk straddled (59, 60 frames), three partials (119)
    ("mse", 69, (1, 3, 59, 60, 1, 119)),
    ("mse", 3, (1, 1365, 1366, 2)),                      # 4095 and 4098 elements round the chunk
    ("mse", 3, (1, _OVER, 2)),
    ("bce_logits", 2, (1, 2047, 2048, 2049, 3)),         # 4094, 4096, 4098 elements; odd frames in front: 8 bytes off the grid
    ("window_mse", 3, (60, 61, 239, 240, 241, 721)),     # a unit's 240 frames below, at, above; four units
    ("pose_fk", 144, (1, 15, 16, 17, 53)),               # a unit's 16 frames below, at, above; four units
]


@pytest.mark.parametrize("kind,W,sizes", CASES, ids=[f"{k}-{w}-{len(s)}groups-{sum(s)}" for k, w, s in CASES])
def test_bitwise_the_loss_of_every_group(kind, W, sizes):
    _bitwise(kind, W, sizes, 1000 + W)


def test_many_small_groups_and_one_group_alone():
    """300 groups of 1-3 frames (the bisection of the table walks every way), and one group alone is the loss of the whole batch."""
    g = torch.Generator().manual_seed(5)
    sizes = [int(v) for v in torch.randint(1, 4, (300,), generator=g)]
    assert {1, 2, 3} == set(sizes)
    _bitwise("mse", 69, sizes, 1100)
    _bitwise("bce_logits", 2, sizes, 1101)
    for kind, W, F in (("mse", 69, 130), ("window_mse", 3, 500), ("pose_fk", 144, 37), ("bce_logits", 2, 4100)):
        x, y, got = _bitwise(kind, W, [F], 1200 + W)
        assert got.shape == (1,)


def test_group_rows_over_ragged_lists_equals_group_sizes():
    net = _shared_net()
    lengths = [5, 1, 9, 2, 7, 3, 4]
    xn, yn = _inputs("mse", sum(lengths), 69, 1300)
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn)
    xs, ys = list(torch.split(x, lengths)), list(torch.split(y, lengths))
    ev = losses.SubnetEval(net, "mse", width=69)
    for k in (1, 2, 3, 7, 8):
        sizes = [sum(lengths[i:i + k]) for i in range(0, len(lengths), k)]
        a, b = ev(xs, ys, group_rows=k), ev(x, y, group_sizes=sizes)
        assert a.shape == (len(sizes),) and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), k


# ---- position_error -----------------------------------------------------------------------------------------------------------------------------
def _position_error_f64(x, y, sizes):
    d = np.asarray(x, np.float64).reshape(-1, 3) - np.asarray(y, np.float64).reshape(-1, 3)
    n = np.sqrt((d * d).sum(1))
    W3 = x.shape[1] // 3
    out, at = [], 0
    for s in sizes:
        out.append(float(n[at * W3:(at + s) * W3].mean()))
        at += s
    return np.array(out)


def _position_error_t32(x, y, sizes):
    """The reference's expression in fp32 on the CPU: (p - t).view(-1, 3).norm(dim=1).mean() per group (articulate/evaluator.py:129)."""
    out = []
    for xg, yg in zip(torch.split(torch.from_numpy(x), sizes), torch.split(torch.from_numpy(y), sizes)):
        out.append(float((xg.reshape(-1, 3) - yg.reshape(-1, 3)).norm(dim=1).mean()))
    return np.array(out)


@pytest.mark.parametrize("W", [69, 3])
def test_position_error_against_float64(W):
    """Groups at the edges of the kind's own unit (EVAL_POINTS points): below, at, above; three partials; more units than workgroups
    (W = 3 only: the smallest such group); 1-3 frame groups in between so that every start moves."""
    P, W3 = losses.EVAL_POINTS, W // 3
    frames = lambda points: max(1, -(-points // W3))
    sizes = [1, max(1, (P - 1) // W3), 2, frames(P), frames(P + 1), 3, frames(2 * P + 1)]
    if W == 3:
        sizes += [1, losses.MAX_PARTIALS * P + 3 * P + 5, 2]
    F = sum(sizes)
    x, y = CPU._rand((F, W), 1400 + W), CPU._rand((F, W), 1401 + W)
    ev = losses.SubnetEval(_shared_net(), "position_error", width=W)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    got = ev(xd, yd, group_sizes=sizes).cpu().numpy()
    again = ev(xd, yd, group_sizes=sizes).cpu().numpy()
    assert got.tobytes() == again.tobytes()
    f64, t32 = _position_error_f64(x, y, sizes), _position_error_t32(x, y, sizes)
    for g, s in enumerate(sizes):
        e, et = abs(float(got[g]) - f64[g]), abs(t32[g] - f64[g])
        print(f"RATIO position_error W={W} group {g} frames {s}: f64 {f64[g]:.9e} err_gpu {e:.3e} err_t32 {et:.3e} "
              f"err_gpu/|f64| {e / abs(f64[g]):.2e}")
    for g, s in enumerate(sizes):
        e, et = abs(float(got[g]) - f64[g]), abs(t32[g] - f64[g])
        assert e <= 1e-7 * abs(f64[g]), (W, g, s, e, f64[g])
        assert e <= K_F32 * et + 1e-7 * abs(f64[g]), (W, g, s, e, et)


def test_position_error_of_one_point_is_exact():
    x, y = CPU._rand((1, 3), 1500), CPU._rand((1, 3), 1501)
    d = x.astype(np.float64) - y.astype(np.float64)
    want = np.float32(np.sqrt((d * d).sum()))
    ev = losses.SubnetEval(_shared_net(), "position_error")
    got = ev(torch.from_numpy(x).cuda(), torch.from_numpy(y), group_sizes=[1]).cpu().numpy()
    print(f"RATIO position_error one point: f64 {float(np.sqrt((d * d).sum())):.17e} gpu {float(got[0]):.9e}")
    assert got.tobytes() == want.tobytes()


# ---- reruns, autograd, bad input -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,W,sizes", [c for c in CASES if sum(c[2]) < 10000], ids=lambda v: None)
def test_two_calls_give_the_same_bits_and_nothing_is_differentiable(kind, W, sizes):
    net = _shared_net()
    sizes = list(sizes)
    xn, yn = _inputs(kind, sum(sizes), W, 1600)
    x, y = torch.from_numpy(np.ascontiguousarray(xn)).cuda().requires_grad_(), torch.from_numpy(np.ascontiguousarray(yn)).cuda()
    ev = losses.SubnetEval(net, kind, pos_weight=PW if kind == "bce_logits" else None, width=W)
    a = ev(x, y, group_sizes=sizes)
    other = ev(x.detach()[:sizes[0]], y[:sizes[0]], group_sizes=sizes[:1])           # another table in between
    b = ev(list(torch.split(x, sizes)), y, group_sizes=sizes)                        # ys that require grad, as split views
    assert not a.requires_grad and a.grad_fn is None and not b.requires_grad
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert other.cpu().numpy().tobytes() == a[:1].cpu().numpy().tobytes()


def test_bad_input_raises_before_anything_is_enqueued(monkeypatch):
    net = _shared_net()
    lib, dev = net._lib, net.device
    calls = []
    real = lib.rc_subnet_eval
    monkeypatch.setattr(lib, "rc_subnet_eval", lambda *args: calls.append(1) or real(*args))
    z = lambda F, W, d=dev: torch.zeros(F, W, device=d)
    with pytest.raises(ValueError, match="kind"):
        losses.SubnetEval(net, "l1")
    with pytest.raises(ValueError, match="pos_weight"):
        losses.SubnetEval(net, "position_error", pos_weight=(1.0, 1.0))
    with pytest.raises(ValueError, match="width"):
        losses.SubnetEval(net, "position_error", width=2)
    ev = losses.SubnetEval(net, "window_mse")
    with pytest.raises(ValueError, match="group 1.*60"):
        ev(z(119, 3), z(119, 3), group_sizes=[60, 59])
    ev = losses.SubnetEval(net, "mse", width=69)
    with pytest.raises(ValueError, match="width"):
        ev(z(4, 3), z(4, 3), group_sizes=[4])
    with pytest.raises(ValueError, match="exactly one"):
        ev(z(4, 69), z(4, 69))
    with pytest.raises(ValueError, match="exactly one"):
        ev(z(4, 69), z(4, 69), group_rows=1, group_sizes=[4])
    with pytest.raises(ValueError, match="sum"):
        ev(z(4, 69), z(4, 69), group_sizes=[3])
    with pytest.raises(ValueError, match="group 1"):
        ev(z(4, 69), z(4, 69), group_sizes=[4, 0])
    with pytest.raises(ValueError, match="frames"):
        ev(z(4, 69), z(5, 69), group_sizes=[4])
    with pytest.raises(ValueError):
        ev(z(4, 69, "cpu"), z(4, 69), group_sizes=[4])
    assert not calls
    # the entry itself
    x, y = z(128, 144), z(128, 144)
    v, pw = torch.full((4,), 7.0, device=dev), torch.ones(2, device=dev)
    sp, P = _lib.stream_ptr(), _lib.ptr
    arr = lambda sizes: (C.c_int64 * len(sizes))(*sizes)

    def call(ctx, kind, sizes, W, aux=None, xx=x, yy=y, vv=v, n=None):
        return real(ctx, kind, P(xx), P(yy), len(sizes) if n is None else n, arr(sizes) if sizes is not None else None, W, P(aux), P(vv), sp)

    err = lambda: lib.rc_last_error(net._ctx)
    assert call(None, 0, [4], 69) == -1                                                      # null context
    assert call(net._ctx, 4, [4], 69) == -1 and b"rc_subnet_eval" in err() and b"kind" in err()
    assert call(net._ctx, 15, [4], 69) == -1 and call(net._ctx, 17, [4], 69) == -1 and call(net._ctx, -1, [4], 69) == -1
    assert call(net._ctx, 0, [4], 144) == -1 and b"rc_subnet_eval" in err() and b"width" in err()
    assert call(net._ctx, 1, [4], 3, pw) == -1 and call(net._ctx, 2, [64], 2) == -1 and call(net._ctx, 3, [4], 69) == -1
    assert call(net._ctx, 16, [4], 2) == -1 and call(net._ctx, 16, [4], 0) == -1 and call(net._ctx, 16, [4], 4) == -1
    assert call(net._ctx, 0, [], 69) == -1 and call(net._ctx, 0, [4], 69, n=-2) == -1 and b"groups" in err()
    assert call(net._ctx, 0, [1] * 4, 69, n=losses.EVAL_MAX_GROUPS + 1) == -1 and b"groups" in err()
    assert call(net._ctx, 0, [4, 0, 3], 69) == -1 and b"rc_subnet_eval" in err() and b"group 1" in err()
    assert call(net._ctx, 0, [4, 3, -1], 69) == -1 and b"group 2" in err()
    assert call(net._ctx, 2, [60, 61, 59, 60], 3) == -1 and b"rc_subnet_eval" in err() and b"group 2" in err() and b"60" in err()
    assert call(net._ctx, 1, [4], 2) == -1 and b"pos_weight" in err()                        # bce_logits without pos_weight
    assert call(net._ctx, 0, None, 69, n=1) == -1                                            # null table
    assert call(net._ctx, 0, [4], 69, xx=None) == -1 and call(net._ctx, 0, [4], 69, yy=None) == -1 and call(net._ctx, 0, [4], 69, vv=None) == -1
    off = x.view(-1)[1:]
    assert call(net._ctx, 0, [4], 69, xx=off) == -1 and b"aligned" in err()                  # off the 16-byte grid where pieces are moved
    assert call(net._ctx, 1, [4], 2, pw, yy=off) == -1 and call(net._ctx, 3, [4], 144, yy=off) == -1
    bare = C.c_void_p()
    assert lib.rc_create(1, 0, C.byref(bare)) == 0
    assert call(bare, 3, [4], 144) == -1 and b"body" in lib.rc_last_error(bare)              # pose_fk without a body
    torch.cuda.synchronize()
    assert bool((v == 7.0).all())                                                            # no refused call wrote anything
    assert call(net._ctx, 2, [60], 3, xx=off, yy=off) == 0 and call(net._ctx, 16, [2, 2], 3, xx=off, yy=off) == 0   # any alignment
    assert call(bare, 0, [4, 4], 69) == 0                                                    # (mse needs no body)
    torch.cuda.synchronize()
    assert lib.rc_destroy(bare) == 0
