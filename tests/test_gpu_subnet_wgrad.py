"""The weight gradients of a trainable sub-net on the device (net.trainable(name, weight_grads="device"): rc_subnet_weight_grads, the
reductions over all frames that articulate/utils/torch/train.py:117-122's loss.backward() leaves in the .grad of rnn.py:121-133's
parameters): the entry alone against float64 and exactly on integers, a long reduction in one and in several parts, the site-1 mask
applied while the operand is loaded, the trainer end to end in eval and train mode, determinism, skipped tensors, bad input, and a loop
that learns."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import subnet_backward_f64 as B64
import subnet_dropout_ref as R
import test_gpu_subnet_backward as BWD
import test_gpu_subnet_dropout as DROP
import test_gpu_subnet_forward as FWD
from robustcap_amd import _lib
from robustcap_amd import train
from robustcap_amd.train import param_names

pytestmark = pytest.mark.gpu

SPEC = FWD.SPEC
K_F32 = BWD.K_F32
_net, _inputs, _same = FWD._net, FWD._inputs, FWD._same
RAGGED = (1, 5, 64, 130, 257)                      # 457 frames
LONG = (235,) * 12                                 # 2,820 frames: where sequential fp32 accumulation measured 8.2 times torch's error
SEED = DROP.SEED
NAMES = [k for k in param_names("rnn8")]           # the twelve tensors, the order of the entry's table (no sub-net but rnn2 has more)


def _operands(name, lengths, seed, integers=False):
    """x, acts, init_h, dy, d_gates, d_p of a call as float32 CPU tensors: random normal, or integers in [-4, 4] (every sum exact)."""
    nin, H, nout = SPEC[name]
    F, N = sum(lengths), len(lengths)
    g = torch.Generator().manual_seed(seed)
    if integers:
        draw = lambda *s: torch.randint(-4, 5, s, generator=g).float()
    else:
        draw = lambda *s: torch.randn(*s, generator=g)
    ops = {"x": draw(F, nin), "acts": draw(3, F, H), "init_h": draw(2, N, H), "dy": draw(F, nout), "d_gates": draw(2, F, 4 * H)}
    ops["d_p"] = draw(F, H) * (ops["acts"][0] > 0)                     # already through the relu mask, as the trainer hands it over
    return ops


def _entry(net, name, lengths, ops, init=True, drop=train.NO_DROPOUT, outs=None, skip=()):
    """rc_subnet_weight_grads on device copies of `ops`; returns (rc, {tensor name: device tensor}). outs: tensors to write into
    (default: new ones); skip: names handed over as null."""
    nin, H, nout = SPEC[name]
    dev = net.device
    d = {k: (v if v.is_cuda else v.to(dev)).contiguous() for k, v in ops.items()}
    sd = FWD._sd()
    if outs is None:
        outs = {k: torch.empty(sd[f"{name}.{k}"].shape, device=dev) for k in NAMES}
    table = (C.c_void_p * 12)(*[None if k in skip else outs[k].data_ptr() for k in NAMES])
    lens = (C.c_int32 * len(lengths))(*lengths)
    p = _lib.ptr
    rc = net._lib.rc_subnet_weight_grads(net._ctx, name.encode(), len(lengths), lens, p(d["x"]), p(d["acts"]), p(d["init_h"]) if init else None,
                                         p(d["dy"]), p(d["d_gates"]), p(d["d_p"]), *drop, table, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, outs


def _assemble64(name, lengths, ops, init):
    """tests/subnet_backward_f64.py::assemble on the operands in float64."""
    nin, H, nout = SPEC[name]
    a = {k: v.double().numpy() for k, v in ops.items()}
    h0 = a["init_h"] if init else np.zeros_like(a["init_h"])
    xs = np.split(a["x"], np.cumsum(lengths)[:-1])
    g, _ = B64.assemble({"linear1.weight": np.zeros((H, nin))}, xs, h0, a["acts"], list(lengths), a["dy"], a["d_gates"], a["d_p"])
    return g


def _assemble32(name, lengths, ops, init):
    """The same formulas in fp32 by torch on the CPU, as robustcap_amd/train.py's "torch" path evaluates them."""
    H = SPEC[name][1]
    acts, dG = ops["acts"], ops["d_gates"]
    g = {"linear2.weight": train.frames_t_matmul(ops["dy"], acts[2]), "linear2.bias": ops["dy"].sum(0)}
    for l in (0, 1):
        h_prev = train.shift_within_sequences(acts[l + 1], list(lengths), ops["init_h"][l] if init else None)
        g[f"rnn.weight_ih_l{l}"], g[f"rnn.weight_hh_l{l}"] = train.frames_t_matmul(dG[l], acts[l]), train.frames_t_matmul(dG[l], h_prev)
        g[f"rnn.bias_ih_l{l}"] = g[f"rnn.bias_hh_l{l}"] = dG[l].sum(0)
    g["linear1.weight"], g["linear1.bias"] = train.frames_t_matmul(ops["d_p"], ops["x"]), ops["d_p"].sum(0)
    return {k: v.double().numpy() for k, v in g.items()}


@functools.lru_cache(maxsize=None)
def _case(name, lengths, seed, init):
    """Operands and the two CPU references of a case, computed once and shared by both gemm modes."""
    ops = _operands(name, lengths, seed)
    return ops, _assemble64(name, lengths, ops, init), _assemble32(name, lengths, ops, init)


def _np(outs):
    return {k: v.detach().double().cpu().numpy() for k, v in outs.items()}


# ---- 1: the entry alone against float64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("init", [True, False])
@pytest.mark.parametrize("name", ["rnn8", "rnn3", "rnn7", "rnn2", "rnn6", "rnn4"])
def test_entry_against_float64(name, init, split):
    """Each of the twelve outputs within K_F32 times the error of the same formulas in torch fp32 on the CPU, plus 1e-7 of its scale.
    rnn8 / rnn3 / rnn7: 2, 3 and 144 outputs (dy rows of 8, 12, 576 bytes); rnn2: 72 inputs, 69 outputs; rnn6 / rnn4: H = 1024 / 1280,
    240 / 171 inputs. 457 frames: one 256-frame block and a ragged second one."""
    ops, f64, t32 = _case(name, RAGGED, 50, init)
    rc, outs = _entry(_net(1, split), name, RAGGED, ops, init)
    assert rc == 0
    BWD._check_bound(f"wgrad-{name}-{'init' if init else 'null'}", split, _np(outs), f64, t32)


# ---- 2: exact indexing -----------------------------------------------------------------------------------------------------------------
def _lengths_of(F):
    return (F,) if F < 3 else (1, F - 1) if F <= 33 else (1, 30, F - 31)


EXACT = [("rnn8", _lengths_of(F)) for F in (1, 31, 32, 33, 255, 256, 257)] + [("rnn8", (1,) * 70), ("rnn8", (40,)), ("rnn4", RAGGED),
                                                                              ("rnn7", RAGGED)]


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("name,lengths", EXACT, ids=[f"{n}-{len(l)}x{sum(l)}" for n, l in EXACT])
def test_exact_on_integers(name, lengths, split):
    """Operands in [-4, 4]: every product and sum is exact in both modes (three bf16 terms hold an integer whole), so the outputs EQUAL
    numpy's -- the shift, the init_h rows (70 sequences of one frame: every h_prev row is one, across the 64-row edge), the column
    order and the tile edges, free of rounding."""
    ops = _operands(name, lengths, 51, integers=True)
    want = _assemble64(name, lengths, ops, True)
    rc, outs = _entry(_net(1, split), name, lengths, ops, True)
    assert rc == 0
    got = _np(outs)
    for k in NAMES:
        assert np.array_equal(got[k], want[k]), (name, lengths, k, float(np.abs(got[k] - want[k]).max()))
    rc, outs = _entry(_net(1, split), name, lengths, ops, False)       # null init_h: zeros at every first frame
    want = _assemble64(name, lengths, ops, False)
    assert rc == 0 and all(np.array_equal(_np(outs)[k], want[k]) for k in NAMES)


# ---- 3: a long reduction ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("parts", [0, 1, 16])
def test_long_reduction(parts, split):
    """2,820 frames = 12 blocks of 256. parts 0: from the tile count (rnn8's LSTM launches have 16 x 8 tiles: 2 parts on a device of
    256 compute units; its dense launches 12, its bias sums 6 or 12); 1: one workgroup per tile sums all twelve blocks; 16: one block per
    part. The bound of test 1 holds for each."""
    ops, f64, t32 = _case("rnn8", LONG, 52, True)
    net = _net(1, split)
    assert net._lib.rc_set_subnet_wgrad_parts(net._ctx, parts) == 0
    rc, outs = _entry(net, "rnn8", LONG, ops, True)
    assert rc == 0
    BWD._check_bound(f"wgrad-long-parts{parts}", split, _np(outs), f64, t32)
    assert net._lib.rc_set_subnet_wgrad_parts(net._ctx, 17) != 0 and net._lib.rc_set_subnet_wgrad_parts(net._ctx, -1) != 0


# ---- 4: the site-1 mask, applied while the operand is loaded -----------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("p", [0.4, 0.1])
def test_mask_fusion(p, split):
    """weight_ih_l1 with (p, seed, call) on the raw acts[1] is bitwise the entry at p = 0 on rc_dropout_apply(acts[1], site 1); the other
    eleven outputs are bitwise their p = 0 values."""
    p = np.float32(p).item()
    net = _net(1, split)
    ops = _operands("rnn8", RAGGED, 53)
    drop = (p, SEED, 3000000001)
    rc, fused = _entry(net, "rnn8", RAGGED, ops, True, drop)
    assert rc == 0
    rc, plain = _entry(net, "rnn8", RAGGED, ops, True)
    assert rc == 0
    masked = dict(ops)
    acts = ops["acts"].to(net.device).clone()
    acts[1] = DROP._apply(net, acts[1].contiguous(), 1, *drop)
    assert not _same(acts[1], ops["acts"][1])
    masked["acts"] = acts
    rc, ref = _entry(net, "rnn8", RAGGED, masked, True)
    assert rc == 0
    assert _same(fused["rnn.weight_ih_l1"], ref["rnn.weight_ih_l1"]) and not _same(fused["rnn.weight_ih_l1"], plain["rnn.weight_ih_l1"])
    for k in NAMES:
        if k != "rnn.weight_ih_l1":
            assert _same(fused[k], plain[k]), k
    # ... and the mask is the numpy restatement's (tests/subnet_dropout_ref.py), applied on the CPU
    F, H = sum(RAGGED), SPEC["rnn8"][1]
    m = R.scaled_mask(F, H, 1, p, SEED, drop[2])
    cpu = dict(ops)
    cpu["acts"] = ops["acts"].clone()
    cpu["acts"][1] = torch.from_numpy(np.where(m != 0, ops["acts"][1].numpy() * R.scale(p), np.float32(0.0)).astype(np.float32))
    rc, ref2 = _entry(net, "rnn8", RAGGED, cpu, True)
    assert rc == 0 and _same(fused["rnn.weight_ih_l1"], ref2["rnn.weight_ih_l1"])


# ---- 5: end to end ---------------------------------------------------------------------------------------------------------------------
class _DeviceNet:
    """`net` whose trainable() hands out trainers with weight_grads="device" (for the helpers that call net.trainable(name))."""

    def __init__(self, net):
        self._net = net

    def trainable(self, name):
        return self._net.trainable(name, weight_grads="device")

    def __getattr__(self, k):
        return getattr(self._net, k)


EVAL = {"rnn8-ragged": ("rnn8", RAGGED, 4, False), "rnn4-ragged": ("rnn4", (1, 5, 33, 70), 4, False), "rnn2-init_net": ("rnn2", (3, 40, 17), 6, True),
        "rnn3-65x3": ("rnn3", (3,) * 65, 4, False)}


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("case", sorted(EVAL))
def test_trainer_against_float64(case, split):
    """weight_grads="device": every quantity within _check_bound of torch's float64 autograd; dx and d init (they do not pass through the
    new code) bitwise the "torch" trainer's, like y and the final state."""
    name, lengths, seed, with_v = EVAL[case]
    xs, init, cot, v, f64, t32 = BWD._case(name, tuple(lengths), seed, with_v)
    net = _net(1, split)
    got = BWD._gpu_grads(_DeviceNet(net), name, xs, init, cot, v)
    BWD._check_bound(f"wgrad-e2e-{case}", split, got, f64, t32)
    ref = BWD._gpu_grads(net, name, xs, init, cot, v)
    for k in ref:
        if not any(k.startswith(q) for q in ("rnn.", "linear1.", "linear2.")):
            assert np.array_equal(got[k], ref[k]), k                   # dx, d init, d x_init and init_net's gradients
    td, tt = net.trainable(name, weight_grads="device"), net.trainable(name)
    arg = [(x, v[i]) for i, x in enumerate(xs)] if with_v else xs
    (yd, (hd, cd)), (yt, (ht, ct)) = td(arg, init, return_state=True), tt(arg, init, return_state=True)
    assert all(_same(a.detach(), b.detach()) for a, b in zip(yd, yt)) and _same(hd.detach(), ht.detach()) and _same(cd.detach(), ct.detach())


def _as_np(q):
    return {k: g.detach().double().cpu().numpy() for k, g in q.items()}


@pytest.mark.parametrize("split", [False, True])
def test_trainer_against_float64_across_a_chunk_boundary(split):
    """The two-chunk shape of the existing chunk tests (31,300 frames: 123 blocks of 256, cut into parts) in eval mode, against the
    restatement in float64 and float32 as torch matmuls on the device (p = 0: its masks are ones)."""
    name, lengths, seed = "rnn3", DROP.TWO_CHUNKS, 22
    xs, cot, init, _ = DROP._inputs_of(name, lengths, seed, False)
    f64, t32 = (DROP._restated(name, lengths, xs, init, None, cot, 0.0, 0, 0, dt, "cuda") for dt in (torch.float64, torch.float32))
    net = _net(1, split)
    c0 = net.subnet_stats()[2]
    got = DROP._run(net.trainable(name, weight_grads="device"), xs, init, cot)
    assert net.subnet_stats()[2] - c0 == 4                                     # two chunks forward, two backward
    BWD._check_bound("wgrad-e2e-two-chunks", split, _as_np(got), f64, t32)
    ref = DROP._run(net.trainable(name), xs, init, cot)
    for k in ("y", "h_n", "c_n", "dx", "d init_h", "d init_c"):
        assert _same(got[k], ref[k]), k


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("case", ["rnn8-ragged", "rnn4-ragged", "rnn7-p0.1", "rnn2-init_net"])
def test_trainer_in_train_mode_against_float64(case, split):
    """Train mode at the sub-net's rate (0.4; rnn7: 0.1) against the dropout restatement handed the same masks: the site-1 mask of
    dW_ih_l1's input is the kernel's own here."""
    name, lengths, with_v = DROP.CASES[case]
    f64, t32 = DROP._references(name, lengths, 20, with_v, "cpu")
    got = DROP._trained(_DeviceNet(_net(1, split)), name, lengths, 20, with_v)
    BWD._check_bound(f"wgrad-e2e-train-{case}", split, got, f64, t32)


# ---- 6: determinism ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
def test_determinism(split):
    """Two calls give the same bits, also after a larger call (more frames, more parts, another sub-net) has left other values in the
    partial-sum scratch."""
    net = _net(1, split)
    ops = _operands("rnn8", LONG, 54)
    _, a = _entry(net, "rnn8", LONG, ops, True, (0.4, SEED, 5))
    _, b = _entry(net, "rnn8", LONG, ops, True, (0.4, SEED, 5))
    big = (300,) * 14
    rc, _ = _entry(net, "rnn3", big, _operands("rnn3", big, 55), True)
    assert rc == 0
    _, c = _entry(net, "rnn8", LONG, ops, True, (0.4, SEED, 5))
    for k in NAMES:
        assert _same(a[k], b[k]) and _same(a[k], c[k]), k


# ---- 7: skipped tensors and bad input ----------------------------------------------------------------------------------------------------
def test_skipped_tensors_and_bad_input():
    net = _net()
    name, lengths = "rnn8", RAGGED
    ops = _operands(name, lengths, 56)
    rc, full = _entry(net, name, lengths, ops, True)
    assert rc == 0
    sentinel = lambda: {k: torch.full_like(full[k], 7.0) for k in NAMES}
    for skip in (("rnn.weight_hh_l0", "rnn.bias_ih_l0", "linear1.weight", "linear2.bias"), ("rnn.weight_ih_l1", "rnn.bias_hh_l1"),
                 ("linear1.weight", "linear1.bias"), tuple(NAMES)):
        rc, outs = _entry(net, name, lengths, ops, True, outs=sentinel(), skip=skip)
        assert rc == 0
        for k in NAMES:
            if k in skip:
                assert bool((outs[k] == 7.0).all()), k                 # nothing written
            else:
                assert _same(outs[k], full[k]), k                      # ... and no other tensor changed
    # bad input: an error code, nothing written
    lib, ctx, dev = net._lib, net._ctx, net.device
    d = {k: v.to(dev) for k, v in ops.items()}
    outs = sentinel()
    table = (C.c_void_p * 12)(*[outs[k].data_ptr() for k in NAMES])
    lens = (C.c_int32 * len(lengths))(*lengths)
    p, sp = _lib.ptr, _lib.stream_ptr()
    good = [ctx, name.encode(), len(lengths), lens, p(d["x"]), p(d["acts"]), p(d["init_h"]), p(d["dy"]), p(d["d_gates"]), p(d["d_p"]), 0.0, 0, 0,
            table, sp]

    def call(**change):
        a = list(good)
        for i, v in change.items():
            a[int(i[1:])] = v
        return lib.rc_subnet_weight_grads(*a)

    assert call(_1=b"rnn9") != 0 and b"rc_subnet_weight_grads" in lib.rc_last_error(ctx)
    assert call(_2=0) != 0 and call(_2=-1) != 0
    for i in (3, 4, 5, 7, 8, 9, 13):                                   # lengths, x, acts, dy, d_gates, d_p, the table
        assert call(**{f"_{i}": None}) != 0, i
    assert call(_10=1.0) != 0 and call(_10=-0.1) != 0                  # p outside [0, 1)
    assert call(_0=None) != 0
    small = torch.zeros(16, device=dev)
    assert call(_8=p(small)) != 0 and call(_5=p(small)) != 0           # an operand whose allocation ends before the call's extent
    bad_table = (C.c_void_p * 12)(*[small.data_ptr() if k == "rnn.weight_hh_l1" else outs[k].data_ptr() for k in NAMES])
    assert call(_13=bad_table) != 0
    zero_len = (C.c_int32 * len(lengths))(*([0] + list(lengths[1:])))
    assert call(_3=zero_len) != 0
    torch.cuda.synchronize()
    assert all(bool((outs[k] == 7.0).all()) for k in NAMES) and bool((small == 0).all())
    # the Python surface
    assert net.trainable(name).weight_grads == "torch"
    with pytest.raises(ValueError):
        net.trainable(name, weight_grads="cuda")
    tr = net.trainable(name, weight_grads="device")
    assert tr.weight_grads == "device"
    with pytest.raises(ValueError):
        tr.weight_grads = "cuda"
    tr.weight_grads = "torch"
    assert tr.weight_grads == "torch"


# ---- 8: a loop that learns ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
def test_a_training_loop_learns(split):
    lengths = (20, 7, 13, 20, 1, 16, 9, 20)
    xs = _inputs("rnn8", lengths, 40)
    net = _net(1, split)
    target = 0.1 * torch.randn(sum(lengths), SPEC["rnn8"][2], generator=torch.Generator().manual_seed(41)).to(net.device)
    tr = net.trainable("rnn8", weight_grads="device")
    tr.manual_seed(42)
    opt = tr.optimizer(lr=1e-3, clip_grad_norm=1.0)

    def eval_loss():
        tr.eval()
        with torch.no_grad():
            return float(torch.nn.functional.mse_loss(torch.cat(tr(xs)), target))

    before = eval_loss()
    for _ in range(20):
        tr.train()
        loss = torch.nn.functional.mse_loss(torch.cat(tr(xs)), target)
        opt.zero_grad()
        loss.backward()
        opt.step()
    after = eval_loss()
    print(f"EVAL LOSS rnn8 mode={int(split)} weight_grads=device: {before:.5f} -> {after:.5f} after 20 train-mode iterations")
    assert after < before
