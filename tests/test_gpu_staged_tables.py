"""Every entry that builds a table on the host and sends it to the device on the caller's stream (csrc/rc_internal.h: StagedTable), driven
through more than one lap of its ring of pinned copies while its device table grows and is reused shrunken: nine calls on one stream with
no host synchronisation between them, their tables sized by SIZES (the capacity doubles: the device table grows at calls 1, 2, 4 and 7),
every call writing into buffers of its own. After ONE synchronise every output is bitwise what a fresh context gives for the same calls
made alone, each followed by a synchronise. No tolerance is involved.

The Python surfaces used here neither read back nor synchronise (their inputs are on the device before the first call); rc_sequence_rows
goes through the C entry, which takes output buffers of the test's own (a sentinel past a row's end). rc_sequence_rows carries the rows' state from call to call, so its fresh
context makes the same nine calls too, one at a time; its table length is the batch, so the lengths vary instead (T <= 4 at batch 8)."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import motion_metrics_f64 as M
import subnet_batches_ref as R
import test_gpu_sequence_rows as ROWS
import test_gpu_subnet_batches as B
import test_gpu_subnet_forward as FWD
from robustcap_amd import _lib, body as body_mod, corpus, losses, preprocess, synth
from robustcap_amd import config as cfg

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 2, 9, 1, 5, 40, 2, 4)                 # groups, samples or sequences of call k
SEED = B.SEED
t = torch.from_numpy


def _bits(x):
    return x.detach().contiguous().view(-1).view(torch.int32)


def _drive(make, call):
    """make() -> what a context needs (made twice); call(made, k) -> the output tensors of call k, enqueued on the current stream."""
    busy = make()
    torch.cuda.synchronize()
    got = [call(busy, k) for k in range(len(SIZES))]               # in flight together: two laps of a ring of four plus one
    torch.cuda.synchronize()
    alone = make()
    for k in range(len(SIZES)):
        want = call(alone, k)
        torch.cuda.synchronize()
        assert len(want) == len(got[k]) > 0
        for i, (a, b) in enumerate(zip(got[k], want)):
            assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), (k, SIZES[k], i)
    del busy, alone, got
    gc.collect()
    torch.cuda.synchronize()


def _frames(k, lo, hi):
    """frames of every group / sample / sequence of call k, in lo .. hi"""
    return [lo + (g + k) % (hi - lo + 1) for g in range(SIZES[k])]


def test_subnet_eval():
    sizes = [_frames(k, 1, 4) for k in range(len(SIZES))]
    g = torch.Generator().manual_seed(11)
    xy = [(torch.randn(sum(s), 3, generator=g).cuda(), torch.randn(sum(s), 3, generator=g).cuda()) for s in sizes]

    def make():
        return losses.SubnetEval(FWD._net(1), "mse", width=3)

    _drive(make, lambda ev, k: (ev(xy[k][0], xy[k][1], group_sizes=sizes[k]),))


def test_motion_metrics_no_mesh():
    sizes = [_frames(k, 3, 5) for k in range(len(SIZES))]
    ins = []
    for k, s in enumerate(sizes):
        parts = [M.motion_pair(100 * k + i, N) for i, N in enumerate(s)]
        ins.append([t(np.ascontiguousarray(np.concatenate([p[q] for p in parts]))).cuda() for q in range(4)])
    body = synth.make_body(1)

    def call(model, k):
        pp, pt, tp, tt = ins[k]
        return model.motion_metrics(pp, pt, tp, tt, group_frames=sizes[k], mesh=False)

    _drive(lambda: body_mod.ParametricModel(body=body), call)


def test_prepare_motions():
    sizes = [_frames(k, 3, 5) for k in range(len(SIZES))]
    g = torch.Generator().manual_seed(12)
    ins = [((0.3 * torch.randn(sum(s), 72, generator=g)).cuda(), torch.randn(sum(s), 3, generator=g).cuda()) for s in sizes]
    body = synth.make_body(1)

    def make():
        model = body_mod.ParametricModel(body=body)
        model._ensure_shape_space(cfg.mp_mask, cfg.vi_mask)         # (what the first prepare_motions would do, in front of the nine calls)
        return model

    def call(model, k):
        p = preprocess.prepare_motions(model, ins[k][0], ins[k][1], smooth_n=1, lengths=sizes[k])
        assert p.lengths == sizes[k]
        return list(p.fields.values()) + [p.vert6, p.rest_joint]

    _drive(make, call)


def _batch_parts(net, name):
    """(plain part, world part) of rnn4 / rnn6 on `net`: samples of 2 .. 3 frames, a pool of 8 rows"""
    tr = net.trainable(name)
    W, Wl = R.WIDTHS[name]
    rng = np.random.default_rng(93)
    pl, wl = (2, 3, 3, 2, 3), (3, 2, 3)
    d, l = rng.normal(size=(sum(pl), W)).astype(np.float32), rng.normal(size=(sum(pl), Wl)).astype(np.float32)
    plain = tr.dataset(B._seqs(d, pl), B._seqs(l, pl))
    wd, wlab = R.world_corpus(91, wl)
    world = tr.dataset(B._seqs(wd, wl), B._seqs(wlab, wl), kind="world", conf_pool=t(R.conf_pool(92, 8)))
    return tr, plain, world


def _batches(pick):
    def make():
        ds = pick(FWD._net(1))
        ds.set_state({"seed": SEED, "call": 3000000001})           # call k of either context draws with the same counter
        return ds

    def call(ds, k):
        xs, labels = ds.batch([(7 * i + k) % len(ds) for i in range(SIZES[k])])
        return xs + labels

    _drive(make, call)


def test_subnet_batch():
    _batches(lambda net: _batch_parts(net, "rnn6")[2])              # kind world: the camera scratch grows beside the table


def test_subnet_batch_parts():
    def pick(net):
        tr, plain, world = _batch_parts(net, "rnn4")
        return tr.concat([plain, world])
    _batches(pick)


def test_subnet_corpus():
    lengths = [3 + i % 2 for i in range(max(SIZES))]
    aist, _ = synth.make_training_dicts(6, lengths, synth.make_body(1), 1)

    def make():
        tr = FWD._net(1).trainable("rnn3")
        ps = []
        for k, n in enumerate(SIZES):
            at = min(k, len(lengths) - n)
            ps.append(corpus.prepare(tr, "aist", {key: v[at:at + n] for key, v in aist.items()}))
        return ps

    def call(ps, k):
        p = ps[k]
        x = torch.empty(p.rows, p.widths[0], device=p.net.device)
        y = torch.empty(p.rows, p.widths[1], device=p.net.device)
        assert p.call(x, y) == 0 and len(p.lengths) == SIZES[k]
        return x, y

    _drive(make, call)


def test_subnet_forward():
    lengths = [_frames(k, 3, 5) for k in range(len(SIZES))]
    xs = [[x.cuda() for x in FWD._inputs("rnn3", s, 20 + k)] for k, s in enumerate(lengths)]
    _drive(lambda: FWD._net(1), lambda net, k: net.rnn3(xs[k]))


def test_sequence_rows(synth_assets):
    Bn, Ts = 8, (1, 3, 2, 4, 1, 4, 3, 2, 4)
    lens = [[(b + k) % (T + 1) for b in range(Bn)] for k, T in enumerate(Ts)]
    m = ROWS._motion(synth_assets, Bn, sum(Ts), [sum(Ts)] * Bn)
    at = np.concatenate([[0], np.cumsum(Ts)])
    ins = [ROWS._dev(m, int(at[k]), int(at[k + 1])) for k in range(len(Ts))]

    def make():
        net = ROWS._net(synth_assets, Bn, 0, 1)
        net.gravityc = t(m["gravityc"])
        net._sync_gravity()
        return net

    def call(net, k):
        T = Ts[k]
        j, a, o = ins[k]
        pose = torch.full((Bn, T, 24, 3, 3), ROWS.SENTINEL, device="cuda")
        tran = torch.full((Bn, T, 3), ROWS.SENTINEL, device="cuda")
        ln = np.ascontiguousarray(np.asarray(lens[k], np.int32))
        rc = net._lib.rc_sequence_rows(net._ctx, T, ln.ctypes.data_as(C.c_void_p), _lib.ptr(j), T * 99, _lib.ptr(a), T * 18, _lib.ptr(o), T * 54,
                                       None, _lib.RC_FLAG_FIRST_FRAME if k == 0 else 0, _lib.ptr(pose), T * 216, _lib.ptr(tran), T * 3,
                                       _lib.stream_ptr())
        _lib.check(net._ctx, rc, "rc_sequence_rows")
        return pose, tran

    _drive(make, call)
