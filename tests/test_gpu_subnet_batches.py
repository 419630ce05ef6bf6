"""The batches of a sub-net's training on the device (tr.dataset(...).batch(...): rc_subnet_batch, csrc/rc_augment.hip; the
DataLoader + RNNDataset.__getitem__ + augment_fn of articulate/utils/torch/rnn.py:64-67 and net/sig_mp.py:360-363, 520-552, 578-581,
649-679, 701-703, 792-795) against the numpy restatement tests/subnet_batches_ref.py: the draws, what is copied bit for bit, the
independence of a draw from the other samples, the ``world`` samples within K = 8 times the float32 restatement's own error of the
float64 one (+ 1e-7 of the quantity's scale; the bound of test_gpu_subnet_loss.py and test_gpu_subnet_dropout.py) with the confidence
rows exact, the gather, a loop that learns, and bad input.

Observed on MI355X (profiles/subnet_batches_ratios.txt): the RATIO lines each accuracy test prints before it asserts."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import subnet_batches_ref as R
import test_gpu_subnet_forward as FWD
from robustcap_amd import _lib, losses

pytestmark = pytest.mark.gpu

_same = FWD._same
SEED = (0x9E3779B9 << 32) | 0x1234ABCD               # both halves of the key in use
K_F32 = 8.0


@functools.lru_cache(maxsize=None)
def _net(split=None):
    return FWD._net(1, split)


def _tr(name, split=None):
    return _net(split).trainable(name)


def _seqs(a, lengths):
    return list(torch.split(torch.from_numpy(np.ascontiguousarray(a)), list(lengths)))


def _plain_ds(name, lengths, seed, zero=False, split_size=-1):
    W, Wl = R.WIDTHS[name]
    g = np.random.default_rng(seed)
    F = sum(lengths)
    d = np.zeros((F, W), np.float32) if zero else g.normal(size=(F, W)).astype(np.float32)
    l = g.normal(size=(F, Wl)).astype(np.float32)
    ds = _tr(name).dataset(_seqs(d, lengths), _seqs(l, lengths), split_size=split_size)
    return ds, d, l


def _np(ts):
    return torch.cat([t for t in ts]).cpu().numpy()


def _check(label, got, f64, f32):
    ratio = R.bound_ratio(got, f64, f32, K_F32)
    print(f"RATIO {label}: {ratio:.4f} of the bound (max |f64| {np.abs(f64).max():.3e}, float32 restatement's error "
          f"{np.abs(np.asarray(f32, np.float64) - f64).max():.3e})")
    return ratio


# ---- 1: the draws, and what is copied ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lengths", [("rnn7", (1,)), ("rnn3", (1, 5, 64)), ("rnn6", (257,))])
def test_plain_draws_and_copies(name, lengths):
    W, Wl = R.WIDTHS[name]
    ds, d, l = _plain_ds(name, lengths, 3, zero=True)
    ds.set_state({"seed": SEED, "call": 3000000001})
    xs, labels = ds.batch(range(len(lengths)))
    assert [tuple(t.shape) for t in xs] == [(T, W) for T in lengths] and [tuple(t.shape) for t in labels] == [(T, Wl) for T in lengths]
    worst = 0.0
    for i, (x, T) in enumerate(zip(xs, lengths)):
        nz64, c0 = R.plain_noise(name, T, i, SEED, 3000000001)
        nz32, _ = R.plain_noise(name, T, i, SEED, 3000000001, np.float32)
        x = x.cpu().numpy()
        assert c0 == (171 if name == "rnn6" else W - nz64.shape[1]) and not x[:, :c0].view(np.int32).any()      # bitwise +0
        worst = max(worst, _check(f"plain {name} sample {i} of {lengths} sigma z", x[:, c0:], nz64, nz32))
    assert worst <= 1.0
    assert _same(torch.cat(labels), torch.from_numpy(l)) and not ds.data.cpu().numpy().view(np.int32).any()
    # a random corpus: the untouched columns and the labels are the corpus, the corpus is unchanged, the noisy columns are x + sigma z
    ds, d, l = _plain_ds(name, lengths, 4)
    ds.set_state({"seed": SEED, "call": 7})
    xs, labels = ds.batch(range(len(lengths)))
    x = _np(xs)
    c0 = R.plain_noise(name, 1, 0, SEED, 7)[1]
    assert np.array_equal(x[:, :c0].view(np.int32), d[:, :c0].view(np.int32)) and _same(torch.cat(labels), torch.from_numpy(l))
    assert _same(ds.data, torch.from_numpy(d)) and _same(ds.label, torch.from_numpy(l))
    at = 0
    for i, T in enumerate(lengths):
        want64, want32 = (R.plain_sample(name, d[at:at + T], i, SEED, 7, f)[:, c0:] for f in (np.float64, np.float32))
        assert _check(f"plain {name} sample {i} x + sigma z", x[at:at + T, c0:], want64, want32) <= 1.0
        at += T


# ---- 2: a draw depends on its own sample only ---------------------------------------------------------------------------------------
def test_draws_do_not_depend_on_the_other_samples():
    name = "rnn8"
    a, da, _ = _plain_ds(name, (1, 200, 7), 10)
    b, db, _ = _plain_ds(name, (5, 200, 7), 11)
    db[5:] = da[1:]
    b = _tr(name).dataset(_seqs(db, (5, 200, 7)), _seqs(np.zeros((212, 2), np.float32), (5, 200, 7)))
    a.manual_seed(SEED), b.manual_seed(SEED)
    xa, _ = a.batch([0, 1, 2])
    xb, _ = b.batch([0, 1, 2])
    assert _same(xa[1], xb[1]) and _same(xa[2], xb[2]) and not _same(xa[0], xb[0][:1])
    assert a.state() == {"seed": SEED, "call": 1}
    a.set_state({"seed": SEED, "call": 0})
    again, _ = a.batch([0, 1, 2])
    assert all(_same(p, q) for p, q in zip(xa, again))                                 # a restored state: the same bits
    nxt, _ = a.batch([0, 1, 2])
    assert not _same(nxt[1], xa[1]) and a.state()["call"] == 2                         # the next call differs
    a.set_state({"seed": SEED ^ (1 << 40), "call": 0})
    assert not _same(a.batch([0, 1, 2])[0][1], xa[1])                                  # the key's high half counts
    # world: the same with the camera, the translation, the pool rows and both noises
    pool = R.conf_pool(12, 256)
    d1, l1 = R.world_corpus(13, (1, 200, 7))
    d2, l2 = R.world_corpus(14, (5, 200, 7))
    d2[5:], l2[5:] = d1[1:], l1[1:]
    for net in ("rnn4", "rnn6"):
        w1 = _tr(net).dataset(_seqs(d1, (1, 200, 7)), _seqs(l1, (1, 200, 7)), kind="world", conf_pool=torch.from_numpy(pool)).manual_seed(SEED)
        w2 = _tr(net).dataset(_seqs(d2, (5, 200, 7)), _seqs(l2, (5, 200, 7)), kind="world", conf_pool=torch.from_numpy(pool)).manual_seed(SEED)
        (x1, y1), (x2, y2) = w1.batch([0, 1, 2]), w2.batch([0, 1, 2])
        assert all(_same(x1[i], x2[i]) and _same(y1[i], y2[i]) for i in (1, 2)) and not _same(x1[0], x2[0][:1])
        w1.manual_seed(SEED)
        x3, y3 = w1.batch([0, 1, 2])
        assert all(_same(p, q) for p, q in zip(x1 + y1, x3 + y3))


# ---- 3: the world samples against float64 ------------------------------------------------------------------------------------------
def _lowest_joint_corpus(name, where):
    """Three frames whose lowest joint in the camera of sample 0 (SEED, call 5) is joint 23 of frame 2 (``last``) or joint 0 of frame 0."""
    d, l = R.world_corpus(30, (3,), box=0.45)
    Rcw = R.world_draws(name, 3, 64, 0, SEED, 5)["Rcw"].astype(np.float64)
    f, j = (2, 23) if where == "last" else (0, 0)
    l = l.reshape(3, 24, 3)
    l[f, j] = (Rcw.T @ np.array([0.0, 0.0, -0.9])).astype(np.float32)                  # camera z -0.9, every other joint above -0.78
    assert np.argmin((l.reshape(-1, 3).astype(np.float64) @ Rcw.T)[:, 2]) == f * 24 + j
    return d, l.reshape(3, 72)


WORLD_CASES = {"one frame": (1,), "ragged": (1, 2, 200), "65 samples": (3,) * 65, "lowest joint last": "last", "lowest joint first": "first"}


@pytest.mark.parametrize("case", list(WORLD_CASES))
@pytest.mark.parametrize("name", ["rnn4", "rnn6"])
def test_world_against_float64(name, case):
    lengths = WORLD_CASES[case]
    if isinstance(lengths, str):
        d, l = _lowest_joint_corpus(name, lengths)
        lengths = (3,)
    else:
        d, l = R.world_corpus(31 + len(lengths), lengths)
    P = 256
    pool = R.conf_pool(32, P)
    ds = _tr(name).dataset(_seqs(d, lengths), _seqs(l, lengths), kind="world", conf_pool=torch.from_numpy(pool))
    ds.set_state({"seed": SEED, "call": 5})
    xs, labels = ds.batch(range(len(lengths)))
    assert _same(ds.data, torch.from_numpy(d)) and _same(ds.label, torch.from_numpy(l)) and _same(ds.pool, torch.from_numpy(pool))
    worst = {}
    at = 0
    for i, T in enumerate(lengths):
        f64 = R.world_sample(name, d[at:at + T], l[at:at + T], pool, i, SEED, 5)
        f32 = R.world_sample(name, d[at:at + T], l[at:at + T], pool, i, SEED, 5, np.float32)
        x, y = xs[i].cpu().numpy(), labels[i].cpu().numpy()
        kp = x[:, 72:171].reshape(T, 33, 3)
        got = {"accc": x[:, :18], "oric": x[:, 18:72], "xy": kp[..., :2].reshape(T, 66), "label": y}
        if name == "rnn6":
            got["tail"] = x[:, 171:]
        assert np.array_equal(kp[..., 2].view(np.int32), pool[R.perm(i, np.arange(T), P, SEED, 5)].view(np.int32)), (case, i)   # bitwise the pool rows
        for k, v in got.items():
            worst[k] = max(worst.get(k, 0.0), R.bound_ratio(v, f64[k], f32[k], K_F32))
        at += T
    for k, v in worst.items():
        print(f"RATIO world {name} {case} {k}: {v:.4f} of the bound")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("P,T", [(200, 200), (201, 200), (1000, 200), (1, 1), (3, 2)])
def test_world_pool_rows_are_the_permutation(P, T):
    pool = R.conf_pool(40, P, distinct=True)
    d, l = R.world_corpus(41, (T, T))
    for name in ("rnn4", "rnn6"):
        ds = _tr(name).dataset(_seqs(d, (T, T)), _seqs(l, (T, T)), kind="world", conf_pool=torch.from_numpy(pool)[..., None])   # [P, 33, 1], as syn_c.pt
        ds.set_state({"seed": SEED, "call": 2})
        xs, _ = ds.batch([1, 0])
        for i in (0, 1):
            conf = xs[i].cpu().numpy()[:, 72:171].reshape(T, 33, 3)[..., 2]
            rows = np.rint(conf[:, 0].astype(np.float64) * P - 0.5).astype(np.int64)
            assert np.array_equal(rows, R.perm(i, np.arange(T), P, SEED, 2)) and len(set(rows.tolist())) == T
            assert np.array_equal(conf.view(np.int32), pool[rows].view(np.int32))


# ---- 4: the gather -----------------------------------------------------------------------------------------------------------------
def test_gather_is_the_same_call_on_a_gathered_copy():
    lengths = (401, 200, 1)
    for name in ("rnn3", "rnn2"):
        ds, d, l = _plain_ds(name, lengths, 50, split_size=200)
        table = R.split_table(lengths, 200)
        assert len(ds) == 5 and ds.samples == table
        idx = [3, 0, 4, 2, 0, 1]                                                       # a shuffle with one repeat
        ds.manual_seed(SEED)
        xs, labels = ds.batch(idx)
        pieces = [(d[a:a + n], l[a:a + n]) for a, n in (table[i] for i in idx)]
        copy = _tr(name).dataset([torch.from_numpy(p[0].copy()) for p in pieces], [torch.from_numpy(p[1].copy()) for p in pieces])
        copy.manual_seed(SEED)
        xc, lc = copy.batch(range(len(idx)))
        first = (lambda t: t[0]) if name == "rnn2" else (lambda t: t)
        assert all(_same(first(p), first(q)) for p, q in zip(xs, xc)) and all(_same(p, q) for p, q in zip(labels, lc))
        plain_x, plain_l = ds.batch(idx, augment=False)
        assert ds.state() == {"seed": SEED, "call": 1}                                 # augment=False draws nothing
        assert all(_same(first(p), torch.from_numpy(q[0])) and _same(r, torch.from_numpy(q[1])) for p, r, q in zip(plain_x, plain_l, pieces))
        if name == "rnn2":                                                             # RNNWithInitDataset: (x_i, label_i[0]); no augmentation
            assert all(isinstance(p, tuple) and _same(p[1], torch.from_numpy(q[1][0])) and tuple(p[1].shape) == (69,) for p, q in zip(xs, pieces))
            assert all(_same(p[0], torch.from_numpy(q[0])) for p, q in zip(xs, pieces))
            ys = _tr(name)(xs)
            assert [tuple(y.shape) for y in ys] == [(q[0].shape[0], 69) for q in pieces]
        else:
            assert not _same(xs[0], plain_x[0]) and _same(xs[0][:, :72], plain_x[0][:, :72])
    pw = losses.pos_weight_from_labels(ds)                                             # a dataset stands for its label buffer
    assert _same(pw, losses.pos_weight_from_labels(ds.label)) and pw.is_cuda


# ---- 5: end to end -----------------------------------------------------------------------------------------------------------------
def _loop(tr, ds, eval_batch, n_iter=20):
    loss_fn = tr.loss(losses.pos_weight_from_labels(ds)) if tr.name == "rnn8" else tr.loss()
    opt = tr.optimizer(lr=1e-3, clip_grad_norm=1.0)

    def eval_loss():
        tr.eval()
        with torch.no_grad():
            return float(loss_fn(tr(eval_batch[0]), eval_batch[1]))

    before = eval_loss()
    g = torch.Generator().manual_seed(1)
    for _ in range(n_iter):
        tr.train()
        xs, labels = ds.batch(torch.randperm(len(ds), generator=g).tolist())         # one shuffled epoch per iteration
        loss = loss_fn(tr(xs), labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
    return before, eval_loss()


@pytest.mark.parametrize("split", [False, True])
def test_a_loop_on_batches_learns(split):
    lengths = (20, 7, 13, 20, 1, 16, 9, 20, 33, 12)
    g = np.random.default_rng(60)
    # rnn8, plain: evaluated on the un-augmented corpus
    tr = _tr("rnn8", split)
    d = g.normal(size=(sum(lengths), 141)).astype(np.float32)
    l = (g.uniform(size=(sum(lengths), 2)) < 0.3).astype(np.float32)
    ds = tr.dataset(_seqs(d, lengths), _seqs(l, lengths), split_size=16).manual_seed(SEED)
    tr.manual_seed(61)
    before, after = _loop(tr, ds, ds.batch(range(len(ds)), augment=False))
    print(f"EVAL LOSS rnn8 plain mode={int(split)}: {before:.5f} -> {after:.5f} after 20 train-mode iterations on ds.batch")
    assert ds.state()["call"] == 20 and after < before
    # rnn4, world: a world sample has no un-augmented form, so the evaluation batch is one fixed draw (its own call) of the whole corpus
    tr = _tr("rnn4", split)
    dw, lw = R.world_corpus(62, lengths)
    ds = tr.dataset(_seqs(dw, lengths), _seqs(lw, lengths), split_size=16, kind="world", conf_pool=torch.from_numpy(R.conf_pool(63, 64)))
    ds.set_state({"seed": SEED, "call": 1 << 20})
    held = ds.batch(range(len(ds)))
    ds.manual_seed(SEED)
    tr.manual_seed(64)
    before, after = _loop(tr, ds, held)
    print(f"EVAL LOSS rnn4 world mode={int(split)}: {before:.5f} -> {after:.5f} after 20 train-mode iterations on ds.batch")
    assert ds.state()["call"] == 20 and after < before


@pytest.mark.parametrize("name", ["rnn8", "rnn4"])
def test_views_of_a_batch_are_not_copied_and_give_the_same_bits(name, monkeypatch):
    tr = _tr(name)
    ds, _, _ = _plain_ds(name, (5, 1, 64, 9), 70)
    xs, _ = ds.batch([2, 0, 3, 1])
    cats = []
    real = torch.cat
    monkeypatch.setattr(torch, "cat", lambda ts, *a, **k: cats.append(len(ts)) or real(ts, *a, **k))
    with torch.no_grad():
        ys = tr(xs)
        assert cats == []                                                              # consecutive views: no concatenation
        yc = tr([t.clone() for t in xs])
        assert cats == [4]
    assert all(_same(a, b) for a, b in zip(ys, yc))
    with torch.no_grad():
        assert all(_same(a, b) for a, b in zip(tr(xs[1:]), yc[1:]))                      # (off the 16-byte grid or not: the same values)
    xg = [t.clone().requires_grad_() for t in xs]                                      # inputs that want a gradient take the old path
    torch.cat(tr(xg)).sum().backward()
    assert all(t.grad is not None for t in xg)


# ---- 6: bad input ------------------------------------------------------------------------------------------------------------------
def test_bad_input_is_rejected_before_anything_is_enqueued(monkeypatch):
    net = _net()
    lib, ctx = net._lib, net._ctx
    d, l = R.world_corpus(80, (5, 3))
    seqs = lambda a: _seqs(a, (5, 3))
    pool = torch.from_numpy(R.conf_pool(81, 4))
    tr4 = _tr("rnn4")
    calls = []
    real = lib.rc_subnet_batch
    monkeypatch.setattr(lib, "rc_subnet_batch", lambda *a: calls.append(1) or real(*a))
    with pytest.raises(ValueError, match="world"):
        _tr("rnn7").dataset(seqs(d), seqs(l), kind="world", conf_pool=pool)
    with pytest.raises(ValueError, match="conf_pool"):
        tr4.dataset(seqs(d), seqs(l), kind="world")
    with pytest.raises(ValueError, match="expected"):
        tr4.dataset(seqs(d[:, :170]), seqs(l), kind="world", conf_pool=pool)           # wrong widths
    with pytest.raises(ValueError, match="expected"):
        tr4.dataset(seqs(d), seqs(l))                                                  # plain rnn4 takes [T, 171] / [T, 69]
    with pytest.raises(ValueError, match="conf_pool"):
        tr4.dataset(seqs(d), seqs(l), kind="world", conf_pool=torch.zeros(4, 32))
    with pytest.raises(ValueError):
        tr4.dataset(seqs(d), _seqs(l[:7], (5, 2)), kind="world", conf_pool=pool)           # the sequences differ in frames
    ds = tr4.dataset(seqs(d), seqs(l), kind="world", conf_pool=pool)
    with pytest.raises(ValueError, match="distinct"):
        ds.batch([1, 0])                                                               # T = 5 > P = 4
    with pytest.raises(ValueError, match="no indices"):
        ds.batch([])
    with pytest.raises(ValueError, match="outside"):
        ds.batch([2])
    with pytest.raises(ValueError, match="un-augmented"):
        ds.batch([1], augment=False)
    with pytest.raises(ValueError):
        ds.set_state({"seed": 1 << 64, "call": 0})
    assert calls == [] and ds.state() == {"seed": 0, "call": 0}
    xs, _ = ds.batch([1, 1])                                                           # T = 3 <= P = 4 works
    assert calls == [1] and ds.state()["call"] == 1 and tuple(xs[1].shape) == (3, 171)
    # the C entry itself: a negative return with a message, nothing enqueued
    INVALID = -1
    p, sp = _lib.ptr, _lib.stream_ptr()
    x, y = torch.empty(8, 171, device=net.device), torch.empty(8, 69, device=net.device)
    off, lens = (C.c_int64 * 2)(0, 5), (C.c_int32 * 2)(5, 3)
    pool8 = torch.from_numpy(R.conf_pool(82, 8)).to(net.device)
    good = [ctx, b"rnn4", 1, p(ds.data), p(ds.label), 2, off, lens, p(pool8), 8, 1, SEED, 0, p(x), p(y), sp]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return real(*a)

    before = x.clone().fill_(7.0)
    x.fill_(7.0)
    assert call(a9=4) == INVALID and b"rc_subnet_batch" in lib.rc_last_error(ctx) and b"distinct" in lib.rc_last_error(ctx)   # T > P
    assert call(a1=b"rnn7") == INVALID and b"world" in lib.rc_last_error(ctx)
    assert call(a1=b"rnn9") == INVALID and call(a2=2) == INVALID
    assert call(a8=None) == INVALID and b"pool" in lib.rc_last_error(ctx)
    assert call(a5=0) == INVALID and call(a5=-1) == INVALID
    assert call(a10=0) == INVALID
    for k in ("a3", "a4", "a6", "a7", "a13", "a14"):
        assert call(**{k: None}) == INVALID, k
    assert call(a6=(C.c_int64 * 2)(0, 1 << 39)) == INVALID and b"corpus" in lib.rc_last_error(ctx)  # a sample past the corpus's allocation
    assert call(a6=(C.c_int64 * 2)(-1, 5)) == INVALID and call(a7=(C.c_int32 * 2)(5, 0)) == INVALID
    assert real(None, *good[1:]) == INVALID
    assert _same(x, before)
    assert call() == 0
