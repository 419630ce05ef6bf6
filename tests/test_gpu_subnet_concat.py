"""Mixed batches on the device (tr.concat(parts).batch(...): rc_subnet_batch_parts over the kernels of csrc/rc_augment.hip) -- the
reference's ConcatDataset([AISTDataset, AMASSDataset]) of net/sig_mp.py:559-566 and :686-693, plain and world samples shuffled into one
batch. The draws are keyed by the sample's position in the WHOLE batch, so every sample must be bitwise the sample at the same position
of a single-kind ds.batch of as many samples at the same seed and call (rc_subnet_batch, whose bits tests/test_gpu_subnet_batches.py
pins to the numpy restatement)."""
import numpy as np
import pytest
import torch

import subnet_batches_ref as R
import test_gpu_subnet_batches as B
from robustcap_amd import batches

pytestmark = pytest.mark.gpu

_same = B._same
SEED = B.SEED
PLAIN_LENGTHS, WORLD_LENGTHS = (5, 1, 70, 9), (3, 66, 7)


def _parts(name, pool_rows=80):
    """(trainer, plain part, world part) of rnn4 / rnn6 on seeded corpora; the plain part is cut into pieces of 8 frames."""
    tr = B._tr(name)
    plain, _, _ = B._plain_ds(name, PLAIN_LENGTHS, 90, split_size=8)
    d, l = R.world_corpus(91, WORLD_LENGTHS)
    pool = torch.from_numpy(R.conf_pool(92, pool_rows))
    world = tr.dataset(B._seqs(d, WORLD_LENGTHS), B._seqs(l, WORLD_LENGTHS), kind="world", conf_pool=pool)
    return tr, plain, world


@pytest.mark.parametrize("name,kind", [("rnn3", "plain"), ("rnn6", "world"), ("rnn2", "plain")])
def test_a_concatenation_of_one_part_is_that_part(name, kind):
    if kind == "plain":
        part, _, _ = B._plain_ds(name, PLAIN_LENGTHS, 93, split_size=8)
    else:
        _, _, part = _parts(name)
    cat = B._tr(name).concat([part])
    assert len(cat) == len(part) and cat.name == name
    idx = [2, 0, len(part) - 1, 2, 1]
    state = {"seed": SEED, "call": 41}
    cat.set_state(state), part.set_state(state)
    a, b = cat.batch(idx), part.batch(idx)
    flat = lambda xs: [t for x in xs for t in (x if isinstance(x, tuple) else (x,))]
    assert all(_same(p, q) for p, q in zip(flat(a[0]) + a[1], flat(b[0]) + b[1]))
    assert cat.state() == part.state() == {"seed": SEED, "call": 42}


@pytest.mark.parametrize("name", ["rnn4", "rnn6"])
def test_every_sample_of_a_mixed_batch_is_the_single_kind_sample_at_its_position(name):
    tr, plain, world = _parts(name)
    cat = tr.concat([plain, world])
    n_p, n_w = len(plain), len(world)
    assert len(cat) == n_p + n_w and n_p == 13 and n_w == 3
    assert cat.samples[n_p - 1] == (0, *plain.samples[-1]) and cat.samples[n_p] == (1, *world.samples[0])       # ConcatDataset's indexing
    idx = [n_p + 1, 0, 10, n_p, 3, n_p + 1, 10, n_p + 2, -1, 1]                                              # interleaved, repeats, a negative index
    kinds = ["w" if (i % len(cat)) >= n_p else "p" for i in idx]
    state = {"seed": SEED, "call": 3000000007}
    for ds in (cat, plain, world):
        ds.set_state(state)
    xs, labels = cat.batch(idx)
    W, Wl = R.WIDTHS[name]
    lengths = [cat.samples[i][2] for i in idx]
    assert [tuple(t.shape) for t in xs] == [(T, W) for T in lengths] and [tuple(t.shape) for t in labels] == [(T, Wl) for T in lengths]
    assert tr._flat_input(xs) is not None                                   # consecutive views of one buffer: tr(xs) takes them without a copy
    assert all(bool(torch.isfinite(t).all()) for t in xs + labels)
    # the same positions in single-kind batches of as many samples (the other kind's positions hold any sample of this kind)
    px, pl = plain.batch([i if k == "p" else 0 for i, k in zip(idx, kinds)])
    wx, wl = world.batch([(i % len(cat)) - n_p if k == "w" else 0 for i, k in zip(idx, kinds)])
    for pos, k in enumerate(kinds):
        ex, el = (px, pl) if k == "p" else (wx, wl)
        assert _same(xs[pos], ex[pos]) and _same(labels[pos], el[pos]), (pos, k)
    # state() / set_state() reproduce a batch; the parts' counters were not moved by the concatenation
    assert cat.state() == {"seed": SEED, "call": 3000000008} and plain.state()["call"] == 3000000008
    cat.set_state(state)
    xs2, labels2 = cat.batch(idx)
    assert all(_same(p, q) for p, q in zip(xs + labels, xs2 + labels2))
    other, _ = cat.batch(idx)
    assert not _same(other[0], xs[0])                                       # the next call draws afresh
    # the forward takes the views
    ys = tr(xs)
    assert [tuple(t.shape) for t in ys] == [(T, Wl) for T in lengths]


def test_a_plain_concatenation_without_augmentation_is_the_corpus():
    a, da, la = B._plain_ds("rnn7", (4, 9), 94)
    b, db, lb = B._plain_ds("rnn7", (6,), 95)
    cat = B._tr("rnn7").concat([a, b])
    xs, labels = cat.batch([2, 0, 1], augment=False)
    for x, l, (d, lab, lo, hi) in zip(xs, labels, [(db, lb, 0, 6), (da, la, 0, 4), (da, la, 4, 13)]):
        assert np.array_equal(x.cpu().numpy().view(np.int32), d[lo:hi].view(np.int32))
        assert np.array_equal(l.cpu().numpy().view(np.int32), lab[lo:hi].view(np.int32))
    assert cat.state()["call"] == 0
    assert [t.data_ptr() for t in cat.label] == [a.label.data_ptr(), b.label.data_ptr()]


def test_bad_input_raises_before_anything_is_enqueued(monkeypatch):
    tr, plain, world = _parts("rnn4", pool_rows=20)
    lib = tr._net._lib
    calls = []
    real = lib.rc_subnet_batch_parts
    monkeypatch.setattr(lib, "rc_subnet_batch_parts", lambda *a: calls.append(1) or real(*a))
    cat = tr.concat([plain, world])
    with pytest.raises(ValueError, match="outside"):
        cat.batch([len(cat)])
    with pytest.raises(ValueError, match="no indices"):
        cat.batch([])
    with pytest.raises(ValueError, match="un-augmented"):
        cat.batch([0, len(plain)], augment=False)
    with pytest.raises(ValueError, match="distinct"):
        cat.batch([0, len(plain) + 1])                                     # 66 frames from a pool of 20
    with pytest.raises(ValueError, match="non-empty"):
        tr.concat([])
    with pytest.raises(ValueError, match="non-empty"):
        tr.concat([plain, "world"])
    other, _, _ = B._plain_ds("rnn3", (4,), 96)
    with pytest.raises(ValueError, match="rnn4"):
        tr.concat([plain, other])
    _, _, world80 = _parts("rnn4", pool_rows=80)
    with pytest.raises(ValueError, match="one confidence pool"):
        tr.concat([world, world80])
    with pytest.raises(ValueError):
        cat.set_state({"seed": -1, "call": 0})
    assert calls == [] and cat.state() == {"seed": 0, "call": 0}
    xs, _ = cat.batch([0, len(plain)], augment=True)                        # 3 frames from a pool of 20 works
    assert calls == [1] and cat.state()["call"] == 1 and tuple(xs[1].shape) == (3, 171)
    assert isinstance(cat, batches.ConcatSubnetDataset)
