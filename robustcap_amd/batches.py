"""The batches of a sub-net's training, built on the device: ``ds = tr.dataset(data, label, split_size=200)`` holds the corpus once on the
device and ``xs, labels = ds.batch(indices)`` is what ``DataLoader(dataset, 256, shuffle=True, collate_fn=RNNDataset.collate_fn)`` hands to
the iteration of ``articulate/utils/torch/train.py:117-122`` -- ``len(indices)`` calls of ``RNNDataset.__getitem__``
(``articulate/utils/torch/rnn.py:64-67``) with the sub-net's ``augment_fn`` -- as ONE C call, ``rc_subnet_batch`` (csrc/rc_augment.hip):

    ds = tr.dataset(data, label, split_size=200)                  # lists of [T_i, W] tensors, as RNNDataset.__init__ takes them
    for idx in torch.randperm(len(ds)).split(256):                # (the reference's whole loop around this: robustcap_amd/fit.py)
        xs, labels = ds.batch(idx.tolist())                       # consecutive views of one [F, in] and one [F, out] device buffer
        loss = loss_fn(tr(xs), labels); opt.zero_grad(); loss.backward(); opt.step()

Two kinds of sample. ``kind="plain"`` (every sub-net): the row with ``torch.normal(x, sigma)`` on the columns ``config.AUGMENT`` names,
every other column and the label copied bit for bit. ``kind="world"`` (rnn4, rnn6): the AMASS ``__getitem__`` of
``net/sig_mp.py:520-552`` / ``:649-679`` on rows ``acc[6,3] | ori[6,3,3] | j3dw_mp[33,3]`` with labels ``j3dw[24,3]`` in the world frame
and a pool of confidence rows ``[P, 33]`` (``syn_c.pt``): random camera (``config.CAMERA``), random root translation, projection, one
pool row per frame (distinct within a sample), confidence-dependent keypoint noise, for rnn4 the bounding-box normalisation, for rnn6
the joint columns and their noise.

Random state. Counter-based, like dropout's (train.py): every draw is Philox4x32-10 of (seed, call, site, the sample's position in
``indices``, the frame within the sample, the unit), so it does not depend on the other samples' lengths. ``call`` counts the
``batch(..., augment=True)`` calls since ``manual_seed``; ``state()`` / ``set_state()`` carry (seed, call) across a resume. The stream is
not torch's and not Python's ``random``: only the distributions, the sites and the order of the arithmetic are the reference's.

Nothing here reads back or waits for the device; the corpus is never written.

``SubnetDataset.from_buffers`` adopts a corpus that is already on the device (``corpus.build``) without a copy;
``ConcatSubnetDataset`` (``tr.concat(parts)``) is the reference's ``ConcatDataset`` of such datasets, plain and world samples in one
batch, as one C call (``rc_subnet_batch_parts``).
"""
import ctypes as C

import torch

from . import _lib
from . import config as cfg
from .losses import _on

KINDS = {"plain": 0, "world": 1}                 # rc_batch_kind
WORLD_WIDTHS = (171, 72)                         # acc | ori | j3dw_mp, and j3dw
_SPEC = {n: (i, o) for n, i, _, o in cfg.NETS}


def _sequences(ts, what):
    ts = list(ts)
    if not ts or any(not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[0] < 1 for t in ts):
        raise ValueError(f"{what}: a non-empty list of [T_i >= 1, W] tensors")
    if len({int(t.shape[1]) for t in ts}) != 1:
        raise ValueError(f"{what}: the tensors differ in width")
    return ts


def _pool(net, kind, conf_pool):
    """The confidence pool of a ``world`` dataset on the device ([P, 33]); None for ``plain``."""
    if kind != "world":
        if conf_pool is not None:
            raise ValueError("conf_pool belongs to kind 'world'")
        return None
    if conf_pool is None:
        raise ValueError("kind 'world' needs conf_pool [P, 33]")
    pool = torch.as_tensor(conf_pool)
    if pool.dim() == 3 and pool.shape[2] == 1:
        pool = pool[:, :, 0]                                                               # syn_c.pt is [P, 33, 1]
    if pool.dim() != 2 or pool.shape[1] != cfg.NUM_KP or pool.shape[0] < 1:
        raise ValueError(f"conf_pool: [P >= 1, 33] expected, got {tuple(pool.shape)}")
    return pool.to(device=net.device, dtype=torch.float32).contiguous()


def _table(lengths, split_size):
    """(first frame, frames) of every sample of sequences of ``lengths`` cut like ``Tensor.split``."""
    samples, at = [], 0
    for T in lengths:
        step = int(split_size) if split_size > 0 else T
        samples += [(at + a, min(step, T - a)) for a in range(0, T, step)]
        at += T
    return samples


class SubnetDataset:
    """``tr.dataset(data, label, split_size=-1, kind="plain", conf_pool=None)``. ``data`` / ``label``: lists of [T_i, W] tensors
    (anywhere; stored once on the device as two concatenated fp32 buffers, ``self.data`` and ``self.label``). ``split_size > 0`` cuts
    every sequence like ``Tensor.split`` (pieces of ``split_size`` frames, the last one shorter). ``samples``: the host table of
    (first frame, frames); ``len(ds)`` its length."""

    def __init__(self, tr, data, label, split_size=-1, kind="plain", conf_pool=None):
        if kind not in KINDS:
            raise ValueError(f"kind {kind!r}: one of {sorted(KINDS)}")
        net, name = tr._net, tr.name
        if kind == "world" and name not in cfg.CAMERA:
            raise ValueError(f"kind 'world' is rnn4's and rnn6's (the AMASS samples), not {name}'s")
        data, label = _sequences(data, "data"), _sequences(label, "label")
        if len(data) != len(label) or any(d.shape[0] != l.shape[0] for d, l in zip(data, label)):
            raise ValueError("data and label must hold the same sequences (count and frames)")
        widths = WORLD_WIDTHS if kind == "world" else _SPEC[name]
        if (int(data[0].shape[1]), int(label[0].shape[1])) != widths:
            raise ValueError(f"{name} ({kind}): data [T, {widths[0]}] and label [T, {widths[1]}] expected, got widths "
                             f"{int(data[0].shape[1])} and {int(label[0].shape[1])}")
        self._tr, self._net, self.name, self.kind = tr, net, name, kind
        self.pool = _pool(net, kind, conf_pool)
        self.data = torch.cat([t.to(dtype=torch.float32) for t in data]).to(net.device).contiguous()
        self.label = torch.cat([t.to(dtype=torch.float32) for t in label]).to(net.device).contiguous()
        self.samples = _table([int(t.shape[0]) for t in data], split_size)
        self.out_widths = _SPEC[name]
        self._seed, self._call = 0, 0

    @classmethod
    def from_buffers(cls, tr, data, label, lengths, split_size=-1, kind="plain", conf_pool=None):
        """The dataset over two device buffers that already hold the concatenated corpus (what ``corpus.build`` returns: ``data``
        [R, W], ``label`` [R, Wl], ``lengths`` the rows of every sequence), adopted WITHOUT the copy the lists-of-tensors constructor
        makes: ``ds.data`` / ``ds.label`` are the tensors handed in."""
        if kind not in KINDS:
            raise ValueError(f"kind {kind!r}: one of {sorted(KINDS)}")
        net, name = tr._net, tr.name
        if kind == "world" and name not in cfg.CAMERA:
            raise ValueError(f"kind 'world' is rnn4's and rnn6's (the AMASS samples), not {name}'s")
        lengths = [int(l) for l in lengths]
        widths = WORLD_WIDTHS if kind == "world" else _SPEC[name]
        for t, w, what in ((data, widths[0], "data"), (label, widths[1], "label")):
            if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32 or not t.is_contiguous() or not _on(t, torch.device(net.device)):
                raise ValueError(f"{what}: one contiguous fp32 [R, W] tensor on {net.device}")
            if int(t.shape[1]) != w:
                raise ValueError(f"{name} ({kind}): {what} [R, {w}] expected, got width {int(t.shape[1])}")
        if not lengths or min(lengths) < 1 or sum(lengths) != int(data.shape[0]) or int(label.shape[0]) != int(data.shape[0]):
            raise ValueError("lengths: at least one frame each, summing to the rows of data and of label")
        self = cls.__new__(cls)
        self._tr, self._net, self.name, self.kind = tr, net, name, kind
        self.pool = _pool(net, kind, conf_pool)
        self.data, self.label = data, label
        self.samples = _table(lengths, split_size)
        self.out_widths = _SPEC[name]
        self._seed, self._call = 0, 0
        return self

    def __len__(self):
        return len(self.samples)

    # ------------------------------------------------------------------------------------------------ random state
    def manual_seed(self, seed):
        """The key of the draws (64 bits); the call counter restarts at 0."""
        self.set_state({"seed": seed, "call": 0})
        return self

    def state(self):
        """{"seed", "call"} as ints (``call``: the value the next ``batch(..., augment=True)`` takes), beside ``tr.dropout_state()``."""
        return {"seed": self._seed, "call": self._call}

    def set_state(self, state):
        seed, call = int(state["seed"]), int(state["call"])
        if not (0 <= seed < 1 << 64 and 0 <= call < 1 << 32):
            raise ValueError(f"batch state out of range: seed {seed} (64 bits), call {call} (32 bits)")
        self._seed, self._call = seed, call

    # ------------------------------------------------------------------------------------------------ the batch
    def batch(self, indices, augment=True):
        """``(xs, labels)`` of the samples ``indices`` (any order, repeats allowed): lists of consecutive views of one [F, in] and one
        [F, out] device buffer; rnn2: ``xs`` is the list of pairs ``(x_i, label_i[0])`` of ``RNNWithInitDataset.__getitem__``
        (rnn.py:87-89). ``augment=False`` (and a sub-net without augmentation): bitwise the corpus slices; a ``world`` sample has no such
        form (ValueError). Bad input raises ValueError before anything is enqueued."""
        idx = [int(i) for i in indices]
        if not idx:
            raise ValueError("batch: no indices")
        ns = len(self.samples)
        if any(not -ns <= i < ns for i in idx):
            raise ValueError(f"batch: an index outside the {ns} samples")
        if self.kind == "world" and not augment:
            raise ValueError("a 'world' sample has no un-augmented form: the camera is part of it")
        picked = [self.samples[i] for i in idx]
        lengths = [l for _, l in picked]
        P = 0 if self.pool is None else int(self.pool.shape[0])
        if self.kind == "world" and max(lengths) > P:
            raise ValueError(f"a sample of {max(lengths)} frames cannot draw distinct rows from a pool of {P} (random.sample raises too)")
        n, F = len(idx), sum(lengths)
        net = self._net
        x = torch.empty(F, self.out_widths[0], device=net.device)
        y = torch.empty(F, self.out_widths[1], device=net.device)
        call = self._call
        rc = net._lib.rc_subnet_batch(net._ctx, self.name.encode(), KINDS[self.kind], _lib.ptr(self.data), _lib.ptr(self.label), n,
                                      (C.c_int64 * n)(*[o for o, _ in picked]), (C.c_int32 * n)(*lengths), _lib.ptr(self.pool), P,
                                      1 if augment else 0, self._seed, call, _lib.ptr(x), _lib.ptr(y), _lib.stream_ptr())
        _lib.check(net._ctx, rc, "rc_subnet_batch")
        if augment:
            self._call = (call + 1) & 0xFFFFFFFF
        xs, labels = list(torch.split(x, lengths)), list(torch.split(y, lengths))
        if self.name == "rnn2":
            xs = [(a, l[0]) for a, l in zip(xs, labels)]
        return xs, labels


class ConcatSubnetDataset:
    """``tr.concat(parts)``: ``torch.utils.data.ConcatDataset(parts)`` over ``SubnetDataset`` s of one sub-net, of either kind -- the
    reference's ``ConcatDataset([AISTDataset, AMASSDataset])`` (net/sig_mp.py:345-352, :559-566, :686-693) -- with the interface
    ``fit.train`` and ``tr.validate`` use. Index i is sample i - (samples of the parts before) of its part. ``batch`` is ONE C call,
    ``rc_subnet_batch_parts``: one table upload, one launch per kind present, every sample written at its rows of one [F, in] and one
    [F, out] buffer in ``indices`` order. The draws are keyed by the sample's position in the whole batch and by the concatenation's own
    (seed, call): the parts' counters are neither read nor moved. World parts share one confidence pool."""

    def __init__(self, tr, parts):
        parts = list(parts)
        if not parts or any(not isinstance(p, SubnetDataset) for p in parts):
            raise ValueError("concat: a non-empty list of SubnetDataset")
        if any(p.name != tr.name or p._net is not tr._net for p in parts):
            raise ValueError(f"concat: every part must be a dataset of this trainer's {tr.name}")
        pools = [p.pool for p in parts if p.kind == "world"]
        if any(q.shape != pools[0].shape or (q.data_ptr() != pools[0].data_ptr() and not torch.equal(q, pools[0])) for q in pools[1:]):
            raise ValueError("concat: the world parts must draw from one confidence pool")
        self._tr, self._net, self.name, self.parts = tr, tr._net, tr.name, parts
        self.pool = pools[0] if pools else None
        self.out_widths = _SPEC[self.name]
        self.samples = [(k, o, l) for k, p in enumerate(parts) for o, l in p.samples]      # (part, first frame, frames)
        self._seed, self._call = 0, 0

    def __len__(self):
        return len(self.samples)

    @property
    def label(self):
        """Every part's label buffer, in order (a list: the parts' widths differ between kinds)."""
        return [p.label for p in self.parts]

    manual_seed = SubnetDataset.manual_seed
    state = SubnetDataset.state
    set_state = SubnetDataset.set_state

    def batch(self, indices, augment=True):
        """``SubnetDataset.batch`` over the concatenation; ``augment=False`` with a world sample among ``indices`` raises ValueError."""
        idx = [int(i) for i in indices]
        if not idx:
            raise ValueError("batch: no indices")
        ns = len(self.samples)
        if any(not -ns <= i < ns for i in idx):
            raise ValueError(f"batch: an index outside the {ns} samples")
        picked = [self.samples[i] for i in idx]
        lengths = [l for _, _, l in picked]
        world = [l for k, _, l in picked if self.parts[k].kind == "world"]
        if world and not augment:
            raise ValueError("a 'world' sample has no un-augmented form: the camera is part of it")
        P = 0 if self.pool is None else int(self.pool.shape[0])
        if world and max(world) > P:
            raise ValueError(f"a sample of {max(world)} frames cannot draw distinct rows from a pool of {P} (random.sample raises too)")
        n, F, m = len(idx), sum(lengths), len(self.parts)
        net = self._net
        x = torch.empty(F, self.out_widths[0], device=net.device)
        y = torch.empty(F, self.out_widths[1], device=net.device)
        call = self._call
        rc = net._lib.rc_subnet_batch_parts(
            net._ctx, self.name.encode(), m, (C.c_int32 * m)(*[KINDS[p.kind] for p in self.parts]),
            (C.c_void_p * m)(*[p.data.data_ptr() for p in self.parts]), (C.c_void_p * m)(*[p.label.data_ptr() for p in self.parts]),
            _lib.ptr(self.pool), P, n, (C.c_int32 * n)(*[k for k, _, _ in picked]), (C.c_int64 * n)(*[o for _, o, _ in picked]),
            (C.c_int32 * n)(*lengths), 1 if augment else 0, self._seed, call, _lib.ptr(x), _lib.ptr(y), _lib.stream_ptr())
        _lib.check(net._ctx, rc, "rc_subnet_batch_parts")
        if augment:
            self._call = (call + 1) & 0xFFFFFFFF
        xs, labels = list(torch.split(x, lengths)), list(torch.split(y, lengths))
        if self.name == "rnn2":
            xs = [(a, l[0]) for a, l in zip(xs, labels)]
        return xs, labels
