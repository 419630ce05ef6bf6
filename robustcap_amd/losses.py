"""The losses the reference trains its six sub-nets with, on the device: ``loss = tr.loss()`` -- the first call of the iteration of
``articulate/utils/torch/train.py:117`` (``loss = loss_fn(net(d), l)``), with ``RNNLossWrapper``'s meaning: the sequences of the batch are
concatenated first, the loss function sees one [F, W] tensor of outputs and one of labels.

    kind          sub-nets            the reference (net/sig_mp.py)
    mse           rnn2, rnn4, rnn6    :340,555,683  MSELoss
    window_mse    rnn3                :409-415      mse + the mse of the sums over windows of 6, 20, 60 frames cut from the END of the batch
    pose_fk       rnn7                :749-767      mse + 100 mse of the joints the 24 r6d rotations give on the rest bones
    bce_logits    rnn8                :829-831      BCEWithLogitsLoss(pos_weight=(1 - l).sum(0) / l.sum(0))

One HIP entry, ``rc_subnet_loss`` (csrc/rc_loss.hip), forms the value and ``dx = d value / d x`` in the same launch, summed in double in a
fixed order: no read-back, no host synchronisation, the same bits on every run. ``dx`` is what ``backward()`` hands to
``rc_subnet_backward_train`` as ``dy``. Labels are constants; there is no double backward.

The validation pass (train.py:101,131: ``sum([eval_fn(net(d), l) for d, l in vald_dataloader]) / num_vald_step``) takes its per-batch
values from a second entry, ``rc_subnet_eval``: ``SubnetEval`` returns one value per validation batch of a concatenated output in one
call -- the four kinds above, each group with the bits of ``SubnetLoss`` on its slice, and ``position_error``, the ``eval_fn`` of rnn2
and rnn4 (net/sig_mp.py:341,556) -- and ``reference_mean`` is the reference's fp32 mean of them.
"""
import ctypes as C

import torch

from . import _lib
from . import body as _body
from . import config as cfg

KINDS = {"mse": 0, "bce_logits": 1, "window_mse": 2, "pose_fk": 3}            # rc_loss_kind
WIDTHS = {"mse": (69, 3), "bce_logits": (2,), "window_mse": (3,), "pose_fk": (144,)}
WINDOWS = (6, 20, 60)
# the geometry of csrc/rc_loss.hip (RC_LOSS_* of rc_internal.h), for the tests that stand on its edges
VEC = 4                  # elements a thread moves at once (mse, bce_logits)
CHUNK = 4096             # elements a workgroup owns at a time (mse, bce_logits)
WINDOW_FRAMES = 240      # frames a workgroup owns at a time, counted from the end of the batch (window_mse)
POSE_FRAMES = 16         # frames a workgroup owns at a time (pose_fk)
MAX_PARTIALS = 1024      # workgroups of a call at most: beyond it a workgroup takes several such shares
# the validation metrics (rc_subnet_eval): the four losses plus the reference's eval_fn of rnn2 and rnn4 (rc_eval_kind)
EVAL_KINDS = dict(KINDS, position_error=16)
EVAL_POINTS = 1024       # 3-D points a workgroup owns at a time (position_error; RC_EVAL_POINTS)
EVAL_MAX_GROUPS = 65536  # groups of a call at most (RC_EVAL_MAX_GROUPS)


def check_frames(kind, frames):
    """ValueError where the reference's loss has no value: ``window_mse`` below 60 frames is the mean of an empty tensor (NaN)."""
    if frames <= 0:
        raise ValueError(f"{kind}: no frames")
    if kind == "window_mse" and frames < max(WINDOWS):
        raise ValueError(f"window_mse needs at least {max(WINDOWS)} frames ({frames} given): no window of {max(WINDOWS)} frames exists "
                         "and the reference's value is the NaN of an empty mean")


def _on(t, device):
    """t lives on `device` ("cuda" names the current device: an index is compared only where both have one)."""
    return t.device.type == device.type and (t.device.index is None or device.index is None or t.device.index == device.index)


def _rows(ts, what, device=None):
    """(tensors, lengths, width) of ``ys`` / ``labels``: one [F, W] tensor or a list of [T_i, W] tensors, float32."""
    ts = [ts] if isinstance(ts, torch.Tensor) else list(ts)
    if not ts or any(not isinstance(t, torch.Tensor) or t.dim() != 2 for t in ts):
        raise ValueError(f"{what}: one [F, W] tensor or a non-empty list of [T_i, W] tensors")
    if any(t.dtype != torch.float32 for t in ts):
        raise ValueError(f"{what}: float32 expected, got {sorted({str(t.dtype) for t in ts})}")
    if len({int(t.shape[1]) for t in ts}) != 1:
        raise ValueError(f"{what}: the tensors differ in width")
    if device is not None and any(not _on(t, device) for t in ts):
        raise ValueError(f"{what}: expected on {device}")
    return ts, [int(t.shape[0]) for t in ts], int(ts[0].shape[1])


def _flat_view(ts):
    """The [F, W] tensor whose rows are those of ``ts`` in list order WITHOUT a copy where the list is the split views of one contiguous
    tensor (what ``tr(...)`` returns: same storage, each view contiguous and starting where the one before ends), else None."""
    first = ts[0]
    W = int(first.shape[1])
    store, at = first.untyped_storage().data_ptr(), first.storage_offset()
    for t in ts:
        if not t.is_contiguous() or t.untyped_storage().data_ptr() != store or t.storage_offset() != at:
            return None
        at += t.shape[0] * W
    return first.as_strided((sum(int(t.shape[0]) for t in ts), W), (W, 1), first.storage_offset())


def _concat(ts):
    if len(ts) == 1 and ts[0].is_contiguous():
        return ts[0]
    flat = _flat_view(ts)
    return flat if flat is not None else torch.cat(ts).contiguous()


def _aligned(t):
    return t if t.data_ptr() % 16 == 0 else t.clone()                           # (a view off the 16-byte grid: the kernels move 16-byte pieces)


class _LossFunction(torch.autograd.Function):
    """inputs: the SubnetLoss, the labels [F, W] on the device, whether dx is wanted, then the sequences of ``ys``."""

    @staticmethod
    def forward(ctx, loss, y, want_dx, *xs):
        x = _aligned(_concat([t.detach() for t in xs]))
        value = torch.empty((), device=x.device)
        dx = torch.empty_like(x) if want_dx else None
        net = loss._net
        rc = net._lib.rc_subnet_loss(net._ctx, KINDS[loss.kind], _lib.ptr(x), _lib.ptr(y), x.shape[0], x.shape[1], _lib.ptr(loss.pos_weight),
                                     _lib.ptr(value), _lib.ptr(dx), _lib.stream_ptr())
        _lib.check(net._ctx, rc, "rc_subnet_loss")
        ctx.dx, ctx.lengths = dx, [int(t.shape[0]) for t in xs]
        return value

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if ctx.dx is None:
            raise RuntimeError("this loss was evaluated without its gradient")
        return (None, None, None) + tuple(torch.split(ctx.dx * g, ctx.lengths))


class SubnetLoss:
    """``loss(ys, labels)`` -> 0-d device tensor, differentiable with respect to ``ys``. ``kind``: a key of ``KINDS``; ``pos_weight``
    ([2], ``bce_logits`` only; None: ones); ``width``: the only width accepted (``tr.loss()`` passes the sub-net's), default any the
    kind has. Each of ``ys`` and ``labels`` is one [F, W] tensor or a list of [T_i, W] tensors, concatenated in list order
    (``RNNLossWrapper``); only the total number of frames has to agree. ``ys`` on the device; ``labels`` anywhere (moved). Every
    check raises ValueError before anything is enqueued. Under ``torch.no_grad()``, or when no ``ys`` requires a gradient, only the
    value is formed."""

    def __init__(self, net, kind, pos_weight=None, width=None):
        if kind not in KINDS:
            raise ValueError(f"loss kind {kind!r}: one of {sorted(KINDS)}")
        if width is not None and width not in WIDTHS[kind]:
            raise ValueError(f"{kind}: width {width} not in {WIDTHS[kind]}")
        if pos_weight is not None and kind != "bce_logits":
            raise ValueError(f"{kind} takes no pos_weight")
        self._net, self.kind = net, kind
        self.widths = WIDTHS[kind] if width is None else (int(width),)
        self.pos_weight = None
        if kind == "bce_logits":
            pw = torch.ones(2) if pos_weight is None else torch.as_tensor(pos_weight).detach()
            if pw.numel() != 2:
                raise ValueError("pos_weight: two values expected")
            self.pos_weight = pw.to(device=net.device, dtype=torch.float32).reshape(2).contiguous()

    def __call__(self, ys, labels):
        net = self._net
        xs, xl, xw = _rows(ys, "ys", net.device)
        ls, ll, lw = _rows(labels, "labels")
        if xw not in self.widths or lw != xw:
            raise ValueError(f"{self.kind}: width {self.widths} expected, ys have {xw}, labels {lw}")
        if sum(xl) != sum(ll):
            raise ValueError(f"ys hold {sum(xl)} frames, labels {sum(ll)}")
        check_frames(self.kind, sum(xl))
        y = _aligned(_concat([t.detach().to(net.device) for t in ls]))
        want_dx = torch.is_grad_enabled() and any(t.requires_grad for t in xs)
        return _LossFunction.apply(self, y, want_dx, *xs)


class SubnetEval:
    """``ev(ys, labels, group_rows=k)`` or ``ev(ys, labels, group_sizes=[...])`` -> device tensor [G]: the validation metric of every
    validation batch of a concatenated output in ONE call (``rc_subnet_eval``), never differentiable. ``kind``: a key of
    ``EVAL_KINDS`` -- a loss kind (value g has the bits of ``SubnetLoss(kind)`` on group g's slice) or ``"position_error"`` (rnn2's and
    rnn4's ``eval_fn``, net/sig_mp.py:341,556: the mean distance of the group's 3-D points); ``pos_weight`` and ``width`` as
    ``SubnetLoss``. ``ys`` / ``labels``: one [F, W] tensor or a list of [T_i, W] tensors each, as ``SubnetLoss`` takes them.
    ``group_sizes``: the FRAMES of every group, in order, summing to F; ``group_rows=k``: consecutive groups of k of the sequences of
    ``ys``, the last one smaller -- the batches of ``DataLoader(dataset, k)``. Every check raises ValueError before anything is
    enqueued; consecutive views of one buffer are taken without a copy."""

    def __init__(self, net, kind, pos_weight=None, width=None):
        if kind not in EVAL_KINDS:
            raise ValueError(f"evaluation kind {kind!r}: one of {sorted(EVAL_KINDS)}")
        if kind == "position_error":
            if pos_weight is not None:
                raise ValueError("position_error takes no pos_weight")
            if width is not None and (width < 3 or width % 3):
                raise ValueError(f"position_error: width {width} is no multiple of 3")
            self._net, self.kind, self.pos_weight = net, kind, None
            self.widths = None if width is None else (int(width),)
        else:
            base = SubnetLoss(net, kind, pos_weight=pos_weight, width=width)
            self._net, self.kind, self.pos_weight, self.widths = net, kind, base.pos_weight, base.widths

    def _fits(self, w):
        return (w >= 3 and w % 3 == 0) if self.widths is None else w in self.widths

    def __call__(self, ys, labels, group_rows=None, group_sizes=None):
        net = self._net
        xs, xl, xw = _rows(ys, "ys", net.device)
        ls, ll, lw = _rows(labels, "labels")
        if not self._fits(xw) or lw != xw:
            raise ValueError(f"{self.kind}: width {self.widths or 'a multiple of 3'} expected, ys have {xw}, labels {lw}")
        if sum(xl) != sum(ll):
            raise ValueError(f"ys hold {sum(xl)} frames, labels {sum(ll)}")
        if (group_rows is None) == (group_sizes is None):
            raise ValueError("exactly one of group_rows and group_sizes")
        if group_rows is not None:
            k = int(group_rows)
            if k < 1:
                raise ValueError(f"group_rows {group_rows}: at least 1")
            sizes = [sum(xl[i:i + k]) for i in range(0, len(xl), k)]
        else:
            sizes = [int(s) for s in group_sizes]
            if sum(sizes) != sum(xl):
                raise ValueError(f"group_sizes sum to {sum(sizes)} frames, ys hold {sum(xl)}")
        if not 1 <= len(sizes) <= EVAL_MAX_GROUPS:
            raise ValueError(f"{len(sizes)} groups: 1 .. {EVAL_MAX_GROUPS} expected")
        for g, s in enumerate(sizes):
            try:
                check_frames(self.kind, s)
            except ValueError as e:
                raise ValueError(f"group {g}: {e}") from None
        needs_grid = self.kind in ("mse", "bce_logits", "pose_fk")
        fit = _aligned if needs_grid else (lambda t: t)
        x = fit(_concat([t.detach() for t in xs]))
        y = fit(_concat([t.detach().to(net.device) for t in ls]))
        G = len(sizes)
        values = torch.empty(G, device=x.device)
        rc = net._lib.rc_subnet_eval(net._ctx, EVAL_KINDS[self.kind], _lib.ptr(x), _lib.ptr(y), G, (C.c_int64 * G)(*sizes), xw,
                                     _lib.ptr(self.pos_weight), _lib.ptr(values), _lib.stream_ptr())
        _lib.check(net._ctx, rc, "rc_subnet_eval")
        return values


def reference_mean(values):
    """The reference's ``sum([eval_fn(net(d), l) for (d, l) in valid_dataloader]) / num_vald_step`` (articulate/utils/torch/train.py:
    101,131) of the per-batch ``values`` [G] as a Python float: Python's ``sum`` over fp32 0-d tensors is a sequential fp32 sum
    starting from the int 0, in order, and the division by the int G stays in fp32. Reads ``values`` back (the one wait of a validation)."""
    v = torch.as_tensor(values).detach().to(device="cpu", dtype=torch.float32).reshape(-1)
    if v.numel() == 0:
        raise ValueError("reference_mean: no values")
    total = v[0].clone()
    for i in range(1, v.numel()):
        total = total + v[i]
    return float(total / v.numel())


def pos_weight_from_labels(labels):
    """``(1 - l).sum(0) / l.sum(0)`` over the concatenated labels (net/sig_mp.py:829-830): rnn8's ``pos_weight``. ``labels``: one tensor,
    a list of tensors, a ``tr.dataset(...)`` (its label buffer on the device: every frame of the corpus once, as the reference's
    ``torch.cat(label)``) or a ``tr.concat(...)`` of such (its parts' buffers, concatenated)."""
    if hasattr(labels, "label") and hasattr(labels, "samples"):
        l = labels.label
        if isinstance(l, (list, tuple)):
            l = torch.cat(list(l))
    else:
        ls, _, _ = _rows(labels, "labels")
        l = torch.cat(ls)
    return (1 - l).sum(dim=0) / l.sum(dim=0)


def position_error(ys, labels, device="cuda"):
    """The reference's ``rnn_dist_eval_fn = RNNLossWrapper(art.PositionErrorEvaluator())`` of rnn2 and rnn4 (net/sig_mp.py:341,556):
    the mean Euclidean distance of the 23 predicted joints, on ``body.position_error`` over the concatenated lists. A Python float;
    no gradient."""
    xs, xl, xw = _rows(ys, "ys")
    ls, ll, lw = _rows(labels, "labels")
    if xw != lw or sum(xl) != sum(ll) or xw % 3:
        raise ValueError(f"ys [{sum(xl)}, {xw}] and labels [{sum(ll)}, {lw}] must hold the same 3-D points")
    return _body.position_error(torch.cat([t.detach() for t in xs]), torch.cat([t.detach() for t in ls]), device=device)


def for_subnet(tr, pos_weight=None):
    """``tr.loss(pos_weight)``: the loss the reference trains this trainer's sub-net with (``config.LOSS``)."""
    return SubnetLoss(tr._net, cfg.LOSS[tr.name], pos_weight=pos_weight, width=dict((n, o) for n, _, _, o in cfg.NETS)[tr.name])
