"""The reference's ``train()`` (``articulate/utils/torch/train.py:15-167``) for ONE sub-net, as ``net/sig_mp.py:354,431,571,694,784,836``
calls it: epochs over a shuffled corpus, a validation pass every ``num_iter_between_vald`` iterations, the state files, resume, early
stop and ``ReduceLROnPlateau`` -- around the device iteration of ``robustcap_amd/train.py`` (``ds.batch`` -> ``tr(xs)`` -> ``tr.loss()``
-> ``backward()`` -> ``opt.step()``).

    tr = net.trainable("rnn8")
    train_ds = tr.dataset(data, label, split_size=200); valid_ds = tr.dataset(vdata, vlabel)
    history = tr.fit(train_ds, valid_ds, "weights/rnn8", pos_weight=losses.pos_weight_from_labels(train_ds))

What is restated line for line (the result depends on it): ``num_train_step = min(len, between)``; a validation when ``i %
num_train_step == num_train_step - 1``; ``train_loss`` reset at each validation and at each epoch start (an epoch's iterations after its
last validation are dropped from the average, as there); without a validation set ``vald_loss = train_loss`` (the reference passes it
through ``torch.tensor([.])``, i.e. rounds it to fp32; here it stays the double); ``min_vald_loss`` starts at 1e9; ``esn`` is reset on an
improvement and decremented otherwise, the run returns at 0; ``lr_scheduler.step(vald_loss_epoch)`` once per epoch with the SUM of the
epoch's validation losses; ``epoch_callback_fn()`` at each epoch end. Not carried over: wandb, tensorboard, ``clever_format`` --
``log_fn(record)`` is called instead and the records are returned (``epoch, it, total_it, train_loss, vald_loss, lr, best``);
``eval_metric_names`` is accepted and unused.

What is ours. Nothing in an iteration waits for the device: ``train_loss += loss.item()`` is an in-place add of the fp32 loss into a
float64 device scalar (the arithmetic of Python's float sum), read only at a validation, together with the validation's values: one
host wait. Validation is ``tr.validate`` on a ``losses.SubnetEval`` -- one ragged forward over all validation sequences, every batch's
value from ``rc_subnet_eval``, then ``losses.reference_mean``; any other callable ``eval_fn`` goes the reference's way, batch by batch.
Epoch e's order is ``torch.randperm(len(train_ds), generator=Generator().manual_seed(f(seed, e)))``: stateless, so the reference's ``if i
< train_info['it']: continue`` skips without drawing a batch.

Files, in the reference's names and layouts: ``weights.pt`` / ``best_weights.pt`` (the sub-net's tensors under the module's own keys,
``rnn.weight_ih_l0 .. linear2.bias``, ``init_net.*`` for rnn2: what ``net.rnnK.load_state_dict`` takes), ``optimizer_states.pt``
(``torch.optim.Adam``'s layout), ``train_info.pt`` (``{'epoch', 'it', 'total_it'}``) -- each loads what the other wrote. Ours beside
them: ``device_states.pt`` (dropout and batch counters, seed, the plateau scheduler, ``min_vald_loss``, ``esn``, the running
``vald_loss_epoch``, ``clip_grad_norm``). With it a resumed run continues BIT FOR BIT and validates nothing on load; without it (a
directory the reference wrote) the run behaves as ``train.py:85-104``: one validation on load sets ``min_vald_loss``.
"""
import os
from collections import OrderedDict

import torch

from . import config as cfg
from . import losses

FILES = {"weights": "weights.pt", "best": "best_weights.pt", "optimizer": "optimizer_states.pt", "info": "train_info.pt",
         "device": "device_states.pt"}


# ---- the schedule -----------------------------------------------------------------------------------------------------------------------
def num_train_step(num_iter_per_epoch, num_iter_between_vald):
    """train.py:79."""
    return min(num_iter_per_epoch, num_iter_between_vald) if num_iter_between_vald > 0 else num_iter_per_epoch


def validation_iterations(num_iter_per_epoch, num_iter_between_vald):
    """The iterations ``i`` of an epoch after which a validation runs (train.py:126)."""
    k = num_train_step(num_iter_per_epoch, num_iter_between_vald)
    return [i for i in range(num_iter_per_epoch) if i % k == k - 1]


def epoch_seed(seed, epoch):
    """f(seed, epoch): the generator seed of an epoch's order, a 63-bit mix of both."""
    return (int(seed) * 0x9E3779B97F4A7C15 + (int(epoch) + 1) * 0xD1B54A32D192ED03) & ((1 << 63) - 1)


def epoch_order(n, seed, epoch):
    """The order of the ``n`` samples in ``epoch``: a function of (seed, epoch) only."""
    return torch.randperm(int(n), generator=torch.Generator().manual_seed(epoch_seed(seed, epoch)))


# ---- ReduceLROnPlateau over anything with a writable ``lr`` ---------------------------------------------------------------------------------
class _GroupLR:
    """``lr`` of a ``torch.optim`` optimiser: read from the first group, written to all."""

    def __init__(self, opt):
        self._opt = opt

    @property
    def lr(self):
        return self._opt.param_groups[0]["lr"]

    @lr.setter
    def lr(self, value):
        for g in self._opt.param_groups:
            g["lr"] = value


def _lr_handle(opt):
    return opt if hasattr(opt, "lr") else _GroupLR(opt)


class ReduceOnPlateau:
    """``torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode='min', factor, patience)`` (train.py:70) with torch's other
    defaults -- relative threshold 1e-4, cooldown 0, min_lr 0, eps 1e-8 -- over any object with a writable ``lr``
    (``SubnetAdam`` is no ``torch.optim.Optimizer``, so torch's class cannot wrap it)."""

    def __init__(self, opt, factor=0.1, patience=10, threshold=1e-4, cooldown=0, min_lr=0.0, eps=1e-8):
        if factor >= 1.0:
            raise ValueError("factor should be < 1.0")
        self.opt, self.factor, self.patience, self.threshold = opt, float(factor), int(patience), float(threshold)
        self.cooldown, self.min_lr, self.eps = int(cooldown), float(min_lr), float(eps)
        self.best, self.num_bad_epochs, self.cooldown_counter, self.last_epoch = float("inf"), 0, 0, 0

    def step(self, metric):
        current = float(metric)
        self.last_epoch += 1
        if current < self.best * (1.0 - self.threshold):
            self.best, self.num_bad_epochs = current, 0
        else:
            self.num_bad_epochs += 1
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.num_bad_epochs = 0
        if self.num_bad_epochs > self.patience:
            old = float(self.opt.lr)
            new = max(old * self.factor, self.min_lr)
            if old - new > self.eps:
                self.opt.lr = new
            self.cooldown_counter, self.num_bad_epochs = self.cooldown, 0

    def state_dict(self):
        return {k: getattr(self, k) for k in ("best", "num_bad_epochs", "cooldown_counter", "last_epoch")}

    def load_state_dict(self, sd):
        for k in ("best", "num_bad_epochs", "cooldown_counter", "last_epoch"):
            setattr(self, k, sd[k])


# ---- files ----------------------------------------------------------------------------------------------------------------------------------
def subnet_state_dict(tr):
    """The trainer's tensors on the host under the reference module's keys, in its order."""
    return OrderedDict((k, p.detach().cpu().clone()) for k, p in tr.named_parameters())


def load_subnet_state_dict(tr, sd):
    """``net.rnnK.load_state_dict(sd)`` (strict) into the trainer's parameters, then commit."""
    names = [k for k, _ in tr.named_parameters()]
    if set(sd) != set(names):
        raise ValueError(f"{tr.name}: keys {sorted(set(sd) ^ set(names))} missing or unexpected")
    with torch.no_grad():
        for k, p in tr.named_parameters():
            if tuple(sd[k].shape) != tuple(p.shape):
                raise ValueError(f"{tr.name}.{k}: shape {tuple(sd[k].shape)}, expected {tuple(p.shape)}")
            p.copy_(sd[k])
    tr.commit()


def merge_best_weights(weight_dir, names=None, file="best_weights.pt"):
    """net/sig_mp.py:850-857: ``weight_dir/<name>/best_weights.pt`` of every sub-net under ``<name>.``-prefixed keys, in
    ``config.state_dict_spec()`` order -- the state dict ``Net.load_state_dict`` takes. ``names``: the sub-nets (default: all six)."""
    names = [n[0] for n in cfg.NETS] if names is None else list(names)
    out = OrderedDict()
    for name in names:
        sd = torch.load(os.path.join(weight_dir, name, file), map_location="cpu")
        keys = [k[len(name) + 1:] for k, _ in cfg.state_dict_spec() if k.startswith(name + ".")]
        if not keys or set(sd) != set(keys):
            raise ValueError(f"{name}: {file} does not hold the sub-net's tensors")
        for k in keys:
            out[f"{name}.{k}"] = sd[k]
    return out


def _first(v):
    """``vald_loss.view(-1)[0]`` of what an ``eval_fn`` returned, as an fp32 0-d tensor on the host."""
    return torch.as_tensor(v).detach().to(device="cpu", dtype=torch.float32).reshape(-1)[0]


# ---- the loop -------------------------------------------------------------------------------------------------------------------------------
def train(tr, train_ds, valid_ds=None, save_dir="weights", loss_fn=None, eval_fn=None, optimizer=None, batch_size=256, valid_batch_size=64,
          num_epoch=5000, num_iter_between_vald=-1, early_stop_threshold=-1, clip_grad_norm=0., load_last_states=True,
          eval_metric_names=None, epoch_callback_fn=None, lr_scheduler_patience=None, log_fn=None, seed=0, valid_rows_per_call=None,
          stop_fn=None):
    """Train ``tr``'s sub-net; returns the validation records (module docstring). ``loss_fn``: default ``tr.loss()``; ``eval_fn``:
    default ``loss_fn``'s kind as a ``SubnetEval`` -- a ``SubnetEval`` validates in one device pass, any other callable per batch as
    ``eval_fn(net(d), l)``; ``optimizer``: default ``tr.optimizer(clip_grad_norm=clip_grad_norm)`` (a ``SubnetAdam`` clips inside its
    step: a positive ``clip_grad_norm`` is written to it; any other optimiser gets ``clip_grad_norm_`` in front of its step).
    ``valid_rows_per_call``: None validates the whole set in ONE ragged forward (measured faster: profiles/subnet_fit_bench.txt),
    else a multiple of ``valid_batch_size``. ``seed`` keys the epoch orders, the dropout masks and both datasets' draws: the trainer and
    the datasets are re-seeded here (a resumed run takes the saved seed and counters instead). ``stop_fn(record) -> bool`` ends the run after that validation's files are written."""
    net, name = tr._net, tr.name
    if train_ds.name != name or (valid_ds is not None and valid_ds.name != name):
        raise ValueError(f"the datasets must be {name}'s")
    if loss_fn is None:
        loss_fn = tr.loss()
    if eval_fn is None:
        eval_fn = losses.SubnetEval(net, loss_fn.kind, pos_weight=loss_fn.pos_weight) if isinstance(loss_fn, losses.SubnetLoss) else loss_fn
    if optimizer is None:
        optimizer = tr.optimizer(clip_grad_norm=clip_grad_norm)
    clips_itself = hasattr(optimizer, "clip_grad_norm")
    if clips_itself and clip_grad_norm > 0:
        optimizer.clip_grad_norm = float(clip_grad_norm)
    lr_of = _lr_handle(optimizer)
    scheduler = ReduceOnPlateau(lr_of, factor=0.1, patience=lr_scheduler_patience) if lr_scheduler_patience is not None else None
    os.makedirs(save_dir, exist_ok=True)
    path = {k: os.path.join(save_dir, v) for k, v in FILES.items()}

    min_vald_loss = 1e9
    num_iter_per_epoch = -(-len(train_ds) // int(batch_size))
    nts = num_train_step(num_iter_per_epoch, num_iter_between_vald)
    fresh_esn = early_stop_threshold if early_stop_threshold > 0 else float("inf")
    esn = fresh_esn
    train_info = {"epoch": 0, "it": 0, "total_it": 0}
    vald_loss_resumed = 0.0
    train_ds.manual_seed(seed)
    if valid_ds is not None:
        valid_ds.manual_seed(epoch_seed(seed, -1))
    tr.manual_seed(seed)

    def validation():
        """([G] fp32 values on the host, the train-loss sum) with one wait, or per batch the reference's way."""
        if valid_ds is None:
            return None, float(acc.cpu())
        if isinstance(eval_fn, losses.SubnetEval):
            values = tr.validate(valid_ds, eval_fn, valid_batch_size, valid_rows_per_call)
            both = torch.cat([values.double(), acc.view(1)]).cpu()
            return both[:-1].float(), float(both[-1])
        was = tr.training
        tr.eval()
        values = []
        with torch.no_grad():
            for a in range(0, len(valid_ds), int(valid_batch_size)):
                xs, labels = valid_ds.batch(range(a, min(len(valid_ds), a + int(valid_batch_size))))
                ys = net._rnn_with_init_forward(xs) if name == "rnn2" else net._subnet_forward(name, xs)
                values.append(_first(eval_fn(ys, labels)))
        tr.train(was)
        return torch.stack(values), float(acc.cpu())

    acc = torch.zeros((), dtype=torch.float64, device=net.device)        # train_loss of train.py:123, on the device
    if load_last_states:
        if os.path.exists(path["info"]):
            train_info = dict(torch.load(path["info"]))
        if os.path.exists(path["optimizer"]):
            optimizer.load_state_dict(torch.load(path["optimizer"], map_location="cpu"))
        if os.path.exists(path["weights"]):
            load_subnet_state_dict(tr, torch.load(path["weights"], map_location="cpu"))
            if os.path.exists(path["device"]):                          # ours: continue bit for bit, no validation on load
                ds = torch.load(path["device"])
                tr.set_dropout_state(ds["dropout"])
                train_ds.set_state(ds["train_ds"])
                if valid_ds is not None and ds["valid_ds"] is not None:
                    valid_ds.set_state(ds["valid_ds"])
                if scheduler is not None and ds["scheduler"] is not None:
                    scheduler.load_state_dict(ds["scheduler"])
                min_vald_loss, esn, vald_loss_resumed, seed = ds["min_vald_loss"], ds["esn"], ds["vald_loss_epoch"], ds["seed"]
                if clips_itself:
                    optimizer.clip_grad_norm = float(ds["clip_grad_norm"])
            elif valid_ds is not None:                                  # the reference's branch (train.py:98-102)
                values, _ = validation()
                min_vald_loss = losses.reference_mean(values)
    total_it = train_info["total_it"]
    history = []

    for epoch in range(train_info["epoch"], num_epoch):
        tr.train()
        acc.zero_()
        vald_loss_epoch, vald_loss_resumed = vald_loss_resumed, 0.0
        order = epoch_order(len(train_ds), seed, epoch).split(int(batch_size))
        for i, idx in enumerate(order):
            if i < train_info["it"]:
                continue
            xs, labels = train_ds.batch(idx.tolist())
            loss = loss_fn(tr(xs), labels)
            optimizer.zero_grad()
            loss.backward()
            if clip_grad_norm > 0 and not clips_itself:
                torch.nn.utils.clip_grad_norm_(list(tr.parameters()), clip_grad_norm)
            optimizer.step()
            acc += loss.detach()                                        # train_loss += loss.item(), without the wait
            total_it += 1

            if i % nts == nts - 1:                                      # validation
                values, train_sum = validation()
                train_loss = train_sum / nts
                vald_loss = train_loss if values is None else losses.reference_mean(values)
                vald_loss_epoch = vald_loss_epoch + vald_loss
                weights = subnet_state_dict(tr)
                torch.save(weights, path["weights"])
                torch.save(optimizer.state_dict(), path["optimizer"])
                torch.save({"epoch": epoch, "it": i + 1, "total_it": total_it}, path["info"])
                best = vald_loss < min_vald_loss
                if best:
                    min_vald_loss = vald_loss
                    torch.save(weights, path["best"])
                    esn = fresh_esn
                else:
                    esn -= 1
                torch.save({"dropout": tr.dropout_state(), "train_ds": train_ds.state(),
                            "valid_ds": None if valid_ds is None else valid_ds.state(), "seed": seed,
                            "scheduler": None if scheduler is None else scheduler.state_dict(), "min_vald_loss": min_vald_loss,
                            "esn": esn, "vald_loss_epoch": vald_loss_epoch,
                            "clip_grad_norm": float(getattr(optimizer, "clip_grad_norm", clip_grad_norm))}, path["device"])
                record = {"epoch": epoch, "it": i + 1, "total_it": total_it, "train_loss": train_loss, "vald_loss": vald_loss,
                          "lr": float(lr_of.lr), "best": best}
                history.append(record)
                if log_fn is not None:
                    log_fn(record)
                if esn == 0:                                            # early stop
                    return history
                if stop_fn is not None and stop_fn(record):
                    return history
                acc.zero_()
                tr.train()
        if scheduler is not None:
            scheduler.step(vald_loss_epoch)
        train_info["it"] = 0
        if epoch_callback_fn is not None:
            epoch_callback_fn()
    return history


# ---- from the dictionaries ------------------------------------------------------------------------------------------------------------------
def train_subnet(net, name, aist=None, amass=None, aist_val=None, amass_val=None, conf_pool=None, save_dir="weights",
                 image_size=(1920, 1080), **overrides):
    """The reference's ``train_rnnK()`` (net/sig_mp.py:301-839) from the preprocessed dictionaries to ``best_weights.pt``:
    ``aist`` / ``amass`` are the ``train.pt`` dictionaries, ``aist_val`` / ``amass_val`` the ``val.pt`` ones, as ``torch.load`` returns
    them (the only host work is reading them). Each present dictionary becomes a corpus on the device (``corpus.build``), the training
    parts cut with ``config.TRAIN[name]["split_size"]``, the validation parts whole; the parts are concatenated in the reference's order
    (AIST, then AMASS; rnn8 trains on AMASS only and refuses ``aist``); rnn8's ``pos_weight`` comes from the training labels; then
    ``tr.fit``. ``conf_pool`` ([P, 33], ``syn_c.pt``): the AMASS parts of rnn4 / rnn6. ``overrides``: any argument of ``fit.train``, and
    ``split_size`` for the training parts. Returns ``tr.fit``'s records."""
    from . import corpus
    if name == "rnn8" and (aist is not None or aist_val is not None):
        raise ValueError("rnn8 trains on AMASS only (net/sig_mp.py:825-827)")
    if aist is None and amass is None:
        raise ValueError("train_subnet: no training dictionary")
    tr = net.trainable(name)
    split = overrides.pop("split_size", cfg.TRAIN[name]["split_size"])

    def parts(a, b, split_size):
        ps = [corpus.dataset(tr, source, d, split_size, conf_pool, image_size) for source, d in (("aist", a), ("amass", b)) if d is not None]
        return tr.concat(ps) if ps else None

    train_ds, valid_ds = parts(aist, amass, split), parts(aist_val, amass_val, -1)
    if name == "rnn8" and "pos_weight" not in overrides:
        overrides["pos_weight"] = losses.pos_weight_from_labels(train_ds)
    return tr.fit(train_ds, valid_ds, save_dir, **overrides)
