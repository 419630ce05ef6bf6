"""The host half of robustcap_amd/fit.py (the reference's train(), articulate/utils/torch/train.py:15-167), without a GPU: the plateau
scheduler against torch's, the stateless epoch order, the reference's fp32 mean of the validation values, the validation schedule,
the merged state dict and the settings tables."""
import os
import re

import numpy as np
import pytest
import torch

from robustcap_amd import config as cfg
from robustcap_amd import fit
from robustcap_amd import losses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Opt:
    def __init__(self, lr):
        self.lr = lr


def _series(kind, seed):
    g = torch.Generator().manual_seed(seed)
    n = 40
    if kind == "plateau":
        return [1.0] * n
    if kind == "below_threshold":                      # improves by less than the relative 1e-4 each step: every step is a bad one
        return [1.0 * (1.0 - 5e-5) ** i for i in range(n)]
    if kind == "above_threshold":                      # improves by more
        return [1.0 * (1.0 - 2e-4) ** i for i in range(n)]
    if kind == "mixed":
        v, out = 1.0, []
        for r in torch.rand(n, generator=g).tolist():
            v = v * (1.0 - 3e-4) if r < 0.3 else v * (1.0 + 1e-3 * r)
            out.append(v)
        return out
    return (1.0 + torch.rand(n, generator=g)).tolist()   # noise


@pytest.mark.parametrize("kind", ["plateau", "below_threshold", "above_threshold", "mixed", "noise"])
@pytest.mark.parametrize("patience,lr", [(0, 1e-3), (2, 1e-3), (5, 1e-4), (1, 3e-8)])
def test_reduce_on_plateau_is_torchs(kind, patience, lr):
    """lr after every step equal to ReduceLROnPlateau(mode='min', factor=0.1, patience) on a dummy SGD; lr 3e-8 meets eps = 1e-8: the
    first reduction (2.7e-8) is taken, the second (2.7e-9) is not."""
    sgd = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    theirs = torch.optim.lr_scheduler.ReduceLROnPlateau(sgd, mode="min", factor=0.1, patience=patience)
    opt = _Opt(lr)
    ours = fit.ReduceOnPlateau(opt, factor=0.1, patience=patience)
    for i, v in enumerate(_series(kind, 7 + patience)):
        theirs.step(v)
        ours.step(v)
        assert opt.lr == sgd.param_groups[0]["lr"], (kind, patience, i)
    if kind == "plateau":
        assert opt.lr < lr
    if kind == "plateau" and lr == 3e-8:
        assert opt.lr == 3e-8 * 0.1                     # stopped by eps
    if kind == "above_threshold":
        assert opt.lr == lr
    state = ours.state_dict()
    again = fit.ReduceOnPlateau(_Opt(opt.lr), factor=0.1, patience=patience)
    again.load_state_dict(state)
    assert again.state_dict() == state


def test_reduce_on_plateau_over_a_torch_optimiser():
    sgd = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1e-2)
    s = fit.ReduceOnPlateau(fit._lr_handle(sgd), patience=0)
    s.step(1.0)
    s.step(1.0)
    assert sgd.param_groups[0]["lr"] == 1e-2 * 0.1


def test_epoch_order():
    for n in (1, 17, 1000):
        a = fit.epoch_order(n, 3, 0)
        assert sorted(a.tolist()) == list(range(n))
    torch.manual_seed(1)
    a = fit.epoch_order(1000, 3, 5)
    torch.manual_seed(2)                                # a function of (seed, epoch) only: not of torch's global generator
    torch.rand(10)
    assert torch.equal(a, fit.epoch_order(1000, 3, 5))
    assert not torch.equal(a, fit.epoch_order(1000, 3, 6)) and not torch.equal(a, fit.epoch_order(1000, 4, 5))
    assert len({tuple(fit.epoch_order(50, 0, e).tolist()) for e in range(20)}) == 20
    assert all(0 <= fit.epoch_seed(s, e) < 1 << 63 for s in (0, 1, (1 << 64) - 1) for e in (-1, 0, 5000))


def test_reference_mean_is_the_sequential_fp32_sum():
    differs = 0
    for seed in range(200):
        g = torch.Generator().manual_seed(seed)
        v = torch.rand(3 + seed % 5, generator=g) * 0.2
        total = np.float32(0.0)
        for x in v.numpy():
            total = np.float32(total + x)
        want = float(np.float32(total / np.float32(v.numel())))
        assert losses.reference_mean(v) == want
        assert want == float(sum([t for t in v]) / v.numel())                     # the reference's expression itself
        differs += want != float(np.float32(v.numpy().astype(np.float64).mean()))
    assert differs > 0                                  # ... which is not the double mean rounded once
    assert losses.reference_mean(torch.tensor([0.25])) == 0.25
    with pytest.raises(ValueError):
        losses.reference_mean(torch.zeros(0))


@pytest.mark.parametrize("n,between,step,its", [(5, 2, 2, [1, 3]), (5, -1, 5, [4]), (3, 7, 3, [2]), (1, 1, 1, [0])])
def test_validation_schedule(n, between, step, its):
    assert fit.num_train_step(n, between) == step
    assert fit.validation_iterations(n, between) == its
    assert its == [i for i in range(n) if i % step == step - 1]


def test_merge_best_weights(tmp_path):
    spec = cfg.state_dict_spec()
    for name, _, _, _ in cfg.NETS:
        os.makedirs(tmp_path / name)
        keys = [(k[len(name) + 1:], s) for k, s in spec if k.startswith(name + ".")]
        sd = {k: torch.zeros(1).expand(*s) for k, s in reversed(keys)}             # (one element of storage each; any order in the file)
        torch.save(sd, tmp_path / name / "best_weights.pt")
    merged = fit.merge_best_weights(str(tmp_path))
    assert list(merged) == [k for k, _ in spec]
    assert all(tuple(merged[k].shape) == tuple(s) for k, s in spec)
    two = fit.merge_best_weights(str(tmp_path), names=["rnn8", "rnn2"])
    assert list(two) == [k for k, _ in spec if k.startswith("rnn8.")] + [k for k, _ in spec if k.startswith("rnn2.")]
    sd = torch.load(tmp_path / "rnn3" / "best_weights.pt")
    sd.pop("linear2.bias")
    torch.save(sd, tmp_path / "rnn3" / "best_weights.pt")
    with pytest.raises(ValueError, match="rnn3"):
        fit.merge_best_weights(str(tmp_path))


def test_settings_tables():
    names = [n[0] for n in cfg.NETS]
    assert sorted(cfg.EVAL) == sorted(cfg.TRAIN) == sorted(names)
    assert all(cfg.EVAL[n] == ("position_error" if n in ("rnn2", "rnn4") else cfg.LOSS[n]) for n in names)
    assert set(losses.EVAL_KINDS) == set(losses.KINDS) | {"position_error"}
    assert all(losses.EVAL_KINDS[k] == v for k, v in losses.KINDS.items()) and losses.EVAL_KINDS["position_error"] == 16
    keys = {"num_epoch", "num_iter_between_vald", "clip_grad_norm", "lr", "lr_scheduler_patience", "batch_size", "valid_batch_size", "split_size"}
    assert all(set(cfg.TRAIN[n]) == keys for n in names)
    assert {n: cfg.TRAIN[n]["num_epoch"] for n in names} == {"rnn2": 150, "rnn3": 200, "rnn4": 200, "rnn6": 100, "rnn7": 120, "rnn8": 80}
    assert {n: cfg.TRAIN[n]["num_iter_between_vald"] for n in names} == {"rnn2": 20, "rnn3": 20, "rnn4": 60, "rnn6": 60, "rnn7": 20, "rnn8": 20}
    assert {n: cfg.TRAIN[n]["lr_scheduler_patience"] for n in names} == {"rnn2": None, "rnn3": None, "rnn4": None, "rnn6": 5, "rnn7": 5, "rnn8": 10}
    assert {n: cfg.TRAIN[n]["lr"] for n in names} == dict({n: 1e-3 for n in names}, rnn4=1e-4)


def test_geometry_constants_are_the_kernels():
    with open(os.path.join(ROOT, "robustcap_amd", "csrc", "rc_internal.h")) as f:
        src = f.read()
    define = lambda k: int(re.search(rf"#define {k} (\d+)", src).group(1))
    assert (losses.EVAL_POINTS, losses.EVAL_MAX_GROUPS) == (define("RC_EVAL_POINTS"), define("RC_EVAL_MAX_GROUPS"))
    with open(os.path.join(ROOT, "include", "robustcap_hip.h")) as f:
        assert re.search(r"RC_EVAL_POSITION_ERROR = 16\b", f.read())


def test_wrapper_checks_need_no_device():
    with pytest.raises(ValueError, match="kind"):
        losses.SubnetEval(None, "l1")
    with pytest.raises(ValueError, match="width"):
        losses.SubnetEval(None, "position_error", width=70)
    with pytest.raises(ValueError, match="pos_weight"):
        losses.SubnetEval(None, "position_error", pos_weight=(1.0, 1.0))
    ev = losses.SubnetEval(None, "position_error", width=69)
    assert ev.kind == "position_error" and ev.widths == (69,)
