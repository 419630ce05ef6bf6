"""fit.train_subnet on the device: the reference's train_rnn4() (AIST views and occlusion samples concatenated with random-camera AMASS
samples, net/sig_mp.py:436-574) and train_rnn8() (AMASS only, pos_weight from the training labels, :790-839) from synthetic dictionaries
(synth.make_training_dicts) to the five state files -- batch 4, split_size 8, two validations -- and a run stopped after the first
validation and resumed, which has to end bit for bit where the uninterrupted run does."""
import functools
import os

import numpy as np
import pytest
import torch

import test_gpu_subnet_forward as FWD
from robustcap_amd import config as cfg
from robustcap_amd import fit, losses, synth

pytestmark = pytest.mark.gpu

LENGTHS, N_CAM = (40, 60), 3
# rnn4: 39 AIST pieces (two views and one occlusion sample per sequence, 38 and 58 rows cut into 5 and 8) + 13 AMASS pieces = 52 samples,
# 13 iterations of 4, a validation after the 6th and the 12th; rnn8: 13 samples, 4 iterations, a validation after the 2nd and the 4th.
# The learning rates are the reference's (config.TRAIN: 1e-4 for rnn4, 1e-3 for rnn8).
SETTINGS = {"rnn4": dict(batch_size=4, valid_batch_size=2, split_size=8, num_epoch=1, num_iter_between_vald=6),
            "rnn8": dict(batch_size=4, valid_batch_size=2, split_size=8, num_epoch=1, num_iter_between_vald=2)}


@functools.lru_cache(maxsize=None)
def _dicts():
    body = synth.make_body(1)
    return synth.make_training_dicts(21, LENGTHS, body, N_CAM), synth.make_training_dicts(22, LENGTHS, body, N_CAM)


def _pool():
    return torch.from_numpy(synth.uniform01(23, 0, 64 * 33).reshape(64, 33, 1).copy())          # syn_c.pt's layout


def _run(name, save_dir, **kw):
    (aist, amass), (aist_val, amass_val) = _dicts()
    s = dict(SETTINGS[name], seed=5)
    s.update(kw)
    net = FWD._net(1)                                                       # a fresh Net: the initial weights
    if name == "rnn8":
        return fit.train_subnet(net, name, amass=amass, amass_val=amass_val, save_dir=str(save_dir), **s)
    return fit.train_subnet(net, name, aist=aist, amass=amass, aist_val=aist_val, amass_val=amass_val, conf_pool=_pool(),
                            save_dir=str(save_dir), **s)


def _files(d):
    out = {}
    for f in ("weights.pt", "best_weights.pt", "optimizer_states.pt", "train_info.pt"):
        obj = torch.load(os.path.join(d, f), map_location="cpu")
        flat = []

        def walk(o):
            if isinstance(o, torch.Tensor):
                flat.append(o.detach().cpu().contiguous().numpy().tobytes())
            elif isinstance(o, dict):
                for k in sorted(o, key=str):
                    flat.append(str(k).encode()), walk(o[k])
            elif isinstance(o, (list, tuple)):
                for v in o:
                    walk(v)
            else:
                flat.append(repr(o).encode())
        walk(obj)
        out[f] = b"|".join(flat)
    return out


@pytest.mark.parametrize("name", ["rnn4", "rnn8"])
def test_train_subnet_from_the_dictionaries(tmp_path, name):
    a, b = tmp_path / "a", tmp_path / "b"
    straight = _run(name, a)
    assert sorted(os.listdir(a)) == sorted(fit.FILES.values())              # the five files
    assert [(r["epoch"], r["it"]) for r in straight] == ([(0, 6), (0, 12)] if name == "rnn4" else [(0, 2), (0, 4)])
    train, vald = [r["train_loss"] for r in straight], [r["vald_loss"] for r in straight]
    print(f"LOSS {name}: train " + " ".join(f"{v:.6f}" for v in train) + " | vald " + " ".join(f"{v:.6f}" for v in vald))
    assert all(np.isfinite(train + vald)) and train[1] < train[0]
    best = torch.load(os.path.join(a, "best_weights.pt"), map_location="cpu")
    assert list(best) == [k[len(name) + 1:] for k, _ in cfg.state_dict_spec() if k.startswith(name + ".")]
    first = _run(name, b, stop_fn=lambda r: True)
    assert len(first) == 1 and first == straight[:1]
    rest = _run(name, b)                                                    # load_last_states: continues from the files
    assert first + rest == straight                                         # floats compared exactly
    assert _files(a) == _files(b)
    assert torch.load(os.path.join(a, "device_states.pt")) == torch.load(os.path.join(b, "device_states.pt"))


def test_what_train_subnet_builds_and_refuses(tmp_path):
    (aist, amass), _ = _dicts()
    net = FWD._net(1)
    with pytest.raises(ValueError, match="AMASS only"):
        fit.train_subnet(net, "rnn8", aist=aist, amass=amass, save_dir=str(tmp_path))
    with pytest.raises(ValueError, match="no training"):
        fit.train_subnet(net, "rnn3", save_dir=str(tmp_path))
    # rnn8's pos_weight is (1 - l).sum(0) / l.sum(0) over the corpus rows, taken from the concatenation's label buffers
    from robustcap_amd import corpus
    tr = net.trainable("rnn8")
    ds = corpus.dataset(tr, "amass", amass, 8)
    cat = tr.concat([ds])
    pw = losses.pos_weight_from_labels(cat).cpu().numpy()
    l = ds.label.cpu().numpy().astype(np.float64)
    assert np.allclose(pw, (1 - l).sum(0) / l.sum(0), rtol=1e-6) and np.isfinite(pw).all() and (pw > 0).all()
    assert len(os.listdir(tmp_path)) == 0
