#!/usr/bin/env python3
"""Write tests/golden/corpus/subnet_corpus.npz by RUNNING THE REFERENCE on the development machine (never on the GPU box): the corpora the
dataset builders inside train_rnn2 .. train_rnn8 (net/sig_mp.py:301-839) form from two synthetic dictionaries, which the restatement
tests/subnet_corpus_ref.py and the device builders (robustcap_amd/corpus.py, rc_subnet_corpus) have to agree with.

Recipe: the dictionaries of ``synth.make_training_dicts(SEED, LENGTHS, body, N_CAM)`` (axis-angles from ``synth._log_map``: cv2.Rodrigues is a
stand-in here) are written as ``train.pt`` / ``val.pt`` under the reference's ``paths.aist_dir`` / ``paths.amass_dir`` in the temporary
working directory, with a ``syn_c.pt``; ``sig_mp.train`` is replaced by a recorder; the six ``train_rnnK()`` run on the CPU; the
VALIDATION datasets (whole sequences) are stored.

  aist.* / amass.*                         the dictionaries as numbers (subnet_corpus_ref.pack_dicts / unpack_dicts)
  <net>.<source>.data / .label / .lengths  the reference's rows of every sample, concatenated, and the rows of each

TEST INFRASTRUCTURE. The reference is imported with the recipe of oracle/capture_reference.py (its stand-in modules and synthetic body
pickle); numbers only are stored. The sha256 goes into tests/golden/corpus/meta.json, which tests/test_subnet_corpus_cpu.py verifies.

Usage:  python tools/capture_subnet_corpus.py
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from oracle import _npz  # noqa: E402
from oracle import capture_reference as CR  # noqa: E402
from robustcap_amd import synth  # noqa: E402
import subnet_corpus_ref as R  # noqa: E402

SEED, LENGTHS, N_CAM = 11, (9, 14), 9


def as_tensors(d):
    """The dictionary as the reference reads it: tensors, lists of tensors (or None) for the keypoints."""
    out = {}
    for k, v in d.items():
        if k in ("joint2d_mp", "joint2d_occ"):
            out[k] = [[None if e is None else torch.from_numpy(np.array(e)) for e in row] for row in v]
        else:
            out[k] = [torch.from_numpy(np.array(a)) for a in v]
    return out


def main():
    art, sig_mp, body = CR.import_reference()                         # (the working directory is now a temporary one)
    aist, amass = synth.make_training_dicts(SEED, LENGTHS, body, N_CAM)
    for path, d in ((sig_mp.paths.aist_dir, aist), (sig_mp.paths.amass_dir, amass)):
        os.makedirs(path, exist_ok=True)
        for kind in ("train", "val"):
            torch.save(as_tensors(d), os.path.join(path, kind + ".pt"))
    os.makedirs("data/dataset_work", exist_ok=True)
    torch.save(torch.from_numpy(synth.uniform01(SEED, 900, 64 * 33).reshape(64, 33, 1).copy()), "data/dataset_work/syn_c.pt")
    recorded = []
    sig_mp.train = lambda net, train_dataloader, valid_dataloader, *a, **k: recorded.append(valid_dataloader.dataset)
    arrays = R.pack_dicts(aist, amass)
    for name in ("rnn2", "rnn3", "rnn4", "rnn6", "rnn7", "rnn8"):
        getattr(sig_mp, "train_" + name)()
        ds = recorded[-1]
        parts = list(ds.datasets) if hasattr(ds, "datasets") else [ds]
        sources = ("aist", "amass") if len(parts) == 2 else ("amass",)
        for source, part in zip(sources, parts):
            data = [t.detach().cpu().numpy().astype(np.float32) for t in part.data]
            label = [t.detach().cpu().numpy().astype(np.float32) for t in part.label]
            arrays[f"{name}.{source}.data"] = np.concatenate(data)
            arrays[f"{name}.{source}.label"] = np.concatenate(label)
            arrays[f"{name}.{source}.lengths"] = np.asarray([len(t) for t in data], np.int64)
            print(name, source, len(data), "samples", arrays[f"{name}.{source}.data"].shape, arrays[f"{name}.{source}.label"].shape)
    out = os.path.join(CR.OUT, "corpus")
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, "subnet_corpus.npz")
    _npz.save(path, **arrays)
    with open(path, "rb") as f:
        digest = hashlib.sha256(f.read()).hexdigest()
    with open(os.path.join(out, "meta.json"), "w") as f:
        json.dump({"sha256": {"subnet_corpus.npz": digest}, "seed": SEED, "lengths": list(LENGTHS), "n_cam": N_CAM}, f, indent=1, sort_keys=True)
    print("wrote tests/golden/corpus/subnet_corpus.npz:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
