"""``RowState`` -- records of rows of a running context (rc_save_rows / rc_load_rows, include/robustcap_hip.h).

One record is everything a body carries from frame to frame: the (h, c) of the six sub-nets (net/sig_mp.py:126-129), the fusion state of
net/sig_mp.py:85-104, the row's gravity, a deferred vision-updater step with its inputs (L264-271) and the row's last trace. It is opaque
here: a ``uint8`` tensor ``[n, bytes_per_row]`` whose bits are never interpreted, only regrouped, moved between devices and stored. The
layout is the library's; ``format`` and the six hidden sizes travel with the records so that a context can refuse
records it did not write the like of. Context parameters, weights, body and gemm mode are NOT in a record.

No GPU and no library are needed to hold, regroup, save or load a ``RowState``; only ``Net.save_rows`` / ``Net.load_rows`` touch a device.
"""
import torch

from . import config as cfg

HIDDEN = tuple(int(h) for _, _, h, _ in cfg.NETS)


class RowState:
    def __init__(self, data, format, hidden=HIDDEN):
        data = torch.as_tensor(data)
        if data.dtype != torch.uint8 or data.dim() != 2:
            raise ValueError(f"RowState: data must be a uint8 tensor [n, bytes_per_row], not {data.dtype} {tuple(data.shape)}")
        if data.shape[1] % 16:
            raise ValueError(f"RowState: bytes_per_row = {data.shape[1]} is not a multiple of 16")
        self.data = data.contiguous()
        self.format = int(format)
        self.hidden = tuple(int(h) for h in hidden)

    # ------------------------------------------------------------------------------------------------ shape
    def __len__(self):
        return int(self.data.shape[0])

    @property
    def bytes_per_row(self):
        return int(self.data.shape[1])

    @property
    def device(self):
        return self.data.device

    def __repr__(self):
        return f"RowState({len(self)} records of {self.bytes_per_row} bytes, format {self.format}, {self.device})"

    # ------------------------------------------------------------------------------------------------ moving
    def to(self, device):
        return RowState(self.data.to(device), self.format, self.hidden)

    def cpu(self):
        return self.to("cpu")

    # ------------------------------------------------------------------------------------------------ storing
    def state_dict(self):
        """Plain tensors and ints (``torch.save`` keeps every bit: the records are bytes, not floats)."""
        return {"data": self.data, "format": self.format, "hidden": list(self.hidden), "bytes_per_row": self.bytes_per_row}

    @classmethod
    def from_state_dict(cls, d):
        missing = [k for k in ("data", "format", "hidden", "bytes_per_row") if k not in d]
        if missing:
            raise ValueError(f"RowState.from_state_dict: missing {missing}")
        s = cls(d["data"], d["format"], d["hidden"])
        if s.bytes_per_row != int(d["bytes_per_row"]):
            raise ValueError(f"RowState.from_state_dict: data has {s.bytes_per_row} bytes per record, the dict says {int(d['bytes_per_row'])}")
        return s

    # ------------------------------------------------------------------------------------------------ regrouping
    def __getitem__(self, i):
        """``state[i]`` (one record, still a RowState), ``state[[i, j, ...]]``, ``state[a:b]``: copies, in the order asked for."""
        if isinstance(i, int):
            if not -len(self) <= i < len(self):
                raise IndexError(f"RowState: record {i} of {len(self)}")
            i = [i % len(self)]
        elif not isinstance(i, slice):
            i = torch.as_tensor(i, dtype=torch.long, device=self.data.device).reshape(-1)
        return RowState(self.data[i].clone(), self.format, self.hidden)

    @staticmethod
    def cat(states):
        states = list(states)
        if not states:
            raise ValueError("RowState.cat: nothing to concatenate")
        a = states[0]
        for s in states[1:]:
            if (s.format, s.hidden, s.bytes_per_row) != (a.format, a.hidden, a.bytes_per_row):
                raise ValueError(f"RowState.cat: records of format {s.format}, hidden sizes {s.hidden}, {s.bytes_per_row} bytes do not go "
                                 f"with records of format {a.format}, hidden sizes {a.hidden}, {a.bytes_per_row} bytes")
        return RowState(torch.cat([s.data for s in states]), a.format, a.hidden)

    def check(self, format, hidden, bytes_per_row, who="load_rows"):
        """ValueError naming both sides unless these records are what a context of (format, hidden, bytes_per_row) reads."""
        hidden = tuple(int(h) for h in hidden)
        if self.format != int(format) or self.hidden != hidden or self.bytes_per_row != int(bytes_per_row):
            raise ValueError(f"{who}: the records have format {self.format}, hidden sizes {self.hidden} and {self.bytes_per_row} bytes each; "
                             f"this context reads format {int(format)}, hidden sizes {hidden} and {int(bytes_per_row)} bytes each")
