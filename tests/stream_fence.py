"""The fenced run of tests/test_gpu_stream_order.py: one call of an entry of include/robustcap_hip.h on a torch side stream that is held
up by a delay kernel, its inputs written in front of it and overwritten behind it ON THAT STREAM ONLY, compared bit for bit with the same
call made alone on the default stream.

A case (Case below) is what _drive of tests/test_gpu_staged_tables.py takes, extended: make() builds what a context needs, inputs(seed)
gives the device payload (floats and byte row masks: nothing a kernel uses as an index or a length), call(made, ins) enqueues on the
current stream and returns the output tensors without reading back or synchronising (entries the header documents to synchronise
`stream` say so in `sync`), after(made) reads what only a synchronising entry can read (recurrent state, traces) once everything is done.

Reference, on the default stream: a fresh context runs call(real), another fresh context runs call(decoy) -- whose bits must differ,
so a read of the decoy cannot pass -- and then call(real): the first is what the COLD fenced call must give (the context's first call),
the second what the WARM one must give (one call with other inputs went before; a context with recurrent state has moved on).

Fenced, on s = torch.cuda.Stream() (non-blocking: the legacy null stream does not wait for it) with the work buffers x holding the decoy
and the default stream idle: delay kernel, event, x <- real, the call, held = the event has not fired, clones of the outputs, x <- decoy,
ONE synchronise. Work that left s (the null stream, an engine stream that did not wait for s) reads the decoy; work s was not made to wait
for leaves the clones stale; work that reads its inputs after the entry returned joined sees the decoy again. Warm and not `sync`: held
must be True -- the entry returned while its stream was still held up, so the fence was real and nothing waited for the device.

The delay is 4 times the host time the same call took to return in the reference run (the cold call's for the cold variant, the warm
call's for the warm one: a first call allocates), at least 20 ms and at most 500 ms, from torch.cuda._sleep calibrated once with two
events. RC_STREAM_FENCE_OUT=path appends one line per fenced run."""
import dataclasses
import gc
import os
import time
from typing import Callable, Optional, Tuple

import torch

REAL, DECOY = 101, 202                       # seeds of the two payloads of every case
FACTOR, FLOOR_MS, CEIL_MS = 4.0, 20.0, 500.0
VARIANTS = ("cold", "warm")


@dataclasses.dataclass
class Case:
    name: str
    entries: Tuple[str, ...]                 # the rc_* entries with a stream parameter that call() goes through
    make: Callable
    inputs: Callable                         # seed -> list of device tensors
    call: Callable                           # (made, ins) -> list of tensors
    after: Optional[Callable] = None         # made -> list of host tensors, read after the final synchronise
    sync: Optional[str] = None               # the clause of the header that lets an entry of this case synchronise `stream`: bits only
    payload: bool = True                     # False: the entry reads no caller buffer (rc_zero_pose), no decoy can differ


def bits(x):
    return x.detach().contiguous().view(-1).view(torch.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a).cpu(), bits(b).cpu())


def assert_same(got, want, what):
    assert len(got) == len(want) > 0, (what, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert same_bits(a, b), (what, "output", i, tuple(a.shape))


_CYCLES_PER_MS = None


def cycles_per_ms():
    """torch.cuda._sleep counts device clock ticks: their rate, measured once with two events round one long sleep"""
    global _CYCLES_PER_MS
    if _CYCLES_PER_MS is None:
        torch.cuda._sleep(1000)                                            # (the kernel's code is loaded outside the measurement)
        torch.cuda.synchronize()
        n = 20_000_000
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(n)
        b.record()
        b.synchronize()
        _CYCLES_PER_MS = n / max(a.elapsed_time(b), 1e-3)
    return _CYCLES_PER_MS


def delay_ms_for(enqueue_ms):
    return min(CEIL_MS, max(FLOOR_MS, FACTOR * enqueue_ms))


def hold(stream, ms):
    """a delay kernel of `ms` on `stream` (the current one) and the event behind it"""
    torch.cuda._sleep(int(ms * cycles_per_ms()))
    return stream.record_event()


def report(line):
    path = os.environ.get("RC_STREAM_FENCE_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _all(case, made, outs):
    outs = [o.clone() for o in outs]
    return outs + ([t.clone() for t in case.after(made)] if case.after else [])


def reference(case):
    """{"real", "decoy": payloads; "cold", "warm": the outputs wanted; "cold_ms", "warm_ms": host time of the call}, default stream"""
    real, decoy = case.inputs(REAL), case.inputs(DECOY)
    ref = {"real": real, "decoy": decoy}
    made = case.make()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs = case.call(made, real)
    ref["cold_ms"] = 1e3 * (time.perf_counter() - t0)
    torch.cuda.synchronize()
    ref["cold"] = _all(case, made, outs)
    del made, outs
    made = case.make()
    torch.cuda.synchronize()
    outs = case.call(made, decoy)
    torch.cuda.synchronize()
    other = _all(case, made, outs)
    if case.payload:
        assert len(other) == len(ref["cold"]) and any(not same_bits(a, b) for a, b in zip(other, ref["cold"])), \
            (case.name, "the decoy gives the bits of the real inputs: reading it would pass unnoticed")
    t0 = time.perf_counter()
    outs = case.call(made, real)
    ref["warm_ms"] = 1e3 * (time.perf_counter() - t0)
    torch.cuda.synchronize()
    ref["warm"] = _all(case, made, outs)
    del made, outs, other
    gc.collect()
    torch.cuda.synchronize()
    return ref


def fenced(case, variant, ref, made=None, stream=None):
    """(outputs, held, delay in ms) of the fenced call; everything is synchronised when it returns"""
    made = case.make() if made is None else made
    real, decoy = ref["real"], ref["decoy"]
    x = [d.clone() for d in decoy]
    s = torch.cuda.Stream() if stream is None else stream
    torch.cuda.synchronize()
    if variant == "warm":
        with torch.cuda.stream(s):
            outs = case.call(made, x)                                      # the other inputs: the decoy itself
            tmp = [o.clone() for o in outs]
        s.synchronize()
        del outs, tmp                                                      # (their blocks go back to s's pool: the fenced call allocates nothing new)
    torch.cuda.synchronize()
    ms = delay_ms_for(ref[variant + "_ms"])
    with torch.cuda.stream(s):
        ev = hold(s, ms)
        for a, b in zip(x, real):
            a.copy_(b)
        t0 = time.perf_counter()
        outs = case.call(made, x)
        held = not ev.query()
        took = 1e3 * (time.perf_counter() - t0)
        kept = [o.clone() for o in outs]
        for a, b in zip(x, decoy):
            a.copy_(b)
        s.synchronize()
    torch.cuda.synchronize()
    kept += [t.clone() for t in case.after(made)] if case.after else []
    report(f"{case.name} {variant}: enqueue {ref[variant + '_ms']:.3f} ms, delay {ms:.1f} ms, returned after {took:.3f} ms, held {held}"
           + (f" (bits only: {case.sync})" if case.sync else ""))
    return kept, held, ms


def run_case(case, variant, ref):
    kept, held, ms = fenced(case, variant, ref)
    assert_same(kept, ref[variant], (case.name, variant))
    if variant == "warm" and not case.sync:
        assert held, (case.name, f"the entry returned only after the {ms:.0f} ms its stream was held up: it waited for the device, "
                                 f"or 4 x {ref['warm_ms']:.2f} ms did not cover its enqueue")
    gc.collect()
    torch.cuda.synchronize()
