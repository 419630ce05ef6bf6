"""Rows of different lengths in one sequence call: the ragged call (rc_sequence_rows) against the padded one (rc_sequence).

    python tools/ragged_bench.py [--padded] [--workloads a b c d] [--repeat 1] [--mode 0|1|2]

Workloads (mixed confidence schedule, seeded): 256 rows, Tmax = 512, lengths (a) all 512, (b) uniform on [128, 512], (c) 224 rows
of 128 frames + 32 of 512; (d) config 3's shape, 72 rows x 600, lengths uniform on [150, 600]. Inputs past a row's length are the
harness's padding (zero keypoints and accelerations, identity orientations: evaluate.camera_inputs_rows).

One timed call = reset_states + forward_sequence on a context that has run it once before (warm-up: buffers, plan tables), HIP
events around it, median of 5; --repeat N prints N such medians and their min-max range (the run-to-run spread).

--padded: every row runs Tmax frames through Net.forward_sequence WITHOUT lengths -- nothing but the API of the commit before the
ragged call, so this leg runs on a checkout of that commit and is the baseline. Without it: forward_sequence(lengths=...).

Per workload one line: time, ticks, body-frames computed, useful body-frames/s = sum(len) / time. The ragged leg adds the time
profiles/r06_batch_sweep.json predicts for the plan from its per-tick live-row counts (rc_plan_wave_rows' counts): a tick that
starts n rows' frames is charged the sweep's ms_per_step at batch n (interpolated in n), the padded call Tmax steps at the full
batch -- a bound from measured full-batch steps, not a promise.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from robustcap_amd import _lib, synth  # noqa: E402
from robustcap_amd.net.sig_mp import Net  # noqa: E402

REPS = 5


def workload(name, seed=7):
    rng = np.random.default_rng(seed)
    if name == "a":
        B, T = 256, 512
        lens = np.full(B, T)
    elif name == "b":
        B, T = 256, 512
        lens = rng.integers(128, T + 1, B)
    elif name == "c":
        B, T = 256, 512
        lens = np.array([128] * 224 + [512] * 32)
    elif name == "d":
        B, T = 72, 600
        lens = rng.integers(150, T + 1, B)
    else:
        raise SystemExit(f"unknown workload {name}")
    lens = np.asarray(lens, np.int32)
    lens[int(np.argmax(lens))] = T                                        # the longest row defines Tmax
    return B, T, lens


def inputs(body, B, T, lens, seed=5):
    m = bench.make_inputs(body, B, T, "mixed", seed)
    j, a, o = (np.ascontiguousarray(m[k], dtype=np.float32) for k in ("j2dc", "accc", "oric"))
    for b in range(B):                                                    # the harness's padding behind a row's end
        j[b, lens[b]:] = 0.0
        a[b, lens[b]:] = 0.0
        o[b, lens[b]:] = np.eye(3, dtype=np.float32)
    t = torch.from_numpy
    return tuple(t(x).cuda() for x in (j, a, o)), t(np.ascontiguousarray(m["gravityc"], dtype=np.float32))


def timed_median(fn):
    fn()
    out = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def sweep_ms(path):
    d = json.load(open(path))
    rows = sorted((r["batch"], r["ms_per_step"]) for r in d["sweep"] if "ms_per_step" in r)
    xs, ys = np.array([r[0] for r in rows], float), np.array([r[1] for r in rows], float)
    return lambda n: float(np.interp(n, xs, ys))


def predicted_ms(net, ins, B, T, lens, sweep):
    """Time of the plan's ticks if a tick with n live rows cost one step of the batch sweep at n rows (rows starting a frame at that tick)."""
    mean = torch.empty(B * T, device="cuda")
    code = torch.empty(B * T, dtype=torch.int8, device="cuda")
    _lib.check(None, net._lib.rc_conf_mean(_lib.ptr(ins[0]), B * T, net.conf_range[0], net.conf_range[1], _lib.ptr(mean), _lib.ptr(code),
                                           _lib.stream_ptr()), "rc_conf_mean")
    torch.cuda.synchronize()
    codes = np.ascontiguousarray(code.cpu().numpy().reshape(B, T).T)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ln, fr, pd = np.ascontiguousarray(lens, np.int32), np.ones(B, np.int32), np.zeros(B, np.int32)
    nt, npre = C.c_int32(), C.c_int32()
    net._lib.rc_plan_wave_rows(p(codes), B, T, 0, p(ln), p(fr), p(pd), 1, 1, None, 0, C.byref(nt), C.byref(npre), None, None)
    fa = np.zeros((npre.value, B), np.int32)
    cnt = np.zeros((4, npre.value), np.int32)
    rc = net._lib.rc_plan_wave_rows(p(codes), B, T, 0, p(ln), p(fr), p(pd), 1, 1, p(fa), fa.size, C.byref(nt), C.byref(npre), p(cnt), None)
    assert rc == 0
    return sum(sweep(n) for n in cnt[0] if n > 0), nt.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--padded", action="store_true")
    ap.add_argument("--workloads", nargs="+", default=["a", "b", "c", "d"])
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--mode", type=int, default=1, choices=(0, 1, 2),
                    help="sequence mode: 0 frame-stepped launches, 1 planner's choice, 2 wavefront engine whenever long enough")
    ap.add_argument("--sweep", default=os.path.join(ROOT, "profiles", "r06_batch_sweep.json"))
    args = ap.parse_args()
    sd, body = synth.make_state_dict(0), synth.make_body(1)
    sweep = sweep_ms(args.sweep) if os.path.exists(args.sweep) else None
    leg = "padded" if args.padded else "ragged"
    for name in args.workloads:
        B, T, lens = workload(name)
        ins, grav = inputs(body, B, T, lens)
        net = Net(body=body, batch=B)
        net.load_state_dict(sd)
        net.gravityc = grav
        net.set_sequence_mode(args.mode != 0, 8, force=args.mode == 2)
        kw = {} if args.padded else {"lengths": lens}

        def call():
            net.reset_states()
            net.forward_sequence(*ins, **kw)

        meds = [timed_median(call) for _ in range(args.repeat)]
        t0 = net.sequence_stats()[2]
        call()
        torch.cuda.synchronize()
        ticks = net.sequence_stats()[2] - t0
        computed = B * T if args.padded else int(lens.sum())
        ms = statistics.median(meds)
        wave, stepped, _ = net.sequence_stats()
        line = {"workload": name, "leg": leg, "mode": args.mode, "engine": "wavefront" if wave else "frame-stepped", "rows": B, "Tmax": T, "sum_len": int(lens.sum()), "ms": round(ms, 3),
                "ms_range": [round(min(meds), 3), round(max(meds), 3)], "ticks": ticks, "body_frames_computed": computed,
                "useful_body_frames_per_s": round(float(lens.sum()) / (ms * 1e-3), 1)}
        if not args.padded and sweep is not None:
            pred, nt = predicted_ms(net, ins, B, T, lens, sweep)
            pred_pad = T * sweep(B)
            line.update({"planned_ticks": nt, "sweep_predicted_ms": round(pred, 3), "sweep_predicted_padded_ms": round(pred_pad, 3),
                         "sweep_predicted_ratio": round(pred_pad / pred, 3)})
        print(json.dumps(line), flush=True)
        del net


if __name__ == "__main__":
    main()
