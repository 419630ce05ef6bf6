"""Inputs and float64 objective of the synthetic closure that pins the device L-BFGS (csrc/rc_smplify.hip: rc_syn_closure_*,
tests/lbfgs_device_emu.cpp), and the fixture's record of a run. Shared by test_lbfgs_device_emu_cpu.py (which writes
tests/golden/lbfgs_device_trace.json from the emulator) and test_gpu_lbfgs_device_exact.py (which reads it)."""
import hashlib
import json
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lbfgs_device_trace.json")
SETTINGS = {"prod": dict(lr=1e-3, max_iter=20, history_env=0), "hist2": dict(lr=1.0, max_iter=12, history_env=2),
            "hist4": dict(lr=1.0, max_iter=60, history_env=4)}
ROWS = ("T1", "T54", "T55")                      # 75, 4,050 and 4,125 elements: inside a block, just under one, two blocks (29 in the second)
GRID = tuple(f"grid_{k}" for k in range(8))      # T = 1 rows of the grid-y case, 8 seeds cycled
GRID_Y_MAX = 65535


def inputs(T, seed, x_scale):
    """(x0, a, b) of a case, float32 [75 T] each: the emulator's generator (a 32-bit LCG, every value exact in fp32)."""
    n, s = 75 * T, int(seed)
    draws = np.empty(3 * n, np.int64)
    for i in range(3 * n):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        draws[i] = s >> 8
    d = draws.reshape(n, 3)
    a = (0.5 + (d[:, 0] % 1024) / 1024.0 * 2.0).astype(np.float32)
    b = (((d[:, 1] % 2048) - 1024) / 1024.0).astype(np.float32)
    x0 = (np.float32(x_scale) * (((d[:, 2] % 2048) - 1024) / 2048.0).astype(np.float32)).astype(np.float32)
    if x_scale == 0.0:
        b = np.zeros(n, np.float32)                  # the row that starts at its optimum
    return x0, a, b


def objective64(x, a, b):
    """Total and analytic gradient in float64, every operation in the order of the closure's kernels (and of the emulator, whose
    Real = double run it therefore equals bit for bit): frame + T * imu + smooth, the IMU term counting T times as in total_loss."""
    T = x.size // 75
    u = x - b
    uu = u * u
    au = a * u
    au = au + au
    g = au + uu * u
    w = x[1:] - x[:-1] * x[:-1]
    g[:-1] = g[:-1] - 8.0 * (x[:-1] * w)
    g[1:] = g[1:] + 4.0 * w
    g[::75] = g[::75] + u[::75]
    r = 0.25 * (uu * uu)
    qr = (a * uu + r).reshape(T, 75)
    ww = w * w
    w2 = np.append(ww + ww, 0.0).reshape(T, 75)      # (no w at the vector's last element)
    f, sm = np.zeros(T), np.zeros(T)
    for e in range(75):                              # a frame's terms in element order
        f = f + qr[:, e]
        sm = sm + w2[:, e]
    imu = (0.5 / T) * (u[::75] * u[::75])
    F = I = S = 0.0
    for t in range(T):
        F, I, S = F + float(f[t]), I + float(imu[t]), S + float(sm[t])
    return F + float(T) * I + S, g


def sample_index(n):
    return [(k * (n - 1)) // 15 for k in range(16)]


def record(case, n_iter, n_eval, loss_bits, x):
    """What the fixture holds of a run: x float32 [n]; losses as fp32 bit patterns."""
    x = np.ascontiguousarray(x, np.float32)
    return {"T": case["T"], "seed": case["seed"], "lr": case["lr"], "max_iter": case["max_iter"], "history_env": case["history_env"],
            "x_scale": case["x_scale"], "n_iter": int(n_iter), "n_eval": int(n_eval), "losses": [int(v) for v in loss_bits],
            "x_sha256": hashlib.sha256(x.tobytes()).hexdigest(), "x_sample": [int(v) for v in x.view(np.uint32)[sample_index(x.size)]],
            "jobs": [int(v) for v in case["jobs"]]}


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def grid_table(cases, n_rows):
    """Largest job table of a lock-step batch of n_rows rows that cycle the GRID cases: a round holds every live row's next request
    (an evaluation asks 5 inner products, a pair its Gram entries; the final flush none)."""
    longest = max(len(cases[g]["jobs"]) for g in GRID)
    return max(sum(cases[GRID[r % 8]]["jobs"][k] for r in range(n_rows) if k < len(cases[GRID[r % 8]]["jobs"])) for k in range(longest))
