"""The CPU restatement of the device-resident L-BFGS (tests/lbfgs_device_emu.cpp: csrc/rc_lbfgs_dev.h on a std::vector backend
that restates every vector kernel of csrc/rc_smplify.hip and the synthetic closure operation by operation in fp32).

  anchor     its Real = double run against rc::Lbfgs<double> through the library (rc_lbfgs_minimize, which test_lbfgs_host.py pins
             to torch.optim.LBFGS) on the same objective, whose analytic gradient is checked against torch autograd in float64
  census     the recorded fp32 cases walk every path of the optimiser and of the line search
  mutations  every wrong variant of the fp32 backend changes a recorded bit
  fixture    tests/golden/lbfgs_device_trace.json is what the emulator prints today, from g++ and from clang++

test_gpu_lbfgs_device_exact.py demands the fixture's bits of rc_lbfgs_device_probe on the GPU. Host code only.
`python tests/test_lbfgs_device_emu_cpu.py` rewrites the fixture."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import lbfgs_device_case as K  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "robustcap_amd", "csrc"),
         os.path.join(ROOT, "tests", "lbfgs_device_emu.cpp")]
CLANG = shutil.which("clang++") or ("/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else None)
RECORDED = [f"{s}_{r}" for s in K.SETTINGS for r in K.ROWS + ("zero",)] + list(K.GRID)
BITS = ("n_iter", "n_eval", "losses", "x")


def _build(compiler, flags, out):
    subprocess.run([compiler] + flags + ["-o", str(out)], check=True)
    return str(out)


def _run(exe, *args):
    out = subprocess.run([exe, *args], check=True, capture_output=True, text=True).stdout
    return {r["name"]: r for r in map(json.loads, out.splitlines())}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    return _build("g++", FLAGS, tmp_path_factory.mktemp("lbfgs_device_emu") / "lbfgs_device_emu")


@pytest.fixture(scope="module")
def f32(exe):
    return _run(exe)


@pytest.fixture(scope="module")
def f64(exe):
    return _run(exe, "--real", "double")


def _fixture_of(records):
    cases = {}
    for name in RECORDED:
        r = records[name]
        cases[name] = K.record(r, r["n_iter"], r["n_eval"], r["losses"], np.array(r["x"], np.uint32).view(np.float32))
    # the grid-y case: the fewest rows (8 seeds cycled) at which some round's job table passes a grid's y extent
    n_rows = 8
    while K.grid_table(cases, n_rows) <= K.GRID_Y_MAX:
        n_rows += 8
    return {"cases": cases, "grid_rows": n_rows, "grid_max_jobs": K.grid_table(cases, n_rows)}


def test_all_cases_ran(f32, f64):
    assert sorted(f32) == sorted(RECORDED) == sorted(f64)


# ---------------------------------------------------------------------------------------------------------------------- anchor
@pytest.mark.parametrize("T,seed", [(1, 9), (2, 3), (54, 8)])
def test_analytic_gradient_against_autograd(T, seed):
    import torch
    x0, a, b = (v.astype(np.float64) for v in K.inputs(T, seed, 1.0))
    loss, g = K.objective64(x0, a, b)
    x, at, bt = torch.tensor(x0, requires_grad=True), torch.tensor(a), torch.tensor(b)
    u, w = x - bt, x[1:] - x[:-1] ** 2
    total = (at * u ** 2 + 0.25 * u ** 4).sum() + T * (0.5 / T * u[::75] ** 2).sum() + (2.0 * w ** 2).sum()
    total.backward()
    assert np.allclose(loss, float(total.detach()), rtol=1e-12, atol=0.0)
    assert np.allclose(g, x.grad.numpy(), rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("name", RECORDED)
def test_double_emulator_matches_the_vector_formulation(f64, name):
    """direction / accept / pair of the emulator's backend mean what rc::Lbfgs<double> does with whole vectors."""
    from robustcap_amd import _lib
    lib = _lib.load()
    r = f64[name]
    x0, a, b = (v.astype(np.float64) for v in K.inputs(r["T"], r["seed"], r["x_scale"]))

    def objective(user, xp, gp, n):
        loss, g = K.objective64(np.ctypeslib.as_array(xp, (n,)).copy(), a, b)
        np.ctypeslib.as_array(gp, (n,))[:] = g
        return loss
    cb = _lib.OBJECTIVE_FN(objective)
    x = x0.copy()
    n_iter, n_eval, losses = C.c_int32(), C.c_int32(), np.zeros(256)
    rc = lib.rc_lbfgs_minimize(cb, None, len(x), x.ctypes.data_as(C.POINTER(C.c_double)), float(np.float32(r["lr"])), r["max_iter"], r["max_eval"],
                               r["history"], 1e-7, 1e-9, C.byref(n_iter), C.byref(n_eval), losses.ctypes.data_as(C.POINTER(C.c_double)), 256)
    assert rc == 0
    assert (r["n_iter"], r["n_eval"]) == (n_iter.value, n_eval.value)
    assert len(r["losses"]) == r["n_eval"]
    assert np.allclose(r["losses"], losses[:n_eval.value], rtol=1e-6, atol=1e-12)
    assert np.allclose(r["x"], x, rtol=1e-6, atol=1e-8)


# ---------------------------------------------------------------------------------------------------------------------- census
def _iterations(r):
    return [s for s in r["steps"][1:] if s]                                   # evaluations of every line search (steps[0]: the one at x)


def _growing(s):
    return sum(1 for i in range(1, len(s)) if s[i] > max(s[:i]))


def _zooming(s):                                                              # bracketing only grows t: a smaller one is a zoom step
    return sum(1 for i in range(1, len(s)) if s[i] < max(s[:i]))


def _accepted_pairs(r):                                                       # the candidate's slot moves on exactly when the pair is kept
    ps = r["pair_slots"]
    return sum(1 for i in range(len(ps) - 1) if ps[i] != ps[i + 1])


def _stop(r):
    return "max_iter" if r["n_iter"] == r["max_iter"] else ("max_eval" if r["n_eval"] >= r["max_eval"] else "tolerance")


def test_cases_walk_every_path(f32):
    rec = [f32[n] for n in RECORDED]
    assert any(len(s) == 1 for r in rec for s in _iterations(r))
    assert any(_growing(s) >= 3 for r in rec for s in _iterations(r))          # a bracket extended over >= 3 growing t
    assert any(_zooming(s) >= 2 for r in rec for s in _iterations(r))          # >= 2 zoom evaluations in one iteration ...
    assert any(r["max_slot"] >= 3 for r in rec)                                # ... so that four gradient slots are live at once,
    assert any(r["max_slot"] >= 3 and r["T"] == 55 for r in rec)               # also on a row of two blocks
    for hist in (2, 4):
        full = [r for r in rec if r["history"] == hist and r["T"] > 1]
        assert full and all(_accepted_pairs(r) > hist and max(r["n_terms"]) == 2 * hist + 1 for r in full)
    assert {_stop(r) for r in rec if r["n_iter"] > 0} == {"max_iter", "max_eval", "tolerance"}
    for s in K.SETTINGS:
        z = f32[f"{s}_zero"]
        assert (z["n_iter"], z["n_eval"], z["n_vec_ops"]) == (0, 1, 0)         # at the optimum: one evaluation, no vector operation
    # the shapes: inside one block, just under one, two blocks with a short second one
    assert sorted({75 * r["T"] for r in rec}) == [75, 4050, 4125]


# ------------------------------------------------------------------------------------------------------------------- mutations
def _mutations(exe):
    return subprocess.run([exe, "--list-mutations"], check=True, capture_output=True, text=True).stdout.split()


def test_mutation_list(exe):
    want = {"gsum_from_gmax", "dmax_from_g", "direction_after_point", "accept_after_point", "y_swapped", "s_from_new_direction",
            "evict_newest", "pair_over_kept_slot", "first_block_only", "short_row_extended", "last_element_dropped",
            "trial_into_bracket_slot", "s_y_coef_swapped", "dots_fp32", "comb_double", "imu_once"}
    assert want <= set(_mutations(exe)) and len(_mutations(exe)) >= 12


def test_every_mutation_changes_a_recorded_bit(exe, f32):
    for m in _mutations(exe):
        got = _run(exe, "--mutate", m)
        moved = [n for n in RECORDED if any(got[n][k] != f32[n][k] for k in BITS)]
        print(f"{m}: {len(moved)} of {len(RECORDED)} cases move ({', '.join(moved[:4])}{' ...' if len(moved) > 4 else ''})")
        assert moved, m


# --------------------------------------------------------------------------------------------------------------------- fixture
def test_fixture_is_what_the_emulator_prints(f32):
    assert _fixture_of(f32) == K.load_fixture(), "tests/golden/lbfgs_device_trace.json is stale: python tests/test_lbfgs_device_emu_cpu.py"


def test_inputs_in_numpy_are_the_emulator_s(f32):
    """The GPU test regenerates the inputs from the seeds in numpy: the start of a run is x0 itself when nothing moves."""
    z = f32["prod_zero"]
    x0, _, b = K.inputs(z["T"], z["seed"], z["x_scale"])
    assert not x0.any() and not b.any() and not np.array(z["x"], np.uint32).view(np.float32).any()
    # the first loss of every case from the numpy inputs in float64 is the emulator's fp32 first loss to fp32 accuracy: a frame's
    # term is a chain of 75 fp32 additions of terms of a few operations each, unit round-off 2^-24, all terms positive
    for n in RECORDED:
        r = f32[n]
        x0, a, b = K.inputs(r["T"], r["seed"], r["x_scale"])
        loss, _ = K.objective64(x0.astype(np.float64), a.astype(np.float64), b.astype(np.float64))
        first = float(np.array(r["losses"][:1], np.uint32).view(np.float32)[0])
        assert abs(first - loss) <= 80 * 2.0 ** -24 * abs(loss), (n, first, loss)


def test_clang_prints_the_same(f32, tmp_path):
    if CLANG is None:
        pytest.skip("clang++ not available")
    exe2 = _build(CLANG, ["-O3" if f == "-O1" else f for f in FLAGS], tmp_path / "lbfgs_device_emu_clang")
    got = _run(exe2)
    for n in RECORDED:
        assert all(got[n][k] == f32[n][k] for k in BITS), n


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        fx = _fixture_of(_run(_build("g++", FLAGS, os.path.join(tmp, "lbfgs_device_emu"))))
    with open(K.FIXTURE, "w") as f:
        lines = [f'"{n}": {json.dumps(c, separators=(",", ":"))}' for n, c in fx["cases"].items()]         # one case per line
        f.write('{"grid_rows": %d, "grid_max_jobs": %d, "cases": {\n%s\n}}\n' % (fx["grid_rows"], fx["grid_max_jobs"], ",\n".join(lines)))
    print(f"wrote {K.FIXTURE}: {len(fx['cases'])} cases, grid-y case {fx['grid_rows']} rows -> {fx['grid_max_jobs']} jobs")
