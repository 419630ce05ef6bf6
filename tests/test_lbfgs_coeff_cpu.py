"""The coefficient-space L-BFGS that drives the device vectors of the smplify path (csrc/rc_lbfgs_dev.h) against the
vector formulation (csrc/rc_lbfgs.h), which test_lbfgs_host.py pins to torch.optim.LBFGS on these very functions and
starting points. The algorithm only consumes inner products and emits coefficients, so it runs here in float64 over
std::vector (tests/lbfgs_coeff_host.cpp, which also checks every index the algorithm hands its backend). Host code only."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["rosen_lr1", "rosen_lr1e-3", "rosen_short_history", "rosen_history1", "kinked", "kinked_lr1e-3", "at_optimum"]


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path_factory.mktemp("lbfgs_coeff") / "lbfgs_coeff_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "robustcap_amd", "csrc"),
                    os.path.join(ROOT, "tests", "lbfgs_coeff_host.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return {r["name"]: r for r in map(json.loads, out.splitlines())}


def test_all_cases_ran(records):
    assert sorted(records) == sorted(CASES)


@pytest.mark.parametrize("name", CASES)
def test_matches_vector_formulation(records, name):
    co, ho = records[name]["coeff"], records[name]["host"]
    assert (co["n_iter"], co["n_eval"]) == (ho["n_iter"], ho["n_eval"])                       # same iteration / evaluation counts
    assert len(co["losses"]) == co["n_eval"] == len(ho["losses"])
    assert np.allclose(co["losses"], ho["losses"], rtol=1e-6, atol=1e-12)                     # same trial points
    assert np.allclose(co["x"], ho["x"], rtol=1e-6, atol=1e-8)


def test_cases_exercise_the_search(records):
    """The comparison means something: the long runs take many iterations with more than one evaluation each, the
    short-history runs evict (more accepted pairs than the history holds), the start at the optimum stops at once."""
    assert records["at_optimum"]["host"]["n_eval"] == 1 and records["at_optimum"]["host"]["n_iter"] == 0
    for name, hist in (("rosen_short_history", 4), ("rosen_history1", 1)):
        h = records[name]["host"]
        assert h["n_iter"] > hist + 10 and h["n_eval"] > h["n_iter"]
