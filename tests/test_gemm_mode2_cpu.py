"""Gemm mode 2 (two round-to-nearest bf16 terms per operand, three products) priced on the CPU, from its specification
(tests/gemm_mode2_ref.py) -- no GPU.

The bound of mode 2 is oracle/lstm_f64.Bound with every tolerance multiplied by ONE factor G = 8, fixed here from the emulation
and never from the device. Over the six nets at B = 37 and 256 (five steps, one masked: test_gemm_bound_cpu.schedule) the
arithmetic as specified measures 2.6 .. 3.4 x the unscaled bound and the weakest mutation, truncated terms, 18.6 .. 21.4 x:
every G in 6.7 .. 9.3 puts the former at or below half of the scaled bound and the latter at or above twice it; 8 is the power of
two in that range. The other mutations are far out (a_mid.w_hi dropped ~900 .. 1200 x, a_hi.w_mid dropped on the layer-input half
of K ~790 .. 970 x, mid rounded from a ~2e6 x). One G separates all four mutations on all twelve cases.

End to end, the CPU oracle with every sub-net GEMM in this arithmetic stays within the project's budget (1e-4 m, 0.1 deg) of the
fixtures with exact branch traces, and within a quarter of it: measured 7.4e-6 m / 1.1e-4 deg at worst over all fifteen fixtures,
against 6.5e-5 m / 1.0e-3 deg with truncated terms. Measured on the seeded synthetic weights of the fixtures; trained weights have
not been tried.
"""
import os

import numpy as np
import pytest
import torch

import gemm_mode2_ref as M
from oracle import sig_mp_oracle as O
from robustcap_amd import config as C, synth

G = 8.0                      # mode 2's bound = G x lstm_f64.Bound (module docstring: where 8 comes from)
NETS = [n for n, _, _, _ in C.NETS]
CASES = [(n, B) for n in NETS for B in (37, 256)]
BUDGET_M, BUDGET_DEG = 1e-4, 0.1


@pytest.fixture(scope="module")
def sd():
    return synth.make_state_dict(0)


@pytest.fixture(scope="module", autouse=True)
def _blas_threads():
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        yield
        return
    with threadpool_limits(limits=16):
        yield


# ------------------------------------------------------------------------------------------------------- the split
def _probe_values():
    """random values of many magnitudes, exact ties (bit 15 set, the bits below clear) above even and odd bf16, the values just
    beside them, both signs, fp32 denormals and zeros"""
    r = synth.normal(11, 3, 8192).astype(np.float32) * np.float32(10.0) ** (np.arange(8192) % 13 - 6).astype(np.float32)
    hi = (np.arange(0x3F00, 0x3F80, dtype=np.uint32) << np.uint32(16))           # even and odd bf16 mantissas
    ties = np.concatenate([hi | np.uint32(0x8000), hi | np.uint32(0x7FFF), hi | np.uint32(0x8001), hi]).view(np.float32)
    den = np.array([1, 2, 0x7FFF, 0x8000, 0x8001, 0x18000, 0x28000, 0x7FFFFF, 0x800000, 0x807FFF, 0x808000], np.uint32).view(np.float32)
    v = np.concatenate([r, ties, den, np.zeros(1, np.float32)])
    return np.concatenate([v, -v])


def test_rn_bf16_is_torch_bfloat16():
    v = _probe_values()
    want = torch.from_numpy(v).to(torch.bfloat16).to(torch.float32).numpy()
    got = M.rn_bf16(v)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.all((got.view(np.uint32) & np.uint32(0xFFFF)) == 0)
    assert np.isnan(M.rn_bf16(np.array([np.nan], np.float32))[0])
    # |a| within half a bf16 ulp of FLT_MAX rounds to inf where truncation does not (documented in the header)
    big = np.array([np.finfo(np.float32).max], np.float32)
    assert np.isinf(M.rn_bf16(big)[0]) and np.isfinite(M.trunc_bf16(big)[0])


def test_split2_keeps_two_terms_and_nothing_below():
    v = _probe_values()
    hi, mid = M.split2_rn(v)
    a = v.astype(np.float64)
    # within 2^-16 |a| -- or, where mid falls among the bf16 denormals (|a| below ~2^-118), half their spacing of 2^-133
    assert np.all(np.abs(a - (hi.astype(np.float64) + mid)) <= np.maximum(2.0 ** -16 * np.abs(a), 2.0 ** -134))
    normal = np.abs(a) >= 2.0 ** -110
    assert np.all(np.abs(a - (hi.astype(np.float64) + mid))[normal] <= 2.0 ** -16 * np.abs(a)[normal])
    assert np.array_equal(M.rn_bf16(hi), hi) and np.array_equal(M.rn_bf16(mid), mid)
    # a - hi is exact in fp32
    assert np.array_equal((v - hi).astype(np.float64), a - hi.astype(np.float64))
    # the truncated split is the weaker one: up to 2^-15 |a| with the same two terms
    th, tm = M.split2_mutated(v, "trunc")
    assert np.max(np.abs(a - (th.astype(np.float64) + tm)) / np.maximum(np.abs(a), 1e-300)) > 2.0 ** -16


def test_gemm3_is_the_three_products():
    a = synth.normal(5, 1, 7 * 96).reshape(7, 96).astype(np.float32)
    w = synth.normal(5, 2, 9 * 96).reshape(9, 96).astype(np.float32)
    ah, am = (t.astype(np.float64) for t in M.split2_rn(a))
    wh, wm = (t.astype(np.float64) for t in M.split2_rn(w))
    want = (am @ wh.T + ah @ wm.T + ah @ wh.T).astype(np.float32)
    assert np.array_equal(M.gemm3(a, w), want)
    exact = a.astype(np.float64) @ w.astype(np.float64).T
    scale = np.abs(a).astype(np.float64) @ np.abs(w).astype(np.float64).T
    assert np.all(np.abs(M.gemm3(a, w) - exact) <= (3 * 2.0 ** -16 + 2.0 ** -23) * scale)


# ------------------------------------------------------------------------------------------------------- the bound
@pytest.mark.parametrize("name,B", CASES, ids=[f"{n}-B{B}" for n, B in CASES])
def test_scaled_bound_passes_mode2_and_rejects_mutations(sd, name, B):
    """As specified: at or below 1/2 of G x Bound. Truncated terms, a_mid.w_hi dropped, a_hi.w_mid dropped on the layer-input
    half of K, mid rounded from a: each at or above 2 x it. (All four are separated by G = 8 on all twelve cases.)"""
    got = {"as_specified": M.worst_ratio(sd, name, B, M.Emulated2(sd, name, B)) / G}
    for m in M.MUTATIONS:
        got[m] = M.worst_ratio(sd, name, B, M.Emulated2(sd, name, B, m)) / G
    print(name, B, {k: round(v, 3) for k, v in got.items()})
    assert got["as_specified"] <= 0.5, (name, B, got)
    for m in M.MUTATIONS:
        assert got[m] >= 2.0, (name, B, m, got[m])


# ------------------------------------------------------------------------------------------------------- end to end
class EmulatedNet(O.OracleNet):
    """The CPU oracle with every sub-net GEMM (linear1, both LSTM layers, linear2, init_net) in mode 2's arithmetic."""

    def __init__(self, body, sd, mutation=None):
        super().__init__(body, batch=1)
        self.load_numpy_state_dict(sd)
        self.emu = {n: M.Emulated2(sd, n, 1, mutation) for n in NETS}
        self.init_w = [(np.asarray(sd[f"rnn2.init_net.{2 * q}.weight"], np.float32), np.asarray(sd[f"rnn2.init_net.{2 * q}.bias"], np.float32))
                       for q in range(3)]
        self.mutation = mutation
        net = self

        class InitNet:
            def __call__(self, v):
                a = v.numpy().astype(np.float32)
                for q, (w, b) in enumerate(net.init_w):
                    a = M.gemm3(a, w, net.mutation) + b
                    if q < 2:
                        a = np.maximum(a, np.float32(0.0))
                return torch.from_numpy(a)
        self.rnn2.__dict__["init_net"] = InitNet()          # (an instance attribute in front of the registered module)

    def _step(self, name, x, rows=None):
        if rows is not None and rows.numel() == 0:
            return torch.zeros(0, getattr(self, name).linear2.out_features)
        e = self.emu[name]
        e.h, e.c = self.h[name].numpy(), self.c[name].numpy()      # (views: the emulation steps the oracle's own state)
        y, _, _ = e.step(x.numpy())
        return torch.from_numpy(y)


@pytest.fixture(scope="module")
def whole_model_cached():
    """every matrix of the six nets keeps its float64 terms for the end-to-end runs (1 GB), released behind them"""
    keep, M.WPLANES_MAX = M.WPLANES_MAX, 32
    yield
    M.WPLANES_MAX = keep
    M._WPLANES.clear()


def _run_fixture(path, assets, mutation=None):
    s = np.load(path)
    assert str(s["live"]) == "", path
    net = EmulatedNet(assets["body"], assets["state_dict"], mutation)
    net.use_flat_floor = bool(s["use_flat_floor"])
    net.use_reproj_opt = bool(s["use_reproj_opt"]) if "use_reproj_opt" in s else False
    net.use_vision_updater = bool(s["use_vision_updater"]) if "use_vision_updater" in s else True
    net.use_imu_updater = bool(s["use_imu_updater"]) if "use_imu_updater" in s else True
    t = torch.from_numpy
    net.gravityc = t(s["gravityc"]).view(1, 3)
    ft = t(s["first_tran"]) if s["first_tran"].size else None
    worst_m = worst_deg = 0.0
    for i in range(s["pose"].shape[0]):
        p, tr = net.forward_online(t(s["j2dc"][i]), t(s["accc"][i]), t(s["oric"][i]), ft if i == 0 else None,
                                   bool(s["first_frame"]) and i == 0)
        tc = net.trace
        got = [int(tc["n4"][0]), int(tc["n6"][0]), int(tc["n_floor_add"][0]), int(tc["n_floor"][0]), int(tc["reach"][0])]
        assert got == [int(x) for x in s["trace"][i][1:6]], f"branch trace differs at frame {i} of {os.path.basename(path)}"
        worst_m = max(worst_m, float(np.abs(tr.numpy().astype(np.float64) - s["tran"][i]).max()))
        worst_deg = max(worst_deg, float(O.rotation_angle_deg(p.view(-1, 3, 3), t(s["pose"][i]).view(-1, 3, 3)).max()))
    return worst_m, worst_deg


@pytest.mark.parametrize("fixture", ["seq_threshold_edges", "seq_long_mixed", "seq_reproj_opt"])
def test_oracle_in_mode2_arithmetic_stays_within_a_quarter_of_the_budget(fixture, golden_dir, synth_assets, whole_model_cached):
    worst_m, worst_deg = _run_fixture(os.path.join(golden_dir, fixture + ".npz"), synth_assets)
    print(f"{fixture}: translation {worst_m:.2e} m, joint rotation {worst_deg:.2e} deg")
    assert worst_m <= BUDGET_M and worst_deg <= BUDGET_DEG
    assert worst_m <= BUDGET_M / 4 and worst_deg <= BUDGET_DEG / 4
