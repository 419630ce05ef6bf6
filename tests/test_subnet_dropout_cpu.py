"""The dropout masks of a trainable sub-net without a GPU: the generator against Random123's known answers, the dropped share of the
mask rc_dropout.hip draws (tests/subnet_dropout_ref.py restates it), the threshold and scale, the restated forward against torch's own
modules, and the host side of the trainer's dropout state."""
import numpy as np
import pytest
import torch

import subnet_dropout_ref as R
from robustcap_amd import config as cfg
from robustcap_amd import train

# Random123's kat_vectors for philox4x32-10: counter, key, output
KAT = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


@pytest.mark.parametrize("counter,key,out", KAT)
def test_philox_known_answers(counter, key, out):
    assert tuple(int(v) for v in R.philox4x32_10(counter, key)) == out


def test_philox_is_elementwise():
    """Arrays of counters give what the same counters give one at a time (the mask is drawn from arrays)."""
    rng = np.random.default_rng(0)
    c = rng.integers(0, 1 << 32, size=(4, 5), dtype=np.uint64)
    both = R.philox4x32_10(tuple(c), (7, 9))
    for i in range(5):
        one = R.philox4x32_10(tuple(int(v) for v in c[:, i]), (7, 9))
        assert [int(v[i]) for v in both] == [int(v) for v in one]


def test_counter_fields():
    """(row, unit >> 2, site, call) and the key's halves each move the bits; lane j serves unit 4 (unit >> 2) + j."""
    b = R.bits(3, 8, 1, (5 << 32) | 6, 2)
    for r in range(3):
        for q in range(2):
            assert [int(v) for v in R.philox4x32_10((r, q, 1, 2), (6, 5))] == [int(v) for v in b[r, 4 * q:4 * q + 4]]
    assert not np.array_equal(b, R.bits(3, 8, 0, (5 << 32) | 6, 2)) and not np.array_equal(b, R.bits(3, 8, 1, (5 << 32) | 6, 3))
    assert not np.array_equal(b, R.bits(3, 8, 1, (6 << 32) | 5, 2))


@pytest.mark.parametrize("p,T,s_bits", [(0.4, 1717986944, 0x3FD55555), (0.1, 429496736, 0x3F8E38E4)])
def test_threshold_and_scale(p, T, s_bits):
    """T = llrint((double)(float)p 2^32): 0.4f = 0x3ECCCCCD = 13421773 / 2^25, 0.1f = 0x3DCCCCCD = 13421773 / 2^27, so T = 13421773 * 128
    and 13421773 * 32 exactly. s = (float)(1 / (1 - (double)p)): the float nearest the exact quotient (1 - (double)p is exact, the
    division and the narrowing each round once; neither of these two lands on a tie)."""
    from fractions import Fraction
    assert 13421773 * 128 == 1717986944 and 13421773 * 32 == 429496736
    assert R.threshold(p) == T
    s = R.scale(p)
    assert s.dtype == np.float32 and int(s.view(np.uint32)) == s_bits
    exact = 1 / (1 - Fraction(float(np.float32(p))))
    for other in (np.nextafter(s, np.float32(0)), np.nextafter(s, np.float32(2))):
        assert abs(Fraction(float(s)) - exact) < abs(Fraction(float(other)) - exact)
    assert R.threshold(0.0) == 0 and R.scale(0.0) == np.float32(1.0)


@pytest.mark.parametrize("rows,cols,p", [(467, 512, 0.4), (467, 512, 0.1), (109, 1280, 0.4)])
@pytest.mark.parametrize("site", [0, 1])
def test_dropped_share(rows, cols, p, site):
    """Seed 1234, call 1: the dropped count of the whole mask, of every row and of every column within 5 sigma of its expectation,
    sigma = sqrt(n p (1 - p)). (Measured: totals within 1.8 sigma, worst row 3.4, worst column 3.6.)"""
    q = float(np.float32(p))
    dropped = ~R.mask(rows, cols, site, p, 1234, 1)
    z = lambda count, n: np.abs(count - n * q) / np.sqrt(n * q * (1 - q))
    zt, zr, zc = z(dropped.sum(), rows * cols), z(dropped.sum(1), cols).max(), z(dropped.sum(0), rows).max()
    print(f"DROPPED [{rows}, {cols}] p={p} site={site}: total {zt:.2f} sigma, worst row {zr:.2f}, worst column {zc:.2f}")
    assert zt <= 5 and zr <= 5 and zc <= 5


def test_scaled_mask_values():
    m = R.scaled_mask(17, 512, 0, 0.4, 99, 3)
    assert m.dtype == np.float32 and set(np.unique(m).tolist()) == {0.0, float(R.scale(0.4))}
    assert not np.signbit(m).any()
    assert np.array_equal(m != 0, R.mask(17, 512, 0, 0.4, 99, 3))
    assert R.mask(4, 8, 0, 0.0, 1, 1).all()


def test_restated_forward_is_torchs_in_eval_mode():
    """With masks of ones the restatement is nn.Linear + nn.LSTM(2 layers) over a packed sequence + nn.Linear, in float64."""
    from torch.nn.utils.rnn import pack_sequence, pad_packed_sequence
    g = torch.Generator().manual_seed(0)
    nin, H, nout, lengths = 6, 8, 3, [3, 7, 1, 5]
    l1, l2, rnn = torch.nn.Linear(nin, H).double(), torch.nn.Linear(H, nout).double(), torch.nn.LSTM(H, H, 2).double()
    P = {"linear1.weight": l1.weight, "linear1.bias": l1.bias, "linear2.weight": l2.weight, "linear2.bias": l2.bias}
    P.update({f"rnn.{k}": v for k, v in rnn.named_parameters()})
    xs = [torch.randn(T, nin, generator=g, dtype=torch.float64) for T in lengths]
    h0, c0 = torch.randn(2, 4, H, generator=g, dtype=torch.float64), torch.randn(2, 4, H, generator=g, dtype=torch.float64)
    ones = torch.ones(sum(lengths), H, dtype=torch.float64)
    with torch.no_grad():
        y, hn, cn = R.forward_train(P, torch.cat(xs), lengths, h0, c0, ones, ones)
        out, (rh, rc) = rnn(pack_sequence([torch.relu(l1(x)) for x in xs], enforce_sorted=False), (h0, c0))
        out, _ = pad_packed_sequence(out)
        ref = torch.cat([l2(out[:T, i]) for i, T in enumerate(lengths)])
    assert float((y - ref).abs().max()) < 1e-12 and float((hn - rh).abs().max()) < 1e-12 and float((cn - rc).abs().max()) < 1e-12


def test_restated_forward_applies_the_masks_at_the_two_sites():
    """Against torch's modules with the dropout written out: the site-0 mask on relu(linear1), the site-1 mask on layer 0's output as
    layer 1's input only (layer 0's recurrent h and final state are unmasked)."""
    g = torch.Generator().manual_seed(1)
    nin, H, nout, T = 5, 8, 2, 6
    l1, l2 = torch.nn.Linear(nin, H).double(), torch.nn.Linear(H, nout).double()
    r0, r1 = torch.nn.LSTM(H, H, 1).double(), torch.nn.LSTM(H, H, 1).double()
    P = {"linear1.weight": l1.weight, "linear1.bias": l1.bias, "linear2.weight": l2.weight, "linear2.bias": l2.bias}
    for l, r in enumerate((r0, r1)):
        P.update({f"rnn.{k[:-1]}{l}": v for k, v in r.named_parameters()})
    x = torch.randn(T, nin, generator=g, dtype=torch.float64)
    m0 = torch.from_numpy(R.scaled_mask(T, H, 0, 0.4, 5, 0)).double()
    m1 = torch.from_numpy(R.scaled_mask(T, H, 1, 0.4, 5, 0)).double()
    z = torch.zeros(2, 1, H, dtype=torch.float64)
    with torch.no_grad():
        y, hn, cn = R.forward_train(P, x, [T], z, z, m0, m1)
        a, (h_0, c_0) = r0((torch.relu(l1(x)) * m0)[:, None])
        b, (h_1, c_1) = r1(a * m1[:, None])
        ref = l2(b[:, 0])
    assert float((y - ref).abs().max()) < 1e-12
    assert float((hn - torch.cat([h_0, h_1])).abs().max()) < 1e-12 and float((cn - torch.cat([c_0, c_1])).abs().max()) < 1e-12


class _NoNet:
    """What SubnetTrainer's dropout state needs of a Net: nothing."""


def _bare_trainer(name):
    tr = train.SubnetTrainer.__new__(train.SubnetTrainer)
    tr._net, tr.name = _NoNet(), name
    tr.training, tr.dropout, tr._seed, tr._call = False, float(cfg.DROPOUT[name]), 0, 0
    return tr


def test_config_rates_are_the_references():
    """net/sig_mp.py:52-81."""
    assert cfg.DROPOUT == {"rnn2": 0.4, "rnn3": 0.4, "rnn4": 0.4, "rnn6": 0.4, "rnn7": 0.1, "rnn8": 0.4}


def test_dropout_state_layout():
    tr = _bare_trainer("rnn7")
    assert tr.training is False and tr.dropout == 0.1
    assert tr.dropout_state() == {"seed": 0, "call": 0}
    assert tr.train() is tr and tr.training is True and tr.eval() is tr and tr.training is False
    assert tr.train(False) is tr and tr.training is False
    assert tr.manual_seed((1 << 63) + 5) is tr
    tr.train()
    assert tr._next_dropout() == (0.1, (1 << 63) + 5, 0) and tr._next_dropout() == (0.1, (1 << 63) + 5, 1)
    state = tr.dropout_state()
    assert state == {"seed": (1 << 63) + 5, "call": 2} and all(type(v) is int for v in state.values())
    with torch.no_grad():
        assert tr._next_dropout() == train.NO_DROPOUT
    tr.eval()
    assert tr._next_dropout() == train.NO_DROPOUT
    tr.train().dropout = 0.0
    assert tr._next_dropout() == train.NO_DROPOUT
    assert tr.dropout_state() == state                                  # none of the three advanced the counter
    tr.dropout = 0.25
    tr.manual_seed(3)
    assert tr.dropout_state() == {"seed": 3, "call": 0}
    tr.set_dropout_state(state)
    assert tr._next_dropout() == (0.25, (1 << 63) + 5, 2)
    for bad in ({"seed": -1, "call": 0}, {"seed": 1 << 64, "call": 0}, {"seed": 0, "call": 1 << 32}, {"seed": 0, "call": -1}):
        with pytest.raises(ValueError):
            tr.set_dropout_state(bad)
    for bad in (1.0, -0.1, float("nan")):
        tr.dropout = bad
        with pytest.raises(ValueError):
            tr._next_dropout()
    assert tr.dropout_state() == {"seed": (1 << 63) + 5, "call": 3}
