"""The lean live frame against the frame-stepped plan, bit for bit -- TEST INFRASTRUCTURE, NOT PRODUCT.

csrc/rc_live.hip sums every linear2 as per-tile partial products in an order of its own (live_lstm_body -> LiveSum), the
frame-stepped plan runs a GEMM: on a generic state dict the two differ by rounding from the second lean frame on, and nothing
tighter than a flat tolerance can be asked (tests/test_gpu_live.py). The state dict of this module is generic everywhere EXCEPT
linear2.weight, where every row holds at most one non-zero entry, +-2^e with e in {-1, 0, 1}:

    y[o] = fl(+-2^e h[u(o)] + b[o])        in every summation order

(one exact product, exact zeros, ONE rounding at the bias). The sub-net outputs of the two plans are then the same bits, and if
the contract written at the top of rc_live.hip holds -- layer steps bitwise those of the frame-stepped plan, lin1_tile the
arithmetic of gemm_tile<1, 1>, K4's fuse the arithmetic of rc_fuse_kernel -- so is everything behind them, for whole sequences,
with generic W1, W_ih, W_hh and biases. A row that picks unit u also pins the bookkeeping of the partial sums: a tile dropped,
doubled or misplaced, or a wrong lane of w2, leaves y[o] its bias or another unit's h.

  exact_sum_state_dict   synth.make_state_dict with the six linear2.weight replaced; `pick` chooses u(o), sign and exponent
  CASES / motion         the scripted sequences of tests/test_gpu_live_exact.py (legs x batch sizes), one pick each
  oracle_run             the float32 CPU oracle on a case: every linear2's input and output, gate pre-activations, regimes
  sum_orders / lean_linear2   one linear2 in float32 in index order, reversed, pairwise and in the lean order of either tile width
  layer_step_f32 / fuse_f32   float32 restatements of one layer step (the K split of live_lstm_body) and of the fuse's product
"""
import dataclasses

import numpy as np
import torch

from robustcap_amd import config as C
from robustcap_amd import synth
from . import sig_mp_oracle as O
from .wiring_f64 import _vm

F32, F64 = np.float32, np.float64
NET_NAMES = tuple(n[0] for n in C.NETS)
SPEC = {n: (i, h, o) for n, i, h, o in C.NETS}

# The operating point (tests/test_live_exact_cpu.py asserts these on the oracle's run of the two `full` cases, weight seed 0):
# at gain 1 the synthetic LSTMs idle (h a few 1e-2); GAIN scales every generic tensor so that each net has gate pre-activations
# beyond |2| and within |0.1| and |h| >= 0.3 somewhere -- sigmoid and tanh work on their curved parts and the products of the cell
# update have full-size operands -- without saturating them (at gain 2.5 the largest gate sums are 15-30 and |h| reaches 1.0
# in every net: a saturated gate forgets the last bits of its sum). At GAIN = 1.5, weight seed 0, cases aql_b1 / aql_b4:
#   largest |gate|  rnn2 9.3 / 11.8  rnn3 9.0 / 6.9  rnn4 8.4 / 7.2  rnn6 5.9 / 5.1  rnn7 7.6 / 7.1  rnn8 6.9 / 8.0
#   smallest |gate| <= 2e-6 in every net; largest |h| 0.92 .. 0.995; smallest non-zero |h| read by a linear2 8.5e-8 (normal)
GAIN = 1.5
WEIGHT_SEED = 0

# ---- the geometry of the lean frame's sums (csrc/rc_live.hip: LiveSum<OUTP, MAXT> in rc_live_k4 / rc_live_k7) -----------------
# OUTP = out rounded up to 4; G = OUTP / 4 column groups; S = min(256 / G, 32) slices; slice sl owns tiles sl, sl + S, ...;
# tiles are UT = 4 (16 x 16 LSTM tiles) or 8 (RC_LIVE_LEAN_NC=2) hidden units wide. Narrow sums (OUTP = 4) meet by a butterfly.
MAXT = {"rnn4": 23, "rnn2": 10, "rnn7": 19, "rnn6": 8, "rnn3": 4, "rnn8": 4}


def geometry(net):
    """(H, out, OUTP, S) of sub-net `net`'s linear2 sum."""
    _, H, out = SPEC[net]
    outp = (out + 3) // 4 * 4
    G = outp // 4
    return H, out, outp, min(256 // G, 32)


def required_units(net):
    """Hidden units whose selection exercises every edge of the sum: unit 0 and H - 1, the tile boundaries of both widths
    (3, 4, 7, 8), every position 0..7 within a tile, and for UT = 4 and 8 a unit in tile S - 1, in tile S (the first a slice
    reaches with q = 1), in the last tile of slice S - 1 and in the last tile of all (the largest q of the sum)."""
    H, _, _, S = geometry(net)
    req = [0, H - 1, 3, 4, 7, 8, 1, 2, 5, 6]
    for ut in (4, 8):
        nt = H // ut
        assert -(-nt // S) <= MAXT[net], (net, ut)
        last_of_last_slice = (S - 1) + ((nt - 1 - (S - 1)) // S) * S
        for tile in (S - 1, S, last_of_last_slice, nt - 1):
            req.append(tile * ut + tile % ut)
    out = []
    for u in req:
        if u not in out:
            out.append(u)
    return out


def pick_units(net, pick):
    """u(o) for every output row of `net` under pick number `pick` (0, 1, 2, ...).
    Narrow outputs (2 or 3 rows) walk through required_units, `out` of them per pick. Wide outputs: pick 0 places a unit in every
    4-unit tile from tile 0 as far as the rows reach (all 128 tiles of rnn7) and fills up with required units; every other pick
    selects all required units first and sweeps the following tiles with the rest, so that the picks together reach every tile."""
    H, out, _, _ = geometry(net)
    req = required_units(net)
    if out <= 4:
        return [req[(pick * out + o) % len(req)] for o in range(out)]
    nt4 = H // 4
    sweep = lambda i, start: 4 * ((start + i) % nt4) + (i + pick) % 4
    if pick == 0:
        n = min(out, nt4)
        return [sweep(i, 0) for i in range(n)] + [req[j % len(req)] for j in range(out - n)]
    rest = out - len(req)
    start = min(out, nt4) + (pick - 1) * rest
    return list(req) + [sweep(i, start) for i in range(rest)]


def exact_sum_state_dict(seed, gain, pick, base=None):
    """synth.make_state_dict(seed, gain) -- its linear2.bias kept: they carry the operating range -- with every linear2.weight
    replaced: row o holds sign(o) 2^e(o) in column u(o) (pick_units), sign and e in {-1, 0, 1} seeded, and zeros.
    `base`: that make_state_dict(seed, gain), when the caller builds several picks (its arrays are shared, not copied)."""
    sd = dict(base) if base is not None else synth.make_state_dict(seed, gain)
    for k, net in enumerate(NET_NAMES):
        H, out, _, _ = geometry(net)
        u = synth.uniform01(seed * 1009 + 17 * pick + 3, 500 + k, 2 * out)
        w = np.zeros((out, H), np.float32)
        for o, unit in enumerate(pick_units(net, pick)):
            w[o, unit] = (1.0 if u[2 * o] < 0.5 else -1.0) * 2.0 ** (int(u[2 * o + 1] * 3.0) - 1)
        sd[f"{net}.linear2.weight"] = w
    return sd


# ---- the scripted sequences ------------------------------------------------------------------------------------------------------
LEGS = {                                   # environment of the live net; the twin is the frame-stepped plan in gemm mode 0
    "aql": {},                                                           # AQL chain, hot argument words
    "graph": {"RC_LIVE_AQL": "0"},                                       # graph replay, hot = 0
    "nc2": {"RC_LIVE_LEAN_NC": "2"},                                     # 16 x 32 tiles
    "nc2_graph": {"RC_LIVE_LEAN_NC": "2", "RC_LIVE_AQL": "0"},
    "prestep": {"RC_LIVE_PRESTEP_IDLE_US": "0"},                         # a pre-step behind every frame (from_pre)
}
CONF_LO, CONF_HI = 0.7, 0.8
HUG_LO = (0.7, 0.70001, 0.69999, 0.7, 0.9, 0.69995, 0.70005, 0.5)
HUG_HI = (0.8, 0.80001, 0.79999, 0.8, 0.79995, 0.80005)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    leg: str
    B: int
    T: int
    pick: int
    full: bool = False          # the oracle's run keeps every step's inputs and gate pre-activations (operating point, mutations)

    @property
    def env(self):
        return LEGS[self.leg]

    @property
    def motion_seed(self):
        return 700 + 13 * self.pick


def _cases():
    out = []
    for leg in LEGS:
        for B in ((1, 4, 2, 3) if leg == "aql" else (1, 4)):
            out.append(Case(f"{leg}_b{B}", leg, B, {1: 56, 4: 48}.get(B, 28), len(out), full=(leg == "aql" and B in (1, 4))))
    return tuple(out)


CASES = _cases()


def conf_script(case):
    """[B, T] mean confidences and the frames whose 33 confidences are all equal (the thresholds hugged)."""
    B, T = case.B, case.T
    c = np.full((B, T), 0.75)
    hug = np.zeros((B, T), bool)
    if B == 1:      # visible, an occluded stretch (the deferred updater step rides lean frames), conf_lo and conf_hi hugged, high
        c[0, 10:22] = 0.4
        c[0, 26:34], hug[0, 26:34] = HUG_LO, True
        c[0, 37:43], hug[0, 37:43] = HUG_HI, True
        c[0, 43:] = 0.9
    elif B == 4:    # rows in different regimes per frame
        c[0, 14:30] = 0.9                                  # mid -> high (init_net) -> mid, then conf_lo hugged
        c[0, 38:42], hug[0, 38:42] = HUG_LO[:4], True
        c[1, 10:28] = 0.45                                 # occluded while the others see the camera
        c[1, 34:] = 0.86
        c[2, :] = 0.95                                     # always high
        c[3, 4:] = 0.3                                     # occluded for good: rnn4 / rnn6 step on the updater's rows only
    else:           # the shortened script: ri = i < B ? i : B - 1 and amask have their edges at B = 2 and 3
        c[0, 14:] = 0.9
        c[1, 6:17] = 0.4
        if B == 3:
            c[2, :] = 0.93
            c[2, 20:24], hug[2, 20:24] = HUG_HI[:4], True
    return c, hug


def motion(case, body):
    """synth.make_motion with the case's confidences: a seeded zero-mean spread over the 33 keypoints, none on the hugged frames."""
    m = synth.make_motion(case.motion_seed, case.B, case.T, body, conf="mid")
    c, hug = conf_script(case)
    for b in range(case.B):
        dk = 0.03 * (synth.uniform01(case.motion_seed + 31 * b, 77, case.T * 33).reshape(case.T, 33).astype(np.float64) - 0.5)
        dk -= dk.mean(1, keepdims=True)
        dk[hug[b]] = 0.0
        m["j2dc"][b, :, :, 2] = (c[b][:, None] + dk).astype(np.float32)
    return m


# ---- the float32 oracle's run -----------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Step:
    frame: int
    net: str
    rows: np.ndarray            # the rows that stepped
    h1: np.ndarray              # [n, H] float32: layer 1's new h, what linear2 reads
    y: np.ndarray               # [n, out] float32: the oracle's own linear2
    x: np.ndarray = None        # full cases: the sub-net's input, the states before and after, the gate pre-activations
    hp: np.ndarray = None
    cp: np.ndarray = None
    hn: np.ndarray = None
    gates: tuple = None


def oracle_run(case, body, sd=None):
    """The float32 OracleNet on the case: (steps, frames) -- every sub-net step in call order, and per frame the regime of every
    row, rnn4 / rnn6 step counts, init_net rows, and the Rcr / j3dc of the fuse."""
    sd = sd if sd is not None else exact_sum_state_dict(WEIGHT_SEED, GAIN, case.pick)
    m = motion(case, body)
    B = case.B
    ora = O.OracleNet(body, batch=B)
    ora.load_numpy_state_dict(sd)
    ora.gravityc = torch.from_numpy(m["gravityc"])
    steps, inner, now = [], ora._step, [0]

    def spy(name, x, rows=None):
        idx = torch.arange(B) if rows is None else rows
        if idx.numel() == 0:
            return inner(name, x, rows)
        hp, cp = ora.h[name][:, idx].clone(), ora.c[name][:, idx].clone()
        y = inner(name, x, rows)
        hn = ora.h[name][:, idx].clone()
        st = Step(now[0], name, idx.numpy().copy(), hn[1].numpy().copy(), y.numpy().copy())
        if case.full:
            mod = getattr(ora, name)
            xs = x if rows is None else x[rows]
            a, gates = torch.relu(mod.linear1(xs)), []
            for l in range(2):
                r = mod.rnn
                g = (a @ getattr(r, f"weight_ih_l{l}").T + hp[l] @ getattr(r, f"weight_hh_l{l}").T
                     + getattr(r, f"bias_ih_l{l}") + getattr(r, f"bias_hh_l{l}"))
                gates.append(g.numpy().copy())
                a = hn[l]
            st.x, st.hp, st.cp, st.hn, st.gates = xs.numpy().copy(), hp.numpy().copy(), cp.numpy().copy(), hn.numpy().copy(), tuple(gates)
        steps.append(st)
        return y

    ora._step = spy
    frames = []
    t = torch.from_numpy
    for i in range(case.T):
        now[0] = i
        ora.forward_batch(t(m["j2dc"][:, i]), t(m["accc"][:, i]), t(m["oric"][:, i]), None, i == 0)
        tr = ora.trace
        c64 = tr["c"].numpy()
        frames.append(dict(regime=np.where(c64 >= CONF_HI, 2, np.where(c64 > CONF_LO, 1, 0)), c=c64.copy(), n4=tr["n4"].numpy().copy(),
                           n6=tr["n6"].numpy().copy(), reach=tr["reach"].numpy().copy(), j3dc=tr["j3dc"].clone(),
                           Rcr=t(m["oric"][:, i, 5]).clone()))
    return steps, frames


def plan_of_frames(frames):
    """Per frame, what the device does with it, from the oracle's trace. The reference runs the vision updater's two steps at the end
    of an occluded frame (L264-271); the device defers them to the start of the next frame. There the row either is occluded again
    -- the deferred step RIDES the frame's own rnn4 / rnn6 launches, lean plan or not -- or steps on camera data as well, which
    takes the three transition launches and the frame off the lean plan; so do the first frame and a row's init_net.
    Returns a list of dict(lean, ride [B], idle [B]: rnn4 / rnn6 computed and discarded on a lean frame, transition [B], init_net [B])."""
    out, pend = [], np.zeros(len(frames[0]["regime"]), bool)
    for i, f in enumerate(frames):
        vis = (f["regime"] > 0) | (i == 0)
        transition, ride = pend & vis, pend & ~vis
        lean = i > 0 and not transition.any() and not f["reach"].any()
        out.append(dict(lean=lean, ride=ride & lean, idle=~vis & ~pend & lean, transition=transition, init_net=f["reach"].copy()))
        pend = f["regime"] == 0                      # (not live: the updater refreshes on every occluded frame)
    return out


# ---- one linear2 in float32, in several orders ------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays: the product is exact in float64; exact as a whole whenever the product or the addend is
    zero (all this dict ever presents to it), otherwise within a double rounding of fmaf."""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def _seq_sum(p):
    return np.add.accumulate(p, axis=-1, dtype=F32)[..., -1]


def sum_orders(W2, b2, h):
    """{order: y [N, out] float32} of y = W2 h + b2 for h [N, H]: index order, reversed, pairwise (bias last in each)."""
    p = (W2[None].astype(F32) * h[:, None, :].astype(F32)).astype(F32)
    out = {"index": _seq_sum(p) + b2, "reversed": _seq_sum(p[..., ::-1]) + b2}
    n = 1
    while n < p.shape[-1]:
        n *= 2
    q = np.zeros(p.shape[:-1] + (n,), F32)
    q[..., :p.shape[-1]] = p
    while q.shape[-1] > 1:
        q = q[..., 0::2] + q[..., 1::2]
    out["pairwise"] = q[..., 0] + b2
    return {k: v.astype(F32) for k, v in out.items()}


MUTATIONS = ("tile 0 left out", "last tile left out", "tile S left out", "a tile added twice", "unit index off by one inside a tile",
             "tile count of the other width", "tile count of UT = 4 on UT = 8 partials", "a stale partial taken")


def tile_partials(W2, h, ut, mut=None):
    """[N, out, H / ut] float32: live_lstm_body's partial of every tile -- p = w[0] h[0], then fmaf(w[u], h[u], p) for u = 1 .. ut - 1."""
    out, H = W2.shape
    nt = H // ut
    Wt, ht = W2.reshape(out, nt, ut).astype(F32), h.reshape(-1, nt, ut).astype(F32)
    if mut == "unit index off by one inside a tile":
        ht = np.roll(ht, -1, axis=2)
    p = (Wt[None, :, :, 0] * ht[:, None, :, 0]).astype(F32)
    for u in range(1, ut):
        p = fma32(Wt[None, :, :, u], ht[:, None, :, u], p)
    return p


def live_sum(p, b2, net, nt_used=None):
    """LiveSum over partials p [N, out, tiles in the buffer]: slice sl adds its tiles sl, sl + S, ... < nt_used in ascending order;
    wide sums add the slices in ascending order (finish), narrow ones (OUTP = 4) by the 64-lane xor butterfly (wave_total); bias last."""
    _, _, outp, S = geometry(net)
    nt = p.shape[-1] if nt_used is None else nt_used
    sl = np.arange(S)
    a = np.where(sl < nt, p[..., np.minimum(sl, p.shape[-1] - 1)], F32(0)).astype(F32)
    for q in range(1, MAXT[net]):
        tl = sl + q * S
        ok = tl < nt
        if ok.any():
            a[..., ok] = a[..., ok] + p[..., tl[ok]]
    if outp == 4:
        v = np.zeros(a.shape[:-1] + (64,), F32)
        v[..., :S] = a
        lanes = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[..., lanes ^ off]
        y = v[..., 0]
    else:
        y = a[..., 0]
        for q in range(1, S):
            y = y + a[..., q]
    return (y + b2).astype(F32)


def lean_linear2(W2, b2, h, net, ut, mut=None, h_stale=None):
    """y [N, out] float32 of the lean frame's linear2 for tile width `ut` (4 or 8); `mut`: one of MUTATIONS. `h_stale` [N, H]: what
    the partial buffer still holds from the row's previous step (a stale partial, the never-written half of a buffer)."""
    H, _, _, S = geometry(net)
    nt = H // ut
    p = tile_partials(W2, h, ut, mut)
    nt_used = None
    if mut in ("tile 0 left out", "last tile left out", "tile S left out"):
        p[..., {"tile 0 left out": 0, "last tile left out": nt - 1, "tile S left out": S}[mut]] = 0
    elif mut == "a tile added twice":                      # the tile of unit 7 / 8 (UT = 8 / 4): twice the one non-zero term, exactly
        p[..., 1] = p[..., 1] + p[..., 1]
    elif mut == "tile count of the other width":           # H / 8 tiles summed of the H / 4 written, or H / 4 of a buffer ...
        nt_used = H // (12 - ut)
        if nt_used > nt:                                   # ... whose upper half was never written by this width: zero-filled
            p = np.concatenate([p, np.zeros(p.shape[:-1] + (nt_used - nt,), F32)], axis=-1)
    elif mut == "tile count of UT = 4 on UT = 8 partials": # ... or still holding the UT = 4 partials of an earlier step
        assert ut == 8
        nt_used = H // 4
        p = np.concatenate([p, tile_partials(W2, h_stale, 4)[..., nt:]], axis=-1)
    elif mut == "a stale partial taken":                   # tile 0 of a row that did not step: the previous step's
        p[..., 0] = tile_partials(W2, h_stale, ut)[..., 0]
    return live_sum(p, b2, net, nt_used)


# ---- float32 restatements of one layer step and of the fuse ---------------------------------------------------------------------
def _sig(v):
    return (F32(1) / (F32(1) + np.exp(-v.astype(F32)))).astype(F32)


def layer_step_f32(Wih, Whh, bias, a, h_prev, c_prev, skip=None):
    """One LSTM layer step of one row in float32 with the K split of live_lstm_body (lstm_f64.step's structure): K = [a | h_prev] in
    chunks of 16, wave w owns chunks [w Qw, (w + 1) Qw), each chunk is four MFMA 16x16x4 (k = 16 q + 4 kq + s: the four kq of one s
    form one instruction, modelled as an exact 4-term dot rounded once onto the accumulator), the wave sums are added in wave order,
    then the bias (b_ih + b_hh in float32), the gates (i, f, g, o) and the cell update. `skip` = (wave, chunk): that chunk left out.
    Returns (h, c) float32 [H]."""
    H = h_prev.shape[0]
    Qw = 2 * H // 64
    W = np.concatenate([Wih, Whh], axis=1).astype(F64)
    k = np.concatenate([a, h_prev]).astype(F64)
    d = (W * k[None]).reshape(4 * H, 4, Qw, 4, 4).sum(axis=3)            # [4H, wave, chunk, s]
    acc = np.zeros((4 * H, 4), F32)
    for q in range(Qw):
        for s in range(4):
            step = d[:, :, q, s].copy()
            if skip is not None and skip[1] == q:
                step[:, skip[0]] = 0.0
            acc = (acc.astype(F64) + step).astype(F32)
    g = (((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]) + bias.astype(F32)
    i, f, gg, o = g[:H], g[H:2 * H], g[2 * H:3 * H], g[3 * H:]
    c = (_sig(f) * c_prev.astype(F32) + _sig(i) * np.tanh(gg).astype(F32)).astype(F32)
    return (_sig(o) * np.tanh(c).astype(F32)).astype(F32), c


def fuse_f32(j3dc, Rcr, fused=False):
    """j3dc.view(23, 3).mm(Rcr) of every row in float32 ([B, 69] torch, [B, 3, 3] torch -> [B, 69] numpy): the three-term product as
    fuse_body and rc_live_k4 write it, (v0 R0c + v1 R1c) + v2 R2c with every product rounded (wiring_f64._vm), or with the two
    additions contracted into fmaf."""
    v = j3dc.view(-1, 23, 3)
    if not fused:
        return _vm(v, Rcr, False)[0].reshape(-1, 69).numpy()
    a, R = v.numpy()[:, :, :, None], Rcr.numpy()[:, None, :, :]          # [B, 23, k, 1] x [B, 1, k, c]
    p = (a[:, :, 0] * R[:, :, 0]).astype(F32)
    p = fma32(a[:, :, 1], R[:, :, 1], p)
    return fma32(a[:, :, 2], R[:, :, 2], p).reshape(-1, 69)
