"""What every sub-net is fed, and when it steps, in float64 -- TEST INFRASTRUCTURE, NOT PRODUCT.

Between the sub-nets the frame does arithmetic of its own: prep (accr = accc . Rcr, orir = Rcr^T . oric, the bbox-normalised
keypoints, and the column each value lands in: prep_values / prep_store in csrc/rc_frame_dev.h), fuse (j3dc . Rcr, the lerp
with the double weight, the regime selection: fuse_body in csrc/rc_frame.hip, restated by rc_live_k4), the vision updater's
inputs written by the tail (kp = j33 / z, its normalisation, joint[1:] - joint[0]), the input of init_net on first reach, and
the SET of rows on which rnn4 and rnn6 step on each frame. oracle/tail_f64.py cannot see any of it: with zero weights nothing a
sub-net reads reaches an output.

The device that makes it visible is a WIRE laid into tail_f64's state dict. Every output stays its linear2 bias, bitwise (every
linear2.weight, every W_hh and layer 1's weights stay zero), so tail_f64 still describes the tail; but
  linear1   W1[2k, k] = +1, W1[2k+1, k] = -1, b1 = 0: units 2k, 2k+1 hold relu(x_k), relu(-x_k) -- one non-zero product of weight
            +-1 per sum, exact in both GEMM modes;
  layer 0   W_ih[2H + u, u] = s_k (a power of two per column group), everything else zero: i = f = o = 1/2 and
                c_t[u] = c_{t-1}[u] / 2 + tanh(s_k a_u) / 2
            a geometric memory of every step the net took on the row and of what it was fed -- a missed or an extra step, or a
            wrong value sixteen steps back, is still 2^-16 of the signal;
  layer 1   zero weights, small generic gate biases: c1 counts the steps and nothing else;
  init_net  +- pairs in layer 0, the identity on those 138 units in layer 1, and layer 2 copies them into the four quarters of
            its 2048 outputs (h0, h1, c0, c1 of rnn2) with weights 1, 1/2, 1/4, 1/8 -- four different powers of two, so that an
            exchange of quarters shows.
`Net.get_state` then reads every sub-net's input history off the device, on every engine. Two more biases are part of the wire:
rnn2.linear2.bias and rnn4.linear2.bias (j3dr_i and j3dc) are zero in tail_f64's dict, and with them zero the rotation, the lerp
and the regime selection of fuse would have nothing to act on; the tail reads neither.

  build_cases   tail_f64's cases (j2dc, IMU 5, gravity, first_tran, calls, resets untouched: regimes, margins and the tail's
                record stay valid) with IMUs 0-4 replaced by seeded generic rotations and acc by seeded accelerations in +-4
  restate       per frame, the ordered list of sub-net steps (input row, row mask) and reaches, following
                OracleNet.forward_batch L138-167, L178-183, L264-271 line for line, in any dtype and two association orders;
                `mut` names a one-line wrong variant (MUTATIONS)
  run_states    lstm_f64.step over those steps with the wire's parameters: the states of all six nets after every frame
  Bound         per state element, lstm_f64.Bound.tol_hc() plus the input's own bound carried through the wire (see its docstring)
"""
import dataclasses

import numpy as np
import torch

from robustcap_amd import config as C
from robustcap_amd import synth
from . import lstm_f64 as L
from . import sig_mp_oracle as O
from . import tail_f64 as F
from .pose_ops_f64 import bbox_A

F32, F64 = torch.float32, torch.float64
EPS32 = 2.0 ** -24
MARGIN = 3.0            # float32 evaluations at most Bound / MARGIN, mutations at least MARGIN * Bound
# M as in tail_f64 and pose_ops_f64: the smallest power of two above MARGIN (an evaluation that defines e32 sits at 1 / M of its own
# input bound). The CPU figures (profiles/wiring_ratios.txt) do not ask for 8 in any group: the worst float32 evaluation is at
# 0.17 of the Bound (rnn7 / rnn8, whose joint columns carry the rotated and blended values), the weakest mutation at 2.3e3; M was
# fixed from these before the device ran, and the device's worst path sits at 0.17 too.
M = 4.0
NET_NAMES = tuple(n[0] for n in C.NETS)
SPEC = {n: (i, h, o) for n, i, h, o in C.NETS}
ORDERS = F.ORDERS
S_MAX, S_MIN = 8.0, 2.0 ** -24
REACH_Q = (1.0, 0.5, 0.25, 0.125)       # layer 2 of init_net: the weight of the copy into h0, h1, c0, c1

# column groups of each net's input row: (group, first column, one past the last)
GROUPS = {
    "rnn2": (("acc", 0, 18), ("ori", 18, 72)),
    "rnn3": (("acc", 0, 18), ("ori", 18, 72), ("joints", 72, 141)),
    "rnn4": (("acc", 0, 18), ("ori", 18, 72), ("keypoints", 72, 171)),
    "rnn6": (("acc", 0, 18), ("ori", 18, 72), ("keypoints", 72, 171), ("joints", 171, 240)),
    "rnn7": (("acc", 0, 18), ("ori", 18, 72), ("joints", 72, 141)),
    "rnn8": (("acc", 0, 18), ("ori", 18, 72), ("joints", 72, 141)),
}

# mutation -> the case it is shown on; each is ONE changed line of `restate` / `run_states`
MUTATIONS = {
    "Rcr transposed in accr": "foot0",
    "oric . Rcr for Rcr^T . oric": "foot0",
    "accr where accc belongs in x4 / x6": "foot0",
    "normalised keypoints into x6": "foot0",
    "raw keypoints into x4": "foot0",
    "confidence column dropped": "foot0",
    "bbox scale from x only": "foot0",
    "lerp weights swapped": "foot0",
    "k clamped in the fuse": "foot0",
    "regime 0 taking j3dr_v": "foot0",
    "regime 2 taking the lerp": "foot0",
    "j3dc not rotated": "foot0",
    "first_frame not forcing rnn4": "novis2",
    "first_frame not forcing rnn6 on occluded rows": "novis2",
    "the updater stepping on c < lo for c <= lo": "lo_edge",
    "the updater ignoring the refresh counter": "reproj_live",
    "kp not divided by z": "foot0",
    "updater joints without the root subtracted": "foot0",
    "the updater's IMU columns taken from the root frame": "foot0",
    "init_net fed j3dr_i": "foot0",
    "the reach writing h and c exchanged": "foot0",
    "a masked reset leaving rnn6's c": "foot0",
}
# "k clamped in the fuse": inside the middle regime 0 < k < 1, so a clamp to [0, 1] is no slip at all; the variant restated is a
# clamp that bites there (k >= 1/2, the middle regime's confidences sit at k = 0.4).


# ----------------------------------------------------------------------------------------------------- cases
@dataclasses.dataclass
class WCase(F.Case):
    acc: torch.Tensor = None        # [B,T,6,3] float32
    j3dr_i: torch.Tensor = None     # rnn2.linear2.bias [69]
    j3dc: torch.Tensor = None       # rnn4.linear2.bias [69]
    seed: int = 0


# name, tail_f64 case it starts from, Params overrides, poke before the second call
_SPEC = (
    ("foot0", "foot0", {}, None),
    ("foot1", "foot1", {}, None),
    ("tie", "tie", {}, None),
    ("hi_lo", "hi_lo", {}, None),
    ("lo_hi", "lo_hi", {}, None),
    ("reproj", "reproj", {}, None),
    ("reproj_live", "reproj_live", {}, None),
    ("live", "reproj_live", {"use_reproj_opt": False}, None),
    ("novis2", "noflat", {}, {"use_vision_updater": False}),
    ("noimu", "hi_lo", {"use_imu_updater": False}, None),
    ("lo_edge", "nan", {}, None),
)
CASE_NAMES = tuple(s[0] for s in _SPEC)
LO_EDGE = (0.75, 0.875)             # conf_range of "lo_edge": both ends are float32 numbers


def _lo_edge(case):
    """A case with a conf_range whose lower end is a float32 number, and every confidence of every second regime-0 row-frame equal
    to it: 33 x 0.75 sums to 24.75 and divides to 0.75 without a rounding in any order and any precision, so the mean EQUALS lo
    there -- the only place where `c <= lo` and `c < lo` can be told apart. The other confidences move with the range (an affine
    map of [0.7, 0.8] onto it), so every regime stays what it was and the tail's trajectory with it."""
    lo0, hi0 = case.prm.conf_range
    lo, hi = LO_EDGE
    j2dc = case.j2dc.clone()
    c = j2dc[..., 2].double()
    reg0 = O.conf_mean(case.j2dc.reshape(-1, 33, 3)).double().view(case.B, case.T) <= lo0
    j2dc[..., 2] = (lo + (c - lo0) * ((hi - lo) / (hi0 - lo0))).float()
    pick = reg0 & (reg0.long().cumsum(dim=1) % 2 == 1)
    j2dc[..., 2] = torch.where(pick.unsqueeze(2), torch.full_like(j2dc[..., 2], lo), j2dc[..., 2])
    return dataclasses.replace(case, j2dc=j2dc, prm=dataclasses.replace(case.prm, conf_range=LO_EDGE))


def build_cases(body, names=None):
    """The cases of tests/test_wiring_bound_cpu.py and tests/test_gpu_wiring.py."""
    want = [s for s in _SPEC if names is None or s[0] in names]
    tails = {c.name: c for c in F.build_cases(body, names={s[1] for s in want})}
    cases = []
    for name, tail, over, poke2 in want:
        i = CASE_NAMES.index(name)
        c = tails[tail]
        B, T = c.B, c.T
        oric = c.oric.clone()
        aa = 1.1 * synth.normal(700 + i, 1, B * T * 15).reshape(B, T, 5, 3).astype(np.float64)
        oric[:, :, :5] = torch.from_numpy(synth._rodrigues(aa).astype(np.float32))
        acc = torch.from_numpy((8.0 * (synth.uniform01(700 + i, 2, B * T * 18).reshape(B, T, 6, 3) - 0.5)).astype(np.float32))
        calls = list(c.calls)
        if poke2:
            calls[1] = dataclasses.replace(calls[1], poke=dict(calls[1].poke or {}, **poke2))
        bias2 = torch.from_numpy((0.35 * synth.normal(700 + i, 3, 69)).astype(np.float32))
        bias4 = torch.from_numpy((0.35 * synth.normal(700 + i, 4, 69)).astype(np.float32))
        w = WCase(**{f.name: getattr(c, f.name) for f in dataclasses.fields(F.Case)}, acc=acc, j3dr_i=bias2, j3dc=bias4, seed=700 + i)
        w = dataclasses.replace(w, name=name, oric=oric, calls=calls, prm=dataclasses.replace(c.prm, **over))
        cases.append(_lo_edge(w) if name == "lo_edge" else w)
    return cases


def call_params(case):
    """the Params in force during each call"""
    out, prm = [], case.prm
    for call in case.calls:
        if call.poke:
            prm = dataclasses.replace(prm, **call.poke)
        out.append(prm)
    return out


# ------------------------------------------------------------------------------------------------ restatement
@dataclasses.dataclass
class Op:
    slot: str                       # rnn2 rnn3 rnn4 rnn6ff rnn6 rnn7 rnn8 reach u6 u4, in the order a frame runs them
    net: str
    x: torch.Tensor                 # [B, n_in] (reach: [B, 69], the input of init_net)
    mask: torch.Tensor              # [B] bool: the rows that step (reach: whose rnn2 state is overwritten)
    A: torch.Tensor = None          # [B, n_in] float64: the magnitude behind each value (0: a bitwise copy of an input)


SLOTS = ("rnn2", "rnn3", "rnn4", "rnn6ff", "rnn6", "rnn7", "rnn8", "reach", "u6", "u4")


def _dot3(a, b, rev):
    p = a * b
    return (p[..., 2] + p[..., 1]) + p[..., 0] if rev else (p[..., 0] + p[..., 1]) + p[..., 2]


def _vm(v, R, rev):
    """rows of v [B,n,3] times R [B,3,3]: out[b,i,j] = sum_k v[b,i,k] R[b,k,j]; also the sum of the magnitudes of its terms"""
    a, b = v.unsqueeze(2), R.transpose(1, 2).unsqueeze(1)
    return _dot3(a, b, rev), _dot3(a.abs(), b.abs(), False).to(F64)


def _normalize(kp, rev, mut=None):
    """sig_mp_oracle.normalize_keypoints in any dtype; `rev`: the scale applied as a reciprocal"""
    u, v = kp[..., 0], kp[..., 1]
    wd, ht = u.max(dim=-1).values - u.min(dim=-1).values, v.max(dim=-1).values - v.min(dim=-1).values
    sc = (wd if mut == "bbox scale from x only" else torch.maximum(wd, ht)).view(-1, 1, 1)
    xy = kp[..., :2] * (1.0 / sc) if rev else kp[..., :2] / sc
    out = xy - xy[:, 23:24]
    out[:, 23] = xy[:, 23]
    return torch.cat((out, kp[..., 2:]), dim=-1)


def body_extent(ob):
    """an upper bound of the magnitudes summed into a landmark or a joint besides the translation: every bone and the farthest
    rest vertex"""
    return float(ob.bone.double().norm(dim=1).sum() + ob.v_rest.double().norm(dim=1).max())


def restate(case, sim, dtype=F64, order="plain", mut=None, extent=0.0):
    """The sub-net steps of every frame of the case: a list over frames of lists of Op. `sim` is tail_f64.simulate of the case in
    the same dtype and order (its record gives the refresh counter and the reach, its `joint` / `j33` what the updater reads)."""
    dt, B, rev = dtype, case.B, order == "reversed"
    flat = lambda *xs: torch.cat([x.reshape(B, -1) for x in xs], dim=1)
    zA = lambda *shape: torch.zeros(*shape, dtype=F64)
    every = torch.ones(B, dtype=torch.bool)
    b2, b4 = case.j3dr_i.to(dt).expand(B, 69), case.j3dc.to(dt).expand(B, 69)
    rec = sim["rec"]
    frames, t = [], 0
    for call, prm in zip(case.calls, call_params(case)):
        lo, hi = prm.conf_range
        for i in range(call.T):
            first_frame = bool(call.first_frame and i == 0)
            j2dc, accc, oric = case.j2dc[:, t].to(dt), case.acc[:, t].to(dt), case.oric[:, t].to(dt)
            c64 = O.conf_mean(j2dc).double() if dt == F32 else j2dc[:, :, 2].mean(dim=1)                      # L138
            is_hi, gt_lo = c64 >= hi, c64 > lo
            is_mid = gt_lo & (c64 < hi)
            vis = gt_lo if mut == "first_frame not forcing rnn4" else gt_lo | first_frame                     # L149
            Rcr = oric[:, 5]                                                                                  # L139
            accr, A_accr = _vm(accc, Rcr.transpose(1, 2) if mut == "Rcr transposed in accr" else Rcr, rev)   # L142
            if mut == "oric . Rcr for Rcr^T . oric":
                orir, A_orir = _vm(oric.reshape(B, 18, 3), Rcr, rev)
            else:                                                                                             # L143
                a, b = Rcr.transpose(1, 2).reshape(B, 1, 3, 1, 3), oric.transpose(-1, -2).unsqueeze(2)
                orir, A_orir = _dot3(a, b, rev), _dot3(a.abs(), b.abs(), False).to(F64)
            imu_r, A_r = flat(accr, orir), flat(A_accr, A_orir)
            imu_c, A_c = flat(accc, oric), zA(B, 72)
            if mut == "accr where accc belongs in x4 / x6":
                imu_c, A_c = flat(accr, oric), flat(A_accr, zA(B, 54))
            ops = [Op("rnn2", "rnn2", imu_r, every, A_r),                                                     # L144
                   Op("rnn3", "rnn3", flat(imu_r, b2), every, flat(A_r, zA(B, 69)))]                          # L145
            nk, A_nk = _normalize(j2dc, rev, mut), torch.cat((bbox_A(j2dc), zA(B, 33, 1)), dim=-1)
            if mut == "raw keypoints into x4":
                nk = j2dc
            if mut == "confidence column dropped":
                nk = torch.cat((nk[..., :2], torch.zeros_like(nk[..., 2:])), dim=-1)
            ops.append(Op("rnn4", "rnn4", flat(imu_c, nk), vis, flat(A_c, A_nk)))                             # L150-153
            j3dc = torch.where(vis.unsqueeze(1), b4, torch.zeros_like(b4))
            kp6 = _normalize(j2dc, rev) if mut == "normalised keypoints into x6" else j2dc
            x6, A6 = flat(imu_c, kp6, j3dc), flat(A_c, zA(B, 168))
            ff = every if mut != "first_frame not forcing rnn6 on occluded rows" else gt_lo
            ops.append(Op("rnn6ff", "rnn6", x6, ff & first_frame, A6))                                        # L155-156
            ops.append(Op("rnn6", "rnn6", x6, gt_lo, A6))                                                     # L161 / L165
            if mut == "j3dc not rotated":
                j3dr_v, A_v = j3dc.clone(), zA(B, 69)
            else:
                j3dr_v, A_v = _vm(j3dc.view(B, 23, 3), Rcr, rev)                                              # L154
                j3dr_v, A_v = j3dr_v.reshape(B, 69), A_v.reshape(B, 69)
            k64 = (c64 - lo) / (hi - lo)                                                                      # L163
            if mut == "k clamped in the fuse":
                k64 = k64.clamp(min=0.5)
            w1, w2 = (1.0 - k64).to(dt).unsqueeze(1), k64.to(dt).unsqueeze(1)
            if mut == "lerp weights swapped":
                w1, w2 = w2, w1
            lerp = b2 + (j3dr_v - b2) * w2 if rev and mut is None else b2 * w1 + j3dr_v * w2
            A_l = b2.abs().to(F64) * w1.abs().to(F64) + j3dr_v.abs().to(F64) * w2.abs().to(F64)
            low, A_low = (j3dr_v, A_v) if mut == "regime 0 taking j3dr_v" else (b2, zA(B, 69))
            high, A_high = (lerp, A_l) if mut == "regime 2 taking the lerp" else (j3dr_v, A_v)
            j3dr = torch.where(is_hi.unsqueeze(1), high, torch.where(is_mid.unsqueeze(1), lerp, low))
            A_j = torch.where(is_hi.unsqueeze(1), A_high, torch.where(is_mid.unsqueeze(1), A_l, A_low))
            x78, A78 = flat(imu_r, j3dr), flat(A_r, A_j)
            ops += [Op("rnn7", "rnn7", x78, every, A78), Op("rnn8", "rnn8", x78, every, A78)]                 # L169-170
            reach = rec["reach"][:, t].bool()                                                                 # L178-183
            ops.append(Op("reach", "rnn2", b2 if mut == "init_net fed j3dr_i" else j3dr, reach, A_j))
            upd = ~gt_lo & rec["refresh"][:, t].bool() & bool(prm.use_vision_updater)                         # L264
            if mut is None:
                assert torch.equal(upd, rec["upd"][:, t].bool()), (case.name, t)
            if mut == "the updater stepping on c < lo for c <= lo":
                upd = upd & (c64 < lo)
            if mut == "the updater ignoring the refresh counter":
                upd = ~gt_lo & bool(prm.use_vision_updater)
            joint, j33 = rec["joint"][:, t].to(dt), rec["j33"][:, t].to(dt)
            z = torch.where(upd.view(B, 1, 1), j33[:, :, 2:], torch.ones_like(j33[:, :, 2:]))   # (rows that do not step: no 0 / 0)
            kp = j33 if mut == "kp not divided by z" else (j33 * (1.0 / z) if rev else j33 / z)               # L266
            j3 = joint[:, 1:] if mut == "updater joints without the root subtracted" else joint[:, 1:] - joint[:, :1]
            tr = sim["tran"][:, t].abs().to(F64).view(B, 1, 3)
            A_L = (sim["A"][:, t].to(F64) + extent).view(B, 1, 1)
            A_kp = A_L * (1.0 + kp.abs().to(F64)) / z.abs().to(F64)
            A_j3 = joint[:, 1:].abs().to(F64) + joint[:, :1].abs().to(F64) + 2.0 * tr
            sc = O.bbox_scale(kp.to(F64)).view(B, 1, 1)
            A_xy = A_kp[..., :2]
            A_un = bbox_A(kp) + (A_xy + A_xy[:, 23:24]) / sc + 2.0 * A_xy.amax(dim=(1, 2), keepdim=True) / sc * _normalize(kp.to(F64), False)[..., :2].abs()
            A_un = torch.cat((A_un, A_kp[..., 2:]), dim=-1)
            imu_u, A_u = (imu_r, A_r) if mut == "the updater's IMU columns taken from the root frame" else (flat(accc, oric), zA(B, 72))
            nan0 = lambda x: torch.where(upd.view(B, *([1] * (x.dim() - 1))), x, torch.zeros_like(x))
            ops.append(Op("u6", "rnn6", nan0(flat(imu_u, kp, j3)), upd, nan0(flat(A_u, A_kp, A_j3))))         # L269
            ops.append(Op("u4", "rnn4", nan0(flat(imu_u, _normalize(kp, rev))), upd, nan0(flat(A_u, A_un))))  # L270
            frames.append(ops)
            t += 1
    return frames


# ------------------------------------------------------------------------------------------------------ the wire
def scales(frames):
    """s per net and input column: per column group the largest power of two (at most S_MAX) with s |x| <= 1 on every row and
    step of the float64 run"""
    out = {}
    for net in NET_NAMES:
        s = np.ones(SPEC[net][0])
        for _, a, b in GROUPS[net]:
            m = 0.0
            for ops in frames:
                for op in ops:
                    if op.net == net and op.slot != "reach" and bool(op.mask.any()):
                        m = max(m, float(op.x[op.mask][:, a:b].abs().max()))
            s[a:b] = S_MAX if m == 0.0 else min(S_MAX, max(S_MIN, 2.0 ** np.floor(-np.log2(m))))
        out[net] = s
    return out


def check_scale(frames, sc):
    """the scale condition: s_k |x_k| <= 1 on every column, row and step; returns the largest product per net"""
    worst = {}
    for net in NET_NAMES:
        w = 0.0
        for ops in frames:
            for op in ops:
                if op.net == net and op.slot != "reach" and bool(op.mask.any()):
                    w = max(w, float((op.x[op.mask].abs().double() * torch.from_numpy(sc[net])).max()))
        assert w <= 1.0, (net, w)
        worst[net] = w
    return worst


def state_dict(case, sc):
    """tail_f64.state_dict(case) plus the wire with the column scales `sc` (see the module docstring)"""
    sd = F.state_dict(case)
    sd["rnn2.linear2.bias"] = case.j3dr_i.numpy().copy()
    sd["rnn4.linear2.bias"] = case.j3dc.numpy().copy()
    for q, net in enumerate(NET_NAMES):
        nin, H, _ = SPEC[net]
        assert 2 * nin <= H
        k, u = np.arange(nin), np.arange(2 * nin)
        sd[f"{net}.linear1.weight"][2 * k, k] = 1.0
        sd[f"{net}.linear1.weight"][2 * k + 1, k] = -1.0
        sd[f"{net}.rnn.weight_ih_l0"][2 * H + u, u] = sc[net][u // 2]
        sd[f"{net}.rnn.bias_ih_l1"][:] = 0.3 * synth.normal(case.seed, 10 + q, 4 * H)
    k, u = np.arange(69), np.arange(138)
    sd["rnn2.init_net.0.weight"][2 * k, k] = 1.0
    sd["rnn2.init_net.0.weight"][2 * k + 1, k] = -1.0
    sd["rnn2.init_net.2.weight"][u, u] = 1.0
    for q, w in enumerate(REACH_Q):
        sd["rnn2.init_net.4.weight"][q * 512 + u, u] = w
    return sd


def wire_params(sd):
    """lstm_f64.params of every net with the weight matrices held sparse (lstm_f64.step runs on them as it stands: a wire is a
    few thousand non-zeros in matrices of millions), and init_net's three layers"""
    try:
        import scipy.sparse as sp
        hold = sp.csr_matrix
    except ImportError:
        hold = lambda w: w
    out = {}
    for net in NET_NAMES:
        p = L.params(sd, net)
        for k in ("W1", "W2", "Wih0", "Whh0", "Wih1", "Whh1"):
            p[k] = hold(p[k])
        out[net] = p
    out["init_net"] = [(hold(np.asarray(sd[f"rnn2.init_net.{i}.weight"], np.float64)), np.asarray(sd[f"rnn2.init_net.{i}.bias"], np.float64)) for i in (0, 2, 4)]
    return out


def init_net(layers, v):
    """init_net of rows v [n,69] in float64 -> (h [2,n,512], c [2,n,512], S: the magnitude scale of each output, same shapes)"""
    a = s = np.asarray(v, np.float64)
    for i, (W, b) in enumerate(layers):
        s = np.abs(a) @ np.abs(W).T + np.abs(b)
        a = a @ W.T + b
        if i < 2:
            a = np.maximum(a, 0.0)
    hc = a.reshape(-1, 2, 2, 512).transpose(1, 2, 0, 3)             # view(-1, 2, 2, 512).permute(1, 2, 0, 3)
    S = s.reshape(-1, 2, 2, 512).transpose(1, 2, 0, 3)
    return hc[0], hc[1], S[0], S[1]


def input_bound(frames64, evals32):
    """Bx = M max(e32, eps32 A) of every value of every op: e32 the largest distance of the float32 evaluations (lists of frames
    aligned with frames64) from float64 on the rows that step. Returns a list over frames of {slot: [B, n] float64 array}."""
    out = []
    for t, ops in enumerate(frames64):
        d = {}
        for j, op in enumerate(ops):
            e = torch.zeros_like(op.A)
            for ev in evals32:
                o = ev[t][j]
                assert o.slot == op.slot and torch.equal(o.mask, op.mask), ("a float32 evaluation steps other rows", t, op.slot)
                e = torch.maximum(e, (o.x.to(F64) - op.x).abs())
            bx = M * torch.maximum(e, EPS32 * op.A)
            d[op.slot] = torch.where(op.mask.unsqueeze(1), bx, torch.zeros_like(bx)).numpy()
        out.append(d)
    return out


class Bound:
    """Bound of every state element of a net against `run_states`:
        lstm_f64.Bound.tol_hc()                  the LSTM step's own error, as it stands, plus
        E_t = E_{t-1} / 2 + s_k Bx_k(t) / 2      on the steps taken (layer 0, units 2k and 2k+1; relu and tanh do not stretch)
    with Bx = M max(e32, eps32 A) the bound of the input value x_k itself (`input_bound`): e32 from the float32 restatement in
    two association orders and from the float32 OracleNet, A per column group
        accc, oric, raw keypoints, confidences, the biases j3dr_i / j3dc    0 (bitwise copies)
        accr, orir, j3dc . Rcr                    the sum of the magnitudes of the three products
        the lerp                                  |vi| (1 - k) + |v| k
        normalised keypoints                      pose_ops_f64.bbox_A
        the updater's joints                      |P_j| + |P_0| + 2 |tran|
        the updater's kp = j33 / z                A_L (1 + |kp|) / |z|, A_L = tail_f64's accumulated magnitude behind tran plus the
                                                  body's extent (every bone and the farthest rest vertex)
        the updater's normalised kp               bbox_A of kp plus kp's own A carried through the scale and the hip row
    A reach overwrites rnn2's state: E of those rows becomes Y_REL 2^-24 S + Y_ABS of init_net's dense sums plus Bx (the quarters'
    weights are at most 1); layer 1 keeps such an E times its forget gate per step. A masked reset clears E."""

    def __init__(self, B, sc, params):
        self.lb = {n: L.Bound(B) for n in NET_NAMES}
        self.E = {n: np.zeros((2, B, SPEC[n][1])) for n in NET_NAMES}
        self.s = {n: np.repeat(sc[n], 2) for n in NET_NAMES}         # per unit u: s of column u // 2
        self.f1 = {n: L._sigmoid(np.split(params[n]["bl1"], 4)[1]) for n in NET_NAMES}

    def step(self, net, mask, bx, S, c):
        self.lb[net].update(S, c)
        m = np.asarray(mask, bool)
        n2 = 2 * SPEC[net][0]
        E = self.E[net]
        e0 = 0.5 * E[0, m]
        e0[:, :n2] += 0.5 * self.s[net] * np.repeat(bx[m], 2, axis=1)
        E[0, m] = e0
        E[1, m] = E[1, m] * self.f1[net]

    def reach(self, mask, bx, Sh, Sc):
        m = np.asarray(mask, bool)
        E = self.E["rnn2"]
        b2 = np.repeat(bx[m], 2, axis=1)
        for l in range(2):
            e = L.Y_REL * EPS32 * np.maximum(Sh[l], Sc[l]) + L.Y_ABS
            e[:, :138] += REACH_Q[0] * b2
            E[l, m] = e

    def reset(self, rows):
        for n in NET_NAMES:
            self.E[n][:, np.asarray(rows, bool)] = 0.0

    def tol(self, net):
        return self.lb[net].tol_hc() + self.E[net]


def run_states(case, params, frames, sc=None, bx=None, mut=None):
    """lstm_f64.step over the steps of `frames` with the wire's parameters, the resets of the case between its calls and the
    init_net overwrite at a reach. Returns a list over frames of {net: (h, c)} [2,B,H] float64 -- and, with `bx` (input_bound),
    a second list of {net: tol [2,B,H] float32}."""
    B = case.B
    h = {n: np.zeros((2, B, SPEC[n][1])) for n in NET_NAMES}
    c = {n: np.zeros((2, B, SPEC[n][1])) for n in NET_NAMES}
    bound = Bound(B, sc, params) if bx is not None else None
    states, tols, t = [], [], 0
    for call in case.calls:
        if call.reset:
            rows = case.reset_rows.numpy()
            for n in NET_NAMES:
                h[n][:, rows] = 0.0
                if not (mut == "a masked reset leaving rnn6's c" and n == "rnn6"):
                    c[n][:, rows] = 0.0
            if bound:
                bound.reset(rows)
        for _ in range(call.T):
            for op in frames[t]:
                m = op.mask.numpy()
                if not m.any():
                    continue
                if op.slot == "reach":
                    hh, cc, Sh, Sc = init_net(params["init_net"], op.x[op.mask].double().numpy())
                    if mut == "the reach writing h and c exchanged":
                        hh, cc = cc, hh
                    h["rnn2"][:, m], c["rnn2"][:, m] = hh, cc
                    if bound:
                        bound.reach(m, bx[t]["reach"], Sh, Sc)
                    continue
                _, h[op.net], c[op.net], S = L.step(params[op.net], op.x.double().numpy(), h[op.net], c[op.net], m)
                if bound:
                    bound.step(op.net, m, bx[t][op.slot], S, c[op.net])
            states.append({n: (h[n].copy(), c[n].copy()) for n in NET_NAMES})
            if bound:
                tols.append({n: bound.tol(n).astype(np.float32) for n in NET_NAMES})
            t += 1
    return (states, tols) if bound else states


# ------------------------------------------------------------------------------------------------ the float32 oracle
def oracle_run(body, case, sd):
    """the float32 OracleNet on the wired state dict: its sub-net inputs as frames of Op (aligned with `restate`) and its states
    after every frame, its pose and tran"""
    ora = O.OracleNet(body, batch=case.B, live=case.prm.live)
    ora.load_numpy_state_dict(sd)
    case.prm.poke_oracle(ora)
    ora.gravityc = case.gravity.clone()
    B = case.B
    every, none = torch.ones(B, dtype=torch.bool), torch.zeros(B, dtype=torch.bool)
    log, inner = [], ora._step

    def spy(name, x, rows=None):
        log.append((name, x.clone(), every if rows is None else torch.zeros(B, dtype=torch.bool).index_fill_(0, rows, True)))
        return inner(name, x, rows)

    ora._step = spy
    ora.rnn2.init_net.register_forward_hook(lambda mod, inp, out: log.append(("reach", inp[0].clone(), None)))
    frames, states, poses, trans, t = [], [], [], [], 0
    for call, prm in zip(case.calls, call_params(case)):
        if call.reset:
            ora.reset_states(case.reset_rows.nonzero().flatten())
        prm.poke_oracle(ora)
        for i in range(call.T):
            del log[:]
            ff = bool(call.first_frame and i == 0)
            p, x = ora.forward_batch(case.j2dc[:, t], case.acc[:, t], case.oric[:, t], case.first_tran if (call.first_tran and i == 0) else None, ff)
            poses.append(p.clone()), trans.append(x.clone())
            tr = ora.trace                                          # the wire leaves every output its bias, bitwise
            seen = ((tr["c"] > prm.conf_range[0]) | ff).unsqueeze(1)     # (pc is rnn6's output on the rows that see the camera)
            assert torch.equal(tr["vr"], case.bias["vr"].expand(B, 3)) and torch.equal(tr["poseg6d"], case.bias["r6d"].expand(B, 144)), (case.name, t)
            assert torch.equal(torch.where(seen, tr["pc"], case.bias["pc"].expand(B, 3)), case.bias["pc"].expand(B, 3)), (case.name, t)
            assert torch.equal(tr["j3dr_i"], case.j3dr_i.expand(B, 69)), (case.name, t)
            got, after7, seen6 = {}, False, 0
            for name, x, m in log:
                if name == "reach":
                    rows = ora.trace["reach"]
                    full = torch.zeros(B, 69)
                    full[rows] = x
                    got["reach"] = (full, rows.clone())
                    continue
                after7 = after7 or name == "rnn7"
                slot = name
                if name == "rnn4" and after7:
                    slot = "u4"
                if name == "rnn6":
                    slot = "u6" if after7 else ("rnn6ff" if ff and seen6 == 0 else "rnn6")
                    seen6 += 1
                assert slot not in got, (case.name, t, slot)
                got[slot] = (x, m)
            ops = []
            for slot in SLOTS:
                net = {"rnn6ff": "rnn6", "u6": "rnn6", "u4": "rnn4", "reach": "rnn2"}.get(slot, slot)
                x, m = got.get(slot, (torch.zeros(B, 69 if slot == "reach" else SPEC[net][0]), none))
                ops.append(Op(slot, net, torch.where(m.unsqueeze(1), x, torch.zeros_like(x)), m))
            frames.append(ops)
            states.append({n: (ora.h[n].double().numpy().copy(), ora.c[n].double().numpy().copy()) for n in NET_NAMES})
            t += 1
    return frames, states, torch.stack(poses, 1), torch.stack(trans, 1)


def _masked(frames):
    """the same frames with the rows that do not step zeroed (so that evaluations compare on the rows that do)"""
    return [[dataclasses.replace(op, x=torch.where(op.mask.unsqueeze(1), op.x, torch.zeros_like(op.x))) for op in ops] for ops in frames]


def ratios(states, ref, tols, active=None):
    """{net: worst |state - ref| / tol over h, c, both layers, every row and the frames given}: states / ref / tols are lists over
    frames; inf where a value is not finite"""
    out = {n: 0.0 for n in NET_NAMES}
    for t in range(len(ref)):
        for n in NET_NAMES:
            for k in (0, 1):
                got = np.asarray(states[t][n][k], np.float64)
                r = np.abs(got - ref[t][n][k]) / tols[t][n]
                r = np.where(np.isfinite(r), r, np.inf)
                if active is not None:
                    r = r[:, active[t]]
                if r.size:
                    out[n] = max(out[n], float(r.max()))
    return out


@dataclasses.dataclass
class Built:
    case: WCase
    sim: dict                       # tail_f64.simulate in float64
    frames: list                    # restate in float64
    sc: dict                        # the wire's column scales
    sd: dict                        # the wired state dict
    params: dict
    states: list                    # float64 states after every frame
    tols: list                      # the Bound after every frame
    r32: dict                       # float32 evaluation -> {net: worst error / Bound}
    scale_worst: dict
    oracle_pose: torch.Tensor       # the float32 OracleNet's outputs on the wired dict
    oracle_tran: torch.Tensor


def build(body, case, evals=True):
    """everything the tests need of a case: the float64 run, the wire, the float32 evaluations, the Bound. `evals=False` leaves
    out the ratios of the float32 evaluations (their inputs still define e32): the device test does not read them."""
    ob64, ob32 = O.OracleBody(body, dtype=F64), O.OracleBody(body, dtype=F32)
    sim = F.simulate(ob64, case)
    frames = _masked(restate(case, sim, extent=body_extent(ob64)))
    sc = scales(frames)
    worst = check_scale(frames, sc)
    sd = state_dict(case, sc)
    params = wire_params(sd)
    ev = {}
    for o in ORDERS:
        ev[o] = _masked(restate(case, F.simulate(ob32, case, dtype=F32, order=o), F32, o))
    ofr, ost, opose, otran = oracle_run(body, case, sd)
    bx = input_bound(frames, list(ev.values()) + [ofr])
    states, tols = run_states(case, params, frames, sc, bx)
    r32 = {}
    if evals:
        r32 = {o: ratios(run_states(case, params, ev[o]), states, tols) for o in ORDERS}
        r32["oracle"] = ratios(ost, states, tols)
    return Built(case, sim, frames, sc, sd, params, states, tols, r32, worst, opose, otran)


CENSUS_FRAMES = ("regime 0", "regime 1", "regime 2", "first_frame in regime 0 (rnn4 and rnn6 step on every row)", "updater taken",
                 "updater withheld by the live refresh counter", "pending step, then a visible frame", "pending step, then an occluded frame")
CENSUS_ROWS = ("pending at the end of the first call, the row goes on (the rider)", "pending at the end of the first call, the row is reset",
               "a reach", "a reach re-armed by the masked reset")


def census(built):
    """{item: count} of one case: row-frames for CENSUS_FRAMES, rows for CENSUS_ROWS"""
    case, frames = built.case, built.frames
    B, T = case.B, case.T
    slot = lambda name: torch.stack([next(op.mask for op in ops if op.slot == name) for ops in frames], dim=1)      # [B,T]
    regime, refresh = built.sim["rec"]["regime"], built.sim["rec"]["refresh"].bool()
    upd, reach, ff6 = slot("u6"), slot("reach"), slot("rnn6ff")
    assert torch.equal(upd, slot("u4")) and torch.equal(slot("rnn6"), regime > 0)
    vis_on = torch.zeros(B, T, dtype=torch.bool)
    t = 0
    for call, prm in zip(case.calls, call_params(case)):
        vis_on[:, t:t + call.T] = bool(prm.use_vision_updater)
        t += call.T
    out = {f"regime {r}": int((regime == r).sum()) for r in (0, 1, 2)}
    out[CENSUS_FRAMES[3]] = int((ff6 & slot("rnn4") & (regime == 0)).sum())
    out[CENSUS_FRAMES[4]] = int(upd.sum())
    out[CENSUS_FRAMES[5]] = int(((regime == 0) & ~refresh & vis_on).sum())
    T1 = case.calls[0].T
    inner = torch.ones(T - 1, dtype=torch.bool)
    inner[T1 - 1] = False                                           # (the call boundary is counted by rows, below)
    out[CENSUS_FRAMES[6]] = int((upd[:, :-1] & (regime[:, 1:] > 0) & inner).sum())
    out[CENSUS_FRAMES[7]] = int((upd[:, :-1] & (regime[:, 1:] == 0) & inner).sum())
    cleared = case.reset_rows if case.calls[1].reset else torch.zeros(B, dtype=torch.bool)
    out[CENSUS_ROWS[0]] = int((upd[:, T1 - 1] & ~cleared).sum())
    out[CENSUS_ROWS[1]] = int((upd[:, T1 - 1] & cleared).sum())
    out[CENSUS_ROWS[2]] = int(reach.any(dim=1).sum())
    out[CENSUS_ROWS[3]] = int((reach[:, :T1].any(dim=1) & reach[:, T1:].any(dim=1) & cleared).sum())
    return out
