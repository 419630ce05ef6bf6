"""The tail of the sig_mp frame in float64, branch by branch -- TEST INFRASTRUCTURE, NOT PRODUCT.

The frame tail (net/sig_mp.py L173-273: 6D -> rotation, IK, foot chains, contact / velocity step, high-regime fusion, floor
sampling and correction, first_tran / first_frame, re-projection refinement, live landmark cache) is `tail_impl` on the device
(csrc/rc_frame_dev.h), instantiated as rc_tail_kernel<1>, rc_tail_kernel<4> and the LIVE form of rc_live.hip.
oracle/sig_mp_oracle.OracleNet.forward_batch restates it in float32 inside the whole frame. Here it stands alone, as
`tail_step`: a pure function of the row state and the frame's inputs that runs in any dtype, records every branch it takes and,
for every comparison it makes, the distance between the two sides.

What makes the tail testable without an entry point of its own: in a state dict whose every tensor is zero except the four
`linear2.bias` vectors, every sub-net's output IS its bias, bitwise, in both product arithmetics and on every engine (0 * h sums
to 0). `state_dict(case)` builds that dict; the biases of rnn7 / rnn8 / rnn3 / rnn6 are the tail's r6d / contact logits / vr / pc.
Everything else the tail consumes varies per row and frame through ordinary inputs (Rcr = IMU 5, gravity, confidences,
first_tran / first_frame, masked resets) and through the state that evolves across frames and calls.

  tail_step    one frame of B rows; `mut` names a one-line wrong variant (MUTATIONS), `order` a second association order
  simulate     a case's calls (frames, first_tran / first_frame, resets) through tail_step
  build_cases  seeded inputs (robustcap_amd.synth, nothing stored): one set of biases per contact situation, rows chosen so
               that float32 and float64 provably take the same branch on every row and frame (`conditions`)
  Bound        M * max(e32, eps32 * A) per output group (see its docstring)

Contact probabilities: every situation keeps sigmoid(logit) at least 1e-3 from the threshold, because an exact equality on a
sigmoid cannot be constructed portably across expf implementations -- with two exceptions that are exact by construction on
every one of them: bitwise equal logits (c0 == c1, the argmax tie) and logit 0 against a threshold of 0.5 (exp(-0) = 1 and
1 / (1 + 1) = 0.5 are exact), the only place where `<` and `<=` can be told apart.
"""
import dataclasses

import numpy as np
import torch

from robustcap_amd import config as C
from robustcap_amd import synth
from . import sig_mp_oracle as O

F32, F64 = torch.float32, torch.float64
EPS32 = 2.0 ** -24
MARGIN = 3.0            # float32 evaluations at most Bound / MARGIN, mutations at least MARGIN * Bound
COND_FACTOR = 8.0       # every comparison's float64 margin is at least COND_FACTOR x the bound of the compared quantity
CONTACT_KEEP = 1e-3     # distance of every contact probability from the threshold (the two exact cases aside)
# M: the CPU conditions alone need M > MARGIN for the evaluations that define e32 (their ratio is at most 1 / M), so M = 4, the
# smallest power of two above 3. Measured (profiles/tail_bound_ratios.txt): the float32 evaluations are at 1 / 4, the weakest
# mutation at 7.8e3. On an MI355X all 14 cases pass every path at this M, the translation at 0.25 of the Bound at most and the
# worst joint at 0.575 (tests/test_gpu_tail_branches.py appends the device ratios to the same file through RC_TAIL_RATIOS_OUT). If a
# path exceeds 1 for an arithmetic reason, M is raised here with that reason, as in smplify_f64.
M = 4.0

CORR = ("none", "use1", "use0", "not applied")
ORDERS = ("plain", "reversed")


@dataclasses.dataclass
class Params:
    conf_range: tuple = (0.7, 0.8)
    contact_threshold: float = 0.7
    distance_threshold: float = 10.0
    height_threshold: float = 0.15
    tran_filter_num: float = 0.05
    use_flat_floor: bool = True
    use_reproj_opt: bool = False
    smooth: float = 1.0
    update_vision_freq: int = 30
    live: bool = False
    use_vision_updater: bool = True
    use_imu_updater: bool = True

    def poke_net(self, net):
        """onto a robustcap_amd Net (the reference's attribute names, typos included)"""
        net.conf_range = tuple(self.conf_range)
        net.contact_threshold = self.contact_threshold
        net.distrance_threshold = self.distance_threshold
        net.height_threhold = self.height_threshold
        net.tran_filter_num = self.tran_filter_num
        net.use_flat_floor = self.use_flat_floor
        net.use_reproj_opt = self.use_reproj_opt
        net.smooth = self.smooth
        net.update_vision_freq = self.update_vision_freq
        net.live = self.live
        net.use_vision_updater = self.use_vision_updater
        net.use_imu_updater = self.use_imu_updater

    def poke_oracle(self, ora):
        ora.conf_range = tuple(self.conf_range)
        ora.contact_threshold = self.contact_threshold
        ora.distance_threshold = self.distance_threshold
        ora.height_threshold = self.height_threshold
        ora.tran_filter_num = self.tran_filter_num
        ora.use_flat_floor = self.use_flat_floor
        ora.use_reproj_opt = self.use_reproj_opt
        ora.smooth = self.smooth
        ora.update_vision_freq = self.update_vision_freq
        ora.live = self.live
        ora.use_vision_updater = self.use_vision_updater
        ora.use_imu_updater = self.use_imu_updater


class State:
    """the row state the tail reads and writes (+ A, the bookkeeping of the Bound: accumulated magnitude behind last_tran)"""

    def __init__(self, B, dtype):
        z = lambda *s: torch.zeros(*s, dtype=dtype)
        self.has_last = torch.zeros(B, dtype=torch.bool)
        self.last_tran, self.last_pfoot = z(B, 3), z(B, 2, 3)
        self.n_floor = torch.zeros(B, dtype=torch.long)
        self.floor = z(B, 11, 3)
        self.count = torch.zeros(B, dtype=torch.long)        # live refresh counter; survives a reset like the reference's
        self.j_temp = z(B, 33, 3)
        self.first_reach = torch.ones(B, dtype=torch.bool)
        self.A = torch.zeros(B, dtype=F64)

    FIELDS = ("has_last", "last_tran", "last_pfoot", "n_floor", "floor", "count", "j_temp", "first_reach", "A")

    def reset(self, rows=None):
        rows = slice(None) if rows is None else torch.as_tensor(rows, dtype=torch.bool)
        self.has_last[rows] = False
        self.n_floor[rows] = 0
        self.first_reach[rows] = True

    def keep(self, old, active):
        """rows outside `active` keep `old` (a row past its length in a ragged call)"""
        for f in self.FIELDS:
            new, o = getattr(self, f), getattr(old, f)
            m = active.view(-1, *([1] * (new.dim() - 1)))
            setattr(self, f, torch.where(m, new, o))

    def clone(self):
        s = State.__new__(State)
        for f in self.FIELDS:
            setattr(s, f, getattr(self, f).clone())
        return s


# mutation name -> the case kinds built for it (see build_cases); each is ONE changed line of tail_step
MUTATIONS = {
    "<= for < at the contact threshold": ("edge",),
    ">= for > at on_ground": ("edge",),
    "argmax tie -> foot 1": ("tie",),
    "foot velocity with the wrong sign": ("foot0", "foot1"),
    "foot velocity of the other foot": ("foot0", "foot1"),
    "vel_scale / 60 dropped": ("below",),
    "far test skipped": ("far", "filter"),
    "lerp weight without the clamp of kconf": ("foot0", "below"),
    "floor mean over samples 0..5": ("foot0", "foot1", "hi_lo"),
    "pick takes the nearer plane": ("foot0", "foot1", "hi_lo"),
    "mean - p0 swapped with mean - p1": ("foot0", "foot1", "hi_lo"),
    "correction applied when not on the ground": ("drop",),
    "sampling on the first frame": ("foot0", "foot1"),
    "first_frame override missing": ("foot0", "below"),
    "root of the pose not replaced by Rcr": ("foot0",),
    "IK with R_parent . R": ("foot0",),
    "second refinement pass on the unshifted landmarks": ("reproj", "reproj_live"),
    "cached landmarks ignored in live mode": ("reproj_live",),
}


def tail_step(ob, st, bias, Rcr, j2dc, g, first_tran, first_frame, prm, order="plain", mut=None):
    """One frame of B rows. ob: OracleBody of the dtype; st: State (updated in place); bias: dict r6d [144], ct [2], vr [3],
    pc [3]; Rcr [B,3,3], j2dc [B,33,3], g [B,3], first_tran [B,3] or None. Returns (pose [B,24,3,3], tran [B,3], record, margins):
    record = {name: [B]} of the branches taken (+ `upd`, and `joint` [B,24,3] / `j33` [B,33,3]: what the vision updater reads, on
    the rows with c <= lo, zero elsewhere), margins = [(name, margin [B], A [B], checked [B])] with A the magnitude behind
    the compared quantity (its float32 error is a few eps32 * A)."""
    dt, B = Rcr.dtype, Rcr.shape[0]
    rev = order == "reversed"
    lo, hi = prm.conf_range
    margins = []

    def dot(a, b):
        p = a * b
        return (p[..., 2] + p[..., 1]) + p[..., 0] if rev else (p[..., 0] + p[..., 1]) + p[..., 2]

    def mv(Mx, v):
        return dot(Mx, v.unsqueeze(-2))

    def nrm(v):
        return dot(v, v).sqrt()

    def amax(v):
        return v.abs().reshape(B, -1).max(dim=1).values.to(F64)

    def note(name, a, b, A, checked):
        margins.append((name, (a.to(F64) - b).abs() if not isinstance(b, float) else (a.to(F64) - b).abs(), A, checked.clone()))

    every = torch.ones(B, dtype=torch.bool)
    ones = torch.ones(B, dtype=F64)
    # L138: the float32 mean in the reference's order is the INPUT of the thresholds (tests/test_conf_order.py pins the order);
    # in float64 the plain mean of the same float32 confidences
    c64 = O.conf_mean(j2dc).double() if dt == F32 else j2dc[:, :, 2].mean(dim=1)
    is_hi, gt_lo = c64 >= hi, c64 > lo
    regime = is_hi.long() * 2 + (gt_lo & ~is_hi).long()
    # (a mean that EQUALS lo is exact by construction -- 33 equal confidences, oracle/wiring_f64.py -- and exempt like the c0 == c1 tie)
    note("conf vs lo", c64, float(lo), ones, every & (c64 != float(lo)))
    note("conf vs hi", c64, float(hi), ones, every)
    k64 = (c64 - lo) / (hi - lo)

    # L173-175
    r6 = bias["r6d"].to(dt).view(24, 6)
    a, b = r6[:, :3], r6[:, 3:]
    c0 = a / nrm(a).unsqueeze(1)
    t_ = b - dot(c0, b).unsqueeze(1) * c0
    c1 = t_ / nrm(t_).unsqueeze(1)
    Rg = torch.stack((c0, c1, torch.linalg.cross(c0, c1, dim=1)), dim=-1)
    Rg = torch.where(torch.isnan(Rg), torch.zeros_like(Rg), Rg)
    par = ob.par
    if mut == "IK with R_parent . R":
        loc = Rg[par[1:]] @ Rg[1:]
    else:
        loc = Rg[par[1:]].transpose(-1, -2) @ Rg[1:]
    pose = torch.cat((Rg[:1], loc), dim=0).unsqueeze(0).repeat(B, 1, 1, 1)
    if mut != "root of the pose not replaced by Rcr":
        pose[:, 0] = Rcr
    # L186
    pf_root = ob.bone_fk(Rg.unsqueeze(0))[0, 10:12]
    pf = torch.stack((mv(Rcr, pf_root[0].expand(B, 3)), mv(Rcr, pf_root[1].expand(B, 3))), dim=1)

    # L187-194
    ct = bias["ct"].to(dt)
    cc = torch.sigmoid(ct)
    cmax = torch.maximum(cc[0], cc[1]).expand(B)
    thr = prm.contact_threshold
    foot = int(cc[1] >= cc[0]) if mut == "argmax tie -> foot 1" else int(cc[1] > cc[0])
    exact_tie = bool(bias["ct"][0] == bias["ct"][1])
    exact_edge = float(bias["ct"].max()) == 0.0 and thr == 0.5
    note("cmax vs contact threshold", cmax, float(thr), ones, every & (not exact_edge))
    note("c1 vs c0", cc[1].expand(B), cc[0].expand(B).to(F64), ones, every & (not exact_tie))
    below = cmax <= thr if mut == "<= for < at the contact threshold" else cmax < thr
    use_vel = below | ~st.has_last
    v_vel = mv(Rcr, bias["vr"].to(dt).expand(B, 3))
    if mut != "vel_scale / 60 dropped":
        v_vel = v_vel * 0.05 if rev else v_vel * C.vel_scale / 60
    f2 = 1 - foot if mut == "foot velocity of the other foot" else foot
    v_foot = st.last_pfoot[:, f2] - pf[:, f2]
    if mut == "foot velocity with the wrong sign":
        v_foot = -v_foot
    v = torch.where(use_vel.unsqueeze(1), v_vel, v_foot)
    vterm = torch.where(use_vel, amax(v_vel), amax(st.last_pfoot[:, f2]) + amax(pf[:, f2]))
    tran = torch.where(st.has_last.unsqueeze(1), st.last_tran + v, v)
    A = torch.where(st.has_last, st.A, torch.zeros_like(st.A)) + vterm + amax(tran)
    start = torch.zeros(B, dtype=torch.bool)              # the row's translation was assigned, not accumulated, in this frame

    # L196-203
    pc = bias["pc"].to(dt).expand(B, 3)
    kf = k64 if mut == "lerp weight without the clamp of kconf" else torch.clamp(k64, max=1.0)
    dist = nrm(pc - tran)
    by_filter = prm.tran_filter_num > 1
    far = (dist > prm.distance_threshold) | by_filter
    note("|pc - tran| vs jump distance", dist, float(prm.distance_threshold), A + amax(pc), is_hi & (not by_filter))
    if mut == "far test skipped":
        far = torch.zeros(B, dtype=torch.bool)
    w = prm.tran_filter_num * kf
    w1, w2 = (1.0 - w).to(dt).unsqueeze(1), w.to(dt).unsqueeze(1)
    lerp = tran + (pc - tran) * w2 if rev else tran * w1 + pc * w2
    fused = torch.where(far.unsqueeze(1), pc, lerp)
    tran = torch.where(is_hi.unsqueeze(1), fused, tran)
    far = far & is_hi
    A = torch.where(far, amax(pc), torch.where(is_hi, A + amax(pc) * w.abs() + amax(tran), A))
    start |= far

    # L206-221
    on_ground = cmax >= thr if mut == ">= for > at on_ground" else cmax > thr
    ft_given = first_tran is not None
    d0, d1 = dot(pf[:, 0] + tran, g), dot(pf[:, 1] + tran, g)
    p0, p1 = d0.unsqueeze(1) * g, d1.unsqueeze(1) * g
    n0, n1 = nrm(p0), nrm(p1)
    p0_lt_p1 = n0 < n1
    first = first_frame or ft_given
    if mut == "sampling on the first frame":
        first = False
    sample = (st.n_floor < 11) & on_ground & is_hi & bool(prm.use_flat_floor) & (not first)
    pick = torch.where(p0_lt_p1.unsqueeze(1), p0, p1) if mut == "pick takes the nearer plane" else torch.where(p0_lt_p1.unsqueeze(1), p1, p0)
    rows = sample.nonzero().flatten()
    st.floor[rows, st.n_floor[rows]] = pick[rows]
    st.n_floor = st.n_floor + sample.long()
    apply = (st.n_floor > 10) & bool(prm.use_flat_floor)
    if mut != "correction applied when not on the ground":
        apply = apply & on_ground
    Ah = A + 1.0
    note("|p0| vs |p1|", n0, n1.to(F64), Ah, sample | apply)
    m = st.floor[:, 0:6] if mut == "floor mean over samples 0..5" else st.floor[:, 5:11]
    if rev:
        mean = (((((m[:, 5] + m[:, 4]) + m[:, 3]) + m[:, 2]) + m[:, 1]) + m[:, 0]) / 6
    else:
        mean = (((((m[:, 0] + m[:, 1]) + m[:, 2]) + m[:, 3]) + m[:, 4]) + m[:, 5]) / 6
    e1, e0 = mean - p1, mean - p0
    ht = prm.height_threshold
    use1 = apply & p0_lt_p1 & (nrm(e1) < ht)
    use0 = apply & ~use1 & (nrm(e0) < ht)
    note("|mean - p1| vs height", nrm(e1), float(ht), Ah + amax(mean), apply & p0_lt_p1)
    note("|mean - p0| vs height", nrm(e0), float(ht), Ah + amax(mean), apply & ~use1)
    if mut == "mean - p0 swapped with mean - p1":
        e1, e0 = e0, e1
    d = torch.where(use1.unsqueeze(1), e1, torch.where(use0.unsqueeze(1), e0, torch.zeros_like(e0)))
    tran = tran + d
    A = torch.where(use1 | use0, A + amax(mean) + amax(p0) + amax(p1) + amax(tran), A)
    corr = torch.where(use1, 1, torch.where(use0, 2, torch.where(apply, 3, 0)))
    # L222-225
    if ft_given:
        tran = first_tran.to(dt).clone()
        A, start = amax(tran), every.clone()
    elif first_frame and mut != "first_frame override missing":
        tran = pc.clone()
        A, start = amax(tran), every.clone()
    st.last_pfoot = pf
    st.has_last = every.clone()

    # L228-242
    moves = prm.live and (prm.use_reproj_opt or prm.use_vision_updater)
    refresh = (st.count == 0) if prm.live else every.clone()
    upd = ~gt_lo & refresh & bool(prm.use_vision_updater)             # L264: the rows whose vision updater fires on this frame
    occl = ~gt_lo & bool(prm.use_vision_updater)                      # ... and those the live refresh counter may withhold it from
    joint_u, j33_u = torch.zeros(B, 24, 3, dtype=dt), torch.zeros(B, 33, 3, dtype=dt)
    if prm.use_reproj_opt or bool(occl.any()):
        _, joint, vert = ob.forward_kinematics(pose, tran)
        j_new = ob.landmarks(vert, joint)
        j33 = j_new if mut == "cached landmarks ignored in live mode" else torch.where(refresh.view(B, 1, 1), j_new, st.j_temp)
        if moves and prm.use_reproj_opt:
            st.j_temp = j33.clone()
        # what the updater reads (oracle/wiring_f64.py): the refinement below leaves the landmarks of a row with c <= lo alone
        joint_u, j33_u = torch.where(occl.view(B, 1, 1), joint, joint_u), torch.where(occl.view(B, 1, 1), j33, j33_u)
    if moves:
        st.count = torch.where(refresh, torch.full_like(st.count, prm.update_vision_freq), st.count - 1)
    # L245-261
    if prm.use_reproj_opt:
        def rsum(x):
            return x.flip(1).sum(dim=1) if rev else x.sum(dim=1)
        p, u2, v2 = j2dc[:, :, 2], j2dc[:, :, 0], j2dc[:, :, 1]
        jx, jy, jz = j33[..., 0], j33[..., 1], j33[..., 2]
        ax = rsum(p / jz.pow(2)) + prm.smooth
        tx, ty = p * (-jx / jz.pow(2) + u2 / jz), p * (-jy / jz.pow(2) + v2 / jz)
        s1 = torch.stack((rsum(tx) / ax, rsum(ty) / ax, torch.zeros(B, dtype=dt)), dim=1)
        j1 = j33 + s1.unsqueeze(1)
        jq = j33 if mut == "second refinement pass on the unshifted landmarks" else j1
        jx, jy, jz = jq[..., 0], jq[..., 1], jq[..., 2]
        az = rsum(p * (jx.pow(2) + jy.pow(2)) / jz.pow(4)) + prm.smooth
        tz = p * ((jx / jz - u2) * jx / jz.pow(2) + (jy / jz - v2) * jy / jz.pow(2))
        s2 = torch.stack((torch.zeros(B, dtype=dt), torch.zeros(B, dtype=dt), rsum(tz) / az), dim=1)
        tran = torch.where(gt_lo.unsqueeze(1), (tran + s1) + s2, tran)
        # the sums cancel: what went into them is the sum of the magnitudes of each term's two parts over the divisor (a shift
        # of all landmarks by the translation's own error moves the quotient by less than that error: a / (a + smooth) < 1)
        j0x, j0y, j0z = j33[..., 0], j33[..., 1], j33[..., 2]
        mx = (p * (j0x.abs() / j0z.pow(2) + u2.abs() / j0z.abs())).sum(1) / ax
        my = (p * (j0y.abs() / j0z.pow(2) + v2.abs() / j0z.abs())).sum(1) / ax
        mz = (p * (((jx / jz).abs() + u2.abs()) * jx.abs() + ((jy / jz).abs() + v2.abs()) * jy.abs()) / jz.pow(2)).sum(1) / az
        A = torch.where(gt_lo, A + (torch.maximum(mx, my) + mz).to(F64) + amax(tran), A)
    reach = is_hi & st.first_reach & bool(prm.use_imu_updater)
    st.first_reach = st.first_reach & ~reach
    st.last_tran = tran.clone()
    st.A = A
    rec = dict(regime=regime, use_vel=use_vel.long(), foot=torch.full((B,), foot), far=far.long(), appended=sample.long(),
               corr=corr, refresh=refresh.long(), n_floor=st.n_floor.clone(), reach=reach.long(), start=start.long(),
               count=st.count.clone(), upd=upd.long(), joint=joint_u, j33=j33_u)
    return pose, tran, rec, margins


# ----------------------------------------------------------------------------------------------------- cases
@dataclasses.dataclass
class Call:
    T: int
    first_tran: bool = False
    first_frame: bool = False
    reset: bool = False             # before the call: reset_states(rows=case.reset_rows)
    poke: dict = None               # before the call: parameters poked on the context (Params fields)


@dataclasses.dataclass
class Case:
    name: str
    kind: str                       # the contact / parameter situation; MUTATIONS refers to it
    situation: str                  # one of SITUATIONS
    prm: Params
    bias: dict                      # float32 tensors r6d [144], ct [2], vr [3], pc [3]
    calls: list
    oric: torch.Tensor              # [B,T,6,3,3] float32 (T over all calls)
    j2dc: torch.Tensor              # [B,T,33,3]
    gravity: torch.Tensor           # [B,3]
    first_tran: torch.Tensor        # [B,3]
    reset_rows: torch.Tensor        # [B] bool: the rows a masked reset clears

    @property
    def B(self):
        return self.oric.shape[0]

    @property
    def T(self):
        return self.oric.shape[1]

    def key(self):
        return (self.name, self.B)


SITUATIONS = ("foot 0", "foot 1", "tie above", "both below", "0 above 1 below", "1 above 0 below", "at threshold")


def state_dict(case):
    """every tensor zero except the four linear2 biases: each sub-net's output is its bias, exactly"""
    sd = {k: np.zeros(shape, np.float32) for k, shape in C.state_dict_spec()}
    for net, name in (("rnn7", "r6d"), ("rnn8", "ct"), ("rnn3", "vr"), ("rnn6", "pc")):
        sd[f"{net}.linear2.bias"] = case.bias[name].numpy().copy()
    return sd


def _logit(p):
    return float(np.log(p / (1.0 - p)))


def _r6d(seed, zero_joint=None):
    """24 generic rotations (angles up to ~1.2 rad about seeded axes) as scaled, sheared 6D vectors: |a|, |b| != 1, a.b != 0"""
    aa = 0.7 * synth.normal(seed, 1, 72).reshape(24, 3).astype(np.float64)
    R = synth._rodrigues(aa)
    u = synth.uniform01(seed, 2, 72).reshape(24, 3).astype(np.float64)
    a = R[:, :, 0] * (0.6 + u[:, :1])
    b = R[:, :, 1] * (0.6 + u[:, 1:2]) + (u[:, 2:3] - 0.5) * R[:, :, 0]
    r = np.concatenate((a, b), axis=1)
    if zero_joint is not None:
        r[zero_joint, :3] = 0.0                                    # NaN -> 0 (angular.py:262)
    return torch.from_numpy(r.reshape(144).astype(np.float32))


def _rows(seed, n, T, prm, far_rows):
    """n candidate rows x T frames: gravity g, Rcr = Q . Rot(u, yaw_t) . Rot(a, tilt_t) with Q u = g (so the yaw leaves the foot
    heights along gravity alone and the tilt moves them), a confidence per frame that interleaves the regimes, keypoints and a
    first_tran near pc (or well beyond the jump distance for `far_rows`)."""
    nrm = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)
    z = synth.normal(seed, 11, n * 12).reshape(n, 12).astype(np.float64)
    un = synth.uniform01(seed, 12, n * 8).reshape(n, 8).astype(np.float64)
    g = nrm(np.array([0.0, 1.0, 0.0]) + 0.12 * z[:, 0:3])
    u = nrm(z[:, 3:6])
    a = nrm(np.cross(u, z[:, 6:9]))
    w = np.cross(u, g)                                             # Q: the shortest rotation u -> g
    s, c = np.linalg.norm(w, axis=1, keepdims=True), (u * g).sum(1, keepdims=True)
    Q = synth._rodrigues(w / np.where(s < 1e-9, 1.0, s) * np.arctan2(s, c))
    tt = np.arange(T)[None, :]
    yaw = 6.28 * un[:, 0:1] + (0.02 + 0.06 * un[:, 1:2]) * tt
    amp = np.where(un[:, 2:3] < 0.3, 0.0, 0.35 * un[:, 3:4])
    tilt = amp * np.sin(0.45 * tt + 6.28 * un[:, 4:5])
    Rcr = Q[:, None] @ synth._rodrigues(u[:, None, :] * yaw[..., None]) @ synth._rodrigues(a[:, None, :] * tilt[..., None])
    oric = np.tile(np.eye(3), (n, T, 6, 1, 1))
    oric[:, :, 5] = Rcr
    # regimes: rows 0 mod 4 stay high (the floor fills at once); the others mix in runs of 1..3 frames
    lo, hi = prm.conf_range
    levels = np.array([hi + 0.07, lo + 0.4 * (hi - lo), lo - 0.2])
    r = synth.uniform01(seed, 13, n * T).reshape(n, T)
    reg = np.where(r < 0.62, 0, np.where(r < 0.8, 1, 2))
    reg = np.repeat(reg[:, ::2], 2, axis=1)[:, :T]
    reg[::4] = 0
    conf = levels[reg][..., None] + 0.02 * (synth.uniform01(seed, 14, n * T * 33).reshape(n, T, 33) - 0.5)
    pc = np.asarray(PC, np.float64)
    uv = (pc[:2] + 0.5 * synth.normal(seed, 15, n * T * 66).reshape(n, T, 33, 2)) / pc[2] + 0.03 * synth.normal(seed, 16, n * T * 2).reshape(n, T, 1, 2)
    j2dc = np.concatenate((uv, conf[..., None]), axis=-1)
    off = nrm(z[:, 9:12]) * (0.03 + 0.1 * un[:, 5:6])
    off = np.where(far_rows(np.arange(n))[:, None], nrm(z[:, 9:12]) * (0.8 + un[:, 5:6]), off)
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32))
    return f(oric), f(j2dc), f(g), f(pc + off), torch.from_numpy(un[:, 6] < 0.4)


PC = (0.3, 2.5, 4.0)
VR = (0.5, -0.2, 0.7)               # x vel_scale / 60: a few cm per frame
T1, T2 = 20, 12                     # frames of the two calls; T1 + T2 is a multiple of update_vision_freq + 1 in the live case


def _calls(variant, poke2=None):
    if variant == 0:
        return [Call(T1, first_tran=True), Call(T2, reset=True, poke=poke2)]
    if variant == 1:
        return [Call(T1, first_frame=True), Call(T2, first_tran=True, reset=True, poke=poke2)]
    if variant == 2:
        return [Call(T1), Call(T2, first_frame=True, reset=True, poke=poke2)]
    if variant == 3:
        return [Call(T1, first_tran=True, first_frame=True), Call(T2, poke=poke2)]
    return [Call(T1), Call(T2, poke=poke2)]


def _select(body, case, n):
    """the first n candidate rows on which every comparison of every frame keeps twice the margin `conditions` asks for
    (rows are independent in the tail, so choosing rows is choosing inputs)"""
    sim = simulate(O.OracleBody(body, dtype=F64), case)
    idx = _margin_ok(sim, 2.0 * COND_FACTOR).nonzero().flatten()[:n]
    assert idx.numel() == n, (case.name, int(idx.numel()), n)
    pickrows = lambda x: x[idx].contiguous()
    return dataclasses.replace(case, oric=pickrows(case.oric), j2dc=pickrows(case.j2dc), gravity=pickrows(case.gravity),
                               first_tran=pickrows(case.first_tran), reset_rows=pickrows(case.reset_rows))


def _margin_ok(sim, factor):
    ok = torch.ones(sim["tran"].shape[0], dtype=torch.bool)
    for name, margin, A, checked in sim["margins"]:
        need = factor * M * EPS32 * A
        if name == "cmax vs contact threshold":
            need = torch.full_like(need, CONTACT_KEEP)
        ok &= ~(checked & ~(margin > need)).any(dim=1)
    return ok


# name, kind, situation, batch, (p0, p1) contact probabilities or logits, call variant, parameter overrides, options
_SPEC = (
    ("foot0", "foot0", "foot 0", 5, (0.93, 0.81), 0, {}, {}),
    ("foot1", "foot1", "foot 1", 48, (0.78, 0.9), 1, {}, {}),
    ("tie", "tie", "tie above", 97, (0.85, 0.85), 2, {}, {}),
    ("below", "below", "both below", 5, (0.45, 0.6), 1, {}, {}),
    ("hi_lo", "hi_lo", "0 above 1 below", 4, (0.9, 0.3), 0, {"height_threshold": 0.06}, {}),
    ("lo_hi", "foot1", "1 above 0 below", 3, (0.2, 0.88), 3, {"height_threshold": 0.3}, {}),
    ("edge", "edge", "at threshold", 5, None, 2, {"contact_threshold": 0.5}, {}),
    ("far", "far", "foot 0", 48, (0.93, 0.81), 0, {"distance_threshold": 0.4}, {"far": True}),
    ("filter", "filter", "both below", 4, (0.45, 0.6), 0, {"tran_filter_num": 1.5}, {}),
    ("nan", "foot0", "foot 1", 5, (0.78, 0.9), 1, {}, {"zero_joint": 4}),
    ("noflat", "noflat", "foot 0", 5, (0.93, 0.81), 2, {"use_flat_floor": False}, {}),
    ("drop", "drop", "both below", 5, (0.45, 0.6), 4, {"contact_threshold": 0.3}, {"poke2": {"contact_threshold": 0.7}}),
    ("reproj", "reproj", "foot 0", 5, (0.93, 0.81), 1, {"use_reproj_opt": True, "smooth": 1.0}, {}),
    ("reproj_live", "reproj_live", "foot 1", 4, (0.78, 0.9), 1,
     {"use_reproj_opt": True, "live": True, "update_vision_freq": 3, "conf_range": (0.85, 0.9), "tran_filter_num": 0.01}, {}),
)


def build_cases(body, names=None):
    """The cases of tests/test_tail_bound_cpu.py and tests/test_gpu_tail_branches.py (14 contexts). Every case is two calls
    (T1 + T2 frames) with first_tran / first_frame given or not and a masked reset between them; rows differ in gravity, in the
    IMU-5 orientation per frame, in the regime per frame and in first_tran."""
    cases = []
    for i, (name, kind, situation, B, probs, variant, over, opt) in enumerate(_SPEC):
        if names is not None and name not in names:
            continue
        prm = Params(**over)
        ct = (0.0, 0.0) if probs is None else (_logit(probs[0]), _logit(probs[1]))
        bias = dict(r6d=_r6d(40 + i, opt.get("zero_joint")), ct=torch.tensor(ct, dtype=F32),
                    vr=torch.tensor(VR, dtype=F32), pc=torch.tensor(PC, dtype=F32))
        n_cand = 4 * B + 24
        far_rows = (lambda k: k % 2 == 0) if opt.get("far") else (lambda k: k < 0)
        oric, j2dc, g, ft, rr = _rows(100 + i, n_cand, T1 + T2, prm, far_rows)
        c = Case(name, kind, situation, prm, bias, _calls(variant, opt.get("poke2")), oric, j2dc, g, ft, rr)
        cases.append(_select(body, c, B))
    return cases


def simulate(ob, case, dtype=F64, order="plain", mut=None, state=None):
    """the case's calls through tail_step: pose [B,T,24,3,3], tran [B,T,3], rec {name: [B,T]}, margins [(name, margin [B,T],
    A [B,T], checked [B,T])], A [B,T] (the accumulated magnitude behind tran), the final State"""
    B = case.B
    st = State(B, dtype) if state is None else state
    bias, prm = case.bias, case.prm
    poses, trans, recs, margs, As = [], [], [], [], []
    t = 0
    for call in case.calls:
        if call.reset:
            st.reset(case.reset_rows)
        if call.poke:
            prm = dataclasses.replace(prm, **call.poke)
        for i in range(call.T):
            ft = case.first_tran.to(dtype) if (call.first_tran and i == 0) else None
            p, tr, rec, mg = tail_step(ob, st, bias, case.oric[:, t, 5].to(dtype), case.j2dc[:, t].to(dtype), case.gravity.to(dtype), ft,
                                       call.first_frame and i == 0, prm, order, mut)
            poses.append(p), trans.append(tr), recs.append(rec), margs.append(mg), As.append(st.A.clone())
            t += 1
    rec = {k: torch.stack([r[k] for r in recs], dim=1) for k in recs[0]}
    margins = [(margs[0][k][0], torch.stack([m[k][1] for m in margs], 1), torch.stack([m[k][2] for m in margs], 1),
                torch.stack([m[k][3] for m in margs], 1)) for k in range(len(margs[0]))]
    return dict(pose=torch.stack(poses, 1), tran=torch.stack(trans, 1), rec=rec, margins=margins, A=torch.stack(As, 1), state=st)


def conditions(body, case, sim=None):
    """Asserts, on every row and frame with nothing excluded, that each comparison's float64 margin is at least COND_FACTOR x
    the bound M eps32 A of the compared quantity (contact probabilities: CONTACT_KEEP), so that a float32 evaluation whose
    error is within the Bound takes the same branch. The c0 == c1 tie and the logit-0 / threshold-0.5 equality are exact by
    construction and exempt. Returns {comparison: smallest margin / need}."""
    sim = sim if sim is not None else simulate(O.OracleBody(body, dtype=F64), case)
    out = {}
    for name, margin, A, checked in sim["margins"]:
        need = COND_FACTOR * M * EPS32 * A
        if name == "cmax vs contact threshold":
            need = torch.full_like(need, CONTACT_KEEP)
        if bool(checked.any()):
            r = (margin / need)[checked]
            out[name] = float(r.min())
            assert out[name] > 1.0, (case.name, name, out[name])
    at_edge = float(case.bias["ct"].max()) == 0.0 and all(dataclasses.replace(case.prm, **(c.poke or {})).contact_threshold == 0.5 for c in case.calls)
    if not at_edge:
        for c in case.calls:
            thr = dataclasses.replace(case.prm, **(c.poke or {})).contact_threshold
            assert float((torch.sigmoid(case.bias["ct"].double()) - thr).abs().min()) >= CONTACT_KEEP, case.name
    return out


# ------------------------------------------------------------------------------------------------------ Bound
def oracle_run(body, case):
    """the float32 OracleNet on the case's zero-weight state dict: pose, tran and its own branch record per frame"""
    ora = O.OracleNet(body, batch=case.B, live=case.prm.live)
    ora.load_numpy_state_dict(state_dict(case))
    case.prm.poke_oracle(ora)
    ora.gravityc = case.gravity.clone()
    B = case.B
    acc = torch.zeros(B, 6, 3)
    poses, trans, tr = [], [], {k: [] for k in ("use_vel", "foot", "far", "n_floor_add", "n_floor", "reach")}
    t = 0
    for call in case.calls:
        if call.reset:
            ora.reset_states(case.reset_rows.nonzero().flatten())
        if call.poke:
            dataclasses.replace(case.prm, **call.poke).poke_oracle(ora)
        for i in range(call.T):
            p, x = ora.forward_batch(case.j2dc[:, t], acc, case.oric[:, t], case.first_tran if (call.first_tran and i == 0) else None,
                                     call.first_frame and i == 0)
            poses.append(p.clone()), trans.append(x.clone())
            for k in tr:
                tr[k].append(ora.trace[k].long().clone())
            if t == 0:                                        # the device that makes the tail testable: outputs ARE the biases
                seen = (ora.trace["c"] > ora.conf_range[0]) | bool(call.first_frame)      # (rnn6 steps on the rows that see the camera)
                assert torch.equal(ora.trace["vr"], case.bias["vr"].expand(B, 3)) and torch.equal(ora.trace["pc"][seen], case.bias["pc"].expand(B, 3)[seen])
                assert torch.equal(ora.trace["poseg6d"], case.bias["r6d"].expand(B, 144))
            t += 1
    return dict(pose=torch.stack(poses, 1), tran=torch.stack(trans, 1), rec={k: torch.stack(v, 1) for k, v in tr.items()})


GROUP_NAMES = ("tran",) + tuple(f"joint{j}" for j in range(24))


class Bound:
    """Bound(group) = M * max(e32, eps32 * A) against the float64 run `sim` of a case, per row and frame.
      tran     A is the accumulated magnitude of what went into the row's translation: reset where the translation is
               assigned (first_tran, first_frame, a jump to pc), else the previous frame's A plus the magnitudes of this
               frame's terms (the step, the fused pc, the floor correction, the refinement's sums over their divisor);
               e32 is the largest distance of the float32 evaluations from float64 on the row since that assignment --
               an error made in one frame stays in the running sum.
      joint j  A = 1 (rotation entries); e32 the largest distance over the rows and frames of the case (the pose of a row
               depends on its biases only, the root on the IMU alone).
    e32 comes from `evals32`: the float32 tail_step in two association orders and the float32 OracleNet."""

    def __init__(self, sim, evals32, m=M):
        self.sim, self.m = sim, m
        B, T = sim["tran"].shape[:2]
        e = torch.zeros(B, T, dtype=F64)
        ej = torch.zeros(24, dtype=F64)
        for ev in evals32:
            e = torch.maximum(e, (ev["tran"].to(F64) - sim["tran"]).abs().amax(dim=2))
            ej = torch.maximum(ej, (ev["pose"].to(F64) - sim["pose"]).abs().amax(dim=(0, 1, 3, 4)))
        start = sim["rec"]["start"].bool()
        run = torch.zeros(B, dtype=F64)
        for t in range(T):                                            # running maximum since the last assignment
            run = torch.where(start[:, t], e[:, t], torch.maximum(run, e[:, t]))
            e[:, t] = run
        self.e32_tran, self.e32_pose = e, ej
        self.tol_tran = m * torch.maximum(e, EPS32 * sim["A"])
        self.tol_pose = m * torch.maximum(ej, torch.full_like(ej, EPS32))

    def ratios(self, pose, tran, active=None):
        """error / Bound of the 25 groups: the translation, then each joint (inf where a value is not finite). `active` [B,T]
        leaves out the row-frames a ragged call did not run."""
        pose, tran = torch.as_tensor(pose).detach().cpu().to(F64), torch.as_tensor(tran).detach().cpu().to(F64)
        act = torch.ones_like(self.tol_tran, dtype=torch.bool) if active is None else active
        et = (tran - self.sim["tran"]).abs().amax(dim=2) / self.tol_tran
        ep = (pose - self.sim["pose"]).abs().amax(dim=(3, 4)) / self.tol_pose.view(1, 1, 24)
        et = torch.where(torch.isfinite(et), et, torch.full_like(et, np.inf))
        ep = torch.where(torch.isfinite(ep), ep, torch.full_like(ep, np.inf))
        et, ep = torch.where(act, et, torch.zeros_like(et)), torch.where(act.unsqueeze(2), ep, torch.zeros_like(ep))
        return np.concatenate(([float(et.max())], ep.amax(dim=(0, 1)).numpy()))


def bound_of(body, case):
    """(float64 run, Bound, {evaluation: ratios[25]}, the oracle's run) of a case"""
    sim = simulate(O.OracleBody(body, dtype=F64), case)
    ob32 = O.OracleBody(body, dtype=F32)
    e32 = {o: simulate(ob32, case, dtype=F32, order=o) for o in ORDERS}
    e32["oracle"] = oracle_run(body, case)
    b = Bound(sim, list(e32.values()))
    return sim, b, {k: b.ratios(v["pose"], v["tran"]) for k, v in e32.items()}, e32
