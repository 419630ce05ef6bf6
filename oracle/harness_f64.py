"""float64 restatement, cases and bounds of the evaluation harness's camera-frame inputs -- TEST INFRASTRUCTURE, NOT PRODUCT.

rc_camera_inputs_kernel / rc_camera_inputs_rows_kernel (rc_frame.hip) with the host routine camera_constants (rc_api.cpp), and the
host routines `labels` / `first_translations` of robustcap_amd/evaluate.py, against evaluate.py:38-51,70-73 of the reference run in
float64 on the float32 inputs the device gets (`restate`):
  K^-1 in float64 from the float32 K; pixels = float64(normalised keypoint) x image size; j2dc = rows 0 and 1 of K^-1 [u, v, 1] with
  the confidence copied; oric = R_cw ori; accc = acc R_cw^T; gravityc = R_cw (0, -1, 0); label root = R_cw R_0; label translation =
  R_cw t + t_cw.
Beside it stands `Ops`: the same formulas written once more over the small arithmetic object of oracle/pose_ops_f64.py (`Ar`: dtype,
association order of every sum of products, fused or separate multiply-add) with a `mut` switch for one-line wrong variants and an
`inv` switch for the route to K^-1: "adjugate" (float64 adjugate rounded once to float32, camera_constants' way) or "torch" (torch's
float32 LU inverse, the reference's way). `Ops(Ar(F64))` must agree with `restate` to 1e-6 of the Bound; `VARIANTS` are the honest
float32 evaluations; `MUTATIONS` the wrong ones (tests/test_harness_bound_cpu.py).

Bounds: Bound = M max(e32, eps32 A) per compared value.
  e32   |restate(float32) - restate(float64)|: plain float32 torch, K.inverse() in float32 included
  A     the sum of the absolute products of the value's dot product:
          j2dc          |Kinv_r0 u| + |Kinv_r1 v| + |Kinv_r2|
          oric, accc    sum_k |R_rk| |x_k|            (root: the same with R_0 for x; gravityc: |R_r1|)
          tran          sum_k |R_rk| |t_k| + |t_cw_r|
  M     per op (M_OF): the smallest power of two with which tests/test_harness_bound_cpu.py holds -- every honest float32 evaluation
        at most Bound / 3, every mutation at least 3 Bound on some case. profiles/harness_inputs_ratios.txt records the ratios.
The confidence column is a copy: it has no bound and is compared bit for bit (`conf_ratio`: 0 or inf).

Not covered here or in the tests built on this file: more than 65535 rows in one rc_camera_inputs_rows launch (grid y) and frame
counts beyond 2^31.
"""
import dataclasses

import numpy as np
import torch

from robustcap_amd import synth
from .pose_ops_f64 import EPS32, F32, F64, MARGIN, Ar, _rodrigues, _unit, ratio, t32  # noqa: F401  (MARGIN: the tests' factor 3)

OPS = ("j2dc", "accc", "oric", "gravityc", "tran", "root")
# M = 4 is the smallest power of two above MARGIN (the float32 evaluation that defines e32 sits at 1 / M). Measured on the CPU with
# M = 4, the worst honest float32 evaluation / Bound over the 8 variants: j2dc 0.619 (general K at 1 x 1), accc 0.514 (fx 1400 fy 900),
# oric 0.557 (K22 = 2), tran 0.573 (180 deg), root 0.374 (general K) -- e32 is taken per value and is often 0, and a three-term sum of
# products in another order or with fused adds lies up to 2.5 eps32 A from float64 -- all above 1 / 3, so these five take M = 8
# (0.309, 0.257, 0.279, 0.286, 0.187); gravityc is exact in every arithmetic (0.000) and keeps M = 4. oracle/harness_oracle.py and
# the host torch of evaluate.labels sit at 0.125 = 1 / M on every op: they are the arithmetic that defines e32. The smallest mutation
# ratio per op with these M: j2dc 5.8e3 (the skew term), accc 5.8e6, oric 7.9e6, gravityc 8.4e6, tran 2.1e6, root 4.4e6.
# The reference's own route, float32 K.inverse(): its e32 / (eps32 A) on j2dc is at most 1.647 on the skewed K (at 1 x 1) and 1.904 on
# the general K (third row (1e-4, 0, 1), at 1 x 1), which is also the largest over all cases -- a float32 LU inverse of these K costs
# less than two roundings of A, no more than the dot product itself.
M_OF = {"j2dc": 8.0, "accc": 8.0, "oric": 8.0, "gravityc": 4.0, "tran": 8.0, "root": 8.0}

# mutation -> (the op that must show it, a word of a case it must show on); profiles/harness_inputs_ratios.txt has the ratios
MUTATIONS = {
    "oric_R_transposed": ("oric", "2 rad about (1,2,3)"),
    "accc_R_transposed": ("accc", "2 rad about (1,2,3)"),
    "oric_ori_times_R": ("oric", "2 rad about (1,2,3)"),
    "kinv_of_K_transposed": ("j2dc", "synthetic camera 1920x1080"),
    "image_size_swapped": ("j2dc", "synthetic camera 1920x1080"),
    "kinv_no_constant_column": ("j2dc", "principal point (300, 900)"),
    "kinv_no_skew_term": ("j2dc", "skew 3.5 1920x1080"),
    "gravity_sign": ("gravityc", "synthetic camera 1920x1080"),
    "gravity_row_1": ("gravityc", "90 deg about x"),
    "accc_imu_5_minus_i": ("accc", "synthetic camera 1920x1080"),
    "conf_scaled": ("conf", "synthetic camera 1920x1080"),
    "tran_no_t_cw": ("tran", "synthetic camera 1920x1080"),
    "root_right": ("root", "2 rad about (1,2,3)"),
}
# a transposition of R_cw cannot show on a symmetric R_cw: these (mutation, case word) pairs must give exactly the honest result
INVISIBLE = (("oric_R_transposed", "180 deg"), ("accc_R_transposed", "180 deg"), ("gravity_row_1", "180 deg"), ("image_size_swapped", "1x1"))


# ------------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass
class Case:
    name: str
    kp: np.ndarray              # [T,33,3] float32 (u / width, v / height, confidence)
    acc: np.ndarray             # [T,6,3] world frame
    ori: np.ndarray             # [T,6,3,3] world frame
    K: np.ndarray               # [3,3]
    Tcw: np.ndarray             # [4,4]
    size: tuple                 # (width, height)
    tran: np.ndarray            # [T,3] label translation, world frame
    root: np.ndarray            # [T,3,3] label root rotation, world frame

    def frames(self, T):
        """the first T frames"""
        return dataclasses.replace(self, kp=self.kp[:T], acc=self.acc[:T], ori=self.ori[:T], tran=self.tran[:T], root=self.root[:T])


T_FRAMES = 3
CONF_EDGES = (0.0, 1.0, -0.0, 1e-40, 0.85)                      # keypoints 0..4 of frame 0 (1e-40 is a float32 denormal)
KP_EDGES = ((0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0), (-0.5, 1.7), (1.7, -0.5))      # keypoints 0..5 of frame 0
SIZES = ((1920, 1080), (1280, 720), (4096, 2160), (1, 1))


def synth_camera(seed=11, image_size=(1920, 1080)):
    """(K, T_cw) float64 by the expressions of synth.make_dataset for a camera c > 0: within 0.25 rad of the identity, no skew"""
    W, H = image_size
    u = synth.uniform01(seed * 977, 51, 8).astype(np.float64)
    Rcw = _rodrigues(np.array([0.05 * (u[1] - 0.5), 0.5 * (u[0] - 0.5), 0.03 * (u[2] - 0.5)]))
    Tcw = np.eye(4)
    Tcw[:3, :3], Tcw[:3, 3] = Rcw, np.array([0.4 * (u[3] - 0.5), 0.2 * (u[4] - 0.5), 3.0 + 0.6 * u[5]])
    f = 1400.0 + 200.0 * u[6]
    return np.array([[f, 0.0, W / 2 + 20 * (u[7] - 0.5)], [0.0, f * 1.002, H / 2], [0.0, 0.0, 1.0]]), Tcw


def _with_R(Tcw, R):
    out = Tcw.copy()
    out[:3, :3] = R
    return out


def _with_K(K, **entries):
    out = K.copy()
    for k, v in entries.items():
        out[int(k[1]), int(k[2])] = v
    return out


def cameras():
    """[(name, K, T_cw)] float64: the cameras of the issue's list; a rotation variant keeps the synthetic K, a K variant the
    synthetic T_cw"""
    K, Tcw = synth_camera()
    a = _unit((1.0, 2.0, 3.0))
    Rx = np.array([[1.0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])
    Ry = np.array([[0, 0, 1.0], [0, 1.0, 0], [-1.0, 0, 0]])
    Rz = np.array([[0, -1.0, 0], [1.0, 0, 0], [0, 0, 1.0]])
    return [("synthetic camera", K, Tcw),
            ("90 deg about x", K, _with_R(Tcw, Rx)), ("90 deg about y", K, _with_R(Tcw, Ry)), ("90 deg about z", K, _with_R(Tcw, Rz)),
            ("2 rad about (1,2,3)/sqrt14", K, _with_R(Tcw, _rodrigues(2.0 * a))),
            ("180 deg about (1,2,3)/sqrt14", K, _with_R(Tcw, 2.0 * np.outer(a, a) - np.eye(3))),
            ("skew 3.5", _with_K(K, k01=3.5), Tcw),
            ("fx 1400 fy 900", _with_K(K, k00=1400.0, k11=900.0), Tcw),
            ("principal point (300, 900)", _with_K(K, k02=300.0, k12=900.0), Tcw),
            ("K22 = 2", _with_K(K, k22=2.0), Tcw),
            ("general K, third row (1e-4, 0, 1)", np.array([[1450.0, 2.0, 950.0], [-1.5, 1390.0, 560.0], [1e-4, 0.0, 1.0]]), Tcw)]


OTHER_SIZE_CAMERAS = ("synthetic camera", "skew 3.5", "K22 = 2", "general K")


def frames(Rcw, seed):
    """T_FRAMES frames (kp, acc, ori, tran, root) float64 holding the frame contents of the issue's list; Rcw: the camera's rotation
    (two accelerations are built orthogonal to one of its rows)"""
    T = T_FRAMES
    kp = np.empty((T, 33, 3))
    kp[..., :2] = 0.05 + 0.9 * synth.uniform01(seed, 0, T * 66).astype(np.float64).reshape(T, 33, 2)      # inside the image
    kp[..., 2] = 0.2 + 0.8 * synth.uniform01(seed, 1, T * 33).astype(np.float64).reshape(T, 33)
    for k, uv in enumerate(KP_EDGES):
        kp[0, k, :2] = uv
    kp[0, :len(CONF_EDGES), 2] = CONF_EDGES
    kp[T - 1, 32] = (1.0, 0.0, 1e-40)                                                  # the last thread of the last frame
    acc = 3.0 * synth.normal(seed, 2, T * 18).astype(np.float64).reshape(T, 6, 3)
    d = _unit(synth.normal(seed, 3, 12).reshape(4, 3))
    Rf = np.asarray(Rcw, np.float32).astype(np.float64)                                # the rows the device multiplies with
    acc[0, 0] = 0.0
    acc[0, 1] = 9.8 * d[0]
    acc[0, 2] = 1e3 * d[1]
    acc[0, 3] = 9.8 * _unit(np.cross(Rf[0], d[2]))                                     # accc[0, 3, 0] cancels, its A does not
    acc[0, 4] = (0.0, -9.8, 0.0)
    acc[1, 5] = 1e3 * _unit(np.cross(Rf[2], d[3]))
    ori = _rodrigues(1.5 * synth.normal(seed, 4, T * 18).astype(np.float64).reshape(T, 6, 3))
    ori[0, 0] = np.eye(3)
    ori[1, 5] = 2.0 * synth.normal(seed, 5, 9).astype(np.float64).reshape(3, 3)        # not orthonormal: a plain product all the same
    tran = np.array([0.3, 0.9, -0.2]) + 0.5 * synth.normal(seed, 6, T * 3).astype(np.float64).reshape(T, 3)
    tran[1] = (100.0, -50.0, 30.0)
    tran[2] = 0.0
    root = _rodrigues(1.2 * synth.normal(seed, 7, T * 3).astype(np.float64).reshape(T, 3))
    root[0] = np.eye(3)
    return kp, acc, ori, tran, root


def case_of(name, K, Tcw, size, seed):
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float32))
    kp, acc, ori, tran, root = frames(np.asarray(Tcw)[:3, :3], seed)
    return Case(f"{name} {size[0]}x{size[1]}", f32(kp), f32(acc), f32(ori), f32(K), f32(Tcw), tuple(size), f32(tran), f32(root))


def cases():
    """the named cases the CPU and the GPU tests share: every camera at 1920 x 1080, four of them at the other image sizes"""
    out = []
    for i, (name, K, Tcw) in enumerate(cameras()):
        for size in SIZES:
            if size == SIZES[0] or name.startswith(OTHER_SIZE_CAMERAS):
                out.append(case_of(name, K, Tcw, size, 200 + i))
    return out


def nan_case():
    """the synthetic camera with one keypoint coordinate NaN (frame 1, keypoint 7, u)"""
    c = cases()[0]
    kp = c.kp.copy()
    kp[1, 7, 0] = np.nan
    return dataclasses.replace(c, name="NaN keypoint: " + c.name, kp=kp)


# ------------------------------------------------------------------------------------------ restatement and Bound
def restate(c, dtype=F64):
    """evaluate.py:38-51,70-73 and the labels of evaluate.py:46-49 in torch at `dtype` on the float32 inputs"""
    cv = lambda a: t32(a).to(dtype)
    K, Tcw = cv(c.K).reshape(3, 3), cv(c.Tcw).reshape(4, 4)
    R, t = Tcw[:3, :3], Tcw[:3, 3]
    kp = cv(c.kp)
    pix = torch.stack((kp[..., 0] * c.size[0], kp[..., 1] * c.size[1], torch.ones_like(kp[..., 0])), dim=-1)
    j = (torch.linalg.inv(K) @ pix.unsqueeze(-1)).squeeze(-1)
    return {"j2dc": j[..., :2], "accc": cv(c.acc) @ R.T, "oric": R @ cv(c.ori), "gravityc": R @ torch.tensor([0.0, -1.0, 0.0], dtype=dtype),
            "tran": cv(c.tran) @ R.T + t, "root": R @ cv(c.root)}


def magnitudes(c):
    """A of every op (float64)"""
    cv = lambda a: t32(a).double().abs()
    Ki = torch.linalg.inv(t32(c.K).double().reshape(3, 3)).abs()
    Ra, ta = cv(c.Tcw)[:3, :3], cv(c.Tcw)[:3, 3]
    kp = cv(c.kp)
    u, v = kp[..., 0] * c.size[0], kp[..., 1] * c.size[1]
    Aj = torch.stack([Ki[r, 0] * u + Ki[r, 1] * v + Ki[r, 2] for r in (0, 1)], dim=-1)
    return {"j2dc": Aj, "accc": cv(c.acc) @ Ra.T, "oric": Ra @ cv(c.ori), "gravityc": Ra[:, 1].clone(), "tran": cv(c.tran) @ Ra.T + ta,
            "root": Ra @ cv(c.root)}


def reference(c):
    """{op: (float64 reference, Bound, e32 / (eps32 A))}"""
    ref, p32, A = restate(c), restate(c, F32), magnitudes(c)
    out = {}
    for op in OPS:
        e32 = (p32[op].double() - ref[op]).abs()
        out[op] = (ref[op], M_OF[op] * torch.maximum(e32, EPS32 * A[op]), ratio(e32, EPS32 * A[op]))
    return out


def value_ratios(ref, bnd, got):
    """|got - ref| / Bound per value; a non-finite reference value must be matched in kind (NaN / +inf / -inf), else inf"""
    got = torch.as_tensor(got).double().reshape(ref.shape)
    fin = torch.isfinite(ref)
    same = torch.where(fin, torch.isfinite(got), (torch.isnan(got) == torch.isnan(ref)) & ((got == ref) | torch.isnan(ref)))
    err = torch.where(fin & torch.isfinite(got), got - ref, torch.zeros_like(ref))
    r = ratio(err, torch.where(fin, bnd, torch.ones_like(bnd)))
    return torch.where(same, r, torch.full_like(r, float("inf")))


def conf_ratio(c, got_conf):
    """0 where the confidence column is bitwise the input's (-0.0 and the denormal included), inf elsewhere"""
    want = t32(c.kp)[..., 2].contiguous().view(torch.int32)
    got = torch.as_tensor(got_conf).float().contiguous().view(torch.int32).reshape(want.shape)
    return torch.where(got == want, 0.0, float("inf")).double()


def all_ratios(c, got, ref=None):
    """{op: worst ratio} of the outputs `got` ({op: tensor}, "conf" optional) of case `c`"""
    ref = reference(c) if ref is None else ref
    out = {op: float(value_ratios(ref[op][0], ref[op][1], got[op]).max()) if ref[op][0].numel() else 0.0 for op in OPS if op in got}
    if "conf" in got:
        out["conf"] = float(conf_ratio(c, got["conf"]).max()) if c.kp.size else 0.0
    return out


# ------------------------------------------------------------------------------------------------ the arithmetic
class Ops:
    """the six ops over one arithmetic; `mut` names a single wrong line; `inv`: the route to K^-1 in float32"""

    def __init__(self, ar=Ar(), mut=None, inv="adjugate"):
        self.ar, self.mut, self.inv = ar, mut, inv

    def c(self, x):
        return t32(x).to(self.ar.dtype)

    def kinv(self, K):
        K = t32(K).reshape(3, 3)
        if self.mut == "kinv_of_K_transposed":
            K = K.t().contiguous()
        if self.inv == "torch" and self.ar.dtype == F32:
            return torch.linalg.inv(K)
        a, b, c, d, e, f, g, h, i = K.double().reshape(9)                               # camera_constants: the adjugate in double,
        det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)          # every entry divided by det, rounded once
        adj = torch.stack((e * i - f * h, c * h - b * i, b * f - c * e, f * g - d * i, a * i - c * g, c * d - a * f,
                           d * h - e * g, b * g - a * h, a * e - b * d))
        return (adj / det).reshape(3, 3).to(self.ar.dtype)

    def run(self, cs):
        """{op: tensor in the arithmetic's dtype} + "conf" (float32)"""
        ar, m = self.ar, self.mut
        W, H = (cs.size[1], cs.size[0]) if m == "image_size_swapped" else cs.size
        Ki, Tcw = self.kinv(cs.K), self.c(cs.Tcw).reshape(4, 4)
        R, t = Tcw[:3, :3], Tcw[:3, 3]
        kp = self.c(cs.kp)
        u, v = kp[..., 0] * W, kp[..., 1] * H                                           # rounded to the dtype like the device's pixels
        one = torch.ones_like(u)
        rows = []
        for r in (0, 1):
            pairs = [(Ki[r, 0], u), (Ki[r, 1], v), (Ki[r, 2], one)]
            if m == "kinv_no_constant_column":
                pairs = pairs[:2]
            if m == "kinv_no_skew_term" and r == 0:
                del pairs[1]
            rows.append(ar.sp(pairs))
        conf = kp[..., 2] * (1.0 + 2.0 ** -20) if m == "conf_scaled" else kp[..., 2]
        acc = self.c(cs.acc)
        if m == "accc_imu_5_minus_i":
            acc = acc.flip(-2)
        ori, root = self.c(cs.ori), self.c(cs.root)
        e = torch.tensor([0.0, 1.0 if m == "gravity_sign" else -1.0, 0.0], dtype=ar.dtype)
        tran = ar.mv(R, self.c(cs.tran))
        return {"j2dc": torch.stack(rows, dim=-1), "conf": conf.float(),
                "accc": ar.mv(R.t() if m == "accc_R_transposed" else R, acc),
                "oric": ar.mm(ori, R) if m == "oric_ori_times_R" else ar.mm(R.t() if m == "oric_R_transposed" else R, ori),
                "gravityc": ar.mv(R.t() if m == "gravity_row_1" else R, e),
                "tran": tran if m == "tran_no_t_cw" else tran + t,
                "root": ar.mm(root, R) if m == "root_right" else ar.mm(R, root)}


VARIANTS = tuple((Ar(F32, o, f), inv) for o in ("fwd", "rev") for f in (False, True) for inv in ("adjugate", "torch"))


class Worst:
    """the largest ratio per op and the case it came from"""

    def __init__(self):
        self.w = {}

    def note(self, ratios, name):
        for op, v in ratios.items():
            if op not in self.w or v > self.w[op][0]:
                self.w[op] = (v, name)

    def lines(self, title):
        return [title] + [f"  {op:9s} " + (f"M = {M_OF[op]:g}" if op in M_OF else "bitwise") + f"  {v:.3f}  ({nm})" for op, (v, nm) in sorted(self.w.items())]
