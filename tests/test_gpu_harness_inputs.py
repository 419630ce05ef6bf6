"""rc_camera_inputs_kernel, rc_camera_inputs_rows_kernel (rc_frame.hip), camera_constants (rc_api.cpp) and the host routines
`labels` / `first_translations` of robustcap_amd/evaluate.py against the float64 restatement of oracle/harness_f64.py.

  values      every case of harness_f64.cases (cameras far from the identity, K with skew / K22 = 2 / a general third row, four image
              sizes, keypoints on and outside the image edge, accelerations that cancel, a non-orthonormal orientation) through
              evaluate.camera_inputs and again as rows of rc_camera_inputs_rows calls: every output within Bound = M max(e32, eps32 A)
              of float64, the confidence column bitwise the input (-0.0 and the denormal included), gravityc within its Bound; a NaN
              keypoint coordinate poisons exactly what it poisons in the float32 oracle; T = 0 and T = 1 of the single-row kernel.
  labels      evaluate.labels within the Bound of R_cw R_0 and R_cw t + t_cw on cameras far from the identity, the other joints
              untouched, and first_translations == labels(...)[1][0] bit for bit on every row of a ragged three-camera dataset
              (`labels` runs the HIP axis-angle kernel, so this cannot stand in the CPU file).
  layout      one rc_camera_inputs_rows call over buffers the test owns: NaN in every padded input frame and in the outputs, 64
              sentinel floats behind each output and behind the camera scratch; frames < len bitwise the single-row kernel, frames
              >= len exactly +0.0 / the identity, no NaN left, no sentinel touched, rows of one sequence equal only under equal cameras.
              (Row (2, 0) has a K with skew, as have cases of `values`: as first written the two kernels were contracted differently by
              the compiler and agreed bitwise only where K[0][1] = K[1][0] = 0; see cam_unproject in rc_frame.hip.)
  arguments   a singular K, a non-finite K or upper 3 x 4 of T_cw, a K whose inverse overflows float32 and null buffers are
              RC_ERR_INVALID and leave device outputs and the host gravity array untouched, whichever row is the bad one.
tests/test_harness_bound_cpu.py shows on the CPU that honest float32 evaluations stay within a third of these bounds and every
mutation lands beyond three times them. RC_HARNESS_RATIOS_OUT=<file> keeps the worst error / Bound per op and its case.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import harness_f64 as Hf
from oracle import harness_oracle as HO

pytestmark = pytest.mark.gpu
WORST = {"evaluate.camera_inputs (rc_camera_inputs_kernel)": Hf.Worst(), "rc_camera_inputs_rows_kernel": Hf.Worst(),
         "evaluate.labels (host torch behind the HIP axis-angle kernel)": Hf.Worst()}
SINGLE_W, ROWS_W, LABELS_W = WORST.values()
RC_OK, RC_ERR_INVALID = 0, -1
TAIL = 64
SENTINEL = 12345.678


def bits(a):
    return torch.as_tensor(a).contiguous().cpu().view(torch.int32)


def bits_equal(a, b):
    """bitwise equality (NaN equals the same NaN, -0 differs from +0)"""
    a, b = bits(a), bits(b)
    return a.shape == b.shape and torch.equal(a, b)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def hp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def suite():
    """[(case, reference)] computed once"""
    return [(c, Hf.reference(c)) for c in Hf.cases()]


def single(c):
    from robustcap_amd.evaluate import camera_inputs
    j, a, o, g = camera_inputs(c.kp, c.acc, c.ori, c.K, c.Tcw, image_size=c.size)
    j = j.cpu()
    return {"j2dc": j[..., :2], "conf": j[..., 2], "accc": a.cpu(), "oric": o.cpu(), "gravityc": g}


class RowsCall:
    """one rc_camera_inputs_rows call on buffers this test owns: outputs prefilled with NaN, TAIL sentinel floats behind each output
    and behind the 72-byte-per-row camera scratch, the host gravity array prefilled with NaN"""

    def __init__(self, kp, acc, ori, seq_of_row, lens, K, Tcw, size, Tmax, n_rows=None, null=()):
        from robustcap_amd import _lib
        n = len(seq_of_row) if n_rows is None else n_rows
        self.n, self.Tmax = max(n, 0), max(Tmax, 0)                               # (a negative count is passed on; the buffers are sized by 0)
        n_arg, T_arg, n, Tmax = n, Tmax, self.n, self.Tmax
        self.inputs = [dev(np.asarray(kp, np.float32)), dev(np.asarray(acc, np.float32)), dev(np.asarray(ori, np.float32)),
                       dev(np.asarray(seq_of_row, np.int32)), dev(np.asarray(lens, np.int32))]
        self.sizes = [n * Tmax * 99, n * Tmax * 18, n * Tmax * 54]
        self.flat = []
        for m in self.sizes + [n * 18]:
            t = torch.full((m + TAIL,), float("nan"), device="cuda")
            t[m:] = SENTINEL
            self.flat.append(t)
        self.flat[3][:n * 18] = SENTINEL                                         # the scratch holds no output: sentinel throughout
        self.before = [bits(t) for t in self.flat]
        self.grav = np.full((n, 3), np.nan, np.float32)
        K, Tcw = np.ascontiguousarray(K, np.float32), np.ascontiguousarray(Tcw, np.float32)
        args = {"kp": _lib.ptr(self.inputs[0]), "acc": _lib.ptr(self.inputs[1]), "ori": _lib.ptr(self.inputs[2]), "sor": _lib.ptr(self.inputs[3]),
                "len": _lib.ptr(self.inputs[4]), "K": hp(K), "Tcw": hp(Tcw), "j": _lib.ptr(self.flat[0]), "a": _lib.ptr(self.flat[1]),
                "o": _lib.ptr(self.flat[2]), "g": hp(self.grav), "scratch": _lib.ptr(self.flat[3])}
        for k in null:
            args[k] = None
        self.rc = _lib.load().rc_camera_inputs_rows(args["kp"], args["acc"], args["ori"], args["sor"], args["len"], args["K"], args["Tcw"],
                                                    float(size[0]), float(size[1]), n_arg, T_arg, args["j"], args["a"], args["o"], args["g"],
                                                    args["scratch"], _lib.stream_ptr())
        torch.cuda.synchronize()

    def outputs(self):
        n, T = self.n, self.Tmax
        return (self.flat[0][:self.sizes[0]].view(n, T, 33, 3).cpu(), self.flat[1][:self.sizes[1]].view(n, T, 6, 3).cpu(),
                self.flat[2][:self.sizes[2]].view(n, T, 6, 3, 3).cpu())

    def tails_untouched(self):
        return all(torch.equal(bits(t[m:]), b[m:]) for t, b, m in zip(self.flat[:3], self.before[:3], self.sizes)) and \
            torch.equal(bits(self.flat[3][self.n * 18:]), self.before[3][self.n * 18:])

    def untouched(self):
        """nothing was launched or copied: every device buffer and the host gravity array are as they were"""
        return all(torch.equal(bits(t), b) for t, b in zip(self.flat, self.before)) and bool(np.isnan(self.grav).all())


# ----------------------------------------------------------------------------------------------------------- values
def test_every_case_within_its_float64_bound_single_row(suite):
    failed = []
    for c, ref in suite:
        got = single(c)
        r = Hf.all_ratios(c, got, ref)
        SINGLE_W.note(r, c.name)
        print(f"{c.name:48s} " + "  ".join(f"{op} {v:.3f}" for op, v in r.items()))
        failed += [(c.name, op, v) for op, v in r.items() if not v <= 1.0]
        for T in (1, 0):                                                        # fewer frames: the same bits, an empty launch
            few = single(c.frames(T))
            assert all(bits_equal(few[op], got[op][:T]) for op in ("j2dc", "conf", "accc", "oric")), (c.name, T)
            assert bits_equal(few["gravityc"], got["gravityc"]) and few["oric"].shape == (T, 6, 3, 3)
    assert not failed, failed


def test_every_case_within_its_float64_bound_as_rows_of_the_batched_kernel(suite):
    failed = []
    for size in Hf.SIZES:
        group = [(c, ref) for c, ref in suite if c.size == size]
        for k in range(0, len(group), 5):                                       # at most five rows a call, each its own sequence
            part = group[k:k + 5]
            n, T = len(part), Hf.T_FRAMES
            call = RowsCall(np.stack([c.kp for c, _ in part]), np.stack([c.acc for c, _ in part]), np.stack([c.ori for c, _ in part]),
                            np.arange(n), [T] * n, np.stack([c.K for c, _ in part]), np.stack([c.Tcw for c, _ in part]), size, T)
            assert call.rc == RC_OK and call.tails_untouched()
            j, a, o = call.outputs()
            for r, (c, ref) in enumerate(part):
                got = {"j2dc": j[r, ..., :2], "conf": j[r, ..., 2], "accc": a[r], "oric": o[r], "gravityc": torch.from_numpy(call.grav[r])}
                ratios = Hf.all_ratios(c, got, ref)
                ROWS_W.note(ratios, c.name)
                failed += [(c.name, op, v) for op, v in ratios.items() if not v <= 1.0]
                one = single(c)
                assert all(bits_equal(got[op], one[op]) for op in got), c.name
    assert not failed, failed


def test_a_nan_keypoint_poisons_what_it_poisons_in_the_float32_oracle():
    c = Hf.nan_case()
    ref = Hf.reference(c)
    want = HO.camera_inputs(c.kp, c.acc, c.ori, c.K, c.Tcw, image_size=c.size)[0]
    call = RowsCall(c.kp[None], c.acc[None], c.ori[None], [0], [Hf.T_FRAMES], c.K[None], c.Tcw[None], c.size, Hf.T_FRAMES)
    assert call.rc == RC_OK
    j = call.outputs()[0][0]
    for got in (single(c), {"j2dc": j[..., :2], "conf": j[..., 2]}):
        full = torch.cat((got["j2dc"], got["conf"][..., None]), dim=-1)
        assert torch.equal(torch.isnan(full), torch.isnan(want)) and int(torch.isnan(full).sum()) == 2      # x and y of that keypoint
        r = Hf.all_ratios(c, got, ref)                                          # the NaN matched in kind, every other value bounded
        assert all(v <= 1.0 for v in r.values()), r


# ----------------------------------------------------------------------------------------------------------- labels
def test_labels_within_their_bound_and_first_translations_bitwise(synth_assets):
    from robustcap_amd import evaluate as ev
    from robustcap_amd import synth
    from robustcap_amd.body import axis_angle_to_rotation_matrix
    ds = synth.make_dataset(9, 3, 16, synth_assets["body"], n_cam=3)
    for i, T in ((1, 9), (2, 1)):                                               # ragged
        for k in ("pose", "tran", "imu_ori", "imu_acc"):
            ds[k][i] = ds[k][i][:T]
        ds["joint2d_mp"][i] = ds["joint2d_mp"][i][:, :T]
    cams = {nm: Tcw for nm, _, Tcw in Hf.cameras()}
    hard = [cams[k] for k in ("2 rad about (1,2,3)/sqrt14", "90 deg about x", "180 deg about (1,2,3)/sqrt14")]
    for i in range(3):
        for j in range(3):
            ds["cam_T"][i][j] = hard[(i + j) % 3].astype(np.float32)
    rows = ev.rows_of(ds)
    assert len(rows) == 9
    ft = ev.first_translations(ds, rows)
    failed = []
    for r, (i, j) in enumerate(rows):
        pose, tran = ev.labels(ds, i, j)
        assert bits_equal(ft[r], tran[0]), (i, j)
        local = axis_angle_to_rotation_matrix(torch.from_numpy(ds["pose"][i]).reshape(-1, 3)).view(-1, 24, 3, 3).cpu()
        assert bits_equal(pose[:, 1:], local[:, 1:]), (i, j)
        T = len(ds["pose"][i])
        c = Hf.Case(f"sequence {i} camera {j}", ds["joint2d_mp"][i][j], ds["imu_acc"][i], ds["imu_ori"][i], ds["cam_K"][i][j],
                    ds["cam_T"][i][j], (1920, 1080), ds["tran"][i], local[:, 0].numpy())
        assert c.tran.shape == (T, 3)
        ratios = Hf.all_ratios(c, {"tran": tran, "root": pose[:, 0]})
        LABELS_W.note(ratios, c.name)
        failed += [(c.name, op, v) for op, v in ratios.items() if not v <= 1.0]
    assert not failed, failed


# ----------------------------------------------------------------------------------------------------------- layout
LAYOUT_ROWS = [(2, 1), (0, 0), (2, 0), (1, 2), (0, 1)]
LAYOUT_LEN = {0: 7, 1: 0, 2: 4}


def _layout_dataset():
    """three sequences of 7 frames (the lengths cut them), cameras per (sequence, camera): (0, 0) and (0, 1) are the same camera,
    (2, 0) and (2, 1) differ in K and in R_cw"""
    cams = {nm: (K, Tcw) for nm, K, Tcw in Hf.cameras()}
    cam_of = {(0, 0): "2 rad about (1,2,3)/sqrt14", (0, 1): "2 rad about (1,2,3)/sqrt14", (2, 0): "skew 3.5", (2, 1): "90 deg about z",
              (1, 2): "general K, third row (1e-4, 0, 1)"}
    seqs, kps = {}, {}
    for i in range(3):
        parts = [Hf.frames(np.eye(3), 300 + 10 * i + k) for k in range(3)]
        seqs[i] = (np.concatenate([p[1] for p in parts])[:7].astype(np.float32), np.concatenate([p[2] for p in parts])[:7].astype(np.float32))
    for r, ij in enumerate(LAYOUT_ROWS):
        kps[ij] = np.concatenate([Hf.frames(np.eye(3), 400 + 10 * r + k)[0] for k in range(3)])[:7].astype(np.float32)
    return {ij: tuple(np.asarray(x, np.float32) for x in cams[nm]) for ij, nm in cam_of.items()}, seqs, kps


@pytest.mark.parametrize("Tmax", (7, 1))
def test_batched_layout_padding_and_sentinels(Tmax):
    from robustcap_amd.evaluate import camera_inputs
    size = (1920, 1080)
    cam, seqs, kps = _layout_dataset()
    n = len(LAYOUT_ROWS)
    lens = [min(LAYOUT_LEN[i], Tmax) for i, _ in LAYOUT_ROWS]
    kp = np.full((n, Tmax, 33, 3), np.nan, np.float32)
    acc = np.full((3, Tmax, 6, 3), np.nan, np.float32)
    ori = np.full((3, Tmax, 6, 3, 3), np.nan, np.float32)
    for i in range(3):
        T = min(LAYOUT_LEN[i], Tmax)
        acc[i, :T], ori[i, :T] = seqs[i][0][:T], seqs[i][1][:T]
    for r, ij in enumerate(LAYOUT_ROWS):
        kp[r, :lens[r]] = kps[ij][:lens[r]]
    assert np.isnan(kp).any() and np.isnan(acc[1]).all() and sorted(lens) == sorted(min(v, Tmax) for v in (4, 7, 4, 0, 7))
    call = RowsCall(kp, acc, ori, [i for i, _ in LAYOUT_ROWS], lens, np.stack([cam[ij][0] for ij in LAYOUT_ROWS]),
                    np.stack([cam[ij][1] for ij in LAYOUT_ROWS]), size, Tmax)
    assert call.rc == RC_OK
    assert call.tails_untouched()
    j, a, o = call.outputs()
    assert not torch.isnan(j).any() and not torch.isnan(a).any() and not torch.isnan(o).any()
    eye = torch.eye(3)
    for r, (ij, T) in enumerate(zip(LAYOUT_ROWS, lens)):
        k1, a1, o1, g1 = camera_inputs(kp[r, :T], acc[ij[0], :T], ori[ij[0], :T], cam[ij][0], cam[ij][1], image_size=size)
        assert bits_equal(j[r, :T], k1) and bits_equal(a[r, :T], a1) and bits_equal(o[r, :T], o1) and bits_equal(call.grav[r], g1), ij
        assert int(bits(j[r, T:]).abs().sum()) == 0 and int(bits(a[r, T:]).abs().sum()) == 0, ij      # +0.0 bitwise, not -0.0
        assert bits_equal(o[r, T:], eye.expand(Tmax - T, 6, 3, 3)), ij
    row = {ij: r for r, ij in enumerate(LAYOUT_ROWS)}
    same, other = (row[(0, 0)], row[(0, 1)]), (row[(2, 0)], row[(2, 1)])
    assert bits_equal(a[same[0]], a[same[1]]) and bits_equal(o[same[0]], o[same[1]])               # one sequence, one camera
    assert not bits_equal(j[same[0]], j[same[1]])                                                    # their keypoints are their own
    T = lens[other[0]]
    assert T >= 1 and not torch.equal(a[other[0], :T], a[other[1], :T]) and not torch.equal(o[other[0], :T], o[other[1], :T])
    assert bits_equal(a[other[0], T:], a[other[1], T:]) and bits_equal(o[other[0], T:], o[other[1], T:])


# -------------------------------------------------------------------------------------------------------- arguments
def _good():
    c = Hf.cases()[0]
    return c, c.K.copy(), c.Tcw.copy()


def bad_cameras():
    """[(name, K, T_cw)] every one of which camera_constants must refuse"""
    _, K, Tcw = _good()
    out = []
    Z = K.copy()
    Z[1] = 0.0
    out.append(("K with a zero row", Z, Tcw))
    out.append(("K with rows 0 and 1 equal", np.array([[1400, 3.5, 960], [1400, 3.5, 960], [0, 0, 1]], np.float32), Tcw))
    out.append(("K with rows 0 and 2 equal", np.array([[2, 3, 5], [0, 7, 1], [2, 3, 5]], np.float32), Tcw))
    out.append(("K^-1 overflows: fx = 1e-39", np.diag([1e-39, 1400.0, 1.0]).astype(np.float32), Tcw))
    out.append(("K^-1 overflows: K02 / K00 = 1e60", np.array([[1e-30, 0, 1e30], [0, 1, 0], [0, 0, 1]], np.float32), Tcw))
    for q in range(9):
        for v in (np.nan, np.inf, -np.inf):
            B = K.copy()
            B.flat[q] = v
            out.append((f"K[{q // 3}][{q % 3}] = {v}", B, Tcw))
    for r in range(3):
        for q in range(4):
            for v in (np.nan, np.inf):
                B = Tcw.copy()
                B[r, q] = v
                out.append((f"T_cw[{r}][{q}] = {v}", K, B))
    return out


def _single_call(c, K, Tcw, n=None, null=()):
    """rc_camera_inputs on NaN-prefilled outputs: (rc, outputs untouched, gravity [3])"""
    from robustcap_amd import _lib
    T = c.kp.shape[0] if n is None else n
    pix = c.kp * np.array([c.size[0], c.size[1], 1], np.float32)
    ins = {"kp": dev(pix), "acc": dev(c.acc), "ori": dev(c.ori)}
    outs = {"j": torch.full((max(T, 1) * 99,), float("nan"), device="cuda"), "a": torch.full((max(T, 1) * 18,), float("nan"), device="cuda"),
            "o": torch.full((max(T, 1) * 54,), float("nan"), device="cuda")}
    g = np.full(3, np.nan, np.float32)
    K, Tcw = np.ascontiguousarray(K, np.float32), np.ascontiguousarray(Tcw, np.float32)
    a = {**{k: _lib.ptr(v) for k, v in {**ins, **outs}.items()}, "K": hp(K), "Tcw": hp(Tcw), "g": hp(g)}
    for k in null:
        a[k] = None
    rc = _lib.load().rc_camera_inputs(a["kp"], a["acc"], a["ori"], a["K"], a["Tcw"], a["j"], a["a"], a["o"], a["g"], T, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, all(bool(torch.isnan(t).all()) for t in outs.values()), g


def test_refused_cameras_leave_everything_untouched():
    c, K, Tcw = _good()
    c = c.frames(1)
    bad = bad_cameras()
    assert len(bad) == 5 + 27 + 24
    for k, (name, Kb, Tb) in enumerate(bad):
        rc, clean, g = _single_call(c, Kb, Tb)
        assert rc == RC_ERR_INVALID and clean and np.isnan(g).all(), name
        for pos in (range(3) if k < 5 else (k % 3,)):                           # whichever row is the bad one
            Ks, Ts = np.stack([K] * 3), np.stack([Tcw] * 3)
            Ks[pos], Ts[pos] = Kb, Tb
            call = RowsCall(np.stack([c.kp] * 3), c.acc[None], c.ori[None], [0, 0, 0], [1, 1, 1], Ks, Ts, c.size, 1)
            assert call.rc == RC_ERR_INVALID and call.untouched(), (name, pos)
    last = Tcw.copy()                                                            # the last row of T_cw is not read
    last[3] = np.nan
    rc, clean, g = _single_call(c, K, last)
    assert rc == RC_OK and not clean and bits_equal(g, single(c)["gravityc"])


def test_empty_calls_return_ok_and_write_nothing():
    c, K, Tcw = _good()
    rc, clean, g = _single_call(c, K, Tcw, n=0)
    assert rc == RC_OK and clean and bits_equal(g, single(c)["gravityc"])        # n = 0: no launch, the gravity vector all the same
    one = c.frames(1)
    for n_rows, Tmax in ((0, 1), (1, 0), (0, 0)):
        call = RowsCall(one.kp[None], one.acc[None], one.ori[None], [0], [min(1, Tmax)], K[None], Tcw[None], c.size, Tmax, n_rows=n_rows)
        assert call.rc == RC_OK and call.untouched(), (n_rows, Tmax)
    assert _single_call(c, K, Tcw, n=-1)[0] == RC_ERR_INVALID
    for n_rows, Tmax in ((-1, 1), (1, -1)):
        assert RowsCall(one.kp[None], one.acc[None], one.ori[None], [0], [1], K[None], Tcw[None], c.size, Tmax, n_rows=n_rows).rc == RC_ERR_INVALID


def test_null_buffers_are_refused():
    c, K, Tcw = _good()
    c = c.frames(1)
    for k in ("kp", "acc", "ori", "K", "Tcw", "j", "a", "o", "g"):
        rc, clean, g = _single_call(c, K, Tcw, null=(k,))
        assert rc == RC_ERR_INVALID and clean and np.isnan(g).all(), k
    for k in ("kp", "acc", "ori", "sor", "len", "K", "Tcw", "j", "a", "o", "g", "scratch"):
        call = RowsCall(c.kp[None], c.acc[None], c.ori[None], [0], [1], K[None], Tcw[None], c.size, 1, null=(k,))
        assert call.rc == RC_ERR_INVALID and call.untouched(), k


def test_zz_report_worst_ratios():
    """The largest error / Bound per op over the tests above (pytest -s shows it)."""
    lines = []
    for title, w in WORST.items():
        if w.w:
            lines += w.lines(f"device, {title}: worst error / Bound per op")
    if not lines:
        print("no test of this file ran before the report")
        return
    for ln in lines:
        print(ln)
    path = os.environ.get("RC_HARNESS_RATIOS_OUT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")
    assert max(v for w in WORST.values() for v, _ in w.w.values()) <= 1.0
