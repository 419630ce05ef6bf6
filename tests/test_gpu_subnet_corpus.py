"""The corpus builders on the device (corpus.build: rc_subnet_corpus, csrc/rc_corpus.hip) against the numpy restatement
tests/subnet_corpus_ref.py of the eleven dataset recipes of net/sig_mp.py:301-839, on synth.make_training_dicts with sequences of
(3, 4, 13, 66) frames and 3 views: one output row; a two-row stencil; a sequence whose rows cross a 64-row and a workgroup edge, with
neighbours on both sides. Accuracy within K = 8 times the float32 restatement's own error of the float64 one (+ 1e-7 of the quantity's
scale), per block of columns; rnn8's labels and the confidence column exact; a sequence's rows bitwise those of a call with that
sequence alone; nothing written outside the R rows; every refusal before anything is enqueued.

Observed on MI355X (profiles/subnet_corpus_ratios.txt): the RATIO lines each accuracy test prints before it asserts."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import subnet_corpus_ref as R
import test_gpu_subnet_batches as B
from subnet_batches_ref import bound_ratio
from robustcap_amd import batches, corpus, synth

pytestmark = pytest.mark.gpu

_same = B._same
LENGTHS, N_CAM, SEED = (3, 4, 13, 66), 3, 6
INVALID = -1


@functools.lru_cache(maxsize=None)
def _dicts():
    aist, amass = synth.make_training_dicts(SEED, LENGTHS, synth.make_body(1), N_CAM)
    return {"aist": aist, "amass": amass}


@functools.lru_cache(maxsize=None)
def _ref(name, source, dtype):
    return R.build(name, source, _dicts()[source], dtype)


@functools.lru_cache(maxsize=None)
def _built(name, source):
    x, y, lengths = corpus.build(B._tr(name), source, _dicts()[source])
    return x, y, lengths


def _only(d, i):
    """The dictionary of sequence i alone."""
    return {k: [v[i]] for k, v in d.items()}


def test_the_inputs_meet_the_label_condition():
    """No foot speed within 1e-3 of the contact threshold and both classes for both feet: rnn8's labels can be compared for equality."""
    speed = np.concatenate([R.foot_speed(j) for j in _dicts()["amass"]["joint3d"]])
    assert np.abs(speed - 0.25).min() > 1e-3
    assert (speed < 0.25).any(0).all() and (speed >= 0.25).any(0).all()


@pytest.mark.parametrize("name,source", R.RECIPES)
def test_recipe_within_the_bound(name, source):
    x, y, lengths = _built(name, source)
    x64, y64 = _ref(name, source, np.float64)
    x32, y32 = _ref(name, source, np.float32)
    assert lengths == [len(a) for a in x64] and tuple(x.shape) == (sum(lengths), x64[0].shape[1]) and tuple(y.shape) == (sum(lengths), y64[0].shape[1])
    x, y = x.cpu().numpy(), y.cpu().numpy()
    x64, x32, y64, y32 = np.concatenate(x64), np.concatenate(x32), np.concatenate(y64), np.concatenate(y32)
    blocks = [(g, x[:, a:b], x64[:, a:b], x32[:, a:b]) for g, a, b in R.column_groups(x.shape[1])] + [("label", y, y64, y32)]
    worst = 0.0
    for what, got, f64, f32 in blocks:
        if name == "rnn8" and what == "label":
            assert np.array_equal(got, f64)
            continue
        r = bound_ratio(got, f64, f32)
        print(f"RATIO {name} {source} {what}: {r:.4f} of the bound (max |f64| {np.abs(f64).max():.3e}, float32 restatement's error "
              f"{np.abs(f32.astype(np.float64) - f64).max():.3e})")
        worst = max(worst, r)
    assert worst <= 1.0
    if source == "aist" and name in ("rnn4", "rnn6"):                      # the un-noised confidence column: a copy
        assert np.array_equal(x[:, 74:171:3].view(np.int32), x32[:, 74:171:3].view(np.int32))
    if source == "amass" and name in ("rnn4", "rnn6"):                     # world corpus: the IMU columns are copies
        assert np.array_equal(x[:, :72].view(np.int32), x32[:, :72].view(np.int32))


@pytest.mark.parametrize("name,source", R.RECIPES)
def test_rows_do_not_depend_on_the_neighbours(name, source):
    """Two calls give the same bits; the rows of a sequence are bitwise those of a call with that sequence alone (a stencil or a
    table search that crossed a sequence's end would read the neighbour)."""
    x, y, lengths = _built(name, source)
    x2, y2, _ = corpus.build(B._tr(name), source, _dicts()[source])
    assert _same(x, x2) and _same(y, y2)
    d = _dicts()[source]
    at = 0
    for i in range(len(LENGTHS)):
        xa, ya, la = corpus.build(B._tr(name), source, _only(d, i))
        n = sum(la)
        assert n == (LENGTHS[i] - 2) * len(la) and _same(xa, x[at:at + n]) and _same(ya, y[at:at + n]), (name, source, i)
        at += n
    assert at == x.shape[0]


@pytest.mark.parametrize("name,source", [("rnn3", "aist"), ("rnn4", "aist"), ("rnn6", "amass"), ("rnn7", "amass")])
def test_nothing_outside_the_rows_is_written(name, source):
    """Over-allocated outputs filled with a sentinel, at an odd row offset (rows of 141 and 171 floats start off the 16-byte grid):
    untouched outside the R rows; the inputs unchanged."""
    p = corpus.prepare(B._tr(name), source, _dicts()[source])
    dev = p.net.device
    W, Wl, Rr, pad = p.widths[0], p.widths[1], p.rows, 3
    bx = torch.full(((Rr + 2 * pad) * W,), 7.25, device=dev)
    by = torch.full(((Rr + 2 * pad) * Wl,), 7.25, device=dev)
    x, y = bx[pad * W:(pad + Rr) * W].view(Rr, W), by[pad * Wl:(pad + Rr) * Wl].view(Rr, Wl)
    before = {k: v.clone() for k, v in p.fields.items() if v is not None}
    kp_before = None if p.kp is None else p.kp.clone()
    assert p.call(x, y) == 0
    ref_x, ref_y, _ = _built(name, source)
    assert _same(x, ref_x) and _same(y, ref_y)
    for buf, w in ((bx, W), (by, Wl)):
        assert bool((buf[:pad * w] == 7.25).all()) and bool((buf[(pad + Rr) * w:] == 7.25).all())
    assert all(_same(v, p.fields[k]) for k, v in before.items()) and (kp_before is None or _same(kp_before, p.kp))


def test_refusals_leave_the_outputs_untouched():
    net = B._tr("rnn3")._net                                                # the trainers' Net: its context holds the messages
    lib, ctx = net._lib, net._ctx
    d = _dicts()

    def attempt(name, src, what, expect=INVALID, **edit):
        p = corpus.prepare(B._tr(name), src, d[src])
        x = torch.full((p.rows, p.widths[0]), 7.25, device=net.device)
        y = torch.full((p.rows, p.widths[1]), 7.25, device=net.device)
        keep = []
        for k, v in edit.items():
            if isinstance(v, torch.Tensor):
                keep.append(v)
                v = C.c_void_p(v.data_ptr())
            p.args[k] = v
        rc = p.call(x, y)
        assert rc == expect, (what, rc)
        if ctx is not None and p.args["ctx"] is not None and expect != 0:
            assert b"rc_subnet_corpus" in lib.rc_last_error(ctx), what
        torch.cuda.synchronize()
        assert bool((x == 7.25).all()) and bool((y == 7.25).all()), what

    attempt("rnn3", "aist", "null context", ctx=None)
    attempt("rnn3", "aist", "null net", net=None)
    attempt("rnn3", "aist", "unknown net", net=b"rnn5")
    attempt("rnn3", "aist", "unknown source", source=2)
    attempt("rnn3", "amass", "rnn8 from AIST", net=b"rnn8", source=0)
    for k in ("pose", "imu_acc", "imu_ori", "joint3d", "seq_frames"):
        attempt("rnn3", "aist", "null " + k, **{k: None})
    attempt("rnn6", "aist", "null tran", tran=None)
    for k in ("kp", "cam_K", "cam_T", "sample_seq"):
        attempt("rnn4", "aist", "null " + k, **{k: None})
    attempt("rnn4", "amass", "null sync_3d_mp", sync_3d_mp=None)
    n = len(LENGTHS)
    attempt("rnn8", "amass", "a sequence of 2 frames", seq_frames=(C.c_int32 * n)(2, 5, 13, 66))
    attempt("rnn8", "amass", "a table that does not sum to the frames", seq_frames=(C.c_int32 * n)(3, 4, 13, 65))
    attempt("rnn8", "amass", "a table that does not sum to the frames", frames=sum(LENGTHS) + 1)
    attempt("rnn4", "aist", "a sample table that does not sum to the keypoint frames", kp_frames=1)
    attempt("rnn4", "aist", "a sample of a sequence that is not there", sample_seq=(C.c_int32 * 64)(*([n] * 64)))
    attempt("rnn8", "amass", "2^31 rows", n_seq=3, seq_frames=(C.c_int32 * 3)(1 << 30, 1 << 30, 1 << 30), frames=3 << 30)
    p = corpus.prepare(B._tr("rnn4"), "aist", d["aist"])
    for what, K in (("singular", torch.zeros(3, 3)), ("non-finite", torch.tensor([[float("nan"), 0, 0], [0, 1, 0], [0, 0, 1.]]))):
        Ks = p.K.clone()
        Ks[1] = K.reshape(9)
        attempt("rnn4", "aist", what + " camera", cam_K=Ks)
    Ts = p.T.clone()
    Ts[0, 3] = float("inf")
    attempt("rnn6", "aist", "non-finite T_cw", cam_T=Ts)
    with pytest.raises(ValueError, match="rnn8"):
        corpus.build(B._tr("rnn8"), "aist", d["aist"])
    bad = dict(d["amass"])
    bad["joint3d"] = [np.zeros((T, 33, 3), np.float32) for T in LENGTHS]
    with pytest.raises(ValueError, match="joint3d.*33"):
        corpus.build(B._tr("rnn2"), "amass", bad)
    short_seq = {k: [v[0][:2]] for k, v in d["amass"].items() if k != "shape"}
    with pytest.raises(ValueError, match="2 frames"):
        corpus.build(B._tr("rnn2"), "amass", short_seq)


def test_sample_selection():
    """Views from len(cam_K[i]); a None view skipped; the occlusion sample skipped where it is None, a frame short, or the dictionary
    has no joint2d_occ; rnn6 has no occlusion samples."""
    d = _dicts()["aist"]
    expect4, expect6 = [], []
    for i, T in enumerate(LENGTHS):
        for j in range(N_CAM):
            if d["joint2d_mp"][i][j] is None:
                continue
            expect4.append(T - 2), expect6.append(T - 2)
            if d["joint2d_occ"][i][j] is not None and len(d["joint2d_occ"][i][j]) == T:
                expect4.append(T - 2)
    assert _built("rnn4", "aist")[2] == expect4 and _built("rnn6", "aist")[2] == expect6 and len(expect4) > len(expect6) == 2 * len(LENGTHS)
    without = {k: v for k, v in d.items() if k != "joint2d_occ"}
    assert corpus.build(B._tr("rnn4"), "aist", without)[2] == expect6
    fewer = dict(d)
    fewer["cam_K"] = [K[:2] for K in d["cam_K"]]
    assert len(corpus.build(B._tr("rnn6"), "aist", fewer)[2]) < len(expect6)


def test_from_buffers_adopts_the_corpus():
    tr = B._tr("rnn3")
    x, y, lengths = corpus.build(tr, "amass", _dicts()["amass"])
    ds = batches.SubnetDataset.from_buffers(tr, x, y, lengths, split_size=5)
    assert ds.data.data_ptr() == x.data_ptr() and ds.label.data_ptr() == y.data_ptr() and ds.data is x
    ref = tr.dataset(list(torch.split(x, lengths)), list(torch.split(y, lengths)), split_size=5)
    assert ds.samples == ref.samples and ref.data.data_ptr() != x.data_ptr()
    a, b = ds.manual_seed(5).batch([3, 0, 7]), ref.manual_seed(5).batch([3, 0, 7])
    assert all(_same(p, q) for p, q in zip(a[0] + a[1], b[0] + b[1]))
    with pytest.raises(ValueError, match="lengths"):
        batches.SubnetDataset.from_buffers(tr, x, y, lengths[:-1])
    with pytest.raises(ValueError, match="expected"):
        batches.SubnetDataset.from_buffers(tr, y, x, lengths)
    w = corpus.dataset(B._tr("rnn4"), "amass", _dicts()["amass"], 8, torch.rand(70, 33))
    assert w.kind == "world" and tuple(w.data.shape) == (sum(LENGTHS) - 2 * len(LENGTHS), 171)
