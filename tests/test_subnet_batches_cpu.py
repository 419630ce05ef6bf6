"""The batches of robustcap_amd/batches.py without a GPU: the draws of tests/subnet_batches_ref.py (uniforms, normals, the pool-row
permutation) as distributions, its camera against the reference's own euler_angle_to_rotation_matrix and get_bbox_scale
(tests/golden/augment/augment_ops.npz, tools/capture_augment_ops.py), its sample arithmetic against a second, independent torch transcription
of the two AMASS ``__getitem__`` s (net/sig_mp.py:520-552, :649-679) handed the same draws, and six deliberate mistakes that each have
to leave the GPU test's tolerance by two orders of magnitude."""
import math
import os

import numpy as np
import pytest
import torch

import subnet_batches_ref as R
from robustcap_amd import config as cfg

SEED = (0x9E3779B9 << 32) | 0x1234ABCD               # both halves of the key in use
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment", "augment_ops.npz")


# ---- the second transcription: torch, line by line, the draws handed in ---------------------------------------------------------------
def torch_get_bbox_scale(uv):
    u_max, u_min = uv[..., 0].max(dim=-1).values, uv[..., 0].min(dim=-1).values
    v_max, v_min = uv[..., 1].max(dim=-1).values, uv[..., 1].min(dim=-1).values
    return torch.max(u_max - u_min, v_max - v_min)


def torch_getitem(name, data, label, conf, Rc0c, u_tran, rows, z_kp, z_tail, dtype=torch.float64):
    """AMASSDataset.__getitem__ of train_rnn4 / train_rnn6 with every random call replaced by its draw: ``Rc0c`` [3, 3] for
    generate_random_rotation_matrix_constrained, ``u_tran`` [3] for torch.rand(3), ``rows`` for random.sample, ``z_kp`` [T, 33, 2] and
    ``z_tail`` [T, 69] standard normals for the two torch.normal calls. conf: [P, 33, 1], as syn_c.pt."""
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    data, label, conf = t(data), t(label), t(conf)
    accw = data[:, :18].reshape(-1, 6, 3, 1)
    oriw = data[:, 18:18 + 6 * 3 * 3].reshape(-1, 6, 3, 3)
    j3dw_mp = data[:, -33 * 3:].reshape(-1, 33, 3, 1)
    j3dw = label.reshape(-1, 24, 3, 1)
    Rwc0 = torch.tensor([[-1, 0, 0], [0, -1, 0], [0, 0, 1.]], dtype=dtype)
    Rcw = Rwc0.mm(t(Rc0c)).t()
    accc = Rcw.matmul(accw)
    oric = Rcw.matmul(oriw)
    j3dc = Rcw.matmul(j3dw).squeeze(-1)
    j3dc_mp = Rcw.matmul(j3dw_mp).squeeze(-1)
    u = t(u_tran)
    random_tranc = torch.tensor([-1, -1, 3.], dtype=dtype) * (1 - u) + torch.tensor([1, 1, 8.], dtype=dtype) * u
    random_tranc[2] -= j3dc[..., -1].min()
    j3dc = j3dc + random_tranc
    j3dc_mp = j3dc_mp + random_tranc
    j2dc = j3dc_mp / j3dc_mp[..., -1:]
    p = conf[torch.as_tensor(np.asarray(rows))]
    j2dc[..., :2] = j2dc[..., :2] + 0.003 * (1 - p) * t(z_kp)                      # torch.normal(mean, std) = mean + std z
    j2dc[..., -1:] = p
    if name == "rnn4":
        j2dc[..., :2] = j2dc[..., :2] / (torch_get_bbox_scale(j2dc)).view(-1, 1, 1)
        j2dc[:, 24:, :2] = j2dc[:, 24:, :2] - j2dc[:, 23:24, :2]
        j2dc[:, :23, :2] = j2dc[:, :23, :2] - j2dc[:, 23:24, :2]
        j3dc = j3dc[:, 1:] - j3dc[:, :1]
        return torch.cat((accc.flatten(1), oric.flatten(1), j2dc.flatten(1)), dim=1), j3dc.flatten(1)
    lab = j3dc[:, 0]
    j3dc = j3dc[:, 1:] - j3dc[:, :1]
    x = torch.cat((accc.flatten(1), oric.flatten(1), j2dc.flatten(1), j3dc.flatten(1)), dim=1)
    x = x.clone()
    x[:, -69:] = x[:, -69:] + 0.03 * t(z_tail)
    return x, lab


def torch_sample(name, data, label, pool, sample, seed, call, dtype=torch.float64):
    """``torch_getitem`` on the draws of sample ``sample`` of a batch (the reference's way to build it, for tools/subnet_batches_bench.py too)."""
    d = R.world_draws(name, data.shape[0], pool.shape[0], sample, seed, call)
    Rc0c = np.diag([-1.0, -1.0, 1.0]) @ d["Rcw"].astype(np.float64).T                  # Rcw = (D Rc0c)^T  <=>  Rc0c = D Rcw^T
    return torch_getitem(name, data, label, pool[..., None], Rc0c, d["ut"], d["rows"], d["kp"](np.float64), d["tail"](np.float64), dtype)


# ---- uniforms and normals ----------------------------------------------------------------------------------------------------------
def test_uniforms_are_inside_their_intervals_and_exact_in_float32():
    w = np.concatenate([np.array([0, 1, 255, 256, 511, 512, 2 ** 32 - 1, 2 ** 32 - 256, 2 ** 31], np.uint32),
                        R.words(0, np.arange(4096), R.SITE_NOISE, 0, SEED, 5)[0]])
    for u, lo_open in ((R.u_closed0(w), False), (R.u_open(w), True)):
        assert (u.astype(np.float32).astype(np.float64) == u).all()
        assert (u < 1.0).all() and ((u > 0.0).all() if lo_open else (u >= 0.0).all())
    assert R.u_closed0(np.uint32(0)) == 0.0 and R.u_open(np.uint32(0)) == 2.0 ** -24 and R.u_open(np.uint32(2 ** 32 - 1)) == 1 - 2.0 ** -24
    assert np.isfinite(R.box_muller(np.uint32(0), np.uint32(0), np.float32)[0])


def test_normals_are_standard_and_the_four_of_a_call_uncorrelated():
    n_calls = 1 << 18
    z = R.normals(3, np.arange(n_calls // 16), R.SITE_NOISE, 64, SEED, 9).reshape(n_calls, 4)      # 2^20 values
    n = z.size
    assert n == 1 << 20
    assert abs(z.mean()) <= 5 / math.sqrt(n)
    assert abs(z.var() - 1.0) <= 5 * math.sqrt(2.0 / n)
    tail = math.erfc(2 / math.sqrt(2))
    assert abs((np.abs(z) > 2).mean() - tail) <= 5 * math.sqrt(tail * (1 - tail) / n)
    for a in range(4):
        for b in range(a + 1, 4):
            assert abs((z[:, a] * z[:, b]).mean()) <= 5 / math.sqrt(n_calls), (a, b)
    z32 = R.normals(3, np.arange(64), R.SITE_NOISE, 64, SEED, 9, np.float32)
    assert z32.dtype == np.float32 and np.abs(z32 - z[:1024].reshape(64, 64)).max() < 1e-5


def test_a_draw_depends_on_seed_call_site_sample_frame_and_unit_only():
    a = R.normals(7, np.arange(5), R.SITE_NOISE, 69, SEED, 2)
    assert np.array_equal(a[3:4], R.normals(7, np.array([3]), R.SITE_NOISE, 69, SEED, 2))                 # other frames do not matter
    assert np.array_equal(a[:, :8], R.normals(7, np.arange(5), R.SITE_NOISE, 8, SEED, 2))                 # nor does the width
    for other in (R.normals(8, np.arange(5), R.SITE_NOISE, 69, SEED, 2), R.normals(7, np.arange(5), R.SITE_NOISE, 69, SEED, 3),
                  R.normals(7, np.arange(5), R.SITE_KP, 69, SEED, 2), R.normals(7, np.arange(5), R.SITE_NOISE, 69, SEED ^ (1 << 40), 2)):
        assert not np.array_equal(a, other)


# ---- perm --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2, 3, 200, 201, 1000, 65537])
def test_perm_is_a_permutation(P):
    p = R.perm(4, np.arange(P), P, SEED, 1)
    assert np.array_equal(np.sort(p), np.arange(P))
    if P >= 200:
        assert not np.array_equal(p, R.perm(5, np.arange(P), P, SEED, 1))
        assert not np.array_equal(p, R.perm(4, np.arange(P), P, SEED, 2))
        assert np.array_equal(p[:50], R.perm(4, np.arange(50), P, SEED, 1))


def test_perm_selects_every_row_equally_often():
    S, T, P = 4000, 50, 200
    count = np.zeros(P)
    for s in range(S):
        count += np.bincount(R.perm(s, np.arange(T), P, SEED, 0), minlength=P)
    q = T / P
    dev = np.abs(count - S * q) / math.sqrt(S * q * (1 - q))
    print("perm: largest deviation of a row's selection count", dev.max(), "sigma")
    assert dev.max() <= 5


# ---- the camera --------------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    return np.abs(a.astype(np.float32).view(np.int32).astype(np.int64) - b.astype(np.float32).view(np.int32).astype(np.int64))


def test_camera_matches_the_reference_functions():
    import hashlib
    import json
    with open(GOLDEN, "rb") as f, open(os.path.join(os.path.dirname(GOLDEN), "meta.json")) as m:      # the fixture is the captured one
        assert hashlib.sha256(f.read()).hexdigest() == json.load(m)["sha256"]["augment_ops.npz"]
    g = np.load(GOLDEN)
    assert g["angles"].shape == (64, 3)
    deg = np.degrees(g["angles"])
    for name in ("rnn4", "rnn6"):                                        # both ends of every range are among the triples
        for k, axis in enumerate(("yaw", "pitch", "roll")):
            for end in cfg.CAMERA[name][axis]:
                assert np.isclose(deg[:, k], end).any(), (name, axis, end)
    for a, want in zip(g["angles"], g["euler_yxz"]):
        got = R.euler_yxz(*a).astype(np.float32)
        # 1 ulp of float32 -- except where the exact entry is 0 (yaw at +-90 / +-180 degrees): there both sides hold a float64 rounding
        # residue below 3e-16 (scipy's through quaternions, ours through the product), whose own ulp means nothing; such an entry is
        # held to 1e-15 absolute, eight orders below an ulp of the matrix's unit entries
        near_zero = np.abs(want) < 1e-15
        assert (_ulps(got, want)[~near_zero] <= 1).all() and np.abs(got - want)[near_zero].max(initial=0) < 1e-15, (a, got, want)
        Rcw = R.rcw_of(R.euler_yxz(*a)).astype(np.float64)
        assert abs(np.linalg.det(Rcw) - 1) < 1e-6 and np.abs(Rcw @ Rcw.T - np.eye(3)).max() < 1e-6
    kp = torch.from_numpy(g["kp"])
    assert np.array_equal(torch_get_bbox_scale(kp).numpy(), g["bbox_scale"])
    xy = g["kp"][..., :2].astype(np.float64)
    sc = np.maximum(xy[..., 0].max(1) - xy[..., 0].min(1), xy[..., 1].max(1) - xy[..., 1].min(1))
    assert np.array_equal(sc.astype(np.float32), g["bbox_scale"])


def test_camera_angles_stay_inside_their_ranges():
    for name in ("rnn4", "rnn6"):
        ang = np.degrees(np.array([R.camera_angles(name, s, SEED, 0) for s in range(256)]))
        for k, axis in enumerate(("yaw", "pitch", "roll")):
            lo, hi = cfg.CAMERA[name][axis]
            assert ang[:, k].min() >= lo and ang[:, k].max() < hi and ang[:, k].max() - ang[:, k].min() > 0.8 * (hi - lo)


def test_constants_agree_with_config():
    for name, a in cfg.AUGMENT.items():
        want = None if a is None else ((a[1], a[2]) if a[0] == "tail" else (dict((n, i) for n, i, _, _ in cfg.NETS)[name], a[1]))
        assert R.AUGMENT[name] == want
    for name, c in cfg.CAMERA.items():
        assert R.CAMERA[name] == (c["yaw"], c["pitch"], c["roll"])
    assert R.WIDTHS == {n: (i, o) for n, i, _, o in cfg.NETS}


# ---- the sample arithmetic ---------------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 37)
CORPUS = R.world_corpus(17, LENGTHS)
POOL = R.conf_pool(18, 64)


def _samples():
    at = 0
    for i, T in enumerate(LENGTHS):
        yield i, CORPUS[0][at:at + T], CORPUS[1][at:at + T]
        at += T


@pytest.mark.parametrize("name", ["rnn4", "rnn6"])
def test_restatement_agrees_with_the_torch_transcription(name):
    for i, d, l in _samples():
        ours = R.world_sample(name, d, l, POOL, i, SEED, 3)
        x, lab = torch_sample(name, d, l, POOL, i, SEED, 3)
        assert ours["x"].shape == (d.shape[0], R.WIDTHS[name][0]) and ours["label"].shape == (d.shape[0], R.WIDTHS[name][1])
        assert np.abs(ours["x"] - x.numpy()).max() <= 1e-12 and np.abs(ours["label"] - lab.numpy()).max() <= 1e-12
        assert np.array_equal(ours["conf"], POOL[R.perm(i, np.arange(d.shape[0]), 64, SEED, 3)].astype(np.float64))


def test_plain_sample_touches_the_noisy_columns_only():
    g = np.random.default_rng(5)
    for name, (W, _) in R.WIDTHS.items():
        d = g.normal(size=(6, W)).astype(np.float32)
        x = R.plain_sample(name, d, 2, SEED, 1)
        nz, c0 = R.plain_noise(name, 6, 2, SEED, 1)
        assert np.array_equal(x[:, :c0], d[:, :c0].astype(np.float64))
        if nz is None:
            assert c0 == W
        else:
            assert np.abs(nz).max() < 6 * R.AUGMENT[name][1] and (nz != 0).all() and np.allclose(x[:, c0:] - d[:, c0:], nz, atol=1e-15)


@pytest.mark.parametrize("mutation,name,keys", [
    ("minz_first_frame", "rnn4", ("xy",)), ("minz_first_frame", "rnn6", ("xy", "label")),
    ("minz_landmarks", "rnn4", ("xy",)), ("minz_landmarks", "rnn6", ("xy", "label")),
    ("row23_relative", "rnn4", ("xy",)),
    ("noise_by_p", "rnn4", ("xy",)), ("noise_by_p", "rnn6", ("xy",)),
    ("root_before_translation", "rnn6", ("label",)),
    ("rcw_not_transposed", "rnn4", ("accc", "oric", "xy", "label")), ("rcw_not_transposed", "rnn6", ("accc", "oric", "xy", "label", "tail")),
])
def test_mutations_leave_the_gpu_tolerance(mutation, name, keys):
    """The bound of the GPU test (8 x the float32 restatement's error + 1e-7 of the quantity's scale) against six deliberate mistakes:
    every quantity named has to move by at least 100 bounds on the last sample (37 frames)."""
    i, d, l = list(_samples())[-1]
    f64 = R.world_sample(name, d, l, POOL, i, SEED, 3)
    f32 = R.world_sample(name, d, l, POOL, i, SEED, 3, np.float32)
    bad = R.world_sample(name, d, l, POOL, i, SEED, 3, mutate=mutation)
    for k in keys:
        ratio = R.bound_ratio(bad[k], f64[k], f32[k])
        print(f"{mutation:24s} {name} {k:6s} moves by {ratio:12.1f} bounds")
        assert ratio >= 100, (mutation, name, k, ratio)
        assert f32[k].dtype == np.float32 and R.bound_ratio(f32[k], f64[k], f32[k]) <= 1 / 8 + 1e-9


# ---- the host table ----------------------------------------------------------------------------------------------------------------
def test_split_table_is_tensor_split():
    lengths = (401, 200, 1)
    want, at = [], 0
    for T in lengths:
        for piece in torch.arange(at, at + T).split(200):
            want.append((int(piece[0]), len(piece)))
        at += T
    assert R.split_table(lengths, 200) == want == [(0, 200), (200, 200), (400, 1), (401, 200), (601, 1)]
    assert R.split_table(lengths, -1) == [(0, 401), (401, 200), (601, 1)]
