"""What building a sub-net's training corpus costs: corpus.build (robustcap_amd/corpus.py, rc_subnet_corpus, csrc/rc_corpus.hip) beside the
reference's way -- the builder loops of net/sig_mp.py:444-486 (rnn4, AIST), :726-747 (rnn7, AMASS) and :797-821 (rnn8, AMASS) transcribed
in torch -- and what a mixed batch costs (ConcatSubnetDataset.batch, rc_subnet_batch_parts) beside the two single-kind ds.batch calls.

    python tools/subnet_corpus_bench.py [--small] [--out profiles/subnet_corpus_bench.txt]

Corpus, per case (rnn4 AIST at 64 sequences x 9 views x 600 frames with an occlusion sample for every view; rnn7 and rnn8 AMASS at 256
sequences x 1200 frames; fields of seeded random numbers: only the shapes matter here): (i) corpus.build through Python from the host
dictionary -- concatenation, upload, the call -- and (ii) the C entry alone on the uploaded fields, HIP events, with its counted bytes
(fields read once per row that uses them, both outputs written) against the 6.3 TB/s the other training rows use; (a) the transcription
on the host with 16 threads plus torch.cat(...).to(device), wall clock ending in a synchronise; (b) the same transcription on device
tensors (the dictionary uploaded beforehand), HIP events. Medians of REPS after a warm-up; peak device memory of (i) and (b) from
torch.cuda.max_memory_allocated over the run. Mixed batches: 256 samples x 200 frames of rnn4, half plain and half world, in one
ConcatSubnetDataset.batch against a plain and a world ds.batch of 128 each. No thresholds."""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--small", action="store_true", help="a tenth of the sizes (a quick look)")
ap.add_argument("--out", help="also append the lines to this file")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import subnet_batches_ref as BR  # noqa: E402
from robustcap_amd import config as cfg  # noqa: E402
from robustcap_amd import corpus, synth  # noqa: E402
from robustcap_amd.net.sig_mp import Net  # noqa: E402

REPS, HOST_REPS, HBM_BYTES_PER_S = 5, 3, 6.3e12
PARENT = cfg.smpl_parent


def say(line):
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def timed(fn, reps=REPS):
    out = []
    fn()
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def walled(fn, reps=HOST_REPS):
    out = []
    fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out)


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


# ---- the reference's builder loops in torch (any device) ------------------------------------------------------------------------------------
def aa2R(a):
    """art.math.axis_angle_to_rotation_matrix (articulate/math/angular.py:221-233)."""
    a = a.reshape(-1, 3)
    angle = a.norm(dim=1, keepdim=True)
    axis = a / angle
    axis[torch.isnan(axis) | torch.isinf(axis)] = 0
    c, s = angle.cos().view(-1, 1, 1), angle.sin().view(-1, 1, 1)
    z = torch.zeros_like(axis[:, 0])
    K = torch.stack([z, -axis[:, 2], axis[:, 1], axis[:, 2], z, -axis[:, 0], -axis[:, 1], axis[:, 0], z], dim=1).view(-1, 3, 3)
    eye = torch.eye(3, device=a.device).expand(a.shape[0], 3, 3)
    return c * eye + (1 - c) * torch.bmm(axis.view(-1, 3, 1), axis.view(-1, 1, 3)) + s * K


def fk_R(R):
    G = [R[:, 0]]
    for i in range(1, 24):
        G.append(torch.bmm(G[PARENT[i]], R[:, i]))
    return torch.stack(G, dim=1)


def bbox_scale(uv):
    u_max, u_min = uv[..., 0].max(dim=-1).values, uv[..., 0].min(dim=-1).values
    v_max, v_min = uv[..., 1].max(dim=-1).values, uv[..., 1].min(dim=-1).values
    return torch.max(u_max - u_min, v_max - v_min)


def append(x, v):
    return torch.cat((x, torch.full_like(x[..., :1], v)), dim=-1)


def rnn4_aist(d):
    data, label = [], []
    for i in range(len(d["pose"])):
        for j in range(len(d["cam_K"][i])):
            if d["joint2d_mp"][i][j] is None:
                continue
            Tcw = d["cam_T"][i][j]
            Kinv = d["cam_K"][i][j].inverse()
            oric = Tcw[:3, :3].matmul(d["imu_ori"][i])
            accc = Tcw.matmul(append(d["imu_acc"][i], 0.0).unsqueeze(-1)).squeeze(-1)[..., :3]
            j3dc = Tcw.matmul(append(d["joint3d"][i], 1.0).unsqueeze(-1)).squeeze(-1)[..., :3]
            j3dc = j3dc[:, 1:] - j3dc[:, :1]
            for k, key in enumerate(("joint2d_mp", "joint2d_occ")):
                kp = d[key][i][j]
                if kp is None or len(kp) != len(oric):
                    continue
                j2dc = torch.zeros(len(oric), 33, 3, device=kp.device)
                j2dc[..., :2] = kp[..., :2]
                j2dc[..., 0] = j2dc[..., 0] * 1920
                j2dc[..., 1] = j2dc[..., 1] * 1080
                j2dc = Kinv.matmul(append(j2dc[..., :2], 1.0).unsqueeze(-1)).squeeze(-1)
                if k == 0:
                    j2dc[..., :2] = j2dc[..., :2] / (bbox_scale(j2dc)).view(-1, 1, 1)
                j2dc[:, 24:, :2] = j2dc[:, 24:, :2] - j2dc[:, 23:24, :2]
                j2dc[:, :23, :2] = j2dc[:, :23, :2] - j2dc[:, 23:24, :2]
                j2dc[..., -1] = kp[..., -1]
                data.append(torch.cat((accc.flatten(1), oric.flatten(1), j2dc.flatten(1)), dim=1)[1:-1])
                label.append(j3dc.flatten(1)[1:-1])
    return data, label


def root_amass(d, name):
    data, label = [], []
    for i in range(len(d["imu_acc"])):
        p = aa2R(d["pose"][i]).view(-1, 24, 3, 3)
        j3dr = (d["joint3d"][i][:, 1:] - d["joint3d"][i][:, :1]).bmm(p[:, 0])
        accw, oriw = d["imu_acc"][i], d["imu_ori"][i]
        Rrw = p[:, 0].transpose(1, 2)
        accr = Rrw.unsqueeze(1).matmul(accw.unsqueeze(-1))
        if name == "rnn7":
            orir = oriw.clone()
            orir[:, :5] = Rrw.unsqueeze(1).matmul(oriw[:, :5])
            p[:, 0] = torch.eye(3, device=p.device)
            y = fk_R(p)[:, :, :, :2].transpose(2, 3).reshape(-1, 144)
        else:
            orir = Rrw.unsqueeze(1).matmul(oriw)
            v3dw = (d["joint3d"][i][2:] - d["joint3d"][i][:-2]) * 30
            y = torch.zeros(v3dw.shape[0], 2, device=v3dw.device)
            y[v3dw[:, 10:12].norm(dim=2) < 0.25] = 1
            y = torch.cat((y[:1], y, y[-1:]), dim=0)
        data.append(torch.cat((accr.flatten(1), orir.flatten(1), j3dr.flatten(1)), dim=1)[1:-1])
        label.append(y.flatten(1)[1:-1])
    return data, label


# ---- seeded dictionaries of the reference's shapes ------------------------------------------------------------------------------------------
def random_dict(seed, n_seq, T, n_cam):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    d = {"pose": [0.3 * r(T, 24, 3) for _ in range(n_seq)], "tran": [r(T, 3) for _ in range(n_seq)],
         "imu_acc": [r(T, 6, 3) for _ in range(n_seq)], "imu_ori": [r(T, 6, 3, 3) for _ in range(n_seq)],
         "joint3d": [0.5 * r(T, 24, 3) + torch.tensor([0.0, 0.0, 5.0]) for _ in range(n_seq)], "sync_3d_mp": [r(T, 33, 3) for _ in range(n_seq)]}
    if n_cam:
        K = torch.tensor([[1500.0, 0.0, 960.0], [0.0, 1500.0, 540.0], [0.0, 0.0, 1.0]])
        d["pose"] = [p.reshape(T, 72) for p in d["pose"]]
        d["cam_K"] = [K.expand(n_cam, 3, 3).clone() for _ in range(n_seq)]
        d["cam_T"] = [torch.eye(4).expand(n_cam, 4, 4).clone() for _ in range(n_seq)]
        d["joint2d_mp"] = [[torch.rand(T, 33, 3, generator=g) for _ in range(n_cam)] for _ in range(n_seq)]
        d["joint2d_occ"] = [[torch.rand(T, 33, 3, generator=g) for _ in range(n_cam)] for _ in range(n_seq)]
    return d


def to_device(d, dev):
    mv = lambda v: None if v is None else v.to(dev)
    return {k: [([mv(e) for e in v] if isinstance(v, list) else mv(v)) for v in vs] for k, vs in d.items()}


def corpus_case(net, name, source, d, transcription):
    dev = net.device
    tr = net.trainable(name)
    t_build = timed(lambda: corpus.build(tr, source, d))
    m_build = peak_of(lambda: corpus.build(tr, source, d))
    p = corpus.prepare(tr, source, d)
    x = torch.empty(p.rows, p.widths[0], device=dev)
    y = torch.empty(p.rows, p.widths[1], device=dev)
    t_entry = timed(lambda: p.call(x, y))
    reads = {"rnn4": 18 + 54 + 72 + 99, "rnn7": 72 + 18 + 54 + 72, "rnn8": 72 + 18 + 54 + 72}[name]
    nbytes = 4 * p.rows * (reads + p.widths[0] + p.widths[1])
    torch.set_num_threads(16)
    t_host = walled(lambda: [torch.cat(t).to(dev) for t in transcription(d)])
    dd = to_device(d, dev)
    t_dev = timed(lambda: [torch.cat(t) for t in transcription(dd)])
    m_dev = peak_of(lambda: [torch.cat(t) for t in transcription(dd)])
    a, b = transcription(dd)
    err = max(float((torch.cat(a) - x).abs().max()), float((torch.cat(b) - y).abs().max()))
    say(f"corpus {name} {source}: {p.rows} rows [{p.widths[0]} | {p.widths[1]}]  corpus.build {t_build:9.2f} (peak {m_build / 1e6:8.1f} MB)  |  "
        f"rc_subnet_corpus alone {t_entry:8.3f}: counted {nbytes / 1e6:8.1f} MB = {100 * nbytes / (t_entry * 1e-3) / HBM_BYTES_PER_S:5.1f} % of 6.3 TB/s  |  "
        f"(a) torch on the host, 16 threads, + upload {t_host:10.2f} = {t_host / t_build:6.1f} x corpus.build  |  (b) torch on device tensors "
        f"{t_dev:9.2f} (peak {m_dev / 1e6:8.1f} MB) = {t_dev / t_entry:7.1f} x the entry  |  max |(b) - entry| {err:.2e}")


def mixed_case(net, N, T):
    name, half = "rnn4", N // 2
    tr = net.trainable(name)
    W, Wl = BR.WIDTHS[name]
    g = np.random.default_rng(0)
    pd, pl = g.normal(size=(half * T, W)).astype(np.float32), g.normal(size=(half * T, Wl)).astype(np.float32)
    wd, wl = BR.world_corpus(1, (T,) * half)
    pool = torch.from_numpy(BR.conf_pool(7, 1000))
    seqs = lambda a: list(torch.from_numpy(a).split(T))
    plain = tr.dataset(seqs(pd), seqs(pl), split_size=T)
    world = tr.dataset(seqs(wd), seqs(wl), split_size=T, kind="world", conf_pool=pool)
    cat = tr.concat([plain, world])
    idx = torch.randperm(N, generator=torch.Generator().manual_seed(2)).tolist()
    ip, iw = [i for i in idx if i < half], [i - half for i in idx if i >= half]
    t_cat = timed(lambda: cat.batch(idx))
    t_two = timed(lambda: (plain.batch(ip), world.batch(iw)))
    say(f"mixed {name}: {N} samples x {T} frames, half plain and half world: ConcatSubnetDataset.batch {t_cat:8.3f}  |  a plain and a world ds.batch of "
        f"{half} each {t_two:8.3f} ({t_two / t_cat:5.2f} x; their outputs would still have to be interleaved)")


def main():
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    net = Net(body=synth.make_body(1), batch=1)
    net.load_state_dict(synth.make_state_dict(0))
    k = 10 if args.small else 1
    say(f"# subnet_corpus_bench: HIP events, median of {REPS} after a warm-up (host: wall clock, median of {HOST_REPS}); ms")
    for run in (1, 2):
        say(f"# run {run}")
        corpus_case(net, "rnn4", "aist", random_dict(run, 64 // k or 1, 600, 9), rnn4_aist)
        amass = random_dict(10 + run, 256 // k, 1200, 0)
        corpus_case(net, "rnn7", "amass", amass, lambda d: root_amass(d, "rnn7"))
        corpus_case(net, "rnn8", "amass", amass, lambda d: root_amass(d, "rnn8"))
        mixed_case(net, 256, 200)


if __name__ == "__main__":
    main()
