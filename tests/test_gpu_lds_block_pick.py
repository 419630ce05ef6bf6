"""Block mode of the shared-weight gate GEMM (rc_gemm_lds.hip, RC_LDS_BLOCK_PICK): a one-tile problem whose active rows need as many
16-row blocks as there are storage blocks holding an active row takes those storage blocks whole, idle rows included.

Which rows a workgroup multiplies together must never show: every case runs with the switch off and on, and both must leave, bit
for bit, what the same rows leave in contexts of 16 rows (split products; those never reach the shared-weight kernel) -- pose and tran
of every frame a row ran, and (h, c) of all six sub-nets after the call. The row masks come from ``lengths`` (a row that has ended, or
never ran, is a bubble of every later tick) and from per-row keypoint confidences (an occlusion exit makes a row lag the batch; an
occluded row rides the rnn4 / rnn6 launches with its deferred input)."""
import numpy as np
import pytest
import torch

from robustcap_amd import synth

pytestmark = pytest.mark.gpu
t = torch.from_numpy
NETS = ("rnn2", "rnn3", "rnn4", "rnn6", "rnn7", "rnn8")
T = 14
REF_B = 16
HI, OCC = 0.95, 0.2


def _case_one_bubble_in_block_0():
    lens = [T] * 72
    lens[5] = 3                                     # rows 0 .. 15 keep 15 active rows from frame 3 on
    occ = {40: (4, 6)}                              # one occlusion exit: row 40 lags and leaves a second bubble for a while
    return 72, lens, occ


def _case_a_whole_storage_block_idle():
    lens = [T] * 96
    for b in range(32, 48):
        lens[b] = 0                                 # 80 rows in 5 of 6 storage blocks: the block list skips block 2
    return 96, lens, {}


def _case_only_the_half_filled_last_block_partly_active():
    lens = [T] * 72
    lens[65], lens[66], lens[70] = 2, 0, 5          # rows 64 .. 71 are all the last storage block holds; 72 .. 79 do not exist
    occ = {71: (0, T)}                              # ... and its last row never sees the camera
    return 72, lens, occ


def _case_bubbles_in_every_block():
    lens = [T] * 256
    for blk in range(16):
        lens[16 * blk + (5 * blk + 3) % 16] = (blk % 4) * 3        # 0, 3, 6 or 9 frames: 236 - 240 rows in 16 blocks
    occ = {16 * blk + (3 * blk + 9) % 16: (3 + blk % 3, 5 + blk % 3) for blk in range(0, 16, 3)}
    return 256, lens, occ


def _case_every_other_row_of_128():
    lens = [T if b % 2 == 0 else 0 for b in range(128)]           # 64 rows = 4 blocks' worth in 8 storage blocks: the row list stays
    return 128, lens, {}


def _case_all_rows_active():
    return 96, [T] * 96, {}                         # no bubble: the launches carry no flags, neither mode is asked


CASES = {
    "one_bubble_in_block_0": _case_one_bubble_in_block_0,
    "a_whole_storage_block_idle": _case_a_whole_storage_block_idle,
    "only_the_half_filled_last_block_partly_active": _case_only_the_half_filled_last_block_partly_active,
    "bubbles_in_every_block": _case_bubbles_in_every_block,
    "every_other_row_of_128": _case_every_other_row_of_128,
    "all_rows_active": _case_all_rows_active,
}


@pytest.fixture(scope="module")
def motion(synth_assets):
    """256 distinct rows x T frames, every keypoint confident; a case takes the first B rows and lowers what it occludes."""
    m = synth.make_motion(11, 256, T, synth_assets["body"], conf="high")
    m = {k: np.ascontiguousarray(m[k], dtype=np.float32) for k in ("j2dc", "accc", "oric", "gravityc", "first_tran")}
    m["j2dc"][..., 2] = HI
    return m


@pytest.fixture(scope="module")
def ref_net(synth_assets):
    from robustcap_amd.net.sig_mp import Net
    n = Net(body=synth_assets["body"], batch=REF_B)
    n.load_state_dict(synth_assets["state_dict"])
    n.set_gemm_mode(True)
    return n


def _inputs(motion, B, occ):
    m = {k: v[:B].copy() for k, v in motion.items()}
    for b, (a, e) in occ.items():
        m["j2dc"][b, a:e, :, 2] = OCC
    return m


def _run(net, m, rows, lens):
    """rows of ``m`` through one forward_sequence call of ``net`` (padded with rows of length 0 up to its batch)."""
    idx = list(rows) + [rows[0]] * (net.batch - len(rows))
    ln = [lens[b] for b in rows] + [0] * (net.batch - len(rows))
    net.gravityc = t(m["gravityc"][idx])
    pose, tran = net.forward_sequence(*(t(m[k][idx]).cuda() for k in ("j2dc", "accc", "oric")), first_tran=t(m["first_tran"][idx]), lengths=ln)
    torch.cuda.synchronize()
    states = {n: net.get_state(n) for n in NETS}
    k = len(rows)
    return pose[:k].cpu(), tran[:k].cpu(), {n: (h[:, :k].clone(), c[:, :k].clone()) for n, (h, c) in states.items()}


def _reference(ref_net, m, B, lens):
    pose, tran, st = [], [], {n: ([], []) for n in NETS}
    before = ref_net.launch_stats()[0]
    for lo in range(0, B, REF_B):
        ref_net.reset_states()
        p, tr, s = _run(ref_net, m, list(range(lo, min(B, lo + REF_B))), lens)
        pose.append(p); tran.append(tr)
        for n in NETS:
            st[n][0].append(s[n][0]); st[n][1].append(s[n][1])
    assert ref_net.launch_stats()[0] == before                           # 16 rows never take the shared-weight kernel
    return torch.cat(pose), torch.cat(tran), {n: (torch.cat(h, 1), torch.cat(c, 1)) for n, (h, c) in st.items()}


def _assert_same(what, got, want, lens):
    gp, gt, gs = got
    wp, wt, ws = want
    for b, L in enumerate(lens):                                         # (past a row's length the outputs are unspecified)
        assert torch.equal(gp[b, :L], wp[b, :L]), (what, "pose", b)
        assert torch.equal(gt[b, :L], wt[b, :L]), (what, "tran", b)
    for n in NETS:
        for k, name in enumerate(("h", "c")):
            same = (gs[n][k] == ws[n][k]).all(0).all(-1)
            assert bool(same.all()), (what, n, name, "rows", torch.nonzero(~same).flatten().tolist())


@pytest.mark.parametrize("case", list(CASES))
def test_block_pick_leaves_every_row_what_16_row_contexts_leave(case, motion, ref_net, synth_assets, monkeypatch):
    from robustcap_amd.net.sig_mp import Net
    B, lens, occ = CASES[case]()
    m = _inputs(motion, B, occ)
    want = _reference(ref_net, m, B, lens)
    got = {}
    for switch in ("0", "1"):
        monkeypatch.setenv("RC_LDS_BLOCK_PICK", switch)                  # read when the context is created
        net = Net(body=synth_assets["body"], batch=B)
        net.load_state_dict(synth_assets["state_dict"])
        net.set_gemm_mode(True)
        net.set_sequence_mode(True, 8, force=True)
        got[switch] = _run(net, m, list(range(B)), lens)
        lds, _ = net.launch_stats()
        assert lds > 0, (case, switch, "no launch of the shared-weight kernel: the case did not run it")
        wave, _, _ = net.sequence_stats()
        assert wave > 0, (case, switch, "the wavefront engine did not run")
        del net
        _assert_same(f"{case}, RC_LDS_BLOCK_PICK={switch} against 16-row contexts", got[switch], want, lens)
    _assert_same(f"{case}, switch on against off", got["1"], got["0"], lens)
