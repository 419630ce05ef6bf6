"""Constants of the sig_mp hot path.

Values are the data constants of the reference's ``config.py`` (L97-101) and the class attributes of
``net/sig_mp.py:Net`` (L27-45). Only what the per-frame path reads is kept; dataset paths, live-camera
settings and split lists are out of scope.
"""

# config.py:97 -- velocity scale of rnn3's output (m/s * 3 / 60 fps)
vel_scale = 3
# config.py:98
tran_offset = (0.0, 0.25, 5.0)
# config.py:99 -- SMPL vertex ids standing in for the 33 MediaPipe landmarks
mp_mask = (332, 2809, 2800, 455, 6260, 3634, 3621, 583, 4071, 45, 3557, 1873, 4123, 1652, 5177, 2235, 5670,
           2673, 6133, 2319, 5782, 2746, 6191, 3138, 6528, 1176, 4662, 3381, 6727, 3387, 6787, 3226, 6624)
# config.py:100 -- SMPL vertex ids the 6 IMUs sit on
vi_mask = (1961, 5424, 1176, 4662, 411, 3021)
# config.py:101 -- SMPL joint ids of the 6 IMUs (L-elbow, R-elbow, L-knee, R-knee, head, pelvis)
ji_mask = (18, 19, 4, 5, 15, 0)

# standard SMPL kinematic tree (kintree_table[0] of the official pickle, articulate/model.py:38-39)
smpl_parent = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)

# sync_mp3d (net/sig_mp.py:287-299): landmark row -> SMPL joint id that overwrites it
mp_joint_override = {11: 16, 12: 17, 13: 18, 14: 19, 15: 20, 16: 21, 23: 1, 24: 2, 25: 4, 26: 5, 27: 7, 28: 8}

# MediaPipe landmark ids whose confidence the smplify residual zeroes (temporal_smplify.py:92)
smplify_ignored_landmarks = (1, 2, 3, 4, 5, 6, 7, 8, 9, 31, 32)

NUM_IMU = 6
NUM_KP = 33
NUM_JOINT = 24

# (name, input, hidden, output) of the six sub-nets, net/sig_mp.py:52-81
NETS = (
    ("rnn2", 72, 512, 69),
    ("rnn3", 141, 512, 3),
    ("rnn4", 171, 1280, 69),
    ("rnn6", 240, 1024, 3),
    ("rnn7", 141, 512, 144),
    ("rnn8", 141, 512, 2),
)
NET_INDEX = {n[0]: i for i, n in enumerate(NETS)}
# dropout rate each sub-net is built with, net/sig_mp.py:52-81 (after linear1 and between the LSTM layers, rnn.py:112,115)
DROPOUT = {n[0]: 0.1 if n[0] == "rnn7" else 0.4 for n in NETS}
# loss each sub-net is trained with, net/sig_mp.py:340,409-418,555,683,749-771,829-831 (robustcap_amd/losses.py)
LOSS = {"rnn2": "mse", "rnn3": "window_mse", "rnn4": "mse", "rnn6": "mse", "rnn7": "pose_fk", "rnn8": "bce_logits"}
# eval_fn each sub-net is validated with, net/sig_mp.py:341,556 (rnn2, rnn4: RNNLossWrapper(PositionErrorEvaluator())); the others pass
# their loss_fn (:431,694,784,836) (robustcap_amd/losses.py: EVAL_KINDS)
EVAL = dict(LOSS, rnn2="position_error", rnn4="position_error")


def _train(num_epoch, between, lr, patience):
    # shared by all six: clip_grad_norm=1 (:355,432,572,695,785,837), DataLoader(train, 256, shuffle=True) (:348,426,562,689,779,825),
    # DataLoader(valid, 64) (:352,430,566,693,783,827), split_size=200 for the training sets (:346-347,423-424,560-561,687-688,776-777,825)
    # and -1 (whole sequences) for the validation sets
    return {"num_epoch": num_epoch, "num_iter_between_vald": between, "clip_grad_norm": 1.0, "lr": lr, "lr_scheduler_patience": patience,
            "batch_size": 256, "valid_batch_size": 64, "split_size": 200}


# what the reference passes to train() for each sub-net (articulate/utils/torch/train.py:15-18), settings only
TRAIN = {
    "rnn2": _train(150, 20, 1e-3, None),       # net/sig_mp.py:354-355; Adam's default lr (train.py:53)
    "rnn3": _train(200, 20, 1e-3, None),       # :431-432
    "rnn4": _train(200, 60, 1e-4, None),       # :571-572; optimizer = Adam(lr=1e-4) at :569
    "rnn6": _train(100, 60, 1e-3, 5),          # :694-697
    "rnn7": _train(120, 20, 1e-3, 5),          # :784-787
    "rnn8": _train(80, 20, 1e-3, 10),          # :836-839
}
# augment_fn of each sub-net's datasets, net/sig_mp.py:360-363,438-442,578-581,701-703,792-795: torch.normal(x, sigma) on the last 69
# columns ("tail") or on every column ("all"); None: the identity (robustcap_amd/batches.py, csrc/rc_augment.hip)
AUGMENT = {"rnn2": None, "rnn3": ("tail", 69, 0.04), "rnn4": None, "rnn6": ("tail", 69, 0.03), "rnn7": ("all", 0.03), "rnn8": ("tail", 69, 0.03)}
# the random camera of the AMASS samples, net/sig_mp.py:528,657 (generate_random_rotation_matrix_constrained, degrees), and whether the
# keypoints are bounding-box normalised afterwards (:546-548; rnn6 keeps them raw)
CAMERA = {"rnn4": {"yaw": (-180, 180), "pitch": (-30, 30), "roll": (-5, 5), "normalise": True},
          "rnn6": {"yaw": (-90, 90), "pitch": (-30, 30), "roll": (-5, 5), "normalise": False}}
# rnn2.init_net: Linear(69,512) ReLU Linear(512,1024) ReLU Linear(1024,2048)  (rnn.py:195-201)
INIT_NET = ((69, 512), (512, 1024), (1024, 2048))

# 2 * MACs of one pass of all six nets (linear1 + 2 LSTM layers + linear2), SURVEY.md section 8(d)
FLOPS_PER_BODY_FRAME = 121_379_840
# of which the six linear2 layers (2 * H * out each); at batch > 16 they run on rc_gemm_small_kernel, everything else
# (linear1 + both LSTM layers of all six sub-nets) on rc_gemm_kernel
FLOPS_LINEAR2_PER_BODY_FRAME = 2 * (512 * 69 + 512 * 3 + 1280 * 69 + 1024 * 3 + 512 * 144 + 512 * 2)


def state_dict_spec():
    """[(key, shape)] of every tensor in the reference ``Net.state_dict()`` in torch's order."""
    spec = []
    for name, nin, h, nout in NETS:
        for l in (0, 1):
            spec += [(f"{name}.rnn.weight_ih_l{l}", (4 * h, h)), (f"{name}.rnn.weight_hh_l{l}", (4 * h, h)),
                     (f"{name}.rnn.bias_ih_l{l}", (4 * h,)), (f"{name}.rnn.bias_hh_l{l}", (4 * h,))]
        spec += [(f"{name}.linear1.weight", (h, nin)), (f"{name}.linear1.bias", (h,)),
                 (f"{name}.linear2.weight", (nout, h)), (f"{name}.linear2.bias", (nout,))]
        if name == "rnn2":
            for i, (a, b) in zip((0, 2, 4), INIT_NET):
                spec += [(f"{name}.init_net.{i}.weight", (b, a)), (f"{name}.init_net.{i}.bias", (b,))]
    return spec

# the twelve LSTM layer steps alone (2 layers x [B, 2H] x [2H, 4H] per sub-net): what rc_gemm_lds_kernel computes
FLOPS_LSTM_PER_BODY_FRAME = 2 * sum(2 * (2 * H) * (4 * H) for H in (512, 512, 1280, 1024, 512, 512))
