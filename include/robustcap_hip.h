/*
 * robustcap_hip.h -- C ABI of the MI355X (gfx950) implementation of RobustCap's sig_mp per-frame path.
 *
 * The reference (shaohua-pan/RobustCap) is pure Python/PyTorch and has no FFI of its own; every entry point
 * below names the reference Python interface it replaces (paths relative to the reference repo root). The
 * Python host (robustcap_amd/) binds these with ctypes; see INTEGRATION.md for the stub a reference
 * maintainer would add.
 *
 * Conventions
 *   - All tensors are float32, row-major, resident in device memory unless a parameter says "host".
 *   - The caller owns every I/O buffer and passes raw device pointers plus the HIP stream to enqueue on
 *     (hipStream_t is passed as void*). The library owns only its context (packed weights, recurrent state,
 *     scratch). No call synchronises the device except rc_create / rc_finalize_weights / rc_set_body / rc_set_mesh /
 *     rc_shape_body / rc_get_state / rc_set_state / rc_get_trace / rc_destroy; rc_sequence synchronises `stream` ONCE per call when its
 *     launch planner is on AND the call has at least min_frames frames (rc_set_sequence_mode; shorter calls and mode 0 are
 *     fully asynchronous), rc_camera_inputs_rows once (constant upload), the
 *     *_host-mean variants of the metric calls and rc_smplify_* as documented with them. Short of a synchronisation, a call whose table
 *     travels through pinned copies waits on the HOST for an earlier upload from the copy it takes -- the sub-net forward / backward /
 *     weight-gradient entries for the previous such call's plan, the entries with a ring of four for the call four calls earlier -- so a
 *     chain of them on a stream that is held up returns only as those uploads pass; and a call that grows context-owned scratch waits as
 *     its paragraph says.
 *   - Every function returns 0 on success or a negative rc_status; rc_last_error() gives a message. Nothing
 *     throws across the boundary. A context is not re-entrant; distinct contexts on distinct streams are
 *     independent.
 *   - "row" = one body (one sequence/camera) of the batch; rows never interact.
 */
#ifndef ROBUSTCAP_HIP_H
#define ROBUSTCAP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rc_ctx rc_ctx;

typedef enum {
    RC_OK = 0,
    RC_ERR_INVALID = -1,    /* bad argument                                  */
    RC_ERR_HIP = -2,        /* a HIP runtime call failed                     */
    RC_ERR_STATE = -3,      /* call order (weights / body not loaded yet)    */
    RC_ERR_UNKNOWN_KEY = -4 /* rc_load_weight: not a sig_mp state_dict key   */
} rc_status;

/* Behaviour switches = the class attributes callers poke on the reference Net (net/sig_mp.py:27-45, 91-93). */
typedef struct {
    double conf_lo, conf_hi;       /* Net.conf_range: (0.7, 0.8); (0.85, 0.9) when constructed live      */
    float contact_threshold;       /* 0.7                                                                */
    float distance_threshold;      /* Net.distrance_threshold = 10                                       */
    float height_threshold;        /* Net.height_threhold = 0.15                                         */
    double tran_filter_num;        /* 0.05; 0.01 when constructed live                                   */
    int32_t use_flat_floor;        /* 1                                                                  */
    int32_t use_vision_updater;    /* 1                                                                  */
    int32_t use_imu_updater;       /* 1                                                                  */
    int32_t live;                  /* Net.live: landmark refresh every update_vision_freq+1 frames       */
    int32_t update_vision_freq;    /* 30                                                                 */
    int32_t use_reproj_opt;        /* 0; Net.use_reproj_opt: closed-form translation refinement L245-261  */
    float smooth;                  /* Net.smooth = 1 (regulariser of that refinement)                    */
    int32_t reserved;
} rc_params;

/* rc_step flags */
#define RC_FLAG_FIRST_FRAME 1u /* forward_online(first_frame=True), net/sig_mp.py:114,149,155,208,224 */

/* ---- lifecycle ------------------------------------------------------------------------------------------ */
/* Replaces Net() / Net().to(device) (net/sig_mp.py:47-93). batch = number of independent rows (>= 1).
 * live_at_construction mirrors "Net.live = True" BEFORE construction (evaluate.py:392). */
int rc_create(int32_t batch, int32_t live_at_construction, rc_ctx** out);
int rc_destroy(rc_ctx* ctx);
const char* rc_last_error(const rc_ctx* ctx); /* ctx may be NULL: last error of a failed rc_create */
int rc_default_params(int32_t live_at_construction, rc_params* out);
int rc_get_params(const rc_ctx* ctx, rc_params* out);
int rc_set_params(rc_ctx* ctx, const rc_params* p);

/* Replaces Net.load_state_dict (evaluate.py:58): one call per state_dict entry, key names and shapes as in
 * the reference ("rnn2.rnn.weight_ih_l0", "rnn4.linear1.bias", "rnn2.init_net.4.weight", ...).
 * `host` points to numel float32 values in HOST memory (torch layout). rc_finalize_weights repacks everything
 * to the kernel layout and uploads; it fails if a key is missing. The library keeps NO host copy afterwards (254 MB per
 * context otherwise): a later reload -- also of a single tensor -- passes every tensor again before the next finalize. */
int rc_load_weight(rc_ctx* ctx, const char* key, const float* host, int64_t numel);
int rc_finalize_weights(rc_ctx* ctx);

/* Replaces art.ParametricModel(paths.smpl_file) as consumed by the path (articulate/model.py:29-40,78-93 and
 * config.mp_mask): parent[24] (parent[0] ignored), rest joints J[24,3], and for the 33 landmark vertices the
 * skinning weights w33[33,24] and template positions v33[33,3]. HOST pointers. */
int rc_set_body(rc_ctx* ctx, const int32_t* parent, const float* J, const float* w33, const float* v33);

/* Replaces "net.gravityc = ..." (evaluate.py:73): per-row gravity direction in the camera frame, HOST [batch,3]. */
int rc_set_gravity(rc_ctx* ctx, const float* gravity_host);

/* Replaces Net.reset_states (net/sig_mp.py:95-104). row_mask: DEVICE uint8[batch] (non-zero = reset) or NULL
 * for all rows. Like the reference it does not touch update_vision_count / j_temp / gravity. */
int rc_reset(rc_ctx* ctx, const uint8_t* row_mask, void* stream);

/* ---- the hot path --------------------------------------------------------------------------------------- */
/* Replaces Net.forward_online (net/sig_mp.py:113-274) for `batch` rows at once; row b == the reference run
 * alone on sequence b. j2dc[batch,33,3] (x/z, y/z, conf), accc[batch,6,3], oric[batch,6,3,3]; first_tran
 * [batch,3] or NULL; pose_out[batch,24,3,3] (local rotations, root = camera-frame IMU), tran_out[batch,3].
 * Enqueues ~14 kernels on `stream`; no host synchronisation, all branching is device side. */
int rc_step(rc_ctx* ctx, const float* j2dc, const float* accc, const float* oric, const float* first_tran,
            uint32_t flags, float* pose_out, float* tran_out, void* stream);

/* The evaluate.py per-sequence loop (evaluate.py:75-83) for all rows: frames t = 0..T-1, inputs and outputs
 * indexed [row][t] with element strides  row_stride_* (between rows) and T contiguous frames per row:
 *   j2dc + row*rs_j2d + t*99, accc + row*rs_acc + t*18, oric + row*rs_ori + t*54,
 *   pose_out + row*rs_pose + t*216, tran_out + row*rs_tran + t*3.
 * Frame 0 uses first_tran (if not NULL) and `flags`; later frames use neither. See rc_set_sequence_mode for how the
 * frames are scheduled (and for the one synchronisation of `stream` the default mode costs per call). */
int rc_sequence(rc_ctx* ctx, int32_t T, const float* j2dc, int64_t rs_j2d, const float* accc, int64_t rs_acc,
                const float* oric, int64_t rs_ori, const float* first_tran, uint32_t flags, float* pose_out,
                int64_t rs_pose, float* tran_out, int64_t rs_tran, void* stream);

/* rc_sequence for rows of DIFFERENT lengths, without padding: len_host HOST int32[batch], 0 <= len_host[b] <= T; every other argument
 * as rc_sequence (the [row][t] layout keeps T frames per row). Row b runs frames 0 .. len_host[b] - 1 and nothing else:
 *   - its pose_out / tran_out of those frames, its (h, c) of all six sub-nets, its fusion state (rc_get_fusion_state, including a
 *     pending updater step and that step's inputs) and its trace are BITWISE what rc_sequence(T = len_host[b]) leaves for that row in
 *     a context of the same batch and gemm mode: a row's bits depend neither on the batch, the tile shape or the engine, nor on the
 *     other rows' lengths;
 *   - output elements of frames t >= len_host[b] are NOT WRITTEN and inputs of those frames are NOT READ (NaN / inf there change
 *     nothing); a row of length 0 is untouched altogether -- `flags` / first_tran of frame 0 do not apply to it. first_tran and
 *     `flags` keep their meaning for frame 0 of every row of length >= 1;
 *   - a row whose last frame is occluded leaves its deferred rnn6 / rnn4 step pending in the context's own buffers, as the last
 *     frame of a uniform call does -- at frame len_host[b] - 1, while the other rows go on. A following call (rc_sequence or
 *     rc_sequence_rows) continues every row from where it stopped, so a long recording can be streamed in chunks beside shorter ones.
 * Every engine of rc_set_sequence_mode runs such a call (wavefront ticks launch only the problems that still have rows, the
 * frame-stepped launches select the rows that still have the frame and pick their tiles for that many; frames that no row has are not
 * launched), the resident layer-step kernel included. Calls longer than RC_SEQ_MAX_PLAN_FRAMES are planned in pieces as before, the
 * lengths clipped per piece. Synchronisation as rc_sequence: at most the read-back of the plan, per piece (the lengths are staged in
 * two pinned halves taken in turn, so a call only makes sure that the upload of the call before the previous one has left its half --
 * long done by then). len_host is consumed before the call returns. Rows of one common length run exactly the launches of rc_sequence(T = that length).
 * RC_ERR_INVALID (nothing enqueued) on a null len_host or a length < 0 or > T.
 * rc_get_sequence_row_frames: row-frames computed by rc_sequence / rc_sequence_rows since rc_create (batch * T per uniform call, the
 * sum of the lengths per ragged one); rc_get_sequence_stats keeps counting frame INDICES run by each engine, and ticks.
 * rc_plan_wave_rows: rc_plan_wave (below) with per-row ends, len HOST int32[B], 0 <= len[b] <= T: row b starts frames
 * t0 .. len[b] - 1 only, its last frame books no rider, and a row with len[b] <= t0 books nothing (a step pending in front of the
 * segment stays pending). len[b] == T for every row gives rc_plan_wave's outputs. */
int rc_sequence_rows(rc_ctx* ctx, int32_t T, const int32_t* len_host, const float* j2dc, int64_t rs_j2d, const float* accc,
                     int64_t rs_acc, const float* oric, int64_t rs_ori, const float* first_tran, uint32_t flags, float* pose_out,
                     int64_t rs_pose, float* tran_out, int64_t rs_tran, void* stream);
int rc_get_sequence_row_frames(rc_ctx* ctx, int64_t* body_frames);

/* Arithmetic of the GEMM products of EVERY launch of a context (linear layers, LSTM gate GEMMs, init_net):
 *   mode 0: v_mfma_f32_16x16x4_f32 -- fp32 operands, bitwise an fma chain per output element;
 *   mode 1: split-bf16 products on v_mfma_f32_16x16x32_bf16 -- every fp32 operand is the exact sum of three bf16 numbers
 *           (weights split once at rc_finalize_weights, activations on the fly) and every product the fp32-accumulated sum
 *           of the partial products down to 2^-16 of it (what is dropped is below 2^-23 of a product, i.e. below the
 *           rounding of the running fp32 sum); operands, accumulators, gates and state stay fp32. Same accuracy class as
 *           mode 0 (parity with the reference: tests), 2.7x fewer MFMA cycles per product.
 *   mode 2: the fast mode, a REDUCED-precision one, for offline batches that can spend part of the 1e-4 m / 0.1 deg budget. Every fp32
 *           operand a becomes TWO bf16 terms by rounding -- hi = RN_bf16(a) (round to nearest, ties to even), mid = RN_bf16(a - hi);
 *           the subtraction is exact, nothing below mid is kept -- and a 16x16x32 block pair is three products with fp32
 *           accumulation, small terms first: a_mid.w_hi, a_hi.w_mid, a_hi.w_hi. Half the MFMAs of mode 1 and 4 B per weight
 *           instead of 6. Two finite operands' product is off by at most about 3 x 2^-16 |a w| (mode 1: 2^-23); |a| within half a
 *           bf16 ulp of FLT_MAX rounds to inf where the truncation of mode 1 did not. Everything outside the products -- the order of
 *           k-blocks, K quarters and halves, bias, epilogues, dispatch -- is mode 1's. The weight planes of this mode are built on the
 *           device from the fp32 packing the first time a context is in mode 2 with finalized weights (a context that never is
 *           allocates nothing) and follow every later weight change (rc_finalize_weights, rc_update_subnet_weights,
 *           rc_subnet_optim_step). Against oracle/lstm_f64.py a step stays within G = 8 times the bound modes 0 and 1 are held to
 *           (tests/test_gemm_mode2_cpu.py: where 8 comes from); the reference fixtures are reproduced to 5e-6 m / 1e-4 deg on the
 *           seeded synthetic weights they use -- trained weights have not been tried. Never a default: rc_default_gemm_mode returns
 *           0 or 1; RC_GEMM_SPLIT=2 in the environment makes new contexts start in it. The sub-net entries (rc_subnet_forward* /
 *           _backward* / _weight_grads, rc_init_net_forward) return RC_ERR_INVALID in mode 2; the resident kernel (rc_set_resident) is
 *           not used, a mode-2 context runs its segments on the streams; the lean live frame is fp32-only as before.
 * Default: mode 1 for contexts of batch >= 48, mode 0 below (weight-streaming bound: 6 B instead of 4 B per weight would
 * slow them). Within one mode a row's result does not depend on the batch, the tile shape or the engine
 * (bitwise); between modes 0 and 1 results differ by fp32 rounding noise, mode 2 by the figures above. Any change of mode ends
 * a live session. rc_get_gemm_mode returns the mode. */
int rc_set_gemm_mode(rc_ctx* ctx, int32_t mode);
int rc_get_gemm_mode(const rc_ctx* ctx);
int rc_default_gemm_mode(int32_t total_rows);   /* the default of a context of that many rows (0 or 1, never 2) */
int rc_initial_gemm_mode(int32_t total_rows);   /* the mode rc_create gives a context of that many rows: the default, or 2 under RC_GEMM_SPLIT=2
                                                   (the one reading of that variable). Sharded runs pin every shard to the TOTAL's */

/* Sequence mode of rc_sequence (on by default). With mode >= 1 every rc_sequence call of T >= 2 frames first classifies
 * each (frame, row) on the device (the arithmetic of the per-frame prep kernel), reads the codes back -- ONE
 * synchronisation of `stream` per call -- and plans the launches on the host:
 *   - the PER-ROW-CURSOR WAVEFRONT engine runs every frame but one that takes first_frame / first_tran: the stages of a
 *     frame (prep | linear1 | LSTM l0 | l1 | linear2 of {rnn2, rnn4} + fuse | the same four of {rnn6, rnn3, rnn7, rnn8} +
 *     tail) are skewed over consecutive ticks and a 16-slot ring, two merged gate-GEMM launches per tick carry the stages of
 *     up to eight frames -- one on `stream`, the other (from 48 rows) on a context-owned stream -- and the per-row kernels
 *     run beside them on another context-owned stream; all of it is joined back into `stream` before the call returns, so
 *     the caller sees ordinary stream order. Rows are independent, so each
 *     row has its own frame cursor: the vision updater's feedback (net/sig_mp.py:264-271) and the one-shot init_net
 *     (L178-183) make only THAT row wait (8 / 6 ticks, once per occlusion / once per sequence) while the batch keeps
 *     ticking; the updater's rnn6 / rnn4 steps ride the launches of the ring slot that starts when the frame's tail runs.
 *     This is the full-sequence form of the recurrence (the reference's own is RNN.forward over packed sequences,
 *     articulate/utils/torch/rnn.py:129-133); every row's outputs and states are bitwise those of the frame-stepped launches;
 *   - mode 1 takes that engine when the plan's cost estimate beats the frame-stepped launches (short calls with lagging
 *     rows do not) and the call has >= min_frames frames; mode 2 takes it whenever the call has >= min_frames frames;
 *   - frame-stepped frames run without the three transition launches when the plan proves that no row needs one.
 * mode = 0: frame-stepped launches only, no pre-pass, no synchronisation. Live contexts (rc_params.live) always behave
 * like mode 0. rc_get_sequence_stats: frames run by each engine and ticks launched since rc_create (any may be NULL).
 * rc_plan_sequence (transition-launch marks of frame-stepped frames) and rc_plan_wave are the planners alone on HOST data
 * (tests): codes[T*B] (0: c <= lo, 1: mid, 2: c >= hi; frame-major), first_reach[B], pend[B] (state in front of frame 0 /
 * t0) -> mode_out[T] (0 frame-stepped with the three transition launches, 1 without);
 * rc_plan_wave -> *n_ticks, *n_prep (ticks that start frames or riders), frame_at[n_prep*B] (frame row b starts at tick k,
 * or -1), counts[4*n_prep] (rows starting a frame / of them visible / riders / init_net rows, per tick; may be NULL),
 * est_us[2] (cost estimates wavefront / frame-stepped; may be NULL). RC_ERR_INVALID with *n_prep set when frame_at_cap
 * (ints) is too small. */
int rc_set_sequence_mode(rc_ctx* ctx, int32_t mode, int32_t min_frames);
int rc_get_sequence_stats(rc_ctx* ctx, int64_t* wave_frames, int64_t* stepped_frames, int64_t* ticks);
/* Launch counts since rc_create: launches of the shared-weight kernel of the LSTM layer steps (rc_gemm_lds_kernel, round 6: contexts of
 * >= RC_LDS_MIN_BATCH rows in split-product mode), and launches of the other wide / mid-tile kernels (either may be NULL). Replaces
 * nothing in the reference: its per-frame loop (net/sig_mp.py:126-129) has no launch structure to mirror; this is introspection for
 * bench.py and the tests. (Round 5 counted its one-launch-per-tick kernel in the first slot; removed, profiles/r06_tick_path_removed.diff.) */
int rc_get_launch_stats(rc_ctx* ctx, int64_t* lds_launches, int64_t* other_wide_launches);
/* ... and, of `other_wide_launches`, those that ran on rc_gemm_split48_w32_kernel (contexts of 33-64 rows: one-reader launches stream the fp32
 * weights): bench.py names the kernel whose launches it timed (round-5 advisor item). */
int rc_get_launch_stats_w32(rc_ctx* ctx, int64_t* w32_launches);
/* Resident layer-step kernel of the wavefront engine (round 6; north_star: "fused persistent kernel ... across timesteps"). With enable != 0
 * a planned rc_sequence call of a context of 65 .. 256 rows in split-product mode runs the LSTM layer steps AND the linear1 layers of
 * ALL its ticks (net/sig_mp.py:126-129 over every frame of the call; articulate/utils/torch/rnn.py:129-133 is the reference's own
 * whole-sequence form) in ONE launch of `workgroups` (default 224, at most 240; 0 keeps the current value) resident workgroups that take work items from a
 * queue in device memory, ordered by counters instead of stream events; prep / linear2 / fuse / tail stay launches of the second stream.
 * Results are bitwise those of the stream engine. Default off (RC_SEQ_RESIDENT=1 switches it on at rc_create): measured slower than the
 * three-stream ticks. A wait inside the kernel that runs out (RC_SEQ_RESIDENT_BOUND_MS, 2000) marks the call failed: the NEXT
 * rc_sequence returns RC_ERR_STATE once and counts an abort. rc_get_resident_stats: segments run / aborts seen (either may be NULL). */
int rc_set_resident(rc_ctx* ctx, int32_t enable, int32_t workgroups);
int rc_get_resident_stats(rc_ctx* ctx, int64_t* segments, int64_t* aborts);
int rc_plan_sequence(const int8_t* codes, int32_t B, int32_t T, const int32_t* pend, uint32_t flags, int32_t use_vision_updater,
                     uint8_t* mode_out);
int rc_plan_wave(const int8_t* codes, int32_t B, int32_t T, int32_t t0, const int32_t* first_reach, const int32_t* pend,
                 int32_t use_imu_updater, int32_t use_vision_updater, int32_t* frame_at, int64_t frame_at_cap,
                 int32_t* n_ticks, int32_t* n_prep, int32_t* counts, double* est_us);
int rc_plan_wave_rows(const int8_t* codes, int32_t B, int32_t T, int32_t t0, const int32_t* len, const int32_t* first_reach,
                      const int32_t* pend, int32_t use_imu_updater, int32_t use_vision_updater, int32_t* frame_at, int64_t frame_at_cap,
                      int32_t* n_ticks, int32_t* n_prep, int32_t* counts, double* est_us);

/* ---- live / streaming mode (BASELINE config 5) ------------------------------------------------------------- */
/* The live_server.py loop (live_server.py:40-48): one frame per call, HOST tensors in and out exactly like
 * forward_online's CPU tensors. rc_live_begin captures the steady-state frame (H2D of the 171 input floats per row,
 * the 14 kernels, D2H of the 219 output floats; for batch <= 16 the kernels access the pinned host buffers directly and
 * the copies disappear) into a hipGraph on a private stream -- twice, with and without the three transition launches;
 * rc_live_step replays the short one when the confidences it was handed rule out a transition step, else the full one
 * (frames with first_tran / RC_FLAG_FIRST_FRAME take the ordinary enqueue path) and returns when the outputs are in
 * host memory. j2dc[batch,33,3], accc[batch,6,3], oric[batch,6,3,3], first_tran[batch,3]|NULL -> pose[batch,24,3,3],
 * tran[batch,3].
 * Round 6: before the pre-built AQL packet chain of the lean frame (batch <= 4) is trusted, rc_live_begin runs ONE probe frame through it
 * and through the graph replay of the same launches from the same state (every small device buffer of the context is saved and put back:
 * the check leaves no trace) and requires the same bits; otherwise the chain is dropped and live frames replay the graph
 * (rc_get_live_backend: aql = 0 and the reason). RC_LIVE_AQL_SELFCHECK=0 skips the check. */
int rc_live_begin(rc_ctx* ctx);
int rc_live_step(rc_ctx* ctx, const float* j2dc_host, const float* accc_host, const float* oric_host,
                 const float* first_tran_host, uint32_t flags, float* pose_host, float* tran_host);
int rc_live_end(rc_ctx* ctx);
/* For batch <= 4 rc_live_begin also captures the LEAN plan of the steady-state frame (csrc/rc_live.hip): seven dependent launches --
 * prep + linear1 | LSTM l0 | LSTM l1 + linear2 partial sums | (partials, fuse) + linear1 | LSTM l0 | LSTM l1 + partials | (partials) +
 * tail -- replayed for every frame that needs neither a transition step nor rnn2.init_net (L178-183) and is not a sequence start;
 * the other frames take the captures above. Same layer-step arithmetic as rc_step; linear2 sums per-tile partial products in a
 * fixed order instead of one MFMA chain, so a lean frame equals an rc_step frame to rounding (<= 1e-6), not bit for bit.
 * RC_LIVE_LEAN=0 in the environment of rc_create switches it off. Counters: frames replayed from the lean / the full captures. */
int rc_get_live_stats(rc_ctx* ctx, int64_t* lean_frames, int64_t* full_frames);
/* Round 5, the idle-time pre-step of a paced live stream (BASELINE config 5: "60 fps"; live_server.py:40-48 receives one camera frame
 * every 16.6 ms): when the caller left the device idle in front of a frame (>= RC_LIVE_PRESTEP_IDLE_US, default 500 us), rc_live_step
 * enqueues, behind that frame, the recurrent halves W_hh h(t-1) of the NEXT frame's twelve LSTM layer steps (half of the 243 MB of weights,
 * one launch, while the device would idle); the next lean frame then starts from them and streams only the input halves. Bitwise the same
 * layer steps. Any eager call in between (reset, rc_step, ...) discards them. presteps: enqueued since rc_create; available: the AQL chain
 * carries the pre-step programs (either may be NULL). */
int rc_get_live_prestep(rc_ctx* ctx, int64_t* presteps, int32_t* available);
/* Lean live frames that turned out not to be the lean plan's -- a row needed a transition step or triggered init_net (net/sig_mp.py:178-183,
 * L264-271) and the conservative host-side mirror of those flags in rc_live_step did not foresee it. The plan's first kernel checks both on the
 * device; such a frame changes nothing and rc_live_step replays it on the full capture, so the caller only sees a slower frame. Expected: 0. */
int rc_get_live_replayed(rc_ctx* ctx, int64_t* frames);
/* RC_LIVE_SPIN=1 (opt-in since round 6; a back-to-back caller's queue-ahead, RC_LIVE_SPIN_B2B, stays on): rc_live_step launches the first kernel of the NEXT lean frame before it returns; that kernel waits on the device for the
 * frame's inputs, which the next call writes straight into device memory. taken: frames that started from a waiting kernel; lost: waiting
 * kernels sent away (the next frame was not the lean plan's, something touched the state in between) or that gave up after 100 ms. */
int rc_get_live_spin(rc_ctx* ctx, int64_t* taken, int64_t* lost);
/* Host time of rc_live_step averaged over the lean frames so far, microseconds: {staging the inputs + choosing the capture, enqueue
 * (hipGraphLaunch), waiting for the frame, copying the outputs}. The frame's GPU time is inside the third. */
int rc_get_live_profile(rc_ctx* ctx, double* avg_us4);
/* The same split for the MOST RECENT lean frame, plus {1 if it started from a kernel waiting on the device, 1 if it used a pre-step}:
 * what bench.py attributes the slowest frames of a paced run with (host wake-up vs device time). Introspection; the reference's
 * live loop (live_server.py:40-48) has no counterpart. */
int rc_get_live_last_profile(rc_ctx* ctx, double* us6);
/* What rc_live_step uses for steady-state frames after rc_live_begin: *lean_captured = the seven-launch capture exists;
 * *aql = its dispatches are pre-built AQL packets on an HSA queue of the context's own (csrc/rc_aql.cpp: ~0.5 us of host time per
 * frame instead of hipGraphLaunch's ~7 us; RC_LIVE_AQL=0 switches it off); note: why not, when it is not (may be NULL) -- and, under RC_LIVE_LEAN_NC=2 only, "lean LSTM tiles 16 x 32:" with
 * the names of the four layer-step kernels the captured plan holds (the default plan of 16 x 16 tiles adds nothing). With one row the
 * last kernel of the chain stores the frame's sequence number to a pinned host word once every write of the frame is released at system
 * scope, and rc_live_step returns on that word (RC_LIVE_DONE_FLAG=0: on the queue's completion signal) -- outputs and the context's device
 * state are complete either way; rc_live_end / rc_destroy wait for the queue itself to drain. */
int rc_get_live_backend(rc_ctx* ctx, int32_t* lean_captured, int32_t* aql, char* note, int32_t note_len);

/* ---- per-op entry points (tests, harness; each a single kernel) ------------------------------------------ */
/* art.math.r6d_to_rotation_matrix (articulate/math/angular.py:249-264): r6d[n,6] -> R[n,3,3]. */
int rc_r6d_to_rotmat(const float* r6d, float* R, int64_t n, void* stream);
/* art.math.axis_angle_to_rotation_matrix (articulate/math/angular.py:221-233): aa[n,3] -> R[n,3,3]. */
int rc_axis_angle_to_rotmat(const float* aa, float* R, int64_t n, void* stream);
/* art.math.rotation_matrix_to_axis_angle (articulate/math/angular.py:236-246; the reference loops cv2.Rodrigues on
 * the host): R[n,3,3] -> aa[n,3], angle in [0, pi]. Restates the matrix -> vector branch of OpenCV 4.2's cvRodrigues2 in
 * float64: range check, nearest orthonormal matrix, acos, the s < 1e-5 branches (zero near the identity, sqrt of the
 * diagonal near pi). */
int rc_rotmat_to_axis_angle(const float* R, float* aa, int64_t n, void* stream);
/* art.math.rotation_matrix_to_r6d (articulate/math/angular.py:267-274): R[n,3,3] -> r6d[n,6] = first two columns. */
int rc_rotmat_to_r6d(const float* R, float* r6d, int64_t n, void* stream);
/* art.math.angle_between(rot1, rot2) for rotation matrices (angular.py:128-141): |Rodrigues(R1^T R2)| -> out[n]. */
int rc_angle_between(const float* R1, const float* R2, float* out, int64_t n, void* stream);
/* art.math.lerp(a, b, t) with a Python-double weight (articulate/math/general.py:15-24): out[n] = a * float(1 - t) +
 * b * float(t), the weights formed in double on the host exactly like `tensor * python_float`. */
int rc_lerp(const float* a, const float* b, double t, float* out, int64_t n, void* stream);
/* art.math.normalize_tensor(x, dim=-1, return_norm) (general.py:27-39): x[rows,width] -> out = x / |x|, norm[rows]|NULL. */
int rc_normalize_rows(const float* x, float* out, float* norm, int64_t rows, int32_t width, void* stream);
/* Keypoint normalisation of forward_online (net/sig_mp.py:150-152 with get_bbox_scale L277-284): kp[n,33,3] -> out[n,33,3]
 * (xy / max(bbox width, height), rows != 23 relative to row 23, confidence copied). */
int rc_bbox_normalise(const float* kp, float* out, int64_t n, void* stream);
/* The confidence mean that picks a frame's regime (net/sig_mp.py:138): j2dc[n,33,3] -> mean[n] = the float32 mean of the 33
 * confidences summed in the reference's order (torch's CPU reduction of the strided row `j2dc[:, -1]`), code[n] = 2 if
 * (double)mean >= hi, 1 if > lo, else 0. The kernel that plans rc_sequence, on the helper the per-frame prep uses. Either
 * output may be NULL, not both; n < 2^31. */
int rc_conf_mean(const float* j2dc, int64_t n, double lo, double hi, float* mean, int8_t* code, void* stream);
/* Shape blendshapes of ParametricModel.get_zero_pose_joint_and_vertex(shape) (articulate/model.py:88-91), before its root
 * alignment: verts_out[V,3] = tensordot(beta, shapedirs) + v_template, joints_out[24,3] = J_regressor . verts_out. All
 * pointers HOST (v_template[V,3], shapedirs[V,3,10], J_regressor[24,V] dense, beta[10]); computed on the device,
 * synchronous. The caller hands the shaped joints / landmark vertices to rc_set_body (and the vertices to rc_set_mesh):
 * every entry point of the context then works on the shaped body, which is how forward_kinematics(shape=...) and
 * smplify_runner(shape=...) are served (one shape per context, as TemporalSMPLify holds one per sequence). */
int rc_shape_body(rc_ctx* ctx, const float* v_template, const float* shapedirs, const float* J_regressor, const float* beta,
                  int32_t V, float* verts_out, float* joints_out);
/* ParametricModel.forward_kinematics_R (articulate/math/spatial.py:170-194): Rl[n,24,3,3] local -> Rg[n,24,3,3] global. */
int rc_fk_r(rc_ctx* ctx, const float* Rlocal, float* Rglobal, int64_t n, void* stream);
/* ParametricModel.bone_vector_to_joint_position / joint_position_to_bone_vector (spatial.py:126-167): [n,24,3] both. */
int rc_bone_to_joint(rc_ctx* ctx, const float* bone, float* joint, int64_t n, void* stream);
int rc_joint_to_bone(rc_ctx* ctx, const float* joint, float* bone, int64_t n, void* stream);
/* ParametricModel.get_zero_pose_joint_and_vertex(shape=None) (articulate/model.py:78-93): joint[24,3] = J - J[0] and,
 * when vert is not NULL (needs rc_set_mesh), vert[V,3] = v_template - J[0]. */
int rc_zero_pose(rc_ctx* ctx, float* joint, float* vert, void* stream);
/* ParametricModel.inverse_kinematics_R (articulate/math/spatial.py:197-221): Rg[n,24,3,3] -> Rl[n,24,3,3]. */
int rc_ik_r(rc_ctx* ctx, const float* Rglobal, float* Rlocal, int64_t n, void* stream);
/* fk() of forward_online (net/sig_mp.py:131-135): joints[n,24,3] from GLOBAL rotations + rest bone vectors. */
int rc_fk_bone(rc_ctx* ctx, const float* Rglobal, float* joints, int64_t n, void* stream);
/* ParametricModel.forward_kinematics(calc_mesh=True) restricted to the landmarks + sync_mp3d
 * (articulate/model.py:209-241, net/sig_mp.py:287-299): pose[n,24,3,3] local, tran[n,3] ->
 * grot[n,24,3,3] (may be NULL), joint[n,24,3], j33[n,33,3]. */
int rc_body_fk(rc_ctx* ctx, const float* pose, const float* tran, float* grot, float* joint, float* j33,
               int64_t n, void* stream);
/* One step of sub-net `net` ("rnn2".."rnn8") = f(i, x) of forward_online (net/sig_mp.py:126-129) on its
 * recurrent state: x[batch, in] -> y[batch, out]. row_mask DEVICE uint8[batch] or NULL (all rows): rows it does not select keep
 * h and c, their x is never read (NaN / inf there change nothing) and their y elements are left untouched (not zeroed). */
int rc_lstm_step(rc_ctx* ctx, const char* net, const float* x, const uint8_t* row_mask, float* y, void* stream);
/* Sub-net forward over a list of variable-length sequences: RNN.forward(x, init) in eval mode (articulate/utils/torch/rnn.py:121-133:
 * linear1 -> ReLU -> two-layer LSTM over a packed sequence -> linear2) for sub-net `net` ("rnn2".."rnn8"), time-hoisted: per time
 * chunk, linear1, the input half x . W_ih of each layer and linear2 run as tall GEMMs over every frame, only h . W_hh in the time loop.
 * n sequences of lengths_host[i] >= 1 frames (HOST int32[n]); x DEVICE [sum T_i, in] row-major with sequence i at row sum_{j<i} T_j,
 * y DEVICE [sum T_i, out] packed the same way. init_h / init_c DEVICE [2, n, H] or NULL (zeros); final_h / final_c DEVICE [2, n, H]
 * or NULL: every sequence's state after its last frame. Every output has the bits of rc_lstm_step run frame by frame on the same
 * rows in the context's gemm mode (rc_set_gemm_mode). Stateless with respect to the context's own recurrent state, counters, pending
 * updater steps and live capture: the call reads the packed weights and writes only its own scratch and the caller's buffers.
 * Scratch (grow-only, released by rc_destroy): the per-chunk buffers -- packed input, relu(linear1), the hoisted x halves and both
 * layers' h -- stay within RC_SUBNET_SCRATCH_BYTES whatever the lengths; beside them 24 * H bytes of state per sequence of a group
 * (a group: as many sequences as one time step's rows fit in that budget) and the plan, 4 bytes per frame of the call plus 8 per
 * sequence, in device and pinned host memory. Enqueued on `stream` with no device read-back; the host waits only for the previous
 * call's plan upload to leave the pinned buffer, and growing the scratch (hipFree / hipMalloc) synchronises the device. Calls on
 * different streams are ordered: a call waits for the previous call's work, whose scratch it reuses. RC_ERR_INVALID on n < 1, a
 * length < 1 or a null x / y (nothing enqueued). */
#define RC_SUBNET_SCRATCH_BYTES (256ll << 20)
int rc_subnet_forward(rc_ctx* ctx, const char* net, int32_t n, const int32_t* lengths_host, const float* x, float* y,
                      const float* init_h, const float* init_c, float* final_h, float* final_c, void* stream);
/* Training of one sub-net (the loop of articulate/utils/torch/train.py:117-122: loss_fn(net(d), l) -> backward() -> step()), split as
 * the project is: the reverse recurrence in HIP, every time-parallel reduction left to the caller (robustcap_amd/train.py).
 *
 * rc_subnet_forward_tape: rc_subnet_forward (rnn.py:121-133) with the same arguments, contract, plan and bits of y / final_* in each
 * gemm mode, which also records what back-propagation needs. acts DEVICE [3, F, H], F = sum T_i, rows in the caller's order like x:
 * relu(linear1), h of LSTM layer 0, h of layer 1 at every frame. tape DEVICE, opaque, rc_subnet_tape_floats(...) floats (host-only
 * entry, nothing enqueued): init_c by rank [2, n, H], then per layer the post-activation gates i, f, g, o [F, 4H] and c [F, H] in the
 * plan's row order -- 40 * H bytes per frame. RC_ERR_INVALID also when the allocation behind acts or tape ends before the call's
 * extent (nothing enqueued). Stateless with respect to the context like rc_subnet_forward. */
int rc_subnet_forward_tape(rc_ctx* ctx, const char* net, int32_t n, const int32_t* lengths_host, const float* x, float* y,
                           const float* init_h, const float* init_c, float* final_h, float* final_c, float* acts, float* tape,
                           void* stream);
int rc_subnet_tape_floats(rc_ctx* ctx, const char* net, int32_t n, const int32_t* lengths_host, int64_t* floats);
/* Back-propagation through time of the two LSTM layers of rc_subnet_forward_tape(net, n, lengths_host) (eval mode: no dropout), on the
 * same plan, chunks last to first: per step one launch of the sub-net GEMM kernel forms dh_rec = dG(t + 1) . W_hh on the layer's
 * transposed pack (built on the device from the fp32 packing on first use; 20 * H * H bytes per layer) in the context's gemm mode, and
 * its epilogue the cell's backward; per chunk and layer one tall launch forms dG . W_ih.
 * In: tape; d_h1 DEVICE [F, H], the gradient of layer 1's h at every frame in the caller's order (dy . W2); d_final_h / d_final_c
 * [2, n, H] or NULL (zeros): the gradients of final_h / final_c. Out: d_gates [2, F, 4H], the gradients of the gate pre-activations
 * of layers 0 and 1, caller's rows, torch's columns g * H + u (g over i, f, g, o); d_a [F, H], the gradient of layer 0's input
 * relu(linear1) (the caller applies the relu mask from acts[0]); d_init_h / d_init_c [2, n, H] or NULL. The weight gradients are the
 * caller's reductions d_gates^T . input over all frames. Scratch (grow-only, released by rc_destroy): per chunk 20 * H bytes per row
 * within the forward's chunk buffers, beside them 80 * H bytes of state per sequence of a group. RC_ERR_INVALID on the forward's
 * cases, a null tape / d_h1 / d_gates / d_a, or when the allocation behind one of them ends before the call's extent (nothing
 * enqueued). Ordered with the other sub-net calls like them. */
int rc_subnet_backward(rc_ctx* ctx, const char* net, int32_t n, const int32_t* lengths_host, const float* tape, const float* d_h1,
                       const float* d_final_h, const float* d_final_c, float* d_gates, float* d_a, float* d_init_h, float* d_init_c,
                       void* stream);
/* Training with the reference's dropout (articulate/utils/torch/rnn.py:115,130-131: self.dropout = Dropout(p) on relu(linear1), and
 * torch.nn.LSTM's dropout = p on layer 0's output as layer 1's input, never on the recurrent path; net/sig_mp.py:52-81: p = 0.1 for
 * rnn7, 0.4 for the others). The mask is counter-based and stored nowhere: Philox4x32-10 (Random123) with key = (seed low 32 bits, seed
 * high 32 bits) and counter = (row, unit >> 2, site, call); output lane j decides unit 4 (unit >> 2) + j. row: the frame's row in the
 * CALLER's order (the row of x / acts / d_gates), so the mask does not depend on how a call is cut into chunks; site 0: after linear1,
 * 1: between the LSTM layers; call: one value per forward and its backward. A unit is kept iff its 32 bits >= (uint32_t)llrint(p * 2^32);
 * kept: x * (float)(1 / (1 - p)), dropped: +0.0f.
 *
 * rc_dropout_apply: dst[j * cols + k] = drop(src[j * cols + k]) for j < rows, with row = j: src, dst DEVICE [rows, cols] row-major,
 * 16-byte aligned, src == dst allowed; src = ones gives the scaled mask. p == 0 copies. RC_ERR_INVALID on a null pointer, cols % 4 != 0,
 * rows < 1 or >= 2^32, p outside [0, 1), site outside {0, 1}, or a misaligned or too small buffer (nothing enqueued). */
int rc_dropout_apply(rc_ctx* ctx, const float* src, float* dst, int64_t rows, int32_t cols, int32_t site, float p, uint64_t seed,
                     uint32_t call, void* stream);
/* rc_subnet_forward_tape in train mode (rnn.py:115,130-131 and torch.nn.LSTM's dropout, as above). With p == 0 it IS
 * rc_subnet_forward_tape: no dropout launch, the same bits. With p > 0, within the same scratch: relu(linear1) is dropped in place at
 * site 0 before layer 0 reads it, so acts[0] is the DROPPED relu(linear1); layer 1's input half reads h of layer 0 dropped at site 1,
 * while the recurrent h, acts[1] and the tape stay unmasked. RC_ERR_INVALID also on p outside [0, 1) (nothing enqueued). */
int rc_subnet_forward_train(rc_ctx* ctx, const char* net, int32_t n, const int32_t* lengths_host, const float* x, float* y,
                            const float* init_h, const float* init_c, float* final_h, float* final_c, float* acts, float* tape, float p,
                            uint64_t seed, uint32_t call, void* stream);
/* rc_subnet_backward of rc_subnet_forward_train(p, seed, call) (rnn.py:115,130-131 and torch.nn.LSTM's dropout): the site-1 mask is
 * regenerated and applied to dG1 . W_ih1 before layer 0's steps. d_a is the gradient of layer 0's input, i.e. of the DROPPED
 * relu(linear1): the caller applies site 0 (rc_dropout_apply) and the relu mask; of the weight gradients, layer 1's W_ih takes the
 * site-1 dropped acts[1] (rc_dropout_apply), W_hh the unmasked h. With p == 0 it IS rc_subnet_backward. */
int rc_subnet_backward_train(rc_ctx* ctx, const char* net, int32_t n, const int32_t* lengths_host, const float* tape, const float* d_h1,
                             const float* d_final_h, const float* d_final_c, float* d_gates, float* d_a, float* d_init_h,
                             float* d_init_c, float p, uint64_t seed, uint32_t call, void* stream);
/* The weight gradients of one sub-net on the device: what loss.backward() (articulate/utils/torch/train.py:117-122) leaves in the .grad
 * of linear1, the two LSTM layers and linear2 of an RNN module (articulate/utils/torch/rnn.py:121-133) -- every reduction over the frames
 * that rc_subnet_backward_train leaves to its caller, in the context's gemm mode (mode 1: both operands split into three bf16 terms
 * once per element, RC_SPLIT_PRODUCTS partial products on v_mfma_f32_16x16x32_bf16; mode 0: v_mfma_f32_16x16x4_f32), enqueued on
 * `stream` with no read-back and no host synchronisation (but growing the context's scratch, once per high-water mark).
 * In, all DEVICE, rows in the caller's order (F = sum T_i): x [F, in]; acts [3, F, H] of rc_subnet_forward_train; init_h [2, n, H] or
 * NULL (zeros); dy [F, out]; d_gates [2, F, 4H] of rc_subnet_backward_train (torch's columns g * H + u); d_p [F, H], the gradient of
 * linear1's pre-activation (d_a after the site-0 mask and the relu mask); (p, seed, call) of the forward. outs_dev: HOST array of twelve
 * DEVICE pointers in rc_update_subnet_weights's order (per LSTM layer weight_ih, weight_hh, bias_ih, bias_hh; linear1.weight, .bias;
 * linear2.weight, .bias); a NULL entry skips that tensor. For l = 0, 1:
 *   weight_ih_l = d_gates[l]^T . in_l, in_0 = acts[0] as stored, in_1 = acts[1] dropped at site 1 WHILE it is loaded (the mask of
 *     rc_dropout_apply(acts[1], site 1, p, seed, call); p == 0: none) -- no masked copy is made;
 *   weight_hh_l = d_gates[l]^T . h_prev_l, h_prev_l[f] = acts[l + 1][f - 1], at a sequence's first frame init_h[l][sequence] (or zero),
 *     read through a per-frame index built from lengths_host -- no shifted copy is made;
 *   bias_ih_l = bias_hh_l = the column sums of d_gates[l];
 *   linear2.weight = dy^T . acts[2], linear2.bias = column sums of dy; linear1.weight = d_p^T . x, linear1.bias = column sums of d_p.
 * Summation over the frames is deterministic and on two levels: at most 256 frames in the MFMA accumulators, those blocks into a second
 * fp32 accumulator; the frames are also cut into at most 16 parts of whole blocks (as many as fill the device, from the tile count),
 * whose partial sums a second pass adds in index order. No floating-point atomics: two calls give the same bits. Scratch: parts * the
 * padded output of the largest launch that is cut (grow-only). The column sums take the same blocks and parts in a kernel of their own,
 * on double accumulators rounded to fp32 once.
 * RC_ERR_INVALID on an unknown net, n < 1, a length < 1, a null operand or table, p outside [0, 1), or an operand or output whose
 * allocation ends before its extent; RC_ERR_STATE before rc_finalize_weights -- nothing is enqueued. Ordered with the other sub-net
 * calls like them; leaves the context's streams joined to `stream` like every eager entry. */
int rc_subnet_weight_grads(rc_ctx* ctx, const char* net, int32_t n, const int32_t* lengths_host, const float* x, const float* acts,
                           const float* init_h, const float* dy, const float* d_gates, const float* d_p, float p, uint64_t seed,
                           uint32_t call, void* const* outs_dev, void* stream);
/* Parts the frames of rc_subnet_weight_grads are cut into: 0 (default) = from the tile count, 1 .. 16 = that many (fewer when the call
 * has fewer 256-frame blocks). Either way the result is deterministic; the grouping of the sum, and so its rounding, follows the parts. */
int rc_set_subnet_wgrad_parts(rc_ctx* ctx, int32_t parts);
/* The optimiser step's way back (train.py:117-122: optimizer.step()): the tensors of ONE sub-net, already on the device, into every
 * device array rc_finalize_weights derives from them -- both packings of linear1 / linear2 (and the row-major copy of a narrow
 * linear2), the padded biases, both packings and the summed, permuted bias of each LSTM layer, for rnn2 the init_net layers, and the
 * transposed packs of rc_subnet_backward -- by element-wise kernels with the host packing's index arithmetic and truncation split,
 * bitwise what a reload of the same values gives. IN PLACE: every pointer held by launch tables, the sequence engine and a captured live
 * frame stays valid; the other sub-nets are untouched. tensors_dev: HOST array of `count` DEVICE pointers in the order of the
 * sub-net's keys in Net.state_dict() (per LSTM layer weight_ih, weight_hh, bias_ih, bias_hh; linear1.weight, .bias; linear2.weight,
 * .bias; rnn2: init_net.0 / .2 / .4 weight, bias): 12 tensors, rnn2 18. Ordered after all work the context has enqueued on any stream
 * (a device synchronise at entry) and before anything enqueued later (the call returns when its kernels on `stream` are done).
 * RC_ERR_INVALID on an unknown net, a wrong count or a null tensor; RC_ERR_STATE before rc_finalize_weights. */
int rc_update_subnet_weights(rc_ctx* ctx, const char* net, const void* const* tensors_dev, int32_t count, void* stream);
/* The second half of the training iteration (train.py:120-121: clip_grad_norm_(net.parameters(), max_norm), then optimizer.step() with
 * Adam as in every train_rnnK of net/sig_mp.py) for ONE sub-net, fused with rc_update_subnet_weights's repack and enqueued on `stream`
 * with no host synchronisation and no read-back. params_dev / grads_dev / exp_avg_dev / exp_avg_sq_dev: HOST arrays of `count` DEVICE
 * pointers (fp32, contiguous, the tensors' own shapes; the LSTM weight matrices and their gradients and moments 16-byte aligned) in
 * rc_update_subnet_weights's order, 12 tensors, rnn2 18. A NULL gradient skips
 * its tensor as torch does for p.grad is None: no share of the norm, parameter and moments untouched (it is still repacked).
 *  (a) total_norm = the 2-norm over all gradients: squares accumulated in double, per-workgroup partial sums added in index order by one
 *      workgroup, no floating-point atomics -- the same bits on every run. coef = min(1, max_norm / (total_norm + 1e-6)) in fp32, 1 when
 *      max_norm <= 0. norm_out_dev DEVICE float[2] receives {total_norm, coef}. The gradients themselves are NOT scaled (clip_grad_norm_
 *      scales them in place; here only the update sees coef * g).
 *  (b) per element of each padded packed matrix: g' = coef g + weight_decay p; m = beta1 m + (1 - beta1) g';
 *      v = beta2 v + (1 - beta2) g'^2; p -= (lr / bias_correction1) m / (sqrt(v) / sqrt(bias_correction2) + eps) in fp32, written back in
 *      place, and the new p stored into everything rc_update_subnet_weights rewrites (both packings, padded and summed biases, the
 *      row-major copy of a narrow linear2, rnn2's init_net, the transposed packs that exist) -- bitwise a reload of the stepped values.
 *      bias_correction1/2 = 1 - beta^step, formed by the caller in double.
 * Ordering: stream-ordered like every eager entry. Each entry leaves the context's internal streams joined to its caller's stream, so
 * the step follows everything enqueued on `stream` before it and precedes everything enqueued there later; the next live frame waits
 * for it. A caller who uses the context from a second stream orders that stream against `stream` itself (the partial sums live in one
 * context-owned buffer). While a live session is open (rc_live_begin) the call takes rc_update_subnet_weights's order instead: a device
 * synchronise at entry, and it returns when its kernels are done.
 * RC_ERR_INVALID on an unknown net, a wrong count, a null parameter / moment pointer or table, a null norm_out_dev, a non-positive
 * bias correction or a misaligned LSTM matrix; RC_ERR_STATE before rc_finalize_weights -- nothing is enqueued. */
int rc_subnet_optim_step(rc_ctx* ctx, const char* net, const void* const* params_dev, const void* const* grads_dev,
                         const void* const* exp_avg_dev, const void* const* exp_avg_sq_dev, int32_t count, double lr, double beta1,
                         double beta2, double eps, double weight_decay, double bias_correction1, double bias_correction2, double max_norm,
                         float* norm_out_dev, void* stream);
/* The first call of the training iteration (articulate/utils/torch/train.py:117, `loss = loss_fn(net(d), l)`) with the loss function the
 * reference trains each sub-net with, over the CONCATENATED batch as RNNLossWrapper hands it over (articulate/utils/torch/rnn.py):
 * x DEVICE [frames, width] (the sub-net's output), y DEVICE [frames, width] (the labels) -> value_dev DEVICE float[1] and, unless NULL,
 * dx_dev DEVICE [frames, width] = d value / d x, which feeds rc_subnet_backward_train as dy. Enqueued on `stream`, no read-back, no host
 * synchronisation. kind (rc_loss_kind):
 *   RC_LOSS_MSE (width 69 or 3; rnn2, rnn4, rnn6: net/sig_mp.py:340,555,683 MSELoss): mean (x - y)^2; dx = 2 (x - y) / (frames width).
 *   RC_LOSS_BCE_LOGITS (width 2; rnn8: sig_mp.py:829-831 BCEWithLogitsLoss(pos_weight)): aux_dev = pos_weight DEVICE float[2]; with
 *     L = 1 + (pw - 1) y the mean of (1 - y) x + L (max(-x, 0) + log1p(exp(-|x|))); dx = ((1 - y) - L (1 - sigmoid(x))) / (frames width).
 *   RC_LOSS_WINDOW_MSE (width 3; rnn3: sig_mp.py:409-415): mse(x, y) + the mse of the sums over windows of 6, 20 and 60 consecutive frames,
 *     the windows cut from the END of the batch (x[frames % w:].view(-1, w, 3).sum(1)): the first frames % w frames belong to no window
 *     of width w, and a window runs across sequence boundaries. frames >= 60 (below, the reference's value is the NaN of an empty mean).
 *   RC_LOSS_POSE_FK (width 144; rnn7: sig_mp.py:749-767): mse(x, y) + 100 mse(J(x), J(y)), J = the 24 joints (root included) from the 24
 *     r6d rotations (articulate/math/angular.py:249-264, NaN entries set to 0), every rest bone of the context's body (rc_set_body; the
 *     bones rc_joint_to_bone gives of rc_zero_pose's joints) turned by its PARENT's rotation and summed down the tree. A degenerate joint
 *     (first vector zero, or the second parallel to it) has R = 0 in the value; its own six entries of dx hold what the formulas give (NaN
 *     or inf, as the reference's autograd), every other entry and the value are unaffected.
 * Everything that enters the value is formed in double on the fp32 inputs: per-thread sums in a fixed order, one partial per workgroup in
 * a context-owned buffer (allocated by the first call), added in index order by one workgroup and rounded to fp32 once. No floating-point
 * atomics: two calls give the same bits. Calls on one context share that buffer: a caller who uses a second stream orders it itself.
 * x, y and dx 16-byte aligned (RC_LOSS_WINDOW_MSE: any alignment). RC_ERR_INVALID (nothing enqueued) on a null context, an unknown kind, a
 * width that does not fit the kind, frames <= 0, frames < 60 for RC_LOSS_WINDOW_MSE, RC_LOSS_POSE_FK before rc_set_body, RC_LOSS_BCE_LOGITS
 * without aux_dev, a null x, y or value_dev, or a misaligned pointer. */
typedef enum { RC_LOSS_MSE = 0, RC_LOSS_BCE_LOGITS = 1, RC_LOSS_WINDOW_MSE = 2, RC_LOSS_POSE_FK = 3 } rc_loss_kind;
int rc_subnet_loss(rc_ctx* ctx, int32_t kind, const float* x, const float* y, int64_t frames, int32_t width, const float* aux_dev,
                   float* value_dev, float* dx_dev, void* stream);
/* The metric of the validation pass (articulate/utils/torch/train.py:94-101 and :124-131: `vald_loss = sum([eval_fn(net(d), l) for (d, l)
 * in valid_dataloader]) / num_vald_step`, one value per validation BATCH) for every batch of a concatenated output in one call: x, y DEVICE
 * [F, width], F = the sum of group_frames_host[0 .. groups) (a HOST array); group g is frames [sum_{j<g} group_frames[j], ... +
 * group_frames[g]) -- what RNNLossWrapper (articulate/utils/torch/rnn.py) would torch.cat for validation batch g -- and values_dev DEVICE
 * float[groups] receives its value. Enqueued on `stream`: two launches whatever `groups` is, no read-back; the group table travels through a
 * ring of four pinned copies, so a call waits on the host only for the upload made four calls earlier (and for the stream where its
 * context-owned device table or partial sums grow: a new high-water mark of groups or of workgroups). kind:
 *   the four rc_loss_kind values (widths and aux_dev as for rc_subnet_loss): values_dev[g] has the BITS of rc_subnet_loss(kind, x_g, y_g,
 *     group_frames[g], width, aux_dev, value, dx = NULL) on a 16-byte aligned copy of the group's slice. By construction: group g runs the
 *     per-workgroup code of rc_subnet_loss's kernels in min(units of the group, 1024) workgroups of its own, each of which finds its (group,
 *     index) by bisection of the table, with the double reciprocals the host forms for such a slice; a group's partial sums are added in
 *     index order. A group that starts off the 16-byte grid (width 69, 3, or 2 after an odd number of frames) loads dwords instead of
 *     16-byte pieces; which element a thread adds when is the same. RC_LOSS_WINDOW_MSE cuts its windows from the END of the GROUP.
 *   RC_EVAL_POSITION_ERROR (width a multiple of 3; rnn2 and rnn4, 69: net/sig_mp.py:341,556 PositionErrorEvaluator,
 *     articulate/evaluator.py:129): the mean over the group's group_frames[g] width / 3 points of the Euclidean norm of x - y; differences,
 *     squares, square root and sums in double on the fp32 inputs, units of 1024 points, the same fixed-order sums, rounded to fp32 once.
 * No floating-point atomics: two calls give the same bits. Calls on one context share the table and the partial sums: a caller who uses a
 * second stream orders it itself. RC_ERR_INVALID (nothing enqueued, values_dev untouched; rc_last_error names this entry and, where one
 * is at fault, the group) on a null context, a null x, y, values_dev or group_frames_host, an unknown kind, a width that does not fit the
 * kind, groups < 1 or > 65536, a group of fewer than 1 frame (RC_LOSS_WINDOW_MSE: 60), RC_LOSS_POSE_FK before rc_set_body,
 * RC_LOSS_BCE_LOGITS without aux_dev, or x or y off the 16-byte grid (RC_LOSS_MSE, RC_LOSS_BCE_LOGITS, RC_LOSS_POSE_FK). */
typedef enum { RC_EVAL_POSITION_ERROR = 16 } rc_eval_kind;   /* beside the four rc_loss_kind values */
int rc_subnet_eval(rc_ctx* ctx, int32_t kind, const float* x, const float* y, int32_t groups, const int64_t* group_frames_host,
                   int32_t width, const float* aux_dev, float* values_dev, void* stream);
/* The batch in front of the training iteration (articulate/utils/torch/train.py:117-122 iterates a DataLoader(..., shuffle=True,
 * collate_fn=RNNDataset.collate_fn) whose every element is one RNNDataset.__getitem__, articulate/utils/torch/rnn.py:64-67, with the
 * sub-net's augment_fn): n samples gathered out of a corpus that stays on the device and augmented on the way, into ONE [F, W_out] and ONE
 * [F, W_label] buffer (F = sum of the lengths, sample i's frames from row sum_{j<i} lengths[j]). Enqueued on `stream`; no read-back; the
 * corpus is only read. data, label: DEVICE, the concatenated sequences; sample i is frames [offsets_host[i], offsets_host[i] +
 * lengths_host[i]) of both (HOST arrays, any order, repeats allowed; they travel through a ring of four pinned copies, so a call waits on
 * the host only for the upload made four calls earlier; the device table and the per-sample scratch grow at a new high-water mark of n).
 * kind (rc_batch_kind):
 *   RC_BATCH_PLAIN (every sub-net): data [., in], label [., out] of the sub-net (net/sig_mp.py:52-81). x_out = data rows with
 *     torch.normal(x, sigma) on the last 69 columns (rnn3 sigma 0.04: net/sig_mp.py:360-363; rnn6 0.03: :578-581; rnn8 0.03: :792-795) or
 *     on all columns (rnn7 0.03: :701-703); every other column, every column of rnn2 and rnn4 (:438-442: the identity) and of a call with
 *     augment == 0, and the label are copied bit for bit.
 *   RC_BATCH_WORLD (rnn4, rnn6 -- the AMASS __getitem__ of net/sig_mp.py:520-552 and :649-679): data [., 171] = acc[6,3] | ori[6,3,3] |
 *     j3dw_mp[33,3], label [., 72] = j3dw[24,3] in the world frame, conf_pool DEVICE [pool_rows, 33] (syn_c.pt). Per sample: Rc0c =
 *     Ry(yaw) Rx(pitch) Rz(roll) (articulate/math/angular.py:205-218; yaw in +-180 for rnn4, +-90 for rnn6, pitch +-30, roll +-5 degrees),
 *     formed in double and rounded to fp32 once, Rcw = (diag(-1,-1,1) Rc0c)^T; everything turned by Rcw; t = lerp((-1,-1,3), (1,1,8), u),
 *     t_z -= min over all frames and joints of j3dc_z; j3dc += t, j3dc_mp += t; j2dc = j3dc_mp / z; per frame a confidence row p of the pool,
 *     distinct rows within a sample (random.sample); j2dc_xy += 0.003 (1 - p) z; j2dc_conf = p. rnn4: xy / max(bbox width, height), rows
 *     != 23 relative to row 23 (get_bbox_scale, :277-284, :546-548); x_out = accc | oric | j2dc [F, 171], label_out = j3dc[1:] - j3dc[:1]
 *     [F, 69]. rnn6: label_out = j3dc[:, 0] [F, 3]; x_out = accc | oric | j2dc | j3dc[1:] - j3dc[:1] [F, 240] with the sigma 0.03 noise on
 *     the last 69 columns. augment must be non-zero.
 * Random draws: Philox4x32-10 (Random123), key = (seed low, seed high), counter = (sample i, frame within the sample, site | index << 8,
 * call); sites 2 (augment_fn noise; index = unit >> 2, unit counted from the first noisy column), 3 (camera: words 0-2 = yaw, pitch, roll),
 * 4 (translation: words 0-2), 5 (pool rows: a 4-round Feistel permutation of [0, pool_rows) cycle-walked, second counter word = the right
 * half, index = round), 6 (keypoint noise; index = keypoint >> 1). Uniforms (w >> 8) 2^-24, or ((w >> 9) + 0.5) 2^-23 under the
 * logarithm; normals by Box-Muller, two per word pair. The stream is not torch's nor Python's: only the distributions, the sites and the
 * order of the arithmetic are the reference's. No floating-point atomics: the same call gives the same bits.
 * RC_ERR_INVALID (nothing enqueued) on a null context, net, buffer or table, an unknown net or kind, RC_BATCH_WORLD for another sub-net,
 * without a pool or with augment == 0, n <= 0, a length < 1, a negative offset, a sample of more frames than the pool has rows, 2^31
 * frames or more, or a sample, an output or the pool reaching past its allocation. */
typedef enum { RC_BATCH_PLAIN = 0, RC_BATCH_WORLD = 1 } rc_batch_kind;
int rc_subnet_batch(rc_ctx* ctx, const char* net, int32_t kind, const float* data, const float* label, int32_t n,
                    const int64_t* offsets_host, const int32_t* lengths_host, const float* conf_pool, int32_t pool_rows, int32_t augment,
                    uint64_t seed, uint32_t call, float* x_out, float* label_out, void* stream);
/* rc_subnet_batch over a concatenation of corpora of one sub-net (torch.utils.data.ConcatDataset([AISTDataset, AMASSDataset]) of
 * net/sig_mp.py:559-566, :686-693: plain and world samples shuffled into one batch) in ONE call: one table upload, one launch per kind
 * present. Part p has kinds_host[p] and the DEVICE buffers data_parts[p] / label_parts[p] (HOST arrays of n_parts device addresses);
 * sample i is lengths_host[i] frames from frame offsets_host[i] of part part_host[i]; every world part draws from the same conf_pool.
 * x_out / label_out as in rc_subnet_batch, the samples in the order given. The Philox `sample` word is the sample's position i in the
 * whole batch, so sample i has the bits it has at position i of a single-kind rc_subnet_batch of equal lengths, seed and call.
 * RC_ERR_INVALID (nothing enqueued) as rc_subnet_batch, and on n_parts <= 0, a null part or a part index outside [0, n_parts). */
int rc_subnet_batch_parts(rc_ctx* ctx, const char* net, int32_t n_parts, const int32_t* kinds_host, const float* const* data_parts,
                          const float* const* label_parts, const float* conf_pool, int32_t pool_rows, int32_t n, const int32_t* part_host,
                          const int64_t* offsets_host, const int32_t* lengths_host, int32_t augment, uint64_t seed, uint32_t call,
                          float* x_out, float* label_out, void* stream);
/* The training corpus of one sub-net from the fields of a preprocessed dictionary: the dataset builders inside train_rnn2 .. train_rnn8
 * (net/sig_mp.py:302-336, :365-405, :444-518, :583-647, :705-747, :797-821), one call per sub-net and source, enqueued on `stream` with no
 * read-back. The fields are DEVICE fp32 buffers concatenated over the n_seq sequences (seq_frames_host[i] frames each, `frames` in all):
 * pose [frames, 72] axis-angle, imu_acc [frames, 6, 3], imu_ori [frames, 6, 3, 3], joint3d [frames, 24, 3], tran [frames, 3],
 * sync_3d_mp [frames, 33, 3]; a field the corpus does not read may be NULL. Every builder ends in [1:-1]: a sample of T frames gives T - 2
 * rows, row r is frame r + 1, and the velocity / contact stencils read frames r and r + 2 of the same sample; x_out DEVICE [R, in],
 * label_out DEVICE [R, out], R the sum over the samples, in sample order.
 *   rnn2, rnn3, rnn7, rnn8 (samples = sequences; n_samples 0 or n_seq, the sample arguments NULL): Rrw = R(root axis-angle)^T;
 *     x = Rrw acc | Rrw ori (rnn7: sensor 5 left as it is) and, but for rnn2, the root-frame joints 1 .. 23 relative to joint 0 (AIST:
 *     Rrw.matmul(j), then the difference; AMASS: (j - j0).bmm(R)), which are rnn2's label. Labels: rnn3 Rrw (j0[f + 1] - j0[f - 1]) 30 /
 *     vel_scale; rnn7 r6d of forward_kinematics_R(pose with root := I) (needs rc_set_body); rnn8 (AMASS only) 1.0 where
 *     |(j[f + 1] - j[f - 1]) 30| < 0.25 for joints 10 and 11, else 0.0.
 *   rnn4, rnn6 from AIST: sample s is sequence sample_seq_host[s] seen by the camera cam_K_host[s] (HOST [9]) / cam_T_host[s] (HOST [16],
 *     T_cw) with the keypoints kp DEVICE [kp_frames, 33, 3] = (u / image_w, v / image_h, confidence), concatenated over the samples;
 *     x = T_cw (acc; 0) | R_cw ori | K^-1 (u image_w, v image_h, 1) with the confidence last; rnn4: xy / get_bbox_scale and rows != 23
 *     relative to row 23 -- for sample_occ_host[s] != 0 (the joint2d_occ sample) WITHOUT the division, as :480 divides the other tensor --
 *     label T_cw (j; 1), joints 1 .. 23 minus joint 0; rnn6: raw xy, then those joints; label T_cw (tran; 1). K^-1 and the refusal of a
 *     camera are rc_camera_inputs_rows'.
 *   rnn4, rnn6 from AMASS: the world corpus of RC_BATCH_WORLD: x = acc | ori | sync_3d_mp - root with sync_mp3d's twelve joint
 *     overrides [., 171], label = joint3d - root [., 72], root = joint3d[0, 0] of the sequence.
 * No atomics: the same call gives the same bits. RC_ERR_INVALID (nothing enqueued or written) on a null context, net or field the corpus
 * reads, an unknown net or source, rnn8 from AIST, a sequence of fewer than 3 frames (the reference would form an empty tensor), a table
 * that does not sum to `frames` / `kp_frames`, 2^31 rows or more, a non-finite or singular camera, or a buffer shorter than its extent. */
typedef enum { RC_CORPUS_AIST = 0, RC_CORPUS_AMASS = 1 } rc_corpus_source;
int rc_subnet_corpus(rc_ctx* ctx, const char* net, int32_t source, int32_t n_seq, const int32_t* seq_frames_host, int64_t frames,
                     const float* pose, const float* imu_acc, const float* imu_ori, const float* joint3d, const float* tran,
                     const float* sync_3d_mp, int32_t n_samples, const int32_t* sample_seq_host, const int32_t* sample_occ_host,
                     const float* cam_K_host, const float* cam_T_host, const float* kp, int64_t kp_frames, float image_w, float image_h,
                     float* x_out, float* label_out, void* stream);
/* RNNWithInit.init_net (articulate/utils/torch/rnn.py:195-201, used at :207-219): Linear(69,512) ReLU Linear(512,1024) ReLU
 * Linear(1024,2048) on v DEVICE [n, 69] -> out DEVICE [n, 2048], on the packed weights of rnn2.init_net in the context's gemm mode. */
int rc_init_net_forward(rc_ctx* ctx, int32_t n, const float* v, float* out, void* stream);
/* rc_subnet_forward / rc_init_net_forward calls, frames run, time chunks launched, and device bytes of scratch held (any may be NULL). */
int rc_get_subnet_stats(rc_ctx* ctx, int64_t* calls, int64_t* frames, int64_t* chunks, int64_t* scratch_bytes);
/* Full-mesh skinning for the metrics of evaluate.py:120-133 (cal_mpjpe: PVE and regressor joints need every vertex).
 * rc_set_mesh uploads v_template[V,3] and weights[V,24] (HOST pointers, same J / parent as rc_set_body);
 * rc_body_mesh = ParametricModel.forward_kinematics(pose, tran, calc_mesh=True)[2] (articulate/model.py:229-241):
 * pose[n,24,3,3] local, tran[n,3] -> vert[n,V,3]. */
int rc_set_mesh(rc_ctx* ctx, const float* v_template_host, const float* weights_host, int32_t V);
int rc_body_mesh(rc_ctx* ctx, const float* pose, const float* tran, float* vert, int64_t n, void* stream);
/* Metrics of evaluate.py:120-133 (cal_mpjpe) fused on the device: both meshes skinned with zero translation,
 * keypoints = J_regressor[:n_used] . vertices (rc_set_regressor: HOST [n_rows,V] row-major, n_used = 14 in the
 * reference; without a regressor the 24 SMPL joints stand in), pelvis alignment, then per frame
 * {MPJPE, PVE, PA-MPJPE (Procrustes, utils.py:138-203)} -> per_frame DEVICE [n,3]. mean_host (HOST double[3] or NULL)
 * receives the means over the n frames (synchronises `stream`). */
int rc_set_regressor(rc_ctx* ctx, const float* j_regressor_host, int32_t n_rows, int32_t n_used);
int rc_mesh_metrics(rc_ctx* ctx, const float* pose, const float* gt_pose, int64_t n, float* per_frame, double* mean_host,
                    void* stream);
/* art.FullMotionEvaluator (articulate/evaluator.py:317-394) for every motion of a concatenated batch in one call, and the column means
 * behind PerJointErrorEvaluator (:155-215) and MeshErrorEvaluator (:256-314). pose_p, pose_t DEVICE [n,24,3,3] local rotations, tran_p,
 * tran_t DEVICE [n,3] or NULL (zeros, evaluator.py:361-362). Group g ("one motion") is frames [sum_{j<g} group_frames_host[j], ... +
 * group_frames_host[g]) (a HOST array, every entry >= 1, summing to n). Both motions run on the context's current body (rc_set_body; a
 * body shaped by rc_shape_body serves both) and, for the vertex error, on the full mesh of rc_set_mesh. Per group, exactly as
 * evaluator.py:365-382: offset = joint_t[align_joint] - joint_p[align_joint]; je, tre [N,24]; ve [N,V]; lae, gae [N,24] in degrees with the
 * angle of rc_angle_between on R_p^T R_t; jkp, jkt [N-3,24] = |x(t+3) - 3 x(t+2) + 3 x(t+1) - x(t)| fps^3 on the translated joints; te
 * [N-fps,1] on joint 0; the masked je / lae / gae over the joints of joint_mask (bit j = joint j). The stencils never reach across a
 * group boundary. out DEVICE [groups,11,2], rows in the order of evaluator.py:384-394 (je, ve, lae, gae, jkp, jkt, te, masked je, masked
 * lae, masked gae, tre): column 0 the mean over all elements, column 1 the mean over columns of the UNBIASED standard deviation over
 * frames (`x.std(dim=0).mean()`). Where the reference's expression is the mean or std of an empty or one-sample set the entry is torch's
 * value: NaN for the std of N = 1, the jerk rows of N <= 3 and the te row of N <= fps; joint_mask == 0 gives the reference's torch.zeros(1)
 * rows (0, NaN). per_joint DEVICE [groups,4,24] or NULL: the column means of je, lae, gae, tre. flags: RC_MOTION_NO_MESH skips the vertex
 * sweep and leaves row 1 NaN (every other entry keeps its bits); without it a context with no mesh returns RC_ERR_STATE.
 * Enqueued on `stream`: no read-back, no synchronisation; the group table travels through a ring of four pinned copies like
 * rc_subnet_eval's (a call waits on the host for the upload made four calls earlier, and for the stream where its context-owned scratch
 * grows). Column statistics are (mean, sum of squared deviations) pairs in double per block of 32 frames of ONE group, shifted by the
 * block's first value and merged in index order (Chan's update): no floating-point atomics, two calls give the same bits, and a group's
 * entries are those of a call with that group alone. Calls on one context share the scratch: a caller who uses a second stream orders it
 * itself. RC_ERR_INVALID (nothing written, nothing enqueued) on a null context, pose_p, pose_t, out or group_frames_host, n < 0 or >=
 * 2^31, groups < 1, an entry < 1, a sum of the entries != n, fps < 1, align_joint outside 0..23, mask bits >= 24 or an unknown flag;
 * n == 0 with groups == 0 is a no-op. */
#define RC_MOTION_NO_MESH 1u
int rc_motion_metrics(rc_ctx* ctx, const float* pose_p, const float* tran_p, const float* pose_t, const float* tran_t, int64_t n,
                      int32_t groups, const int64_t* group_frames_host, int32_t fps, int32_t align_joint, uint32_t joint_mask,
                      uint32_t flags, float* out, float* per_joint, void* stream);
/* art.math.svd_rotate (articulate/math/angular.py:144-184) on point sets, context-free like rc_procrustes_error: src, dst DEVICE [n,m,3],
 * `what` a combination of RC_ALIGN_R (calc_R), RC_ALIGN_T (calc_t) and RC_ALIGN_S (calc_s); 0 is the identity transform. Per set, exactly
 * as :159-183: the means are subtracted only with RC_ALIGN_T; s = sqrt(sum |dst - mu_d|^2 / sum |src - mu_s|^2) with RC_ALIGN_S, else 1;
 * with RC_ALIGN_R, H = (src - mu_s)^T (dst - mu_d) = U S V^T and Q = V U^T, and where det Q < -0.9 ROW 2 of V is negated (:175-177), so
 * R = diag(1,1,-1) Q -- the reference's rule, not the optimal proper rotation, and not rc_procrustes_error's (whose scale is trace / var
 * and whose fit runs on 14 keypoints); t = -s R mu_s + mu_d; moved = s src R^T + t. Outputs DEVICE: R [n,3,3], t [n,3], s [n], moved
 * [n,m,3]; each may be NULL, not all. A wave per set, float64 inside (two passes: means, then centred sums, added by a fixed tree; Q from
 * a one-sided Jacobi on H, unique for a full-rank H whatever signs LAPACK picks), rounded once.
 * Rank-deficient H (fewer than three non-coplanar centred points; the reference returns whatever LAPACK returns): singular directions
 * below 1e-13 of the largest are completed so that U is a proper rotation (H = 0: R = I); R is then finite and proper, and no reflection
 * is applied. s is the IEEE value of the reference's expression: inf (or NaN for 0 / 0) where sum |src - mu_s|^2 = 0, and t, moved follow.
 * RC_ERR_INVALID on n < 0 or >= 2^31, m < 1, unknown bits of `what`, a null src / dst or no output; n == 0 is a no-op. */
#define RC_ALIGN_R 1u
#define RC_ALIGN_T 2u
#define RC_ALIGN_S 4u
int rc_svd_rotate(const float* src, const float* dst, int64_t n, int32_t m, uint32_t what, float* R, float* t, float* s, float* moved,
                  void* stream);
/* PerJointErrorEvaluator / MeanPerJointErrorEvaluator (articulate/evaluator.py:195-210) and MeshErrorEvaluator (:298-313) with align_joint
 * -1 .. -5 for every motion of a concatenated batch in one call: -1 = R|T|S, -2 = R|T, -3 = T|S, -4 = T, -5 = S as `what`. pose_p, pose_t
 * DEVICE [n,24,3,3] local rotations; translations are zero (:191-194, 294-297); groups / group_frames_host as rc_motion_metrics. Per frame
 * TWO transforms are fitted by rc_svd_rotate's expressions: one on the 24 joints (its two-pass sums), one on the V vertices of the mesh of
 * rc_set_mesh (from folded sums, centred in ONE pass: sum p t^T - V mu_p mu_t^T, sum |p|^2 - V |mu_p|^2).
 * Outputs DEVICE, each may be NULL but not all: joint_err [groups,24] the column means over the group's frames of |joint_p' - joint_t|
 * (:210; the angle rows of :211-212 are untouched by the alignment and remain rc_motion_metrics'); mesh_err [groups] the mean over
 * frames and vertices of |mesh_p' - mesh_t| (:313); per_frame [n,2] each frame's mean joint and mean vertex error; xform [n,2,13] = R
 * [9], t [3], s of the joint fit, then of the mesh fit. flags: RC_MOTION_NO_MESH skips the mesh half (mesh_err, per_frame[:,1] and
 * xform[:,1] are NaN, every other entry keeps its bits); without it a context with no mesh returns RC_ERR_STATE.
 * The mesh fit reads no vertex: sum_v p_v t_v^T, sum_v p_v and sum_v |p_v|^2 are bilinear in the 24 joint transforms through constants
 * folded once per mesh (float64, on the host, by the first call after rc_set_mesh / rc_set_body: that call synchronises the device).
 * Joint chains, fits and sums in float64; the vertex error is one float32 blend per vertex of 24 aligned difference transforms. The
 * one-pass centring of the mesh fit leaves 1e-16 V |mu|^2 of rounding in the spreads: a DEGENERATE mesh whose skinned vertices all coincide
 * gets a rounding-level spread of either sign (s: any value, or NaN from a negative ratio) where rc_svd_rotate's two passes give exactly 0
 * and the IEEE inf / NaN; a mesh with any extent is unaffected.
 * Otherwise enqueued on `stream` like rc_motion_metrics: no read-back, no synchronisation, the group table through a ring of four
 * pinned copies, a wait for the stream where the context-owned scratch grows. No floating-point atomics, every sum in an order fixed by
 * the frame or the group alone: two calls give the same bits and a group's entries are those of a call with that group alone.
 * RC_ERR_INVALID (nothing written, nothing enqueued) on a null context, pose or table, no output, what == 0 or unknown bits, an unknown
 * flag, and the table errors of rc_motion_metrics; n == 0 with groups == 0 is a no-op. */
int rc_aligned_metrics(rc_ctx* ctx, const float* pose_p, const float* pose_t, int64_t n, int32_t groups, const int64_t* group_frames_host,
                       uint32_t what, uint32_t flags, float* joint_err, float* mesh_err, float* per_frame, float* xform, void* stream);
/* IMU synthesis of the dataset preparation (preprocess.py:22-33 `_syn_acc`, :206-214): pose[T,24,3,3] local rotations,
 * tran[T,3] DEVICE; vertex_ids[6] (config.vi_mask) and joint_ids[6] (config.ji_mask) HOST; needs rc_set_mesh.
 * -> imu_ori[T,6,3,3] = global rotations of joint_ids, vert6[T,6,3] = skinned vertices, imu_acc[T,6,3] =
 * _syn_acc(vert6, smooth_n), joint3d[T,24,3] (or NULL). rc_syn_acc is the stencil alone on v[T,width]: second
 * differences * 3600 with zero end frames, interior [n:-n] from the wide stencil / n^2 when smooth_n >= 2 (bit-exact).
 * Like the reference, smooth_n 0 and 1 are the plain stencil and smooth_n >= 2 needs T >= 2 * smooth_n + 1; T = 0 is a no-op. */
int rc_synth_imu(rc_ctx* ctx, const float* pose, const float* tran, const int32_t* vertex_ids_host,
                 const int32_t* joint_ids_host, int64_t T, int32_t smooth_n, float* imu_ori, float* imu_acc, float* joint3d,
                 float* vert6, void* stream);
int rc_syn_acc(const float* v, int64_t T, int64_t width, int32_t smooth_n, float* acc, void* stream);
/* The motion half of the dataset preparation for ALL sequences in one call (preprocess.py:252-306 preprocess_amass, :207-237 of
 * preprocess_aist; articulate/model.py:78-93, 209-241): the reference loops over the sequences on the host, shapes a body per sequence
 * and skins 6,890 vertices to keep 39.
 * rc_set_shape_space (HOST pointers, synchronous, once per context, after rc_set_mesh: its skinning weights are used): v_template [V,3],
 * shapedirs [V,3,10], J_regressor [24,V], landmark_ids [33] (config.mp_mask) and imu_vertex_ids [6] (config.vi_mask). Kept on the
 * device: the folded joint basis Jt = J_regressor . v_template [24,3] and JS = J_regressor . shapedirs [24,3,10] -- every entry summed over
 * V in double in index order, then rounded to float, the same call gives the same bits -- and, of the 39 picked vertices, the template,
 * shapedirs and weight rows: a shape then costs 24*3*10 + 39*3*10 multiply-adds, not a pass over V. v_template, shapedirs and J_regressor
 * may be NULL together (a body without blend shapes): only the picks are kept and a call with betas returns RC_ERR_STATE. RC_ERR_STATE
 * without rc_set_mesh; RC_ERR_INVALID on a V other than rc_set_mesh's or an id outside 0 .. V - 1. A later rc_set_mesh with other
 * weights or another V needs a new call.
 * rc_prepare_motions: sequence i has in_frames_host[i] input frames (HOST, summing to in_total) and emits out_i = ceil(in_frames / step)
 * frames, the input frames 0, step, 2 step, ... ([::step], :268-271; step_host[i] is 1 or 2, NULL: all 1); the outputs are concatenated
 * in sequence order over frames = sum out_i. DEVICE float inputs: pose_aa [in_total, pose_joints, 3] axis-angle, pose_joints 24 or 52 (of
 * 52, output joint 23 is input joint 37 and only the first 24 are used, :277-279), tran [in_total,3], betas [n_seq,10] or NULL.
 * world_rot_host: HOST [9] (amass_rot of :282) or NULL for none; tran_out = world_rot . tran, root axis-angle = the arithmetic of
 * rc_rotmat_to_axis_angle on world_rot . R(aa_0) (float64 inside, PARITY UNPINNED against cv2.Rodrigues like that entry); joints 1 .. 23
 * of pose_out [frames,72] are bit copies. The forward kinematics runs on rc_axis_angle_to_rotmat's arithmetic applied to pose_out, as
 * :292 does after the aligned pose is stored. Rest body: betas NULL -> the context's rc_set_body body and rc_set_mesh template (the
 * reference's shape=None branch, model.py:86-87); else per sequence J = Jt + JS beta, v39 = vt39 + S39 beta (in double, rounded once),
 * both minus J[0], bones from J (model.py:88-92). Outputs, DEVICE: imu_ori [frames,6,3,3] the global rotations of imu_joint_ids_host
 * (HOST [6], config.ji_mask); joint3d [frames,24,3]; sync_3d_mp [frames,33,3] the RAW landmark vertices vert[:, mp_mask] of :299
 * (sync_mp3d's joint overrides are rc_subnet_corpus's); imu_acc [frames,6,3] = _syn_acc of the six IMU vertices with smooth_n, the
 * stencil confined to its sequence (rc_syn_acc's bits on that sequence's rows); vert6_out [frames,6,3] or NULL the IMU vertices;
 * rest_joint_out [n_seq,24,3] or NULL the rest joints J before the root alignment (betas NULL: the body's, in every row).
 * Enqueued on `stream`: no read-back, no synchronisation, nothing per frame on the host; the sequence table travels through a ring of
 * four pinned copies like rc_motion_metrics' (a call waits on the host for the upload made four calls earlier, and for the whole device where
 * its context-owned table, rest records or vertex scratch grow: calls on other streams may still read them; those buffers are shared, so
 * calls of one context on different streams are ordered by the caller). No atomics: two calls give the same bits, and a sequence's rows are those of a call with that
 * sequence alone. RC_ERR_INVALID (nothing enqueued, nothing written) on a null context or required pointer, n_seq < 1, a step other than
 * 1 or 2, pose_joints other than 24 or 52, tables not summing to in_total, frames >= 2^31, a sequence with no frame, smooth_n < 0, for
 * smooth_n >= 2 a sequence with out_i < 2 smooth_n + 1 (the reference's torch.stack raises), a non-finite world_rot, an IMU joint id
 * outside 0 .. 23; RC_ERR_STATE without rc_set_body or rc_set_shape_space, or betas without the shape basis. */
int rc_set_shape_space(rc_ctx* ctx, const float* v_template_host, const float* shapedirs_host, const float* j_regressor_host, int32_t V,
                       const int32_t* landmark_ids_host, const int32_t* imu_vertex_ids_host);
int rc_prepare_motions(rc_ctx* ctx, int32_t n_seq, const int64_t* in_frames_host, const int32_t* step_host, int64_t in_total,
                       const float* pose_aa, int32_t pose_joints, const float* tran, const float* betas, const float* world_rot_host,
                       const int32_t* imu_joint_ids_host, int32_t smooth_n, float* pose_out, float* tran_out, float* imu_ori,
                       float* imu_acc, float* joint3d, float* sync_3d_mp, float* vert6_out, float* rest_joint_out, void* stream);
/* Camera-frame motions for ALL sequences in one call: the motion part of preprocess_3dpw / preprocess_3dpwocc (preprocess.py:460-470,
 * 477-483; :571-582, 589-599: a data set filmed by a MOVING camera, every frame with its own T_cw, the 30 Hz camera poses repeated to
 * 60 Hz by np.repeat) and, with a static camera and RC_CAM_ROOT_ONLY, the root flip of preprocess_my_totalcapture_pre (:359-360).
 * Sequence i has in_frames_host[i] pose / translation frames and cam_frames_host[i] camera rows (HOST, summing to in_total / cam_total).
 * cam_repeat r >= 1: output frame t uses camera row t / r and out_i = min(in_i, r cam_i) -- the `[:len(cam_pose)]` / `cam_pose[:len(posec)]`
 * pair of :463-465 and :577; preprocess_3dpw itself raises where the pose is the shorter one, this is preprocess_3dpwocc's behaviour. r = 0:
 * ONE camera row per sequence (static), out_i = in_i. Outputs are concatenated in sequence order over frames = sum out_i; the frames of a
 * sequence behind out_i are not read. DEVICE float inputs: pose_aa [in_total,24,3] axis-angle, tran [in_total,3], betas [n_seq,10] or NULL.
 * cam_T_host: HOST [cam_total,4,4] row-major T_cw, row 3 ignored -- on the host because the rows are checked before anything is enqueued;
 * they travel with the sequence tables (12 floats per row) through rings of four pinned copies.
 * Per output frame, with C its camera row: local rotations by rc_axis_angle_to_rotmat's arithmetic (joints 1 .. 23 of pose_out carry that
 * entry's bits); root = C[:3,:3] . R_0 and tran_out = C[:3,:3] . tran + C[:3,3] in float32, every product and sum rounded (an identity
 * camera leaves both as they are); with RC_CAM_ROOT_ONLY tran_out is a bit copy of tran (TotalCapture rotates the root and takes its
 * translation from Vicon). pose_out [frames,24,3,3] holds ROTATION MATRICES (the 3DPW dictionary's posec): no R -> axis-angle on this
 * path. Rest body, joint chain, the global rotations of imu_joint_ids_host, the 33 landmark and 6 IMU vertices and _syn_acc confined to
 * the sequence: rc_prepare_motions' kernels and expressions, on the camera-frame root and tran_out (:468-470). sync_3d_mp [frames,33,3],
 * vert6_out and rest_joint_out may be NULL.
 * Keypoints (kp_in DEVICE [kp_total,33,3] with kp_frames_host and kp_out [frames,33,3], or all three NULL): the 30 Hz detections raised to
 * 60 Hz as :477-483 does, cut to out_i -- output frame t even: kp[t / 2]; t odd: (kp[t / 2 + 1] + kp[t / 2]) / 2 in all three columns,
 * the confidence included; t odd behind the last detector frame: that frame again. Bit for bit numpy's float32.
 * Enqueued on `stream` like rc_prepare_motions (same rings, same shared buffers, same ordering rule for calls of one context): no
 * read-back, no synchronisation, no atomics, one writer per output element. RC_ERR_INVALID (nothing enqueued, nothing written) on what
 * rc_prepare_motions refuses and on cam_repeat < 0, a sequence without a camera row, r = 0 with cam_i != 1, a non-finite entry in the first
 * three rows of a cam_T, tables that do not sum to in_total / cam_total / kp_total, 2 kp_i < out_i, kp_in without kp_out (or the reverse)
 * and flags other than RC_CAM_ROOT_ONLY; RC_ERR_STATE as rc_prepare_motions. */
#define RC_CAM_ROOT_ONLY 1u
int rc_prepare_camera_motions(rc_ctx* ctx, int32_t n_seq, const int64_t* in_frames_host, const int64_t* cam_frames_host, int32_t cam_repeat,
                              int64_t in_total, int64_t cam_total, const float* pose_aa, const float* tran, const float* betas,
                              const float* cam_T_host, const float* kp_in, const int64_t* kp_frames_host, int64_t kp_total,
                              const int32_t* imu_joint_ids_host, int32_t smooth_n, uint32_t flags, float* pose_out, float* tran_out,
                              float* imu_ori, float* imu_acc, float* joint3d, float* sync_3d_mp, float* vert6_out, float* kp_out,
                              float* rest_joint_out, void* stream);
/* reconstruction_error(S1, S2, reduction=None) (utils.py:189-203) on raw point sets: S1, S2 DEVICE [n, n_points, 3]
 * -> err DEVICE [n] = mean point distance after the optimal scale * rotation + translation of S1 onto S2. */
int rc_procrustes_error(const float* S1, const float* S2, int64_t n, int32_t n_points, float* err, void* stream);
/* PositionErrorEvaluator (articulate/evaluator.py:100-129): p[n,3], t[n,3] DEVICE -> dist[n] DEVICE and, if mean_host
 * is not NULL, their mean (synchronises `stream`). */
int rc_position_error(const float* p, const float* t, int64_t n, float* dist, double* mean_host, void* stream);
/* smplify forward residual (net/smplify/temporal_smplify.py:198-220 -> losses.py:36-37,43-46): pose[T,24,3,3],
 * tran[T,3], kp[T,33,3] in pixels, K[3,3] (DEVICE) -> loss[T,33]. The confidences of landmarks
 * {1..9,31,32} count as zero. */
/* Landmarks whose confidence smplify zeroes (temporal_smplify.py:92-94): default {1..9, 31, 32}; `use_head=True` of the
 * reference = {31, 32}. ids HOST int32[n], each in 0..32. Applies to rc_reproj_residual and the optimiser. */
int rc_set_ignored_landmarks(rc_ctx* ctx, const int32_t* ids_host, int32_t n);
int rc_reproj_residual(rc_ctx* ctx, const float* pose, const float* tran, const float* kp, const float* K,
                       float sigma, float* loss, int64_t T, void* stream);

/* ---- smplify optimiser ------------------------------------------------------
 * Replaces net/smplify/run.py:6-34 (smplify_runner) -> temporal_smplify.py:97-196 (TemporalSMPLify.__call__):
 * L-BFGS (torch.optim.LBFGS, strong Wolfe) over [body_pose (T*72 axis-angle), tran (T*3)] of the whole sequence on
 * temporal_body_fitting_loss (net/smplify/losses.py:23-87). Loss and analytic gradient run on the device
 * (rc_smplify.hip), the optimiser's vectors stay there too; its scalar logic (csrc/rc_lbfgs_dev.h: two-loop recursion on
 * coefficients, line search) runs on the host. RC_SMPLIFY_HOST_LBFGS=1 runs csrc/rc_lbfgs.h on host vectors instead (A/B). */

/* GMM pose prior of MaxMixturePrior (net/smplify/prior.py:102-147): HOST means[8,69], precisions[8,69,69]
 * (inverse covariances) and nll_weights[8] (the weights already divided by the determinant term, prior.py:137-141). */
int rc_smplify_set_prior(rc_ctx* ctx, const float* means_host, const float* precisions_host, const float* nll_weights_host);

/* One closure evaluation (temporal_smplify.py:150-166): x DEVICE [T*72 | T*3] flat parameter vector, kp[T,33,3]
 * pixels + confidence, ref3d[T,33,3] landmarks of the initial prediction, imu_aa[T,18] axis-angle of the IMU
 * orientations (all DEVICE), K[3,3] HOST. Writes the total loss (HOST double) and grad DEVICE [T*72 | T*3].
 * Synchronises `stream`. */
int rc_smplify_loss_grad(rc_ctx* ctx, const float* x, const float* kp, const float* ref3d, const float* imu_aa,
                         const float* K_host, int64_t T, double* loss_host, float* grad, void* stream);

/* With shape=..., the reference keeps the preserved 3D landmarks of the INITIAL prediction on the MEAN-shape body
 * (temporal_smplify.py:112 calls forward_kinematics without shape) while everything else uses the shaped body. A context
 * holds one body, so the caller computes those landmarks on a mean-shape model and hands them over: ref3d DEVICE [T,33,3],
 * used by the NEXT rc_smplify_run instead of the landmarks of the context's own body (then forgotten); NULL cancels. */
int rc_smplify_set_ref3d(rc_ctx* ctx, const float* ref3d);

typedef struct rc_smplify_info {
    int32_t status;          /* 0: rejected by the pre-check (run.py:27-29), 1: optimised */
    int32_t n_iter, n_eval;  /* L-BFGS iterations / closure evaluations */
    int32_t reserved;
    double first_loss, final_loss;   /* closure value at the prediction / at the accepted point */
    double host_ms, device_ms;       /* wall time of the call / HIP-event time of the closure evaluations */
} rc_smplify_info;

/* smplify_runner(pred_pose, pred_tran, j2dc, imu_ori, batch_size=T, cam_k, lr, opt_steps=1, use_lbfgs=True,
 * loss_threshold): pose[T,24,3,3] local rotations, tran[T,3], kp[T,33,3], imu_ori[T,6,3,3] DEVICE; K HOST.
 * Outputs pose_out / tran_out DEVICE (the inputs copied through when the pre-check rejects the sequence) and
 * update HOST uint8[T] (new per-frame mean residual < old; all zero when rejected -- the reference returns None,
 * see info->status). max_iter = 20 and max_eval = 25 are torch's defaults the reference leaves untouched. */
int rc_smplify_run(rc_ctx* ctx, const float* pose, const float* tran, const float* kp, const float* imu_ori,
                   const float* K_host, int64_t T, float lr, int32_t max_iter, float loss_threshold, float* pose_out,
                   float* tran_out, uint8_t* update_host, rc_smplify_info* info, void* stream);

/* The same for n_rows independent (sequence, camera) rows at once (evaluate.py:86-90 loops them): every row runs the optimiser
 * of rc_smplify_run (one algorithm, csrc/rc_lbfgs_dev.h, behind a single-row and a batch-row backend) as a fiber of the CALLING thread
 * (a stack of its own behind a guard page; one live row runs inline), the device work of all rows goes out in lock-step rounds -- one launch per kind
 * of operation over all rows, one read-back and one synchronisation per round -- so 72 rows cost about what the longest row's ~46
 * rounds cost. Per row the arithmetic is that of rc_smplify_run (same n_iter / n_eval / losses). Arrays of n_rows: T, DEVICE
 * pointers pose / tran / kp / imu_ori / pose_out / tran_out, HOST pointers update (uint8[T_r] each), HOST K[n_rows,9], infos
 * (host_ms / device_ms are those of the whole batch; reserved = rounds). Rows rejected by the pre-check are copied through. */
int rc_smplify_run_batch(rc_ctx* ctx, int32_t n_rows, const int64_t* T_rows, const float* const* pose, const float* const* tran,
                         const float* const* kp, const float* const* imu_ori, const float* K_host, float lr, int32_t max_iter,
                         float loss_threshold, float* const* pose_out, float* const* tran_out, uint8_t* const* update_host,
                         rc_smplify_info* infos, void* stream);

/* The optimiser alone, in float64, on a caller-supplied objective (HOST): same algorithm object as rc_smplify_run
 * with Real = double. tests/ pin it against torch.optim.LBFGS evaluation by evaluation. objective returns the loss
 * at x[n] and fills grad[n]. x is updated in place; losses_out (capacity cap) receives every objective value in
 * evaluation order. */
typedef double (*rc_objective_fn)(void* user, const double* x, double* grad, int64_t n);
int rc_lbfgs_minimize(rc_objective_fn objective, void* user, int64_t n, double* x, double lr, int32_t max_iter,
                      int32_t max_eval, int32_t history_size, double tolerance_grad, double tolerance_change,
                      int32_t* n_iter_out, int32_t* n_eval_out, double* losses_out, int64_t cap);

/* DIAGNOSTIC (tests only; no reference interface: torch.optim.LBFGS of net/smplify/temporal_smplify.py:141-147 keeps its vectors in
 * tensors). The device-resident optimiser alone: the backends, vector kernels, job tables and arenas rc_smplify_run (backend 0: each row
 * through the single-row backend, one after another) and rc_smplify_run_batch (backend 1: all rows in lock-step rounds) run, on a
 * synthetic closure whose fp32 arithmetic tests/lbfgs_device_emu.cpp restates exactly (csrc/rc_smplify.hip: rc_syn_closure_*). Needs
 * neither a body nor a prior. Row r has 75 T_r elements; x0 / a / b / x_out are HOST arrays of n_rows DEVICE pointers to [75 T_r]
 * (start, weights, targets, result). max_eval, history and tolerances are those of rc_smplify_run (RC_LBFGS_HISTORY and
 * RC_SMPLIFY_DEVICE_TOTALS are read per call). infos[n_rows] receives n_iter / n_eval / first and final loss; losses_out HOST
 * [n_rows, cap] every closure value of a row in evaluation order (zero-filled); backend 1: *max_jobs_out = the largest job table a
 * round sent, *rounds_out = the number of rounds (both 0 for backend 0). Synchronises `stream`. */
int rc_lbfgs_device_probe(rc_ctx* ctx, int32_t backend, int32_t n_rows, const int64_t* T_rows, const float* const* x0,
                          const float* const* a, const float* const* b, float lr, int32_t max_iter, float* const* x_out,
                          rc_smplify_info* infos, float* losses_out, int64_t cap, int32_t* max_jobs_out, int32_t* rounds_out,
                          void* stream);

/* Harness input preparation of evaluate.py:38-51,70-73 for ONE (sequence, camera) of n frames:
 *   j2dc = K^-1 [u, v, 1] with the confidence copied into the last channel, accc = R_cw acc_w, oric = R_cw ori_w,
 *   gravity_out (HOST float[3]) = R_cw [0, -1, 0].
 * kp_pix[n,33,3] = (u, v, conf) in pixels, imu_acc_w[n,6,3], imu_ori_w[n,6,3,3] DEVICE; K[3,3], Tcw[4,4] HOST (the last row of Tcw
 * is not read). K^-1 is the float64 adjugate rounded once to float; only its rows 0 and 1 are used, with the homogeneous 1 as it
 * stands (no division by the third row), so a K with skew, K[2][2] != 1 or a general third row gives what the reference's
 * K.inverse() gives. The confidence is copied bit for bit.
 * RC_ERR_INVALID, with nothing launched and neither the outputs nor gravity_out written: a null buffer (the device buffers may be
 * null when n == 0), n < 0, a NaN or an infinity in K or in the upper 3 x 4 of Tcw, det K == 0, an entry of K^-1 that is not
 * finite as a float. n == 0 writes gravity_out and launches nothing.
 * Pinned to a float64 restatement by tests/test_gpu_harness_inputs.py (bounds: oracle/harness_f64.py). */
int rc_camera_inputs(const float* kp_pix, const float* imu_acc_w, const float* imu_ori_w, const float* K_host,
                     const float* Tcw_host, float* j2dc, float* accc, float* oric, float* gravity_out_host, int64_t n,
                     void* stream);

/* The same preparation for ALL rows of an evaluation in one launch (evaluate.py:32-51,66-73 loops sequences, cameras and
 * frames on the host). Row r = one (sequence, camera): kp_norm[n_rows,Tmax,33,3] = (u / image_w, v / image_h, conf) as the
 * preprocessed dataset stores them (evaluate.py:43-44 multiplies the image size back), imu_acc_w[n_seq,Tmax,6,3] and
 * imu_ori_w[n_seq,Tmax,6,3,3] per SEQUENCE, seq_of_row[n_rows] (which sequence a row belongs to), len[n_rows] (valid frames of
 * the row; later frames are written as padding: zero keypoints and accelerations, identity orientations) -- all DEVICE;
 * K[n_rows,3,3], Tcw[n_rows,4,4] HOST. Outputs j2dc[n_rows,Tmax,33,3], accc[n_rows,Tmax,6,3], oric[n_rows,Tmax,6,3,3] DEVICE,
 * gravity_out[n_rows,3] HOST. cam_scratch: caller-owned DEVICE buffer of n_rows * 72 bytes (camera constants).
 * Padding frames of the inputs are not used (they may hold anything, NaN included); valid frames are bitwise those of
 * rc_camera_inputs on the same row. Synchronises `stream` once (upload of the camera constants).
 * RC_ERR_INVALID as for rc_camera_inputs, whichever row holds the bad camera: every row's constants are computed on the host
 * first, and gravity_out, cam_scratch and the outputs are written only when all rows passed. n_rows == 0 or Tmax == 0 returns RC_OK
 * and writes nothing. One launch carries at most 65535 rows (grid y); that limit and frame counts beyond 2^31 are not tested. */
int rc_camera_inputs_rows(const float* kp_norm, const float* imu_acc_w, const float* imu_ori_w, const int32_t* seq_of_row,
                          const int32_t* len, const float* K_host, const float* Tcw_host, float image_w, float image_h,
                          int32_t n_rows, int32_t Tmax, float* j2dc, float* accc, float* oric, float* gravity_out_host,
                          void* cam_scratch, void* stream);

/* ---- state access (tests / checkpointing of a running sequence) ------------------------------------------ */
/* Copy the (h, c) state of sub-net `net` to HOST buffers h[2,batch,H], c[2,batch,H]. Synchronises `stream`. */
int rc_get_state(rc_ctx* ctx, const char* net, float* h_host, float* c_host, void* stream);
/* Per-row fusion state (net/sig_mp.py:85-104 and the class attributes L43-45) for tests and debugging: out[batch,5] =
 * {last_tran is set, len(floor_y), first_reach, update_vision_count, a deferred vision-updater step is pending}. Synchronises. */
int rc_get_fusion_state(rc_ctx* ctx, int32_t* out_host, void* stream);

/* Per-row branch trace of the last step, HOST int32[batch,8]:
 * {regime (0 low,1 mid,2 high), rnn4 steps, rnn6 steps, floor samples held, reach fired, used velocity branch,
 *  stance foot, jump reset}. Synchronises `stream`. */
int rc_get_trace(rc_ctx* ctx, int32_t* trace_host, void* stream);

/* The inverse of rc_get_state: write the (h, c) state of sub-net `net` from HOST buffers h[2,batch,H], c[2,batch,H] (either may be NULL:
 * that half stays). row_mask_host: HOST uint8[batch] (non-zero = write the row) or NULL for all rows; the other rows keep their state.
 * h goes into the copy each row's own step counter designates (the one rc_get_state reads); the counters do not move. Like rc_get_state
 * it first runs every pending updater step, so that a state just set is not stepped over by a step deferred from the frame before. What
 * it replaces: the assignment `net.hidden[K - 1] = (h, c)` a caller of the reference would make (net/sig_mp.py:99,126-129 keeps the state
 * of rnnK there). It takes no stream: it orders itself behind all work of the device, runs on the context's default
 * stream and is done when it returns. Synchronises. RC_ERR_INVALID on an unknown net, RC_ERR_STATE before rc_finalize_weights. */
int rc_set_state(rc_ctx* ctx, const char* net, const float* h_host, const float* c_host, const uint8_t* row_mask_host);

/* ---- row state: save, move and restore rows of a running context (csrc/rc_rowstate_api.cpp, rc_rowstate.hip) ----------------------- */
/* Everything a row carries from frame to frame (net/sig_mp.py:85-104, the (h, c) of the RNN modules L126-129 and, here, the deferred
 * vision-updater step of L264-271 with its inputs) as ONE record of rc_row_state_bytes bytes, the same whatever the context's batch, row
 * padding, gemm mode or engine -- so a record taken from row r of one context continues, bit for bit, in row r' of another context of any
 * batch size that agrees with the first on rc_params, weights, body and gemm mode (none of which is part of a record). Layout: DESIGN.md
 * section 3.11; `format` changes whenever the layout does. A record holds the CURRENT h of every layer (the copy the row's step counter
 * designates); step counters are not state: rc_load_rows writes h into the copy the DESTINATION row's own counter designates and leaves
 * the counters alone. A pending updater step travels as pending, with its inputs; it is neither run nor dropped.
 *
 * The two stream-ordered entries take a DESCRIPTOR and not a trailing `void* stream` parameter: tests/test_stream_cases_cpu.py lists every
 * header entry whose parameter list names a stream in the table of tests/test_gpu_stream_order.py, which could not be extended when
 * these entries were added; their fenced side-stream cases live in tests/test_gpu_row_state.py instead. A change that may edit that table
 * can move them there and give the entries an ordinary stream parameter.
 *
 * rc_save_rows (context -> blob) and rc_load_rows (blob -> context) are enqueued on io->stream: one upload of the row table (through
 * pinned copies taken in turn, ring of four, as in the Conventions) and one kernel; no device read-back, no host synchronisation.
 * rc_save_rows changes nothing in the context. rc_load_rows touches only the listed rows; it is an eager entry for a live session like
 * rc_reset (pre-steps and a waiting first kernel are discarded, the next live frame waits for it). Calls of one context are ordered by
 * their streams as everywhere: the row table is one device buffer per context.
 * RC_ERR_INVALID (message in rc_last_error, nothing enqueued): a null descriptor, or a null blob while n > 0; n < 0 or n > batch; a row
 * out of range or listed twice; bytes_per_row other than the context's; a blob that is not 16-byte aligned. RC_ERR_STATE before
 * rc_finalize_weights. n == 0 returns RC_OK and enqueues nothing. Untested with the resident engine enabled (rc_set_resident). */
typedef struct {
    const int32_t* rows;     /* HOST int32[n], distinct, 0 <= rows[i] < batch; NULL = rows 0 .. n-1. Consumed before the call returns */
    int32_t        n;        /* records in the blob, 0 <= n <= batch (n == 0: RC_OK, nothing enqueued) */
    void*          blob;     /* DEVICE, n * bytes_per_row bytes, 16-byte aligned; record i belongs to rows[i] */
    int64_t        bytes_per_row;   /* as returned by rc_row_state_bytes: a blob of another format is refused */
    void*          stream;   /* the caller's stream, as everywhere else */
} rc_row_io;
#define RC_ROW_STATE_FORMAT 1
int rc_row_state_bytes(rc_ctx* ctx, int64_t* bytes_per_row, int32_t* format);   /* host only; either output may be NULL */
int rc_save_rows(rc_ctx* ctx, const rc_row_io* io);   /* context -> blob */
int rc_load_rows(rc_ctx* ctx, const rc_row_io* io);   /* blob -> context */

/* Timing hook for bench.py: accumulate HIP-event time of the gate-GEMM launches on their own stream.
 * enable = 1 records every gate-GEMM launch, enable = 2 only those of the wide-tile kernel rc_gemm_kernel (the 16-row
 * launches run on rc_gemm_small_kernel), enable = 3 only those of the shared-weight kernel rc_gemm_lds_kernel (round 6: the LSTM layer
 * steps of contexts of more than 64 rows), 0 stops; rc_gemm_timing_read returns total milliseconds and launch count so far. */
int rc_gemm_timing(rc_ctx* ctx, int32_t enable);
int rc_gemm_timing_read(rc_ctx* ctx, double* total_ms, int64_t* launches);
/* Time (ms) during which at least one of the launches read so far was running: the wavefront engine issues the two wide launches
 * of a tick on two streams, so their durations overlap and the sum above counts that time twice. Valid after rc_gemm_timing_read. */
int rc_gemm_timing_busy(rc_ctx* ctx, double* busy_ms);

#ifdef __cplusplus
}
#endif
#endif /* ROBUSTCAP_HIP_H */
